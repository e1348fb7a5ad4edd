"""readers for the committed mapping fixtures (tests/golden/lr/*, tests/golden/sr/*; inputs made by tools/synth.py /
tools/synth_sr_var.py, golden SAM by the reference binaries oracle/_ref/gdiet_{lr,sr}_avx with the command in *.cmd)"""
import gzip
import hashlib
import json
import os

LR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lr")
SR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sr")
REP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rep")
OPTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "opts")
# kind -> (directory, read set / golden stem, Mapper preset)
# "hifi_w1": the first 8 reads of hifi.fq with -k 15 -w 1 (every sparsified base is a minimizer: the per-read scratch of the
# seeding kernel overflows its first estimate and the batch is retried with the hard bound)
# "*_edge": reads shorter than k / k+w, all-N, poly-A, lower case, IUPAC codes, chimeras, duplications, lengths around the 300 bp
# switches of both variants, indels, reads flush with a contig start (golden: tools of the reference on these very files)
# "hifi_sv" / "ont_sv": reads with one structural difference each (deletion, insertion, chimera, tandem duplication, inversion;
# tools/synth.py --kind *_sv): second voting round, linked candidates, concatenate_cigars, supplementary and secondary records
# "*_rep": the repeat-rich reference of tools/synth_rep.py (tests/golden/rep/ref.fa.gz: dispersed families, tandem satellites with
# keys above mid_occ and above max_max_occ = 4095, microsatellites) and reads drawn across and inside the repeats: the drop branch of
# mm_seed_mz_flt, mm_seed_select's rescue heap, the max_max_occ cut, multi-occurrence position lists in the index and strands with
# far more than 4096 hits all fire (oracle/make_golden.py prints the counts; tests/test_map_host.py asserts them)
# "hifi_n" / "sr_n": the first 12 reads of hifi.fq / 200 reads of sr.fq with 1 to 3 bases each replaced by N (tools/synth_n.py): Ns inside
# alignments, which the DP scores as -e2 -- the option grid maps them at e2 = 2
# "sr_rep_f60": the sr_rep reads with -f 60 (mid_occ = 60): at the preset's mid_occ = 1000 the query-side filter cannot fire in the
# ShortReads variant, whose mm_sketch3 stops at 800 minimizers (SR/map.c:621-622)
SETS = {"hifi_rep": (REP, "hifi_rep", "hifi"), "ont_rep": (REP, "ont_rep", "ont"), "sr_rep": (REP, "sr_rep", "sr"), "sr_rep_f60": (REP, "sr_rep_f60", "sr"),
        "hifi_sv": (LR, "hifi_sv", "hifi"), "ont_sv": (LR, "ont_sv", "ont"), "hifi_edge": (LR, "edge_hifi", "hifi"), "ont_edge": (LR, "edge_ont", "ont"), "sr_edge": (SR, "edge", "sr"),
        "hifi_w1": (LR, "w1", "hifi"), "hifi": (LR, "hifi", "hifi"), "ont": (LR, "ont", "ont"), "sr": (SR, "sr", "sr"), "sr_var": (SR, "var", "sr"),
        "hifi_n": (LR, "hifi_n", "hifi"), "sr_n": (SR, "sr_n", "sr")}
# options of var.cmd that differ from the sr preset (README command): -N 5 -n 0.3,0.1 -s 40 --AF_max_loc 20
OVERRIDES = {"hifi_w1": dict(k=15, w=1), "ont_sv": dict(min_dp_max=4000),  # ont_sv.cmd: -s 4000 (reads of ~14 kbp)
             "ont_rep": dict(min_dp_max=4000), "sr_rep_f60": dict(mid_occ=60),
             "sr_var": dict(best_n=5, min_cnt=0.3, rec_threshold_frac=0.1, min_dp_max=40, AF_max_loc=20)}


# kinds whose --print-seeds stage trace is committed next to the golden SAM (<stem>.trace.gz, oracle/make_golden.py), reduced
# to the lines that start with one of TRACE_PREFIXES
TRACED = ("hifi", "ont", "hifi_sv", "ont_sv", "sr", "hifi_rep", "ont_rep", "sr_rep")
TRACE_PREFIXES = ("Final shift", "RS ", "SD\t", "VT\t", "AVT\t", "BE\t", "AL_SCORE", "CONQ", "CONT")
# kinds whose committed trace holds, per read, ONE line "SDX\t<number of SD lines>\t<sha1 of the sorted SD lines>" in place of the SD
# lines themselves (a read of the repeat-rich sets has up to 280 000 seed hits on a strand: millions of lines per set)
SD_DIGESTED = ("hifi_rep", "ont_rep", "sr_rep")


def variant_of(kind):
    """which of the reference's two trees maps this kind: "sr" = GDiet-ShortReads, "lr" = GDiet-LongReads"""
    return "sr" if SETS[kind][2] == "sr" else "lr"


def digest_sd(lines):
    """the trace lines of a run with every read's SD lines replaced by their count and digest (see SD_DIGESTED)"""
    out, sd = [], []

    def flush():
        if sd:
            out.append("SDX\t%d\t%s" % (len(sd), hashlib.sha1("\n".join(sorted(sd)).encode()).hexdigest()))
            del sd[:]
    for line in lines:
        if line.startswith("SD\t"):
            sd.append(line)
        else:
            flush()
            out.append(line)
    flush()
    return out


# kinds with a committed PAF golden as well (<stem>.golden.paf.gz: the same command with -x instead of -ax, no -a, plus -c
# --paf-no-hit: mm_write_paf3 with the cg:Z: tag and the unmapped lines)
PAF_KINDS = ("hifi_sv", "sr")


def paf_cmd_of(kind):
    out = []
    for tok in cmd_of(kind):
        if tok == "-a":
            continue
        out.append("-x" if tok == "-ax" else tok)
    return out + ["-c", "--paf-no-hit"]


def golden_paf(kind):
    d, stem, _ = SETS[kind]
    return [l.rstrip("\n") for l in gzip.open(os.path.join(d, stem + ".golden.paf.gz"), "rt")]


def read_fasta(path):
    names, seqs, cur = [], [], []
    op = gzip.open if path.endswith(".gz") else open
    for line in op(path, "rt"):
        line = line.rstrip()
        if line.startswith(">"):
            if names:
                seqs.append("".join(cur))
            names.append(line[1:].split()[0])
            cur = []
        else:
            cur.append(line)
    seqs.append("".join(cur))
    return names, seqs


def read_fastq(path):
    op = gzip.open if path.endswith(".gz") else open
    lines = [l.rstrip() for l in op(path, "rt")]
    return [(lines[i][1:].split()[0], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def golden_sam(kind):
    d, stem, _ = SETS[kind]
    return [l.rstrip("\n") for l in gzip.open(os.path.join(d, stem + ".golden.sam.gz"), "rt")]


def trace_of(kind):
    d, stem, _ = SETS[kind]
    return [l.rstrip("\n") for l in gzip.open(os.path.join(d, stem + ".trace.gz"), "rt")]


def reads_of(kind):
    """the read set a golden SAM was made from"""
    d, stem, _ = SETS[kind]
    if kind == "sr_rep_f60":
        return read_fastq(os.path.join(d, "sr_rep.fq.gz"))
    if kind == "hifi_w1":
        return read_fastq(os.path.join(d, "hifi.fq.gz"))[:8]
    if kind.endswith("_edge"):
        return read_fastq(os.path.join(d, "edge.fq.gz"))
    return read_fastq(os.path.join(d, stem + ".fq.gz"))


def cmd_of(kind):
    d, stem, _ = SETS[kind]
    name = {"hifi_edge": "hifi", "ont_edge": "ont", "sr_edge": "sr", "hifi_n": "hifi", "sr_n": "sr"}.get(kind, stem)
    return open(os.path.join(d, name + ".cmd")).read().split()


# ---- the option grid (tests/golden/opts/grid.json): the mapping path away from the README command lines -----------------------------
# A row = a kind of SETS above (its reference, read file, .cmd and Mapper preset / OVERRIDES), n_reads reads of that file from
# first_read on, command-line options appended to the .cmd ("extra") and the same options as Mapper overrides.  The three
# reverse-strand reads over the reference's N run (hifi_27 / hifi_sv_61 / ont_sv_3) are left out: their ms:i tag is an out-of-bounds
# read in the reference (test_map_host.py::_norm_ms) and may change from run to run.
# "build": which of the reference's two builds printed the row's goldens ("avx" = GDiet_avx; "scalar" = GDiet, only at window sizes
# where the two disagree: DESIGN.md).
# "min_mapped": the share of the reads the reference itself must map (a row must not pass on unmapped reads alone).
# "sensitive": the option groups of "extra"; the reference prints something else when any one of them is left out (asserted by the
# writer, and by test_map_host.py with the host path), so no option of a row rides along without effect.
# "tags" select rows: "kw" (pattern / k / w rows: both seed executors, host- and device-built index), "boxes", "post", "mmi" (index
# file digest in opts/mmi.sha256.json), "strand" (--for-only / --rev-only: mapped and unmapped reads), "mz_flt" (the query-side
# minimizer filter must fire), "retry" (more minimizers per read than the GPU path's first scratch estimate), "sv" (reads with a
# structural difference: second voting round, links), "vote_cap" / "vote_min" (reads of the repeat-rich reference with more vote
# candidates than any preset keeps / than vt_nb_loc = 1 keeps).
# oracle/make_grid_golden.py writes, per row, <name>.golden.sam.gz (SEQ and QUAL printed as "*": echoes of the input, pinned by the
# full goldens of SETS) and <name>.trace.gz (the --print-seeds trace reduced as for TRACED kinds, SD lines always digested).
PRESET_PATTERN = {"hifi": (19, 19), "ont": (15, 10), "sr": (21, 11)}  # (k, w) of the .cmd files a row builds on


def grid_rows(tag=None):
    rows = json.load(open(os.path.join(OPTS, "grid.json")))["rows"]
    return [r for r in rows if tag is None or tag in r["tags"]]


def grid_ids(tag=None):
    return [r["name"] for r in grid_rows(tag)]


def grid_row(name):
    return next(r for r in grid_rows() if r["name"] == name)


def grid_reads(row):
    return reads_of(row["kind"])[row["first_read"]:row["first_read"] + row["n_reads"]]


def grid_cmd(row, without=None):
    """the row's command line; without: one of the row's option groups (row["sensitive"]) left out"""
    extra = row["extra"]
    if without is not None:
        assert without in row["sensitive"] and extra.count(without) == 1
        extra = extra.replace(without, "")
    return cmd_of(row["kind"]) + extra.split()


def grid_mapper_args(row):
    """(directory of ref.fa.gz, Mapper preset, Mapper overrides) of a row"""
    d, _, preset = SETS[row["kind"]]
    ov = dict(OVERRIDES.get(row["kind"], {}))
    ov.update(row["overrides"])
    return d, preset, ov


def star_seq_qual(line):
    """a SAM line with SEQ and QUAL replaced by "*" (the form of the grid's goldens)"""
    f = line.split("\t")
    if len(f) > 10:
        f[9] = f[10] = "*"
    return "\t".join(f)


def grid_golden_sam(row):
    return [l.rstrip("\n") for l in gzip.open(os.path.join(OPTS, row["name"] + ".golden.sam.gz"), "rt")]


def grid_trace(row):
    return [l.rstrip("\n") for l in gzip.open(os.path.join(OPTS, row["name"] + ".trace.gz"), "rt")]


def mapped_share(sam_lines):
    """(reads with at least one mapped record, reads) of a SAM body"""
    names, mapped = set(), set()
    for l in sam_lines:
        f = l.split("\t")
        names.add(f[0])
        if f[2] != "*":
            mapped.add(f[0])
    return len(mapped), len(names)


# ---- the scoring rows of the grid (tag "score"): what each must hold to test its point --------------------------------------------
# tags of a "score" row: "wave" / "generic" (whether the register-resident DP kernels take the row's scoring: gdo.wave_scoring_ok -- a
# refused scoring sends every box of the mapping batch to the generic kernel), "single" (q == q2, e == e2), "prefilter" (short reads at
# a scoring whose widened pre-filter answers m <= 1 mismatches instead of the presets' m <= 3), "n_e2" (Ns inside alignments at e2 = 2)
def grid_scoring(row):
    """(a, b, q, e, q2, e2) a row maps with: its preset's scoring with the row's overrides"""
    import gdo
    s = dict(zip(("a", "b", "q", "e", "q2", "e2"), gdo.PRESETS[SETS[row["kind"]][2]]))
    s.update({k: v for k, v in row["overrides"].items() if k in s})
    return tuple(s[k] for k in ("a", "b", "q", "e", "q2", "e2"))


def grid_wave_scoring_ok(row):
    import gdo
    return gdo.wave_scoring_ok(*grid_scoring(row))


def prefilter_split(row, sam_lines):
    """the mapped records of a SAM body whose CIGAR is one M run and whose NM:i: is m > 0, counted by the side of the widened pre-filter's
    bound they fall on: (m (a + b) <= a + 2 (q + e): answered without the DP, above it: through the DP)"""
    import re
    a, b, q, e, _, _ = grid_scoring(row)
    lo = hi = 0
    for l in sam_lines:
        f = l.split("\t")
        nm = [int(x[5:]) for x in f[11:] if x.startswith("NM:i:")]
        if f[2] == "*" or not re.fullmatch(r"\d+M", f[5]) or not nm or nm[0] <= 0:
            continue
        if nm[0] * (a + b) <= a + 2 * (q + e):
            lo += 1
        else:
            hi += 1
    return lo, hi


def records_with_n_inside(row, sam_lines):
    """mapped records with at least one non-ACGT base of SEQ (the row's reads: the goldens star SEQ) inside the aligned query span, as
    read from the CIGAR's clips"""
    import re
    reads = {r[0]: r[1] for r in grid_reads(row)}
    comp = str.maketrans("ACGTacgt", "TGCAtgca")
    n = 0
    for l in sam_lines:
        f = l.split("\t")
        if f[2] == "*":
            continue
        seq = reads[f[0]]
        if int(f[1]) & 16:
            seq = seq.translate(comp)[::-1]
        left, right = re.match(r"(\d+)[SH]", f[5]), re.search(r"(\d+)[SH]$", f[5])
        span = seq[int(left.group(1)) if left else 0:len(seq) - (int(right.group(1)) if right else 0)]
        n += re.search(r"[^ACGTacgt]", span) is not None
    return n


def assert_score_row_conditions(row, sam_lines):
    """what a "score" row of the grid must hold, from the reference's own SAM: its wave / generic tag is what gdo.wave_scoring_ok says of
    its scoring; a "prefilter" row has at least 10 single-M records on either side of the pre-filter's bound; an "n_e2" row maps with
    e2 = 2 and has at least 3 records with an N inside the alignment"""
    tags = row["tags"]
    assert ("wave" in tags) != ("generic" in tags) and ("wave" in tags) == grid_wave_scoring_ok(row), row["name"]
    a, b, q, e, q2, e2 = grid_scoring(row)
    assert ("single" in tags) == (q == q2 and e == e2), row["name"]
    if "prefilter" in tags:
        lo, hi = prefilter_split(row, sam_lines)
        assert row["variant"] == "sr" and a + b > (a + 2 * (q + e)) // 2, row["name"]  # m = 2 is past the bound already
        assert lo >= 10 and hi >= 10, (row["name"], lo, hi)
    if "n_e2" in tags:
        n = records_with_n_inside(row, sam_lines)
        assert e2 == 2 and n >= 3, (row["name"], n)


# ---- B4: the output of gdiet_hip_seed_batch against a --print-seeds trace ---------------------------------------------------------
def seed_trace_per_read(lines):
    """per read of a trace: its "Final shift" line, its "RS" line and its SD / SDX lines, sorted"""
    out, cur = [], None
    for l in lines:
        if l.startswith("Final shift"):
            cur = {"shift": l, "RS": None, "SD": []}
            out.append(cur)
        elif cur is not None and l.startswith("RS "):
            cur["RS"] = l
        elif cur is not None and l.startswith(("SD\t", "SDX\t")):
            cur["SD"].append(l)
    for r in out:
        r["SD"].sort()
    return out


def assert_seed_batch_matches_trace(got, want, names, digested, flag=0):
    """got: Mapper.seed_batch's list; want: seed_trace_per_read of the reference's trace; names: the reference's contig names.  Every
    kept seed's occurrences are expanded as collect_seed_hits does (LR/map.c:861-955) and compared with the read's pattern phase, hit
    counts and SD lines (as a multiset; digested: as their count and sha1).  flag: the MM_F_* bits of the mapping options -- the seed level
    hands back every occurrence; with --for-only / --rev-only collect_seed_hits drops those of the other strand (skip_seed,
    LR/map.c:724-730), so the expansion here does too.  Returns the number of seed hits compared."""
    assert len(got) == len(want)
    n_sd = 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert "Final shift: %d" % g["shift"] == w["shift"], (i, g["shift"], w["shift"])
        lines, nf, nr = [], 0, 0
        at = 0
        for n_occ, q_pos in g["seeds"]:
            qpos, qstrand = int(q_pos) >> 1, int(q_pos) & 1
            for y in g["occ"][at:at + int(n_occ)]:
                y = int(y)
                rid, loc, strand = y >> 32, (y & 0xffffffff) >> 1, y & 1
                if flag & (0x200000 if strand == qstrand else 0x100000):  # MM_F_REV_ONLY drops same-strand hits, MM_F_FOR_ONLY the others
                    continue
                if strand ^ qstrand:  # reverse: target = loc + qpos, printed as (uint32)target + 1   (LR/map.c:897-903, :1335)
                    lines.append("SD\t%s\t%d\t-\t%d" % (names[rid], ((loc + qpos) & 0xffffffff) + 1, qpos))
                    nr += 1
                else:  # forward: target = loc + tmp_extracted_len - qpos, printed as (int32)target + 1 - tmp_extracted_len   (:904-910, :1331)
                    t = (loc + g["tel"] - qpos) & 0xffffffff
                    t = t - (1 << 32) if t >= 1 << 31 else t
                    lines.append("SD\t%s\t%d\t+\t%d" % (names[rid], t + 1 - g["tel"], qpos))
                    nf += 1
            at += int(n_occ)
        assert at == len(g["occ"])
        assert "RS n_a_for: %d, n_a_rev: %d" % (nf, nr) == w["RS"], (i, nf, nr, w["RS"])
        mine = sorted(digest_sd(lines) if digested else lines)
        assert mine == w["SD"], (i, mine[:2], w["SD"][:2])
        n_sd += nf + nr
    return n_sd


def flat_index(pkg, names, seqs, preset, overrides, builder, monkeypatch):
    """(keys, counts, positions in key order, S, mid_occ, n_keys) of the index a fresh context builds with GDIET_INDEX_BUILD=builder
    ("host" / "device": chosen when the context is created)"""
    import numpy as np
    monkeypatch.setenv("GDIET_INDEX_BUILD", builder)
    ctx = pkg.Context(0)
    try:
        m = pkg.Mapper(ctx, names, seqs, preset=preset, **overrides)
        try:
            f = m.export_index()
            order = np.argsort(f["keys"], kind="stable")
            start = np.concatenate([[0], np.cumsum(f["cnt"].astype(np.int64))])
            pos = np.concatenate([f["pos"][start[j]:start[j + 1]] for j in order]) if len(order) else f["pos"]
            return f["keys"][order], f["cnt"][order], pos, f["S"], m.mid_occ, m.n_keys()
        finally:
            m.close()
    finally:
        ctx.close()

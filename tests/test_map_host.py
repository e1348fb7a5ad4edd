"""CPU: the product's seeding/voting stage code (map_stages.h, compiled for the host) + host geometry and CIGAR
post-processing (map_host.h), with the oracle's ksw_extd2 standing in for the HIP kernel, reproduce the reference's
SAM byte for byte: against the committed golden SAM, and -- where oracle/_ref has been built -- against a fresh run of
the reference binary on a new random read set."""
import gzip
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from fixture_io import (LR, PAF_KINDS, REP, SD_DIGESTED, SETS, SR, TRACE_PREFIXES, assert_score_row_conditions, cmd_of, digest_sd, golden_paf, golden_sam, grid_cmd, grid_golden_sam, grid_ids,
                        grid_reads, grid_row, grid_rows, grid_trace, mapped_share, paf_cmd_of, reads_of, star_seq_qual, trace_of)


@pytest.fixture(scope="module")
def host_driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("maphost")
    exe = str(d / "map_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-w", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"),
                           "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "emul", "map_host_main.cpp"),
                           "-x", "c", os.path.join(ROOT, "oracle", "gdo_ksw2.c"), "-o", exe])
    for sub, base, files in (("lr", LR, ("ref.fa", "hifi.fq", "ont.fq")), ("sr", SR, ("ref.fa", "sr.fq", "var.fq")), ("rep", REP, ("ref.fa",))):
        os.makedirs(str(d / sub))
        for f in files:
            with gzip.open(os.path.join(base, f + ".gz"), "rb") as src, open(str(d / sub / f), "wb") as dst:
                shutil.copyfileobj(src, dst)
    return exe, str(d)


THREADS = ["-t", str(min(8, os.cpu_count() or 1))]
REP_KINDS = ("hifi_rep", "ont_rep", "sr_rep", "sr_rep_f60")
_rep_cache = {}


def _rep_run(host_driver, kind, tmp_path):
    """(SAM lines, stderr) of ONE run of the host driver on a repeat-rich set, with --print-seeds --stats: the golden-SAM, stage-trace
    and branch-count tests of these sets share it (a run is 10-15 s: the oracle's scalar DP on reads with tens of thousands of seed hits)"""
    if kind not in _rep_cache:
        exe, d = host_driver
        fq = str(tmp_path / "reads.fq")
        with open(fq, "w") as f:
            for name, seq, qual in reads_of(kind):
                f.write("@%s\n%s\n+\n%s\n" % (name, seq, qual))
        out = subprocess.run([exe] + THREADS + cmd_of(kind) + ["--print-seeds", "--stats", os.path.join(d, "rep", "ref.fa"), fq], capture_output=True, text=True, check=True)
        _rep_cache[kind] = (out.stdout.rstrip("\n").split("\n"), out.stderr)
    return _rep_cache[kind]


@pytest.mark.parametrize("kind", ["hifi", "ont", "sr", "sr_var", "hifi_w1", "hifi_edge", "ont_edge", "sr_edge", "hifi_sv", "ont_sv", "hifi_rep", "ont_rep", "sr_rep", "sr_rep_f60", "hifi_n", "sr_n"])
def test_host_path_matches_golden_sam(host_driver, kind, tmp_path):
    exe, d = host_driver
    base = SETS[kind][0]
    if kind in REP_KINDS:
        got, want = _rep_run(host_driver, kind, tmp_path)[0], golden_sam(kind)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a == b, (a[:200], b[:200])
        return
    fq = str(tmp_path / "reads.fq")
    with open(fq, "w") as f:
        for name, seq, qual in reads_of(kind):
            f.write("@%s\n%s\n+\n%s\n" % (name, seq, qual))
    out = subprocess.run([exe] + THREADS + cmd_of(kind) + [os.path.join(d, os.path.basename(base), "ref.fa"), fq], capture_output=True, text=True, check=True)
    got = out.stdout.rstrip("\n").split("\n")
    want = golden_sam(kind)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a == b, (a[:200], b[:200])


@pytest.mark.parametrize("kind", list(PAF_KINDS))
def test_host_path_matches_golden_paf(host_driver, kind, tmp_path):
    """mm_write_paf3 restated (gd_write_paf): the PAF lines of the reference for the same reads -- -c (cg:Z: tag), --paf-no-hit (lines of
    unmapped reads), supplementary / secondary records, the negative de:f values the reference prints for long insertions"""
    exe, d = host_driver
    base = SETS[kind][0]
    fq = str(tmp_path / "reads.fq")
    with open(fq, "w") as f:
        for name, seq, qual in reads_of(kind):
            f.write("@%s\n%s\n+\n%s\n" % (name, seq, qual))
    out = subprocess.run([exe] + THREADS + paf_cmd_of(kind) + [os.path.join(d, os.path.basename(base), "ref.fa"), fq], capture_output=True, text=True, check=True)
    got, want = out.stdout.rstrip("\n").split("\n"), golden_paf(kind)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a == b, (a[:300], b[:300])


def test_host_path_matches_reference_binary_on_fresh_reads(host_driver, tmp_path):
    ref_bin = os.path.join(ROOT, "oracle", "_ref", "gdiet_lr_avx")
    if not os.path.exists(ref_bin):
        pytest.skip("oracle/_ref not built (no /root/reference on this machine)")
    exe, d = host_driver
    fq = str(tmp_path / "fresh.fq")
    ref_fa = os.path.join(d, "lr", "ref.fa")
    subprocess.check_call(["python3", os.path.join(ROOT, "tools", "synth.py"), "reads", fq, "--ref", ref_fa, "--kind", "hifi", "--n", "20", "--seed", "77"])
    cmd = open(os.path.join(LR, "hifi.cmd")).read().split()
    want = subprocess.run([ref_bin, "-t", "4"] + cmd + [ref_fa, fq], capture_output=True, text=True, check=True).stdout
    want = [l for l in want.rstrip("\n").split("\n") if not l.startswith("@")]
    got = subprocess.run([exe] + cmd + [ref_fa, fq], capture_output=True, text=True, check=True).stdout.rstrip("\n").split("\n")
    assert [_norm_ms(x) for x in got] == [_norm_ms(x) for x in want]


def _norm_ms(line):
    """known, documented divergence (DESIGN.md "undefined behaviour in the reference"): for a reverse-strand record
    whose window contains reference Ns, mm_update_extra indexes mat[4*5+7] -- two bytes past the 25-entry
    matrix on mm_map_frag's stack -- so its ms:i value depends on the reference binary's stack layout (and may differ
    between two runs of the same binary).  Such a record is compared without that tag."""
    f = line.split("\t")
    if len(f) > 11 and f[1] in ("16", "272", "2064") and "nn:i:0" not in f:
        f = [x for x in f if not x.startswith("ms:i:")]
    return "\t".join(f)


@pytest.mark.parametrize("extra", ["", "-N 5 -n 0.3,0.1 -s 40 --AF_max_loc 20", "-k 15 -w 10 -Z 110 -W 3 -i 0.5 -r 0.1,20,100 -n 2,1 -s 30 -N 3"])
def test_sr_host_path_matches_reference_binary_on_fresh_reads(host_driver, tmp_path, extra):
    """ShortReads variant on a fresh read set of mixed lengths (60-600 bp: both geometry branches, SR/map.c:796/809),
    reads flush with the contig ends, Ns -- against a run of the reference binary"""
    ref_bin = os.path.join(ROOT, "oracle", "_ref", "gdiet_sr_avx")
    if not os.path.exists(ref_bin):
        pytest.skip("oracle/_ref not built (no /root/reference on this machine)")
    exe, d = host_driver
    fq = str(tmp_path / "fresh.fq")
    ref_fa = os.path.join(d, "sr", "ref.fa")
    subprocess.check_call(["python3", os.path.join(ROOT, "tools", "synth_sr_var.py"), "41", "1500", fq, ref_fa])
    cmd = (open(os.path.join(SR, "sr.cmd")).read() + " " + extra).split()
    want = subprocess.run([ref_bin, "-t", "4"] + cmd + [ref_fa, fq], capture_output=True, text=True, check=True).stdout
    want = [l for l in want.rstrip("\n").split("\n") if not l.startswith("@")]
    got = subprocess.run([exe] + cmd + [ref_fa, fq], capture_output=True, text=True, check=True).stdout.rstrip("\n").split("\n")
    assert got == want


@pytest.mark.parametrize("kind", ["hifi", "sr"])
def test_mmi_files_are_exchangeable_with_the_reference(host_driver, tmp_path, kind):
    """the .mmi reader / writer behind gdiet_hip_index_load_mmi / _dump_mmi (map_index.h): (1) an index file written by the
    reference (`GDiet_avx -d`) gives the golden SAM through our path; (2) an index file written by us is accepted by the
    reference and gives the golden SAM through ITS path -- and is the very file `GDiet_avx -d` writes, byte for byte"""
    variant = "sr" if kind == "sr" else "lr"
    ref_bin = os.path.join(ROOT, "oracle", "_ref", "gdiet_%s_avx" % variant)
    if not os.path.exists(ref_bin):
        pytest.skip("oracle/_ref not built (no /root/reference on this machine)")
    exe, d = host_driver
    ref_fa = os.path.join(d, variant, "ref.fa")
    fq = str(tmp_path / "reads.fq")
    reads = reads_of(kind)[:400]
    with open(fq, "w") as f:
        for name, seq, qual in reads:
            f.write("@%s\n%s\n+\n%s\n" % (name, seq, qual))
    names = {r[0] for r in reads}
    golden = [l for l in golden_sam(kind) if l.split("\t")[0] in names]
    cmd = cmd_of(kind)
    want = subprocess.run([ref_bin, "-t", "4"] + cmd + [ref_fa, fq], capture_output=True, text=True, check=True).stdout
    want = [l for l in want.rstrip("\n").split("\n") if not l.startswith("@")]
    theirs, ours = str(tmp_path / "theirs.mmi"), str(tmp_path / "ours.mmi")
    subprocess.run([ref_bin, "-t", "4"] + cmd + ["-d", theirs, ref_fa], capture_output=True, check=True)
    got = subprocess.run([exe] + cmd + ["--mmi=" + theirs, ref_fa, fq], capture_output=True, text=True, check=True).stdout.rstrip("\n").split("\n")
    assert got == golden  # our path is deterministic: the committed golden SAM, every tag included
    assert [_norm_ms(x) for x in got] == [_norm_ms(x) for x in want]
    subprocess.run([exe] + cmd + ["--dump-mmi=" + ours, ref_fa, fq], capture_output=True, check=True)
    assert open(ours, "rb").read() == open(theirs, "rb").read()  # byte-identical to mm_idx_dump, khash slot order included
    back = subprocess.run([ref_bin, "-t", "4"] + cmd + [ours, fq], capture_output=True, text=True, check=True).stdout
    assert [_norm_ms(l) for l in back.rstrip("\n").split("\n") if not l.startswith("@")] == [_norm_ms(x) for x in want]


def _split_trace(lines):
    """per read: the --print-seeds lines by stage (a read starts at its "Final shift" line)"""
    per_read, cur = [], None
    for line in lines:
        if line.startswith("Final shift"):
            cur = {"shift": line, "RS": [], "SD": [], "VT": [], "AVT": [], "BE": [], "AL": [], "CON": []}
            per_read.append(cur)
        elif cur is not None:
            for key, prefix in (("RS", "RS "), ("SD", "SD\t"), ("SD", "SDX\t"), ("VT", "VT\t"), ("AVT", "AVT\t"), ("BE", "BE\t"), ("AL", "AL_SCORE"), ("CON", "CON")):
                if line.startswith(prefix):
                    cur[key].append(line)
    for r in per_read:
        r["SD"].sort()
    return per_read


@pytest.mark.parametrize("kind", ["hifi", "ont", "sr", "hifi_sv", "ont_sv", "hifi_rep", "ont_rep", "sr_rep"])
def test_stage_trace_matches_the_reference(host_driver, tmp_path, kind):
    """stage-level parity (the reference's --print-seeds trace, committed as <kind>.trace.gz by oracle/make_golden.py):
    chosen pattern phase, sorted seed hits of both strands, vote candidates before and after linking (second voting round
    included), DP boxes, DP scores and the CONQ / CONT line pairs of every concatenate_cigars call, line for line.  Hits with
    equal targets may be ordered differently by the two sorts, so the SD lines are compared as a multiset per read (for the
    repeat-rich sets, whose reads have up to 280 000 hits per strand: as their count and the sha1 of the sorted lines)."""
    exe, d = host_driver
    ref_fa = os.path.join(d, os.path.basename(SETS[kind][0]), "ref.fa")
    fq = str(tmp_path / "reads.fq")
    reads = reads_of(kind)
    if kind in REP_KINDS:
        err = _rep_run(host_driver, kind, tmp_path)[1]
    else:
        with open(fq, "w") as f:
            for name, seq, qual in reads:
                f.write("@%s\n%s\n+\n%s\n" % (name, seq, qual))
        err = subprocess.run([exe] + THREADS + cmd_of(kind) + ["--print-seeds", ref_fa, fq], capture_output=True, text=True, check=True).stderr
    mine = [l for l in err.split("\n") if l.startswith(TRACE_PREFIXES)]
    want, got = _split_trace(trace_of(kind)), _split_trace(digest_sd(mine) if kind in SD_DIGESTED else mine)
    assert len(want) == len(got) == len(reads)
    for a, b in zip(want, got):
        assert a == b
    assert sum(len(r["SD"]) for r in want) > (20 if kind in SD_DIGESTED else 100) and sum(len(r["VT"]) for r in want) > 0
    if kind.endswith("_sv"):  # the fixtures exist for these stages
        assert sum(len(r["CON"]) for r in want) >= 2 * 20


# what each repeat-rich set must reach, as counted by the host emulator's --stats (every number a lower bound on the count of READS
# on which the branch fires): mm_seed_mz_flt dropping minimizers (SR/seed.c:5-29); a streak of seeds above mid_occ with a rescue
# budget (SR/seed.c:79-98) and with more seeds than the budget, i.e. the heap with replacement (:89-94); a seed above max_max_occ
# (:101-102); a strand with more than 4096 hits (the wave vote kernel's LDS-run merge path, MAP_VOTE_CAP)
REP_MUST_REACH = {"hifi_rep": dict(mz_flt_drops=10, rescue=20, heap_replace=10, over_max_max_occ=5, big_strand=50),
                  "ont_rep": dict(mz_flt_drops=4, rescue=10, heap_replace=10, over_max_max_occ=5, big_strand=30),
                  "sr_rep": dict(mz_flt_drops=0, rescue=5, heap_replace=5, over_max_max_occ=100, big_strand=50),
                  "sr_rep_f60": dict(mz_flt_drops=5, rescue=10, heap_replace=10, over_max_max_occ=100, big_strand=1)}


@pytest.mark.parametrize("kind", list(REP_MUST_REACH))
def test_rep_fixtures_reach_the_high_occurrence_branches(host_driver, tmp_path, kind):
    """the repeat-rich sets exist to make the high-occurrence branches of the seeding stage fire; count them (and the index keys
    above mid_occ / max_max_occ) with the product's own stage code on the host"""
    import re
    err = _rep_run(host_driver, kind, tmp_path)[1]
    st = dict(re.findall(r"([a-z_>0-9()]+)=(\d+)", " ".join(l for l in err.split("\n") if l.startswith("[stats]"))))
    num = {k.split("(")[0]: int(v) for k, v in st.items()}
    assert num["keys>mid_occ"] >= 5 and num["keys>max_max_occ"] >= 3 and num["multi"] >= 2000 and num["max_count"] > 4095
    need = REP_MUST_REACH[kind]
    assert num["mz_flt_drops"] >= need["mz_flt_drops"] and num["rescue"] >= need["rescue"] and num["heap_replace"] >= need["heap_replace"]
    assert num["over_max_max_occ"] >= need["over_max_max_occ"] and num["strand>4096hits"] >= need["big_strand"]


def test_rep_mmi_files_are_the_reference_s(host_driver, tmp_path):
    """the .mmi writer on an index with thousands of multi-occurrence position lists (p[] arrays of up to 8 000 entries, khash
    buckets with non-singleton keys): the file has the size and sha256 of the one `GDiet_avx -d` wrote for the same reference and
    command line (tests/golden/rep/mmi.sha256.json, oracle/make_golden.py) -- the other references' p[] arrays are empty"""
    import hashlib
    import json
    exe, d = host_driver
    want = json.load(open(os.path.join(REP, "mmi.sha256.json")))
    fq = str(tmp_path / "none.fq")
    open(fq, "w").write("@r\nACGT\n+\nIIII\n")
    for tag, kind in (("k19w19", "hifi_rep"), ("k15w10", "ont_rep"), ("k21w11", "sr_rep")):
        ours = str(tmp_path / (tag + ".mmi"))
        subprocess.run([exe] + cmd_of(kind) + ["--dump-mmi=" + ours, os.path.join(d, "rep", "ref.fa"), fq], capture_output=True, check=True)
        data = open(ours, "rb").read()
        assert len(data) == want[tag]["size"] and hashlib.sha256(data).hexdigest() == want[tag]["sha256"], tag


def test_sv_fixtures_reach_concatenation_supplementary_and_secondary_records():
    """what the *_sv goldens hold (>= 50 concatenate_cigars events, >= 30 supplementary, >= 5 secondary records)"""
    flags, conq = {}, 0
    for kind in ("hifi_sv", "ont_sv"):
        for line in golden_sam(kind):
            fl = int(line.split("\t")[1])
            flags[fl] = flags.get(fl, 0) + 1
        conq += sum(1 for l in trace_of(kind) if l.startswith("CONQ"))
    assert conq >= 50 and flags.get(2048, 0) + flags.get(2064, 0) >= 30 and flags.get(256, 0) + flags.get(272, 0) >= 5


def test_committed_goldens_are_what_the_reference_prints():
    """oracle/make_golden.py in check mode: every committed golden SAM / trace / parser fixture is reproduced by the reference
    binaries compiled here (skipped where /root/reference, hence oracle/_ref, does not exist)"""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "gdiet_lr_avx")):
        pytest.skip("oracle/_ref not built (no /root/reference on this machine)")
    r = subprocess.run(["python3", os.path.join(ROOT, "oracle", "make_golden.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- the option grid (tests/golden/opts/grid.json): patterns, k, w, vote / gap / band options, strand flags and scorings away from
# the README command lines; goldens by the reference binaries (oracle/make_grid_golden.py) ----------------------------------------
@pytest.mark.parametrize("name", grid_ids())
def test_grid_host_path_matches_committed_sam_and_trace(host_driver, tmp_path, name):
    """every row of the grid through the product's stage code on the host: the SAM the reference printed (SEQ / QUAL starred on both
    sides) and its stage trace (pattern phase, seed hits of both strands as count + sha1, vote candidates of both rounds, boxes, DP
    scores, concatenations), line for line.  Rows with "build": "scalar" hold what scalar GDiet printed at a window size where GDiet_avx
    sketches differently ("Known divergence"): the library's choice between the two is pinned here."""
    import re
    exe, d = host_driver
    row = grid_row(name)
    ref_fa = os.path.join(d, os.path.basename(SETS[row["kind"]][0]), "ref.fa")
    fq = str(tmp_path / "reads.fq")
    reads = grid_reads(row)
    assert len(reads) == row["n_reads"]
    with open(fq, "w") as f:
        for qn, seq, qual in reads:
            f.write("@%s\n%s\n+\n%s\n" % (qn, seq, qual))
    out = subprocess.run([exe] + THREADS + grid_cmd(row) + ["--print-seeds", "--stats", ref_fa, fq], capture_output=True, text=True, check=True)
    got, want = [star_seq_qual(l) for l in out.stdout.rstrip("\n").split("\n")], grid_golden_sam(row)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a == b, (a[:300], b[:300])
    mine = digest_sd([l for l in out.stderr.split("\n") if l.startswith(TRACE_PREFIXES)])
    want_t, got_t = _split_trace(grid_trace(row)), _split_trace(mine)
    assert len(want_t) == len(got_t) == len(reads)
    for a, b in zip(want_t, got_t):
        assert a == b
    st = dict(re.findall(r"([a-z_>0-9()]+)=(\d+)", " ".join(l for l in out.stderr.split("\n") if l.startswith("[stats]"))))
    if "mz_flt" in row["tags"]:  # -f low enough for the query-side filter of the ShortReads variant (see "sr_rep_f60" in fixture_io.py)
        assert int(st["mz_flt_drops"]) >= 5
    if "retry" in row["tags"]:  # reads whose minimizers overflow the first scratch estimate of the GPU path (map_plan.h gd_scratch_layout)
        assert int(st["over_first_scratch"]) >= row["n_reads"] // 2


@pytest.mark.parametrize("name", [r["name"] for r in grid_rows() if not {"kw", "strand"} & set(r["tags"])])
def test_grid_options_are_not_inert(host_driver, tmp_path, name):
    """the vote / gap / band / capacity / scoring rows: leaving out any one option group of the row makes the host path print something
    other than the committed SAM and trace -- every option the row names decides part of its golden (the writer asserts the same of
    the reference for every row)"""
    exe, d = host_driver
    row = grid_row(name)
    ref_fa = os.path.join(d, os.path.basename(SETS[row["kind"]][0]), "ref.fa")
    fq = str(tmp_path / "reads.fq")
    with open(fq, "w") as f:
        for qn, seq, qual in grid_reads(row):
            f.write("@%s\n%s\n+\n%s\n" % (qn, seq, qual))
    want = (grid_golden_sam(row), _split_trace(grid_trace(row)))
    assert row["sensitive"]
    for group in row["sensitive"]:
        out = subprocess.run([exe] + THREADS + grid_cmd(row, group) + ["--print-seeds", ref_fa, fq], capture_output=True, text=True, check=True)
        sam = [star_seq_qual(l) for l in out.stdout.rstrip("\n").split("\n")]
        trace = _split_trace(digest_sd([l for l in out.stderr.split("\n") if l.startswith(TRACE_PREFIXES)]))
        assert (sam, trace) != want, (name, group)


def test_grid_rows_cannot_pass_vacuously():
    """what oracle/make_grid_golden.py asserts when it writes the fixtures, again on the committed files: the reference maps at least
    min_mapped of every row's reads (0.9 for LongReads rows; 0.4 where the row is built to starve seeds or keeps one strand of a
    two-strand read set; 0.5 for ShortReads rows on var.fq; 0.25 for the scoring rows, whose scorings the reference itself maps fewer reads
    at), strand rows hold mapped and unmapped reads, the *_sv rows reach the second voting round's concatenations, every read has a trace,
    and a scoring row holds the records it was chosen for (fixture_io.assert_score_row_conditions: both sides of the widened pre-filter's
    bound, Ns inside alignments at e2 = 2, a wave / generic tag that gdo.wave_scoring_ok confirms)"""
    for row in grid_rows():
        sam, trace = grid_golden_sam(row), grid_trace(row)
        mapped, n = mapped_share(sam)
        assert n == row["n_reads"] and mapped >= row["min_mapped"] * n, (row["name"], mapped, n)
        floor = 0.25 if row["kind"] in ("sr", "sr_rep") or "score" in row["tags"] else 0.5 if row["variant"] == "sr" else 0.4 if ("strand" in row["tags"] or row["overrides"].get("k") == 28) else 0.9
        assert row["min_mapped"] >= floor, row["name"]
        if "strand" in row["tags"]:
            assert 0 < mapped < n, row["name"]
            flags = {int(l.split("\t")[1]) & 16 for l in sam if l.split("\t")[2] != "*"}
            assert flags == ({0} if "--for-only" in row["extra"] else {16}), row["name"]
        if "sv" in row["tags"]:
            assert sum(1 for l in trace if l.startswith("CONQ")) >= 5, row["name"]
        if "score" in row["tags"]:
            assert_score_row_conditions(row, sam)
        if "vote_cap" in row["tags"]:  # reads of the repeat-rich reference with more candidates than any preset's vt_nb_loc + 2 = 7 keeps
            per_read = [len(r["VT"]) for r in _split_trace(trace)]
            assert sum(1 for c in per_read if c > 7) >= 10, (row["name"], per_read)
        assert sum(1 for l in trace if l.startswith("Final shift")) == n and all(l.split("\t")[9] == "*" for l in sam)


def test_grid_covers_what_it_was_built_for():
    """the table itself: between them the rows reach the patterns, k / w limits, vote capacities, flags and scorings no README command
    line reaches; both the command-line form and the Mapper overrides of a row name the same options"""
    rows = grid_rows()
    assert len({r["name"] for r in rows}) == len(rows)
    ov = [dict(r["overrides"], variant=r["variant"], build=r["build"]) for r in rows]
    pats = [o["Z"] for o in ov if "Z" in o]
    assert sum(1 for z in set(pats) if z.count("1") > 1) >= 3 and any(z[0] == "0" and z.count("1") > 1 for z in pats)
    assert "1" in pats and any(len(z) >= 32 and z.count("1") <= 8 for z in pats) and any(z.count("1") == 40 for z in pats)
    ks, ws = {o.get("k") for o in ov}, {o.get("w") for o in ov}
    assert 28 in ks and any(k is not None and k <= 12 for k in ks) and 64 in ws and ws & {8, 9} and any("retry" in r["tags"] for r in rows)
    lr, sr = [o for o in ov if o["variant"] == "lr"], [o for o in ov if o["variant"] == "sr"]
    assert {22, 1} <= {o.get("vt_nb_loc") for o in lr} and any(o.get("max_seeds", 0) >= 1 for o in lr) and any(0 < o.get("max_seeds", 0) < 1 for o in lr)
    for key in ("vt_dis", "vt_df1", "vt_df2", "vt_cov", "vt_f", "max_min_gap", "max_max_gap", "bw"):
        assert any(key in o for o in lr), key
    assert any(o.get("best_n", 1) > 1 for o in lr)
    assert {24, 1} <= {o.get("AF_max_loc") for o in sr} and any("bw_max" in o for o in sr) and any("rec_threshold_frac" in o for o in sr)
    assert any("mz_flt" in r["tags"] for r in rows)
    for var in ("lr", "sr"):
        fl = {o.get("flag", 0) & 0x300000 for o in ov if o["variant"] == var}
        assert {0x100000, 0x200000} <= fl, var
        # one row per variant pinned to the scalar build, at a window size in 2..7 -- and no GDiet_avx row there
        assert [o["w"] for o in ov if o["variant"] == var and o["build"] == "scalar"] == [4]
    assert all(not (2 <= o.get("w", 10) <= 7) for o in ov if o["build"] == "avx")
    assert sum(1 for o in ov if "q2" in o) >= 2 and len(grid_rows("mmi")) == 3
    # the scoring rows: every kind of scoring the DP dispatch, the pre-filter and the post kernels treat differently, per variant
    from fixture_io import grid_scoring, grid_wave_scoring_ok
    import gdo
    score = grid_rows("score")
    assert all("post" in r["tags"] and ("wave" in r["tags"]) == grid_wave_scoring_ok(r) != ("generic" in r["tags"]) for r in score)
    sc_of = {r["name"]: grid_scoring(r) + (0,) for r in score}
    lr_sc = {n: v for n, v in sc_of.items() if grid_row(n)["variant"] == "lr"}
    sr_sc = {n: v for n, v in sc_of.items() if grid_row(n)["variant"] == "sr"}
    table = gdo.SCORINGS
    for want in ("bound120_last", "bound120_first", "k3_2_16_24_1"):  # long reads at the table's own entries
        assert table[want] in lr_sc.values(), want
    assert gdo.wave_scoring_ok(*table["bound120_last"]) and not gdo.wave_scoring_ok(*table["bound120_first"]) and not gdo.wave_scoring_ok(*table["k3_2_16_24_1"])
    assert any(v[:6] == (1, 4, 6, 2, 6, 2) for v in lr_sc.values())  # single affine at the HiFi preset's a, b
    assert any(v == table["a16"] and grid_row(n)["kind"] == "ont_sv" for n, v in lr_sc.items())
    assert any(v[5] == 2 and v[3] > 2 for v in lr_sc.values()) and any("n_e2" in grid_row(n)["tags"] for n in lr_sc)
    for want in ("a16", "skey_corner", "single_affine"):  # short reads
        assert table[want] in sr_sc.values(), want
    assert all("prefilter" in grid_row(n)["tags"] for n, v in sr_sc.items() if v in (table["a16"], table["skey_corner"]))
    assert any(not gdo.wave_scoring_ok(*v) and v[4] == 48 for v in sr_sc.values())
    assert any(v[5] == 2 and grid_row(n)["kind"] == "sr_edge" for n, v in sr_sc.items()) and any("n_e2" in grid_row(n)["tags"] for n in sr_sc)
    for r in rows:  # every option of a row is one of its sensitive groups
        assert " ".join(r["sensitive"]).split() == r["extra"].split(), r["name"]
    for r in rows:  # the two forms of a row agree on the options both can be read from
        toks = r["extra"].replace("=", " ").split()
        for opt, key in (("-k", "k"), ("-w", "w"), ("-Z", "Z"), ("-W", "W"), ("-N", "best_n"), ("--vt_nb_loc", "vt_nb_loc"), ("--AF_max_loc", "AF_max_loc"), ("-A", "a"), ("-B", "b")):
            assert (opt in toks) == (key in r["overrides"]), (r["name"], opt)
            if opt in toks:
                assert str(r["overrides"][key]) == toks[toks.index(opt) + 1], (r["name"], opt)


def test_grid_goldens_are_what_the_reference_prints():
    """oracle/make_grid_golden.py in check mode: every committed file of the grid is reproduced by the reference binaries compiled here,
    and the conditions it asserts on them hold (skipped where the reference's sources, hence oracle/_ref, do not exist)"""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "gdiet_lr_avx")):
        pytest.skip("oracle/_ref not built (no /root/reference on this machine)")
    r = subprocess.run(["python3", os.path.join(ROOT, "oracle", "make_grid_golden.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_grid_mmi_files_are_the_reference_s(host_driver, tmp_path):
    """the host index builder + .mmi writer at three non-preset k / w / pattern settings: size and sha256 of the file the reference wrote"""
    import hashlib
    import json
    from fixture_io import OPTS
    exe, d = host_driver
    want = json.load(open(os.path.join(OPTS, "mmi.sha256.json")))
    fq = str(tmp_path / "none.fq")
    open(fq, "w").write("@r\nACGT\n+\nIIII\n")
    for row in grid_rows("mmi"):
        ours = str(tmp_path / (row["name"] + ".mmi"))
        ref_fa = os.path.join(d, os.path.basename(SETS[row["kind"]][0]), "ref.fa")
        subprocess.run([exe] + grid_cmd(row) + ["--dump-mmi=" + ours, ref_fa, fq], capture_output=True, check=True)
        data = open(ours, "rb").read()
        assert len(data) == want[row["name"]]["size"] and hashlib.sha256(data).hexdigest() == want[row["name"]]["sha256"], row["name"]

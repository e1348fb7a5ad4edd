#!/usr/bin/env python3
"""Test infrastructure: (re)makes the fixtures of --eqx for the ShortReads variant (tests/golden/eqx/) with THE REFERENCE ITSELF, in the
style of tools/make_tags_golden.py.  The only writer of that directory.

    python tools/make_eqx_golden.py            # check: every committed file equals what the reference prints today
    python tools/make_eqx_golden.py --write    # rewrite them

Sets: sr_edge, sr, sr_var (tests/golden/sr/, their committed command lines) and "syn", a synthetic set made here (SYN_* below): one contig
of a few kbp with a short N run, and a few dozen 150 bp reads built so that the reference itself prints every kind of record
tests/eqx_ref.py names (KIND_NAMES).
  syn_ref.fa.gz, syn.fq.gz  the synthetic reference and reads (from the fixed recipe below: nothing random is left at run time)
  syn.golden.sam.gz         `gdiet_sr_avx -t 4 <sr.cmd>` on them: the plain SAM of the synthetic set
  <set>.sam.tsv.gz          one row per SAM record of `gdiet_sr_avx -t 4 <set's .cmd> --eqx`: qname, FLAG, POS, CIGAR
  sr.paf.tsv.gz             one row per PAF line of `gdiet_sr_avx -t 4 <paf_cmd_of("sr")> --eqx` (-c --paf-no-hit): qname, query start,
                            strand, the text of cg:Z: ("" for an unmapped read)
What is asserted on the way: under --eqx no M is left in a CIGAR; every column of a SAM line but the CIGAR, and every column and tag of a
PAF line but cg:Z:, is the committed plain one (printed as "other PAF columns moved: 0 lines"; a line that moves fails the run);
--eqx --MD / --cs / --cs=long print the --eqx line with the tag of tests/golden/tags/ (sr, sr_edge); every set holds at least one record
of each kind of COVER.  The counts are printed.
Nothing of the product is involved in what is written."""
import argparse
import gzip
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import eqx_ref as er  # noqa: E402
from diffstr_ref import tag_rows  # noqa: E402
from fixture_io import SR, cmd_of, golden_paf, paf_cmd_of  # noqa: E402
from make_golden import REF, _gunzip_to, _write_gz  # noqa: E402

BIN = REF["sr"]
MODES = {"md": ["--MD"], "cs": ["--cs"], "cs_long": ["--cs=long"]}
# (mapped records, records with an X, lines) the reference gave when the fixtures were written
COUNTS = {"sr": (1693, 1201, 2000), "sr_var": (861, 539, 1200), "sr_edge": (13, 2, 20)}
# the kinds (eqx_ref.KIND_NAMES) every set must hold at least one record of: what its reads give -- no committed read set has an N facing
# an N of the reference inside an alignment, and only sr has count-rule records; the synthetic set is written to have them all
COVER = {"sr": ("count_rule", "lead_x", "exact", "diag_x", "shift"), "sr_var": ("lead_x", "exact", "diag_x", "shift"),
         "sr_edge": ("exact", "diag_x", "shift"), "syn": er.KIND_NAMES}

# ---- the synthetic set -------------------------------------------------------------------------------------------------------------------
SYN_LEN, SYN_N_AT, SYN_N_LEN, SYN_RL = 6000, 3000, 2, 150
# (name, start on the contig, strand, edits in read coordinates on the forward strand, before the reverse complement)
#   ("s", at, k): substitute base at by the k-th other base;  ("d", at, n): drop n reference bases behind read base at;
#   ("i", at, n): insert n bases in front of read base at;  ("n", at): an N in the read
SYN_READS = (
    ("exact_f0", 200, "+", ()), ("exact_f1", 1234, "+", ()), ("exact_r0", 500, "-", ()), ("exact_r1", 4100, "-", ()),
    ("sub1_f", 800, "+", (("s", 75, 1),)), ("sub3_f", 1000, "+", (("s", 10, 0), ("s", 11, 2), ("s", 140, 1))), ("sub2_r", 1500, "-", (("s", 30, 0), ("s", 100, 2))),
    ("first_x_f", 1700, "+", (("s", 0, 1),)), ("first2_x_f", 1900, "+", (("s", 0, 0), ("s", 1, 2), ("s", 90, 1))), ("last_x_f", 2100, "+", (("s", 149, 1),)),
    ("first_x_r", 2300, "-", (("s", 149, 2),)), ("last_x_r", 2500, "-", (("s", 0, 0),)),
    ("nn_f", 2930, "+", ()), ("nn_f_sub", 2900, "+", (("s", 20, 1),)), ("nn_r", 2940, "-", ()), ("nn_r_sub", 2890, "-", (("s", 60, 0),)),
    ("n_read_f", 3300, "+", (("n", 70),)), ("n_read_r", 3500, "-", (("n", 40),)), ("n_edge_f", 2999, "+", ()), ("n_edge_r", 2852, "-", ()),
    ("del5_f", 3700, "+", (("d", 75, 5),)), ("del5_r", 3900, "-", (("d", 75, 5),)), ("ins4_f", 4300, "+", (("i", 80, 4),)), ("ins4_r", 4500, "-", (("i", 80, 4),)),
    ("del1_end_f", 4700, "+", (("d", 148, 1),)), ("del1_start_f", 4900, "+", (("d", 1, 1),)), ("ins1_end_f", 5100, "+", (("i", 148, 1),)), ("ins1_start_f", 5300, "+", (("i", 1, 1),)),
    ("del20_f", 5500, "+", (("d", 100, 20),)), ("del20_r", 300, "-", (("d", 100, 20),)), ("ins10_f", 600, "+", (("i", 50, 10),)), ("ins10_r", 900, "-", (("i", 50, 10),)),
    ("del3_sub_f", 1100, "+", (("d", 60, 3), ("s", 20, 1))), ("ins2_sub_r", 1300, "-", (("i", 90, 2), ("s", 120, 0))), ("del2_lastx_f", 1600, "+", (("d", 40, 2), ("s", 149, 2))),
    ("del1_near_end_r", 1800, "-", (("d", 5, 1),)), ("ins1_near_end_r", 2000, "-", (("i", 5, 1),)), ("del1_sub_end_f", 2200, "+", (("d", 146, 1), ("s", 149, 0))),
    ("ins1_sub_end_f", 2400, "+", (("i", 146, 1), ("s", 149, 1))), ("start_of_contig", 0, "+", (("s", 3, 1),)), ("end_of_contig", SYN_LEN - SYN_RL, "+", (("s", 147, 2),)),
    ("end_of_contig_r", SYN_LEN - SYN_RL, "-", ()), ("start_of_contig_r", 0, "-", (("s", 100, 1),)),
)


def syn_set():
    """(contig, [(name, sequence, quality)]) of the recipe"""
    rng = np.random.default_rng(20240607)
    ref = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, SYN_LEN)].copy()
    ref[SYN_N_AT:SYN_N_AT + SYN_N_LEN] = ord("N")
    ref = ref.tobytes().decode()
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    reads = []
    for name, at, strand, edits in SYN_READS:
        src = list(ref[at:at + SYN_RL + 64])  # (what a deletion pulls in from behind the read)
        rd = [[c] for c in src]  # per reference base: the read bases it gives
        for e in sorted(edits, key=lambda e: -e[1]):
            if e[0] == "s":
                rd[e[1]] = ["ACGT".replace(src[e[1]], "")[e[2]] if src[e[1]] != "N" else "A"]
            elif e[0] == "n":
                rd[e[1]] = ["N"]
            elif e[0] == "d":
                for j in range(e[1] + 1, e[1] + 1 + e[2]):
                    rd[j] = []
            elif e[0] == "i":
                ins = "".join("ACGT"[(ord(src[e[1]]) + 1 + j) % 4] for j in range(e[2]))
                rd[e[1]] = list(ins) + rd[e[1]]
        seq = "".join(c for b in rd for c in b)[:SYN_RL]
        if strand == "-":
            seq = "".join(comp[c] for c in reversed(seq))
        assert len(seq) == SYN_RL, name
        reads.append(("syn_%s" % name, seq, "I" * SYN_RL))
    return ref, reads


# ---- running the reference ---------------------------------------------------------------------------------------------------------------
def inputs(kind, tmp):
    """(reference FASTA, reads FASTQ) of a set as plain files under tmp"""
    ref_fa = os.path.join(tmp, ("syn" if kind == "syn" else "sr") + "_ref.fa")
    if not os.path.exists(ref_fa):
        _gunzip_to(os.path.join(er.EQX, "syn_ref.fa.gz") if kind == "syn" else os.path.join(SR, "ref.fa.gz"), ref_fa)
    fq = os.path.join(tmp, kind + ".fq")
    if not os.path.exists(fq):
        with open(fq, "w") as f:
            for name, seq, qual in er.reads_of_kind(kind):
                f.write("@%s\n%s\n+\n%s\n" % (name, seq, qual))
    return ref_fa, fq


def cmd(kind):
    return cmd_of("sr" if kind == "syn" else kind)


def run(kind, args, tmp):
    ref_fa, fq = inputs(kind, tmp)
    out = subprocess.run([BIN, "-t", "4"] + args + [ref_fa, fq], capture_output=True, text=True, check=True).stdout
    return [l for l in out.split("\n") if l and not l.startswith("@")]


def sam_rows(kind, tmp):
    """[(qname, FLAG, POS, CIGAR)] of the reference's SAM under --eqx, after the checks of the module text"""
    lines, plain = run(kind, cmd(kind) + ["--eqx"], tmp), er.plain_sam(kind)
    assert len(lines) == len(plain), (kind, len(lines), len(plain))
    out = []
    for l, g in zip(lines, plain):
        f, fg = l.split("\t"), g.split("\t")
        assert f[:5] + f[6:] == fg[:5] + fg[6:], (kind, f[0])  # only the CIGAR column changes
        assert "M" not in f[5] and (f[5] == "*") == (fg[5] == "*"), (kind, f[0], f[5])
        out.append((f[0], f[1], f[3], f[5]))
    n_map, n_x = sum(1 for r in out if r[3] != "*"), sum(1 for r in out if "X" in r[3])
    if kind in COUNTS:
        assert (n_map, n_x, len(out)) == COUNTS[kind], (kind, n_map, n_x, len(out))
    print("    %s: %d mapped of %d, %d with an X" % (kind, n_map, len(out), n_x))
    return out


def check_tags(kind, rws, tmp):
    """--eqx --MD / --cs / --cs=long: the --eqx line with the committed tag in front of rl:i:0"""
    plain = er.plain_sam(kind)
    for mode, arg in MODES.items():
        tags = tag_rows("%s.%s" % (kind, mode))
        lines = run(kind, cmd(kind) + ["--eqx"] + arg, tmp)
        assert len(lines) == len(plain)
        for l, g, r, tg in zip(lines, plain, rws, tags):
            f, fg = l.split("\t"), g.split("\t")
            fg[5] = r[3]
            if tg[4]:
                assert fg[-1] == "rl:i:0"
                fg.insert(len(fg) - 1, ("MD:Z:" if mode == "md" else "cs:Z:") + tg[4])
            assert f == fg, (kind, mode, f[0])
    print("    %s: --eqx with --MD / --cs / --cs=long carries the committed tags" % kind)


def paf_rows(kind, tmp):
    """[(qname, query start, strand, cg text)] of the reference's PAF under -c --paf-no-hit --eqx; every other field must be the committed one"""
    lines, plain = run(kind, paf_cmd_of(kind) + ["--eqx"], tmp), golden_paf(kind)
    assert len(lines) == len(plain), (kind, len(lines), len(plain))
    out, moved = [], 0
    for l, g in zip(lines, plain):
        f, fg = l.split("\t"), g.split("\t")
        cg = [x for x in f if x.startswith("cg:Z:")]
        assert len(cg) == (f[4] != "*") and all("M" not in x[5:] for x in cg), (kind, f[0])
        moved += [x for x in f if not x.startswith("cg:Z:")] != [x for x in fg if not x.startswith("cg:Z:")]
        out.append((f[0], f[2], f[4], cg[0][5:] if cg else ""))
    print("    %s: other PAF columns moved: %d lines" % (kind, moved))
    assert moved == 0, (kind, moved)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    if not os.path.exists(BIN):
        sys.exit("oracle/_ref is not built (make -f oracle/Makefile.ref needs the reference's sources)")
    os.makedirs(er.EQX, exist_ok=True)
    bad = 0

    def put(name, text):
        nonlocal bad
        path = os.path.join(er.EQX, name)
        same = os.path.exists(path) and gzip.open(path, "rt").read() == text
        if not same and a.write:
            _write_gz(path, text)
        bad += not same
        print("%-44s %s" % (os.path.relpath(path, ROOT), "ok" if same else ("WRITTEN" if a.write else "DIFFERS")))

    ref, reads = syn_set()
    put("syn_ref.fa.gz", ">syn1\n" + "".join(ref[i:i + 60] + "\n" for i in range(0, len(ref), 60)))
    put("syn.fq.gz", "".join("@%s\n%s\n+\n%s\n" % r for r in reads))
    if bad and not a.write:
        sys.exit("the synthetic inputs differ from the recipe: nothing else checked")
    with tempfile.TemporaryDirectory() as tmp:
        put("syn.golden.sam.gz", "".join(l + "\n" for l in run("syn", cmd("syn"), tmp)))
        if bad and not a.write:
            sys.exit("the plain SAM of the synthetic set differs: nothing else checked")
        for kind in er.KINDS:
            rws = sam_rows(kind, tmp)
            got = er.kinds_of(kind, rws)
            print("    %s: %s" % (kind, got))
            for what in COVER[kind]:
                assert got[what] > 0, (kind, what)
            if kind in ("sr", "sr_edge"):
                check_tags(kind, rws, tmp)
            put(kind + ".sam.tsv.gz", "".join("\t".join(r) + "\n" for r in rws))
        put("sr.paf.tsv.gz", "".join("\t".join(r) + "\n" for r in paf_rows("sr", tmp)))
    sys.exit(0 if a.write or not bad else 1)


if __name__ == "__main__":
    main()

"""CPU: the per-base difference strings (cs / cs=long / MD; LR/format.c:150-268).
  * tools/make_tags_golden.py in check mode: the committed tags are what the reference prints;
  * the Python restatement (tests/diffstr_ref.py) reproduces every committed tag from the golden SAM's POS / CIGAR (the golden PAF's
    columns), the read and ref.fa.gz -- that pins it as the expected value of the synthetic cases here and on the GPU;
  * the kernel's per-lane core (map_diffstr.h) on 64 emulated lanes (tests/emul/diffstr_emul.cpp), count pass and write pass, over
    every record of the goldens in the three modes (hifi_sv under qstrand as well) and over the synthetic set."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import diffstr_ref as dr
from fixture_io import SETS, golden_paf, golden_sam, read_fasta, reads_of

SAM_KINDS = ("hifi_sv", "ont_sv", "hifi_edge", "sr", "sr_edge")
PAF_ROWS = (("hifi_sv", "cs", "cs", False), ("hifi_sv", "qstrand_cs", "cs", True), ("hifi_sv", "qstrand_md", "md", True), ("sr", "cs", "cs", False))
TAGGED = {"hifi_sv": (187, 193), "ont_sv": (65, 71), "sr": (1693, 2000), "hifi_edge": (7, 17), "sr_edge": (13, 20)}

_cache = {}


def kind_inputs(kind):
    """(contig names, contigs as nt4, read names -> index, reads as nt4) of a kind, made once"""
    if kind not in _cache:
        names, seqs = read_fasta(os.path.join(SETS[kind][0], "ref.fa.gz"))
        reads = reads_of(kind)
        _cache[kind] = (names, [dr.nt4(s) for s in seqs], {r[0]: i for i, r in enumerate(reads)}, [dr.nt4(r[1]) for r in reads])
    return _cache[kind]


def sam_records(kind):
    """(records of the kind's mapped golden SAM lines, their line numbers)"""
    names, _, ridx, reads4 = kind_inputs(kind)
    recs, at = [], []
    for i, line in enumerate(golden_sam(kind)):
        f = line.split("\t")
        if f[5] == "*":
            continue
        recs.append(dr.record_of_sam(f, ridx[f[0]], len(reads4[ridx[f[0]]]), names.index(f[2])))
        at.append(i)
    return recs, at


def paf_records(kind):
    names, _, ridx, _ = kind_inputs(kind)
    recs, at = [], []
    for i, line in enumerate(golden_paf(kind)):
        f = line.split("\t")
        if f[4] == "*":
            continue
        recs.append(dr.record_of_paf(f, ridx[f[0]], names.index(f[5])))
        at.append(i)
    return recs, at


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return dr.Emulator(ROOT, tmp_path_factory.mktemp("diffstr"))


def test_tag_goldens_are_what_the_reference_prints():
    """tools/make_tags_golden.py in check mode (skipped where the reference's sources, hence oracle/_ref, do not exist)"""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "gdiet_lr_avx")):
        pytest.skip("oracle/_ref not built (no reference sources on this machine)")
    r = subprocess.run(["python3", os.path.join(ROOT, "tools", "make_tags_golden.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_committed_tags_line_up_with_the_golden_sam_and_paf():
    """a row per golden line, same qname / flag / rname / pos; a tag exactly on the lines with an alignment (the counts of the writer);
    --qstrand changes the tag of the 90 reverse-strand PAF lines of hifi_sv and of no other -- i.e. the files are the ones the other
    tests think they are"""
    for kind in SAM_KINDS:
        plain = [l.split("\t") for l in golden_sam(kind)]
        for mode in dr.MODES:
            rows = dr.tag_rows("%s.%s" % (kind, mode))
            assert [r[:4] for r in rows] == [f[:4] for f in plain], (kind, mode)
            assert [bool(r[4]) for r in rows] == [f[5] != "*" for f in plain], (kind, mode)
            assert (sum(1 for r in rows if r[4]), len(rows)) == TAGGED[kind]
    for kind, name, _, _ in PAF_ROWS:
        rows, plain = dr.tag_rows("%s.paf.%s" % (kind, name)), [l.split("\t") for l in golden_paf(kind)]
        assert [(r[0], r[1], r[2]) for r in rows] == [(f[0], f[2], f[4]) for f in plain], (kind, name)
    a, b = dr.tag_rows("hifi_sv.paf.cs"), dr.tag_rows("hifi_sv.paf.qstrand_cs")
    assert all((x[3] != y[3]) == (x[2] == "-") for x, y in zip(a, b)) and sum(x[2] == "-" for x in a) == 90


@pytest.mark.parametrize("kind", SAM_KINDS)
def test_restatement_reproduces_every_committed_sam_tag(kind):
    _, contigs4, _, reads4 = kind_inputs(kind)
    recs, at = sam_records(kind)
    assert len(recs) == TAGGED[kind][0]
    for mode in dr.MODES:
        rows = dr.tag_rows("%s.%s" % (kind, mode))
        for r, i in zip(recs, at):
            assert dr.same_tag(dr.expected(mode, r, reads4, contigs4), rows[i][4]), (kind, mode, rows[i][:4])


@pytest.mark.parametrize("kind,name,mode,qstrand", PAF_ROWS)
def test_restatement_reproduces_every_committed_paf_tag(kind, name, mode, qstrand):
    _, contigs4, _, reads4 = kind_inputs(kind)
    recs, at = paf_records(kind)
    rows = dr.tag_rows("%s.paf.%s" % (kind, name))
    for r, i in zip(recs, at):
        assert dr.same_tag(dr.expected(mode, r, reads4, contigs4, qstrand), rows[i][3]), (kind, name, rows[i][:3])


@pytest.mark.parametrize("kind", SAM_KINDS)
def test_emulated_wavefront_reproduces_every_committed_sam_tag(emu, kind):
    _, contigs4, _, reads4 = kind_inputs(kind)
    recs, at = sam_records(kind)
    for mode in dr.MODES:
        rows = dr.tag_rows("%s.%s" % (kind, mode))
        got = emu.run(recs, reads4, contigs4, mode)
        for g, i in zip(got, at):
            assert dr.same_tag(g, rows[i][4]), (kind, mode, rows[i][:4])


@pytest.mark.parametrize("name,mode", [("qstrand_cs", "cs"), ("qstrand_md", "md")])
def test_emulated_wavefront_under_qstrand(emu, name, mode):
    _, contigs4, _, reads4 = kind_inputs("hifi_sv")
    recs, at = paf_records("hifi_sv")
    rows = dr.tag_rows("hifi_sv.paf." + name)
    got = emu.run(recs, reads4, contigs4, mode, qstrand=True)
    assert len(got) == len(at) and all(dr.same_tag(g, rows[i][3]) for g, i in zip(got, at))
    assert sum(rows[i][3].startswith("#") for i in at) == 90  # the reverse-strand rows are stored as length and sha1
    # ... and cs=long under qstrand, which no golden holds, against the restatement pinned above
    got = emu.run(recs[:40], reads4, contigs4, "cs_long", qstrand=True)
    assert got == [dr.expected("cs_long", r, reads4, contigs4, True) for r in recs[:40]]


@pytest.mark.parametrize("qstrand", [False, True])
@pytest.mark.parametrize("mode", dr.MODES)
def test_emulated_wavefront_on_the_synthetic_set(emu, mode, qstrand):
    contigs4, reads4, recs, notes = dr.synthetic_set()
    got = emu.run(recs, reads4, contigs4, mode, qstrand)
    for g, r, note in zip(got, recs, notes):
        assert g == dr.expected(mode, r, reads4, contigs4, qstrand), (note, mode, qstrand)


def test_synthetic_set_reaches_what_it_was_built_for():
    """the cases by their expected strings: MD's 0 runs and letter endings, every digit count, carried and not carried runs, the N
    operation, upper and lower case N.
    The N operation is the one item no reference output pins: no read set of tests/golden/ gives the reference an N in a CIGAR (its
    presets never splice), so the "~" item of the restatement (diffstr_ref.diff_string, op == 3) rests on a reading of
    LR/format.c:192-196 alone, and the kernel is checked against that reading."""
    contigs4, reads4, recs, notes = dr.synthetic_set()
    exp = {m: dict(zip(notes, (dr.expected(m, r, reads4, contigs4) for r in recs))) for m in dr.MODES}
    md, cs, lg = exp["md"], exp["cs"], exp["cs_long"]
    assert len(set(notes)) == len(notes) < 100
    assert md["record that is one mismatch"][0] == "0" and len(md["record that is one mismatch"]) == 2
    assert md["record ending in a mismatch"][-1] in "ACGT" and md["record ending in a mismatch"].startswith("69")
    assert "0" in [x for x in md["mismatches in lanes 0 and 63 and in adjacent lanes"].replace("A", " ").replace("C", " ").replace("G", " ").replace("T", " ").split()]
    for n in (9, 10, 99, 100, 999, 1000, 9999, 10000):
        assert md["run of %d then a mismatch" % n].startswith("%d" % n) and md["run of %d then a mismatch" % n].endswith("4")
        assert md["run of %d closing the record" % n].endswith("%d" % n) and cs["run of %d closing the record" % n].endswith(":%d" % n)
    carried = "MD run carried across an insertion and two M operations; cs run not carried"
    assert md[carried].split("A")[-1].split("C")[-1].split("G")[-1].split("T")[-1] == "109"  # 39 + 40 + 30 over the insertion and both seams
    assert cs[carried].endswith(":40:30") and lg[carried].count("=") == 4
    assert md["mismatch directly behind a deletion"].count("^") == 1 and "^" in md["deletion of 65"]
    assert "0" == md["mismatch directly behind a deletion"].split("^")[1][5:6]
    first = "N of 2 first, at base 0 of the first contig"
    r0 = recs[notes.index(first)]
    assert (r0["rid"], r0["rs"], r0["cigar"][0]) == (0, 0, (3, 2)) and cs[first].startswith("~") and cs[first][3] == "2"
    assert cs["1M 2N at base 0 of the first contig"][:4] in ["*%s%s~" % (a, b) for a in "acgt" for b in "acgt"]
    assert cs["N of 3 first, at base 0 of the first contig"].startswith("~") and md["N of 3 first, at base 0 of the first contig"] == "10"
    assert cs["N operation"].count("~") == 1 and "~" not in md["N operation"] and "120" in cs["N operation"]
    assert "N" in md["N in the target"] and "n" in cs["N in the query"] and "N" in lg["N on both sides (equal codes)"]
    assert len({r["rs"] % 8 for r in recs}) == 8 and any(r["rev"] for r in recs)
    last = recs[notes.index("ends on the last base of the last contig")]
    assert last["rid"] == len(contigs4) - 1 and last["re"] == len(contigs4[-1])
    offs = np.cumsum([0] + [len(c) for c in contigs4])
    assert offs[1] % 2 == 1 and any(r["rid"] == 1 for r in recs)


def test_host_check_refuses_records_the_kernel_must_not_see(emu):
    """gdd_check_record: the reference's assertions (LR/format.c:156,199,232) as an error, and the kernel's bounds"""
    contigs4, reads4, recs, _ = dr.synthetic_set()
    rl, cl = [len(r) for r in reads4], [len(c) for c in contigs4]
    assert emu.check(recs, rl, cl, True) == -1 and emu.check(recs, rl, cl, False) == -1

    def bad(i, **change):
        out = [dict(r) for r in recs]
        out[i].update(change)
        return out
    k = 5
    r = recs[k]
    assert emu.check(bad(k, qe=r["qe"] - 1), rl, cl, True) == k       # CIGAR query sum != qe - qs
    assert emu.check(bad(k, re=r["re"] + 1), rl, cl, True) == k       # CIGAR target sum != re - rs
    assert emu.check(bad(k, cigar=[(4, 3)] + r["cigar"]), rl, cl, True) == k  # an operation outside 0-3, 7, 8
    assert emu.check(bad(k, rid=3), rl, cl, True) == k                # rid out of range
    assert emu.check(bad(k, rid=-1), rl, cl, True) == k
    n2 = len(contigs4[2])
    assert emu.check(bad(k, rid=2, rs=n2 - 10, re=n2 + 1, cigar=[(0, 1), (2, 10)], qe=r["qs"] + 1), rl, cl, True) == k  # re past the contig
    assert emu.check(bad(k, qs=rl[r["read"]], qe=rl[r["read"]] + 1, cigar=[(0, 1)], re=r["rs"] + 1), rl, cl, True) == k  # qe past the read
    short_n = bad(k, cigar=[(0, 1), (3, 1), (0, 1)], qe=r["qs"] + 2, re=r["rs"] + 3)
    assert emu.check(short_n, rl, cl, True) == k and emu.check(short_n, rl, cl, False) == -1  # cs reads two bases at either end of an N

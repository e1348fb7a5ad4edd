"""CPU: --eqx of the ShortReads variant (mm_update_cigar_eqx, SR/align.c:174-257).
  * tools/make_eqx_golden.py in check mode: the committed fixtures (tests/golden/eqx/) are what the reference prints;
  * the Python restatement (tests/eqx_ref.py) turns every committed plain CIGAR into the one the reference printed under --eqx, from
    windows rebuilt out of the read, the strand, the clips and the reference FASTA -- 0 differences over the four sets;
  * the shared host / device code (map_post.h: gdp_update_extra, then gdp_cigar_eqx in a slot of exactly qlen + tlen words) as a
    stand-alone program under AddressSanitizer and UBSan (tests/emul/eqx_emul.cpp) on the same triples;
  * the fixtures hold every kind of record the rewrite can go wrong on."""
import os
import subprocess

import pytest

from conftest import ROOT
import eqx_ref as er
from fixture_io import golden_paf

# what the reference gave when the fixtures were written (tools/make_eqx_golden.py prints and asserts the same)
COUNTS = {"sr": (1693, 1201, 2000), "sr_var": (861, 539, 1200), "sr_edge": (13, 2, 20)}
COVER = {"sr": ("count_rule", "lead_x", "exact", "diag_x", "shift"), "sr_var": ("lead_x", "exact", "diag_x", "shift"),
         "sr_edge": ("exact", "diag_x", "shift"), "syn": er.KIND_NAMES}

_trip = {}


def trip(kind):
    if kind not in _trip:
        _trip[kind] = er.triples(kind)
    return _trip[kind]


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("eqx") / "eqx_emul")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "genome-on-diet_amd", "csrc"), os.path.join(ROOT, "tests", "emul", "eqx_emul.cpp"), "-o", exe])
    return exe


def test_eqx_goldens_are_what_the_reference_prints():
    """tools/make_eqx_golden.py in check mode (skipped where the reference's sources, hence oracle/_ref, do not exist)"""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "gdiet_sr_avx")):
        pytest.skip("oracle/_ref not built (no reference sources on this machine)")
    r = subprocess.run(["python3", os.path.join(ROOT, "tools", "make_eqx_golden.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("kind", er.KINDS)
def test_fixture_rows_line_up_with_the_plain_sam(kind):
    """a row per plain line with its qname / FLAG / POS; a CIGAR exactly on the mapped lines, none with an M, the same clips and the same
    query and target spans as the plain one; the counts of the writer"""
    plain, rws = [l.split("\t") for l in er.plain_sam(kind)], er.rows(kind + ".sam")
    assert [(f[0], f[1], f[3]) for f in plain] == [tuple(r[:3]) for r in rws]
    for f, r in zip(plain, rws):
        assert (f[5] == "*") == (r[3] == "*") and "M" not in r[3]
        if f[5] != "*":
            a, b = er.parse_cigar(f[5]), er.parse_cigar(r[3])
            span = lambda cg, ops: sum(n for o, n in cg if o in ops)
            assert [x for x in a if x[0] in (1, 2, 3, 4, 5)] == [x for x in b if x[0] in (1, 2, 3, 4, 5)]
            assert span(a, (0,)) == span(b, (7, 8))
    if kind in COUNTS:
        assert (sum(r[3] != "*" for r in rws), sum("X" in r[3] for r in rws), len(rws)) == COUNTS[kind]
    assert er.eqx_sam(kind) != er.plain_sam(kind)


def test_paf_fixture_lines_up_with_the_golden_paf():
    plain, rws = [l.split("\t") for l in golden_paf("sr")], er.rows("sr.paf")
    assert [(f[0], f[2], f[4]) for f in plain] == [tuple(r[:3]) for r in rws]
    sam = {(r[0], er.cigar_text([x for x in er.parse_cigar(r[3]) if x[0] not in (4, 5)])) for r in er.rows("sr.sam")}
    for f, r in zip(plain, rws):
        cg = [x[5:] for x in f if x.startswith("cg:Z:")]
        assert bool(cg) == bool(r[3]) and "M" not in r[3]
        if cg:
            assert [x for x in er.parse_cigar(cg[0]) if x[0] != 0] == [x for x in er.parse_cigar(r[3]) if x[0] not in (7, 8)]
            assert (r[0], r[3]) in sam  # every PAF cg is a SAM CIGAR of that read without its clips


@pytest.mark.parametrize("kind", er.KINDS)
def test_fixtures_hold_every_kind(kind):
    got = er.kinds_of(kind, er.rows(kind + ".sam"))
    for what in COVER[kind]:
        assert got[what] > 0, (kind, what, got)
    if kind == "sr":  # the two count-rule records of the read set: a mismatch-only M labelled =
        by_name = {r[0]: r[3] for r in er.rows("sr.sam")}
        assert by_name["sr_165_c1_18140_-"] == "20S128=20D1=" and by_name["sr_213_c2_195336_+"] == "113=1D34=1I1=" and got["count_rule"] == 2


@pytest.mark.parametrize("kind", er.KINDS)
def test_restatement_reproduces_every_fixture_cigar(kind):
    rws = er.rows(kind + ".sam")
    bad = []
    for i, f, core, head, tail, q, t in trip(kind):
        got = head + er.cigar_text(er.update_cigar_eqx(core, q, t)) + tail
        if got != rws[i][3]:
            bad.append((f[0], got, rws[i][3]))
    assert not bad and len(trip(kind)) == sum(r[3] != "*" for r in rws) > 0, bad[:5]


@pytest.mark.parametrize("kind", er.KINDS)
def test_shared_code_under_the_sanitizers_reproduces_every_fixture_cigar(emul, kind, tmp_path):
    """gdp_update_extra + gdp_cigar_eqx in heap slots of exactly qlen + tlen words: the fixture's CIGARs, a clean exit, nothing on stderr;
    mm_fix_cigar finds nothing left to do on a CIGAR it has already fixed (no shift), and mlen / blen are those of NM and de"""
    inp = str(tmp_path / "in.txt")
    er.write_emul_input(inp, trip(kind))
    r = subprocess.run([emul, inp], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    out = [l.split("\t") for l in r.stdout.rstrip("\n").split("\n")]
    rws = er.rows(kind + ".sam")
    assert len(out) == len(trip(kind))
    for o, (i, f, core, head, tail, q, t) in zip(out, trip(kind)):
        assert head + o[0] + tail == rws[i][3], (f[0], o[0], rws[i][3])
        assert o[1] == o[2] == "0", f[0]
        nm = int(next(x for x in f if x.startswith("NM:i:"))[5:]), int(next(x for x in f if x.startswith("nn:i:"))[5:])
        assert int(o[4]) - int(o[3]) + nm[1] == nm[0], f[0]  # NM = blen - mlen + n_ambi


def test_shared_code_on_cigars_that_grow_to_the_size_of_the_slot(emul, tmp_path):
    """hand-made alignments against the pinned restatement: every base of an M a run of its own (150 operations from one), the same
    around indels and N operations, an M of 8 k + r bases for every r (the eight-base groups and their tails, forwards and backwards),
    runs that end on a group's edge"""
    import numpy as np
    rng = np.random.default_rng(5)
    cases = []

    def case(core, flip):
        ql = sum(n for o, n in core if o in (0, 1))
        tl = sum(n for o, n in core if o in (0, 2, 3))
        q, t = rng.integers(0, 4, ql).astype(np.uint8), rng.integers(0, 4, tl).astype(np.uint8)
        qo = to = 0
        for o, n in core:  # make the M operations equal except where flip says otherwise
            if o == 0:
                d = flip(n)
                q[qo:qo + n] = np.where(d, (t[to:to + n] + 1) % 4, t[to:to + n])
                qo, to = qo + n, to + n
            elif o == 1:
                qo += n
            else:
                to += n
        cases.append((None, None, core, "", "", q, t))
    alt = lambda n: np.arange(n) % 2 == 1
    case([(0, 150)], alt)
    case([(0, 150)], lambda n: np.arange(n) % 2 == 0)
    case([(0, 1), (1, 1), (0, 1), (2, 1), (0, 146), (3, 2), (0, 1)], alt)
    for r in range(0, 18):
        case([(0, 64 + r), (3, 3), (0, 9 + r)], lambda n: rng.integers(0, 3, n) == 0)  # (an N operation: mm_fix_cigar moves none)
        case([(0, 16 + r)], lambda n: (np.arange(n) // 8) % 2 == 1)
        case([(0, 16 + r)], lambda n: np.ones(n, bool))
    inp = str(tmp_path / "in.txt")
    er.write_emul_input(inp, cases)
    r = subprocess.run([emul, inp], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    got = [l.split("\t")[0] for l in r.stdout.rstrip("\n").split("\n")]
    want = [er.cigar_text(er.update_cigar_eqx(c[2], c[5], c[6])) for c in cases]
    assert got == want
    assert want[0].count("=") + want[0].count("X") == 150 and want[-1] == "33="  # (a lone mismatch-only M: the count rule)

"""CPU: read and alignment statistics from BAM records.  The oracle is tests/stats_ref.py, an independent restatement of the section
"Alignment statistics" of include/gdiet_hip.h that books one base at a time.  tests/emul/stats_emul.cpp runs the statements of the kernel
(csrc/stats.h, which uses csrc/pile.h and csrc/cov.h) as a stand-alone program under AddressSanitizer / UBSan on exact-size buffers,
block by block with local memory as a plain array, with the lanes running 0..63 and 63..0.
  * the restatement is checked on records read by eye;
  * the emulator equals the restatement, integer for integer -- the summary and all eleven tables -- on every designed set of
    tests/stats_inputs.py, with the driver's block count and with one block;
  * every kind of bad record is named with its place and reason and contributes nothing;
  * a second, independent oracle reads the committed golden SAM text line by line against the letters of ref.fa.gz; it must equal the
    restatement on the BAM bytes bam_ref makes from the same lines."""
import os
import subprocess

import numpy as np
import pytest

import cov_inputs as ci
import pile_inputs as pi
import pile_ref as pr
import stats_inputs as si
import stats_ref as sr
from conftest import ROOT
from fixture_io import SETS, read_fasta

DESIGNED = si.designed()


def build_emul(tmp_path_factory, tag):
    exe = str(tmp_path_factory.mktemp(tag) / "stats_emul")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "genome-on-diet_amd", "csrc"), os.path.join(ROOT, "tests", "emul", "stats_emul.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory, "stats")


def shaped(flat, opt):
    """the eleven tables, in the order of GDIET_STATS_*, shaped as Stats.finish shapes them"""
    rows = dict(base_cycle=5, qual_cycle=2, subst=5, cmp_cycle=2)
    return {name: np.array(t, np.uint64).reshape(-1, rows[name]) if name in rows else np.array(t, np.uint64) for name, t in zip(sr.TABLES, flat)}


def run_emul(emul, data, ref_lens, ref_codes, tmp_path, blocks=0, **opt):
    """the emulator's output as a stats_ref.Result"""
    opt = dict(si.OPTIONS, **opt)
    p, c = str(tmp_path / "in.recs"), str(tmp_path / "ref.codes")
    with open(p, "wb") as f:
        f.write(data)
    with open(c, "wb") as f:
        f.write(bytes(x for codes in ref_codes for x in codes))
    args = [emul, p, c, opt["excl_flags"], opt["min_mapq"], opt["cycles"], opt["max_len"], opt["max_indel"], opt["bound"], blocks, len(ref_lens)] + list(ref_lens)
    r = subprocess.run([str(x) for x in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = sr.Result()
    out.bad, flat = None, []
    for line in r.stdout.split("\n")[:-1]:
        f = line.split(" ")
        if f[0] == "BAD":
            out.bad = (int(f[1]), (None, "ref", "pos", "op", "ref_end", "qry_end", "cg", "aux", "fields")[int(f[2])])
        elif f[0] == "SUMMARY":
            out.summary = dict(zip(sr.SUMMARY, (int(x) for x in f[1:])))
        elif f[0] == "TABLE":
            assert int(f[1]) == len(flat)
            flat.append([int(x) for x in f[2:]])
    out.tables = shaped(flat, opt)
    return out


def expect(data, ref_lens, ref_codes, **opt):
    opt = dict(si.OPTIONS, **opt)
    opt.pop("bound")
    return sr.stats(data, ref_lens, ref_codes, **opt)


def same(got, want, what=""):
    assert got.summary == want.summary, (what, {k: (got.summary[k], want.summary[k]) for k in sr.SUMMARY if got.summary[k] != want.summary[k]})
    assert sorted(got.tables) == sorted(want.tables) == sorted(sr.TABLES)
    for k in sr.TABLES:
        a, b = got.tables[k], want.tables[k]
        assert a.dtype == b.dtype == np.uint64 and a.shape == b.shape and np.array_equal(a, b), (what, k, np.argwhere(a != b)[:5] if a.shape == b.shape else (a.shape, b.shape))
    assert got.bad == want.bad, (what, got.bad, want.bad)


WANT = {}


def want_of(name):
    """the restatement on a designed set, computed once"""
    if name not in WANT:
        data, lens, codes, opt = si.flat(DESIGNED[name])
        WANT[name] = expect(data, lens, codes, **opt)
    return WANT[name]


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------
def test_restatement_on_records_read_by_eye():
    """three records on contig c0 over its known bases: a forward read 2H 1S 4M whose last base differs, the same bases as a reverse
    secondary alignment (an alignment, not a read), and an unmapped read"""
    r = si.ref_at(0, 10, 4)
    seq = "N" + r[:3] + si.other(r[3])
    recs = [pi.rec(0, 10, [(2, "H"), (1, "S"), (4, "M")], seq=seq, qual=bytes([5, 10, 20, 30, 96]), mapq=7, name=b"a"),
            pi.rec(0, 10, [(2, "H"), (1, "S"), (4, "M")], seq=seq, qual=None, flag=0x110, mapq=9, name=b"b"), pi.rec(-1, -1, [], flag=4, seq="GGCA", qual=bytes([1, 1, 1, 1]), mapq=0, name=b"c")]
    got = sr.stats(b"".join(recs), pi.REF_LENS, [pr.codes_of(s) for s in pi.REF_SEQS], excl_flags=0x600, cycles=5, max_len=4, max_indel=2)
    S, T = got.summary, got.tables
    assert S == dict(records=3, unmapped=1, secondary=1, supplementary=0, primary_mapped=1, reverse=1, excluded_by_flag=1, excluded_by_mapq=0, counted=2, bad=0, duplicate=0, qcfail=0,
                     reads=2, read_bases=9, aligned_bases=8, matches=6, mismatches=2, other_bases=0, ins_events=0, ins_bases=0, del_events=0, del_bases=0, soft_clipped=2, hard_clipped=4,
                     no_seq=0, no_identity=0)
    assert T["read_len"].tolist() == [0, 0, 0, 0, 2] and T["mapq"][7] == T["mapq"][9] == 1 and int(T["mapq"].sum()) == 2 and T["identity"][75] == 2
    code = lambda ch: "ACGTN".index(ch)
    want = np.zeros((6, 5), np.uint64)
    for k, ch in enumerate(seq):  # read a: cycles 2 .. 6, of which 5 and 6 fall on row 5
        want[min(2 + k, 5), code(ch)] += 1
    for k, ch in enumerate("GGCA"):
        want[k, code(ch)] += 1
    assert np.array_equal(T["base_cycle"], want)
    assert T["qual_cycle"].tolist() == [[1, 1], [1, 1], [2, 6], [2, 11], [1, 20], [2, 126]] and T["base_qual"][95] == 1 and T["base_qual"][1] == 4
    # a compares at cycles 3 .. 6 (rows 3 4 5 5), b, reverse with no trailing hard clip, at cycles 3 2 1 0: the mismatch is its cycle 0
    assert T["cmp_cycle"].tolist() == [[1, 1], [1, 0], [1, 0], [2, 0], [1, 0], [2, 1]]
    assert int(T["subst"].sum()) == 8 and T["subst"][code(r[3]), code(si.other(r[3]))] == 2
    a, g = 8, sum(seq.count(c) for c in "CG")  # the N of read a is no base of a
    assert T["gc"][(200 * g + 4) // 8] == 1 and T["gc"][75] >= 1 and int(T["gc"].sum()) == 2 and a == 8


def test_designed_sets_hold_what_they_are_for():
    W = {k: want_of(k) for k in DESIGNED}
    assert all(w.bad is None for w in W.values())
    assert [W["count%d" % n].summary["records"] for n in (1, 3, 4, 5, 9)] == [1, 3, 4, 5, 9] and W["copies"].summary["records"] == 2000
    for n in (1, 63, 64, 65, 5000):
        assert W["run%d" % n].summary["aligned_bases"] == n == W["run%d" % n].summary["read_bases"]
    assert W["run5000_tail8"].tables["base_cycle"][8].sum() == 2 * (5000 - 8) and W["run5000_tail8"].tables["cmp_cycle"][8, 0] == 2 * (5000 - 8)
    assert W["cycles8"].tables["base_cycle"].sum(axis=1).tolist() == [6] * 7 + [4, 2] and W["cycles1"].tables["base_cycle"].sum(axis=1).tolist() == [4, 2]
    assert W["max_len16"].tables["read_len"][15:].tolist() == [2, 4] and W["max_len1"].tables["read_len"].tolist() == [2, 4]
    assert W["max_indel4"].tables["ins_len"].tolist() == [0, 0, 0, 1, 2] == W["max_indel4"].tables["del_len"].tolist() and W["max_indel1"].tables["ins_len"].tolist() == [0, 2]
    nib = W["nibbles"].tables["subst"]
    assert (nib >= 2).all() and int(nib[:, 4].min()) >= 2 * 12  # every reference code against every read code; twelve nibbles are "other"
    assert W["qualities"].tables["base_qual"][[0, 94, 95]].tolist() == [2, 2, 3 * 2 + 10] and W["qualities"].tables["base_qual"][40] == 3 + 3 + 70
    assert W["gc"].tables["gc"][[0, 1, 3, 13, 100]].tolist() == [1, 1, 1, 2, 2] and W["gc"].tables["gc"][50] == 0 and int(W["gc"].tables["gc"].sum()) == 7
    idn = W["identity"]
    assert idn.tables["identity"][[0, 50, 94, 100]].tolist() == [2, 1, 1, 1] and idn.summary["no_identity"] == 3 and idn.summary["no_seq"] == 1 and idn.summary["ins_events"] == 1
    assert W["no_seq"].summary["no_seq"] == 1 and W["placeholder"].summary["counted"] == 3 and W["placeholder"].summary["del_bases"] == 5 + 5 + 40
    assert W["unmapped"].summary["reads"] == 5 and W["unmapped"].summary["counted"] == 0 and W["unmapped"].summary["excluded_by_flag"] == 4
    f = {k: W[k].summary for k in W if k.startswith("flags_")}
    assert f["flags_700_0"]["duplicate"] == 3 and f["flags_700_0"]["qcfail"] == 2 and len({(s["reads"], s["counted"]) for s in f.values()}) == len(f)
    cc = W["clip_cycles"]
    assert cc.summary["hard_clipped"] == 2 * (12 + 4 + 9 + 3 + 6) and cc.summary["soft_clipped"] == 2 * (5 + 3) and cc.tables["base_cycle"][:4].sum() == 4 * 4  # cycles below 4: H_inside on both strands, `trail` forward, `lead` reverse
    for a, b in (("copies_flush", None), ("direct", None), ("direct_all", None)):
        assert DESIGNED[a]["opt"]["bound"] > 0


# ---- the emulator against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_emulator_equals_restatement(name, emul, tmp_path):
    data, lens, codes, opt = si.flat(DESIGNED[name])
    want = want_of(name)
    same(run_emul(emul, data, lens, codes, tmp_path, **opt), want, name)
    same(run_emul(emul, data, lens, codes, tmp_path, blocks=1, **opt), want, name + " (one block)")
    assert want.summary["reads"] + want.summary["counted"] > 0


@pytest.mark.parametrize("name", sorted(ci.BAD))
def test_bad_records(name, emul, tmp_path):
    """named with its place and reason, counted in `bad`, and nothing else: the tables are those of the set without it"""
    recs = pi.counted(9)
    recs.insert(3, ci.BAD[name][0])
    codes = [pr.codes_of(s) for s in pi.REF_SEQS]
    want = expect(b"".join(recs), pi.REF_LENS, codes)
    same(run_emul(emul, b"".join(recs), pi.REF_LENS, codes, tmp_path), want, name)
    assert want.bad == (3, ci.BAD[name][1]) and want.summary["bad"] == 1
    clean = expect(b"".join(recs[:3] + recs[4:]), pi.REF_LENS, codes)
    assert all(np.array_equal(want.tables[k], clean.tables[k]) for k in sr.TABLES)
    assert {k: v for k, v in want.summary.items() if k not in ("records", "bad", "primary_mapped")} == {k: v for k, v in clean.summary.items() if k not in ("records", "bad", "primary_mapped")}


def test_order_freedom(emul, tmp_path):
    recs = [r for k in ("clip_cycles", "qualities", "identity", "flags_700_0", "count9", "long") for r in DESIGNED[k]["recs"]]
    codes = [pr.codes_of(s) for s in pi.REF_SEQS]
    want = expect(b"".join(recs), pi.REF_LENS, codes, cycles=20)
    shuffled = list(recs)
    np.random.default_rng(3).shuffle(shuffled)
    same(run_emul(emul, b"".join(shuffled), pi.REF_LENS, codes, tmp_path, cycles=20, bound=1024, blocks=3), want)


# ---- the second oracle: the reference's own SAM text -----------------------------------------------------------------------------------
GOLDEN_OPT = dict(cycles=150, max_len=20000, max_indel=16)


@pytest.mark.parametrize("kind", ci.GOLDEN)
def test_golden_sam_text_line_by_line(kind, emul, tmp_path):
    """SEQ, QUAL, CIGAR, FLAG and MAPQ of every golden line against the letters of ref.fa.gz equal the restatement on the BAM bytes of
    the same lines; the emulator equals both"""
    recs, names, lens, lines = ci.golden_records(kind)
    fa_names, seqs = read_fasta(os.path.join(SETS[kind][0], "ref.fa.gz"))
    assert fa_names == names
    codes = [pr.codes_of(s) for s in seqs]
    data = b"".join(recs)
    for excl, mapq in ((0x700, 0), (0x800, 1)):
        want = expect(data, lens, codes, excl_flags=excl, min_mapq=mapq, **GOLDEN_OPT)
        S, T = sr.sam_stats(lines, names, seqs, excl_flags=excl, min_mapq=mapq, **GOLDEN_OPT)
        assert want.bad is None and {k: want.summary[k] for k in sr.SAM_COUNTERS} == S and S["counted"] > 0 and S["matches"] > 0
        for k in sr.TABLES:
            assert np.array_equal(want.tables[k], T[k]), (kind, k)
    same(run_emul(emul, data, lens, codes, tmp_path, excl_flags=0x800, min_mapq=1, **GOLDEN_OPT), want, kind)


def test_text_file_from_integers():
    """the layout of the file, on numbers that can be checked by eye"""
    r = si.ref_at(0, 10, 4)
    recs = [pi.rec(0, 10, [(4, "M"), (2, "I")], seq=r[:3] + si.other(r[3]) + "AA", qual=bytes([10, 20, 30, 40, 50, 60]), mapq=5, name=b"a")]
    w = sr.stats(b"".join(recs), pi.REF_LENS, [pr.codes_of(s) for s in pi.REF_SEQS], cycles=2, max_len=8, max_indel=4)
    text = sr.stats_tsv(w.summary, w.tables)
    body = [l for l in text.split("\n") if l and not l.startswith("#")]
    assert "SN\treads:\t1" in body and "SN\terror_rate:\t0.25" in body and "SN\taverage_length:\t6" in body and "SN\taverage_quality:\t35" in body
    assert [l for l in body if l.startswith(("RL", "MQ", "IL", "IDN", "QC", "MPC"))] == ["RL\t6\t1", "QC\t1\t10\t1", "QC\t2\t20\t1", "QC\t3\t45\t4", "MQ\t5\t1", "IL\t2\t1", "MPC\t1\t0\t1", "MPC\t2\t0\t1",
                                                                                          "MPC\t3\t1\t2", "IDN\t60\t1"]
    assert len([l for l in body if l.startswith("SUB")]) == 25 and all(l.split("\t")[0] in ("SN", "RL", "GCF", "GCC", "QC", "BQ", "MQ", "IL", "DL", "SUB", "MPC", "IDN") for l in body)

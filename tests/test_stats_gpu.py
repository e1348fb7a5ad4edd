"""GPU: read and alignment statistics on the device (stats_scatter_kernel) through the kernel-level boundary Stats.add_bam, through
Stats.add, through an attached BgzfWriter and BamSorter, and through tools/map_file.py --stats.  The oracles are the restatement
tests/stats_ref.py, the host emulator tests/emul/stats_emul.cpp, fed the same bytes, and, on the whole path, the line-by-line reading of
the golden SAM text against the letters of ref.fa.gz.  Everything is compared integer for integer: the summary and all eleven tables."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cov_inputs as ci
import cov_ref as cr
import pile_inputs as pi
import pile_ref as pr
import stats_inputs as si
import stats_ref as sr
from conftest import ROOT
from fixture_io import SETS, read_fasta
from test_coverage_gpu import as_cov, mapped, small  # noqa: F401  (fixtures: the mapper over the designed reference, the mapped golden reads)
from test_samopts_gpu import write_fastq
from test_stats import GOLDEN_OPT, build_emul, expect, run_emul, same, want_of

pytestmark = pytest.mark.gpu

DESIGNED = si.designed()
CODES = [pr.codes_of(s) for s in pi.REF_SEQS]


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory, "stats_gpu")


@pytest.fixture(scope="module")
def with_n(pkg, gpu_ctx):
    """a second small mapper whose reference holds an N"""
    names, seqs = pi.REF_N
    m = pkg.Mapper(gpu_ctx, names, seqs, preset="hifi")
    yield m
    m.close()


def as_result(stats):
    out = sr.Result()
    out.summary, out.tables = stats.finish()
    out.bad = None
    return out


def gpu_stats(pkg, m, parts, bound=0, **opt):
    with pkg.Stats(m, _bound=bound, **opt) as stats:
        for p in parts:
            stats.add_bam(p)
        return as_result(stats)


# ---- the kernel-level boundary on the designed sets -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_designed_sets(name, pkg, small, with_n, emul, tmp_path):
    """record counts around the block of four wavefronts, 2 000 copies, operations around the round carry, runs of 1 to 5 000 bases, the
    borders of every table, all sixteen nibbles against all five reference codes, both nibble halves, both strands under hard and soft
    clips, qualities 0 94 95 96 254 and none, records without SEQ, the placeholder, unmapped reads, the filters, GC ties, identities 0, 100
    and none, the flush on a bound and records too heavy for local memory: Stats.add_bam equals the restatement and the emulator"""
    data, lens, codes, opt = si.flat(DESIGNED[name])
    got = gpu_stats(pkg, with_n if DESIGNED[name]["ref"] == "withN" else small, [data], **opt)
    same(got, want_of(name), name)
    same(got, run_emul(emul, data, lens, codes, tmp_path, **opt), name + " (emulator)")


def test_order_freedom(pkg, small):
    """the same records reversed and shuffled, cut into 1, 2 and 7 add_bam calls: identical tables"""
    recs = [r for k in ("clip_cycles", "qualities", "identity", "flags_700_0", "count9", "long", "run5000") for r in DESIGNED[k]["recs"]]
    want = expect(b"".join(recs), pi.REF_LENS, CODES, cycles=20)
    for order, calls, bound in ((recs, 1, 0), (recs[::-1], 1, 0), (recs, 2, 0), (recs[::-1], 7, 1024)):
        cuts = [len(order) * k // calls for k in range(calls + 1)]
        same(gpu_stats(pkg, small, [b"".join(order[a:b]) for a, b in zip(cuts, cuts[1:])], cycles=20, bound=bound), want, (calls, bound))


@pytest.mark.parametrize("name", sorted(ci.BAD))
def test_bad_records(name, pkg, small, emul, tmp_path):
    """GDIET_E_PARAM naming the call's first bad record as the emulator and the restatement name it; the accumulator refuses add and finish
    from then on; a fresh one works, so the context goes on"""
    recs = pi.counted(9)
    recs.insert(3, ci.BAD[name][0])
    data = b"".join(recs)
    assert expect(data, pi.REF_LENS, CODES).bad == run_emul(emul, data, pi.REF_LENS, CODES, tmp_path).bad == (3, ci.BAD[name][1])
    stats = pkg.Stats(small)
    try:
        with pytest.raises(pkg.GdietError, match=r"error -3: .*stats: record 3 of the call: "):
            stats.add_bam(data)
        for call in (lambda: stats.add_bam(recs[0]), stats.finish):
            with pytest.raises(pkg.GdietError, match="error -3: .*used after a bad record"):
                call()
    finally:
        stats.close()
    clean = b"".join(recs[:3] + recs[4:])
    same(gpu_stats(pkg, small, [clean]), expect(clean, pi.REF_LENS, CODES), name + " (fresh)")


def test_options_are_checked_at_open(pkg, small):
    for kw, what in ((dict(cycles=0), "cycles is 0"), (dict(cycles=1025), "cycles is 1025"), (dict(max_len=0), "max_len is 0"), (dict(max_len=(1 << 20) + 1), "max_len is 1048577"),
                     (dict(max_indel=0), "max_indel is 0"), (dict(max_indel=4097), "max_indel is 4097")):
        with pytest.raises(pkg.GdietError, match="error -3: .*" + what):
            pkg.Stats(small, **kw)
    data = b"".join(DESIGNED["long"]["recs"] + DESIGNED["clip_cycles"]["recs"])
    for kw in (dict(cycles=1, max_len=1, max_indel=1), dict(cycles=1024, max_len=1 << 20, max_indel=4096)):  # the ends of the ranges; the second needs 72 KB of local memory
        same(gpu_stats(pkg, small, [data], **kw), expect(data, pi.REF_LENS, CODES, **kw), kw)


def test_read_only_after_finish_and_close_after_the_context(pkg, small):
    data = b"".join(DESIGNED["clip_cycles"]["recs"])
    with pkg.Stats(small) as stats:
        stats.add_bam(data)
        with pytest.raises(pkg.GdietError, match="not finished"):
            stats._check(stats.lib.gdiet_hip_stats_table(stats._h, 0, None, 0))
        first = stats.finish()
        again = stats.finish()  # again: the same figures
        assert first[0] == again[0] == want_of("clip_cycles").summary and all(np.array_equal(first[1][k], again[1][k]) for k in sr.TABLES)
        with pytest.raises(pkg.GdietError, match="read-only"):
            stats.add_bam(data)
        assert stats.lib.gdiet_hip_stats_table(stats._h, 11, None, 0) == -3 and stats.lib.gdiet_hip_stats_table(stats._h, -1, None, 0) == -3
        room = np.zeros(100, np.uint64)
        assert stats.lib.gdiet_hip_stats_table(stats._h, 0, room.ctypes.data, 100) == -3 and not room.any()  # gc holds 101 counters
    with pytest.raises(pkg.GdietError, match="ends inside a record"):
        with pkg.Stats(small) as stats:
            stats.add_bam(data[:-1])
    ctx = pkg.Context(0)
    m = pkg.Mapper(ctx, ["a"], ["ACGT" * 500], preset="hifi")
    stats = pkg.Stats(m)
    stats.add_bam(pi.rec(0, 10, [(30, "M")]))
    m.close()
    ctx.close()
    for call in (lambda: stats.add_bam(pi.rec(0, 10, [(30, "M")])), stats.finish):
        with pytest.raises(pkg.GdietError, match="context has been destroyed"):
            call()
    stats.close()


# ---- the whole path ----------------------------------------------------------------------------------------------------------------------
def golden_want(kind, **opt):
    """the restatement on the golden lines' BAM bytes, checked against the SAM-text oracle"""
    recs, names, lens, lines = ci.golden_records(kind)
    _, seqs = read_fasta(os.path.join(SETS[kind][0], "ref.fa.gz"))
    want = expect(b"".join(recs), lens, [pr.codes_of(s) for s in seqs], **opt)
    S, T = sr.sam_stats(lines, names, seqs, **opt)
    assert {k: want.summary[k] for k in sr.SAM_COUNTERS} == S and all(np.array_equal(want.tables[k], T[k]) for k in sr.TABLES) and S["counted"] > 50 and S["mismatches"] > 0
    return want


@pytest.mark.parametrize("kind", ["hifi_sv", "sr"])
def test_whole_path_three_routes(kind, mapped, pkg, gpu_ctx, tmp_path):
    """the mapped records delivered through Stats.add, through a BgzfWriter with a context, and through a BamSorter, alone and beside an
    attached Coverage and Pileup: all equal the line-by-line reading of the golden SAM text (our records are those lines); the BAM and
    sorted-BAM files are byte-identical with and without the accumulators, whose own results do not change"""
    m, batches = mapped(kind)
    want = golden_want(kind, **GOLDEN_OPT)
    recs, names, lens, lines = ci.golden_records(kind)
    want_cov = cr.coverage(b"".join(recs), lens)
    want_pile = pr.pileup(b"".join(recs), lens)

    def write(path, stats, cov=None, pile=None):
        with pkg.BgzfWriter(path, ctx=gpu_ctx) as w:
            for obj, attach in ((stats, w.set_stats), (cov, w.set_coverage), (pile, w.set_pileup)):
                if obj is not None:
                    attach(obj)
            w.write(m.bam_header("v", ["x"]))
            for b in batches:
                w.write_bam(m, *b.args())
        return open(path, "rb").read()

    def sort(path, stats, cov=None, pile=None):
        os.makedirs(str(tmp_path / "spool"), exist_ok=True)
        s = pkg.BamSorter(path, m, tmp_dir=str(tmp_path / "spool"), version="v", argv=["x"])
        for obj, attach in ((pile, s.set_pileup), (stats, s.set_stats), (cov, s.set_coverage)):
            if obj is not None:
                attach(obj)
        for b in batches:
            s.add(*b.args())
        s.close()
        return open(path, "rb").read(), open(path + ".bai", "rb").read()

    new = lambda: pkg.Stats(m, **GOLDEN_OPT)
    with new() as stats:
        for b in batches:
            stats.add(*b.args())
        same(as_result(stats), want, kind + " (add)")
    plain_w, plain_s = write(str(tmp_path / "w.bam"), None), sort(str(tmp_path / "s.bam"), None)
    with new() as stats:
        assert write(str(tmp_path / "w_stats.bam"), stats) == plain_w
        same(as_result(stats), want, kind + " (writer)")
    with new() as stats:
        assert sort(str(tmp_path / "s_stats.bam"), stats) == plain_s
        same(as_result(stats), want, kind + " (sorter)")
    for route, plain in ((write, plain_w), (sort, plain_s)):
        with new() as stats, pkg.Coverage(m) as cov, pkg.Pileup(m) as pile:
            assert route(str(tmp_path / "all.bam"), stats, cov, pile) == plain
            same(as_result(stats), want, kind + " (all three)")
            assert as_cov(cov).contigs == want_cov.contigs and pile.finish() == want_pile.summary
            assert all(np.array_equal(pile.counts(rid, 0, n), c) for (rid, _, n), c in zip(want_pile.regions, want_pile.counts))


def test_attached_accumulator_that_takes_no_more(mapped, pkg, gpu_ctx, tmp_path):
    """a Stats from another context is refused at attach; a finished one makes the attached calls fail before they encode; a writer
    without a context cannot take one"""
    m, batches = mapped("sr")
    other = pkg.Context(0)
    try:
        m2 = pkg.Mapper(other, ["a"], ["ACGT" * 500], preset="hifi")
        with pkg.Stats(m2) as foreign, pkg.BgzfWriter(str(tmp_path / "f.bam"), ctx=gpu_ctx) as w:
            with pytest.raises(pkg.GdietError, match="one context"):
                w.set_stats(foreign)
            s = pkg.BamSorter(str(tmp_path / "fs.bam"), m, tmp_dir=str(tmp_path), version="v", argv=["x"])
            with pytest.raises(pkg.GdietError, match="one context"):
                s.set_stats(foreign)
            s.close()
        m2.close()
    finally:
        other.close()
    with pkg.Stats(m) as stats:
        stats.finish()
        with pkg.BgzfWriter(str(tmp_path / "x.bam"), ctx=gpu_ctx) as w:
            w.set_stats(stats)
            with pytest.raises(pkg.GdietError, match="read-only"):
                w.write_bam(m, *batches[0].args())
            w.set_stats(None)
            w.write_bam(m, *batches[0].args())
        with pkg.BgzfWriter(str(tmp_path / "y.bam")) as w:
            with pytest.raises(pkg.GdietError, match="one context"):
                w.set_stats(stats)


# ---- the tool --------------------------------------------------------------------------------------------------------------------------
def test_map_file_stats(tmp_path):
    """tools/map_file.py --stats from file to file on sr: sorted BAM beside --coverage and --pileup (attached), SAM (Stats.add on the
    writer thread); the text file is the one stats_ref prints from the golden lines' records; without the option nothing changes"""
    fq = str(tmp_path / "reads.fq")
    write_fastq("sr", fq)
    opt = dict(cycles=150, max_len=300, max_indel=8, min_mapq=1, excl_flags=0x300)
    want = golden_want("sr", **opt)
    base = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "map_file.py"), "--preset", "sr", os.path.join(SETS["sr"][0], "ref.fa.gz"), fq]
    flags = ["--stats-cycles", "150", "--stats-max-len", "300", "--stats-max-indel", "8", "--stats-min-mapq", "1", "--stats-excl-flags", "0x300"]
    for tag, extra, attached in (("sorted", ["--bam", "--sort", "--tmp-dir", str(tmp_path), "--coverage", str(tmp_path / "c"), "--pileup", str(tmp_path / "p")], True), ("sam", [], False)):
        prefix = str(tmp_path / tag)
        r = subprocess.run(base + extra + flags + ["-o", prefix + ".out", "--stats", prefix], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads(r.stdout.strip().split("\n")[-1])
        rep = line["stats"]
        assert rep["attached"] is attached and {k: rep[k] for k in sr.SUMMARY} == want.summary and ("coverage" in line) == ("pileup" in line) == attached
        assert open(prefix + ".stats.tsv").read() == sr.stats_tsv(want.summary, want.tables)
    r = subprocess.run(base + ["-o", str(tmp_path / "plain.sam")], capture_output=True, text=True)  # without the flag: no key, the same SAM
    assert r.returncode == 0 and "stats" not in json.loads(r.stdout.strip().split("\n")[-1])
    assert open(str(tmp_path / "plain.sam"), "rb").read() == open(str(tmp_path / "sam.out"), "rb").read()

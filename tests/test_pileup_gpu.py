"""GPU: base counts per position and variant sites on the device (pile_scatter_kernel, pile_call_kernel, hipCUB's exclusive sum in chunks,
pile_site_kernel) through the kernel-level boundary Pileup.add_bam, through Pileup.add, through an attached BgzfWriter and BamSorter, and
through tools/map_file.py --pileup.  The oracles are the restatement tests/pile_ref.py, the host emulator tests/emul/pile_emul.cpp, fed the
same bytes, and, on the whole path, the base-by-base reading of the golden SAM text.  Everything is compared integer for integer: the
summary, all eight counters of every position, the consensus bytes and the site rows."""
import ctypes as C
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
from conftest import ROOT
from fixture_io import SETS, read_fasta
from test_coverage_gpu import _hip_runtime, as_cov, mapped, small  # noqa: F401  (fixtures: the mapper over the designed reference, the mapped golden reads)
from test_pileup import REF_CODES, Got, build_emul, expect, golden_regions, run_emul, same
from test_samopts_gpu import write_fastq

pytestmark = pytest.mark.gpu

DESIGNED = pi.designed()


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory, "pile_gpu")


def as_got(pile, chunk=0, min_depth=8, min_alt=2, frac=(1, 5), cons_depth=1):
    """what a Pileup says, finished, as a test_pileup.Got"""
    out = Got()
    out.summary, out.bad = pile.finish(chunk), None
    out.counts = [pile.counts(rid, beg, end) for rid, beg, end in pile.regions]
    out.cons = [pile.consensus(i, cons_depth) for i in range(len(pile.regions))]
    out.sites = [(int(r["rid"]), int(r["pos"]), int(r["ref"]), int(r["alt"]), int(r["depth"]), tuple(int(x) for x in r["cnt"])) for r in pile.sites(min_depth, min_alt, frac)]
    return out


def gpu_pile(pkg, m, parts, chunk=0, regions=None, excl_flags=0x704, min_mapq=0, min_baseq=0, **calls):
    with pkg.Pileup(m, regions=regions, excl_flags=excl_flags, min_mapq=min_mapq, min_baseq=min_baseq) as pile:
        for p in parts:
            pile.add_bam(p)
        return as_got(pile, chunk, **calls)


# ---- the kernel-level boundary on the designed sets -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_designed_sets(name, pkg, small, emul, tmp_path):
    """record counts around the blocks of four wavefronts, operations around the round carry with every code, runs of 1 to 5 000 bases over
    the 64 lanes, all sixteen nibble codes, qualities at the threshold, both nibble halves, every placement of an I, D and N across region
    borders, region lists, contention, strands, the placeholder, coverage's filter and quality records, records without SEQ, the call set:
    Pileup.add_bam equals the restatement and the emulator, with the scan cut every 7 positions"""
    v = DESIGNED[name]
    data = b"".join(v["recs"])
    kw = dict(regions=v["regions"], min_baseq=v["min_baseq"], **pi.CALL_OPT)
    got = gpu_pile(pkg, small, [data], chunk=7, cons_depth=pi.CALL_OPT["min_depth"], **kw)
    same(got, expect(data, pi.REF_LENS, REF_CODES, cons_depth=pi.CALL_OPT["min_depth"], **kw), name)
    same(got, run_emul(emul, data, pi.REF_LENS, REF_CODES, tmp_path, chunk=7, **kw), name + " (emulator)")


def test_reference_n(pkg, gpu_ctx):
    """a site at a reference N, over a second small mapper whose reference holds one: every allele is "other" there"""
    names, seqs = pi.REF_N
    recs, kinds = pi.call_set_n()
    m = pkg.Mapper(gpu_ctx, names, seqs, preset="hifi")
    try:
        got = gpu_pile(pkg, m, [b"".join(recs)], **pi.CALL_OPT)
    finally:
        m.close()
    same(got, expect(b"".join(recs), [len(seqs[0])], [pr.codes_of(seqs[0])], **pi.CALL_OPT), "ref N")
    assert [r[:5] for r in got.sites] == [(0, 50, 4, 0, 6)]


@pytest.mark.parametrize("chunk", (1, 256, 0))
def test_chunks(chunk, pkg, small):
    """sites on both sides of every border of the scan's chunk; thousands of them, in position order"""
    data = b"".join(ci.border_set() + pi.call_set()[0] + pi.counted(257))
    kw = dict(min_depth=1, min_alt=1, frac=(1, 10))
    got = gpu_pile(pkg, small, [data], chunk=chunk, **kw)
    same(got, expect(data, pi.REF_LENS, REF_CODES, **kw), chunk)
    assert len(got.sites) > 3000


@pytest.mark.parametrize("excl,mapq", ci.FILTERS)
def test_filters(excl, mapq, pkg, small):
    data = b"".join(ci.filter_set() + pi.no_seq_recs())
    kw = dict(excl_flags=excl, min_mapq=mapq, min_depth=1, min_alt=1)
    same(gpu_pile(pkg, small, [data], **kw), expect(data, pi.REF_LENS, REF_CODES, **kw), (excl, mapq))


@pytest.mark.parametrize("name", sorted(ci.BAD))
def test_bad_records(name, pkg, small, emul, tmp_path):
    """GDIET_E_PARAM naming the call's first bad record as the emulator and the restatement name it; the accumulator refuses add and finish
    from then on; a fresh one works, so the context goes on"""
    recs = pi.counted(9)
    recs.insert(3, ci.BAD[name][0])
    data = b"".join(recs)
    assert expect(data, pi.REF_LENS, REF_CODES).bad == run_emul(emul, data, pi.REF_LENS, REF_CODES, tmp_path).bad == (3, ci.BAD[name][1])
    pile = pkg.Pileup(small)
    try:
        with pytest.raises(pkg.GdietError, match=r"error -3: .*record 3 of the call: "):
            pile.add_bam(data)
        for call in (lambda: pile.add_bam(recs[0]), pile.finish):
            with pytest.raises(pkg.GdietError, match="error -3: .*used after a bad record"):
                call()
    finally:
        pile.close()
    clean = b"".join(recs[:3] + recs[4:])
    same(gpu_pile(pkg, small, [clean]), expect(clean, pi.REF_LENS, REF_CODES), name + " (fresh)")


def test_regions_are_refused_at_open(pkg, small):
    for regions, what in (([(0, 0, 10), (0, 5, 5)], "region 1 .*is empty"), ([(0, 0, 301)], "region 0 .*past its contig"), ([(5, 0, 1)], "region 0 .*past its contig"),
                          ([(2, 0, 5), (0, 0, 5)], "region 1 .*not sorted"), ([(0, 5, 9), (0, 2, 4)], "region 1 .*not sorted"), ([(0, 0, 10), (0, 9, 12)], "region 1 .*overlaps")):
        assert pr.check_regions(regions, pi.REF_LENS) is not None
        with pytest.raises(pkg.GdietError, match="error -3: .*" + what):
            pkg.Pileup(small, regions=regions)
    with pkg.Pileup(small, regions=[(0, 0, 300), (1, 0, 1), (2, 5, 9), (2, 9, 12)]) as pile:  # abutting regions are allowed
        assert pile.finish()["records"] == 0


def test_calls_after_finish(pkg, small):
    data = b"".join(pi.border_recs())
    want = expect(data, pi.REF_LENS, REF_CODES, regions=pi.BORDER_REGIONS)
    with pkg.Pileup(small, regions=pi.BORDER_REGIONS) as pile:
        pile.add_bam(data)
        for call in (lambda: pile.counts(3, 100, 101), lambda: pile.consensus(0), pile.sites):
            with pytest.raises(pkg.GdietError, match="not finished"):
                call()
        assert pile.finish() == want.summary == pile.finish()  # again: the same figures
        with pytest.raises(pkg.GdietError, match="read-only"):
            pile.add_bam(data)
        assert np.array_equal(pile.counts(3, 103, 110), want.counts[0][3:]) and pile.counts(3, 110, 110).shape == (0, 8) and np.array_equal(pile.counts(3, 130, 131), want.counts[2])
        for rid, beg, end in ((3, 105, 115), (3, 99, 101), (3, 120, 121), (0, 0, 1), (9, 0, 1), (3, 105, 104)):  # across two abutting regions, outside, in a gap, no region
            with pytest.raises(pkg.GdietError, match="inside one region"):
                pile.counts(rid, beg, end)
        with pytest.raises(pkg.GdietError, match="den == 0"):
            pile.sites(frac=(1, 0))
        n = pile.lib.gdiet_hip_pile_sites(pile._h, 1, 1, 1, 10, None, 0)
        rows = np.zeros(n, pkg.pileup.SITE)
        assert n > 2 and pile.lib.gdiet_hip_pile_sites(pile._h, 1, 1, 1, 10, rows.ctypes.data, n - 1) == -3  # too little room: refused, with the number in the text
    with pytest.raises(pkg.GdietError, match="ends inside a record"):
        with pkg.Pileup(small) as pile:
            pile.add_bam(data[:-1])


def test_order_freedom(pkg, small):
    """the same records shuffled, and cut into 1, 2 and 7 add_bam calls: identical arrays"""
    recs = DESIGNED["borders"]["recs"] + DESIGNED["clips"]["recs"] + DESIGNED["placeholder"]["recs"] + DESIGNED["calls"]["recs"] + DESIGNED["long"]["recs"]
    want = expect(b"".join(recs), pi.REF_LENS, REF_CODES, min_baseq=10, **pi.CALL_OPT)
    for seed, calls in ((None, 1), (1, 2), (2, 7)):
        order = list(recs)
        if seed is not None:
            np.random.default_rng(seed).shuffle(order)
        cuts = [len(order) * k // calls for k in range(calls + 1)]
        same(gpu_pile(pkg, small, [b"".join(order[a:b]) for a, b in zip(cuts, cuts[1:])], chunk=256, min_baseq=10, **pi.CALL_OPT), want, (seed, calls))


# ---- the whole path ----------------------------------------------------------------------------------------------------------------------
CALLS = dict(min_depth=2, min_alt=2, frac=(1, 5))


@pytest.mark.parametrize("kind", ["hifi_sv", "sr"])
def test_whole_path_three_routes(kind, mapped, pkg, gpu_ctx, tmp_path):
    """the mapped records delivered through Pileup.add, through a BgzfWriter with a context, and through a BamSorter: all three equal the
    base-by-base reading of the golden SAM text (our records are those lines) and the restatement on the golden lines' BAM bytes, over a
    region list; the BAM and sorted-BAM files are byte-identical with and without a pileup, and with a pileup and a coverage accumulator
    attached together, whose coverage still equals cov_ref"""
    m, batches = mapped(kind)
    recs, names, lens, lines = ci.golden_records(kind)
    _, seqs = read_fasta(os.path.join(SETS[kind][0], "ref.fa.gz"))
    regions = golden_regions(lens)
    want = expect(b"".join(recs), lens, [pr.codes_of(s) for s in seqs], regions=regions, min_baseq=40, **CALLS)
    counts, skipped, counted = pr.sam_pileup(lines, names, lens, regions, min_baseq=40)
    assert all(a.tolist() == b for a, b in zip(want.counts, counts)) and want.summary["counted"] == counted > 50 and len(want.sites) > 0
    want_cov = cr.coverage(b"".join(recs), lens)

    def write(path, pile, cov=None):
        with pkg.BgzfWriter(path, ctx=gpu_ctx) as w:
            if pile is not None:
                w.set_pileup(pile)
            if cov is not None:
                w.set_coverage(cov)
            w.write(m.bam_header("v", ["x"]))
            for b in batches:
                w.write_bam(m, *b.args())
        return open(path, "rb").read()

    def sort(path, pile, cov=None):
        os.makedirs(str(tmp_path / "spool"), exist_ok=True)
        s = pkg.BamSorter(path, m, tmp_dir=str(tmp_path / "spool"), version="v", argv=["x"])
        if pile is not None:
            s.set_pileup(pile)
        if cov is not None:
            s.set_coverage(cov)
        for b in batches:
            s.add(*b.args())
        s.close()
        return open(path, "rb").read(), open(path + ".bai", "rb").read()

    new = lambda: pkg.Pileup(m, regions=regions, min_baseq=40)
    with new() as pile:
        for b in batches:
            pile.add(*b.args())
        same(as_got(pile, **CALLS), want, kind + " (add)")
    plain_w, plain_s = write(str(tmp_path / "w.bam"), None), sort(str(tmp_path / "s.bam"), None)
    with new() as pile:
        assert write(str(tmp_path / "w_pile.bam"), pile) == plain_w
        same(as_got(pile, **CALLS), want, kind + " (writer)")
    with new() as pile:
        assert sort(str(tmp_path / "s_pile.bam"), pile) == plain_s
        same(as_got(pile, **CALLS), want, kind + " (sorter)")
    with new() as pile, pkg.Coverage(m) as cov:
        assert write(str(tmp_path / "w_both.bam"), pile, cov) == plain_w
        same(as_got(pile, **CALLS), want, kind + " (writer, both)")
        got_cov = as_cov(cov)
        assert got_cov.summary == want_cov.summary and got_cov.contigs == want_cov.contigs and all(np.array_equal(a, b) for a, b in zip(got_cov.depth, want_cov.depth))
    with new() as pile, pkg.Coverage(m) as cov:
        assert sort(str(tmp_path / "s_both.bam"), pile, cov) == plain_s
        same(as_got(pile, **CALLS), want, kind + " (sorter, both)")
        assert as_cov(cov).contigs == want_cov.contigs


def test_attached_accumulator_that_takes_no_more(mapped, pkg, gpu_ctx, tmp_path):
    """a finished accumulator makes the attached calls fail before they encode; a writer without a context cannot take one"""
    m, batches = mapped("sr")
    with pkg.Pileup(m) as pile:
        pile.finish()
        with pkg.BgzfWriter(str(tmp_path / "x.bam"), ctx=gpu_ctx) as w:
            w.set_pileup(pile)
            with pytest.raises(pkg.GdietError, match="read-only"):
                w.write_bam(m, *batches[0].args())
            w.set_pileup(None)
            w.write_bam(m, *batches[0].args())
        with pkg.BgzfWriter(str(tmp_path / "y.bam")) as w:
            with pytest.raises(pkg.GdietError, match="one context"):
                w.set_pileup(pile)


# ---- the tool --------------------------------------------------------------------------------------------------------------------------
def test_map_file_pileup(tmp_path):
    """tools/map_file.py --pileup from file to file on sr: sorted BAM with a region file (attached), SAM without one (Pileup.add on the
    writer thread); the two text files are the ones pile_ref prints from the golden lines' records"""
    fq = str(tmp_path / "reads.fq")
    write_fastq("sr", fq)
    recs, names, lens, lines = ci.golden_records("sr")
    _, seqs = read_fasta(os.path.join(SETS["sr"][0], "ref.fa.gz"))
    codes = [pr.codes_of(s) for s in seqs]
    regions = golden_regions(lens)
    bed = str(tmp_path / "regions.bed")
    with open(bed, "w") as f:
        f.write("#comment\n" + "".join("%s\t%d\t%d\n" % (names[rid], beg, end) for rid, beg, end in regions))
    base = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "map_file.py"), "--preset", "sr", os.path.join(SETS["sr"][0], "ref.fa.gz"), fq]
    calls = ["--pile-min-depth", "3", "--pile-min-alt", "2", "--pile-frac", "1/4", "--pile-min-baseq", "40"]
    for tag, extra, attached, reg in (("sorted", ["--bam", "--sort", "--tmp-dir", str(tmp_path), "--pile-regions", bed], True, regions), ("sam", [], False, None)):
        prefix = str(tmp_path / tag)
        r = subprocess.run(base + extra + calls + ["-o", prefix + ".out", "--pileup", prefix], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        want = pr.pileup(b"".join(recs), lens, reg, min_baseq=40)
        rep = json.loads(r.stdout.strip().split("\n")[-1])["pileup"]
        assert rep["attached"] is attached and {k: rep[k] for k in pr.SUMMARY} == want.summary and rep["regions"] == len(want.regions)
        rows = pr.sites(want, codes, min_depth=3, min_alt=2, frac=(1, 4))
        assert len(rows) > 0 and open(prefix + ".pileup.tsv").read() == pr.pileup_tsv(rows, names)
        assert open(prefix + ".consensus.fa").read() == pr.consensus_fa(want, names, 3)
    r = subprocess.run(base + ["-o", str(tmp_path / "plain.sam")], capture_output=True, text=True)  # without the flag: no key, the same SAM
    assert r.returncode == 0 and "pileup" not in json.loads(r.stdout.strip().split("\n")[-1])
    assert open(str(tmp_path / "plain.sam"), "rb").read() == open(str(tmp_path / "sam.out"), "rb").read()


# ---- memory ----------------------------------------------------------------------------------------------------------------------------
def test_nothing_is_left_behind(pkg, gpu_ctx, small):
    """open / add / finish / close in rounds, refused calls among them: hipMemGetInfo is back where it started and the stream-ordered pool
    holds nothing more; an accumulator that outlives its context has lost its arrays and takes nothing but close"""
    hip = _hip_runtime()
    pool = C.c_void_p()
    assert hip.hipDeviceGetDefaultMemPool(C.byref(pool), 0) == 0

    def used():
        assert hip.hipDeviceSynchronize() == 0
        v, free, total = C.c_uint64(), C.c_size_t(), C.c_size_t()
        assert hip.hipMemPoolGetAttribute(pool, 7, C.byref(v)) == 0  # hipMemPoolAttrUsedMemCurrent
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return v.value, free.value

    data = b"".join(ci.border_set() + pi.call_set()[0])
    bad = b"".join(pi.counted(3) + [ci.BAD["op9"][0]])

    def round_(refusals):
        if refusals:
            with pytest.raises(pkg.GdietError):
                pkg.Pileup(small, regions=[(0, 5, 5)])
        with pkg.Pileup(small, regions=None if refusals else pi.BORDER_REGIONS) as pile:
            pile.add_bam(data)
            if refusals:
                with pytest.raises(pkg.GdietError):
                    pile.add_bam(data[:-3])
                with pytest.raises(pkg.GdietError):
                    pile.add_bam(bad)
                with pytest.raises(pkg.GdietError):
                    pile.finish()
            else:
                pile.finish(chunk=256)
                pile.counts(4, 0, 6000), pile.consensus(4), pile.sites(1, 1, (1, 10))
                with pytest.raises(pkg.GdietError):
                    pile.counts(0, 0, 1)

    round_(False), round_(True)  # warm-up: the lane's stream, the pool's first pages
    first = used()
    for k in range(4):
        round_(k % 2 == 1)
    assert used() == first

    def own_context(with_pile):
        """a context of its own with a mapper, destroyed -- with an accumulator still open"""
        ctx = pkg.Context(0)
        m = pkg.Mapper(ctx, ["a"], ["ACGT" * 500], preset="hifi")
        pile = pkg.Pileup(m) if with_pile else None
        if pile is not None:
            pile.add_bam(pi.rec(0, 10, [(30, "M")]))
        m.close()
        ctx.close()
        if pile is not None:
            with pytest.raises(pkg.GdietError, match="context has been destroyed"):
                pile.add_bam(pi.rec(0, 10, [(30, "M")]))
            pile.close()

    own_context(False)  # warm-up: what the first further context of a process costs once
    first = used()
    own_context(False)
    assert used() == first
    own_context(True)
    assert used() == first

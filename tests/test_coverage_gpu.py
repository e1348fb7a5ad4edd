"""GPU: coverage and depth accumulated on the device (cov_scatter_kernel, hipCUB's inclusive sum in chunks, cov_window_kernel) through the
kernel-level boundary Coverage.add_bam, through Coverage.add, through an attached BgzfWriter and BamSorter, and through
tools/map_file.py --coverage.  The oracles are the restatement tests/cov_ref.py, the host emulator tests/emul/cov_emul.cpp, fed the same
bytes, and, on the whole path, the brute-force reading of the golden SAM text.  Everything is compared integer for integer: the summary,
the per-contig counters, the windows and the depth of every position of every contig."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cov_inputs as ci
import cov_ref as cr
from conftest import ROOT
from fixture_io import OVERRIDES, SETS, read_fasta, reads_of
from test_bam_sort_gpu import Slice
from test_coverage import build_emul, run_emul, same
from test_samopts_gpu import write_fastq

pytestmark = pytest.mark.gpu

DESIGNED = ci.designed()


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory, "cov_gpu")


@pytest.fixture(scope="module")
def small(pkg, gpu_ctx):
    """a mapper over the designed reference: five random contigs of cov_inputs.REF_LENS bases (one of them a single base)"""
    rng = np.random.default_rng(5)
    m = pkg.Mapper(gpu_ctx, ci.REFS, ["".join("ACGT"[c] for c in rng.integers(0, 4, n)) for n in ci.REF_LENS], preset="hifi")
    assert [int(x) for x in m.index_info()["lens"]] == ci.REF_LENS
    yield m
    m.close()


def as_cov(cov, chunk=0):
    """what a finished Coverage says, as a cov_ref.Cov: every counter, every window, the depth of every position"""
    contigs, summary = cov.finish(chunk)
    out = cr.Cov()
    out.summary, out.bad = summary, None
    out.contigs = [dict((k, int(c[k])) for k in cr.CONTIG) for c in contigs]
    out.depth = [cov.depth(rid, 0, n) for rid, n in enumerate(cov.lens)]
    out.windows = [cov.windows(rid) for rid in range(len(cov.lens))] if cov.window else None
    return out


def gpu_cov(pkg, m, parts, chunk=0, **kw):
    with pkg.Coverage(m, **kw) as cov:
        for p in parts:
            cov.add_bam(p)
        return as_cov(cov, chunk)


# ---- the kernel-level boundary on the designed sets -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_designed_sets(name, pkg, small, emul, tmp_path):
    """record counts around the blocks of four wavefronts, operations around the round carry of both scans with every code, the edges of
    the difference array, contention, the cooperative quality loop, qualities, the placeholder with CG:B:I, the filters' records, runs
    across chunk borders: Coverage.add_bam equals the restatement and the emulator"""
    data = b"".join(DESIGNED[name])
    want = cr.coverage(data, ci.REF_LENS, window=64)
    got = gpu_cov(pkg, small, [data], chunk=7, window=64)
    same(got, want, name)
    same(got, run_emul(emul, data, ci.REF_LENS, tmp_path, window=64, chunk=7), name + " (emulator)")


def test_edges_of_the_difference_array(pkg, small):
    """a run that ends exactly at its contig's end puts its -1 on slot 0 of the next contig, or on the array's last slot: the next
    contig's position 0 is what its own reads make it, covered or not"""
    for covered in (True, False):
        got = gpu_cov(pkg, small, [b"".join(ci.edge_set(covered))])
        assert list(got.depth[0][-21:]) == [0] + [1] * 20 and list(got.depth[0][:4]) == [1, 1, 1, 0]
        assert list(got.depth[1]) == [int(covered)] and got.contigs[1]["cov_bases"] == int(covered)
        assert list(got.depth[2]) == [1] * ci.REF_LENS[2] and list(got.depth[4][-10:]) == [0] + [1] * 9
        assert got.summary["counted"] == 4 + covered and got.summary["bad"] == 0 and got.summary["records"] == 6 + covered


@pytest.mark.parametrize("name", sorted(ci.BAD))
def test_bad_records(name, pkg, small, emul, tmp_path):
    """GDIET_E_PARAM naming the call's first bad record as the emulator and the restatement name it; the accumulator refuses add and
    finish from then on; a fresh one works"""
    recs = ci.with_bad(name)
    data = b"".join(recs)
    want = cr.coverage(data, ci.REF_LENS)
    e = run_emul(emul, data, ci.REF_LENS, tmp_path)
    assert want.bad == e.bad == (3, ci.BAD[name][1])
    cov = pkg.Coverage(small)
    try:
        with pytest.raises(pkg.GdietError, match=r"error -3: .*record 3 of the call: ") as err:
            cov.add_bam(data)
        for call in (lambda: cov.add_bam(recs[0]), cov.finish):
            with pytest.raises(pkg.GdietError, match="error -3: .*used after a bad record"):
                call()
    finally:
        cov.close()
    assert "record 3 of the call" in str(err.value)
    clean = recs[:3] + recs[4:]
    same(gpu_cov(pkg, small, [b"".join(clean)]), cr.coverage(b"".join(clean), ci.REF_LENS), name + " (fresh)")


def test_finish_is_refused_after_a_bad_record(pkg, small):
    """after a bad record finish is refused at the C boundary too (GDIET_E_PARAM) and hands nothing out; what the other records of the
    call would have given is read from a fresh accumulator in test_bad_records"""
    recs = ci.with_bad("op9")
    cov = pkg.Coverage(small)
    try:
        with pytest.raises(pkg.GdietError):
            cov.add_bam(b"".join(recs))
        contigs = np.zeros(len(ci.REF_LENS), pkg.coverage.CONTIG)
        summary = (C.c_uint64 * 10)()
        assert cov.lib.gdiet_hip_cov_finish_chunked(cov._h, 0, contigs.ctypes.data, summary) == -3  # refused: nothing is handed out
        assert not contigs["n_reads"].any() and not any(summary)
    finally:
        cov.close()


@pytest.mark.parametrize("excl,mapq", ci.FILTERS)
def test_filters(excl, mapq, pkg, small):
    data = b"".join(ci.filter_set())
    same(gpu_cov(pkg, small, [data], excl_flags=excl, min_mapq=mapq), cr.coverage(data, ci.REF_LENS, excl_flags=excl, min_mapq=mapq), (excl, mapq))


@pytest.mark.parametrize("window", ci.WINDOWS)
def test_chunks_and_windows(window, pkg, small):
    """chunks of 1, 7 and 256 slots and one larger than the array, on a set with a run across every chunk border; windows of 1, 63, 64,
    65, larger than a contig, dividing one and dividing none: the results are identical"""
    data = b"".join(ci.border_set())
    want = cr.coverage(data, ci.REF_LENS, window=window)
    for chunk in ci.CHUNKS if window in (1, 64) else (7, 0):
        same(gpu_cov(pkg, small, [data], chunk=chunk, window=window), want, (window, chunk))


def test_windows_and_depth_calls(pkg, small):
    data = b"".join(ci.border_set())
    want = cr.coverage(data, ci.REF_LENS)
    with pkg.Coverage(small) as cov:
        cov.add_bam(data)
        with pytest.raises(pkg.GdietError, match="not finished"):
            cov.depth(0, 0, 1)
        contigs, _ = cov.finish()
        assert [int(c["cov_bases"]) for c in contigs] == [c["cov_bases"] for c in want.contigs]  # (the internal window)
        assert cov.finish()[1] == want.summary  # again: the same figures
        with pytest.raises(pkg.GdietError, match="without a window"):
            cov.windows(0)
        with pytest.raises(pkg.GdietError, match="read-only"):
            cov.add_bam(data)
        assert np.array_equal(cov.depth(4, 5990, 6000), want.depth[4][5990:]) and len(cov.depth(4, 6000, 6000)) == 0 and np.array_equal(cov.depth(1, 0, 1), want.depth[1])
        for rid, beg, end in ((4, 5990, 6001), (5, 0, 1), (0, 2, 1)):
            with pytest.raises(pkg.GdietError, match="outside the contig"):
                cov.depth(rid, beg, end)
    with pytest.raises(pkg.GdietError, match="ends inside a record"):
        with pkg.Coverage(small) as cov:
            cov.add_bam(data[:-1])


def test_order_freedom(pkg, small):
    """the same records shuffled, and split into 1, 2 and 7 add_bam calls: identical integers"""
    recs = DESIGNED["borders"] + DESIGNED["quality"] + DESIGNED["placeholder"] + DESIGNED["long_quality_run"]
    want = cr.coverage(b"".join(recs), ci.REF_LENS, window=65)
    for seed, calls in ((None, 1), (1, 2), (2, 7)):
        order = list(recs)
        if seed is not None:
            np.random.default_rng(seed).shuffle(order)
        cuts = [len(order) * k // calls for k in range(calls + 1)]
        same(gpu_cov(pkg, small, [b"".join(order[a:b]) for a, b in zip(cuts, cuts[1:])], chunk=256, window=65), want, (seed, calls))


# ---- the whole path ----------------------------------------------------------------------------------------------------------------------
N_BATCHES = 3
_mapped = {}


@pytest.fixture(scope="module")
def mapped(pkg, gpu_ctx):
    """kind -> (mapper, batches): the kind's reads mapped once with the committed options, cut into batches"""
    def get(kind):
        if kind not in _mapped:
            base, _, preset = SETS[kind]
            names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
            reads = reads_of(kind)
            m = pkg.Mapper(gpu_ctx, names, seqs, preset=preset, **OVERRIDES.get(kind, {}))
            res = m.map([r[1] for r in reads])
            cuts = [len(reads) * k // N_BATCHES for k in range(N_BATCHES + 1)]
            _mapped[kind] = (m, [Slice(pkg, reads, res, a, b) for a, b in zip(cuts, cuts[1:])], res)
        return _mapped[kind][:2]
    yield get
    for v in _mapped.values():
        v[0].close()
    _mapped.clear()


@pytest.mark.parametrize("kind", ["hifi_sv", "sr"])
def test_whole_path_three_routes(kind, mapped, pkg, gpu_ctx, tmp_path):
    """the mapped records delivered through Coverage.add, through a BgzfWriter with a context followed by write_bam, and through a
    BamSorter followed by add / close: all three equal the brute-force reading of the golden SAM text (our records are those lines) and
    the restatement on the golden lines' BAM bytes; the BAM files written with an accumulator attached are byte-identical to the ones
    written without"""
    m, batches = mapped(kind)
    recs, names, lens, lines = ci.golden_records(kind)
    assert names == m.names
    depth, contigs, counted = cr.sam_depth(lines, names, lens)
    want = cr.coverage(b"".join(recs), lens, window=1000)
    assert want.contigs == contigs and all(np.array_equal(a, b) for a, b in zip(want.depth, depth)) and want.summary["counted"] == counted > 50

    def write(path, cov):
        with pkg.BgzfWriter(path, ctx=gpu_ctx) as w:
            if cov is not None:
                w.set_coverage(cov)
            w.write(m.bam_header("v", ["x"]))
            for b in batches:
                w.write_bam(m, *b.args())
        return open(path, "rb").read()

    def sort(path, cov):
        os.makedirs(str(tmp_path / "spool"), exist_ok=True)
        s = pkg.BamSorter(path, m, tmp_dir=str(tmp_path / "spool"), version="v", argv=["x"])
        if cov is not None:
            s.set_coverage(cov)
        for b in batches:
            s.add(*b.args())
        s.close()
        return open(path, "rb").read(), open(path + ".bai", "rb").read()

    with pkg.Coverage(m, window=1000) as cov:
        for b in batches:
            cov.add(*b.args())
        same(as_cov(cov), want, kind + " (add)")
    with pkg.Coverage(m, window=1000) as cov:
        attached = write(str(tmp_path / "w_cov.bam"), cov)
        same(as_cov(cov), want, kind + " (writer)")
    assert attached == write(str(tmp_path / "w.bam"), None) and len(gzip.decompress(attached)) > sum(len(r) for r in recs)
    with pkg.Coverage(m, window=1000) as cov:
        attached = sort(str(tmp_path / "s_cov.bam"), cov)
        same(as_cov(cov), want, kind + " (sorter)")
    assert attached == sort(str(tmp_path / "s.bam"), None)


def test_attached_accumulator_that_takes_no_more(mapped, pkg, gpu_ctx, tmp_path):
    """a finished accumulator makes the attached calls fail before they encode; a writer without a context cannot take one"""
    m, batches = mapped("sr")
    with pkg.Coverage(m) as cov:
        cov.finish()
        with pkg.BgzfWriter(str(tmp_path / "x.bam"), ctx=gpu_ctx) as w:
            w.set_coverage(cov)
            with pytest.raises(pkg.GdietError, match="read-only"):
                w.write_bam(m, *batches[0].args())
            w.set_coverage(None)
            w.write_bam(m, *batches[0].args())
        with pkg.BgzfWriter(str(tmp_path / "y.bam")) as w:
            with pytest.raises(pkg.GdietError, match="one context"):
                w.set_coverage(cov)


# ---- the tool --------------------------------------------------------------------------------------------------------------------------
def test_map_file_coverage(tmp_path):
    """tools/map_file.py --bam --sort --coverage p --cov-window 100 from file to file on sr: the two text files are the ones printed from
    the oracle's integers; SAM output with --coverage (Coverage.add on the writer thread) writes the same two files"""
    fq = str(tmp_path / "reads.fq")
    write_fastq("sr", fq)
    recs, names, lens, lines = ci.golden_records("sr")
    want = cr.coverage(b"".join(recs), lens, window=100)
    base = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "map_file.py"), "--preset", "sr", os.path.join(SETS["sr"][0], "ref.fa.gz"), fq]
    for tag, extra, attached in (("sorted", ["--bam", "--sort", "--tmp-dir", str(tmp_path)], True), ("sam", [], False)):
        prefix = str(tmp_path / tag)
        r = subprocess.run(base + extra + ["-o", prefix + ".out", "--coverage", prefix, "--cov-window", "100"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        rep = json.loads(r.stdout.strip().split("\n")[-1])["coverage"]
        assert rep["attached"] is attached and {k: rep[k] for k in cr.SUMMARY} == want.summary
        assert open(prefix + ".coverage.tsv").read() == cr.coverage_tsv(want, names, lens)
        assert open(prefix + ".regions.bed").read() == cr.regions_bed(want, names, lens, 100)
    r = subprocess.run(base + ["-o", str(tmp_path / "plain.sam")], capture_output=True, text=True)  # without the flag: no files, no key
    assert r.returncode == 0 and "coverage" not in json.loads(r.stdout.strip().split("\n")[-1])
    assert open(str(tmp_path / "plain.sam"), "rb").read() == open(str(tmp_path / "sam.out"), "rb").read()


# ---- memory ----------------------------------------------------------------------------------------------------------------------------
def _hip_runtime():
    """the HIP runtime this process has loaded"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "no HIP runtime is loaded"
    return C.CDLL(paths[0])


def test_nothing_is_left_behind(pkg, gpu_ctx, small):
    """open / add / finish / close in rounds, refused calls among them: hipMemGetInfo is back where it started and the stream-ordered
    pool holds nothing more; an accumulator that outlives its context has lost its arrays and takes nothing but close"""
    hip = _hip_runtime()
    pool = C.c_void_p()
    assert hip.hipDeviceGetDefaultMemPool(C.byref(pool), 0) == 0

    def used():
        assert hip.hipDeviceSynchronize() == 0
        v, free, total = C.c_uint64(), C.c_size_t(), C.c_size_t()
        assert hip.hipMemPoolGetAttribute(pool, 7, C.byref(v)) == 0  # hipMemPoolAttrUsedMemCurrent
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return v.value, free.value

    data, bad = b"".join(ci.border_set()), b"".join(ci.with_bad("op9"))

    def round_(refusals):
        with pkg.Coverage(small, window=64) as cov:
            cov.add_bam(data)
            if refusals:
                with pytest.raises(pkg.GdietError):
                    cov.add_bam(data[:-3])
                with pytest.raises(pkg.GdietError):
                    cov.add_bam(bad)
                with pytest.raises(pkg.GdietError):
                    cov.finish()
            else:
                cov.finish(chunk=256)
                cov.windows(4), cov.depth(4, 0, 6000)

    round_(False), round_(True)  # warm-up: the lane's stream, the pool's first pages
    first = used()
    for k in range(4):
        round_(k % 2 == 1)
    assert used() == first
    def own_context(with_cov):
        """a context of its own with a mapper, destroyed -- with an accumulator still open"""
        ctx = pkg.Context(0)
        m = pkg.Mapper(ctx, ["a"], ["ACGT" * 500], preset="hifi")
        cov = pkg.Coverage(m) if with_cov else None
        if cov is not None:
            cov.add_bam(ci.rec(0, 10, [(30, "M")]))
        m.close()
        ctx.close()
        if cov is not None:
            with pytest.raises(pkg.GdietError, match="context has been destroyed"):
                cov.add_bam(ci.rec(0, 10, [(30, "M")]))
            cov.close()

    own_context(False)  # warm-up: what the first further context of a process costs once
    first = used()
    own_context(False)
    assert used() == first  # (a context comes and goes without a trace: the next line can be read)
    own_context(True)
    assert used() == first

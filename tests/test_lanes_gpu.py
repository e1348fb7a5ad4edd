"""GPU: the side lanes of a context (GdLane in csrc/gdiet_hip.hip: difference strings, the reader's device mode, BGZF inflate and deflate,
the BAM encoder) through their whole life -- every lane opened once in a fresh context that is then destroyed, a context destroyed with
one lane opened -- and their stream-ordered allocations (GdStreamMem): after rounds of calls, refused ones among them, the device's
default memory pool holds what it held before."""
import ctypes as C
import gzip

import numpy as np
import pytest

import bam_in_inputs as bam_in
import bgzf_inputs as bz
import diffstr_ref as dr
from test_diffstr_gpu import HandRes

pytestmark = pytest.mark.gpu

TEXT = b"@r0\nACGT\n+\nIIII\n"
MEMBER = bz.member(TEXT)  # one member of under 100 bytes
CUT = bz.member_of_stream(bz.deflate_raw(TEXT * 20)[:-6], TEXT * 20)  # a whole member around a deflate stream that ends early
BAM_RECORD = bam_in.rec(b"a", [1, 2], [3, 4])
FASTQ = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, b"ACGTTGCA" * (i + 2), b"I" * (8 * (i + 2))) for i in range(4))
assert len(MEMBER) < 100


class Small:
    """a mapper over one random contig, three reads cut from it and a hand-made record for each"""

    def __init__(self, pkg, ctx, tmp_path):
        rng = np.random.default_rng(11)
        contig = "".join("ACGT"[c] for c in rng.integers(0, 4, 3000))
        self.ctx, self.pkg = ctx, pkg
        self.m = pkg.Mapper(ctx, ["c0"], [contig], preset="hifi")
        at = [(100, 70), (900, 129), (2000, 64)]
        self.reads = [contig[s:s + n] for s, n in at]
        self.res = HandRes(pkg, 3, [dict(read=i, qs=0, qe=n, rs=s, re=s + n, rid=0, rev=0, cigar=[(0, n)]) for i, (s, n) in enumerate(at)])
        self.fastq = str(tmp_path / "four.fq")
        with open(self.fastq, "wb") as f:
            f.write(FASTQ)

    def round(self, refusals=False):
        """every lane once; what the calls returned is dropped before it returns"""
        ctx, m, pkg = self.ctx, self.m, self.pkg
        got = m.diffstr(self.res, self.reads, dr.MODE_FLAG["cs"])
        assert [s for per in got for s in per] == [b":70", b":129", b":64"]
        assert ctx.bgzf_inflate(MEMBER) == TEXT
        assert gzip.decompress(ctx.bgzf_deflate(b"0123456789")) == b"0123456789"
        text, off, lens = ctx.bam_in_unpack(BAM_RECORD * 2)
        assert text == b"AC\0$%\0" * 2 and list(lens) == [2, 2]
        assert len(m.bam_batch(self.res, [("r%d" % i, s, None) for i, s in enumerate(self.reads)])) > 3 * 36
        with pkg.FastxReader(self.fastq, ctx=ctx) as r:
            n, _, _, seqs, _, lens, _, batch = r.read_raw(100000, resident=True)
            try:
                assert n == 4 and [seqs[i] for i in range(n)] == [b"ACGTTGCA" * (i + 2) for i in range(4)]
            finally:
                m.free_batch(batch)
        if refusals:
            with pytest.raises(pkg.GdietError, match="member 0"):  # refused by the kernel's result, after it has run
                ctx.bgzf_inflate(CUT)
            with pytest.raises(pkg.GdietError, match="ends inside a record"):
                ctx.bam_in_unpack(BAM_RECORD + BAM_RECORD[:-1])

    def seconds(self):
        """the sums of the three lanes that keep events: inflate, deflate, BAM encoder"""
        with self.pkg.FastxReader(self.fastq, ctx=self.ctx) as r:
            t = (C.c_double * 6)()
            assert r.lib.gdiet_hip_debug_bgzf_seconds(r._h, t) == 0
        return sum(t[3:6]), sum(self.ctx.bgzf_deflate_seconds()), sum(self.m.bam_device_seconds())


def test_lanes_open_on_first_use_and_go_with_the_context(pkg, gpu_ctx, tmp_path):
    ctx = pkg.Context(0)  # (gpu_ctx: the session's runtime is up)
    try:
        s = Small(pkg, ctx, tmp_path)
        try:
            before = s.seconds()
            assert before == (0, 0, 0)
            s.round()
            after = s.seconds()
            assert all(a > b for a, b in zip(after, before)), (before, after)
        finally:
            s.m.close()
    finally:
        ctx.close()
    ctx = pkg.Context(0)  # ... and a context whose other lanes were never opened
    try:
        assert gzip.decompress(ctx.bgzf_deflate(b"0123456789")) == b"0123456789"
    finally:
        ctx.close()


def _hip_runtime():
    """the HIP runtime this process has loaded"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "no HIP runtime is loaded"
    return C.CDLL(paths[0])


def test_nothing_is_left_in_the_memory_pool(pkg, gpu_ctx, tmp_path):
    hip = _hip_runtime()
    pool = C.c_void_p()
    assert hip.hipDeviceGetDefaultMemPool(C.byref(pool), 0) == 0

    def used():
        assert hip.hipDeviceSynchronize() == 0
        v = C.c_uint64()
        assert hip.hipMemPoolGetAttribute(pool, 7, C.byref(v)) == 0  # hipMemPoolAttrUsedMemCurrent
        return v.value

    s = Small(pkg, gpu_ctx, tmp_path)
    try:
        s.round()  # warm-up: the lanes' streams and the buffers that stay with the context
        first = used()
        for k in range(3):
            s.round(refusals=k == 1)
        assert used() == first
    finally:
        s.m.close()

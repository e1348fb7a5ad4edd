"""Per-contig coverage and depth accumulated on the device: ``Coverage`` over the library's accumulator (``gdiet_hip_cov_*``,
csrc/cov_driver.hip.h; what it shares with ``Pileup`` is in accum.py).  The records of every batch are walked where they are resident
(csrc/cov.hip.h: one wavefront per record scatters +1 / -1 into a difference array over the whole reference); ``finish`` sums the array
and reduces it per window.  The rules are the section "Coverage" of include/gdiet_hip.h.  The array costs 4 bytes per reference base
while the object lives."""
import ctypes as C

import numpy as np

from .accum import Accumulator
from .hip_abi import load_library
from .map_api import Reg

SUMMARY = ("records", "unmapped", "secondary", "supplementary", "primary_mapped", "reverse", "excluded_by_flag", "excluded_by_mapq", "counted", "bad")
CONTIG = np.dtype([(k, "<u8") for k in ("n_reads", "cov_bases", "sum_depth", "sum_mapq", "sum_baseq", "n_baseq")])


def _bind(lib):
    if getattr(lib, "_cov_bound", False):
        return
    vp, cpp, i32p, u32, u64 = C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_uint32, C.c_uint64
    lib.gdiet_hip_cov_open.argtypes = [vp, vp, u32, u32, u32, C.POINTER(vp)]
    lib.gdiet_hip_cov_add_bam.argtypes = [vp, C.c_char_p, C.c_size_t]
    lib.gdiet_hip_cov_add.argtypes = [vp, vp, C.c_int, cpp, cpp, cpp, i32p, i32p, C.POINTER(C.POINTER(Reg)), cpp, C.c_int64]
    lib.gdiet_hip_cov_finish_chunked.argtypes = [vp, u64, vp, vp]
    lib.gdiet_hip_cov_windows.argtypes = [vp, u32, vp, vp, C.c_size_t]
    lib.gdiet_hip_cov_windows.restype = C.c_int64
    lib.gdiet_hip_cov_depth.argtypes = [vp, u32, u32, u32, vp]
    lib.gdiet_hip_cov_close.argtypes = [vp]
    lib.gdiet_hip_bgzf_out_set_coverage.argtypes = [vp, vp]
    lib.gdiet_hip_bam_sort_set_coverage.argtypes = [vp, vp]
    lib._cov_bound = True


class Coverage(Accumulator):
    """``Coverage(mapper, excl_flags=0x704, min_mapq=0, window=0)``.  Records come in through ``add`` (a mapped batch: the arguments of
    ``Mapper.bam_batch_raw``; encoded and scattered on the device, nothing comes down), ``add_bam`` (bytes of uncompressed BAM records) or
    an attached ``BgzfWriter`` / ``BamSorter`` (``set_coverage``).  ``finish()`` returns (per-contig numpy records, summary dict); then
    ``windows(rid)``, ``depth(rid, beg, end)`` and ``write(prefix)`` read the result.  A bad record raises ``GdietError`` and leaves the
    object refusing everything but ``close``."""
    _prefix, _name = "cov", "Coverage"

    def __init__(self, mapper, excl_flags=0x704, min_mapq=0, window=0):
        self.lib = load_library()
        _bind(self.lib)
        self.mapper, self.window = mapper, int(window)
        info = mapper.index_info()
        self.names, self.lens = info["names"], [int(x) for x in info["lens"]]
        self._h = C.c_void_p()
        self._result = None
        self._check(self.lib.gdiet_hip_cov_open(mapper.ctx._h, mapper._idx, int(excl_flags), int(min_mapq), self.window, C.byref(self._h)))

    def finish(self, chunk=0):
        """(contigs, summary): numpy records n_reads cov_bases sum_depth sum_mapq sum_baseq n_baseq, one per contig, and the dict of the
        ten counters.  ``chunk`` is the scan's chunk in slots (0: the default); the result does not depend on it."""
        self._open()
        contigs = np.zeros(len(self.lens), CONTIG)
        summary = (C.c_uint64 * len(SUMMARY))()
        self._check(self.lib.gdiet_hip_cov_finish_chunked(self._h, int(chunk), contigs.ctypes.data, summary))
        self._result = (contigs, dict(zip(SUMMARY, (int(x) for x in summary))))
        return self._result

    def windows(self, rid):
        """(cov_bases uint32, sum_depth uint64) of the windows of contig rid; after finish, window > 0"""
        self._open()
        n = self._check(self.lib.gdiet_hip_cov_windows(self._h, rid, None, None, 0))
        cov, sums = np.zeros(n, np.uint32), np.zeros(n, np.uint64)
        self._check(self.lib.gdiet_hip_cov_windows(self._h, rid, cov.ctypes.data, sums.ctypes.data, n))
        return cov, sums

    def depth(self, rid, beg, end):
        self._open()
        out = np.zeros(max(0, end - beg), np.uint32)
        self._check(self.lib.gdiet_hip_cov_depth(self._h, rid, beg, end, out.ctypes.data))
        return out

    def write(self, prefix):
        """``<prefix>.coverage.tsv`` in the layout of `samtools coverage` with a #summary trailer, and, with a window,
        ``<prefix>.regions.bed`` (rname start end mean depth).  The ratios are formed here, in double, from the device's integers."""
        contigs, summary = self._result if self._result is not None else self.finish()
        ratio = lambda num, den, fmt, scale=1.0: fmt % (scale * int(num) / int(den)) if int(den) else "0"
        with open(str(prefix) + ".coverage.tsv", "w") as f:
            f.write("#rname\tstartpos\tendpos\tnumreads\tcovbases\tcoverage\tmeandepth\tmeanbaseq\tmeanmapq\n")
            for name, n, c in zip(self.names, self.lens, contigs):
                f.write("\t".join([name, "1", str(n), str(int(c["n_reads"])), str(int(c["cov_bases"])), ratio(c["cov_bases"], n, "%.6g", 100.0), ratio(c["sum_depth"], n, "%.6g"),
                                   ratio(c["sum_baseq"], c["n_baseq"], "%.3g"), ratio(c["sum_mapq"], c["n_reads"], "%.3g")]) + "\n")
            f.write("#summary\t" + "\t".join("%s=%d" % (k, summary[k]) for k in SUMMARY) + "\n")
        if self.window > 0:
            with open(str(prefix) + ".regions.bed", "w") as f:
                for rid, (name, n) in enumerate(zip(self.names, self.lens)):
                    _, sums = self.windows(rid)
                    for k, s in enumerate(sums):
                        beg, end = k * self.window, min(n, (k + 1) * self.window)
                        f.write("%s\t%d\t%d\t%.2f\n" % (name, beg, end, int(s) / (end - beg)))

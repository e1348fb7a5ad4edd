"""Base counts per position and variant sites accumulated on the device: ``Pileup`` over the library's accumulator (``gdiet_hip_pile_*``,
csrc/pile_driver.hip.h; what it shares with ``Coverage`` is in accum.py).  The records of every batch are walked where they are
resident (csrc/pile.hip.h: one wavefront per record adds every base, deletion and insertion anchor to the eight counters of its
position); after ``finish`` the consensus and the sites are formed on the device in integers.  The rules are the section "Pileup" of
include/gdiet_hip.h.  The counters cost 32 bytes per position of the regions while the object lives."""
import ctypes as C

import numpy as np

from .accum import Accumulator
from .hip_abi import load_library
from .map_api import Reg

SUMMARY = ("records", "unmapped", "secondary", "supplementary", "primary_mapped", "reverse", "excluded_by_flag", "excluded_by_mapq", "counted", "bad", "no_seq", "skipped_baseq")
COUNTERS = ("A", "C", "G", "T", "N", "DEL", "INS", "REV")
REGION = np.dtype([("rid", "<u4"), ("beg", "<u4"), ("end", "<u4")])
SITE = np.dtype([("rid", "<u4"), ("pos", "<u4"), ("ref", "<u4"), ("alt", "<u4"), ("depth", "<u4"), ("cnt", "<u4", (8,))])
REF_LETTERS, ALT_LETTERS = "ACGTN", "ACGT*+"


def _bind(lib):
    if getattr(lib, "_pile_bound", False):
        return
    vp, cpp, i32p, u32, u64 = C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_uint32, C.c_uint64
    lib.gdiet_hip_pile_open.argtypes = [vp, vp, vp, C.c_size_t, u32, u32, u32, C.POINTER(vp)]
    lib.gdiet_hip_pile_add_bam.argtypes = [vp, C.c_char_p, C.c_size_t]
    lib.gdiet_hip_pile_add.argtypes = [vp, vp, C.c_int, cpp, cpp, cpp, i32p, i32p, C.POINTER(C.POINTER(Reg)), cpp, C.c_int64]
    lib.gdiet_hip_pile_finish_chunked.argtypes = [vp, u64, vp]
    lib.gdiet_hip_pile_counts.argtypes = [vp, u32, u32, u32, vp]
    lib.gdiet_hip_pile_consensus.argtypes = [vp, C.c_size_t, u32, vp]
    lib.gdiet_hip_pile_sites.argtypes = [vp, u32, u32, u32, u32, vp, C.c_size_t]
    lib.gdiet_hip_pile_sites.restype = C.c_int64
    lib.gdiet_hip_pile_close.argtypes = [vp]
    lib.gdiet_hip_bgzf_out_set_pileup.argtypes = [vp, vp]
    lib.gdiet_hip_bam_sort_set_pileup.argtypes = [vp, vp]
    lib._pile_bound = True


class Pileup(Accumulator):
    """``Pileup(mapper, regions=None, excl_flags=0x704, min_mapq=0, min_baseq=0)``; ``regions`` is a list of (rid, beg, end), 0-based and
    half-open, sorted and disjoint (None: every contig whole).  Records come in through ``add`` (a mapped batch: the arguments of
    ``Mapper.bam_batch_raw``; encoded and scattered on the device, nothing comes down), ``add_bam`` (bytes of uncompressed BAM records) or
    an attached ``BgzfWriter`` / ``BamSorter`` (``set_pileup``).  ``finish()`` returns the summary dict; then ``counts``, ``consensus``,
    ``sites`` and ``write`` read the result.  A bad record raises ``GdietError`` and leaves the object refusing everything but ``close``.
    Keep the mapper open while the object is used."""
    _prefix, _name = "pile", "Pileup"

    def __init__(self, mapper, regions=None, excl_flags=0x704, min_mapq=0, min_baseq=0):
        self.lib = load_library()
        _bind(self.lib)
        self.mapper = mapper
        info = mapper.index_info()
        self.names, self.lens = info["names"], [int(x) for x in info["lens"]]
        self.regions = [tuple(int(x) for x in r) for r in regions] if regions else [(rid, 0, n) for rid, n in enumerate(self.lens) if n]
        given = np.array([tuple(int(x) for x in r) for r in regions], REGION) if regions else np.zeros(0, REGION)
        self._h = C.c_void_p()
        self._summary = None
        self._check(self.lib.gdiet_hip_pile_open(mapper.ctx._h, mapper._idx, given.ctypes.data if len(given) else None, len(given), int(excl_flags), int(min_mapq), int(min_baseq),
                                                 C.byref(self._h)))

    def finish(self, chunk=0):
        """the dict of the twelve summary counters.  ``chunk`` is the chunk, in positions, of the scan ``sites`` runs (0: the default); no
        result depends on it."""
        self._open()
        summary = (C.c_uint64 * len(SUMMARY))()
        self._check(self.lib.gdiet_hip_pile_finish_chunked(self._h, int(chunk), summary))
        self._summary = dict(zip(SUMMARY, (int(x) for x in summary)))
        return self._summary

    def counts(self, rid, beg, end):
        """(end - beg, 8) uint32: A C G T N DEL INS REV of positions [beg, end) of contig rid, which must lie inside one region"""
        self._open()
        out = np.zeros((max(0, end - beg), 8), np.uint32)
        self._check(self.lib.gdiet_hip_pile_counts(self._h, rid, beg, end, out.ctypes.data))
        return out

    def consensus(self, i, min_depth=1):
        """the consensus bytes of region i (A C G T, * for a deletion, N below min_depth or without an allele)"""
        self._open()
        if not 0 <= i < len(self.regions):
            raise ValueError("region %d of %d" % (i, len(self.regions)))
        out = np.zeros(self.regions[i][2] - self.regions[i][1], np.uint8)
        self._check(self.lib.gdiet_hip_pile_consensus(self._h, i, int(min_depth), out.ctypes.data))
        return out.tobytes()

    def sites(self, min_depth=8, min_alt=2, frac=(1, 5)):
        """the sites as a structured array (rid pos ref alt depth cnt[8]) in position order; ref 0..4 is A C G T N, alt 0..5 A C G T * +"""
        self._open()
        args = (int(min_depth), int(min_alt), int(frac[0]), int(frac[1]))
        n = self._check(self.lib.gdiet_hip_pile_sites(self._h, *args, None, 0))
        out = np.zeros(n, SITE)
        if n:
            self._check(self.lib.gdiet_hip_pile_sites(self._h, *args, out.ctypes.data, n))
        return out

    def write(self, prefix, min_depth=8, min_alt=2, frac=(1, 5)):
        """``<prefix>.pileup.tsv``, the sites (contig, 1-based position, ref, alt, depth, the eight counters), and ``<prefix>.consensus.fa``,
        one record per region at this min_depth; both formed here from the device's integers and bytes"""
        if self._summary is None:
            self.finish()
        with open(str(prefix) + ".pileup.tsv", "w") as f:
            f.write("#contig\tpos\tref\talt\tdepth\t" + "\t".join(COUNTERS) + "\n")
            for r in self.sites(min_depth, min_alt, frac):
                f.write("\t".join([self.names[int(r["rid"])], str(int(r["pos"]) + 1), REF_LETTERS[int(r["ref"])], ALT_LETTERS[int(r["alt"])], str(int(r["depth"]))] +
                                  [str(int(x)) for x in r["cnt"]]) + "\n")
        with open(str(prefix) + ".consensus.fa", "wb") as f:
            for i, (rid, beg, end) in enumerate(self.regions):
                s = np.frombuffer(self.consensus(i, min_depth), np.uint8)
                f.write((">%s:%d-%d\n" % (self.names[rid], beg + 1, end)).encode())
                whole = len(s) // 60 * 60  # lines of 60 bases; a whole chromosome is tens of millions of them
                if whole:
                    f.write(np.concatenate([s[:whole].reshape(-1, 60), np.full((whole // 60, 1), 10, np.uint8)], axis=1).tobytes())
                if whole < len(s):
                    f.write(s[whole:].tobytes() + b"\n")

"""Coordinate-sorted, indexed BAM output: ``BamSorter`` over the library's sorter (``gdiet_hip_bam_sort_*``, csrc/bam_sorter.h).
Batches are encoded on the device into a resident run buffer; a full run is sorted there (csrc/bam_sort.hip.h) and spooled; ``close``
merges the runs on the device in chunks, writes the BGZF stream and ``<path>.bai``.  The order and the index are defined in
include/gdiet_hip.h, "Sorted BAM output"."""
import ctypes as C

import numpy as np

from .hip_abi import DupStats, GdietError, load_library
from .map_api import Reg


class SortStats(C.Structure):
    _fields_ = [("records", C.c_int64), ("runs", C.c_int64), ("spooled_bytes", C.c_int64), ("chunks", C.c_int64), ("members", C.c_int64), ("n_no_coor", C.c_int64),
                ("seconds", C.c_double * 5)]


class BamSorter:
    """``BamSorter(path, mapper, bgzf="device", level=-1, threads=4, run_bytes=1 << 29, chunk_bytes=1 << 28, tmp_dir=None, index=True,
    version=None, argv=(), markdup=False)``: writes the header ``mapper.bam_header(version, argv, sort_order="coordinate")`` at once.  ``add`` takes a
    mapped batch (the arguments of ``Mapper.bam_batch_raw``); ``close`` returns the stats: records, runs, spooled_bytes, chunks, members,
    n_no_coor and the sorter's seconds (device: key_sort, gather; wall: spool_write, spool_read, compress).  ``bgzf="host"``: zlib at
    ``level`` on ``threads`` host threads compresses.  The spools live in ``tmp_dir`` (default: the output's directory) without a
    name: nothing is left behind.  ``markdup=True``: bit 0x400 of the file's records is decided on the device under the rule "Duplicate
    marking" of include/gdiet_hip.h (one decision over the whole file, before its first chunk is streamed), and ``close`` returns one
    more entry, ``"dup"``: examined, eligible, duplicates, max_group."""

    def __init__(self, path, mapper, bgzf="device", level=-1, threads=4, run_bytes=1 << 29, chunk_bytes=1 << 28, tmp_dir=None, index=True, version=None, argv=(), markdup=False):
        if bgzf not in ("device", "host"):
            raise ValueError("bgzf is 'device' or 'host'")
        self.lib = load_library()
        vp, cpp, i32p = C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32)
        self.lib.gdiet_hip_bam_sort_open.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_char_p, C.c_int, C.POINTER(vp)]
        self.lib.gdiet_hip_bam_sort_add.argtypes = [vp, vp, C.c_int, cpp, cpp, cpp, cpp, i32p, i32p, C.POINTER(C.POINTER(Reg)), C.c_int64]
        self.lib.gdiet_hip_bam_sort_close.argtypes = [vp, C.POINTER(SortStats)]
        self.lib.gdiet_hip_bam_sort_close_dup.argtypes = [vp, C.POINTER(SortStats), C.POINTER(DupStats)]
        self.lib.gdiet_hip_bam_sort_set_markdup.argtypes = [vp, C.c_int]
        self.markdup = False
        self.mapper, self.path = mapper, str(path)
        self._h = C.c_void_p()
        self.stats = None
        header = mapper.bam_header(version, argv, sort_order="coordinate")
        rc = self.lib.gdiet_hip_bam_sort_open(mapper.ctx._h, self.path.encode(), header, len(header), int(bgzf == "device"), int(level), int(threads), int(run_bytes), int(chunk_bytes),
                                              None if tmp_dir is None else str(tmp_dir).encode(), int(bool(index)), C.byref(self._h))
        if rc:  # (the handle of a refused open takes nothing but its close)
            text = self._text()
            h, self._h = self._h, C.c_void_p()
            if h:
                self.lib.gdiet_hip_bam_sort_close(h, None)
            raise GdietError("gdiet_hip error %d: %s" % (rc, text))
        if markdup:
            self.set_markdup(True)

    def set_markdup(self, on):
        """gdiet_hip_bam_sort_set_markdup: chosen before the first ``add``; afterwards it is refused (GdietError)"""
        if not self._h:
            raise ValueError("set_markdup on a closed BamSorter")
        rc = self.lib.gdiet_hip_bam_sort_set_markdup(self._h, int(bool(on)))
        if rc:
            raise GdietError("gdiet_hip error %d: %s" % (rc, self._text()))
        self.markdup = bool(on)

    def _text(self):
        t = self.lib.gdiet_hip_strerror(self.mapper.ctx._h)
        return t.decode() if t else ""

    def add(self, res, n, names, seqs, quals, lens, comments=None):
        if not self._h:
            raise ValueError("add to a closed BamSorter")
        cpp = C.POINTER(C.c_char_p)
        rc = self.lib.gdiet_hip_bam_sort_add(self._h, self.mapper._idx, n, C.cast(names, cpp), C.cast(seqs, cpp), C.cast(quals, cpp), C.cast(comments, cpp), lens, res.n_regs,
                                             res.regs, self.mapper.opt.flag)
        if rc:
            raise GdietError("gdiet_hip error %d: %s" % (rc, self._text()))

    def _attach(self, kind, obj):
        if not self._h:
            raise ValueError("set_%s on a closed BamSorter" % kind)
        fn = getattr(self.lib, "gdiet_hip_bam_sort_set_" + kind)
        fn.argtypes = [C.c_void_p, C.c_void_p]
        rc = fn(self._h, obj._h if obj is not None else None)
        if rc:
            raise GdietError("gdiet_hip error %d: %s" % (rc, self._text()))
        setattr(self, "_" + kind, obj)  # (kept alive while attached)

    def set_coverage(self, cov):
        """Attach a ``Coverage`` (None: detach): every later ``add`` scatters into it from the records it has just encoded into the run
        buffer, before they are sorted; the file's bytes do not change.  Keep ``cov`` open while attached.  With ``markdup`` the scatter
        still happens at ``add``, before any duplicate flag exists, so duplicates are counted: to leave them out, feed the finished
        file's records to a ``Coverage`` through ``add_bam``."""
        self._attach("coverage", cov)

    def set_pileup(self, pile):
        """Attach a ``Pileup`` (None: detach), beside ``set_coverage`` and under its rules; both may be attached at once.  Like an
        attached ``Coverage`` it sees the records before ``markdup`` has flagged any: duplicates are piled up too (``add_bam`` of the
        finished records leaves them out)."""
        self._attach("pileup", pile)

    def set_stats(self, stats):
        """Attach a ``Stats`` (None: detach), beside ``set_coverage`` and ``set_pileup`` and under their rules; all three may be attached at
        once.  Like them it sees the records before ``markdup`` has flagged any: marked duplicates are counted like any other record
        (``add_bam`` of the finished records leaves them out)."""
        self._attach("stats", stats)

    def add_reads(self, res, reads):
        """add on Python objects: reads = [(qname, seq, qual or None[, comment or None]), ...]"""
        n = len(reads)
        enc = lambda x: x if isinstance(x, bytes) else x.encode()
        qn = (C.c_char_p * n)(*[enc(r[0]) for r in reads])
        sq = (C.c_char_p * n)(*[enc(r[1]) for r in reads])
        ql = (C.c_char_p * n)(*[None if len(r) < 3 or r[2] is None else enc(r[2]) for r in reads])
        cm = (C.c_char_p * n)(*[None if len(r) < 4 or r[3] is None else enc(r[3]) for r in reads])
        lens = np.array([len(r[1]) for r in reads], np.int32)
        self.add(res, n, qn, sq, ql, lens.ctypes.data_as(C.POINTER(C.c_int32)), comments=cm)

    def close(self):
        """ends the file, writes the index, frees the spools; returns the stats (also after a failure: the handle is freed either way)"""
        if not self._h:
            return self.stats
        st, dup = SortStats(), DupStats()
        h, self._h = self._h, C.c_void_p()
        rc = self.lib.gdiet_hip_bam_sort_close_dup(h, C.byref(st), C.byref(dup))
        self.stats = dict(records=st.records, runs=st.runs, spooled_bytes=st.spooled_bytes, chunks=st.chunks, members=st.members, n_no_coor=st.n_no_coor,
                          seconds=dict(zip(("key_sort", "gather", "spool_write", "spool_read", "compress"), (round(x, 6) for x in st.seconds))))
        if self.markdup:
            self.stats["dup"] = dup.as_dict()
        if rc:
            raise GdietError("gdiet_hip error %d: %s" % (rc, self._text()))
        return self.stats

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

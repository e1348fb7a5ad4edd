"""BGZF output (the blocked gzip of htslib's bgzip): ``BgzfWriter``, a binary sink over the library's stream writer
(``gdiet_hip_bgzf_out_*``, csrc/bgzf_out.h).  With a context the members are compressed on the device, one wavefront per member of
65280 input bytes (csrc/bgzf_deflate.hip.h); without one by zlib on host threads.  Either way the file is ordinary multi-member gzip."""
import ctypes as C

from .hip_abi import GdietError, load_library


class BgzfWriter:
    """``BgzfWriter(path, ctx=None, level=-1, threads=4)``: ``write`` takes any object with the buffer protocol, so
    ``Mapper.sam_batch_raw(..., sink=writer)`` works as with a file.  Members are full except where ``flush`` or ``close`` ends one;
    ``close`` writes the end-of-file member.  ``level`` and ``threads`` are zlib's and the host's: they mean nothing with a context."""

    def __init__(self, path, ctx=None, level=-1, threads=4):
        self.lib = load_library()
        self._ctx = ctx  # (kept alive: the writer uses its stream)
        self._h = C.c_void_p()
        self._stats = None
        self._check(self.lib.gdiet_hip_bgzf_out_open(ctx._h if ctx is not None else None, str(path).encode(), int(level), int(threads), C.byref(self._h)))

    def _check(self, rc):
        if rc != 0:
            raise GdietError("gdiet_hip error %d: %s" % (rc, self.lib.gdiet_hip_strerror(self._ctx._h if self._ctx is not None else None).decode()))

    def _open(self):
        if not self._h:
            raise ValueError("write to a closed BgzfWriter")

    def write(self, buffer):
        self._open()
        mv = memoryview(buffer)
        if not mv.c_contiguous:
            mv = memoryview(mv.tobytes())
        n = mv.nbytes
        if n == 0:
            return 0
        if mv.readonly:  # (ctypes takes a pointer from bytes only: a read-only view of anything else is copied)
            self._check(self.lib.gdiet_hip_bgzf_out_write(self._h, buffer if type(buffer) is bytes else mv.tobytes(), n))
        else:
            self._check(self.lib.gdiet_hip_bgzf_out_write(self._h, (C.c_char * n).from_buffer(mv.cast("B")), n))
        return n

    def write_bam(self, mapper, res, n, names, seqs, quals, lens, comments=None):
        """The BAM records of a mapped batch appended to the stream (``gdiet_hip_bgzf_out_write_bam``; the arguments of
        ``Mapper.bam_batch_raw``, which this is with the writer as sink).  With a context the records are encoded on the device behind the
        writer's waiting tail and compressed there: the uncompressed records never reach the host.  Write ``mapper.bam_header()`` first."""
        self._open()
        mapper.bam_batch_raw(res, n, names, seqs, quals, lens, sink=self, comments=comments)

    def write_sam(self, mapper, res, n, names, seqs, quals, lens, comments=None):
        """The SAM lines of a mapped batch appended to the stream (``gdiet_hip_bgzf_out_write_sam``; the arguments of
        ``Mapper.sam_batch_raw``, which this is with ``device=True`` and the writer as sink).  With a context the lines are written on the
        device behind the writer's waiting tail and compressed there: the uncompressed text never reaches the host.  Write
        ``mapper.sam_header()`` first, through ``write``."""
        self._open()
        mapper.sam_batch_raw(res, n, names, seqs, quals, lens, sink=self, comments=comments, device=True)

    def _attach(self, kind, obj):
        self._open()
        fn = getattr(self.lib, "gdiet_hip_bgzf_out_set_" + kind)
        fn.argtypes = [C.c_void_p, C.c_void_p]
        self._check(fn(self._h, obj._h if obj is not None else None))
        setattr(self, "_" + kind, obj)  # (kept alive while attached)

    def set_coverage(self, cov):
        """Attach a ``Coverage`` (None: detach): every later ``write_bam`` scatters into it from the records it has just encoded on the
        device, before they are compressed; the file's bytes do not change.  The writer needs a context.  Keep ``cov`` open while attached."""
        self._attach("coverage", cov)

    def set_pileup(self, pile):
        """Attach a ``Pileup`` (None: detach), beside ``set_coverage`` and under its rules; both may be attached at once."""
        self._attach("pileup", pile)

    def set_stats(self, stats):
        """Attach a ``Stats`` (None: detach), beside ``set_coverage`` and ``set_pileup`` and under their rules; all three may be attached at once."""
        self._attach("stats", stats)

    def flush(self):
        self._open()
        self._check(self.lib.gdiet_hip_bgzf_out_flush(self._h))

    def stats(self):
        """members compressed by the device and by zlib, bytes taken and bytes written to the file (after close: the final figures)"""
        if not self._h:
            return dict(self._stats)
        v = [C.c_int64() for _ in range(4)]
        self.lib.gdiet_hip_bgzf_out_stats(self._h, *[C.byref(x) for x in v])
        return dict(zip(("members_device", "members_host", "bytes_in", "bytes_out"), (x.value for x in v)))

    def close(self):
        if not self._h:
            return
        rc = self.lib.gdiet_hip_bgzf_out_flush(self._h)  # (so that the figures read here are final but for the end-of-file member)
        self._stats = self.stats()
        h, self._h = self._h, C.c_void_p()
        rc2 = self.lib.gdiet_hip_bgzf_out_close(h)  # frees the writer whatever it returns
        if rc == 0 and rc2 == 0:
            self._stats["bytes_out"] += 28
        self._check(rc or rc2)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

"""ctypes mirror of the read-input entry points of include/gdiet_hip.h (gdiet_hip_fastx_*): FASTA / FASTQ, plain, gzip or BGZF,
mini-batch by mini-batch with the reference's record grammar and batching rule (LR/bseq.c:80-121, LR/kseq.h:191-232)."""
import ctypes as C

from .hip_abi import GdietError, load_library

W_TRUNCATED = 1


class FastxReader:
    """ctx: a Context; the reader is then attached to it (gdiet_hip_fastx_attach): the strict four-line FASTQ records at the front of
    every block are parsed on its device, and read_raw(..., resident=True) returns the resident batch next to the host arrays.  The
    records, batches and truncation flags do not depend on it.  Close the reader before the context.
    A BAM stream (its first four bytes, decompressed, are BAM\\1) is read record by record in place of the FASTQ grammar: SEQ and QUAL are
    unpacked on `threads` threads or, with ctx, on the device; format() says which grammar reads the file.
    A BGZF file (a regular file with the BGZF end-of-file member; GDIET_BGZF=0 turns it off) is inflated member by member: on `threads`
    threads, or, with ctx, on the device; bgzf_stats() says by whom."""

    def __init__(self, path, threads=1, ctx=None):
        self.lib = load_library()
        L = self.lib
        cpp = C.POINTER(C.c_char_p)
        L.gdiet_hip_fastx_open.argtypes = [C.POINTER(C.c_void_p), C.c_char_p]
        L.gdiet_hip_fastx_read.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(cpp), C.POINTER(cpp),
                                           C.POINTER(cpp), C.POINTER(cpp), C.POINTER(C.POINTER(C.c_int32))]
        L.gdiet_hip_fastx_close.argtypes = [C.c_void_p]
        L.gdiet_hip_fastx_close.restype = None
        self._h = C.c_void_p()
        if L.gdiet_hip_fastx_open(C.byref(self._h), path.encode() if isinstance(path, str) else path) != 0:
            raise GdietError("cannot open %r" % (path,))
        self.truncated = self.truncated_now = False
        L.gdiet_hip_fastx_set_threads.argtypes = [C.c_void_p, C.c_int]
        if threads > 1:
            L.gdiet_hip_fastx_set_threads(self._h, threads)
        L.gdiet_hip_fastx_attach.argtypes = [C.c_void_p, C.c_void_p]
        L.gdiet_hip_fastx_read_resident.argtypes = L.gdiet_hip_fastx_read.argtypes + [C.POINTER(C.c_void_p)]
        i64p = C.POINTER(C.c_int64)
        L.gdiet_hip_fastx_stats.argtypes = [C.c_void_p, i64p, i64p, i64p, i64p]
        L.gdiet_hip_fastx_bgzf_stats.argtypes = [C.c_void_p, i64p, i64p, i64p, i64p]
        L.gdiet_hip_debug_bgzf_seconds.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.gdiet_hip_fastx_strerror.argtypes = [C.c_void_p]
        L.gdiet_hip_fastx_strerror.restype = C.c_char_p
        L.gdiet_hip_fastx_format.argtypes = [C.c_void_p]
        self.ctx = ctx
        if ctx is not None and L.gdiet_hip_fastx_attach(self._h, ctx._h) != 0:
            raise GdietError("gdiet_hip_fastx_attach failed")

    def read(self, chunk_size, with_qual=True, with_comment=False, frag_mode=False):
        """next mini-batch as a list of (name, seq, qual or None, comment or None), all bytes; [] at the end of the input"""
        cpp = C.POINTER(C.c_char_p)
        n = C.c_int32()
        names, comments, seqs, quals, lens = cpp(), cpp(), cpp(), cpp(), C.POINTER(C.c_int32)()
        rc = self.lib.gdiet_hip_fastx_read(self._h, chunk_size, int(with_qual), int(with_comment), int(frag_mode), C.byref(n), C.byref(names),
                                           C.byref(comments), C.byref(seqs), C.byref(quals), C.byref(lens))
        if rc < 0:
            raise self._read_error()
        self.truncated_now = rc == W_TRUNCATED  # this batch was closed by a malformed record
        self.truncated = self.truncated or self.truncated_now
        out = []
        for i in range(n.value):
            s = seqs[i]
            assert len(s) == lens[i]
            out.append((names[i], s, quals[i], comments[i]))
        return out

    def read_raw(self, chunk_size, with_qual=True, with_comment=False, frag_mode=False, detach=False, resident=False):
        """next mini-batch as C arrays: (n, names, comments, seqs, quals, lens, token).  With detach=True the arrays stay valid until
        release(token) (several mini-batches in flight); otherwise until the next read.  With resident=True (a reader made with ctx) an
        eighth element follows: the resident batch of these reads (gdiet_hip_fastx_read_resident) as Mapper.upload_raw would return it,
        for Mapper.submit / map_uploaded / free_batch -- None when n is 0."""
        cpp = C.POINTER(C.c_char_p)
        n = C.c_int32()
        names, comments, seqs, quals, lens = cpp(), cpp(), cpp(), cpp(), C.POINTER(C.c_int32)()
        if resident:
            if self.ctx is None:
                raise GdietError("a resident batch needs a reader made with ctx")
            bh = C.c_void_p()
            rc = self.lib.gdiet_hip_fastx_read_resident(self._h, chunk_size, int(with_qual), int(with_comment), int(frag_mode), C.byref(n), C.byref(names),
                                                        C.byref(comments), C.byref(seqs), C.byref(quals), C.byref(lens), C.byref(bh))
        else:
            rc = self.lib.gdiet_hip_fastx_read(self._h, chunk_size, int(with_qual), int(with_comment), int(frag_mode), C.byref(n), C.byref(names),
                                               C.byref(comments), C.byref(seqs), C.byref(quals), C.byref(lens))
        if rc < 0:
            raise self._read_error()
        self.truncated_now = rc == W_TRUNCATED
        self.truncated = self.truncated or self.truncated_now
        token = None
        if detach and n.value:
            self.lib.gdiet_hip_fastx_detach.restype = C.c_void_p
            self.lib.gdiet_hip_fastx_detach.argtypes = [C.c_void_p]
            token = C.c_void_p(self.lib.gdiet_hip_fastx_detach(self._h))
        if resident:
            return n.value, names, comments, seqs, quals, lens, token, ((bh, n.value) if bh.value else None)
        return n.value, names, comments, seqs, quals, lens, token

    def stats(self):
        """gdiet_hip_fastx_stats: who parsed what since the reader was opened"""
        v = [C.c_int64() for _ in range(4)]
        self.lib.gdiet_hip_fastx_stats(self._h, *[C.byref(x) for x in v])
        return dict(zip(("records_device", "records_host", "blocks", "blocks_handed_over"), (x.value for x in v)))

    def format(self):
        """gdiet_hip_fastx_format: "bam" when the stream is BAM, else "fastx"; valid after the first read"""
        return "bam" if self.lib.gdiet_hip_fastx_format(self._h) == 1 else "fastx"

    def bgzf_stats(self):
        """gdiet_hip_fastx_bgzf_stats (all zero for a file that did not take the BGZF route), and the I/O thread's seconds per stage"""
        v = [C.c_int64() for _ in range(4)]
        self.lib.gdiet_hip_fastx_bgzf_stats(self._h, *[C.byref(x) for x in v])
        t = (C.c_double * 6)()
        self.lib.gdiet_hip_debug_bgzf_seconds(self._h, t)
        out = dict(zip(("members_device", "members_host", "bytes_in", "bytes_out"), (x.value for x in v)))
        # (h2d / kernel / d2h: the device's side of inflate_s, summed over the context's life, not the reader's)
        out.update(zip(("raw_read_s", "inflate_s", "check_s", "h2d_s", "kernel_s", "d2h_s"), (round(x, 4) for x in t)))
        return out

    def _read_error(self):
        return GdietError("read error: " + self.lib.gdiet_hip_fastx_strerror(self._h).decode() +
                          (" (" + self.lib.gdiet_hip_strerror(self.ctx._h).decode() + ")" if self.ctx is not None else ""))

    def release(self, token):
        if token:
            self.lib.gdiet_hip_fastx_batch_free.argtypes = [C.c_void_p]
            self.lib.gdiet_hip_fastx_batch_free.restype = None
            self.lib.gdiet_hip_fastx_batch_free(token)

    def close(self):
        if self._h:
            self.lib.gdiet_hip_fastx_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

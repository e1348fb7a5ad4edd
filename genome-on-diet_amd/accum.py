"""What ``Coverage``, ``Pileup`` and ``Stats`` share: the handle of an accumulator over BAM records (csrc/accum_driver.hip.h) and the calls that
bring records in.  A subclass names the prefix of its entry points (``gdiet_hip_<prefix>_*``) and itself, binds them, opens ``self._h`` in its
constructor and adds ``finish`` and its readers."""
import ctypes as C

import numpy as np

from .hip_abi import GdietError


class Accumulator:
    _prefix = None  # "cov" / "pile" / "stats"
    _name = None  # the class's name in the message of a closed object

    def _fn(self, name):
        return getattr(self.lib, "gdiet_hip_%s_%s" % (self._prefix, name))

    def _check(self, rc):
        if rc < 0:
            t = self.lib.gdiet_hip_strerror(self.mapper.ctx._h)
            raise GdietError("gdiet_hip error %d: %s" % (rc, t.decode() if t else ""))
        return rc

    def _open(self):
        if not self._h:
            raise ValueError("a closed %s" % self._name)

    def add(self, res, n, names, seqs, quals, lens, comments=None):
        self._open()
        cpp = C.POINTER(C.c_char_p)
        self._check(self._fn("add")(self._h, self.mapper._idx, n, C.cast(names, cpp), C.cast(seqs, cpp), C.cast(quals, cpp), lens, res.n_regs, res.regs, C.cast(comments, cpp),
                                    self.mapper.opt.flag))

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

    def add_bam(self, data):
        self._open()
        data = bytes(data)
        self._check(self._fn("add_bam")(self._h, data, len(data)))

    def close(self):
        if self._h:
            h, self._h = self._h, C.c_void_p()
            self._fn("close")(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

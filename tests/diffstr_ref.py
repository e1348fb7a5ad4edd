"""The three per-base difference strings of an alignment record, restated in Python from write_MD_core / write_cs_core /
write_cs_or_MD (LR/format.c:150-268), plus what the tests of the device path need around them: records from golden SAM / PAF lines, the
packed reference, the flat arrays of the host emulator (tests/emul/diffstr_emul.cpp) and the synthetic record set.
The restatement is pinned by tests/test_diffstr.py on every tag the reference printed (tests/golden/tags/); for the synthetic set it
is the expected value."""
import ctypes as C
import gzip
import hashlib
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TAGS = os.path.join(HERE, "golden", "tags")
MODES = ("md", "cs", "cs_long")
MODE_FLAG = {"md": 0x1000000, "cs": 0x40, "cs_long": 0x40 | 0x800}  # MM_F_OUT_MD, MM_F_OUT_CS, MM_F_OUT_CS_LONG
F_QSTRAND = 0x100000000
NT4 = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    NT4[ord(_c)] = NT4[ord(_c.lower())] = _i
NT4[ord("U")] = NT4[ord("u")] = 3  # seq_nt4_table


def nt4(seq):
    return NT4[np.frombuffer(seq.encode() if isinstance(seq, str) else seq, np.uint8)]


_UP, _LO = np.frombuffer(b"ACGTN", np.uint8), np.frombuffer(b"acgtn", np.uint8)


def _text(tab, codes):
    return tab[codes].tobytes().decode()


def diff_string(mode, cigar, q, t):
    """cigar: [(op, len)]; q / t: nt4 codes of the query / target stretch as write_cs_or_MD lays them out.  The walk of the reference,
    with the identical stretches between two mismatches of an M operation taken in one step."""
    out, qo, to, run = [], 0, 0, 0  # run: l_MD (carried over the record) / l_tmp (per M operation)
    up, lo = "ACGTN", "acgtn"

    def iden(end, n):  # the identity item of cs for the n bases in front of query offset end
        return ":%d" % n if mode == "cs" else "=" + _text(_UP, q[end - n:end])
    for op, n in cigar:
        if op in (0, 7, 8):
            if mode != "md":
                run = 0
            last = 0
            for j in np.nonzero(q[qo:qo + n] != t[to:to + n])[0].tolist():
                run += j - last
                if mode == "md":
                    out.append("%d%s" % (run, up[t[to + j]]))
                else:
                    if run:
                        out.append(iden(qo + j, run))
                    out.append("*%s%s" % (lo[t[to + j]], lo[q[qo + j]]))
                run, last = 0, j + 1
            run += n - last
            if mode != "md" and run:
                out.append(iden(qo + n, run))
            qo, to = qo + n, to + n
        elif op == 1:
            if mode != "md":
                out.append("+" + _text(_LO, q[qo:qo + n]))
            qo += n
        elif op == 2:
            if mode == "md":
                out.append("%d^%s" % (run, _text(_UP, t[to:to + n])))
                run = 0
            else:
                out.append("-" + _text(_LO, t[to:to + n]))
            to += n
        elif op == 3:
            if mode != "md":
                out.append("~%s%s%d%s%s" % (lo[t[to]], lo[t[to + 1]], n, lo[t[to + n - 2]], lo[t[to + n - 1]]))
            to += n
        else:
            raise ValueError(op)
    assert qo == len(q) and to == len(t)
    if mode == "md" and run:
        out.append("%d" % run)
    return "".join(out)


def record_seqs(read4, contig4, qs, qe, rs, re_, rev, qstrand=False):
    """(query, target) codes of a record: LR/format.c:245-259; under qstrand the target is this tree's mm_idx_getseq_rev, which takes
    st / en on the REVERSE strand (LR/index.c:168-181): base j is the complement of contig base len - rs - 1 - j"""
    comp = np.array([3, 2, 1, 0, 4], np.uint8)
    if qstrand:
        q = read4[qs:qe]
        if rev:
            n = len(contig4)
            t = comp[contig4[n - re_:n - rs][::-1]]
        else:
            t = contig4[rs:re_]
        return q, t
    q = comp[read4[qs:qe][::-1]] if rev else read4[qs:qe]
    return q, contig4[rs:re_]


def expected(mode, rec, reads4, contigs4, qstrand=False):
    q, t = record_seqs(reads4[rec["read"]], contigs4[rec["rid"]], rec["qs"], rec["qe"], rec["rs"], rec["re"], rec["rev"], qstrand)
    return diff_string(mode, rec["cigar"], q, t)


_CG = re.compile(r"(\d+)([MIDNSHP=X])")


def parse_cigar(text):
    return [("MIDNSHP=X".index(o), int(n)) for n, o in _CG.findall(text)]


def record_of_sam(fields, read_idx, read_len, rid):
    """the record behind a mapped golden SAM line (clips give qs / qe: LR/format.c:474-480)"""
    cg = parse_cigar(fields[5])
    rev = bool(int(fields[1]) & 16)
    clip0 = cg[0][1] if cg[0][0] in (4, 5) else 0
    clip1 = cg[-1][1] if len(cg) > 1 and cg[-1][0] in (4, 5) else 0
    core = [(o, n) for o, n in cg if o not in (4, 5)]
    qs, qe = (clip1, read_len - clip0) if rev else (clip0, read_len - clip1)
    rs = int(fields[3]) - 1
    re_ = rs + sum(n for o, n in core if o in (0, 2, 3, 7, 8))
    assert qe - qs == sum(n for o, n in core if o in (0, 1, 7, 8))
    return dict(read=read_idx, qs=qs, qe=qe, rs=rs, re=re_, rid=rid, rev=int(rev), cigar=core)


def record_of_paf(fields, read_idx, rid):
    """the record behind a mapped golden PAF line printed WITHOUT --qstrand (columns 8 / 9 are rs / re)"""
    cg = next(x for x in fields if x.startswith("cg:Z:"))[5:]
    return dict(read=read_idx, qs=int(fields[2]), qe=int(fields[3]), rs=int(fields[7]), re=int(fields[8]), rid=rid, rev=int(fields[4] == "-"),
                cigar=parse_cigar(cg))


def tag_rows(name):
    """rows of tests/golden/tags/<name>.tsv.gz; the last column is the tag text ("" = none, "#<len>:<sha1>" = digested)"""
    return [l.rstrip("\n").split("\t") for l in gzip.open(os.path.join(TAGS, name + ".tsv.gz"), "rt")]


def same_tag(got, want):
    if want.startswith("#"):
        return want == "#%d:%s" % (len(got), hashlib.sha1(got.encode()).hexdigest())
    return got == want


def pack_reference(contigs4):
    """(S words, offsets, lengths) as mm_idx_t holds them: 4 bits per base, contigs back to back (LR/index.c:380-400)"""
    lens = np.array([len(c) for c in contigs4], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))]).astype(np.uint64)
    flat = np.concatenate(contigs4).astype(np.uint32) if len(contigs4) else np.zeros(0, np.uint32)
    pad = np.zeros((-len(flat)) % 8 + 8, np.uint32)
    flat = np.concatenate([flat, pad]).reshape(-1, 8)
    S = np.zeros(len(flat), np.uint32)
    for k in range(8):
        S |= flat[:, k] << np.uint32(4 * k)
    return S, offs[:-1].copy(), lens


class Rec(C.Structure):  # GddRec of map_diffstr.h
    _fields_ = [(n, C.c_int32) for n in ("read", "qs", "qe", "rs", "re", "rid", "rev")] + [("n_cigar", C.c_uint32), ("cig_off", C.c_int64)]


def flat_records(recs):
    arr = (Rec * max(1, len(recs)))()
    words = []
    for i, r in enumerate(recs):
        arr[i] = Rec(r["read"], r["qs"], r["qe"], r["rs"], r["re"], r["rid"], r["rev"], len(r["cigar"]), len(words))
        words += [n << 4 | o for o, n in r["cigar"]]
    return arr, np.array(words + [0], np.uint32)


class Emulator:
    """tests/emul/diffstr_emul.cpp: map_diffstr.h compiled for the host, count pass and write pass on 64 emulated lanes"""

    def __init__(self, root, tmp_path):
        so = os.path.join(str(tmp_path), "diffstr_emul.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(root, "genome-on-diet_amd", "csrc"),
                               os.path.join(root, "tests", "emul", "diffstr_emul.cpp"), "-o", so])
        self.lib = C.CDLL(so)
        vp = C.c_void_p
        self.lib.diffstr_emul.argtypes = [C.c_int64, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp]
        self.lib.diffstr_emul.restype = C.c_int64
        self.lib.diffstr_check.argtypes = [C.c_int64, vp, vp, vp, vp, C.c_uint32, C.c_int]
        self.lib.diffstr_check.restype = C.c_int64

    def run(self, recs, reads4, contigs4, mode, qstrand=False):
        """every record's string; raises if a pass of the emulator found a lane out of step, a byte written twice or not at all, or a
        store outside the record's counted slice"""
        arr, words = flat_records(recs)
        reads = np.concatenate(list(reads4) + [np.zeros(8, np.uint8)]).astype(np.uint8)
        roff = np.concatenate([[0], np.cumsum([len(r) for r in reads4])]).astype(np.int64)
        S, offs, lens = pack_reference(contigs4)
        n = len(recs)
        bad = self.lib.diffstr_check(n, C.addressof(arr), words.ctypes.data, roff.ctypes.data, lens.ctypes.data, len(lens), int(mode != "md"))
        assert bad == -1, "record %d fails the host check" % bad
        off = np.zeros(n + 1, np.int64)
        a = (n, C.addressof(arr), words.ctypes.data, reads.ctypes.data, roff.ctypes.data, S.ctypes.data, offs.ctypes.data, lens.ctypes.data,
             MODES.index(mode), int(qstrand), off.ctypes.data)
        rc = self.lib.diffstr_emul(*a, None)
        assert rc == 0, "count pass: %d" % rc
        text = np.zeros(int(off[n]) + 1, np.uint8)
        rc = self.lib.diffstr_emul(*a, text.ctypes.data)
        assert rc == 0, "write pass: %d" % rc
        raw = text.tobytes()
        return [raw[off[i]:off[i + 1]].decode() for i in range(n)]

    def check(self, recs, read_lens, contig_lens, cs):
        """index of the first record the host check refuses, -1 if none"""
        arr, words = flat_records(recs)
        roff = np.concatenate([[0], np.cumsum(read_lens)]).astype(np.int64)
        lens = np.array(contig_lens, np.uint32)
        return self.lib.diffstr_check(len(recs), C.addressof(arr), words.ctypes.data, roff.ctypes.data, lens.ctypes.data, len(lens), int(cs))


# ---- the synthetic set: where this kernel can go wrong --------------------------------------------------------------------------
def synthetic_set(seed=5):
    """(contigs4, reads4, recs, notes): a 3-contig reference of a few kbp (the first contig's length is odd, so the second one starts at
    an odd offset, i.e. in the upper half of a byte of S; the last record ends on the last base of the last contig) and hand-built records whose
    reads are made FROM the target stretch through the CIGAR, with mismatches placed where the notes say.  < 100 records."""
    rng = np.random.default_rng(seed)
    contigs = [rng.integers(0, 4, n).astype(np.uint8) for n in (12345, 4097, 14001)]
    contigs[0][3000:3040] = 4  # an N run in the reference
    reads, recs, notes = [], [], []
    comp = np.array([3, 2, 1, 0, 4], np.uint8)

    def other(c):  # a base that differs from c (a code 0..3 for N too)
        return np.uint8((int(c) + 1 + int(rng.integers(0, 3))) % 4) if c < 4 else np.uint8(rng.integers(0, 4))

    def add(note, rid, rs, cigar, mism=(), rev=0, qn=(), lead=0, trail=0):
        """cigar: [(op, len)]; mism: query offsets (within the aligned stretch) to make mismatches; qn: query offsets set to N"""
        t = contigs[rid]
        q, to = [], rs
        for op, n in cigar:
            if op in (0, 7, 8):
                q.append(t[to:to + n].copy())
                to += n
            elif op == 1:
                q.append(rng.integers(0, 4, n).astype(np.uint8))
            else:
                to += n
        q = np.concatenate(q) if q else np.zeros(0, np.uint8)
        for p in mism:
            q[p] = other(q[p])
        for p in qn:
            q[p] = 4
        assert to <= len(t)
        body = comp[q[::-1]] if rev else q
        read = np.concatenate([rng.integers(0, 4, lead).astype(np.uint8), body, rng.integers(0, 4, trail).astype(np.uint8)])
        recs.append(dict(read=len(reads), qs=lead, qe=lead + len(q), rs=rs, re=to, rid=rid, rev=rev, cigar=list(cigar)))
        reads.append(read)
        notes.append(note)

    for n in (1, 63, 64, 65, 127, 128, 129):  # M operations around the 64-lane round
        add("M%d clean" % n, 0, 100 + n, [(0, n)])
        add("M%d mismatches at both ends" % n, 0, 500 + n, [(0, n)], mism=sorted({0, n - 1}))
    add("run carried across a round seam", 0, 1000, [(0, 200)], mism=[30, 100])
    add("mismatches in lanes 0 and 63 and in adjacent lanes", 0, 1300, [(0, 192)], mism=[0, 63, 64, 65, 66, 127, 128, 191])
    add("MD run carried across an insertion and two M operations; cs run not carried", 0, 1600, [(0, 50), (1, 3), (0, 40), (0, 30)], mism=[10])
    for n in (9, 10, 99, 100, 999, 1000, 9999, 10000):  # digit counts
        add("run of %d then a mismatch" % n, 2, 7, [(0, n + 5)], mism=[n])
        add("run of %d closing the record" % n, 2, 11, [(0, n + 1)], mism=[0])
    add("mismatch directly behind a deletion", 0, 2000, [(0, 20), (2, 5), (0, 20)], mism=[20])
    add("record ending in a mismatch", 0, 2100, [(0, 70)], mism=[69])
    add("record that is one mismatch", 0, 2200, [(0, 1)], mism=[0])
    for n in (1, 64, 65):
        add("deletion of %d" % n, 1, 300, [(0, 33), (2, n), (0, 33)], mism=[40])
        add("insertion of %d" % n, 1, 700, [(0, 33), (1, n), (0, 33)], mism=[5])
    add("N operation", 1, 1000, [(0, 40), (3, 120), (0, 40)], mism=[3, 50])
    add("N operation of 2", 1, 1300, [(0, 10), (3, 2), (0, 10)])
    # an N operation in front, at base 0 of S: nothing of the record lies in front of its last two bases (they must not be named by an
    # offset that is negative from the start of S)
    add("N of 2 first, at base 0 of the first contig", 0, 0, [(3, 2), (0, 10)], mism=[4])
    add("N of 3 first, at base 0 of the first contig", 0, 0, [(3, 3), (0, 10)])
    add("1M 2N at base 0 of the first contig", 0, 0, [(0, 1), (3, 2), (0, 5)], mism=[0])
    add("N of 2 first, at base 0, reverse strand", 0, 0, [(3, 2), (0, 70)], mism=[69], rev=1)
    add("N last, on the last base of the last contig", 2, len(contigs[2]) - 12, [(0, 10), (3, 2)])
    for k in range(8):  # rs at every residue mod 8 of the S words, contig 0 (offset 0) and contig 1 (odd offset)
        add("rs = %d mod 8" % k, 0, 4000 + k, [(0, 70)], mism=[1, 68])
        add("rs = %d mod 8, odd contig offset" % k, 1, 2000 + k, [(0, 70), (2, 3), (0, 9)], mism=[1, 68])
    add("N in the target", 0, 2990, [(0, 70)], mism=[15, 20])
    add("N in the query", 0, 2400, [(0, 70)], qn=[0, 33, 69])
    add("N on both sides (equal codes)", 0, 2995, [(0, 60)], qn=[0, 50])
    add("reverse strand", 2, 5000, [(0, 100), (1, 4), (0, 100), (2, 6), (0, 100)], mism=[0, 99, 150, 299], rev=1, lead=13, trail=7)
    add("reverse strand with N on both sides", 0, 2980, [(0, 80)], qn=[1, 30], rev=1, lead=5)
    add("reverse strand, one base", 1, 50, [(0, 1)], rev=1)
    add("operations 7 / 8", 1, 3000, [(7, 30), (8, 1), (7, 64), (8, 2), (7, 10)], mism=[30, 95, 96])
    add("insertion first, deletion last", 1, 3300, [(1, 2), (0, 64), (2, 2)], mism=[63])
    add("soft ends: the record covers the middle of its read", 2, 9000, [(0, 130)], mism=[64], lead=40, trail=40)
    n_last = len(contigs[2])
    add("ends on the last base of the last contig", 2, n_last - 131, [(0, 64), (2, 3), (0, 64)], mism=[127])
    add("ends on the last base of the last contig, reverse", 2, n_last - 65, [(0, 65)], mism=[0, 64], rev=1)
    assert len(recs) < 100
    return contigs, reads, recs, notes

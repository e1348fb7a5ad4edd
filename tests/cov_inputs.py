"""Inputs of the coverage tests (CPU and GPU): hand-built BAM records at the edges of the accumulator -- the blocks of four wavefronts, the
round carry of the two scans, the ends of the difference array, contention, qualities, the placeholder CIGAR, the filters, chunk and
window borders -- and the golden SAM lines as records (bam_ref.encode_record, as bam_sort_inputs makes them)."""
import random
import struct

import numpy as np

import bam_ref
import os

from fixture_io import SETS, golden_sam, read_fasta

REFS = ["c0", "one", "c2", "c3", "long"]
REF_LENS = [300, 1, 257, 500, 6000]  # a one-base contig between two others; 7058 positions in all
OPS = "MIDNSHP=X"
GOLDEN = ("hifi_sv", "ont_sv", "sr", "hifi_edge")  # (hifi_edge: the golden edge_hifi)


def rec(ref_id, pos, ops, flag=0, mapq=30, l_seq=None, qual="random", aux=b"", name=b"r", seed=0, words=None):
    """one record from numbers: ops = [(length, letter or code)]; l_seq defaults to what the operations consume of the query; qual is
    "random" (seeded bytes below 94), None (0xff), or bytes; `words`, if given, is the CIGAR field instead of ops (a placeholder)"""
    code = lambda o: o if isinstance(o, int) else OPS.index(o)
    w = [n << 4 | code(o) for n, o in ops] if words is None else list(words)
    if l_seq is None:
        l_seq = sum(n for n, o in ops if code(o) in (0, 1, 4, 7, 8))
    if qual == "random":
        q = bytes(np.random.default_rng(seed + 7 * l_seq).integers(0, 94, l_seq, dtype=np.uint8))
    else:
        q = b"\xff" * l_seq if qual is None else bytes(qual)
    assert len(q) == l_seq
    nm = name + b"\0"
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(nm), mapq, 0, len(w), flag, l_seq, -1, -1, 0) + nm + struct.pack("<%dI" % len(w), *w)
    body += bytes((l_seq + 1) // 2) + q + aux
    return struct.pack("<i", len(body)) + body


def pool():
    """simple valid records on every contig"""
    out = []
    for k in range(40):
        rid = (0, 2, 3, 4)[k % 4]
        n = 5 + 3 * (k % 7)
        out.append(rec(rid, (11 * k) % (REF_LENS[rid] - 40), [(2, "S"), (n, "M"), (1, "I"), (2, "D"), (n, "=")], flag=16 * (k % 2), mapq=k, seed=k, name=b"p%d" % k))
    out.append(rec(1, 0, [(1, "M")], name=b"one"))
    return out


def counted(n):
    p = pool()
    rng = random.Random(100 + n)
    return [p[rng.randrange(len(p))] for _ in range(n)]


def ops_record(k, rid=3, pos=7):
    """k operations, every code in turn; lengths 1 and 2: the reference length of 129 of them stays below 500"""
    return rec(rid, pos, [(1 + i % 2, OPS[i % 9]) for i in range(k)], seed=k, name=b"ops%d" % k)


def ops_sets():
    return {k: [ops_record(k), ops_record(1, rid=0, pos=0)] for k in (0, 1, 63, 64, 65, 129)}


def edge_set(next_covered):
    n0, last = REF_LENS[0], len(REF_LENS) - 1
    out = [rec(0, n0 - 20, [(20, "M")], name=b"to_end"), rec(0, 0, [(3, "M")], name=b"pos0"), rec(last, REF_LENS[last] - 9, [(9, "X")], name=b"last_end"),
           rec(-1, -1, [(10, "M")], flag=4, name=b"unplaced_cigar"), rec(-1, 5, [(10, "M")], flag=0, name=b"no_ref_cigar"), rec(2, 0, [(REF_LENS[2], "M")], name=b"whole")]
    if next_covered:
        out.append(rec(1, 0, [(1, "M")], name=b"one_base"))
    return out


BAD = {  # name -> (record, reason as cov_ref names it)
    "op9": (rec(3, 5, [(4, "M"), (3, 9), (4, "M")], l_seq=8, name=b"op9"), "op"),
    "past_end": (rec(0, REF_LENS[0] - 20, [(21, "M")], name=b"past"), "ref_end"),
    "past_end_by_D": (rec(0, REF_LENS[0] - 20, [(20, "M"), (1, "D")], name=b"pastd"), "ref_end"),
    "ref_n": (rec(len(REF_LENS), 0, [(1, "M")], name=b"refn"), "ref"),
    "pos_neg": (rec(0, -1, [(1, "M")], name=b"posneg"), "pos"),
    "query_past": (rec(0, 0, [(5, "M"), (3, "S")], l_seq=7, name=b"qpast"), "qry_end"),
    "placeholder_bare": (rec(3, 5, [], l_seq=6, words=[6 << 4 | 4, 30 << 4 | 3], aux=b"XAAx", name=b"bare"), "cg"),
    "placeholder_cg_Z": (rec(3, 5, [], l_seq=6, words=[6 << 4 | 4, 30 << 4 | 3], aux=b"CGZabc\0", name=b"cgz"), "cg"),
    "placeholder_cg_cut": (rec(3, 5, [], l_seq=6, words=[6 << 4 | 4, 30 << 4 | 3], aux=b"CGBI" + struct.pack("<iI", 2, 6 << 4), name=b"cut"), "cg"),
    "placeholder_aux_leaves": (rec(3, 5, [], l_seq=6, words=[6 << 4 | 4, 30 << 4 | 3], aux=b"XZZno_nul", name=b"leaves"), "aux"),
    "placeholder_aux_type": (rec(3, 5, [], l_seq=6, words=[6 << 4 | 4, 30 << 4 | 3], aux=b"XQq1", name=b"type"), "aux"),
}


def with_bad(name, at=3, n=9):
    """n valid records with the bad one at place `at`"""
    out = counted(n)
    out.insert(at, BAD[name][0])
    return out


def contention_sets():
    one = rec(0, 100, [(50, "M")], seed=1, name=b"copy")
    long_run = rec(4, 100, [(1, "M"), (1, "D")] * 64 + [(5000, "M")], seed=2, name=b"long")
    return {"copies": [one] * 1000,
            "strands": [rec(2, 40, [(30, "M")], flag=0, name=b"fwd"), rec(2, 40, [(30, "M")], flag=16, name=b"rev")],
            "long_quality_run": [long_run, rec(4, 4000, [(1, "M"), (1, "I")] * 64, seed=3, name=b"ones")]}


def quality_set():
    return [rec(0, 10, [(20, "M")], l_seq=0, name=b"no_seq"), rec(0, 12, [(20, "M")], qual=None, name=b"no_qual"),
            rec(0, 14, [(5, "S"), (20, "M"), (7, "S")], seed=4, name=b"soft"), rec(0, 16, [(5, "H"), (20, "M"), (7, "H")], seed=5, name=b"hard"),
            rec(0, 18, [(3, "H"), (2, "S"), (9, "M"), (2, "P"), (4, "I"), (9, "M"), (1, "S"), (6, "H")], seed=6, name=b"both"),
            rec(0, 20, [(20, "M")], qual=bytes([0] + [93] * 19), name=b"q0_first")]


def placeholder_set():
    """the real CIGAR in CG:B:I behind aux fields of every type; the N of the field says something else on purpose"""
    every = (b"XAAq" + b"Xcc\xfe" + b"XCC\x07" + b"Xss\x00\x80" + b"XSS\xff\xff" + b"Xii" + struct.pack("<i", -5) + b"XII" + struct.pack("<I", 7) + b"Xff" + struct.pack("<f", 1.5)
             + b"XZZtext\0" + b"XHH1AE3\0" + b"XBBs" + struct.pack("<ihh", 2, -1, 2) + b"XDBf" + struct.pack("<if", 1, 2.0) + b"XEBC" + struct.pack("<i", 0))
    real = [(3, "S"), (10, "M"), (2, "I"), (5, "D"), (8, "="), (4, "N"), (6, "X"), (1, "S")]
    l_seq = 3 + 10 + 2 + 8 + 6 + 1
    cg = b"CGBI" + struct.pack("<i%dI" % len(real), len(real), *[n << 4 | OPS.index(o) for n, o in real])
    words = [l_seq << 4 | 4, 400 << 4 | 3]
    return [rec(3, 50, [], l_seq=l_seq, words=words, aux=every + cg + b"rlC\x09", seed=8, name=b"placeholder"),
            rec(3, 60, [], l_seq=l_seq, words=words, aux=cg, seed=9, name=b"cg_first"),
            rec(3, 70, [(l_seq, "S"), (40, "D")], l_seq=l_seq, seed=10, name=b"S_then_D_is_no_placeholder"),
            rec(3, 80, [(l_seq - 1, "S"), (40, "N")], l_seq=l_seq, seed=11, name=b"shorter_S_is_no_placeholder")]


def filter_set():
    out = []
    for k, (flag, mapq) in enumerate([(0, 0), (0, 1), (0, 60), (0, 61), (0, 255), (16, 30), (4, 0), (4 | 16, 0), (0x100, 30), (0x100 | 16, 2), (0x800, 30), (0x800 | 16, 0), (0x900, 9),
                                      (0x200, 30), (0x400, 30), (0x400 | 0x100, 30), (1 | 2 | 0x40, 30), (4 | 0x100, 0)]):
        out.append(rec(k % 3 + 2, 10 + k, [(15, "M")], flag=flag, mapq=mapq, seed=k, name=b"f%d" % k))
    out.append(rec(-1, -1, [], flag=4, mapq=0, l_seq=5, name=b"unmapped"))
    out.append(rec(-1, -1, [], flag=0, mapq=70, l_seq=5, name=b"unplaced_passing"))
    return out


FILTERS = [(e, q) for e in (0, 0x704, 0x900) for q in (0, 1, 61)]


def border_set():
    """a run across every border of a chunk of 7 and of 256 slots, on every contig: a 10M every 3 positions"""
    out = []
    for rid, n in enumerate(REF_LENS[:4]):
        out += [rec(rid, p, [(min(10, n - p), "M")], seed=p, name=b"b") for p in range(0, n, 3)]
    out += [rec(4, p, [(40, "M"), (20, "D"), (40, "=")], seed=p, name=b"bl") for p in range(0, 5900, 37)]
    out.append(rec(4, 5900, [(100, "X")], seed=1, name=b"tail"))
    return out


CHUNKS = (1, 7, 256, 1 << 20)
WINDOWS = (1, 63, 64, 65, 299, 300, 7000)  # larger than a contig, dividing one, not dividing any


_golden = {}


def golden_records(kind):
    """(records of the kind's golden SAM lines in file order, contig names and lengths of its reference, the lines)"""
    if kind not in _golden:
        names, seqs = read_fasta(os.path.join(SETS[kind][0], "ref.fa.gz"))
        lines = golden_sam(kind)
        _golden[kind] = ([bam_ref.encode_record(l, names) for l in lines], names, [len(x) for x in seqs], lines)
    return _golden[kind]


def designed():
    """name -> records: every valid designed set"""
    out = {"count%d" % n: counted(n) for n in (0, 1, 3, 4, 5, 63, 64, 65, 257)}
    out.update({"ops%d" % k: v for k, v in ops_sets().items()})
    out.update(edges_covered=edge_set(True), edges_uncovered=edge_set(False), quality=quality_set(), placeholder=placeholder_set(), filters=filter_set(), borders=border_set())
    out.update(contention_sets())
    return out

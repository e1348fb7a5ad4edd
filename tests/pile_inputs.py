"""Inputs of the pileup tests (CPU and GPU): hand-built BAM records with a SEQ of their own (cov_inputs.rec writes zero nibbles) over the
designed reference of the coverage tests -- cov_inputs.REFS / REF_LENS, 7 058 positions with a one-base contig, the bases those of the
seeded strings test_coverage_gpu.small builds its mapper from, so that every reference base is known here.  A designed case is
(records, regions or None, min_baseq)."""
import struct

import numpy as np

import cov_inputs as ci

REFS, REF_LENS, OPS = ci.REFS, ci.REF_LENS, ci.OPS
NIBBLES = "=ACMGRSVTWYHKDBN"  # the SEQ codes 0..15
CALL_OPT = dict(min_depth=4, min_alt=2, frac=(1, 5))  # the options the call set is designed for


def ref_seqs():
    rng = np.random.default_rng(5)
    return ["".join("ACGT"[c] for c in rng.integers(0, 4, n)) for n in REF_LENS]


REF_SEQS = ref_seqs()
REF_N = ["withN"], ["".join("ACGT"[c] for c in np.random.default_rng(6).integers(0, 4, 50)) + "N" + "".join("ACGT"[c] for c in np.random.default_rng(7).integers(0, 4, 149))]


def rec(ref_id, pos, ops, seq=None, flag=0, mapq=30, l_seq=None, qual="random", aux=b"", name=b"r", seed=0, words=None):
    """one record from numbers: ops = [(length, letter or code)]; seq: a string over NIBBLES (default: seeded A C G T); l_seq defaults to
    what the operations consume of the query; qual is "random" (seeded bytes below 94), None (0xff) or bytes; `words`, if given, is the
    CIGAR field instead of ops (a placeholder)"""
    code = lambda o: o if isinstance(o, int) else OPS.index(o)
    w = [n << 4 | code(o) for n, o in ops] if words is None else list(words)
    if l_seq is None:
        l_seq = len(seq) if seq is not None else sum(n for n, o in ops if code(o) in (0, 1, 4, 7, 8))
    if seq is None:
        seq = "".join("ACGT"[c] for c in np.random.default_rng(1000 + seed + 3 * l_seq).integers(0, 4, l_seq))
    assert len(seq) == l_seq
    nib = [NIBBLES.index(c) for c in seq] + [0]
    packed = bytes(nib[2 * k] << 4 | nib[2 * k + 1] for k in range((l_seq + 1) // 2))
    if qual == "random":
        q = bytes(np.random.default_rng(seed + 7 * l_seq).integers(0, 94, l_seq, dtype=np.uint8))
    else:
        q = b"\xff" * l_seq if qual is None else bytes(qual)
    assert len(q) == l_seq
    nm = name + b"\0"
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(nm), mapq, 0, len(w), flag, l_seq, -1, -1, 0) + nm + struct.pack("<%dI" % len(w), *w)
    return struct.pack("<i", len(body) + len(packed) + len(q) + len(aux)) + body + packed + q + aux


def case(recs, regions=None, min_baseq=0):
    return dict(recs=list(recs), regions=regions, min_baseq=min_baseq)


def pool():
    out = []
    for k in range(40):
        rid = (0, 2, 3, 4)[k % 4]
        n = 5 + 3 * (k % 7)
        out.append(rec(rid, (11 * k) % (REF_LENS[rid] - 40), [(2, "S"), (n, "M"), (1, "I"), (2, "D"), (n, "=")], flag=16 * (k % 2), mapq=k, seed=k, name=b"p%d" % k))
    out.append(rec(1, 0, [(1, "M")], name=b"one"))
    return out


def counted(n):
    p = pool()
    rng = np.random.default_rng(100 + n)
    return [p[int(rng.integers(len(p)))] for _ in range(n)]


def ops_record(k, rid=3, pos=7):
    """k operations, every code in turn; lengths 1 and 2"""
    return rec(rid, pos, [(1 + i % 2, OPS[i % 9]) for i in range(k)], seed=k, name=b"ops%d" % k)


def run_record(n):
    return rec(4, 17, [(n, "M")], seed=n, name=b"run%d" % n)


def quality_recs():
    """qualities exactly at, one below and one above every threshold of the quality cases, and a record without qualities"""
    q = bytes([0, 1, 2, 19, 20, 21, 93, 93, 20, 0])
    return [rec(0, 30, [(10, "M")], qual=q, name=b"edges"), rec(0, 32, [(10, "M")], qual=None, name=b"no_qual"), rec(0, 34, [(3, "S"), (7, "M")], qual=q, flag=16, name=b"edges_rev"),
            rec(0, 36, [(10, "M")], qual=bytes([94] * 10), name=b"all94")]


def clip_recs():
    """an odd and an even soft clip: the run starts on either nibble half; odd and even lengths end on either"""
    return [rec(2, 10 + 7 * k, [(s, "S"), (n, "M")], seed=k, name=b"clip%d" % k) for k, (s, n) in enumerate([(0, 4), (1, 4), (2, 5), (3, 5), (1, 1), (0, 1), (5, 64), (4, 65)])]


def ins_recs():
    n0 = REF_LENS[0]
    return [rec(0, 50, [(3, "I"), (10, "M")], name=b"I_first"), rec(0, 60, [(2, "S"), (3, "I"), (10, "M")], name=b"I_after_S"), rec(0, 70, [(5, "M"), (3, "I"), (5, "M")], name=b"I_after_M"),
            rec(0, n0 - 5, [(5, "M"), (2, "I")], name=b"I_at_last_base"), rec(0, 80, [(2, "D"), (1, "I"), (4, "M")], name=b"I_after_D"),
            rec(0, 195, [(5, "M"), (2, "I"), (5, "M")], name=b"I_anchor_199"), rec(0, 196, [(5, "M"), (2, "I"), (5, "M")], name=b"I_anchor_200")]


INS_REGIONS = [(0, 0, 199), (0, 201, 300)]  # anchor 199 lies outside by one base, anchor 200 likewise; 198 and 201 are not anchors
BORDER_REGIONS = [(3, 100, 110), (3, 110, 120), (3, 130, 131), (3, 140, 150), (4, 0, 6000)]  # abutting, a gap, one base, a gap


def border_recs():
    return [rec(3, 95, [(8, "M"), (20, "D"), (8, "M")], name=b"D_across"), rec(3, 98, [(4, "M"), (30, "N"), (10, "M")], name=b"N_across"),
            rec(3, 90, [(70, "M")], name=b"three_regions_two_gaps"), rec(3, 105, [(10, "X")], flag=16, name=b"abutting"), rec(3, 200, [(30, "M")], name=b"outside"),
            rec(2, 10, [(30, "M")], name=b"other_contig"), rec(3, 129, [(3, "=")], name=b"one_base")]


def placeholder_recs():
    every = b"XAAq" + b"Xss\x00\x80" + b"XZZtext\0" + b"XBBs" + struct.pack("<ihh", 2, -1, 2)
    real = [(3, "S"), (10, "M"), (2, "I"), (5, "D"), (8, "="), (4, "N"), (6, "X"), (1, "S")]
    l_seq = 3 + 10 + 2 + 8 + 6 + 1
    cg = b"CGBI" + struct.pack("<i%dI" % len(real), len(real), *[n << 4 | OPS.index(o) for n, o in real])
    words = [l_seq << 4 | 4, 400 << 4 | 3]
    return [rec(3, 50, [], l_seq=l_seq, words=words, aux=every + cg + b"rlC\x09", seed=8, name=b"placeholder"), rec(3, 60, [], l_seq=l_seq, words=words, aux=cg, seed=9, flag=16, name=b"cg_first"),
            rec(3, 70, [(l_seq, "S"), (40, "D")], l_seq=l_seq, seed=10, name=b"S_then_D_is_no_placeholder")]


def no_seq_recs():
    return [rec(0, 10, [(20, "M")], l_seq=0, name=b"no_seq"), rec(0, 10, [(20, "M")], l_seq=0, flag=0x100, name=b"no_seq_secondary"), rec(-1, -1, [], l_seq=0, name=b"no_seq_unplaced"),
            rec(0, 12, [(5, "M"), (2, "D"), (5, "M")], name=b"with_seq")]


def stack(rid, pos, bases, name=b"s", **kw):
    """one 1M record per base of the string `bases`, all at pos"""
    return [rec(rid, pos, [(1, "M")], seq=b, name=name, **kw) for b in bases]


def call_set(seqs=None, rid=3):
    """(records, {kind: (rid, pos, is a site, alt or None)}): under CALL_OPT every kind of site and of near miss the header names"""
    ref = (seqs or REF_SEQS)[rid]
    other = lambda p, k=0: [b for b in "ACGT" if b != ref[p]][k]
    recs, want = [], {}

    def put(kind, p, bases, site, alt=None, extra=()):
        recs.extend(stack(rid, p, bases))
        recs.extend(extra)
        want[kind] = (rid, p, site, alt)

    put("snv_at_min_alt", 10, ref[10] * 8 + other(10) * 2, True, "ACGT".index(other(10)))            # 2 of 10: 2 * 5 >= 1 * 10
    put("snv_below_min_alt", 20, ref[20] * 4 + other(20), False)                                       # 1 of 5: the fraction holds, min_alt does not
    put("at_fraction", 30, ref[30] * 12 + other(30) * 3, True, "ACGT".index(other(30)))               # 3 of 15: 15 >= 15
    put("below_fraction", 40, ref[40] * 13 + other(40) * 3, False)                                     # 3 of 16: 15 < 16
    put("del", 50, "", True, 4, extra=[rec(rid, 48, [(2, "M"), (1, "D"), (2, "M")], seq=ref[48:50] + ref[51:53], name=b"d")] * 5 + [rec(rid, 48, [(5, "M")], seq=ref[48:53], name=b"m")] * 5)
    put("ins_only", 62, "", True, 5, extra=[rec(rid, 60, [(3, "M"), (2, "I"), (3, "M")], seq=ref[60:63] + "GG" + ref[63:66], name=b"i")] * 4 + [rec(rid, 60, [(6, "M")], seq=ref[60:66], name=b"n")] * 4)
    put("tie", 70, ref[70] * 2 + other(70, 0) * 4 + other(70, 1) * 4, True, "ACGT".index(other(70, 0)))
    put("depth_at_min_depth", 80, ref[80] * 2 + other(80, 2) * 2, True, "ACGT".index(other(80, 2)))
    put("depth_below_min_depth", 90, ref[90] + other(90) * 2, False)
    return recs, want


def call_set_n():
    """the call set's site at a reference N, over REF_N: six A on the N, a plain column beside it"""
    return stack(0, 50, "AAAAAA") + stack(0, 52, REF_N[1][0][52] * 6), {"ref_n": (0, 50, True, 0), "plain": (0, 52, False, None)}


def designed():
    """name -> case: every valid designed set"""
    out = {"count%d" % n: case(counted(n)) for n in (0, 1, 3, 4, 5, 63, 64, 65, 257)}
    out.update({"ops%d" % k: case([ops_record(k), ops_record(1, rid=0, pos=0)]) for k in (0, 1, 63, 64, 65, 129)})
    out.update({"run%d" % n: case([run_record(n)]) for n in (1, 63, 64, 65, 129, 5000)})
    out["nibbles"] = case([rec(2, 100, [(16, "M")], seq=NIBBLES, name=b"nib"), rec(2, 101, [(1, "S"), (15, "M")], seq=NIBBLES, flag=16, name=b"nib_rev")])
    out.update({"baseq%d" % q: case(quality_recs(), min_baseq=q) for q in (0, 1, 20, 94)})
    out["clips"] = case(clip_recs())
    out["ins"] = case(ins_recs())
    out["ins_regions"] = case(ins_recs(), INS_REGIONS)
    out["borders"] = case(border_recs(), BORDER_REGIONS)
    out["borders_whole"] = case(border_recs())
    out["one_base_region"] = case(border_recs() + counted(20), [(1, 0, 1), (3, 129, 130)])
    out["copies"] = case([rec(0, 100, [(50, "M")], seed=1, flag=16, name=b"copy")] * 1000)
    out["strands"] = case([rec(2, 40, [(30, "M")], seed=3, flag=0, name=b"fwd"), rec(2, 40, [(30, "M")], seed=3, flag=16, name=b"rev")])
    out["long"] = case([rec(4, 100, [(1, "M"), (1, "D")] * 64 + [(5000, "M")], seed=2, name=b"long"), rec(4, 4000, [(1, "M"), (1, "I")] * 64, seed=3, name=b"ones")], min_baseq=10)
    out["placeholder"] = case(placeholder_recs())
    out["cov_filters"] = case(ci.filter_set())
    out["cov_quality"] = case(ci.quality_set(), min_baseq=30)
    out["no_seq"] = case(no_seq_recs())
    out["calls"] = case(call_set()[0])
    return out

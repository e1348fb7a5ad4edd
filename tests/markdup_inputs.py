"""Inputs of the duplicate-marking tests (CPU and GPU): hand-built BAM records (cov_inputs.rec) at the edges of the key pass -- the blocks of
four wavefronts, the clip runs on both strands, the rounds of 64 CIGAR words, the placeholder CIGAR, the dword split of the QUAL sum,
eligibility, the tie-break -- and the doubled goldens of the sorter tests."""
import random
import struct

import numpy as np

from cov_inputs import rec

OPS = "MIDNSHP=X"
COUNTS = (0, 1, 2, 63, 64, 65, 257)


def quals(n, seed):
    """n quality bytes on both sides of 15"""
    return bytes(np.random.default_rng(seed).integers(0, 41, n, dtype=np.uint8))


def simple(k, rid, pos, rev=False, n=20, flag=0, name=None, qual=None):
    return rec(rid, pos, [(n, "M")], flag=flag | (16 if rev else 0), qual=quals(n, k) if qual is None else qual, name=name or b"s%d" % k)


def counted(n):
    """n records on twenty sites of both strands: groups of every small size, and single records"""
    rng = random.Random(300 + n)
    return [simple(k, rng.randrange(3), 100 + 7 * rng.randrange(10), rev=rng.random() < 0.5, name=b"c%d" % k) for k in range(n)]


def group_sizes():
    """groups of 1, 2, 64 and 65 members, shuffled: the winner is anywhere in the buffer"""
    out = []
    for g, size in enumerate((1, 2, 64, 65)):
        out += [simple(1000 * g + k, 1, 500 + 50 * g, rev=bool(g & 1), name=b"g%d_%d" % (size, k)) for k in range(size)]
    random.Random(4).shuffle(out)
    return out


def one_group(n=257):
    return [simple(k, 0, 1234, name=b"all%d" % k) for k in range(n)]


def alignments():
    """names of 1 .. 8 letters: record starts, and QUAL fields, at all four alignments mod 4"""
    out = [simple(k, 2, 40 + (k % 3), n=9 + k % 5, name=b"n" * (1 + k % 8)) for k in range(32)]
    at, seen = 0, set()
    for r in out:
        seen.add(at % 4)
        at += len(r)
    assert seen == {0, 1, 2, 3}
    return out


def clip_cases():
    """forward: none, S, H, H+S in front; reverse: none, S, H, S+H behind.  `apart`: equal pos, unequal clips, no two group.  `together`:
    unequal pos, equal u, one group per strand -- the reverse one with a member whose pos differs through a deletion"""
    fwd = [[], [(3, "S")], [(4, "H")], [(2, "H"), (3, "S")]]
    rev = [[], [(3, "S")], [(4, "H")], [(3, "S"), (2, "H")]]
    clip = lambda ops: sum(n for n, _ in ops)
    apart, together = [], []
    for k, f in enumerate(fwd):
        apart.append(rec(0, 100, f + [(20, "M"), (5, "S")], qual=quals(20 + 5 + sum(n for n, o in f if o == "S"), k), name=b"fa%d" % k))  # (clips behind a forward read say nothing)
        together.append(rec(0, 100 + clip(f), f + [(20, "M")], qual=quals(20 + sum(n for n, o in f if o == "S"), 10 + k), name=b"ft%d" % k))
    for k, r in enumerate(rev):
        apart.append(rec(0, 200, [(6, "S"), (20, "M")] + r, flag=16, qual=quals(26 + sum(n for n, o in r if o == "S"), 20 + k), name=b"ra%d" % k))  # (nor clips in front of a reverse one)
        together.append(rec(0, 200 - clip(r), [(20, "M")] + r, flag=16, qual=quals(20 + sum(n for n, o in r if o == "S"), 30 + k), name=b"rt%d" % k))
    together.append(rec(0, 195, [(10, "M"), (5, "D"), (10, "M")], flag=16, qual=quals(20, 40), name=b"rt_del"))  # ends at 219 like rt0, from another pos
    together.append(rec(0, 219, [(20, "M")], qual=quals(20, 41), name=b"f_at_the_reverse_u"))                    # same u, other strand: a group of its own
    return apart, together


def long_cigars():
    """130 operations, two rounds of 64 words and a rest: the first operation other than S / H at index 70; the last one at index 39 with
    ninety clips behind it; a clip at index 64 and at index 65 behind other operations (the second word of lanes 0 and 1), which belongs
    to no clip run.  Each with a plain mate at the u the rule gives it"""
    lead = [(1 + k % 3, "SH"[k % 2]) for k in range(70)]
    a_ops = lead + [(2, "MI"[k % 2]) for k in range(60)]
    a = rec(1, 5000, a_ops, qual=quals(sum(n for n, o in a_ops if o in "MIS"), 50), name=b"lead70")
    a_mate = simple(51, 1, 5000 - sum(n for n, _ in lead), name=b"lead70_mate")
    trail = [(1 + k % 4, "HS"[k % 2]) for k in range(90)]
    b_ops = [(3, "MD"[k % 2]) for k in range(40)] + trail
    b = rec(1, 6000, b_ops, flag=16, qual=quals(sum(n for n, o in b_ops if o in "MIS"), 52), name=b"trail90")
    b_mate = simple(53, 1, 6000 + 120 - 1 + sum(n for n, _ in trail) - 19, rev=True, name=b"trail90_mate")
    c_ops = [(2, "S")] + [(1, "MI"[k % 2]) for k in range(63)] + [(7, "S"), (9, "H")] + [(1, "M")] * 63 + [(4, "S")]
    c = rec(1, 7000, c_ops, qual=quals(sum(n for n, o in c_ops if o in "MIS"), 54), name=b"wrap_fwd")
    c_mate = simple(55, 1, 7000 - 2, name=b"wrap_fwd_mate")
    d = rec(1, 8000, c_ops, flag=16, qual=quals(sum(n for n, o in c_ops if o in "MIS"), 56), name=b"wrap_rev")
    d_ref = sum(n for n, o in c_ops if o in "MDN=X")
    d_mate = simple(57, 1, 8000 + d_ref - 1 + 4 - 19, rev=True, name=b"wrap_rev_mate")
    assert len(a_ops) == len(b_ops) == len(c_ops) == 130
    return [a, a_mate, b, b_mate, c, c_mate, d, d_mate]


def placeholder():
    """a placeholder record whose real CIGAR is a CG:B:I array of 65 536 operations, on the reverse strand, and its plain mate"""
    real = [(5, "S")] + [(1, "MD"[k % 2]) for k in range(65536 - 2)] + [(3, "S")]
    l_seq = 5 + 32767 + 3
    cg = b"CGBI" + struct.pack("<i%dI" % len(real), len(real), *[n << 4 | OPS.index(o) for n, o in real])
    p = rec(2, 1000, [], flag=16, l_seq=l_seq, words=[l_seq << 4 | 4, 9 << 4 | 3], aux=b"XAAq" + cg, qual=quals(l_seq, 60), name=b"cg65536")
    return [p, simple(61, 2, 1000 + 65534 - 1 + 3 - 19, rev=True, name=b"cg65536_mate")]


QUAL_LENS = (0, 1, 3, 63, 64, 65, 4097)


def qual_cases():
    """one group: QUAL of every length (missing too), values on both sides of 15, 0xff inside, and pairs of equal score"""
    out = []
    for k, n in enumerate(QUAL_LENS):
        out.append(rec(3, 300, [(n, "M")] if n else [], l_seq=n, qual=quals(n, 70 + k), name=b"q%d" % n))
        out.append(rec(3, 300, [(n, "M")] if n else [], l_seq=n, qual=None, name=b"q%d_missing" % n))
    out.append(rec(3, 300, [(8, "M")], qual=bytes([14, 15, 16, 0xff, 14, 40, 0, 15]), name=b"edge_a"))         # 15 + 16 + 40 + 15 = 86
    out.append(rec(3, 300, [(9, "M")], qual=bytes([43, 14, 13, 43, 0xff, 1, 2, 3, 4]), name=b"edge_b_same_score"))  # 86 as well: edge_a comes first
    out.append(rec(3, 300, [(4097, "M")], qual=bytes([40] * 4097), name=b"best"))
    out.append(rec(3, 300, [(4097, "M")], qual=bytes([40] * 4097), name=b"best_again"))  # equal scores: the first in the buffer wins
    return out


INELIGIBLE_FLAGS = (0x4, 0x100, 0x200, 0x800)


def eligibility():
    """at one site: every ineligible flag on its own, refID -1, pos -1, each once with and once without 0x400; an eligible winner that
    carries 0x400 and an eligible loser that does not; an ineligible record with an operation code 9, which nobody looks at"""
    out = [simple(80, 0, 900, qual=bytes([40] * 20), flag=0x400, name=b"winner_was_marked"), simple(81, 0, 900, qual=bytes([20] * 20), name=b"loser_was_clear")]
    for k, f in enumerate(INELIGIBLE_FLAGS):
        out += [simple(82 + k, 0, 900, flag=f, name=b"in%x" % f), simple(90 + k, 0, 900, flag=f | 0x400, name=b"in%x_marked" % f)]
    out += [simple(98, -1, 900, name=b"no_ref"), simple(99, -1, 900, flag=0x400, name=b"no_ref_marked"), simple(100, 0, -1, name=b"no_pos"), simple(101, 0, -1, flag=0x400, name=b"no_pos_marked")]
    out.append(rec(0, 900, [(4, "M"), (3, 9), (4, "M")], l_seq=8, flag=0x100, name=b"secondary_op9"))
    out.append(simple(102, 0, 900, rev=True, flag=1 | 2 | 0x40, name=b"paired_bits_do_not_matter"))
    return out


def _patched(r, offset, fmt, value):
    b = bytearray(r)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


BIG = (1 << 28) - 1
BAD = {  # name -> (record, reason as markdup_ref names it)
    "l_seq_past_the_record": (_patched(simple(110, 0, 50, name=b"lseq"), 20, "<i", 1000), "fields"),
    "l_seq_negative": (_patched(simple(111, 0, 50, flag=4, name=b"neg"), 20, "<i", -1), "fields"),  # (an ineligible record's head counts too)
    "placeholder_bare": (rec(3, 5, [], l_seq=6, words=[6 << 4 | 4, 30 << 4 | 3], aux=b"XAAx", name=b"bare"), "cg"),
    "placeholder_cg_cut": (rec(3, 5, [], l_seq=6, words=[6 << 4 | 4, 30 << 4 | 3], aux=b"CGBI" + struct.pack("<iI", 2, 6 << 4), name=b"cut"), "cg"),
    "placeholder_aux_leaves": (rec(3, 5, [], l_seq=6, words=[6 << 4 | 4, 30 << 4 | 3], aux=b"XZZno_nul", name=b"leaves"), "aux"),
    "op9": (rec(3, 5, [(4, "M"), (3, 9), (4, "M")], l_seq=8, name=b"op9"), "op"),
    "op15_in_the_second_round": (rec(3, 5, [(1, "M")] * 100 + [(1, 15)], l_seq=100, name=b"op15"), "op"),
    "u_below": (rec(0, 7, [(BIG, "S")] * 17 + [(5, "M")], l_seq=5, name=b"below"), "range"),
    "u_above": (rec(0, 7, [(5, "M")] + [(BIG, "N")] * 17, l_seq=5, flag=16, name=b"above"), "range"),
    "ref_id_2_30": (simple(112, 1 << 30, 5, name=b"ref30"), "range"),
}


def with_bad(name, at=5, n=9):
    out = counted(n)
    out.insert(at, BAD[name][0])
    return out


def range_edges():
    """the largest and the smallest u the key holds, and the largest refID: eligible, and never the sentinel"""
    return [rec((1 << 30) - 1, 2 ** 31 - 1, [(1, "M")] + [(BIG, "H")] * 8 + [(7, "H")], l_seq=1, flag=16, name=b"top"),   # u = 2^31 - 1 + 8 * (2^28 - 1) + 7 = 2^32 - 2
            rec((1 << 30) - 1, 2 ** 31 - 1, [(1, "M")] + [(BIG, "H")] * 8 + [(7, "H")], l_seq=1, flag=16, name=b"top_again"),
            rec(0, 0, [(BIG, "S")] * 16 + [(16, "S"), (1, "M")], l_seq=1, name=b"bottom")]                                   # u = -2^32


def designed():
    """name -> records, every set a buffer of its own"""
    apart, together = clip_cases()
    sets = {"count%d" % n: counted(n) for n in COUNTS}
    sets.update(groups=group_sizes(), one_group=one_group(), alignments=alignments(), clips_apart=apart, clips_together=together, long_cigars=long_cigars(),
                placeholder=placeholder(), quals=qual_cases(), eligibility=eligibility(), range_edges=range_edges())
    both = apart + together
    random.Random(9).shuffle(both)
    sets["clips_mixed"] = both
    return sets


# ---- the sorter's inputs ----------------------------------------------------------------------------------------------------------------
def renamed_and_lowered(r, k):
    """record r a second time: another name of the same length, every quality one lower (0 and 0xff stay)"""
    b = bytearray(r)
    l_name, n_cig, l_seq = b[12], struct.unpack_from("<H", b, 16)[0], struct.unpack_from("<i", b, 20)[0]
    tag = (b"%x" % (k + 1))[::-1]
    for i, c in enumerate(tag[:max(l_name - 1, 0)]):
        b[36 + i] = c if c != b[36 + i] else ord("Z")
    q0 = 36 + l_name + 4 * n_cig + (l_seq + 1) // 2
    for i in range(q0, q0 + l_seq):
        if b[i] not in (0, 0xff):
            b[i] -= 1
    return bytes(b)


def doubled(recs):
    return list(recs) + [renamed_and_lowered(r, k) for k, r in enumerate(recs)]


def spread_groups(n_groups=40, size=5, filler=200):
    """groups of `size` whose members lie `filler` records apart in input order: with small runs every member is in another run, and with
    chunks of one record in another chunk.  The best score is the group's LAST member, so the winner is decided across runs"""
    out = []
    for m in range(size):
        for g in range(n_groups):
            out.append(simple(7000 + g * size + m, g % 3, 1000 + 11 * g, rev=bool(g & 1), qual=bytes([16 + m] * 20), name=b"sp%d_%d" % (g, m)))
        out += [simple(9000 + m * filler + k, (m + k) % 3, 5000 + 13 * k, name=b"fill%d_%d" % (m, k)) for k in range(filler)]
    return out

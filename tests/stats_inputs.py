"""Inputs of the statistics tests (CPU and GPU): hand-built BAM records (pile_inputs.rec) over the designed reference of the coverage and
pileup tests -- every base of it is known here (pile_inputs.REF_SEQS) -- and over pile_inputs.REF_N, the small reference that holds an N.
A designed case is dict(recs, ref, opt): ref is "designed" or "withN", opt the options of Stats that differ from the defaults (with
`bound`, the weight a block holds between two flushes: small values reach the flush and the path of a record too heavy for local memory)."""
import numpy as np

import cov_inputs as ci
import pile_inputs as pi

rec, REF_LENS, REF_SEQS, NIBBLES = pi.rec, pi.REF_LENS, pi.REF_SEQS, pi.NIBBLES
REFS = {"designed": (REF_LENS, REF_SEQS), "withN": ([len(pi.REF_N[1][0])], pi.REF_N[1])}
OPTIONS = dict(excl_flags=0x700, min_mapq=0, cycles=512, max_len=65536, max_indel=64, bound=0)


def case(recs, ref="designed", **opt):
    assert all(k in OPTIONS for k in opt)
    return dict(recs=list(recs), ref=ref, opt=opt)


def ref_at(rid, pos, n):
    return REF_SEQS[rid][pos:pos + n]


def other(base, k=1):
    return "ACGT"[("ACGT".index(base) + k) % 4]


def mutate(s, every):
    """s with every `every`-th base replaced by another letter"""
    return "".join(other(c) if i % every == 0 else c for i, c in enumerate(s))


def length_recs(lens, strands=(0, 16)):
    """reads of exactly these lengths on both strands, copied from the reference with a mismatch every 4 bases"""
    return [rec(0, 20 + k, [(n, "M")] if n else [], seq=mutate(ref_at(0, 20 + k, n), 4), l_seq=n, flag=f, seed=n, name=b"len%d_%d" % (n, f)) for k, n in enumerate(lens) for f in strands]


def indel_recs(lengths):
    return [rec(4, 100 + 50 * k, [(5, "M"), (L, "I"), (5, "M"), (L, "D"), (5, "M")], seed=L, flag=16 * (k % 2), name=b"indel%d" % L) for k, L in enumerate(lengths)]


def nibble_recs():
    """over withN: every one of the sixteen nibbles on a position of every one of the five reference codes, on both strands"""
    ref = pi.REF_N[1][0]
    at = {c: ref.index(c) for c in "ACGTN"}
    return [rec(0, at[c], [(1, "M")], seq=n, flag=f, name=b"nib") for c in "ACGTN" for n in NIBBLES for f in (0, 16)] + \
           [rec(0, 44, [(16, "M")], seq=NIBBLES, name=b"all16"), rec(0, 43, [(1, "S"), (15, "M")], seq=NIBBLES, flag=16, name=b"all16_rev")]


def clip_cycle_recs():
    """both strands with leading and trailing hard and soft clips, a hard clip at one end only, a lone hard clip, and a hard clip that is
    not at an end (it moves no cycle)"""
    out = []
    for f in (0, 16):
        out += [rec(0, 16, [(5, "H"), (3, "S"), (20, "M"), (2, "S"), (7, "H")], seq=mutate("GGG" + ref_at(0, 16, 20) + "TT", 5), flag=f, name=b"both"),
                rec(0, 40, [(4, "H"), (12, "M")], seq=ref_at(0, 40, 12), flag=f, name=b"lead"), rec(0, 60, [(12, "M"), (9, "H")], seq=ref_at(0, 60, 12), flag=f, name=b"trail"),
                rec(0, 80, [(2, "S"), (6, "M"), (3, "H"), (6, "M"), (1, "S")], seq=mutate("A" + "C" + ref_at(0, 80, 12) + "G", 3), flag=f, name=b"H_inside"),
                rec(0, 90, [(6, "H")], l_seq=0, flag=f, name=b"H_alone")]
    return out


def quality_recs():
    q = bytes([0, 94, 95, 96, 254, 1, 93, 40, 40, 40])
    return [rec(0, 30, [(10, "M")], qual=q, name=b"edges"), rec(0, 32, [(10, "M")], qual=None, name=b"no_qual"), rec(0, 34, [(3, "S"), (7, "M")], qual=q, flag=16, name=b"edges_rev"),
            rec(0, 36, [(70, "M")], qual=bytes([40] * 70), name=b"binned"), rec(0, 38, [(10, "M")], qual=bytes([254] * 10), name=b"all254")]


def unmapped_recs():
    return [rec(-1, -1, [], flag=4, l_seq=10, mapq=0, name=b"unmapped"), rec(0, 30, [], flag=4, l_seq=11, mapq=0, name=b"unmapped_placed"),
            rec(0, 30, [], flag=4 | 16, l_seq=9, mapq=0, name=b"unmapped_placed_rev"), rec(-1, -1, [], flag=0, l_seq=5, mapq=70, name=b"unplaced_passing"),
            rec(0, 31, [(8, "M")], flag=4, mapq=0, name=b"unmapped_with_cigar")]


def flag_recs():
    out = []
    for k, (flag, mapq) in enumerate([(0, 0), (0, 1), (0, 60), (0, 255), (16, 30), (4, 0), (0x100, 30), (0x100 | 16, 2), (0x800, 30), (0x800 | 16, 0), (0x900, 9), (0x200, 30), (0x400, 30),
                                      (0x400 | 0x100, 30), (0x400 | 0x200 | 16, 61), (1 | 2 | 0x40, 30), (4 | 0x100, 0)]):
        out.append(rec(k % 3 + 2, 10 + k, [(2, "S"), (15, "M"), (1, "I"), (3, "D"), (4, "M")], flag=flag, mapq=mapq, seed=k, name=b"f%d" % k))
    return out


FILTERS = [(0x700, 0), (0, 0), (0x704, 1), (0x900, 61), (0x400, 30)]


def gc_recs():
    """a == 0; exact half-percent ties (1 of 8: 12.5, 1 of 40: 2.5, 1 of 200: 0.5, 199 of 200: 99.5); all and none"""
    seqs = ["NNNN=", "C" + "A" * 7, "G" + "T" * 39, "C" + "A" * 199, "G" * 199 + "T", "GC" * 5, "AT" * 5, "GN" + "A" * 7]
    return [rec(-1, -1, [], flag=4, seq=s, mapq=0, name=b"gc%d" % k) for k, s in enumerate(seqs)]


def identity_recs():
    r = ref_at(2, 50, 20)
    return [rec(2, 50, [(20, "M")], seq=r, name=b"id100"), rec(2, 50, [(20, "M")], seq="".join(other(c) for c in r), name=b"id0"),
            rec(2, 50, [(20, "M")], seq="N" * 20, name=b"den0_other"), rec(2, 50, [(20, "S")], seq=r, name=b"den0_clip"), rec(2, 50, [(4, "N"), (3, "P")], l_seq=0, name=b"den0_no_seq"),
            rec(2, 50, [(10, "M"), (2, "I"), (8, "M")], seq=r[:10] + "AA" + r[10:18], name=b"id94"), rec(2, 50, [(10, "=")] + [(1, "D")] * 10, seq=r[:10], name=b"id50"),
            rec(2, 50, [(0, "I"), (0, "D"), (1, "X")], seq=other(r[0]), name=b"zero_runs")]


def copies(n=2000):
    r = ref_at(0, 100, 50)
    return [rec(0, 100, [(50, "M")], seq=mutate(r, 7), seed=1, flag=16, qual=bytes([40] * 25 + [12] * 25), name=b"copy")] * n


def designed():
    """name -> case: every valid designed set"""
    out = {"count%d" % n: case(pi.counted(n)) for n in (1, 3, 4, 5, 9)}
    out["copies"] = case(copies())
    out["copies_flush"] = case(copies(300), bound=4096)  # 51 a record: a flush every 20 steps
    out.update({"ops%d" % k: case([pi.ops_record(k), pi.ops_record(1, rid=0, pos=0)]) for k in (63, 64, 65, 129)})
    out.update({"run%d" % n: case([pi.run_record(n)]) for n in (1, 63, 64, 65, 5000)})
    out["run5000_tail8"] = case([pi.run_record(5000), rec(4, 17, [(5000, "M")], seed=5000, flag=16, name=b"rev")], cycles=8)
    out["direct"] = case([pi.run_record(5000)] + pi.counted(9) + quality_recs(), bound=256)  # 5001 > 64: past local memory; the others flush
    out["direct_all"] = case(pi.counted(9) + clip_cycle_recs() + quality_recs(), bound=4)
    out["cycles8"] = case(length_recs((7, 8, 9)), cycles=8)
    out["cycles1"] = case(length_recs((0, 1, 2)), cycles=1)
    out["max_len16"] = case(length_recs((15, 16, 17)), max_len=16)
    out["max_len1"] = case(length_recs((0, 1, 2)), max_len=1)
    out["max_indel4"] = case(indel_recs((3, 4, 5)), max_indel=4)
    out["max_indel1"] = case(indel_recs((1, 2)), max_indel=1)
    out["nibbles"] = case(nibble_recs(), ref="withN")
    out["halves"] = case(pi.clip_recs())
    out["clip_cycles"] = case(clip_cycle_recs())
    out["clip_cycles8"] = case(clip_cycle_recs(), cycles=8)
    out["qualities"] = case(quality_recs())
    out["no_seq"] = case(pi.no_seq_recs())
    out["placeholder"] = case(pi.placeholder_recs())
    out["unmapped"] = case(unmapped_recs())
    out.update({"flags_%x_%d" % (e, q): case(flag_recs() + pi.no_seq_recs(), excl_flags=e, min_mapq=q) for e, q in FILTERS})
    out["gc"] = case(gc_recs())
    out["identity"] = case(identity_recs())
    out["long"] = case(pi.designed()["long"]["recs"], cycles=1024, max_indel=4096)
    return out


def flat(v):
    """(records joined, contig lengths, reference codes per contig, options) of a case"""
    import pile_ref as pr
    lens, seqs = REFS[v["ref"]]
    return b"".join(v["recs"]), lens, [pr.codes_of(s) for s in seqs], dict(OPTIONS, **v["opt"])

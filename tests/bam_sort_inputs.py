"""Inputs of the sorted-BAM tests (CPU and GPU): bare BAM records made by bam_ref.sam_to_bam from golden SAM lines, shuffled with a fixed
seed, and hand-built records at the edges of the sort key, of the record sizes and of the CIGAR field."""
import random
import struct

import bam_ref
from fixture_io import golden_sam

REFS = ["c1", "c2", "c3"]  # of the hand-built records
REF_LENS = [400000, 100000, 70000]


def line(name, flag, ref, pos1, cigar, seq="*", qual="*", tags=()):
    """a SAM line; pos1 is 1-based (0: the record's pos is -1)"""
    return "\t".join([name, str(flag), ref, str(pos1), "30", cigar, "*", "0", "0", seq, qual] + list(tags))


def golden_records(kind, seed=5, limit=None):
    """(records of the kind's golden SAM lines in shuffled order, reference names)"""
    lines = golden_sam(kind)
    names = sorted({l.split("\t")[2] for l in lines} - {"*"})
    recs = [bam_ref.encode_record(l, names) for l in lines]
    random.Random(seed).shuffle(recs)
    return recs[:limit], names


def key_cases():
    """records whose order is decided by every part of the key; names say what the record is"""
    L = []
    L.append(line("unplaced_a", 4, "*", 0, "*", "ACGT", "IIII"))
    L.append(line("c3_late", 0, "c3", 5000, "10M", "A" * 10, "I" * 10))
    L.append(line("c1_rev", 16, "c1", 100, "4M", "ACGT", "IIII"))
    L.append(line("c1_fwd", 0, "c1", 100, "4M", "ACGT", "IIII"))
    L.append(line("c2_x", 0, "c2", 7, "1M", "A", "I"))
    L.append(line("equal_1", 0, "c1", 100, "4M", "ACGT", "IIII", ["XO:i:1"]))
    L.append(line("c1_posm1", 0, "c1", 0, "*", "A", "I"))  # pos -1 on a placed record: first of its contig
    L.append(line("equal_2", 0, "c1", 100, "4M", "ACGT", "IIII", ["XO:i:2"]))
    L.append(line("c3_early", 16, "c3", 1, "3M", "ACG", "III"))
    L.append(line("unplaced_b", 4, "*", 0, "*", "A", "*"))
    L.append(line("c2_y", 16, "c2", 7, "1M", "A", "I"))
    L.append(line("equal_3", 0, "c1", 100, "4M", "ACGT", "IIII", ["XO:i:3"]))
    L.append(line("c1_first", 0, "c1", 1, "2M", "AC", "II"))
    L.append(line("c1_unmapped_placed", 4, "c1", 16385, "*", "AC", "II"))
    recs = [bam_ref.encode_record(l, REFS) for l in L]
    # an unmapped read placed at its mate's position carries the bin of that position, as samtools writes it (bam_ref gives every
    # unmapped record bin 4680, which no region query looks into)
    placed = bytearray(recs[-1])
    struct.pack_into("<H", placed, 14, bam_ref.reg2bin(16384, 16385))
    recs[-1] = bytes(placed)
    return recs


def cigar_cases():
    """n_cigar_op 0, 1, 64, 65 and a placeholder record whose CG tag disagrees with its N on purpose: `end` must come from the N"""
    L = [line("ops0", 0, "c1", 20000, "*", "A", "I"), line("ops1", 0, "c1", 16384, "30M", "*", "*")]
    for n in (64, 65):
        cg = "".join("%d%s" % (1 + k % 3, "MIDN=X"[k % 6]) for k in range(n))
        L.append(line("ops%d" % n, 16, "c2", 16383 - n, cg))
    recs = [bam_ref.encode_record(l, REFS) for l in L]
    # <l_seq>S<ref_len>N with the real CIGAR in CG: written by hand, so that the tag says 7M while the field says 40000N
    name = b"placeholder\0"
    words = struct.pack("<II", 5 << 4 | 4, 40000 << 4 | 3)
    tag = b"CGBI" + struct.pack("<iI", 1, 7 << 4)
    body = struct.pack("<iiBBHHHiiii", 0, 32768, len(name), 9, bam_ref.reg2bin(32768, 32768 + 40000), 2, 0, 5, -1, -1, 0) + name + words + b"\x12\x48\x10" + b"\xff" * 5 + tag
    recs.append(struct.pack("<i", len(body)) + body)
    return recs


def size_cases():
    """records from the smallest there is (a 1-byte name, no CIGAR, l_seq 0 / 1) to more than 64 x 16 bytes, one at every size mod 16"""
    recs = [bam_ref.encode_record(line("x", 4, "*", 0, "*"), REFS), bam_ref.encode_record(line("y", 0, "c1", 3, "*", "A", "I"), REFS)]
    for k in range(16):
        recs.append(bam_ref.encode_record(line("n" * (1 + k), 0, "c2", 50000 - 100 * k, "3M", "ACG", "III"), REFS))
        recs.append(bam_ref.encode_record(line("L%d" % k, 16, "c3", 1 + k, "%dM" % (1100 + k), "A" * (1100 + k), "*", ["XZ:Z:" + "z" * k]), REFS))
    assert sorted({len(r) % 16 for r in recs}) == list(range(16)) and min(len(r) for r in recs) == 38 and max(len(r) for r in recs) > 64 * 16
    return recs


def hand_built(seed=3):
    recs = key_cases() + cigar_cases() + size_cases()
    random.Random(seed).shuffle(recs)
    return recs


def counted(n, seed=1):
    """n records drawn from the hand-built ones in a fixed order (with repetition: records that are drawn twice have equal keys)"""
    pool = hand_built(seed)
    rng = random.Random(100 + n)
    return [pool[rng.randrange(len(pool))] for _ in range(n)]


REGIONS = [(0, 99, 100), (0, 100, 101), (0, 102, 103), (0, 103, 104), (0, 0, 1), (0, 16383, 16384), (0, 16384, 16385), (0, 16385, 16386), (0, 16384 - 1, 16384 + 1),
           (0, 2 * 16384 - 1, 2 * 16384), (0, 2 * 16384, 2 * 16384 + 1), (0, 2 * 16384 + 1, 2 * 16384 + 2), (0, 4 * 16384 - 1, 4 * 16384 + 1), (0, 72767, 72768), (0, 72768, 72769),
           (0, 0, REF_LENS[0]), (1, 0, REF_LENS[1]), (2, 0, REF_LENS[2]), (0, 200000, 300000), (1, 16383, 16384), (1, 16384, 16385), (1, 49999, 50003), (2, 0, 1), (2, 1115, 1116)]

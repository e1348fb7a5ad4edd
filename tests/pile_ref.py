"""Pileup and variant sites from BAM records: an independent restatement, in Python, of the section "Pileup" of include/gdiet_hip.h.
Written from that text alone -- nothing here is taken from csrc/ or from cov_ref's walk -- one base at a time into a dict of positions, so
that the 64-lane statements (csrc/pile.h through tests/emul/pile_emul.cpp) and the kernels can be compared against it integer for integer.

  check_regions(regions, ref_lens)   None, or (index of the first offending region, "empty" | "past" | "unsorted" | "overlap")
  pileup(data, ref_lens, regions=None, excl_flags=0x704, min_mapq=0, min_baseq=0) -> Pile
      .regions   the list (every contig whole for None / [])
      .summary   dict of the twelve counters
      .counts    one (n, 8) uint32 array per region: A C G T N DEL INS REV
      .bad       None, or (index of the first bad record, reason)
  consensus(pile, ref_codes, i, min_depth=1) -> bytes        ref_codes: per contig a sequence of codes 0..4
  sites(pile, ref_codes, min_depth=8, min_alt=2, frac=(1, 5)) -> list of (rid, pos, ref, alt, depth, (eight counters))
  sam_pileup(lines, names, ref_lens, regions, ...)           the second oracle: the SAM text columns, one base at a time
  pileup_tsv / consensus_fa                                   the two text files of Pileup.write"""
import re
import struct

import numpy as np

SUMMARY = ("records", "unmapped", "secondary", "supplementary", "primary_mapped", "reverse", "excluded_by_flag", "excluded_by_mapq", "counted", "bad", "no_seq", "skipped_baseq")
COUNTERS = ("A", "C", "G", "T", "N", "DEL", "INS", "REV")
A, C, G, T, N, DEL, INS, REV = range(8)
REF_LETTERS, ALT_LETTERS = "ACGTN", "ACGT*+"
_AUX = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
_NIBBLE = {1: A, 2: C, 4: G, 8: T}


class Pile:
    pass


def records(data):
    at = 0
    while at < len(data):
        n = struct.unpack_from("<i", data, at)[0]
        assert n >= 32 and at + 4 + n <= len(data)
        yield data[at + 4:at + 4 + n]
        at += 4 + n


def check_regions(regions, ref_lens):
    for i, (rid, beg, end) in enumerate(regions):
        if beg >= end:
            return i, "empty"
        if rid >= len(ref_lens) or end > ref_lens[rid]:
            return i, "past"
        if i and (regions[i - 1][0], regions[i - 1][1]) > (rid, beg):
            return i, "unsorted"
        if i and regions[i - 1][0] == rid and regions[i - 1][2] > beg:
            return i, "overlap"
    return None


def whole(ref_lens):
    return [(rid, 0, n) for rid, n in enumerate(ref_lens) if n]


def _real_cigar(b, words, l_seq, aux_at):
    """the words of the real CIGAR, or the reason it has none"""
    if not (len(words) == 2 and words[0] == (l_seq << 4 | 4) and words[1] & 15 == 3):
        return words, None
    at = aux_at
    while at < len(b):
        if len(b) - at < 3:
            return None, "aux"
        tag, t = b[at:at + 2], chr(b[at + 2])
        at += 3
        if t in _AUX:
            size = _AUX[t]
        elif t in "ZH":
            z = b.find(b"\0", at)
            if z < 0:
                return None, "aux"
            size = z + 1 - at
        elif t == "B":
            if len(b) - at < 5:
                return None, "aux"
            sub, cnt = chr(b[at]), struct.unpack_from("<i", b, at + 1)[0]
            if sub not in _AUX or sub == "A" or cnt < 0:
                return None, "aux"
            size = 5 + _AUX[sub] * cnt
            if tag == b"CG":
                if sub != "I" or at + size > len(b):
                    return None, "cg"
                return list(struct.unpack_from("<%dI" % cnt, b, at + 5)), None
        else:
            return None, "aux"
        if tag == b"CG":
            return None, "cg"
        if at + size > len(b):
            return None, "aux"
        at += size
    return None, "cg"


def _read(b, ref_lens):
    """(fields, reason): the fields of one record body and why it is bad, if it is"""
    rid, pos, l_name, mapq, _bin, n_op, flag, l_seq = struct.unpack_from("<iiBBHHHi", b, 0)
    f = dict(rid=rid, pos=pos, mapq=mapq, flag=flag, l_seq=l_seq)
    seq_at = 32 + l_name + 4 * n_op
    if l_seq < 0 or seq_at + (l_seq + 1) // 2 + l_seq > len(b):
        return f, "fields"
    qual_at = seq_at + (l_seq + 1) // 2
    f["seq"] = [b[seq_at + k // 2] >> 4 if k % 2 == 0 else b[seq_at + k // 2] & 15 for k in range(l_seq)]
    f["qual"] = b[qual_at:qual_at + l_seq] if l_seq and b[qual_at] != 0xff else None
    words, why = _real_cigar(b, list(struct.unpack_from("<%dI" % n_op, b, 32 + l_name)), l_seq, qual_at + l_seq)
    if why:
        return f, why
    f["ops"] = ops = [("MIDNSHP=X????????"[w & 15], w >> 4) for w in words]
    if rid >= len(ref_lens):
        return f, "ref"
    if rid >= 0 and pos < 0:
        return f, "pos"
    if any(o == "?" for o, _ in ops):
        return f, "op"
    if rid >= 0 and pos + sum(n for o, n in ops if o in "MDN=X") > ref_lens[rid]:
        return f, "ref_end"
    if l_seq > 0 and sum(n for o, n in ops if o in "MIS=X") > l_seq:
        return f, "qry_end"
    return f, None


def pileup(data, ref_lens, regions=None, excl_flags=0x704, min_mapq=0, min_baseq=0):
    regions = list(regions) if regions else whole(ref_lens)
    assert check_regions(regions, ref_lens) is None
    where = {}  # (rid, pos) -> (region, row)
    counts = [np.zeros((end - beg, 8), np.int64) for _, beg, end in regions]
    for i, (rid, beg, end) in enumerate(regions):
        for p in range(beg, end):
            where[rid, p] = (i, p - beg)
    S = dict.fromkeys(SUMMARY, 0)
    bad = None

    def add(rid, p, k):
        if (rid, p) in where:
            i, row = where[rid, p]
            counts[i][row, k] += 1

    for index, b in enumerate(records(data)):
        f, why = _read(b, ref_lens)
        flag = f["flag"]
        S["records"] += 1
        S["unmapped"] += bool(flag & 4)
        S["secondary"] += bool(flag & 0x100)
        S["supplementary"] += bool(flag & 0x800)
        S["primary_mapped"] += not flag & 0x904
        S["reverse"] += bool(flag & 0x10) and not flag & 4
        if why:
            S["bad"] += 1
            bad = bad or (index, why)
            continue
        if flag & excl_flags:
            S["excluded_by_flag"] += 1
            continue
        if f["mapq"] < min_mapq:
            S["excluded_by_mapq"] += 1
            continue
        if f["rid"] < 0:
            continue
        if f["l_seq"] == 0:
            S["no_seq"] += 1
            continue
        S["counted"] += 1
        rid, r, q = f["rid"], f["pos"], 0
        for o, n in f["ops"]:
            if o in "M=X":
                for k in range(n):
                    if (rid, r + k) not in where:
                        continue
                    if f["qual"] is not None and f["qual"][q + k] < min_baseq:
                        S["skipped_baseq"] += 1
                        continue
                    add(rid, r + k, _NIBBLE.get(f["seq"][q + k], N))
                    if flag & 0x10:
                        add(rid, r + k, REV)
                r, q = r + n, q + n
            elif o == "D":
                for k in range(n):
                    add(rid, r + k, DEL)
                r += n
            elif o == "N":
                r += n
            elif o == "I":
                if r > f["pos"]:
                    add(rid, r - 1, INS)
                q += n
            elif o == "S":
                q += n
    out = Pile()
    out.regions, out.summary, out.bad = regions, S, bad
    out.counts = [c.astype(np.uint32) for c in counts]
    return out


# ---- the calls ---------------------------------------------------------------------------------------------------------------------
def _alleles(c):
    return [int(c[A]), int(c[C]), int(c[G]), int(c[T]), int(c[DEL])]


def consensus(pile, i, min_depth=1):
    out = bytearray()
    for c in pile.counts[i]:
        al, depth = _alleles(c), int(c[:6].sum(dtype=np.int64))
        out.append(ord("N") if depth < min_depth or max(al) == 0 else ord("ACGT*"[al.index(max(al))]))
    return bytes(out)


def sites(pile, ref_codes, min_depth=8, min_alt=2, frac=(1, 5)):
    num, den = frac
    assert den > 0
    rows = []
    for (rid, beg, _), counts in zip(pile.regions, pile.counts):
        for k, c in enumerate(counts):
            depth, ref = int(c[:6].sum(dtype=np.int64)), int(ref_codes[rid][beg + k])
            if depth < min_depth:
                continue
            ok = lambda v: v >= min_alt and v * den >= num * depth
            al = _alleles(c)
            good = [a for a in range(5) if (a == 4 or a != ref) and ok(al[a])]
            if good:
                alt = max(good, key=lambda a: (al[a], -a))
            elif ok(int(c[INS])):
                alt = 5
            else:
                continue
            rows.append((rid, beg + k, ref, alt, depth, tuple(int(x) for x in c)))
    return rows


def codes_of(seq):
    return ["ACGT".find(ch) if ch in "ACGT" else 4 for ch in seq.upper()]


# ---- the second oracle: SAM text -----------------------------------------------------------------------------------------------------
_OP = re.compile(r"(\d+)([MIDNSHP=X])")


def sam_pileup(lines, ref_names, ref_lens, regions=None, excl_flags=0x704, min_mapq=0, min_baseq=0):
    """(counts per region as lists of 8-lists, skipped_baseq, records counted) of SAM lines: FLAG, RNAME, POS, MAPQ, CIGAR, SEQ and QUAL of
    the text, piled up one base at a time"""
    regions = list(regions) if regions else whole(ref_lens)
    counts = [[[0] * 8 for _ in range(end - beg)] for _, beg, end in regions]
    skipped = counted = 0

    def row(rid, p):
        for i, (g, beg, end) in enumerate(regions):
            if g == rid and beg <= p < end:
                return counts[i][p - beg]
        return None

    for l in lines:
        if not l or l.startswith("@"):
            continue
        f = l.split("\t")
        flag, rname, pos, mapq, cigar, seq, qual = int(f[1]), f[2], int(f[3]) - 1, int(f[4]), f[5], f[9], f[10]
        if flag & excl_flags or mapq < min_mapq or rname == "*" or seq == "*":
            continue
        rid = list(ref_names).index(rname)
        counted += 1
        r, q, first = pos, 0, pos
        for n, op in _OP.findall("" if cigar == "*" else cigar):
            n = int(n)
            if op == "I" and r > first:
                c = row(rid, r - 1)
                if c is not None:
                    c[INS] += 1
            for _ in range(n):
                if op in "M=X":
                    c = row(rid, r)
                    if c is not None:
                        if qual != "*" and ord(qual[q]) - 33 < min_baseq:
                            skipped += 1
                        else:
                            c["ACGT".find(seq[q].upper()) if seq[q].upper() in "ACGT" else N] += 1
                            c[REV] += bool(flag & 16)
                    r, q = r + 1, q + 1
                elif op == "D":
                    c = row(rid, r)
                    if c is not None:
                        c[DEL] += 1
                    r += 1
                elif op == "N":
                    r += 1
                elif op in "IS":
                    q += 1
    return counts, skipped, counted


# ---- the text files ----------------------------------------------------------------------------------------------------------------
def pileup_tsv(rows, names):
    out = ["#contig\tpos\tref\talt\tdepth\t" + "\t".join(COUNTERS)]
    for rid, pos, ref, alt, depth, c in rows:
        out.append("\t".join([names[rid], str(pos + 1), REF_LETTERS[ref], ALT_LETTERS[alt], str(depth)] + [str(x) for x in c]))
    return "\n".join(out) + "\n"


def consensus_fa(pile, names, min_depth=1, width=60):
    out = []
    for i, (rid, beg, end) in enumerate(pile.regions):
        out.append(">%s:%d-%d" % (names[rid], beg + 1, end))
        s = consensus(pile, i, min_depth).decode()
        out += [s[k:k + width] for k in range(0, len(s), width)]
    return "\n".join(out) + "\n"

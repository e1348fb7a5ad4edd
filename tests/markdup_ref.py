"""An independent restatement of the section "Duplicate marking" of include/gdiet_hip.h, in plain Python: no import from the package, nothing
shared with csrc/bam_markdup.h.  It is the oracle of tests/test_markdup.py (CPU) and tests/test_markdup_gpu.py (GPU).

    markdup(data) -> (data with bit 0x400 rewritten, dict(examined, eligible, duplicates, max_group))
raises Bad(index, reason) for the first bad record of the buffer; reason is one of "fields", "cg", "aux", "op", "range"."""
import struct

INELIGIBLE = 0xB04
DUP = 0x400
SENTINEL = (1 << 64) - 1
REASON_TEXT = {"fields": "the fields leave the record", "cg": "a placeholder CIGAR without a well-formed CG:B:I tag", "aux": "the aux fields leave the record",
               "op": "an operation code above 8", "range": "leaves the range of the group key"}


class Bad(Exception):
    def __init__(self, index, reason):
        Exception.__init__(self, "record %d: %s" % (index, reason))
        self.index, self.reason = index, reason


def split(data):
    out, at = [], 0
    while at < len(data):
        assert len(data) - at >= 4
        bs = struct.unpack_from("<i", data, at)[0]
        assert bs >= 32 and at + 4 + bs <= len(data), "the buffer ends inside a record"
        out.append(data[at:at + 4 + bs])
        at += 4 + bs
    return out


def _cg_array(rec, at):
    """the CG:B:I array of a placeholder record, the aux fields walked from `at`; a reason otherwise"""
    n = len(rec)
    while at < n:
        if n - at < 3:
            return "aux"
        tag, t = rec[at:at + 2], chr(rec[at + 2])
        at += 3
        if t in "AcC":
            sz = 1
        elif t in "sS":
            sz = 2
        elif t in "iIf":
            sz = 4
        elif t in "ZH":
            z = rec.find(b"\0", at)
            if z < 0:
                return "aux"
            sz = z + 1 - at
        elif t == "B":
            if n - at < 5:
                return "aux"
            sub, cnt = chr(rec[at]), struct.unpack_from("<I", rec, at + 1)[0]
            w = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}.get(sub, 0)
            if not w or cnt > 0x7fffffff:
                return "aux"
            sz = 5 + w * cnt
            if tag == b"CG":
                if sub != "I" or n - at < sz:
                    return "cg"
                return list(struct.unpack_from("<%dI" % cnt, rec, at + 5))
        else:
            return "aux"
        if tag == b"CG":
            return "cg"
        if n - at < sz:
            return "aux"
        at += sz
    return "cg"


def head(rec):
    """(refID, pos, flag, words of the real CIGAR, qual bytes) or a reason"""
    n = len(rec)
    ref_id, pos, l_name, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 4)
    if l_seq < 0:
        return "fields"
    cig_at = 36 + l_name
    qual_at = cig_at + 4 * n_cig + (l_seq + 1) // 2
    if qual_at + l_seq > n:
        return "fields"
    words = list(struct.unpack_from("<%dI" % n_cig, rec, cig_at))
    if n_cig == 2 and words[0] == (l_seq << 4 | 4) and words[1] & 15 == 3:
        words = _cg_array(rec, qual_at + l_seq)
        if isinstance(words, str):
            return words
    return ref_id, pos, flag, words, rec[qual_at:qual_at + l_seq]


def entry(rec):
    """None for an ineligible record, ((refID, u, strand), score) for an eligible one, a reason (str) for a bad one"""
    h = head(rec)
    if isinstance(h, str):
        return h
    ref_id, pos, flag, words, qual = h
    if flag & INELIGIBLE or ref_id < 0 or pos < 0:
        return None
    ops = [(w & 15, w >> 4) for w in words]
    if any(op > 8 for op, _ in ops):
        return "op"
    rev = flag >> 4 & 1
    if rev:
        ops_from_5p = ops[::-1]
    else:
        ops_from_5p = ops
    clip = 0
    for op, ln in ops_from_5p:
        if op not in (4, 5):
            break
        clip += ln
    ref_len = sum(ln for op, ln in ops if op in (0, 2, 3, 7, 8))
    u = pos + ref_len - 1 + clip if rev else pos - clip
    if not (-(1 << 32) <= u <= (1 << 32) - 2) or ref_id >= 1 << 30:
        return "range"
    score = sum(q for q in qual if 15 <= q != 0xff) & 0xffffffff
    return (ref_id, u, rev), score


def key64(triple):
    """the suggested 64-bit layout of a group's key: injective on the triples that pass, and never the sentinel"""
    ref_id, u, rev = triple
    return ref_id << 34 | (u + (1 << 32)) << 1 | rev


def decide(entries):
    """entries in output order (None: ineligible) -> (set of duplicate places, eligible, max_group)"""
    groups = {}
    for j, e in enumerate(entries):
        if e is not None:
            groups.setdefault(e[0], []).append((e[1], j))
    dups = set()
    for members in groups.values():
        best = max(s for s, _ in members)
        winner = min(j for s, j in members if s == best)
        dups |= {j for _, j in members if j != winner}
    return dups, sum(len(m) for m in groups.values()), max([len(m) for m in groups.values()] or [0])


def markdup_records(recs):
    entries = []
    for k, r in enumerate(recs):
        e = entry(r)
        if isinstance(e, str):
            raise Bad(k, e)
        entries.append(e)
    dups, eligible, max_group = decide(entries)
    out = []
    for j, (r, e) in enumerate(zip(recs, entries)):
        if e is not None:
            flag = struct.unpack_from("<H", r, 18)[0]
            flag = (flag & ~DUP) | (DUP if j in dups else 0)
            r = r[:18] + struct.pack("<H", flag) + r[20:]
        out.append(r)
    return out, dict(examined=len(recs), eligible=eligible, duplicates=len(dups), max_group=max_group)


def markdup(data):
    out, st = markdup_records(split(data))
    return b"".join(out), st


def only_dup_bit_differs(a, b):
    """two buffers of records that differ in bit 0x400 of the flags alone"""
    ra, rb = split(a), split(b)
    if len(a) != len(b) or len(ra) != len(rb):
        return False
    for x, y in zip(ra, rb):
        fx, fy = struct.unpack_from("<H", x, 18)[0], struct.unpack_from("<H", y, 18)[0]
        if x[:18] != y[:18] or x[20:] != y[20:] or (fx ^ fy) & ~DUP:
            return False
    return True

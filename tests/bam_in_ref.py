"""BAM input as a function of the decompressed stream: an independent restatement, in Python, of the "BAM input" section of
include/gdiet_hip.h.  Written from that definition alone -- nothing here is taken from csrc/ -- so that the host grammar, the 64-lane
unpack statements and the kernel can be compared against it.

  reads_of(stream, with_qual=True, with_comment=False) -> (reads, status, where)
      reads   [(name, comment or None, seq, qual or None, l_seq)], all bytes, in file order, secondary / supplementary records left out
      status  "ok", "truncated" (the stream ends inside the header or a record) or "error" (a record that contradicts itself)
      where   (ordinal, offset) of the malformed record, counting every record of the stream from 0; None otherwise
  records_of(records, ...)   the same for bare records without a header
"""
import struct

import numpy as np

LETTERS = b"=ACMGRSVTWYHKDBN"
# the complement of every code as the letters say it: = and N stay, A<->T, C<->G, and the ambiguity codes by their sets
_SETS = {"=": "=", "A": "A", "C": "C", "G": "G", "T": "T", "M": "AC", "R": "AG", "W": "AT", "S": "CG", "Y": "CT", "K": "GT", "V": "ACG", "H": "ACT", "D": "AGT",
         "B": "CGT", "N": "ACGT"}
_PAIR = {"A": "T", "C": "G", "G": "C", "T": "A", "=": "="}
_BY_SET = {"".join(sorted(v)): k for k, v in _SETS.items()}
COMPLEMENT = bytes(ord(_BY_SET["".join(sorted(_PAIR[x] for x in _SETS[chr(c)]))]) for c in LETTERS)
_INT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


def f32_text(b4):
    v = np.frombuffer(b4, "<f4")[0]
    if v != v:
        return "nan"
    if abs(v) == np.inf:
        return "-inf" if v < 0 else "inf"
    return np.format_float_positional(v, unique=True, trim="-")


def _value(t, b, at):
    if t == "f":
        return f32_text(b[at:at + 4]), at + 4
    n = struct.calcsize(_INT[t])
    if at + n > len(b):
        raise ValueError
    return str(struct.unpack_from(_INT[t], b, at)[0]), at + n


def aux_text(b):
    """the aux fields of one record as SAM text joined by tabs; ValueError when a field runs past the record or has no known type"""
    out, at = [], 0
    while at < len(b):
        if at + 4 > len(b):
            raise ValueError
        tag, t = b[at:at + 2].decode("latin1"), chr(b[at + 2])
        at += 3
        if t == "A":
            out.append("%s:A:%s" % (tag, chr(b[at])))
            at += 1
        elif t in _INT or t == "f":
            if at + (4 if t == "f" else struct.calcsize(_INT[t])) > len(b):
                raise ValueError
            v, at = _value(t, b, at)
            out.append("%s:%s:%s" % (tag, "f" if t == "f" else "i", v))
        elif t in "ZH":
            z = b.find(b"\0", at)
            if z < 0:
                raise ValueError
            out.append("%s:%s:%s" % (tag, t, b[at:z].decode("latin1")))
            at = z + 1
        elif t == "B":
            if at + 5 > len(b):
                raise ValueError
            sub, cnt = chr(b[at]), struct.unpack_from("<i", b, at + 1)[0]
            at += 5
            if (sub not in _INT and sub != "f") or cnt < 0:
                raise ValueError
            w = 4 if sub == "f" else struct.calcsize(_INT[sub])
            if at + w * cnt > len(b):
                raise ValueError
            vals = []
            for _ in range(cnt):
                v, at = _value(sub, b, at)
                vals.append(v)
            out.append("%s:B:%s" % (tag, ",".join([sub] + vals)))
        else:
            raise ValueError
    return "\t".join(out)


def header_end(s):
    """offset of the first record, None when the stream ends inside the header; ValueError for a negative count"""
    if len(s) < 12:
        return None
    l_text = struct.unpack_from("<i", s, 4)[0]
    if l_text < 0:
        raise ValueError
    at = 8 + l_text
    if at + 4 > len(s):
        return None
    n_ref = struct.unpack_from("<i", s, at)[0]
    if n_ref < 0:
        raise ValueError
    at += 4
    for _ in range(n_ref):
        if at + 4 > len(s):
            return None
        l_name = struct.unpack_from("<i", s, at)[0]
        if l_name < 0:
            raise ValueError
        at += 4 + l_name + 4
        if at > len(s):
            return None
    return at


def records_of(s, at=0, with_qual=True, with_comment=False):
    reads, ordinal = [], 0
    while at < len(s):
        bad = (reads, "error", (ordinal, at))
        if len(s) - at < 4:
            return reads, "truncated", None
        bs = struct.unpack_from("<i", s, at)[0]
        if bs < 32:
            return bad
        if len(s) - at - 4 < bs:
            return reads, "truncated", None
        r = s[at + 4:at + 4 + bs]
        _ref, _pos, l_name, _mapq, _bin, n_op, flag, l_seq = struct.unpack_from("<iiBBHHHi", r, 0)
        if l_seq < 0 or l_name == 0:
            return bad
        p_seq = 32 + l_name + 4 * n_op
        p_qual = p_seq + (l_seq + 1) // 2
        p_aux = p_qual + l_seq
        if p_aux > bs or r[32 + l_name - 1] != 0:
            return bad
        comment = None
        if with_comment:
            try:
                comment = aux_text(r[p_aux:]).encode("latin1") or None
            except ValueError:
                return bad
        ordinal += 1
        at += 4 + bs
        if flag & 0x900:
            continue
        name = r[32:32 + l_name]
        name = name[:name.index(b"\0")]
        codes = np.frombuffer(r[p_seq:p_qual], np.uint8)
        nib = np.empty(2 * len(codes), np.uint8)
        nib[0::2], nib[1::2] = codes >> 4, codes & 15
        nib = nib[:l_seq]
        q = np.frombuffer(r[p_qual:p_aux], np.uint8)
        have_q = with_qual and l_seq > 0 and q[0] != 0xff
        if flag & 0x10:
            seq = bytes(COMPLEMENT[c] for c in nib[::-1])
            q = q[::-1]
        else:
            seq = bytes(LETTERS[c] for c in nib)
        qual = ((q.astype(np.uint16) + 33) & 255).astype(np.uint8).tobytes() if have_q else None
        reads.append((name, comment, seq, qual, l_seq))
    return reads, "ok", None


def reads_of(stream, with_qual=True, with_comment=False):
    assert stream[:4] == b"BAM\1"
    try:
        at = header_end(stream)
    except ValueError:
        return [], "error", (0, 0)
    if at is None:
        return [], "truncated", None
    return records_of(stream, at, with_qual, with_comment)

"""BAM records as a fixed function of their SAM lines: an independent restatement, in Python, of the format section of the BAM issue (SAM
specification 4.2 with this project's choices).  Written from that text alone -- nothing here is taken from csrc/ -- so that the C++
flattening, the 64-lane record code and the kernel can be compared against it.  All integers little-endian.

  sam_to_bam(lines, ref_names)   the uncompressed records of the SAM lines (header lines, starting with @, are skipped)
  bam_header(text, refs)         magic, header text (no NUL), dictionary; refs = [(name, length)]
  bam_to_sam(data[, ref_names])  the inverse: SAM lines of the records; a stream that starts with the magic gives its header text's
                                 lines first and takes the names from its dictionary
  reg2bin(beg, end)              the bin of a 0-based half-open interval

Tags: `i` becomes the smallest type that holds the value (c s i only for negative values, else C S I); `f` the float32 nearest to the
decimal text; Z / H text and NUL; B subtype, count, values.  A CIGAR of more than 65 535 operations becomes <l_seq>S<reference length>N
with the operations in a CG:B:I tag, placed in front of the rl:i: tag (where the SAM writer puts it under -L).  A field that is no tag and
a name of more than 254 bytes raise ValueError.  The decoder prints every integer tag as `i` and a float as the shortest decimal text whose
float32 it is, so encode(decode(x)) == x always, and decode(encode(line)) == line for lines that print their floats that way."""
import re
import struct

import numpy as np

SEQ_CODES = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
UNMAPPED_BIN = 4680
_CG = re.compile(r"(\d+)([MIDNSHP=X])")
_INT = re.compile(r"^[-+]?[0-9]+$")
_FLOAT = re.compile(r"^[-+]?[0-9]*\.?[0-9]+([eE][-+]?[0-9]+)?$")
_TAG = re.compile(r"^[A-Za-z][A-Za-z0-9]:[AifZHB]:")
_CODE_OF = bytes(SEQ_CODES.find(chr(c).upper()) if chr(c).upper() in SEQ_CODES and c < 128 else 15 for c in range(256))
_B_FMT = {"c": ("b", -128, 127), "C": ("B", 0, 255), "s": ("h", -32768, 32767), "S": ("H", 0, 65535), "i": ("i", -2 ** 31, 2 ** 31 - 1), "I": ("I", 0, 2 ** 32 - 1)}


def reg2bin(beg, end):
    end -= 1
    for shift, offset in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return offset + (beg >> shift)
    return 0


def _int_tag(v):
    if v < 0:
        if v >= -128:
            return b"c" + struct.pack("<b", v)
        if v >= -32768:
            return b"s" + struct.pack("<h", v)
        if v >= -2 ** 31:
            return b"i" + struct.pack("<i", v)
    elif v <= 255:
        return b"C" + struct.pack("<B", v)
    elif v <= 65535:
        return b"S" + struct.pack("<H", v)
    elif v <= 2 ** 32 - 1:
        return b"I" + struct.pack("<I", v)
    raise ValueError("integer tag out of range: %d" % v)


def _f32(text):
    if not _FLOAT.match(text):
        raise ValueError("not a float: %r" % text)
    return struct.pack("<f", float(text))


def encode_tag(field):
    """one optional field XX:T:value as BAM bytes"""
    if not _TAG.match(field):
        raise ValueError("not a tag: %r" % field[:40])
    name, t, v = field[:2].encode(), field[3], field[5:]
    if t == "A":
        if len(v) != 1 or not "!" <= v <= "~":
            raise ValueError("bad A tag: %r" % field)
        return name + b"A" + v.encode()
    if t == "i":
        if not _INT.match(v) or len(v.lstrip("+-")) > 10:
            raise ValueError("bad i tag: %r" % field)
        return name + _int_tag(int(v))
    if t == "f":
        return name + b"f" + _f32(v)
    if t == "Z":
        return name + b"Z" + v.encode() + b"\0"
    if t == "H":
        if len(v) % 2 or not re.match(r"^[0-9A-Fa-f]*$", v):
            raise ValueError("bad H tag: %r" % field)
        return name + b"H" + v.encode() + b"\0"
    if not v or v[0] not in "cCsSiIf":  # B
        raise ValueError("bad B tag: %r" % field[:40])
    items = v[1:].split(",")
    if items[0] != "":
        raise ValueError("bad B tag: %r" % field[:40])
    items = items[1:]
    out = name + b"B" + v[0].encode() + struct.pack("<i", len(items))
    if v[0] == "f":
        return out + b"".join(_f32(x) for x in items)
    fmt, lo, hi = _B_FMT[v[0]]
    vals = []
    for x in items:
        if not _INT.match(x) or len(x.lstrip("+-")) > 10 or not lo <= int(x) <= hi:
            raise ValueError("bad B value %r in %r" % (x, field[:40]))
        vals.append(int(x))
    return out + struct.pack("<%d%s" % (len(vals), fmt), *vals)


def _cigar_words(text):
    if text == "*":
        return []
    ops = _CG.findall(text)
    if "".join(n + o for n, o in ops) != text:
        raise ValueError("bad CIGAR %r" % text[:40])
    return [int(n) << 4 | CIGAR_OPS.index(o) for n, o in ops]


def encode_record(line, ref_names):
    f = line.rstrip("\n").split("\t")
    if len(f) < 11:
        raise ValueError("a SAM line has eleven fields at least")
    qname, flag, rname, pos, mapq, cigar, seq, qual, tags = f[0], int(f[1]), f[2], int(f[3]) - 1, int(f[4]), f[5], f[9], f[10], f[11:]
    if len(qname.encode()) > 254:
        raise ValueError("read %s...: a name of more than 254 bytes" % qname[:32])
    ref_id = -1 if rname == "*" else list(ref_names).index(rname)
    words = _cigar_words(cigar)
    real = words
    for t in tags:
        if t.startswith("CG:B:I"):
            real = [int(x) for x in t[7:].split(",")] if len(t) > 7 else []
    ref_len = sum(w >> 4 for w in real if CIGAR_OPS[w & 15] in "MDN=X")
    bin_ = UNMAPPED_BIN if flag & 4 else reg2bin(pos, pos + (ref_len if ref_len else 1))
    l_seq = 0 if seq == "*" else len(seq)
    if len(words) > 65535:
        cg = "CG:B:I," + ",".join(str(w) for w in words)
        at = next((i for i, t in enumerate(tags) if t.startswith("rl:i:")), len(tags))
        tags = tags[:at] + [cg] + tags[at:]
        words = [l_seq << 4 | 4, ref_len << 4 | 3]
    if l_seq:
        codes = np.frombuffer(seq.encode().translate(_CODE_OF), np.uint8)
        if l_seq & 1:
            codes = np.concatenate([codes, np.zeros(1, np.uint8)])
        packed = (codes[0::2] << 4 | codes[1::2]).astype(np.uint8).tobytes()
        if qual == "*":
            q = b"\xff" * l_seq
        else:
            if len(qual) != l_seq:
                raise ValueError("SEQ and QUAL differ in length")
            q = (np.frombuffer(qual.encode(), np.uint8) - 33).astype(np.uint8).tobytes()
    else:
        packed, q = b"", b""
    name = qname.encode() + b"\0"
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name), mapq, bin_, len(words), flag, l_seq, -1, -1, 0) + name
    body += struct.pack("<%dI" % len(words), *words) + packed + q + b"".join(encode_tag(t) for t in tags)
    return struct.pack("<i", len(body)) + body


def sam_to_bam(lines, ref_names):
    if isinstance(lines, (str, bytes)):
        lines = (lines.decode() if isinstance(lines, bytes) else lines).split("\n")
    return b"".join(encode_record(l, ref_names) for l in lines if l and not l.startswith("@"))


def bam_header(text, refs):
    t = text.encode() if isinstance(text, str) else text
    out = b"BAM\1" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(refs))
    for name, length in refs:
        n = name.encode() + b"\0"
        out += struct.pack("<i", len(n)) + n + struct.pack("<I", length & 0xffffffff)
    return out


def f32_text(bits4):
    """the shortest decimal text whose float32 is the value"""
    v = np.frombuffer(bits4, "<f4")[0]
    return np.format_float_positional(v, unique=True, trim="-") if v == v and abs(v) != np.inf else str(v)


def _decode_tags(b, at, end):
    out = []
    while at < end:
        name, t = b[at:at + 2].decode(), chr(b[at + 2])
        at += 3
        if t == "A":
            out.append("%s:A:%s" % (name, chr(b[at])))
            at += 1
        elif t in "cCsSiI":
            fmt = _B_FMT[t][0]
            n = struct.calcsize(fmt)
            out.append("%s:i:%d" % (name, struct.unpack("<" + fmt, b[at:at + n])[0]))
            at += n
        elif t == "f":
            out.append("%s:f:%s" % (name, f32_text(b[at:at + 4])))
            at += 4
        elif t in "ZH":
            z = b.index(b"\0", at)
            out.append("%s:%s:%s" % (name, t, b[at:z].decode()))
            at = z + 1
        elif t == "B":
            sub = chr(b[at])
            cnt = struct.unpack("<i", b[at + 1:at + 5])[0]
            at += 5
            if sub == "f":
                vals = [f32_text(b[at + 4 * k:at + 4 * k + 4]) for k in range(cnt)]
                at += 4 * cnt
            else:
                fmt = _B_FMT[sub][0]
                n = struct.calcsize(fmt)
                vals = [str(x) for x in struct.unpack("<%d%s" % (cnt, fmt), b[at:at + n * cnt])]
                at += n * cnt
            out.append("%s:B:%s" % (name, ",".join([sub] + vals)))
        else:
            raise ValueError("unknown tag type %r" % t)
    if at != end:
        raise ValueError("tags run past the record")
    return out


def bam_to_sam(data, ref_names=None):
    """SAM lines of a BAM stream (with its header: the header's lines first) or of bare records (ref_names needed)"""
    lines, at = [], 0
    if data[:4] == b"BAM\1":
        l_text = struct.unpack("<i", data[4:8])[0]
        text = data[8:8 + l_text].decode()
        lines += text.split("\n")[:-1] if text.endswith("\n") else text.split("\n")
        at = 8 + l_text
        n_ref = struct.unpack("<i", data[at:at + 4])[0]
        at += 4
        ref_names = []
        for _ in range(n_ref):
            l_name = struct.unpack("<i", data[at:at + 4])[0]
            ref_names.append(data[at + 4:at + 4 + l_name - 1].decode())
            at += 4 + l_name + 4
    while at < len(data):
        bs = struct.unpack("<i", data[at:at + 4])[0]
        b = data[at + 4:at + 4 + bs]
        if len(b) != bs:
            raise ValueError("the stream ends inside a record")
        ref_id, pos, l_name, mapq, _bin, n_op, flag, l_seq, nref, npos, tlen = struct.unpack("<iiBBHHHiiii", b[:32])
        p = 32
        qname = b[p:p + l_name - 1].decode()
        p += l_name
        words = struct.unpack("<%dI" % n_op, b[p:p + 4 * n_op])
        p += 4 * n_op
        packed = np.frombuffer(b[p:p + (l_seq + 1) // 2], np.uint8)
        p += (l_seq + 1) // 2
        codes = np.empty(2 * len(packed), np.uint8)
        codes[0::2], codes[1::2] = packed >> 4, packed & 15
        seq = "".join(SEQ_CODES[c] for c in codes[:l_seq]) if l_seq else "*"
        q = b[p:p + l_seq]
        p += l_seq
        qual = "*" if l_seq == 0 or q == b"\xff" * l_seq else (np.frombuffer(q, np.uint8) + 33).astype(np.uint8).tobytes().decode()
        cigar = "".join("%d%s" % (w >> 4, CIGAR_OPS[w & 15]) for w in words) if n_op else "*"
        f = [qname, str(flag), ref_names[ref_id] if ref_id >= 0 else "*", str(pos + 1), str(mapq), cigar, "*" if nref < 0 else ref_names[nref], str(npos + 1), str(tlen),
             seq, qual] + _decode_tags(b, p, bs)
        lines.append("\t".join(f))
        at += 4 + bs
    return lines


def normal(line):
    """a SAM line as the decoder prints it: SEQ upper-cased, every float as the shortest text of its float32 (B:f arrays too)"""
    f = line.split("\t")
    if line.startswith("@") or len(f) < 11:
        return line
    f[9] = f[9].upper()
    for i in range(11, len(f)):
        if f[i][2:5] == ":f:":
            f[i] = f[i][:5] + f32_text(_f32(f[i][5:]))
        elif f[i][2:6] == ":B:f":
            f[i] = f[i][:6] + "".join("," + f32_text(_f32(x)) for x in f[i][7:].split(",") if f[i][6:])
    return "\t".join(f)

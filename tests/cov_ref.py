"""Coverage and depth from BAM records: an independent restatement, in Python, of the section "Coverage" of include/gdiet_hip.h.  Written
from that text alone -- nothing here is taken from csrc/ -- with a plain numpy depth array per contig and no difference trick, so that
the 64-lane statements (csrc/cov.h through tests/emul/cov_emul.cpp) and the kernels can be compared against it integer for integer.

  coverage(data, ref_lens, excl_flags=0x704, min_mapq=0, window=0) -> Cov
      .summary   dict of the ten counters
      .contigs   one dict per contig: n_reads cov_bases sum_depth sum_mapq sum_baseq n_baseq
      .depth     one uint32 array per contig
      .windows   None, or per contig (cov_bases uint32 array, sum_depth uint64 array)
      .bad       None, or (index of the first bad record, reason): reason is one of REASONS
  split(data)                 the records of a stream
  sam_depth(lines, refs, ...) the second oracle: FLAG, RNAME, POS, MAPQ, CIGAR and QUAL of SAM text, accumulated by brute force
  coverage_tsv / regions_bed  the two text files of Coverage.write, from a Cov and the contig names"""
import re
import struct

import numpy as np

SUMMARY = ("records", "unmapped", "secondary", "supplementary", "primary_mapped", "reverse", "excluded_by_flag", "excluded_by_mapq", "counted", "bad")
CONTIG = ("n_reads", "cov_bases", "sum_depth", "sum_mapq", "sum_baseq", "n_baseq")
REASONS = (None, "ref", "pos", "op", "ref_end", "qry_end", "cg", "aux", "fields")  # in the order the header lists them; the index is the library's code
_AUX_SIZE = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


class Cov:
    pass


def split(data):
    out, at = [], 0
    while at < len(data):
        bs = struct.unpack_from("<i", data, at)[0]
        assert bs >= 32 and at + 4 + bs <= len(data), "not a stream of whole records"
        out.append(data[at:at + 4 + bs])
        at += 4 + bs
    return out


def _cg_array(b, at):
    """the operations of the first CG tag in the aux fields b[at:], which must be CG:B:I; raises ValueError("cg" | "aux")"""
    n = len(b)
    while at < n:
        if n - at < 3:
            raise ValueError("aux")
        name, t = b[at:at + 2], chr(b[at + 2])
        at += 3
        if t in _AUX_SIZE:
            size = _AUX_SIZE[t]
        elif t in "ZH":
            z = b.find(b"\0", at)
            if z < 0:
                raise ValueError("aux")
            size = z + 1 - at
        elif t == "B":
            if n - at < 5:
                raise ValueError("aux")
            sub, cnt = chr(b[at]), struct.unpack_from("<i", b, at + 1)[0]
            if sub not in "cCsSiIf" or cnt < 0:
                raise ValueError("aux")
            size = 5 + _AUX_SIZE[sub] * cnt
            if name == b"CG":
                if sub != "I" or at + size > n:
                    raise ValueError("cg")
                return list(struct.unpack_from("<%dI" % cnt, b, at + 5))
        else:
            raise ValueError("aux")
        if name == b"CG":
            raise ValueError("cg")
        if at + size > n:
            raise ValueError("aux")
        at += size
    raise ValueError("cg")


def parse(rec):
    """(fields dict, reason or None) of one record with its block_size; the fields that could be read are there either way"""
    b = rec[4:]
    ref_id, pos, l_name, mapq, _bin, n_op, flag, l_seq = struct.unpack_from("<iiBBHHHi", b, 0)
    f = dict(ref_id=ref_id, pos=pos, mapq=mapq, flag=flag, l_seq=l_seq, ops=[], qual=None)
    if l_seq < 0:
        return f, "fields"
    cig_at = 32 + l_name
    qual_at = cig_at + 4 * n_op + (l_seq + 1) // 2
    if qual_at + l_seq > len(b):
        return f, "fields"
    words = list(struct.unpack_from("<%dI" % n_op, b, cig_at))
    if l_seq > 0 and b[qual_at] != 0xff:
        f["qual"] = np.frombuffer(b, np.uint8, l_seq, qual_at)
    if n_op == 2 and words[0] == (l_seq << 4 | 4) and words[1] & 15 == 3:
        try:
            words = _cg_array(b, qual_at + l_seq)
        except ValueError as e:
            return f, str(e)
    f["ops"] = [(w & 15, w >> 4) for w in words]
    return f, None


def coverage(data, ref_lens, excl_flags=0x704, min_mapq=0, window=0):
    n_ref = len(ref_lens)
    depth = [np.zeros(n, np.int64) for n in ref_lens]
    S = dict.fromkeys(SUMMARY, 0)
    contigs = [dict.fromkeys(CONTIG, 0) for _ in ref_lens]
    bad = None
    for index, rec in enumerate(split(data)):
        f, reason = parse(rec)
        flag, rid, pos = f["flag"], f["ref_id"], f["pos"]
        S["records"] += 1
        S["unmapped"] += bool(flag & 4)
        S["secondary"] += bool(flag & 0x100)
        S["supplementary"] += bool(flag & 0x800)
        S["primary_mapped"] += not flag & 0x904
        S["reverse"] += bool(flag & 0x10) and not flag & 4
        if reason is None:
            ref_end = pos + sum(n for op, n in f["ops"] if op in (0, 2, 3, 7, 8))
            qry_end = sum(n for op, n in f["ops"] if op in (0, 1, 4, 7, 8))
            if rid >= n_ref:
                reason = "ref"
            elif rid >= 0 and pos < 0:
                reason = "pos"
            elif any(op > 8 for op, _ in f["ops"]):
                reason = "op"
            elif rid >= 0 and ref_end > ref_lens[rid]:
                reason = "ref_end"
            elif f["l_seq"] > 0 and qry_end > f["l_seq"]:
                reason = "qry_end"
        if reason is not None:
            S["bad"] += 1
            if bad is None:
                bad = (index, reason)
            continue
        if flag & excl_flags:
            S["excluded_by_flag"] += 1
            continue
        if f["mapq"] < min_mapq:
            S["excluded_by_mapq"] += 1
            continue
        if rid < 0:
            continue
        S["counted"] += 1
        c = contigs[rid]
        c["n_reads"] += 1
        c["sum_mapq"] += f["mapq"]
        r, q = pos, 0
        for op, n in f["ops"]:
            if op in (0, 7, 8):
                depth[rid][r:r + n] += 1
                c["sum_depth"] += n
                if f["qual"] is not None:
                    c["sum_baseq"] += int(f["qual"][q:q + n].sum(dtype=np.int64))
                    c["n_baseq"] += n
                r, q = r + n, q + n
            elif op in (2, 3):
                r += n
            elif op in (1, 4):
                q += n
    out = Cov()
    out.summary, out.contigs, out.bad = S, contigs, bad
    out.depth = [d.astype(np.uint32) for d in depth]
    for c, d in zip(contigs, depth):
        c["cov_bases"] = int((d > 0).sum())
    out.windows = None
    if window > 0:
        out.windows = []
        for d in depth:
            edges = range(0, len(d), window)
            out.windows.append((np.array([int((d[e:e + window] > 0).sum()) for e in edges], np.uint32), np.array([int(d[e:e + window].sum()) for e in edges], np.uint64)))
    return out


# ---- the second oracle: SAM text ---------------------------------------------------------------------------------------------------
_OP = re.compile(r"(\d+)([MIDNSHP=X])")


def sam_depth(lines, ref_names, ref_lens, excl_flags=0x704, min_mapq=0):
    """(depth arrays, per-contig dicts without cov_bases filled from anything but depth, records counted) of SAM lines, by brute force: one
    position at a time, from the text fields alone"""
    depth = [[0] * n for n in ref_lens]
    contigs = [dict.fromkeys(CONTIG, 0) for _ in ref_lens]
    counted = 0
    for l in lines:
        if not l or l.startswith("@"):
            continue
        f = l.split("\t")
        flag, rname, pos, mapq, cigar, qual = int(f[1]), f[2], int(f[3]) - 1, int(f[4]), f[5], f[10]
        if flag & excl_flags or mapq < min_mapq or rname == "*":
            continue
        rid = list(ref_names).index(rname)
        counted += 1
        c = contigs[rid]
        c["n_reads"] += 1
        c["sum_mapq"] += mapq
        r, q = pos, 0
        for n, op in _OP.findall("" if cigar == "*" else cigar):
            for _ in range(int(n)):
                if op in "M=X":
                    depth[rid][r] += 1
                    c["sum_depth"] += 1
                    if qual != "*":
                        c["sum_baseq"] += ord(qual[q]) - 33
                        c["n_baseq"] += 1
                    r, q = r + 1, q + 1
                elif op in "DN":
                    r += 1
                elif op in "IS":
                    q += 1
    for c, d in zip(contigs, depth):
        c["cov_bases"] = sum(1 for x in d if x > 0)
    return [np.array(d, np.uint32) for d in depth], contigs, counted


# ---- the text files ----------------------------------------------------------------------------------------------------------------
def _ratio(num, den, fmt, scale=1.0):
    return fmt % (scale * num / den) if den else "0"


def coverage_tsv(cov, names, ref_lens):
    out = ["#rname\tstartpos\tendpos\tnumreads\tcovbases\tcoverage\tmeandepth\tmeanbaseq\tmeanmapq"]
    for name, n, c in zip(names, ref_lens, cov.contigs):
        out.append("\t".join([name, "1", str(n), str(c["n_reads"]), str(c["cov_bases"]), _ratio(c["cov_bases"], n, "%.6g", 100.0), _ratio(c["sum_depth"], n, "%.6g"),
                              _ratio(c["sum_baseq"], c["n_baseq"], "%.3g"), _ratio(c["sum_mapq"], c["n_reads"], "%.3g")]))
    out.append("#summary\t" + "\t".join("%s=%d" % (k, cov.summary[k]) for k in SUMMARY))
    return "\n".join(out) + "\n"


def regions_bed(cov, names, ref_lens, window):
    out = []
    for name, n, (_, sums) in zip(names, ref_lens, cov.windows):
        for k, s in enumerate(sums):
            beg, end = k * window, min(n, (k + 1) * window)
            out.append("%s\t%d\t%d\t%.2f" % (name, beg, end, int(s) / (end - beg)))
    return "".join(x + "\n" for x in out)

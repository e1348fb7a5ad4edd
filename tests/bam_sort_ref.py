"""Coordinate order and the BAI index: an independent restatement, in Python, of the section "Sorted BAM output" of include/gdiet_hip.h
(SAM specification 5.2 / 5.3 with this project's choices).  Written from that text alone -- nothing here is taken from csrc/ -- so that
the 64-lane code, the kernels, the merge plan and the index builder can be compared against it byte for byte.

  split(data)                      the records of a stream of bare records, as bytes objects (each with its block_size)
  key(rec)                         the 64-bit sort key of a record
  sort_records(data)               the records in coordinate order (Python's sorted: stable)
  rows(data)                       one tuple (key, offset, refID, pos, end, bin, flag) per record of a stream, in stream order
  members(raw)                     [(input bytes, file bytes)] of the BGZF members of a file, read from the file itself
  bai(rows, n_ref, base, records_len, log)   the bytes of the .bai file
  parse_bai(b), query(index, stream, log, base, ref, beg, end), brute(stream, base, ref, beg, end)
                                   a BAI reader with the region query of section 5.3, and the overlap scan it must agree with"""
import struct
import zlib

PSEUDO_BIN = 37450


def split(data):
    out, at = [], 0
    while at < len(data):
        n = struct.unpack_from("<i", data, at)[0] + 4
        assert n >= 36 and at + n <= len(data)
        out.append(data[at:at + n])
        at += n
    return out


def fields(rec):
    """(refID, pos, l_name, bin, n_cigar_op, flag) of a record"""
    ref_id, pos, l_name, _mapq, bin_, n_op, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    return ref_id, pos, l_name, bin_, n_op, flag


def key(rec):
    ref_id, pos, _, _, _, flag = fields(rec)
    return (ref_id & 0xffffffff) << 32 | ((((pos + 1) & 0xffffffff) << 1) & 0xffffffff) | (flag >> 4 & 1)


def sort_records(data):
    return b"".join(sorted(split(data), key=key))


def ref_len(rec):
    _, _, l_name, _, n_op, _ = fields(rec)
    words = struct.unpack_from("<%dI" % n_op, rec, 36 + l_name)
    return sum(w >> 4 for w in words if (w & 15) in (0, 2, 3, 7, 8)) & 0xffffffff


def _i32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v >> 31 else v


def rows(data):
    out, at = [], 0
    for rec in split(data):
        ref_id, pos, _, bin_, _, flag = fields(rec)
        out.append((key(rec), at, ref_id, pos, _i32(pos + max(ref_len(rec), 1)), bin_, flag))
        at += len(rec)
    return out


# ---- the container -----------------------------------------------------------------------------------------------------------------
def members(raw):
    """[(ISIZE, BSIZE + 1)] of every member of a BGZF file, the end-of-file member included"""
    out, at = [], 0
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 12:at + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        out.append((struct.unpack_from("<I", raw, at + bsize - 4)[0], bsize))
        at += bsize
    assert at == len(raw)
    return out


def stored_members(stream, member_in=65280):
    """the member log of a file that holds the stream in stored (uncompressed) members: 18 + (5 + n) + 8 bytes each"""
    log = [(min(member_in, len(stream) - at), 18 + 5 + min(member_in, len(stream) - at) + 8) for at in range(0, len(stream), member_in)]
    return log + [(0, 28)]


def zlib_members(stream, level=6, member_in=65280):
    log = []
    for at in range(0, len(stream), member_in):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = c.compress(stream[at:at + member_in]) + c.flush()
        log.append((len(stream[at:at + member_in]), 18 + len(body) + 8))
    return log + [(0, 28)]


def voffset(log, x):
    """the virtual offset of stream offset x: in the first member that ends behind x; the end of the stream is where the data members end"""
    in_at = file_at = 0
    for n_in, n_file in log:
        if n_in and x < in_at + n_in:
            return file_at << 16 | (x - in_at)
        in_at, file_at = in_at + n_in, file_at + n_file
    data_end = sum(n_file for n_in, n_file in log)
    # members without input behind the last data member (the end-of-file member) hold no offset: the end is where they start
    for n_in, n_file in reversed(log):
        if n_in:
            break
        data_end -= n_file
    return data_end << 16


def stream_offset(log, v):
    """the inverse of voffset for offsets inside data members"""
    in_at = file_at = 0
    for n_in, n_file in log:
        if file_at == v >> 16 and n_in:
            return in_at + (v & 0xffff)
        in_at, file_at = in_at + n_in, file_at + n_file
    return in_at  # the end


# ---- the index ---------------------------------------------------------------------------------------------------------------------
def bai(rws, n_ref, base, records_len, log):
    out = [b"BAI\1", struct.pack("<i", n_ref)]
    starts = [voffset(log, base + r[1]) for r in rws]
    ends = [voffset(log, base + (rws[i + 1][1] if i + 1 < len(rws) else records_len)) for i in range(len(rws))]
    placed = 0
    for ref in range(n_ref):
        mine = [i for i, r in enumerate(rws) if r[2] == ref]
        placed += len(mine)
        if not mine:
            out.append(struct.pack("<ii", 0, 0))
            continue
        bins, lin, prev = {}, {}, None
        for i in mine:
            _, _, _, pos, end, bin_, _ = rws[i]
            if prev is not None and prev == i - 1 and rws[prev][5] == bin_:
                bins[bin_][-1][1] = ends[i]
            else:
                bins.setdefault(bin_, []).append([starts[i], ends[i]])
            prev = i
            w0 = max(pos, 0) >> 14
            w1 = max((max(end, 1) - 1) >> 14, w0)
            for w in range(w0, w1 + 1):
                lin.setdefault(w, starts[i])
        out.append(struct.pack("<i", len(bins) + 1))
        for b in sorted(bins):
            out.append(struct.pack("<Ii", b, len(bins[b])) + b"".join(struct.pack("<QQ", c[0], c[1]) for c in bins[b]))
        n_un = sum(1 for i in mine if rws[i][6] & 4)
        out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, starts[mine[0]], ends[mine[-1]], len(mine) - n_un, n_un))
        n_intv = max(lin) + 1
        vals, nxt = [0] * n_intv, 0
        for w in range(n_intv - 1, -1, -1):
            nxt = lin.get(w, nxt)
            vals[w] = nxt
        out.append(struct.pack("<i", n_intv) + struct.pack("<%dQ" % n_intv, *vals))
    out.append(struct.pack("<Q", len(rws) - placed))
    return b"".join(out)


def parse_bai(b):
    assert b[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<i", b, 4)[0]
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", b, at)[0]
        at += 4
        bins, pseudo = {}, None
        for _ in range(n_bin):
            bin_, n_chunk = struct.unpack_from("<Ii", b, at)
            at += 8
            chunks = [struct.unpack_from("<QQ", b, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            if bin_ == PSEUDO_BIN:
                pseudo = chunks
            else:
                assert bin_ not in bins
                bins[bin_] = chunks
        n_intv = struct.unpack_from("<i", b, at)[0]
        lin = list(struct.unpack_from("<%dQ" % n_intv, b, at + 4))
        at += 4 + 8 * n_intv
        refs.append((bins, pseudo, lin))
    n_no_coor = struct.unpack_from("<Q", b, at)[0]
    assert at + 8 == len(b)
    return refs, n_no_coor


def reg2bins(beg, end):
    """the bins that may hold records overlapping [beg, end) (SAM specification 5.3)"""
    end -= 1
    out = [0]
    for shift, offset in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += list(range(offset + (beg >> shift), offset + (end >> shift) + 1))
    return out


def query(index, stream, log, base, ref, beg, end):
    """the records of reference `ref` that overlap [beg, end), through the index: the chunks of the region's bins that end behind the
    linear index's offset for beg's window, read record by record; returns the set of the records' stream offsets"""
    refs, _ = index
    bins, _pseudo, lin = refs[ref]
    w = beg >> 14
    min_off = lin[w] if w < len(lin) else (lin[-1] if lin else 0)
    got = set()
    for b in reg2bins(beg, end):
        for c_beg, c_end in bins.get(b, ()):
            if c_end <= min_off:
                continue
            at, stop = stream_offset(log, c_beg), stream_offset(log, c_end)
            while at < stop:
                n = struct.unpack_from("<i", stream, at)[0] + 4
                rec = stream[at:at + n]
                ref_id, pos, _, _, _, _ = fields(rec)
                if ref_id == ref and pos < end and pos + max(ref_len(rec), 1) > beg:
                    got.add(at - base)
                at += n
    return got


def brute(stream, base, ref, beg, end):
    got, at = set(), base
    while at < len(stream):
        n = struct.unpack_from("<i", stream, at)[0] + 4
        rec = stream[at:at + n]
        ref_id, pos, _, _, _, _ = fields(rec)
        if ref_id == ref and pos < end and pos + max(ref_len(rec), 1) > beg:
            got.add(at - base)
        at += n
    return got

"""inputs of the BAM input tests (tests/test_bam_in.py on the CPU, tests/test_bam_in_gpu.py on the GPU): records packed by hand, the
tags at the edges of every type, streams around them, and the helpers that read a file through the library."""
import gzip
import os
import struct
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bam_ref  # noqa: E402
import bgzf_inputs  # noqa: E402
import make_ubam  # noqa: E402

LENGTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257]
GOLDENS = ["lr/hifi.fq.gz", "lr/hifi_n.fq.gz", "lr/edge.fq.gz", "sr/sr.fq.gz", "sr/edge.fq.gz"]


def rec(name, codes, qual, flag=4, cigar=(), ref_id=-1, pos=-1, mapq=0, aux=b"", nul=True):
    """one alignment record: codes are the 4-bit codes of SEQ, qual the raw quality bytes (None: 0xFF)"""
    l_seq = len(codes)
    c = list(codes) + [0] * (l_seq & 1)
    packed = bytes(c[i] << 4 | c[i + 1] for i in range(0, len(c), 2))
    q = bytes([0xff] * l_seq) if qual is None else bytes(qual)
    nm = name + (b"\0" if nul else b"")
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(nm), mapq, 4680, len(cigar), flag, l_seq, -1, -1, 0) + nm
    body += struct.pack("<%dI" % len(cigar), *cigar) + packed + q + aux
    return struct.pack("<i", len(body)) + body


def hand_records(rng):
    """every length of LENGTHS on both strands, with quality and with 0xFF, all 16 codes; names of 1 and 254 bytes; aligned records with
    a CIGAR and reference fields; secondary and supplementary records between kept ones"""
    out = []
    for n in LENGTHS:
        for flag in (4, 20):
            for has_q in (True, False):
                codes = rng.integers(0, 16, size=n).tolist()
                out.append(rec(b"r%d_%d_%d" % (n, flag, has_q), codes, rng.integers(0, 94, size=n).tolist() if has_q else None, flag))
    out.append(rec(b"all16", list(range(16)), list(range(16))))
    out.append(rec(b"all16r", list(range(16)), list(range(16)), 16))
    out.append(rec(b"x", [1, 2, 4, 8], [0, 1, 2, 93]))
    out.append(rec(b"n" * 254, [1, 2, 4, 8, 15], [40] * 5, 16))
    out.append(rec(b"sec", [1] * 10, [30] * 10, 0x100, cigar=(10 << 4,), ref_id=0, pos=5))
    out.append(rec(b"aln", [1, 2, 4, 8] * 5, list(range(20)), 0, cigar=(3 << 4 | 4, 15 << 4, 2 << 4 | 4), ref_id=1, pos=99, mapq=60, aux=bam_ref.encode_tag("NM:i:0")))
    out.append(rec(b"sup", [2] * 7, [30] * 7, 0x800 | 16, cigar=(7 << 4,), ref_id=0, pos=1))
    out.append(rec(b"alnr", [1, 2, 4, 8, 15] * 3, list(range(15)), 16, cigar=(15 << 4,), ref_id=0, pos=0, mapq=3))
    out.append(rec(b"both", [8] * 3, [1] * 3, 0x900))
    out.append(rec(b"q255", [1, 2], [0, 0xff]))  # 0xFF behind the first quality byte is a quality like any other
    return out


TAGS = ["XA:A:!", "XB:A:~", "c0:i:-128", "c1:i:-1", "C0:i:0", "C1:i:255", "s0:i:-32768", "s1:i:-129", "S0:i:256", "S1:i:65535", "i0:i:-2147483648", "i1:i:-32769",
        "I0:i:65536", "I1:i:4294967295", "f0:f:0", "f1:f:-0", "f2:f:0.5", "f3:f:3.1415927", "f4:f:0.0000000001", "f5:f:100000000000000000000", "f6:f:16777216",
        "f7:f:-1.17549435e-38", "f8:f:3.4028235e38", "f9:f:0.1", "fa:f:1e-45", "Z0:Z:", "Z1:Z:text with spaces", "H0:H:", "H1:H:1AE301", "Bc:B:c,-128,127", "BC:B:C,0,255",
        "Bs:B:s,-32768,32767", "BS:B:S,0,65535", "Bi:B:i,-2147483648,2147483647", "BI:B:I,0,4294967295", "Bf:B:f,0.5,-2,1e20", "Be:B:C", "MM:Z:C+m,1,3;", "ML:B:C,200,13"]


def tag_records():
    """records carrying TAGS: all on one record, one each, and none; explicit c s i types for non-negative values too"""
    all_ = b"".join(bam_ref.encode_tag(t) for t in TAGS)
    wide = b"pc" + b"c" + struct.pack("<b", 5) + b"ps" + b"s" + struct.pack("<h", 5) + b"pi" + b"i" + struct.pack("<i", 5) + b"fn" + b"f" + struct.pack("<I", 0x7fc00000) + \
        b"fi" + b"f" + struct.pack("<f", float("inf")) + b"fm" + b"f" + struct.pack("<f", float("-inf"))
    out = [rec(b"tags_all", [1, 2, 4, 8], [30] * 4, 4, aux=all_), rec(b"tags_none", [1], [1]), rec(b"tags_wide", [1, 2], [1, 2], 16, aux=wide)]
    out += [rec(b"tag%d" % i, [1, 2, 3], None, 4, aux=bam_ref.encode_tag(t)) for i, t in enumerate(TAGS)]
    return out


def stream(records, text="@HD\tVN:1.6\tSO:unknown\n", refs=(("chr1", 1000), ("chr2", 2000))):
    return bam_ref.bam_header(text, list(refs)) + b"".join(records)


def golden_stream(rel, **kw):
    with gzip.open(os.path.join(ROOT, "tests", "golden", rel), "rb") as f:
        return make_ubam.ubam_stream(f.read(), **kw)


def write_bgzf(path, data, member_bytes=bgzf_inputs.MAX_MEMBER_BYTES, level=6, eof=True):
    with open(path, "wb") as f:
        f.write(b"".join(bgzf_inputs.members_of(data, member_bytes, level)) + (bgzf_inputs.EOF_MARKER if eof else b""))
    return path


def read_all(pkg, path, chunk=10 ** 9, threads=1, ctx=None, with_qual=True, with_comment=False, frag_mode=False):
    """([(rows, closed early)], error message or None, stats, format) of a whole file; rows as FastxReader.read returns them"""
    out, err = [], None
    with pkg.FastxReader(path, threads=threads, ctx=ctx) as r:
        while True:
            try:
                b = r.read(chunk, with_qual=with_qual, with_comment=with_comment, frag_mode=frag_mode)
            except pkg.GdietError as e:
                err = str(e)
                break
            if not b and not r.truncated_now:
                break
            out.append((b, r.truncated_now))
        return out, err, r.stats(), r.format()


def rows_of(batches):
    return [x for b, _ in batches for x in b]


def expected(reads):
    """the restatement's reads in the order of FastxReader.read's tuples"""
    return [(n, s, q, c) for n, c, s, q, _ in reads]

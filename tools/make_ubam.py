#!/usr/bin/env python3
"""FASTA / FASTQ (plain or gzip) in, unaligned BAM out: the shape in which PacBio instruments deliver HiFi reads, for tests and for the
files of measurements.  Pure Python: the records are packed by tests/bam_ref.py, the members written by tests/bgzf_inputs.py.

    python tools/make_ubam.py reads.fq[.gz] reads.bam [--level 6] [--member-bytes 65280] [--flag 4] [--tags] [--no-qual]

Every read becomes one record: refID -1, pos -1, MAPQ 0, no CIGAR, FLAG --flag (4: unmapped).  With a FLAG that holds 0x10 the record
stores the reverse complement of the read and its quality reversed, as an aligner would, so a reader that restores the original
strand returns the FASTQ's read.  --tags takes the comment of the header line as SAM tags joined by tabs (MM:Z:..., ML:B:C,...) and
stores them as aux fields; a comment that is no list of tags is an error.  Without it comments are dropped.  Letters outside
=ACMGRSVTWYHKDBN become N and case is lost: BAM holds sixteen codes.  The header holds @HD VN:1.6 SO:unknown and no reference."""
import argparse
import gzip
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import bam_ref  # noqa: E402
import bgzf_inputs  # noqa: E402

HEADER_TEXT = "@HD\tVN:1.6\tSO:unknown\n"
_COMP = bytes.maketrans(b"ACGTMRWSYKVHDBNacgtmrwsykvhdbn", b"TGCAKYWSRMBDHVNtgcakywsrmbdhvn")


def fastx_records(data):
    """(name, comment or None, seq, qual or None) of FASTA / FASTQ text, multi-line records included"""
    lines = data.split(b"\n")
    i, n = 0, len(lines)
    while i < n:
        line = lines[i].rstrip(b"\r")
        i += 1
        if not line or line[:1] not in b">@":
            continue
        body = line[1:]
        k = next((j for j, c in enumerate(body) if c in b" \t\v\f\r"), len(body))
        name, comment = body[:k], body[k + 1:]  # the name ends at the first white space; the rest of the line is the comment
        seq = []
        while i < n and lines[i][:1] not in (b">", b"@", b"+"):
            seq.append(lines[i].rstrip(b"\r"))
            i += 1
        seq = b"".join(seq)
        qual = None
        if i < n and lines[i][:1] == b"+":
            i += 1
            q = b""
            while i < n and len(q) < len(seq):
                q += lines[i].rstrip(b"\r")
                i += 1
            if len(q) != len(seq):
                raise ValueError("read %s: SEQ and QUAL differ in length" % name.decode())
            qual = q
        yield name, comment or None, seq, qual


def record(name, seq, qual, flag=4, tags=()):
    """one unaligned record through bam_ref.encode_record; the strand of FLAG 0x10 is applied here"""
    if flag & 0x10:
        seq = seq.translate(_COMP)[::-1]
        qual = qual[::-1] if qual is not None else None
    f = [name.decode("latin1"), str(flag), "*", "0", "0", "*", "*", "0", "0", seq.decode("latin1") or "*",
         (qual.decode("latin1") if qual is not None and seq else "*")] + list(tags)
    return bam_ref.encode_record("\t".join(f), [])


def ubam_stream(data, flag=4, tags=False, with_qual=True, header_text=HEADER_TEXT, refs=()):
    """the uncompressed BAM stream of FASTA / FASTQ text"""
    out = [bam_ref.bam_header(header_text, list(refs))]
    for name, comment, seq, qual in fastx_records(data):
        t = comment.decode("latin1").split("\t") if tags and comment else []
        out.append(record(name, seq, qual if with_qual else None, flag, t))
    return b"".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--level", type=int, default=6, choices=range(0, 10))
    ap.add_argument("--member-bytes", type=int, default=bgzf_inputs.MAX_MEMBER_BYTES)
    ap.add_argument("--flag", type=int, default=4, help="FLAG of every record (default 4: unmapped)")
    ap.add_argument("--tags", action="store_true", help="the FASTQ comment holds SAM tags: store them as aux fields")
    ap.add_argument("--no-qual", action="store_true", help="store 0xff in place of the qualities")
    a = ap.parse_args()
    if not 1 <= a.member_bytes <= bgzf_inputs.MAX_MEMBER_BYTES:
        ap.error("--member-bytes must be 1 .. %d" % bgzf_inputs.MAX_MEMBER_BYTES)
    with open(a.src, "rb") as probe:
        gz = probe.read(2) == b"\x1f\x8b"
    with (gzip.open(a.src, "rb") if gz else open(a.src, "rb")) as f:
        stream = ubam_stream(f.read(), a.flag, a.tags, not a.no_qual)
    n_out = 0
    with open(a.dst, "wb") as out:
        group = a.member_bytes * 256
        for i in range(0, len(stream), group):
            c = b"".join(bgzf_inputs.members_of(stream[i:i + group], a.member_bytes, a.level))
            out.write(c)
            n_out += len(c)
        out.write(bgzf_inputs.EOF_MARKER)
        n_out += len(bgzf_inputs.EOF_MARKER)
    print("%s -> %s: %d bytes of BAM in %d bytes, members of %d bytes at level %d" % (a.src, a.dst, len(stream), n_out, a.member_bytes, a.level))


if __name__ == "__main__":
    main()

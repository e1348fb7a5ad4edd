"""Reference files for the reference-input tests (tests/test_ref_fasta.py on the CPU, tests/test_ref_fasta_gpu.py on the GPU), built in pure
Python, deterministically, from the committed tests/golden/{lr,sr,rep}/ref.fa.gz.

  canonical   the references re-wrapped at 60, 70, 1023, 1024 and 1025 columns and as single lines, with and without a final newline,
              plain, gzip and BGZF.  Nothing in them disqualifies a block (csrc/ref_fasta.h): the device places every base.  lr and sr
              take the whole product; rep (3 Mbases) two widths, plain and BGZF.
  odd         files the device claims as well although they look unusual: blank lines, spaces and tabs inside sequence lines, lower case
              and IUPAC codes, an empty contig, duplicate names, headers with comments, a header line of 1 500 bytes, contigs of 1, 7, 8
              and 9 bases (contig boundaries inside a word of S), a file that is only a header.
  awkward     files with at least one block only the sequential grammar reads: "\\r\\n" line ends, a FASTQ-format reference, a sequence
              line that starts with '+' and one that starts with '@', junk in front of the first '>' -- each carrying some of the odd
              features as well -- and the empty file, which holds no block at all.
`files(dir)` writes them once and returns {name: path}; GROUPS says which group a name belongs to.
"""
import gzip
import hashlib
import io
import os

import bgzf_inputs
from fixture_io import LR, REP, SR

WIDTHS = (60, 70, 1023, 1024, 1025, 0)  # 0: every contig on a single line
IUPAC = "RYKMSWBDHVN"


def _records(path):
    names, seqs = [], []
    for line in gzip.open(path, "rt"):
        line = line.rstrip("\n")
        if line.startswith(">"):
            names.append(line[1:])
            seqs.append([])
        else:
            seqs[-1].append(line)
    return names, ["".join(s) for s in seqs]


def wrap(names, seqs, width, final_newline=True, eol="\n"):
    out = []
    for n, s in zip(names, seqs):
        out.append(">" + n)
        out.extend([s] if width == 0 else [s[i:i + width] for i in range(0, len(s), width)])
    text = eol.join(out) + eol
    return (text if final_newline else text[:-len(eol)]).encode()


def _gzip(data):
    b = io.BytesIO()
    with gzip.GzipFile(fileobj=b, mode="wb", compresslevel=6, mtime=0) as f:
        f.write(data)
    return b.getvalue()


def _rng_bytes(tag, n):
    out, i = b"", 0
    while len(out) < n:
        out += hashlib.sha256(("%s/%d" % (tag, i)).encode()).digest()
        i += 1
    return out[:n]


def _mutate(seq, tag):
    """lower case on a stretch, IUPAC codes sprinkled in: deterministic"""
    r = _rng_bytes(tag, len(seq) // 97 + 1)
    s = list(seq)
    for j, b in enumerate(r):
        s[min(j * 97 + b % 97, len(s) - 1)] = IUPAC[b % len(IUPAC)]
    s = "".join(s)
    third = len(s) // 3
    return s[:third] + s[third:2 * third].lower() + s[2 * third:]


def canonical():
    out = {}
    for tag, d in (("lr", LR), ("sr", SR), ("rep", REP)):
        names, seqs = _records(os.path.join(d, "ref.fa.gz"))
        for width in WIDTHS if tag != "rep" else (60, 1024):
            for nl in (True, False) if tag != "rep" else (True,):
                text = wrap(names, seqs, width, nl)
                stem = "%s_w%d_%s" % (tag, width, "nl" if nl else "nonl")
                out[stem + ".fa"] = text
                if tag != "rep":
                    out[stem + ".fa.gz"] = _gzip(text)
                out[stem + ".fa.bgz"] = bgzf_inputs.bgzf(text)
    return out


def _small():
    names, seqs = _records(os.path.join(LR, "ref.fa.gz"))
    return [s[:l] for s, l in zip(seqs * 2, (9000, 7001, 5003, 3000, 2500, 1200))]


def odd():
    p = _small()
    out = {}
    # blank lines (also in front of the first sequence line and doubled), spaces and tabs inside sequence lines, lower case, IUPAC
    s0, s1 = _mutate(p[0], "odd0"), _mutate(p[1], "odd1")
    lines = [">blank one", ""]
    for i in range(0, len(s0), 70):
        l = s0[i:i + 70]
        lines.append(l[:20] + " " + l[20:40] + "\t" + l[40:] if (i // 70) % 5 == 2 else l)
        if (i // 70) % 7 == 3:
            lines += ["", ""]
    lines += [">blank two\tcomment with > and @ and + inside", " " + s1[:50], s1[50:]]
    out["odd_blank_space_iupac.fa"] = ("\n".join(lines) + "\n").encode()
    # an empty contig, duplicate names, comments, a header line of 1 500 bytes, contigs of 1, 7, 8 and 9 bases, no final newline
    long_hdr = ">long " + ("x" * 57 + " ") * 26
    long_hdr = long_hdr[:1500]
    assert len(long_hdr) == 1500
    lines = [">dup first", p[2][:1], ">empty", ">dup second", p[2][1:8], ">c8 eight", p[2][8:16], ">c9", p[2][16:25], long_hdr]
    lines += [p[3][i:i + 60] for i in range(0, len(p[3]), 60)] + [">dup", p[4][:777], ">last"]
    out["odd_tiny_dup_longhdr.fa"] = "\n".join(lines).encode()
    out["odd_only_header.fa"] = b">alone with a comment\n"
    return out


def awkward():
    p = _small()
    out = {}
    names = ["crlf1 a comment", "crlf2", "dup", "dup"]
    text = wrap(names, [_mutate(p[0], "crlf"), p[1], p[2][:9], p[3]], 60, True, "\r\n")
    out["awk_crlf.fa"] = text.replace(b">crlf2\r\n", b">crlf2\r\n\r\n", 1)  # (and a blank "\r\n" line)
    # a reference in FASTQ format: four-line records and one whose sequence and quality wrap
    q = lambda n, tag: bytes(33 + b % 41 for b in _rng_bytes(tag, n)).replace(b"@", b"I").replace(b"+", b"J").decode()
    fq = ["@fq1 comment", _mutate(p[0], "fq"), "+", q(len(p[0]), "q1"), "@fq2", p[1][:3000], p[1][3000:], "+fq2", q(3000, "q2a"), q(len(p[1]) - 3000, "q2b"),
          "@fq3", p[2], "+", q(len(p[2]), "q3")]
    out["awk_ref.fq"] = ("\n".join(fq) + "\n").encode()
    # a sequence line that starts with '+': the record ends there, the line behind it is read as its quality string, and the scan for
    # the next header goes on from there.  A sequence line that starts with '@': a record of that name begins.
    w = 60
    a = [p[0][i:i + w] for i in range(0, 1200, w)]
    plus = [">plus", a[0], "+" + a[1], a[2], a[3], a[4]]
    at = [">at spaces inside", a[5][:30] + " " + a[5][30:], "@" + a[6] + " rest", a[7], a[8], ">after", p[4][:1], ">c7", p[4][1:8], ">c8", p[4][8:16], ">c9", p[4][16:25]]
    tail = [">tail"] + [p[1][i:i + w] for i in range(0, len(p[1]), w)]
    out["awk_plus_at.fa"] = ("\n".join(plus + at + tail) + "\n").encode()
    # junk in front of the first '>' -- the first record starts at the first '>' or '@' anywhere, not only at a line start
    junk = ["# a comment line", "", "more junk >early name", p[5][:100]]
    rest = [">empty", ">real"] + [p[3][i:i + 70] for i in range(0, len(p[3]), 70)]
    out["awk_junk_front.fa"] = ("\n".join(junk + rest) + "\n").encode()
    out["awk_empty.fa"] = b""
    return out


GROUPS = {}
_contents = {}


def contents():
    """{name: bytes} of every input, made once per process; fills GROUPS"""
    if not _contents:
        for g, f in (("canonical", canonical), ("odd", odd), ("awkward", awkward)):
            for k, v in f().items():
                _contents[k] = v
                GROUPS[k] = g
    return _contents


_written = {}


def files(directory):
    """writes every input below `directory` once per process; {name: path}"""
    if directory not in _written:
        os.makedirs(directory, exist_ok=True)
        paths = {}
        for k, v in contents().items():
            paths[k] = os.path.join(directory, k)
            with open(paths[k], "wb") as f:
                f.write(v)
        _written[directory] = paths
    return _written[directory]


def group(name):
    if not GROUPS:
        contents()
    return GROUPS[name]

"""CPU: BAM input (include/gdiet_hip.h "BAM input"; csrc/bam_in.h, the BAM grammar of csrc/fastx_reader.h) against its restatement
tests/bam_in_ref.py, and against the FASTQ reader on the FASTQ twin of a file.  tests/emul/bam_in_emul.cpp runs the walk, the statements of
bam_unpack_kernel as 64 lanes in both orders on exact-size buffers, and the host grammar inside a real GdFastx as a stand-alone program
under AddressSanitizer / UBSan; the unattached reader is also driven through the library, as every caller drives it.
tests/test_bam_in_gpu.py repeats the comparisons with the kernel."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_pkg
import bam_in_inputs as bi
import bam_in_ref as ref
import bam_ref
from fixture_io import SR, golden_sam, read_fasta, read_fastq


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bam_in") / "bam_in_emul")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "genome-on-diet_amd", "csrc"), os.path.join(ROOT, "tests", "emul", "bam_in_emul.cpp"), "-o", exe, "-lz", "-pthread"])
    return exe


def emul_unpack(emul, records, with_qual, tmp_path, status=0):
    """(text, off[n, 4], lens) of bam_in_emul unpack; its stderr when status is not 0"""
    src, dst = str(tmp_path / "recs.bin"), str(tmp_path / "unpacked.bin")
    with open(src, "wb") as f:
        f.write(records)
    r = subprocess.run([emul, "unpack", src, str(int(with_qual)), dst], capture_output=True, text=True)
    assert r.returncode == status, (r.returncode, r.stderr[-2000:])
    if status:
        return r.stderr
    raw = open(dst, "rb").read()
    head, rest = raw.split(b"\n", 1)
    n, text_len = (int(x) for x in head.split())
    off = np.frombuffer(rest[:32 * n], np.int64).reshape(n, 4)
    lens = np.frombuffer(rest[32 * n:36 * n], np.int32)
    text = rest[36 * n:]
    assert len(text) == text_len
    return text, off, lens


def unpacked_reads(records, text, off, lens):
    """(name, None, seq, qual, len) per row of an unpack result, as the restatement lists reads"""
    out = []
    for (o_name, _, o_seq, o_qual), n in zip(off.tolist(), lens.tolist()):
        name = records[o_name:records.index(b"\0", o_name)]
        assert text[o_seq + n] == 0 and (o_qual < 0 or text[o_qual + n] == 0)
        out.append((name, None, text[o_seq:o_seq + n], None if o_qual < 0 else text[o_qual:o_qual + n], n))
    return out


def emul_read(emul, path, tmp_path, chunk=10 ** 9, with_qual=True, with_comment=False, frag=False, threads=1, env=None):
    """([(rows, closed early)], rc, message, (host, device, format)) of bam_in_emul read"""
    dst = str(tmp_path / "read.out")
    subprocess.run([emul, "read", path, str(chunk), str(int(with_qual)), str(int(with_comment)), str(int(frag)), str(threads), dst], check=True,
                   env=dict(os.environ, **(env or {})))
    raw = open(dst, "rb").read()
    at, batches = 0, []

    def line():
        nonlocal at
        e = raw.index(b"\n", at)
        s, at = raw[at:e], e + 1
        return s

    def field():
        nonlocal at
        n = int(line())
        if n < 0:
            return None
        s, at = raw[at:at + n], at + n + 1
        return s
    while True:
        l = line()
        if l.startswith(b"E "):
            rc, msg = int(l.split(b" ", 2)[1]), l.split(b" ", 2)[2].decode()
            st = tuple(int(x) for x in line().split()[1:])
            return batches, rc, msg, st
        _, n, bad = l.split()
        rows = []
        for _ in range(int(n)):
            name, comment, seq, qual = field(), field(), field(), field()
            rows.append((name, seq, qual, comment))
        batches.append((rows, bool(int(bad))))


def test_the_complement_is_the_bit_reversal_and_the_writers():
    """three statements of one table: the letters' meaning (bam_in_ref), the 4-bit reversal of the code, and what the writer's restatement
    stores for the complemented letter"""
    for c in range(16):
        rev = int(format(c, "04b")[::-1], 2)
        assert ref.COMPLEMENT[c] == ref.LETTERS[rev], c
    comp = bytes.maketrans(b"ACGTMRWSYKVHDBN=", b"TGCAKYWSRMBDHVN=")
    assert ref.LETTERS.translate(comp) == ref.COMPLEMENT


@pytest.mark.parametrize("with_qual", [True, False])
def test_hand_built_records_through_the_lanes(with_qual, emul, tmp_path):
    records = b"".join(bi.hand_records(np.random.default_rng(5)))
    want, status, _ = ref.records_of(records, 0, with_qual)
    assert status == "ok" and len(want) == 4 * len(bi.LENGTHS) + 7
    got = unpacked_reads(records, *emul_unpack(emul, records, with_qual, tmp_path))
    assert got == want
    assert {r[4] for r in want} >= set(bi.LENGTHS) and any(r[3] is None for r in want) == True  # noqa: E712
    assert b"sec" not in [r[0] for r in want] and b"sup" not in [r[0] for r in want] and b"both" not in [r[0] for r in want]
    assert (b"all16", None, b"=ACMGRSVTWYHKDBN", bytes(range(33, 49)) if with_qual else None, 16) in want
    assert (b"all16r", None, b"NVHMDRWABSYCKGT=", bytes(range(48, 32, -1)) if with_qual else None, 16) in want


def test_unpack_refuses_a_range_that_is_no_list_of_records(emul, tmp_path):
    good = bi.rec(b"a", [1, 2], [3, 4])
    assert "ends inside a record" in emul_unpack(emul, good + good[:-1], True, tmp_path, status=5)
    assert "BAM record 1 at offset %d" % len(good) in emul_unpack(emul, good + struct.pack("<i", 31) + b"\0" * 31, True, tmp_path, status=5)


@pytest.mark.parametrize("rel", bi.GOLDENS)
def test_goldens_as_bam_are_their_fastq(rel, tmp_path):
    """the reader's records of <golden>.bam are its records of the FASTQ, letters upper-cased (BAM holds no case), on either strand"""
    pkg = load_pkg()
    fq = os.path.join(ROOT, "tests", "golden", rel)
    want, err, _, fmt = bi.read_all(pkg, fq)
    assert err is None and fmt == "fastx"
    want = [(n, s.upper(), q, c) for n, s, q, c in bi.rows_of(want)]
    for flag, threads in ((4, 1), (20, 2), (4, 4)):
        s = bi.golden_stream(rel, flag=flag)
        assert bi.expected(ref.reads_of(s)[0]) == want
        path = bi.write_bgzf(str(tmp_path / "g.bam"), s)
        got, err, st, fmt = bi.read_all(pkg, path, threads=threads)
        assert err is None and fmt == "bam" and bi.rows_of(got) == want, (flag, threads)
        assert st["records_host"] == len(want) and st["records_device"] == 0
    got, err, _, _ = bi.read_all(pkg, path, with_qual=False)
    assert bi.rows_of(got) == [(n, s, None, c) for n, s, q, c in want]


@pytest.fixture(scope="module")
def mixed_stream():
    """hand-built records and tag records behind a header longer than a 4 096-byte block"""
    rng = np.random.default_rng(9)
    refs = [("contig_%d_%s" % (i, "x" * (i % 40)), 1000 + i) for i in range(150)]
    return bi.stream(bi.hand_records(rng) + bi.tag_records() + bi.hand_records(rng), "@HD\tVN:1.6\n@CO\t" + "c" * 900 + "\n", refs)


def test_every_tag_type_at_its_edges(mixed_stream, tmp_path):
    pkg = load_pkg()
    s = bi.stream(bi.tag_records())
    want, status, _ = ref.reads_of(s, with_comment=True)
    assert status == "ok"
    got, err, _, _ = bi.read_all(pkg, bi.write_bgzf(str(tmp_path / "t.bam"), s), with_comment=True, threads=2)
    assert err is None and bi.rows_of(got) == bi.expected(want)
    by_name = {r[0]: r[3] for r in bi.rows_of(got)}
    assert by_name[b"tags_none"] is None
    # the writer's restatement prints the same tags the same way (an independent second statement of the text forms)
    texts = by_name[b"tags_all"].decode().split("\t")
    assert texts == bam_ref.normal("\t".join(["x"] * 11 + bi.TAGS)).split("\t")[11:]
    assert by_name[b"tags_wide"] == b"pc:i:5\tps:i:5\tpi:i:5\tfn:f:nan\tfi:f:inf\tfm:f:-inf"
    for want_text in ("f0:f:0", "f1:f:-0", "f4:f:0.0000000001", "f5:f:100000000000000000000", "f9:f:0.1", "Z0:Z:", "H0:H:", "Be:B:C", "I1:i:4294967295", "c0:i:-128"):
        assert want_text in texts
    # every tag the comment holds goes back into a record unchanged: what -y needs
    assert b"".join(bam_ref.encode_tag(t) for t in texts) == b"".join(bam_ref.encode_tag(t) for t in bi.TAGS)


@pytest.mark.parametrize("block", [256, 4096, 0])
@pytest.mark.parametrize("member", [300, 4096, 65280])
def test_member_and_block_seams(member, block, mixed_stream, tmp_path, monkeypatch):
    """records, the block_size field itself and the header straddle members and reader blocks; 1, 2 and 4 threads"""
    pkg = load_pkg()
    if block:
        monkeypatch.setenv("GDIET_FASTX_BLOCK", str(block))
    else:
        monkeypatch.delenv("GDIET_FASTX_BLOCK", raising=False)
    want, status, _ = ref.reads_of(mixed_stream, with_comment=True)
    assert status == "ok" and len(want) == 2 * (4 * len(bi.LENGTHS) + 7) + len(bi.tag_records())
    path = bi.write_bgzf(str(tmp_path / "m.bam"), mixed_stream, member)
    for threads in (1, 2, 4):
        got, err, st, fmt = bi.read_all(pkg, path, chunk=700, threads=threads, with_comment=True)
        assert err is None and fmt == "bam" and bi.rows_of(got) == bi.expected(want), threads
        assert st["blocks"] > (1 if block and member < 65280 else 0)  # (a read takes whole members: one of 65 280 bytes holds the file)


def test_every_source_detects_bam(mixed_stream, tmp_path, monkeypatch, emul):
    """BGZF route, gzread (no end marker; GDIET_BGZF=0; single-stream gzip) and a raw uncompressed stream"""
    pkg = load_pkg()
    want = bi.expected(ref.reads_of(mixed_stream)[0])
    paths = [bi.write_bgzf(str(tmp_path / "a.bam"), mixed_stream), bi.write_bgzf(str(tmp_path / "b.bam"), mixed_stream, eof=False), str(tmp_path / "c.bam"), str(tmp_path / "d.bam")]
    with gzip.open(paths[2], "wb") as f:
        f.write(mixed_stream)
    with open(paths[3], "wb") as f:
        f.write(mixed_stream)
    for p in paths:
        got, err, _, fmt = bi.read_all(pkg, p)
        assert err is None and fmt == "bam" and bi.rows_of(got) == want, p
    monkeypatch.setenv("GDIET_BGZF", "0")
    got, err, _, fmt = bi.read_all(pkg, paths[0])
    assert err is None and fmt == "bam" and bi.rows_of(got) == want
    # and the stand-alone program under the sanitizers, with small blocks and comments
    want_c = bi.expected(ref.reads_of(mixed_stream, with_comment=True)[0])
    for threads in (1, 4):
        got, rc, msg, st = emul_read(emul, paths[3], tmp_path, chunk=500, with_comment=True, threads=threads, env={"GDIET_FASTX_BLOCK": "256"})
        assert rc == 0 and msg == "" and bi.rows_of(got) == want_c and st == (len(want_c), 0, 1)


@pytest.mark.parametrize("block", [256, 0])
def test_batches_are_those_of_the_fastq_twin(block, tmp_path, monkeypatch):
    """mm_bseq_read3's rule is untouched: at several chunk sizes, and in fragment mode on pairs, the batches of the BAM are the batches of
    the FASTQ it was made from"""
    pkg = load_pkg()
    if block:
        monkeypatch.setenv("GDIET_FASTX_BLOCK", str(block))
    fq = os.path.join(SR, "sr.fq.gz")
    bam = bi.write_bgzf(str(tmp_path / "sr.bam"), bi.golden_stream("sr/sr.fq.gz"), 300 if block else 65280)
    for chunk in (1, 1000, 45000, 10 ** 9):
        a, b = bi.read_all(pkg, bam, chunk, threads=2)[0], bi.read_all(pkg, fq, chunk)[0]
        assert a == b and len(a) == len(b)
    pairs = b"".join(b"@p%d/%d\n" % (i, m) + b"ACGT" * 25 + b"\n+\n" + b"I" * 100 + b"\n" for i in range(50) for m in (1, 2))
    fq = str(tmp_path / "pairs.fq")
    with open(fq, "wb") as f:
        f.write(pairs)
    bam = bi.write_bgzf(str(tmp_path / "pairs.bam"), bi.make_ubam.ubam_stream(pairs), 300)
    a, b = bi.read_all(pkg, bam, 250, frag_mode=True)[0], bi.read_all(pkg, fq, 250, frag_mode=True)[0]
    assert a == b and all(rows[-1][0].endswith(b"/2") for rows, _ in a) and len(a) > 10


def test_every_truncation_point(tmp_path):
    """a three-record file cut at every byte: the restatement's reads, and truncated exactly where it says so"""
    pkg = load_pkg()
    s = bi.stream([bi.rec(b"one", [1, 2, 4], [1, 2, 3]), bi.rec(b"two", [8] * 5, None, 16, aux=bam_ref.encode_tag("XX:Z:abc")), bi.rec(b"three", [15] * 4, [9] * 4)], refs=[("c", 5)])
    path = str(tmp_path / "cut.bam")
    seen = set()
    for cut in range(4, len(s) + 1):
        with open(path, "wb") as f:
            f.write(s[:cut])
        want, status, _ = ref.reads_of(s[:cut], with_comment=True)
        got, err, _, fmt = bi.read_all(pkg, path, with_comment=True)
        assert fmt == "bam" and err is None and bi.rows_of(got) == bi.expected(want), cut
        assert any(t for _, t in got) == (status == "truncated"), cut
        seen.add((len(want), status))
    assert seen == {(0, "truncated"), (0, "ok"), (1, "truncated"), (1, "ok"), (2, "truncated"), (2, "ok"), (3, "ok")}


def _bad_cases():
    good = bi.rec(b"good", [1, 2, 4, 8], [5] * 4)
    b = bytearray(good)
    cases = {}
    cases["block_size below 32"] = struct.pack("<i", 31) + bytes(31)
    x = bytearray(good); x[0:4] = struct.pack("<i", len(good) - 4 - 1); cases["fields past the record"] = bytes(x[:-1])  # noqa: E702
    x = bytearray(good); x[12] = 0; cases["l_read_name 0"] = bytes(x)  # noqa: E702
    cases["name without NUL"] = bi.rec(b"name", [1, 2], [1, 2], nul=False)
    x = bytearray(good); x[20:24] = struct.pack("<i", -1); cases["negative l_seq"] = bytes(x)  # noqa: E702
    cases["aux past the record"] = bi.rec(b"aux", [1], [1], aux=b"XXZabc")  # (only with comments)
    cases["aux of unknown type"] = bi.rec(b"aux", [1], [1], aux=b"XXq\0")
    cases["aux B count past the record"] = bi.rec(b"aux", [1], [1], aux=b"XXBi" + struct.pack("<i", 3) + bytes(8))
    del b
    return good, cases


@pytest.mark.parametrize("case", sorted(_bad_cases()[1]))
def test_malformed_records_are_read_errors_behind_the_good_ones(case, tmp_path):
    pkg = load_pkg()
    good, cases = _bad_cases()
    s = bi.stream([good, bi.rec(b"skipped", [1], [1], 0x100), good, cases[case], good])
    path = str(tmp_path / "bad.bam")
    with open(path, "wb") as f:
        f.write(s)
    for with_comment in (True, False):
        want, status, where = ref.reads_of(s, with_comment=with_comment)
        got, err, _, _ = bi.read_all(pkg, path, with_comment=with_comment, chunk=1)
        assert bi.rows_of(got) == bi.expected(want)
        if case.startswith("aux") and not with_comment:
            assert status == "ok" and err is None and len(want) == 4
        else:
            assert status == "error" and len(want) == 2 and where[0] == 3
            assert err is not None and "BAM record 3 at offset %d:" % where[1] in err, err
    with open(path, "wb") as f:
        f.write(b"BAM\1" + struct.pack("<i", -5) + bytes(40))
    got, err, _, _ = bi.read_all(pkg, path)
    assert got == [] and "l_text" in err


def test_single_byte_mutations_under_the_sanitizers(emul, tmp_path, mixed_stream):
    """3 000 copies of a small file with one byte changed, read with 1, 2 and 3 threads in blocks of 256 bytes and with comments: any
    outcome but a sanitizer report, an abort or a hang"""
    small = bi.stream(bi.hand_records(np.random.default_rng(2))[:24] + bi.tag_records()[:3], refs=[("c", 5)])
    src = str(tmp_path / "small.bam")
    with open(src, "wb") as f:
        f.write(small)
    r = subprocess.run([emul, "mutate", src, "3000", "7", str(tmp_path / "mut.bam"), "1"], capture_output=True, text=True, timeout=300, env=dict(os.environ, GDIET_FASTX_BLOCK="256"))
    assert r.returncode == 0, r.stderr[-3000:]
    clean, trunc, errors = (int(x.split()[0]) for x in r.stdout.split(",")[:3])
    print(r.stdout)
    assert clean + trunc + errors == 3000 and clean > 0 and errors > 0


def test_the_writers_output_read_back_gives_the_reads():
    """bam_ref.sam_to_bam of the sr golden SAM (primary records on both strands, unmapped ones too): read back, the reads that went in"""
    names, _ = read_fasta(os.path.join(SR, "ref.fa.gz"))
    lines = golden_sam("sr")
    s = bam_ref.bam_header("", [(n, 1) for n in names]) + bam_ref.sam_to_bam(lines, names)
    flags = [int(l.split("\t")[1]) for l in lines if not l.startswith("@")]
    assert sum(1 for f in flags if f & 16 and not f & 0x900) > 100 and sum(1 for f in flags if not f & 16 and not f & 0x904) > 100
    reads, status, _ = ref.reads_of(s)
    want = [(n.encode(), None, q.upper().encode(), ql.encode(), len(q)) for n, q, ql in read_fastq(os.path.join(SR, "sr.fq.gz"))]
    assert status == "ok" and reads == want
    pkg = load_pkg()
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        got, err, _, _ = bi.read_all(pkg, bi.write_bgzf(os.path.join(d, "rt.bam"), s), threads=2)
    assert err is None and bi.rows_of(got) == bi.expected(want)

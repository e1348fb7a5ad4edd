"""GPU: BAM records encoded on the device (bam_encode_kernel) through every entry point -- Mapper.bam_header / bam_batch / bam_batch_raw,
BgzfWriter.write_bam on a writer with a context (the resident route: records encoded behind the writer's tail and compressed where they
are) and tools/map_file.py --bam from file to file.  The oracle is the SAM text of the same call shape (pinned to the reference by the
SAM tests) through the restatement tests/bam_ref.py, and the host emulator tests/emul/bam_emul.cpp fed with the very records."""
import ctypes as C
import gzip
import io
import json
import os
import struct
import subprocess
import sys
import types

import numpy as np
import pytest

import bam_ref
from conftest import ROOT
from fixture_io import OVERRIDES, SETS, read_fasta
import samopts_io as so
from test_samopts_gpu import under, write_fastq

pytestmark = pytest.mark.gpu

KINDS = ("sr", "hifi_sv", "ont_sv")
_mapped, _sam_of_tool = {}, {}


@pytest.fixture(scope="module")
def mapped(pkg, gpu_ctx):
    """kind -> (mapper, reads with comments, MapResult, plain BAM bytes), each kind mapped and encoded once for the module"""
    def get(kind):
        if kind not in _mapped:
            base, _, preset = SETS[kind]
            names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
            reads = so.reads_with_comments(kind)
            m = pkg.Mapper(gpu_ctx, names, seqs, preset=preset, **OVERRIDES.get(kind, {}))
            res = m.map([r[1] for r in reads])
            _mapped[kind] = (m, reads, res, m.bam_batch(res, reads))
        return _mapped[kind]
    yield get
    for m, _, _, _ in _mapped.values():
        m.close()
    _mapped.clear()


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bam_gpu") / "bam_emul")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "genome-on-diet_amd", "csrc"), os.path.join(ROOT, "tests", "emul", "bam_emul.cpp"), "-o", exe])
    return exe


def dump_of(m, reads, res, flag, rg=None):
    """the emulator's dump of a MapResult: every field of every record as the library returned it"""
    t = ["MODE\tsam", "FLAG\t%d" % flag] + (["RG\t" + rg] if rg else []) + ["SQ\t%s\t%d" % (n, l) for n, l in zip(m.names, m.lens)]
    for i, r in enumerate(reads):
        t.append("READ\t%s\t%s\t%s" % (r[0], r[1], r[2] if r[2] is not None else "*"))
        if len(r) > 3 and r[3] is not None:
            t.append("COMMENT\t" + r[3])
        for j in range(res.n_regs[i]):
            g = res.regs[i][j]
            nums = [g.id, g.cnt, g.rid, g.score, g.qs, g.qe, g.rs, g.re, g.parent, g.subsc, g.mlen, g.blen, g.mapq, g.rev, g.sam_pri, g.dp_score, g.dp_max, g.n_ambi, 1]
            cg = "".join("%d%s" % (g.cigar[k] >> 4, "MIDNSHP=XB"[g.cigar[k] & 15]) for k in range(g.n_cigar))
            t.append("REG\t%s\t%s\t-" % (" ".join(str(x) for x in nums), cg))
    return "\n".join(t) + "\n"


def emul_bytes(emul, text, tmp_path):
    path, out = str(tmp_path / "in.txt"), str(tmp_path / "out.bam")
    with open(path, "w") as f:
        f.write(text)
    r = subprocess.run([emul, "fmt", path, out], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return open(out, "rb").read()


@pytest.mark.parametrize("kind", KINDS)
def test_bam_batch_is_the_function_of_the_sam_text(kind, mapped, emul, tmp_path):
    """plain and under the all-options mode (-Y -y -R --sam-hit-only): the device's bytes are sam_to_bam of the SAM text of the same
    results, and the emulator's bytes for the very records"""
    m, reads, res, plain = mapped(kind)
    assert plain == bam_ref.sam_to_bam(m.sam_batch(res, reads), m.names)
    assert plain == emul_bytes(emul, dump_of(m, reads, res, 0), tmp_path)
    with under(m, "all"):
        got, sam, flag = m.bam_batch(res, reads), m.sam_batch(res, reads), m.opt.flag
    assert got == bam_ref.sam_to_bam(sam, m.names) and got != plain
    assert got == emul_bytes(emul, dump_of(m, reads, res, flag & (so.F_SOFTCLIP | so.F_COPY_COMMENT | so.F_SAM_HIT_ONLY), rg=so.RG_ARG), tmp_path)
    lines = bam_ref.bam_to_sam(got, m.names)
    assert len(lines) == sam.count("\n") and all("\tRG:Z:%s\t" % so.RG_ID in l for l in lines)


def test_bam_header(mapped):
    m = mapped("hifi_sv")[0]
    argv = ["prog", "-a", "x y"]
    try:
        m.set_read_group(so.RG_ARG)
        head = m.bam_header(so.VERSION, argv)
        assert head == bam_ref.bam_header(m.sam_header(so.VERSION, argv), list(zip(m.names, (int(x) for x in m.lens))))
        assert so.RG_LINE.encode() in head
    finally:
        m.set_read_group(None)
    assert m.bam_header() == bam_ref.bam_header(m.sam_header(), list(zip(m.names, (int(x) for x in m.lens))))


# ---- the smallest shapes at which the kernel can go wrong: hand-made gdiet_reg_t ---------------------------------------------------------
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257)


@pytest.fixture(scope="module")
def tiny(pkg, gpu_ctx):
    rng = np.random.default_rng(11)
    seqs = ["".join("ACGT"[c] for c in rng.integers(0, 4, n)) for n in (3000, 1500)]
    m = pkg.Mapper(gpu_ctx, ["t1", "t2"], seqs, preset="sr")
    yield m
    m.close()


class Batch:
    """C arrays of a hand-made batch; regs[i] = list of dicts (fields of gdiet_reg_t; `cigar` a list of words)"""

    def __init__(self, pkg, reads, regs):
        Reg = pkg.map_api.Reg
        n = len(reads)
        self.n, self.reads = n, reads
        self.names = (C.c_char_p * n)(*[r[0].encode() for r in reads])
        self.seqs = (C.c_char_p * n)(*[r[1].encode() for r in reads])
        self.quals = (C.c_char_p * n)(*[None if r[2] is None else r[2].encode() for r in reads])
        self.lens = np.array([len(r[1]) for r in reads], np.int32)
        self.lens_p = self.lens.ctypes.data_as(C.POINTER(C.c_int32))
        self.keep = []
        n_regs, arr = (C.c_int32 * n)(), (C.POINTER(Reg) * n)()
        for i, rr in enumerate(regs):
            n_regs[i] = len(rr)
            if rr:
                a = (Reg * len(rr))()
                for j, d in enumerate(rr):
                    cg = (C.c_uint32 * max(1, len(d["cigar"])))(*d["cigar"])
                    self.keep.append(cg)
                    for k, v in d.items():
                        if k != "cigar":
                            setattr(a[j], k, v)
                    a[j].n_cigar, a[j].cigar = len(d["cigar"]), C.cast(cg, C.POINTER(C.c_uint32))
                self.keep.append(a)
                arr[i] = C.cast(a, C.POINTER(Reg))
        self.res = types.SimpleNamespace(n_regs=n_regs, regs=arr)  # (no MapResult: these arrays are Python's, not the library's)


def make_reg(L, rev, n_ops, clip, j=0, parent=None, pri=1, rid=0, rs=100):
    """a record of read length L with n_ops operations alternating M and D (0: none), clip bases clipped at both ends"""
    qs, qe = (clip, L - clip) if L - 2 * clip >= 1 else (0, L)
    q = qe - qs
    n_m = (n_ops + 1) // 2
    if n_ops and n_m > q:
        n_ops, n_m = 1, 1
    cigar = []
    for k in range(n_ops):
        if k % 2 == 0:
            cigar.append((q // n_m + (1 if k // 2 < q % n_m else 0)) << 4)
        else:
            cigar.append((1 + k % 3) << 4 | 2)
    m_sum, d_sum = sum(c >> 4 for c in cigar if c & 15 == 0), sum(c >> 4 for c in cigar if c & 15 == 2)
    assert n_ops == 0 or m_sum == q
    return dict(id=j, cnt=3 + L, rid=rid, score=2 * L, qs=qs, qe=qe, rs=rs, re=rs + m_sum + d_sum, parent=j if parent is None else parent, subsc=L - 70000 if L & 1 else L,
                mlen=m_sum if n_ops else L, blen=m_sum + d_sum if n_ops else L, mapq=L % 61, rev=rev, sam_pri=pri, dp_score=q, dp_max=q + 1, n_ambi=L % 3, cigar=cigar)


def tiny_batch(pkg):
    rng = np.random.default_rng(5)
    reads, regs, k = [], [], 0
    for L in LENGTHS:
        for rev in (0, 1):
            seq = "".join("ACGTNacgtRYKMSWBDHVn"[c] for c in rng.integers(0, 20, L))
            qual = "".join(chr(33 + c) for c in rng.integers(0, 94, L))
            name = "rdxy"[:1 + k % 4] if k < 4 else "%s%d" % ("abcd"[:1 + k % 4][:max(1, 1 + k % 4 - len(str(k)))], k)
            n_ops = (0, 1, 64, 65)[k % 4] if L >= 63 else (0, 1)[k % 2]
            if L >= 63 and k % 8 >= 4:
                n_ops = (65, 64, 1, 0)[k % 4]
            reads.append((name, seq, qual))
            regs.append([make_reg(L, rev, n_ops, clip=(0, 1, 2, 5)[(k // 2) % 4], rid=k % 2, rs=17 * k)])
            k += 1
    reads.append(("un", "ACGTNNA", "IIIIIII"))                     # an unmapped read
    regs.append([])
    reads.append(("sec", "ACGTACGTACGTA", "ABCDEFGHIJKLM"))          # a primary and a secondary record: SEQ * on the second
    regs.append([make_reg(13, 0, 1, 0), make_reg(13, 1, 1, 2, j=1, parent=0, rid=1)])
    reads.append(("nq", "ACGTACGTAC" * 13, None))                   # no qualities
    regs.append([make_reg(130, 1, 64, 1)])
    reads.append(("sup", "ACGTTGCA" * 20, "I" * 160))                # a supplementary record: hard clips and the slice of SEQ / QUAL
    regs.append([make_reg(160, 0, 1, 0), make_reg(160, 1, 65, 7, j=1, pri=0, rid=1)])
    return Batch(pkg, reads, regs)


def test_shape_of_the_hand_made_batch(pkg):
    """the variable part of a record starts at every offset modulo 4, and every operation count occurs on both strands"""
    b = tiny_batch(pkg)
    assert {len(r[0]) % 4 for r in b.reads} == {0, 1, 2, 3} and [len(r[0]) for r in b.reads[:4]] == [1, 2, 3, 4]
    seen = {(b.res.regs[i][0].n_cigar, b.res.regs[i][0].rev) for i in range(2 * len(LENGTHS))}
    assert seen >= {(n, r) for n in (0, 1, 64, 65) for r in (0, 1)}
    assert [len(r[1]) for r in b.reads[:2 * len(LENGTHS):2]] == list(LENGTHS)


@pytest.mark.parametrize("flag", [0, so.F_SOFTCLIP, so.F_NO_QUAL, 0x4000], ids=["plain", "Y", "Q", "no2nd"])
def test_hand_made_records(flag, tiny, pkg):
    b = tiny_batch(pkg)
    old = tiny.opt.flag
    tiny.opt.flag = old | flag
    try:
        sam = tiny.sam_batch_raw(b.res, b.n, b.names, b.seqs, b.quals, b.lens_p)
        bam = tiny.bam_batch_raw(b.res, b.n, b.names, b.seqs, b.quals, b.lens_p)
    finally:
        tiny.opt.flag = old
    want = bam_ref.sam_to_bam(sam, tiny.names)
    assert len(bam) == len(want) and bam == want
    lines = bam_ref.bam_to_sam(bam, tiny.names)
    assert len(lines) == len(b.reads) + (1 if flag == 0x4000 else 2)
    if flag == 0:
        sec = [l.split("\t") for l in lines if l.startswith("sec\t")]
        assert sec[1][1] == "272" and sec[1][9:11] == ["*", "*"] and [l.split("\t")[10] for l in lines if l.startswith("nq\t")] == ["*"]
        assert [l.split("\t")[5][-2:] for l in lines if l.startswith("sup\t")][1] == "7H"


def test_single_record_and_empty_batches(tiny, pkg):
    one = Batch(pkg, [("q", "ACGTA", "IIIII")], [[make_reg(5, 1, 1, 1)]])
    bam = tiny.bam_batch_raw(one.res, 1, one.names, one.seqs, one.quals, one.lens_p)
    assert bam == bam_ref.sam_to_bam(tiny.sam_batch_raw(one.res, 1, one.names, one.seqs, one.quals, one.lens_p), tiny.names) and len(bam) > 40
    none = Batch(pkg, [("u1", "ACGT", "IIII"), ("u2", "AC", None)], [[], []])
    old = tiny.opt.flag
    tiny.opt.flag = old | so.F_SAM_HIT_ONLY
    try:
        assert tiny.bam_batch_raw(none.res, 2, none.names, none.seqs, none.quals, none.lens_p) == b""  # no record, and no failure
    finally:
        tiny.opt.flag = old
    assert len(bam_ref.bam_to_sam(tiny.bam_batch_raw(none.res, 2, none.names, none.seqs, none.quals, none.lens_p), tiny.names)) == 2


def test_refusals_name_the_read(tiny, pkg):
    bad = Batch(pkg, [("fine", "ACGT", "IIII", "XX:i:1"), ("culprit", "ACGT", "IIII", "free text")], [[], []])
    cm = (C.c_char_p * 2)(b"XX:i:1", b"free text")
    old = tiny.opt.flag
    tiny.opt.flag = old | so.F_COPY_COMMENT
    try:
        with pytest.raises(pkg.GdietError, match="culprit"):
            tiny.bam_batch_raw(bad.res, 2, bad.names, bad.seqs, bad.quals, bad.lens_p, comments=cm)
    finally:
        tiny.opt.flag = old
    assert len(tiny.bam_batch_raw(bad.res, 2, bad.names, bad.seqs, bad.quals, bad.lens_p, comments=cm)) > 0  # without -y nobody looks at it
    long_name = Batch(pkg, [("n" * 255, "ACGT", "IIII")], [[]])
    with pytest.raises(pkg.GdietError, match="254"):
        tiny.bam_batch_raw(long_name.res, 1, long_name.names, long_name.seqs, long_name.quals, long_name.lens_p)


# ---- the resident route -----------------------------------------------------------------------------------------------------------
def members_of(raw):
    out, at = [], 0
    while at < len(raw):
        bsize = struct.unpack("<H", raw[at + 16:at + 18])[0] + 1
        out.append(raw[at:at + bsize])
        at += bsize
    assert at == len(raw)
    return out


def test_resident_route(mapped, pkg, gpu_ctx, tmp_path):
    """BgzfWriter(path, ctx): header, two batches through write_bam, close.  The file inflates to header + the two bam_batch results; every
    member is Context.bgzf_deflate of its own 65280-byte slice (a member depends on its input alone: the tail was carried from call to
    call and the resident input is the same input); every member was compressed on the device"""
    m, reads, res, plain = mapped("sr")
    head = m.bam_header(so.VERSION, ["x"])
    cut = 701
    parts = []
    path = str(tmp_path / "out.bam")
    with pkg.BgzfWriter(path, ctx=gpu_ctx) as w:
        w.write(head)
        for lo, hi in ((0, cut), (cut, len(reads))):
            rr = reads[lo:hi]
            n = len(rr)
            qn = (C.c_char_p * n)(*[r[0].encode() for r in rr])
            sq = (C.c_char_p * n)(*[r[1].encode() for r in rr])
            ql = (C.c_char_p * n)(*[r[2].encode() for r in rr])
            lens = np.array([len(r[1]) for r in rr], np.int32)
            sub = types.SimpleNamespace(n_regs=(C.c_int32 * n)(*res.n_regs[lo:hi]), regs=(C.POINTER(pkg.map_api.Reg) * n)(*[res.regs[i] for i in range(lo, hi)]))
            lp = lens.ctypes.data_as(C.POINTER(C.c_int32))
            parts.append(m.bam_batch_raw(sub, n, qn, sq, ql, lp))
            w.write_bam(m, sub, n, qn, sq, ql, lp)
    st = w.stats()
    stream = head + parts[0] + parts[1]
    assert parts[0] + parts[1] == plain and all(len(p) % 65280 for p in (head, head + parts[0], stream))
    raw = open(path, "rb").read()
    assert gzip.decompress(raw) == stream
    mem = members_of(raw)
    n_data = (len(stream) + 65279) // 65280
    assert len(mem) == n_data + 1 and len(mem[-1]) == 28
    for k in range(n_data):
        assert mem[k] == gpu_ctx.bgzf_deflate(stream[65280 * k:65280 * (k + 1)], eof=False), k
    assert (st["members_device"], st["members_host"], st["bytes_in"]) == (n_data, 0, len(stream))
    assert w.stats()["bytes_out"] == len(raw)


def test_write_bam_on_a_host_writer(mapped, pkg, tmp_path):
    m, reads, res, plain = mapped("ont_sv")
    path = str(tmp_path / "host.bam")
    with pkg.BgzfWriter(path, level=1, threads=2) as w:
        w.write(m.bam_header())
        n = len(reads)
        qn, sq, ql = ((C.c_char_p * n)(*[r[k].encode() for r in reads]) for k in range(3))
        lens = np.array([len(r[1]) for r in reads], np.int32)
        w.write_bam(m, res, n, qn, sq, ql, lens.ctypes.data_as(C.POINTER(C.c_int32)))
        st = w.stats()
    assert gzip.decompress(open(path, "rb").read()) == m.bam_header() + plain and st["members_device"] == 0 and st["members_host"] > 0
    sink = io.BytesIO()
    assert m.bam_batch_raw(res, n, qn, sq, ql, lens.ctypes.data_as(C.POINTER(C.c_int32)), sink=sink) == len(plain) and sink.getvalue() == plain


# ---- the tool ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["device", "host"])
@pytest.mark.parametrize("kind", ["sr", "hifi_sv"])
def test_map_file_bam(kind, route, tmp_path):
    """tools/map_file.py --bam from file to file: the decoded BAM is the --header SAM output of the same configuration, line for line
    (floats as the float32 of their text); -Y, -y and -R ride along"""
    fq, bam, sam = str(tmp_path / "reads.fq"), str(tmp_path / "out.bam"), str(tmp_path / "out.sam")
    write_fastq(kind, fq)
    base = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "map_file.py"), "--preset", SETS[kind][2], "-R", so.RG_ARG, "-Y", "-y",
            os.path.join(SETS[kind][0], "ref.fa.gz"), fq]
    r = subprocess.run(base + ["--bam", "--bgzf", route, "-o", bam], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rep = json.loads(r.stdout.strip().split("\n")[-1])
    assert rep["bam"] is True and rep["bgzf_out"]["route"] == route and rep["bgzf_out"]["members_device" if route == "host" else "members_host"] == 0
    assert rep["bgzf_out"]["members_host" if route == "host" else "members_device"] > 0
    if kind not in _sam_of_tool:  # (one SAM run per kind serves both routes)
        r = subprocess.run(base + ["--header", "-o", sam], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        _sam_of_tool[kind] = open(sam).read().split("\n")[:-1]
    raw = open(bam, "rb").read()
    assert raw.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    got = bam_ref.bam_to_sam(gzip.decompress(raw))
    want = _sam_of_tool[kind]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w.startswith("@PG"):  # the command lines differ: --bam --bgzf <route> -o x.bam against --header -o x.sam
            assert g.startswith("@PG\tID:minimap2\tPN:minimap2\tVN:") and "--bam" in g
        else:
            assert g == bam_ref.normal(w), w.split("\t")[:4]

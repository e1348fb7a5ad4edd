"""GPU: SAM lines formatted on the device (sam_encode_kernel) through every entry point -- Mapper.sam_batch_raw(..., device=True),
BgzfWriter.write_sam on a writer with a context (the resident route: lines written behind the writer's tail and compressed where they are)
and on one without, and tools/map_file.py --sam-device from file to file.  The oracle is the host formatter's text for the same call
(pinned to the reference by the SAM tests), and the host emulator tests/emul/sam_emul.cpp fed with the very records."""
import ctypes as C
import gzip
import io
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT
from fixture_io import OVERRIDES, SETS, read_fasta
import samopts_io as so
from test_bam_gpu import Batch, KINDS, dump_of, members_of, tiny_batch
from test_sam_device import build_emul, cigar_of
from test_samopts_gpu import under, write_fastq

pytestmark = pytest.mark.gpu

_mapped = {}


@pytest.fixture(scope="module")
def mapped(pkg, gpu_ctx):
    """kind -> (mapper, reads with comments, MapResult, C arrays of the reads), each kind mapped once for the module"""
    def get(kind):
        if kind not in _mapped:
            base, _, preset = SETS[kind]
            names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
            reads = so.reads_with_comments(kind)
            m = pkg.Mapper(gpu_ctx, names, seqs, preset=preset, **OVERRIDES.get(kind, {}))
            res = m.map([r[1] for r in reads])
            _mapped[kind] = (m, reads, res, arrays(reads))
        return _mapped[kind]
    yield get
    for m, _, _, _ in _mapped.values():
        m.close()
    _mapped.clear()


def arrays(reads):
    n = len(reads)
    qn, sq, ql = ((C.c_char_p * n)(*[r[k].encode() for r in reads]) for k in range(3))
    cm = (C.c_char_p * n)(*[None if len(r) < 4 or r[3] is None else r[3].encode() for r in reads])
    lens = np.array([len(r[1]) for r in reads], np.int32)
    return n, qn, sq, ql, lens, lens.ctypes.data_as(C.POINTER(C.c_int32)), cm


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory.mktemp("sam_device_gpu"))


def emul_text(emul, text, tmp_path):
    path, out = str(tmp_path / "in.txt"), str(tmp_path / "out.sam")
    with open(path, "w") as f:
        f.write(text)
    r = subprocess.run([emul, "fmt", path, out], capture_output=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return open(out, "rb").read()


def both(m, res, a, comments=False):
    """(host text, device text) of sam_batch_raw for the same arguments"""
    n, qn, sq, ql, _, lp, cm = a
    host = m.sam_batch_raw(res, n, qn, sq, ql, lp, comments=cm if comments else None)
    dev = m.sam_batch_raw(res, n, qn, sq, ql, lp, comments=cm if comments else None, device=True)
    return host, dev


@pytest.mark.parametrize("kind", KINDS)
def test_device_text_is_the_host_text(kind, mapped, emul, tmp_path):
    """plain and under the all-options mode (-Y -y -R --sam-hit-only): the device's bytes are the host formatter's, and the emulator's for
    the very records"""
    m, reads, res, a = mapped(kind)
    host, dev = both(m, res, a)
    assert len(dev) == len(host) and dev == host and host.count(b"\n") >= len(reads)
    assert dev == emul_text(emul, dump_of(m, reads, res, 0), tmp_path)
    with under(m, "all"):
        host2, dev2 = both(m, res, a, comments=True)
        flag = m.opt.flag
    assert len(dev2) == len(host2) and dev2 == host2 and dev2 != dev and ("\tRG:Z:%s\t" % so.RG_ID).encode() in dev2
    assert dev2 == emul_text(emul, dump_of(m, reads, res, flag & (so.F_SOFTCLIP | so.F_COPY_COMMENT | so.F_SAM_HIT_ONLY), rg=so.RG_ARG), tmp_path)


# ---- the smallest shapes at which the kernel can go wrong: hand-made gdiet_reg_t ---------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(pkg, gpu_ctx):
    rng = np.random.default_rng(11)
    seqs = ["".join("ACGT"[c] for c in rng.integers(0, 4, n)) for n in (3000, 1500)]
    m = pkg.Mapper(gpu_ctx, ["t1", "t2"], seqs, preset="sr")
    yield m
    m.close()


_FIELDS = ("id", "cnt", "rid", "score", "qs", "qe", "rs", "re", "parent", "subsc", "mlen", "blen", "mapq", "rev", "sam_pri", "dp_score", "dp_max", "n_ambi")


def hand_made(pkg):
    """tiny_batch's reads and records (read lengths 1 .. 257 on both strands with 0 / 1 / 64 / 65 operations, the unmapped, secondary,
    no-quality and supplementary reads) and two more: 129 operations with lengths of 1 to 9 digits mixed, and the -L case of 65 534
    operations between two clips (65 536 with them: in the CG:B:I tag under -L, 1 025 rounds of the scan in the column without)"""
    b = tiny_batch(pkg)
    reads = list(b.reads)
    regs = [[dict({k: getattr(b.res.regs[i][j], k) for k in _FIELDS}, cigar=[b.res.regs[i][j].cigar[k] for k in range(b.res.regs[i][j].n_cigar)])
             for j in range(b.res.n_regs[i])] for i in range(b.n)]
    ops = cigar_of(129, True)
    q, ref = sum(n for n, op in ops if op == "M"), sum(n for n, _ in ops)
    reads.append(("wide", ("ACGTN" * (q + 9))[:q + 9], ("IJKLMNO" * (q + 9))[:q + 9]))
    regs.append([dict(id=0, cnt=1, rid=1, score=5, qs=2, qe=2 + q, rs=7, re=7 + ref, parent=0, subsc=0, mlen=q, blen=ref, mapq=3, rev=1, sam_pri=1, dp_score=9, dp_max=9, n_ambi=0,
                      cigar=[n << 4 | "MID".index(op) for n, op in ops])])
    n_ops = 65534
    L = 3 + n_ops + 5
    reads.append(("long", ("ACGT" * (L // 4 + 1))[:L], None))
    regs.append([dict(id=0, cnt=7, rid=0, score=70, qs=3, qe=3 + n_ops, rs=1000, re=1000 + n_ops // 2, parent=0, subsc=3, mlen=n_ops, blen=n_ops, mapq=33, rev=0, sam_pri=1, dp_score=90,
                      dp_max=91, n_ambi=0, cigar=[1 << 4 | (k & 1) for k in range(n_ops)])])
    return Batch(pkg, reads, regs)


@pytest.mark.parametrize("long_cigar", [0, so.F_LONG_CIGAR], ids=["", "L"])
@pytest.mark.parametrize("flag", [0, so.F_SOFTCLIP, so.F_NO_QUAL, 0x4000], ids=["plain", "Y", "Q", "no2nd"])
def test_hand_made_records(flag, long_cigar, tiny, pkg):
    b = hand_made(pkg)
    old = tiny.opt.flag
    tiny.opt.flag = old | flag | long_cigar
    try:
        host = tiny.sam_batch_raw(b.res, b.n, b.names, b.seqs, b.quals, b.lens_p)
        dev = tiny.sam_batch_raw(b.res, b.n, b.names, b.seqs, b.quals, b.lens_p, device=True)
    finally:
        tiny.opt.flag = old
    assert len(dev) == len(host)
    assert dev == host
    lines = host.decode().split("\n")[:-1]
    assert len(lines) == len(b.reads) + (1 if flag == 0x4000 else 2)
    assert ("\tCG:B:I,52," in lines[-1]) == bool(long_cigar) and lines[-1].split("\t")[5].startswith("65542S32767N" if long_cigar else "3S1M1I")
    assert "100000000D" in [l for l in lines if l.startswith("wide\t")][0].split("\t")[5]


def test_single_record_and_empty_batches(tiny, pkg):
    from test_bam_gpu import make_reg
    one = Batch(pkg, [("q", "ACGTA", "IIIII")], [[make_reg(5, 1, 1, 1)]])
    host = tiny.sam_batch_raw(one.res, 1, one.names, one.seqs, one.quals, one.lens_p)
    assert tiny.sam_batch_raw(one.res, 1, one.names, one.seqs, one.quals, one.lens_p, device=True) == host and host.count(b"\n") == 1
    none = Batch(pkg, [("u1", "ACGT", "IIII"), ("u2", "AC", None)], [[], []])
    old = tiny.opt.flag
    tiny.opt.flag = old | so.F_SAM_HIT_ONLY
    try:
        assert tiny.sam_batch_raw(none.res, 2, none.names, none.seqs, none.quals, none.lens_p, device=True) == b""  # no line, and no failure
    finally:
        tiny.opt.flag = old
    assert tiny.sam_batch_raw(none.res, 0, none.names, none.seqs, none.quals, none.lens_p, device=True) == b""
    host = tiny.sam_batch_raw(none.res, 2, none.names, none.seqs, none.quals, none.lens_p)
    assert tiny.sam_batch_raw(none.res, 2, none.names, none.seqs, none.quals, none.lens_p, device=True) == host and host.count(b"\n") == 2


def test_a_record_outside_its_read_names_the_read(tiny, pkg):
    from test_bam_gpu import make_reg
    bad = Batch(pkg, [("fine", "ACGT", "IIII"), ("culprit", "ACGT", "IIII")], [[make_reg(4, 0, 1, 0)], [dict(make_reg(4, 0, 1, 0), qe=5)]])
    with pytest.raises(pkg.GdietError, match="culprit"):
        tiny.sam_batch_raw(bad.res, 2, bad.names, bad.seqs, bad.quals, bad.lens_p, device=True)


# ---- the resident route -----------------------------------------------------------------------------------------------------------
def test_resident_route(mapped, pkg, gpu_ctx, tmp_path):
    """BgzfWriter(path, ctx): header text through write, two batches through write_sam with a cut inside, close.  The file inflates to
    header + the two host-formatted texts; every member is Context.bgzf_deflate of its own 65280-byte slice; every member was compressed
    on the device.  The same through a writer without a context gives an identical inflated stream."""
    m, reads, res, _ = mapped("sr")
    head = m.sam_header(so.VERSION, ["x"]).encode()
    cut = 701
    parts, subs = [], []
    for lo, hi in ((0, cut), (cut, len(reads))):
        a = arrays(reads[lo:hi])
        n = a[0]
        sub = types.SimpleNamespace(n_regs=(C.c_int32 * n)(*res.n_regs[lo:hi]), regs=(C.POINTER(pkg.map_api.Reg) * n)(*[res.regs[i] for i in range(lo, hi)]))
        subs.append((sub, a))
        parts.append(m.sam_batch_raw(sub, n, a[1], a[2], a[3], a[5]))  # the host formatter
    stream = head + parts[0] + parts[1]
    assert all(len(p) % 65280 for p in (head, head + parts[0], stream)) and len(stream) > 3 * 65280
    raws = []
    for ctx in (gpu_ctx, None):
        path = str(tmp_path / ("dev.sam.gz" if ctx is not None else "host.sam.gz"))
        with pkg.BgzfWriter(path, ctx=ctx, **({} if ctx is not None else dict(level=1, threads=2))) as w:
            w.write(head)
            for sub, a in subs:
                w.write_sam(m, sub, a[0], a[1], a[2], a[3], a[5])
        st = w.stats()
        raw = open(path, "rb").read()
        assert gzip.decompress(raw) == stream
        raws.append(raw)
        n_data = (len(stream) + 65279) // 65280
        if ctx is not None:
            mem = members_of(raw)
            assert len(mem) == n_data + 1 and len(mem[-1]) == 28
            for k in range(n_data):
                assert mem[k] == gpu_ctx.bgzf_deflate(stream[65280 * k:65280 * (k + 1)], eof=False), k
            assert (st["members_device"], st["members_host"], st["bytes_in"]) == (n_data, 0, len(stream)) and st["bytes_out"] == len(raw)
        else:
            assert st["members_device"] == 0 and st["members_host"] > 0
    # any other sink: the text is written from the kept buffer
    sub, a = subs[0]
    sink = io.BytesIO()
    assert m.sam_batch_raw(sub, a[0], a[1], a[2], a[3], a[5], sink=sink, device=True) == len(parts[0]) and sink.getvalue() == parts[0]


# ---- the tool ---------------------------------------------------------------------------------------------------------------------
def test_map_file_sam_device(tmp_path):
    """tools/map_file.py --sam-device from file to file on sr: plain output is the file written without the flag, --bgzf device inflates
    to it, and --sam-device --bam is an error; -Y, -y and -R ride along"""
    fq = str(tmp_path / "reads.fq")
    write_fastq("sr", fq)
    base = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "map_file.py"), "--preset", SETS["sr"][2], "-R", so.RG_ARG, "-Y", "-y",
            os.path.join(SETS["sr"][0], "ref.fa.gz"), fq]
    out = {}
    for name, extra in (("host", []), ("dev", ["--sam-device"]), ("bgzf", ["--sam-device", "--bgzf", "device"])):
        path = str(tmp_path / (name + ".sam"))
        r = subprocess.run(base + extra + ["-o", path], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        out[name] = open(path, "rb").read()
        assert ('"sam_device": true' in r.stdout) == bool(extra)
        if name == "bgzf":
            assert '"members_host": 0' in r.stdout
    assert len(out["host"]) > 100000 and out["dev"] == out["host"] and gzip.decompress(out["bgzf"]) == out["host"]
    r = subprocess.run(base + ["--sam-device", "--bam", "-o", str(tmp_path / "x.bam")], capture_output=True, text=True)
    assert r.returncode != 0 and "--sam-device" in r.stderr

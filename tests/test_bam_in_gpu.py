"""GPU: BAM input with the unpack kernel (gdiet_hip_bam_in_unpack, the attached reader's BAM route; csrc/bam_in.hip.h).  The kernel
against the 64-lane emulator on the hand-built records; the attached reader against the unattached one and the restatement
(tests/bam_in_ref.py) on the goldens and on the seam cases; its resident batch against gdiet_hip_batch_upload of the same strings; and
tools/map_file.py from a .bam file to the golden SAM.  tests/test_bam_in.py checks the same statements on the CPU."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
import bam_in_inputs as bi
import bam_in_ref as ref
import bam_ref
from fixture_io import LR, SR, golden_sam, read_fasta
from test_bam_in import emul, emul_unpack, mixed_stream, unpacked_reads  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("with_qual", [True, False])
def test_unpack_kernel_against_the_emulator(with_qual, gpu_ctx, emul, tmp_path):  # noqa: F811
    """gdiet_hip_bam_in_unpack == the 64 lanes on the host, byte for byte: text, offsets and lengths; and both are the restatement"""
    rng = np.random.default_rng(5)
    records = b"".join(bi.hand_records(rng) + bi.tag_records())
    e_text, e_off, e_lens = emul_unpack(emul, records, with_qual, tmp_path)
    text, off, lens = gpu_ctx.bam_in_unpack(records, with_qual)
    assert text == e_text and np.array_equal(off, e_off) and np.array_equal(lens, e_lens)
    assert unpacked_reads(records, text, off, lens) == ref.records_of(records, 0, with_qual)[0]
    # more than one block of four records, and a record far longer than a wavefront's stride
    big = b"".join(bi.rec(b"big%d" % i, rng.integers(0, 16, size=n).tolist(), rng.integers(0, 94, size=n).tolist(), 16 * (i & 1)) for i, n in enumerate([30001, 7, 4099, 1, 0, 64 * 9]))
    text, off, lens = gpu_ctx.bam_in_unpack(big, with_qual)
    assert unpacked_reads(big, text, off, lens) == ref.records_of(big, 0, with_qual)[0]


def test_unpack_refusals(gpu_ctx, pkg):
    good = bi.rec(b"a", [1, 2], [3, 4])
    for bad, what in ((good + good[:-1], "ends inside a record"), (good + b"\x1f\0\0\0" + bytes(31), "BAM record 1 at offset %d" % len(good))):
        with pytest.raises(pkg.GdietError, match=what):
            gpu_ctx.bam_in_unpack(bad)
    text, off, lens = gpu_ctx.bam_in_unpack(b"")
    assert text == b"" and len(off) == 0 and len(lens) == 0
    text, off, lens = gpu_ctx.bam_in_unpack(good)  # the context is still usable
    assert text == b"AC\0$%\0"


@pytest.mark.parametrize("rel", bi.GOLDENS)
def test_attached_reader_on_the_goldens(rel, gpu_ctx, pkg, tmp_path):
    """attached == unattached == restatement, on both strands; every record is the kernel's"""
    for flag in (4, 20):
        s = bi.golden_stream(rel, flag=flag)
        want = bi.expected(ref.reads_of(s)[0])
        path = bi.write_bgzf(str(tmp_path / "g.bam"), s)
        got, err, st, fmt = bi.read_all(pkg, path, chunk=100000, ctx=gpu_ctx)
        host, _, hst, _ = bi.read_all(pkg, path, chunk=100000, threads=2)
        assert err is None and fmt == "bam" and got == host and bi.rows_of(got) == want
        assert (st["records_device"], st["records_host"]) == (len(want), 0) and (hst["records_device"], hst["records_host"]) == (0, len(want))


@pytest.mark.parametrize("member,block", [(300, 256), (4096, 4096), (65280, 0)])
def test_attached_reader_on_the_seams(member, block, mixed_stream, gpu_ctx, pkg, tmp_path, monkeypatch):  # noqa: F811
    """hand-built and tag records behind a header longer than a block, members of 300 bytes in blocks of 256: batches, comments and the
    truncation flag of the unattached reader"""
    if block:
        monkeypatch.setenv("GDIET_FASTX_BLOCK", str(block))
    else:
        monkeypatch.delenv("GDIET_FASTX_BLOCK", raising=False)
    want = bi.expected(ref.reads_of(mixed_stream, with_comment=True)[0])
    path = bi.write_bgzf(str(tmp_path / "m.bam"), mixed_stream[:-3], member)  # (cut inside the last record)
    got, err, st, _ = bi.read_all(pkg, path, chunk=700, ctx=gpu_ctx, with_comment=True)
    host, _, _, _ = bi.read_all(pkg, path, chunk=700, with_comment=True)
    assert err is None and got == host and bi.rows_of(got) == want[:-1] and got[-1][1] is True
    assert st["records_device"] == len(want) - 1 and st["records_host"] == 0
    got, err, _, _ = bi.read_all(pkg, path, chunk=700, ctx=gpu_ctx, with_qual=False)
    assert err is None and bi.rows_of(got) == [(n, s, None, None) for n, s, q, c in want[:-1]]


def test_a_malformed_record_behind_device_records(gpu_ctx, pkg, tmp_path):
    good = bi.rec(b"good", [1, 2, 4, 8], [5] * 4)
    s = bi.stream([good, good, b"\x1f\0\0\0" + bytes(31), good])
    path = str(tmp_path / "bad.bam")
    with open(path, "wb") as f:
        f.write(s)
    got, err, st, _ = bi.read_all(pkg, path, ctx=gpu_ctx, chunk=1)
    assert len(bi.rows_of(got)) == 2 and st["records_device"] == 2 and "BAM record 2 at offset" in err


@pytest.fixture(scope="module")
def mappers(pkg, gpu_ctx):
    out = {}
    for kind, d, preset in (("sr", SR, "sr"), ("hifi", LR, "hifi")):
        names, seqs = read_fasta(os.path.join(d, "ref.fa.gz"))
        out[kind] = pkg.Mapper(gpu_ctx, names, seqs, preset=preset)
    yield out
    for m in out.values():
        m.close()


@pytest.mark.parametrize("block", [0, 4096])
def test_resident_batch_is_the_uploaded_batch(block, mappers, pkg, tmp_path, monkeypatch):
    """export_batch of the reader's batch == export_batch of upload_raw on the same strings: offsets, host copy and device copy; with
    blocks of 4096 bytes a batch draws on many chunks, and a chunk is shared by two batches.  Reverse-strand records, and the
    hand-built ones with their empty reads and IUPAC codes"""
    if block:
        monkeypatch.setenv("GDIET_FASTX_BLOCK", str(block))
    m = mappers["sr"]
    rng = np.random.default_rng(3)
    for name, s, chunk in (("sr", bi.golden_stream("sr/sr.fq.gz", flag=20), 45000), ("hand", bi.stream(bi.hand_records(rng) * 3), 2000)):
        path = bi.write_bgzf(str(tmp_path / (name + ".bam")), s, 4096)
        k = total = 0
        with pkg.FastxReader(path, ctx=m.ctx) as r:
            while True:
                n, names, comments, seqs, quals, lens, _, batch = r.read_raw(chunk, resident=True)
                if n == 0:
                    assert batch is None
                    break
                up = m.upload_raw(n, seqs, lens)
                try:
                    a, b = m.export_batch(batch), m.export_batch(up)
                finally:
                    m.free_batch(up)
                    m.free_batch(batch)
                for x, y, what in zip(a, b, ("roff", "host copy", "device copy")):
                    assert np.array_equal(x, y), (name, what)
                assert np.array_equal(a[1], a[2]) and int(a[0][n]) == sum(lens[i] for i in range(n))
                k, total = k + 1, total + n
            st = r.stats()
        assert k > 3 and st["records_device"] == total == len(ref.reads_of(s)[0]) and st["records_host"] == 0, (name, k, st)


def test_bam_file_to_sam(mappers, pkg, tmp_path):
    """tools/map_file.py on lr/hifi and sr/sr given as BAM, with and without --device-reader: the golden SAM of the FASTQ run, line for line"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import map_file
    try:
        for kind, rel, chunk, n_reads in (("sr", "sr/sr.fq.gz", 45000, 2000), ("hifi", "lr/hifi.fq.gz", 200000, 28)):
            bam = bi.write_bgzf(str(tmp_path / (kind + ".bam")), bi.golden_stream(rel))
            for device_reader in (True, False):
                out = str(tmp_path / ("%s%d.sam" % (kind, device_reader)))
                with open(out, "wb") as f:
                    n, _ = map_file.map_file(pkg, mappers[kind], bam, f, chunk, 3, 2, device_reader=device_reader)
                st = map_file.map_file.last_reader_stats
                assert n == n_reads and (st["records_device"], st["records_host"]) == ((n_reads, 0) if device_reader else (0, n_reads))
                assert open(out).read() == "".join(l + "\n" for l in golden_sam(kind)), (kind, device_reader)
    finally:
        mappers["sr"].set_inflight(2)  # map_file() set three on the session's context; two is what a fresh context has, and later tests count on it


@pytest.mark.parametrize("device_reader", [True, False])
def test_tags_survive_into_bam_output(device_reader, tmp_path, monkeypatch, capsys):
    """-y with MM / ML and one tag of every other kind, from a .bam through tools/map_file.py --bam and back through bam_ref.bam_to_sam"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import map_file
    tags = ["MM:Z:C+m,1,3;", "ML:B:C,200,13", "np:i:12", "rq:f:0.999", "XA:A:q", "XH:H:1AE3", "XB:B:s,-3,4"]
    with gzip.open(os.path.join(SR, "sr.fq.gz"), "rb") as f:
        lines = f.read().split(b"\n")
    fq = b"".join(lines[i] + (b" " + "\t".join(tags).encode() if (i // 4) % 3 else b"") + b"\n" + b"\n".join(lines[i + 1:i + 4]) + b"\n" for i in range(0, 4 * 300, 4))
    src, dst = bi.write_bgzf(str(tmp_path / "in.bam"), bi.make_ubam.ubam_stream(fq, tags=True), 4096), str(tmp_path / "out.bam")
    monkeypatch.setattr(sys, "argv", ["map_file.py", "--preset", "sr", "--inflight", "3", "-y", "--bam"] + (["--device-reader"] if device_reader else []) +
                        [os.path.join(SR, "ref.fa.gz"), src, "-o", dst])
    map_file.main()
    line = json.loads(capsys.readouterr().out.strip().split("\n")[-1])
    assert line["reads"] == 300 and line["reads_format"] == "bam"
    if device_reader:
        assert line["reader_stats"]["records_device"] == 300
    got = [l for l in bam_ref.bam_to_sam(gzip.decompress(open(dst, "rb").read())) if not l.startswith("@")]
    seen = {}
    for l in got:
        f = l.split("\t")
        if not int(f[1]) & 0x900:
            seen[f[0]] = f[11:]
    assert len(seen) == 300
    want_tags = bam_ref.normal("\t".join(["x"] * 11 + tags)).split("\t")[11:]
    for i in range(300):
        name = lines[4 * i][1:].decode()
        assert (seen[name][-len(tags):] == want_tags) == bool(i % 3), (name, seen[name])

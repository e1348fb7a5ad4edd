"""GPU: BGZF members inflated on the device (gdiet_hip_bgzf_inflate, csrc/bgzf_inflate.hip.h) and the reader's BGZF route
(gdiet_hip_fastx_bgzf_stats): the kernel on the whole member matrix of tests/bgzf_inputs.py, the trailer checks, and the attached and
unattached readers on the BGZF forms of the golden reads against the reader on the plain text, up to the golden SAM.
tests/test_bgzf.py checks the same statements, and corrupt streams, on the CPU emulator."""
import gzip
import os
import sys
import zlib

import numpy as np
import pytest

import bgzf_inputs as bi
from conftest import ROOT
from fixture_io import LR, SR, golden_sam, read_fasta

pytestmark = pytest.mark.gpu

READS = {"sr": (os.path.join(SR, "sr.fq.gz"), 10000, 45000, 2000), "hifi": (os.path.join(LR, "hifi.fq.gz"), bi.MAX_MEMBER_BYTES, 100000, 28)}


@pytest.fixture(scope="module")
def the_matrix():
    m = bi.matrix(np.random.default_rng(1))
    for name, member, data in m:
        assert zlib.decompress(member[18 + (member[10] - 6):-8], -15) == data and int.from_bytes(member[-4:], "little") == len(data), name
    return m


def test_inflate_the_member_matrix(the_matrix, gpu_ctx):
    """every strategy crossed with every content, and the hand-assembled streams, in one call: one wavefront per member"""
    raw = b"".join(m for _, m, _ in the_matrix) + bi.EOF_MARKER
    want = b"".join(d for _, _, d in the_matrix)
    got = gpu_ctx.bgzf_inflate(raw)
    assert len(got) == len(want) == sum(int.from_bytes(m[-4:], "little") for _, m, _ in the_matrix)
    if got != want:  # name the member
        at = 0
        for name, _, d in the_matrix:
            assert got[at:at + len(d)] == d, name
            at += len(d)
    assert gpu_ctx.bgzf_inflate(b"") == b"" and gpu_ctx.bgzf_inflate(bi.EOF_MARKER) == b""


def test_inflate_the_hand_assembled_members_alone(the_matrix, gpu_ctx):
    hand = [(n, m, d) for n, m, d in the_matrix if n.startswith("hand-")]
    assert len(hand) == 4
    for name, member, data in hand:
        assert data == bi.HAND_EXPECT[name[5:]]
        assert gpu_ctx.bgzf_inflate(member) == data, name


def test_wrong_trailers_are_refused_and_the_context_goes_on(gpu_ctx, pkg):
    text = bi.fastq_text(np.random.default_rng(3), 40)
    members = bi.members_of(text, 1000)
    for what, f in (("CRC32 mismatch", bi.corrupt_crc), ("ISIZE says", bi.corrupt_isize)):
        bad = list(members)
        bad[2] = f(bad[2])
        with pytest.raises(pkg.GdietError) as e:
            gpu_ctx.bgzf_inflate(b"".join(bad))
        assert "error -3" in str(e.value) and "member 2" in str(e.value) and what in str(e.value), str(e.value)
        assert gpu_ctx.bgzf_inflate(b"".join(members)) == text
    for raw, what in ((b"".join(members)[:-5], "ends inside a member"), (gzip.compress(text), "BGZF")):
        with pytest.raises(pkg.GdietError) as e:
            gpu_ctx.bgzf_inflate(raw)
        assert "error -3" in str(e.value) and what in str(e.value), str(e.value)
    assert gpu_ctx.bgzf_inflate(b"".join(members)) == text


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """which -> (plain path, BGZF path, plain size, BGZF size): the golden reads decompressed and re-blocked"""
    d = tmp_path_factory.mktemp("bgzf_reads")
    out = {}
    for which, (src, member_bytes, _, _) in READS.items():
        with gzip.open(src, "rb") as f:
            data = f.read()
        z = bi.bgzf(data, member_bytes)
        plain, path = str(d / (which + ".fq")), str(d / (which + ".fq.gz"))
        with open(plain, "wb") as f:
            f.write(data)
        with open(path, "wb") as f:
            f.write(z)
        out[which] = (plain, path, len(data), len(z))
    return out


def batches_of(pkg, path, chunk, ctx=None, threads=1):
    out = []
    with pkg.FastxReader(path, threads=threads, ctx=ctx) as r:
        while True:
            b = r.read(chunk, with_qual=True, with_comment=True)
            if not b and not r.truncated_now:
                break
            out.append((b, r.truncated_now))
        return out, r.stats(), r.bgzf_stats()


def set_block(monkeypatch, block):
    if block:
        monkeypatch.setenv("GDIET_FASTX_BLOCK", str(block))
    else:
        monkeypatch.delenv("GDIET_FASTX_BLOCK", raising=False)


@pytest.fixture(scope="module")
def sr_mapper(pkg, gpu_ctx):
    names, seqs = read_fasta(os.path.join(SR, "ref.fa.gz"))
    m = pkg.Mapper(gpu_ctx, names, seqs, preset="sr")
    yield m
    m.close()


@pytest.mark.parametrize("block", [4096, 0])
@pytest.mark.parametrize("which", sorted(READS))
def test_attached_reader_on_bgzf(which, block, files, sr_mapper, gpu_ctx, pkg, monkeypatch):
    """the batches of the unattached reader on the plain text, with and without resident batches; every member inflated on the device;
    the resident batch is the encoding of the host strings"""
    set_block(monkeypatch, block)
    plain, path, n_plain, n_z = files[which]
    _, _, chunk, n_reads = READS[which]
    ref, _, ref_bz = batches_of(pkg, plain, chunk)
    assert sum(len(b) for b, _ in ref) == n_reads and not any(ref_bz[k] for k in ("members_device", "members_host", "bytes_in", "bytes_out"))
    got, st, bz = batches_of(pkg, path, chunk, gpu_ctx)
    assert got == ref
    assert bz["members_device"] > 0 and bz["members_host"] == 0 and (bz["bytes_in"], bz["bytes_out"]) == (n_z, n_plain), bz
    assert st["records_device"] + st["records_host"] == n_reads and st["records_device"] > 0, st
    m, k, rows = sr_mapper, 0, []
    with pkg.FastxReader(path, ctx=gpu_ctx) as r:
        while True:
            n, names, comments, seqs, quals, lens, _, batch = r.read_raw(chunk, with_comment=True, resident=True)
            if n == 0:
                assert batch is None
                break
            try:
                up = m.upload_raw(n, seqs, lens)
                try:
                    a, b = m.export_batch(batch), m.export_batch(up)
                finally:
                    m.free_batch(up)
                for x, y, what in zip(a, b, ("roff", "host copy", "device copy")):
                    assert np.array_equal(x, y), (k, what)
                assert np.array_equal(a[1], a[2])
                rows.append([(names[i], seqs[i], quals[i], comments[i]) for i in range(n)])
            finally:
                m.free_batch(batch)
            k += 1
        bz = r.bgzf_stats()
    assert rows == [b for b, _ in ref]
    assert bz["members_device"] > 0 and bz["members_host"] == 0 and bz["bytes_out"] == n_plain, bz


@pytest.mark.parametrize("which", sorted(READS))
def test_unattached_reader_with_four_threads_on_bgzf(which, files, pkg, monkeypatch):
    plain, path, n_plain, n_z = files[which]
    _, _, chunk, n_reads = READS[which]
    for block in (4096, 0):
        set_block(monkeypatch, block)
        ref, _, _ = batches_of(pkg, plain, chunk)
        got, st, bz = batches_of(pkg, path, chunk, None, threads=4)
        assert got == ref and sum(len(b) for b, _ in got) == n_reads
        assert bz["members_host"] > 0 and bz["members_device"] == 0 and (bz["bytes_in"], bz["bytes_out"]) == (n_z, n_plain), bz
        assert st["records_device"] == 0
    monkeypatch.setenv("GDIET_BGZF", "0")  # the switch: zlib's gzread, the same batches
    got, _, bz = batches_of(pkg, path, chunk, None, threads=4)
    assert got == ref and not any(bz[k] for k in ("members_device", "members_host", "bytes_in", "bytes_out")), bz


def test_a_corrupt_member_fails_the_read_with_a_message(files, gpu_ctx, pkg, tmp_path):
    """a wrong CRC in the middle of the file, attached and unattached: GdietError naming the member; the context goes on"""
    with open(files["sr"][0], "rb") as f:
        data = f.read()[:60000]
    members = bi.members_of(data, 5000)
    members[7] = bi.corrupt_crc(members[7])
    path = str(tmp_path / "bad.fq.gz")
    with open(path, "wb") as f:
        f.write(b"".join(members) + bi.EOF_MARKER)
    for ctx in (gpu_ctx, None):
        with pkg.FastxReader(path, threads=4, ctx=ctx) as r:
            with pytest.raises(pkg.GdietError) as e:
                while r.read(45000):
                    pass
            assert "member 7" in str(e.value) and "CRC32" in str(e.value), str(e.value)
    assert gpu_ctx.bgzf_inflate(b"".join(members[:7])) == data[:35000]


def test_bgzf_file_to_sam(files, sr_mapper, pkg, tmp_path):
    """tools/map_file.py on the BGZF reads, with the device reader and without: the golden SAM bodies"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import map_file
    try:
        for device_reader in (True, False):
            out = str(tmp_path / ("sr%d.sam" % device_reader))
            with open(out, "wb") as f:
                n, _ = map_file.map_file(pkg, sr_mapper, files["sr"][1], f, 45000, 3, 4, device_reader=device_reader)
            bz = map_file.map_file.last_bgzf_stats
            assert n == 2000 and bz["bytes_out"] == files["sr"][2] and (bz["members_device"] > 0) == device_reader and (bz["members_host"] > 0) != device_reader, bz
            assert open(out).read() == "".join(l + "\n" for l in golden_sam("sr"))
        names, seqs = read_fasta(os.path.join(LR, "ref.fa.gz"))
        m = pkg.Mapper(sr_mapper.ctx, names, seqs, preset="hifi")
        try:
            out = str(tmp_path / "hifi.sam")
            with open(out, "wb") as f:
                n, _ = map_file.map_file(pkg, m, files["hifi"][1], f, 200000, 3, 1, device_reader=True)
            assert n == 28 and map_file.map_file.last_bgzf_stats["members_device"] > 0
            assert open(out).read() == "".join(l + "\n" for l in golden_sam("hifi"))
        finally:
            m.close()
    finally:
        sr_mapper.set_inflight(2)  # (what a fresh context has, and later tests count on it: map_file() set three)

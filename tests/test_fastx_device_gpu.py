"""GPU: the device mode of the reader (gdiet_hip_fastx_attach / _read_resident / _stats, gdiet_hip_batch_export; csrc/fastx_dev.hip.h).
An attached reader must return, byte for byte and batch for batch, what the unattached reader returns, and its resident batch must be
what gdiet_hip_batch_upload builds of the same strings -- on strict four-line FASTQ (all of it the device's), on inputs the device must
hand over to the host grammar, and on files that mix both.  tests/test_fastx_device.py checks the same statements on the CPU emulator."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from fastx_device_inputs import mixed_file, sweep_file
from fastx_inputs import awkward_inputs
from fixture_io import LR, SR, golden_sam, read_fasta
import samopts_io as so

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden", "fastx")


def batches_of(pkg, path, chunk, ctx=None, with_comment=True, frag_mode=False):
    """([(rows, closed early)], truncated, stats) of a whole file"""
    out = []
    with pkg.FastxReader(path, ctx=ctx) as r:
        while True:
            b = r.read(chunk, with_qual=True, with_comment=with_comment, frag_mode=frag_mode)
            if not b and not r.truncated_now:
                break
            out.append((b, r.truncated_now))
        return out, r.truncated, r.stats()


def set_block(monkeypatch, block):
    if block:
        monkeypatch.setenv("GDIET_FASTX_BLOCK", str(block))
    else:
        monkeypatch.delenv("GDIET_FASTX_BLOCK", raising=False)


def write(tmp_path, name, data, gz=False):
    path = str(tmp_path / (name + (".gz" if gz else "")))
    with (gzip.open(path, "wb") if gz else open(path, "wb")) as f:
        f.write(data)
    return path


@pytest.mark.parametrize("block", [256, 4096, 0])
@pytest.mark.parametrize("with_comment", [False, True])
def test_awkward_inputs_against_the_goldens(with_comment, block, gpu_ctx, pkg, tmp_path, monkeypatch):
    """every awkward input, plain and gzip: the rows of the committed goldens (the reference's own view), the batch sizes and truncation
    flags of the unattached reader, and the device's share where it is known"""
    set_block(monkeypatch, block)
    for name, data in awkward_inputs(np.random.default_rng(31)).items():
        with open(os.path.join(GOLD, "%s.%s.expected.json" % (name, "y" if with_comment else "n"))) as f:
            want = [tuple(x.encode("latin1") if x is not None else None for x in row) for row in json.load(f)]
        for gz in (False, True):
            path = write(tmp_path, name, data, gz)
            got, trunc, st = batches_of(pkg, path, 1500, gpu_ctx, with_comment)
            ref, ref_trunc, ref_st = batches_of(pkg, path, 1500, None, with_comment)
            rows = [(n, s, q, (c if with_comment else None)) for b, _ in got for n, s, q, c in b]
            assert rows == want, (name, gz)
            assert got == ref and trunc == ref_trunc == (name in ("truncated.fq", "broken_mid.fq")), (name, gz)
            assert ref_st["records_device"] == 0 and st["records_device"] + st["records_host"] == len(want), (name, gz, st)
            if name == "plain.fq":
                assert (st["records_device"], st["records_host"]) == (40, 0), (gz, st)
            if name in ("multiline.fq", "crlf.fq", "multi.fa"):
                assert st["records_device"] == 0, (name, gz, st)


@pytest.mark.parametrize("block", [256, 1000, 4096])
def test_geometry_sweep(block, gpu_ctx, pkg, tmp_path, monkeypatch):
    """reads of every length 1..70 and 1000..1100 with newlines on every residue of a lane and on both sides of a tile edge: all the device's"""
    set_block(monkeypatch, block)
    data, n = sweep_file()
    path = write(tmp_path, "sweep.fq", data)
    got, _, st = batches_of(pkg, path, 20000, gpu_ctx)
    ref, _, _ = batches_of(pkg, path, 20000, None)
    assert got == ref and sum(len(b) for b, _ in got) == n
    assert (st["records_device"], st["records_host"]) == (n, 0), st


def resident_batches(pkg, m, path, chunk, check):
    """read a file batch by batch with resident=True and hand every batch to check(n, names, comments, seqs, quals, lens, batch)"""
    k = 0
    with pkg.FastxReader(path, ctx=m.ctx) as r:
        while True:
            n, names, comments, seqs, quals, lens, _, batch = r.read_raw(chunk, with_comment=True, resident=True)
            if n == 0 and not r.truncated_now:
                assert batch is None
                break
            if n:
                try:
                    check(n, names, comments, seqs, quals, lens, batch)
                finally:
                    m.free_batch(batch)
                k += 1
        return k, r.stats()


@pytest.fixture(scope="module")
def sr_mapper(pkg, gpu_ctx):
    names, seqs = read_fasta(os.path.join(SR, "ref.fa.gz"))
    m = pkg.Mapper(gpu_ctx, names, seqs, preset="sr")
    yield m
    m.close()


@pytest.mark.parametrize("block", [0, 4096])
@pytest.mark.parametrize("which", ["sweep", "sr"])
def test_resident_batch_is_the_uploaded_batch(which, block, sr_mapper, pkg, tmp_path, monkeypatch):
    """export_batch of the reader's batch == export_batch of upload_raw on the same strings: offsets, host copy and device copy.  With
    blocks of 4096 bytes a batch draws on many chunks, and a chunk is shared by two batches"""
    set_block(monkeypatch, block)
    m = sr_mapper
    if which == "sweep":
        path, chunk = write(tmp_path, "sweep.fq", sweep_file()[0]), 20000
    else:
        path, chunk = os.path.join(SR, "sr.fq.gz"), 45000

    def check(n, names, comments, seqs, quals, lens, batch):
        up = m.upload_raw(n, seqs, lens)
        try:
            a, b = m.export_batch(batch), m.export_batch(up)
        finally:
            m.free_batch(up)
        assert batch[1] == n and int(a[0][n]) == sum(lens[i] for i in range(n))
        for x, y, what in zip(a, b, ("roff", "host copy", "device copy")):
            assert np.array_equal(x, y), what
        assert np.array_equal(a[1], a[2])

    k, st = resident_batches(pkg, m, path, chunk, check)
    assert k > 3 and st["records_host"] == 0 and st["records_device"] == (sweep_file()[1] if which == "sweep" else 2000), st


def test_record_longer_than_the_block(gpu_ctx, pkg, monkeypatch):
    """28 HiFi records of ~29 kbp in blocks of 4096 bytes: the reader reads on in bigger steps until a record is complete"""
    set_block(monkeypatch, 4096)
    path = os.path.join(LR, "hifi.fq.gz")
    got, _, st = batches_of(pkg, path, 100000, gpu_ctx)
    ref, _, _ = batches_of(pkg, path, 100000, None)
    assert got == ref and sum(len(b) for b, _ in got) == 28
    assert (st["records_device"], st["records_host"]) == (28, 0), st


def test_fragment_mode_keeps_mates_together(gpu_ctx, pkg, tmp_path):
    path = str(tmp_path / "pairs.fq")
    with open(path, "wb") as f:
        for i in range(50):
            for mate in (1, 2):
                f.write(b"@p%d/%d\n" % (i, mate) + b"ACGT" * 25 + b"\n+\n" + b"I" * 100 + b"\n")
    got, _, st = batches_of(pkg, path, 250, gpu_ctx, frag_mode=True)  # 250 bases: closes after the third read, i.e. in the middle of a pair
    for b, _ in got:
        assert b[-1][0].endswith(b"/2"), [x[0] for x in b]
    assert [x[0] for b, _ in got for x in b] == [b"p%d/%d" % (i, mate) for i in range(50) for mate in (1, 2)]
    assert st["records_device"] == 100, st


@pytest.fixture(scope="module")
def mixed_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("mixed") / "mixed.fq")
    with open(path, "wb") as f:
        f.write(mixed_file())
    return path


@pytest.mark.parametrize("block", [4096, 65536])
def test_mixed_file_batches(block, mixed_path, gpu_ctx, pkg, monkeypatch):
    """strict zones, multi-line, CRLF and FASTA zones and one malformed record: the batches of the unattached reader, the one early close
    included, with both parsers at work"""
    set_block(monkeypatch, block)
    for chunk in (3000, 10 ** 7):
        got, _, st = batches_of(pkg, mixed_path, chunk, gpu_ctx)
        ref, _, _ = batches_of(pkg, mixed_path, chunk, None)
        assert got == ref
        assert sum(len(b) for b, _ in got) == 6000 and sum(1 for _, t in got if t) == 1
        print("block %d chunk %d: %r" % (block, chunk, st))
        assert st["records_device"] > 0 and st["records_host"] > 0 and st["blocks_handed_over"] > 0, st


def regs_of(res):
    out = []
    for i in range(res.n):
        regs = []
        for j in range(res.n_regs[i]):
            g = res.regs[i][j]
            regs.append((g.rid, g.qs, g.qe, g.rs, g.re, g.rev, g.score, g.mapq, g.parent, g.id, tuple(g.cigar[k] for k in range(g.n_cigar))))
        out.append(regs)
    return out


def test_a_batch_of_both_kinds_maps_like_its_strings(mixed_path, gpu_ctx, pkg, monkeypatch):
    """one resident batch with device-parsed and host-parsed reads (the whole mixed file up to the malformed record: stats() shows both
    parsers contributed to it), mapped against a contig made of the reads themselves: the records of Mapper.map on the same strings"""
    set_block(monkeypatch, 65536)
    rows, _, _ = batches_of(pkg, mixed_path, 10 ** 7, None)
    contig = b"".join(s for b, _ in rows for _, s, _, _ in b)
    m = pkg.Mapper(gpu_ctx, ["mix"], [contig], preset="sr")
    try:
        with pkg.FastxReader(mixed_path, ctx=gpu_ctx) as r:
            n, names, comments, seqs, quals, lens, _, batch = r.read_raw(10 ** 7, with_comment=True, resident=True)
            st = r.stats()
            try:
                assert r.truncated_now and n == len(rows[0][0])  # the batch the malformed record closes: 2751 reads from five zones
                assert 0 < st["records_device"] < n, st  # (the device's records all precede the end of this batch, and are not all of it)
                strings = [seqs[i] for i in range(n)]
                assert strings == [s for _, s, _, _ in rows[0][0]]
                got = regs_of(m.map_uploaded(batch))
            finally:
                m.free_batch(batch)
        want = regs_of(m.map(strings))
        assert got == want
        assert sum(1 for g in got if g) > n // 2  # (the reads do map: the contig is made of them)
    finally:
        m.close()


def test_file_to_sam_with_the_device_reader(sr_mapper, pkg, tmp_path):
    """tools/map_file.py --device-reader: three mini-batches in flight, no upload stage -- the golden SAM bodies"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import map_file
    try:
        for chunk in (30000, 45000):
            out = str(tmp_path / ("sr%d.sam" % chunk))
            with open(out, "wb") as f:
                n, _ = map_file.map_file(pkg, sr_mapper, os.path.join(SR, "sr.fq.gz"), f, chunk, 3, 1, device_reader=True)
            assert n == 2000 and map_file.map_file.last_stage_seconds["upload"] == 0.0
            assert map_file.map_file.last_reader_stats["records_device"] == 2000 and map_file.map_file.last_reader_stats["records_host"] == 0
            assert open(out).read() == "".join(l + "\n" for l in golden_sam("sr"))
        names, seqs = read_fasta(os.path.join(LR, "ref.fa.gz"))
        m = pkg.Mapper(sr_mapper.ctx, names, seqs, preset="hifi")
        try:
            out = str(tmp_path / "hifi.sam")
            with open(out, "wb") as f:
                n, _ = map_file.map_file(pkg, m, os.path.join(LR, "hifi.fq.gz"), f, 200000, 3, 1, device_reader=True)
            assert n == 28
            assert open(out).read() == "".join(l + "\n" for l in golden_sam("hifi"))
        finally:
            m.close()
    finally:
        sr_mapper.set_inflight(2)  # map_file() set three on the session's context; two is what a fresh context has, and later tests count on it


def test_file_to_sam_with_options_and_the_device_reader(tmp_path, monkeypatch, capsys):
    """the tool as a whole on sr with --device-reader --MD --header -R ... -Y -y --sam-hit-only: with the MD:Z: field taken out, the
    reference's output of mode `all` (tests/golden/samopts/sr.all.sam.gz; @PG names this tool); with it, the run without --device-reader"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import map_file
    fq = str(tmp_path / "reads.fq")
    with open(fq, "w") as f:
        for name, seq, qual, cm in so.reads_with_comments("sr"):
            f.write("@%s%s\n%s\n+\n%s\n" % (name, "" if cm is None else " " + cm, seq, qual))
    outs = {}
    for flag in (["--device-reader"], []):
        out = str(tmp_path / ("out%d.sam" % len(flag)))
        monkeypatch.setattr(sys, "argv", ["map_file.py", "--preset", "sr", "--inflight", "3", "--MD", "--header", "-R", so.RG_ARG, "-Y", "-y", "--sam-hit-only"] + flag +
                            [os.path.join(SR, "ref.fa.gz"), fq, "-o", out])
        map_file.main()
        line = json.loads(capsys.readouterr().out.strip().split("\n")[-1])
        assert ("reader_stats" in line) == bool(flag)
        if flag:
            assert line["reader_stats"]["records_device"] == 2000 and line["reader_stats"]["records_host"] == 0
        outs[len(flag)] = open(out).read().split("\n")
    not_pg = lambda lines: [l for l in lines if not l.startswith("@PG")]
    assert not_pg(outs[1]) == not_pg(outs[0])
    hdr, body = so.golden("sr", "all")
    lines = outs[1][:-1]
    assert outs[1][-1] == "" and len(lines) == len(hdr) + len(body)
    assert lines[:len(hdr) - 1] == hdr[:-1] and lines[len(hdr) - 1].startswith("@PG\tID:minimap2\tPN:minimap2\tVN:")
    strip_md = lambda l: "\t".join(f for f in l.split("\t") if not f.startswith("MD:Z:"))
    assert [so.digest_line(strip_md(l)) for l in lines[len(hdr):]] == body
    assert sum(1 for l in lines[len(hdr):] if "\tMD:Z:" in l) > 1000

"""GPU: BGZF members written on the device (gdiet_hip_bgzf_deflate, csrc/bgzf_deflate.hip.h), the stream writer (BgzfWriter) on both of
its routes and tools/map_file.py --bgzf.  The kernel's members must be the bytes of the CPU emulator (tests/emul/bgzf_deflate_emul.cpp,
built here without a sanitizer), which tests/test_bgzf_deflate.py checks against zlib, the scan and the project's own decoder: so what
holds there holds for the kernel."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys

import pytest

import bgzf_deflate_inputs as di
import bgzf_inputs as bi
from bgzf_deflate_inputs import same_members
from conftest import ROOT
from fixture_io import SR, golden_sam, read_fasta

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_deflate_gpu")
    exe = str(d / "emul")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-w", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul", "bgzf_deflate_emul.cpp"), "-o", exe, "-lz"])

    def run(data):
        src, dst = str(d / "in"), str(d / "out.gz")
        with open(src, "wb") as f:
            f.write(data)
        subprocess.run([exe, "deflate", src, dst], check=True, capture_output=True, timeout=120)
        return open(dst, "rb").read()
    return run


def test_every_input_in_one_call(gpu_ctx, emul):
    """all inputs one behind the other, cut every 65280 bytes: one wavefront per member, about forty of them"""
    data = b"".join(d for _, d in di.inputs())
    z = gpu_ctx.bgzf_deflate(data)
    assert len(di.member_sizes(z)) == -(-len(data) // bi.MAX_MEMBER_BYTES) + 1 and z.endswith(bi.EOF_MARKER)
    assert gzip.decompress(z) == data
    assert gpu_ctx.bgzf_inflate(z) == data  # kernel to kernel
    same_members(z, emul(data), "all inputs")
    assert gpu_ctx.bgzf_deflate(data) == z  # a member's bytes depend on its input alone
    assert gpu_ctx.bgzf_deflate(data, eof=False) == z[:-28]


def test_every_input_alone(gpu_ctx, emul):
    for name, data in di.inputs():
        z = gpu_ctx.bgzf_deflate(data)
        assert gzip.decompress(z) == data and gpu_ctx.bgzf_inflate(z) == data, name
        same_members(z, emul(data), name)
    assert gpu_ctx.bgzf_deflate(b"") == bi.EOF_MARKER and gpu_ctx.bgzf_deflate(b"", eof=False) == b""


def test_bad_arguments_are_refused_on_the_host(gpu_ctx, pkg):
    lib, n = gpu_ctx.lib, C.c_size_t()
    out = C.create_string_buffer(2 * 65536 + 28)
    assert lib.gdiet_hip_bgzf_deflate(gpu_ctx._h, None, 10, C.cast(out, C.c_void_p), len(out), C.byref(n), 1) == -3
    assert "no input" in lib.gdiet_hip_strerror(gpu_ctx._h).decode()
    data = b"A" * 70000  # two members: the bound is 2 * 65536 + 28
    assert lib.gdiet_hip_bgzf_deflate(gpu_ctx._h, data, len(data), None, 0, C.byref(n), 1) == 0 and n.value == 2 * 65536 + 28
    assert lib.gdiet_hip_bgzf_deflate(gpu_ctx._h, data, len(data), C.cast(out, C.c_void_p), 2 * 65536 + 27, C.byref(n), 1) == -3
    assert "bound" in lib.gdiet_hip_strerror(gpu_ctx._h).decode() and n.value == 0
    assert lib.gdiet_hip_bgzf_deflate(gpu_ctx._h, data, len(data), C.cast(out, C.c_void_p), len(out), None, 1) == -3  # (no place for the length)
    assert gzip.decompress(gpu_ctx.bgzf_deflate(data)) == data  # the context goes on


def test_nothing_written_is_the_marker_alone(gpu_ctx, pkg, tmp_path):
    for ctx in (gpu_ctx, None):
        path = str(tmp_path / "empty.gz")
        w = pkg.BgzfWriter(path, ctx=ctx)
        assert w.write(b"") == 0
        w.close()
        assert open(path, "rb").read() == bi.EOF_MARKER
        assert w.stats() == {"members_device": 0, "members_host": 0, "bytes_in": 0, "bytes_out": 28}
        with pytest.raises(ValueError):
            w.write(b"x")


@pytest.fixture(scope="module")
def sr_mapper(pkg, gpu_ctx):
    names, seqs = read_fasta(os.path.join(SR, "ref.fa.gz"))
    m = pkg.Mapper(gpu_ctx, names, seqs, preset="sr")
    yield m
    m.close()


def test_writer_as_the_sink_of_the_golden_reads(gpu_ctx, sr_mapper, pkg, tmp_path):
    """Mapper.sam_batch_raw(..., sink=writer) through tools/map_file.py's three stages: the golden SAM back out of the file, members full
    but the last, and the statistics say who compressed"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import map_file
    want = "".join(l + "\n" for l in golden_sam("sr")).encode()
    try:
        for route, ctx in (("device", gpu_ctx), ("host", None)):
            path = str(tmp_path / (route + ".sam.gz"))
            with pkg.BgzfWriter(path, ctx=ctx, level=1, threads=2) as w:
                n, _ = map_file.map_file(pkg, sr_mapper, os.path.join(SR, "sr.fq.gz"), w, 45000, 3, 2)
            z = open(path, "rb").read()
            assert n == 2000 and gzip.decompress(z) == want and z.endswith(bi.EOF_MARKER)
            sizes = di.member_sizes(z)
            assert all(i == bi.MAX_MEMBER_BYTES for _, i in sizes[:-2]) and sizes[-1] == (28, 0)
            st = w.stats()
            assert st["bytes_in"] == len(want) and st["bytes_out"] == len(z), st
            assert (st["members_device"], st["members_host"]) == ((len(sizes) - 1, 0) if ctx else (0, len(sizes) - 1)), st
            if ctx:
                assert gpu_ctx.bgzf_inflate(z) == want
    finally:
        sr_mapper.set_inflight(2)  # (what a fresh context has, and later tests count on it: map_file() set three)


def test_tool_with_bgzf_writes_the_same_sam(capsys, monkeypatch, tmp_path):
    """tools/map_file.py --preset sr --header with --bgzf device, --bgzf host and without: the same bytes once decompressed -- but for the
    CL: field of the @PG line, which records each run's own command line"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import map_file
    texts, stats = {}, {}
    for route in (None, "device", "host"):
        out = str(tmp_path / ("x.%s.sam" % route))
        argv = ["map_file.py", os.path.join(SR, "ref.fa.gz"), os.path.join(SR, "sr.fq.gz"), "--preset", "sr", "--header", "-K", "45000", "-o", out] + (["--bgzf", route] if route else [])
        monkeypatch.setattr(sys, "argv", argv)
        map_file.main()
        info = json.loads(capsys.readouterr().out.strip().split("\n")[-1])
        raw = open(out, "rb").read()
        assert ("bgzf_out" in info) == bool(route)
        if route:
            assert raw[:4] == b"\x1f\x8b\x08\x04" and raw.endswith(bi.EOF_MARKER)
            stats[route] = info["bgzf_out"]
            raw = gzip.decompress(raw)
        texts[route] = raw.split(b"\n")
    pg = [k for k, l in enumerate(texts[None]) if l.startswith(b"@PG")]
    assert len(pg) == 1 and texts[None][0].startswith(b"@SQ")
    for route in ("device", "host"):
        a, b = list(texts[None]), list(texts[route])
        assert a[pg[0]].split(b"\tCL:")[0] == b[pg[0]].split(b"\tCL:")[0] and b"--bgzf " + route.encode() in b[pg[0]]
        del a[pg[0]], b[pg[0]]
        assert a == b, route
    assert stats["device"]["members_device"] > 0 and stats["device"]["members_host"] == 0, stats
    assert stats["host"]["members_host"] > 0 and stats["host"]["members_device"] == 0, stats

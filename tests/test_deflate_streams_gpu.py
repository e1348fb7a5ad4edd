"""GPU: bgzf_inflate_kernel (csrc/bgzf_inflate.hip.h) on the DEFLATE streams of tests/deflate_streams.py -- every length and distance
symbol, codes of 15 bits, run codes across the literal/distance boundary, 300 blocks in a member, the edges of the input ring, a full
window at every alignment, 300 seeded random streams -- against zlib's bytes, and on the streams that must be refused; then
bgzf_deflate_kernel on the input that makes the code builder's limiter act, against the writer's emulator.
tests/test_deflate_streams.py holds the same streams to zlib, to their coverage conditions and to the sanitized emulator on the CPU:
what is left to find here is what differs on the device."""
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_deflate_inputs as di
import bgzf_inputs as bi
import deflate_streams as ds
from bgzf_deflate_inputs import same_members
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fam", list(ds.FAMILIES))
def test_inflate_a_family_in_one_call(fam, gpu_ctx):
    """all members of the family in one file, one wavefront each; the `full` family is its sixteen placements"""
    streams = ds.family(fam)
    for name, stream, want in streams:
        assert zlib.decompress(stream, -15) == want, name
    raw = b"".join(ds.member(s, want) for _, s, want in streams) + bi.EOF_MARKER
    want = b"".join(w for _, _, w in streams)
    got = gpu_ctx.bgzf_inflate(raw)
    assert len(got) == len(want)
    if got != want:  # name the member
        at = 0
        for name, _, w in streams:
            assert got[at:at + len(w)] == w, name
            at += len(w)
    assert got == want


def test_invalid_streams_are_refused_and_the_context_goes_on(gpu_ctx, pkg):
    """every entry of invalid(), each in a call of its own behind a valid member: GdietError with the member's number and the class's
    text (tests/test_deflate_streams.py has passed the same bytes through zlib and the sanitized emulator), and the next call works"""
    text = bi.fastq_text(np.random.default_rng(3), 8)
    good = bi.member(text)
    for name, stream, isize, err in ds.invalid():
        assert ds.zlib_refuses(stream, isize), name
        with pytest.raises(pkg.GdietError) as e:
            gpu_ctx.bgzf_inflate(good + ds.member_with_trailer(stream, isize) + bi.EOF_MARKER)
        assert "error -3" in str(e.value) and "member 1:" in str(e.value) and err in str(e.value), (name, str(e.value))
        assert gpu_ctx.bgzf_inflate(good) == text, name


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """the writer's emulator, without a sanitizer (as in tests/test_bgzf_deflate_gpu.py)"""
    d = tmp_path_factory.mktemp("deflate_streams_gpu")
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


def test_deflate_where_the_limiter_acts(gpu_ctx, emul):
    """the inputs for which gdd_build_lengths cuts a code to its limit inside a block: the kernel's members are the emulator's, gzip reads
    them, and so does the inflate kernel"""
    for name, data in di.limiter_inputs():
        z = gpu_ctx.bgzf_deflate(data)
        assert gzip.decompress(z) == data, name
        assert gpu_ctx.bgzf_inflate(z) == data, name  # kernel to kernel
        same_members(z, emul(data), name)

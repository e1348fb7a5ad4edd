"""CPU: the BGZF writing side (csrc/bgzf_deflate.h, csrc/bgzf_out.h) on the host emulator tests/emul/bgzf_deflate_emul.cpp, a stand-alone
program built under AddressSanitizer / UBSan, twice: with the lane loops running 0..63 and 63..0.  The emulator runs the statements of
bgzf_deflate_kernel as loops over 64 lanes on exact-size copies of every input and slot and checks every member itself (zlib's raw
inflate, CRC32, ISIZE, BSIZE, gd_bgzf_scan, the project's own decoder); it ends with status 1 on any difference.  Here: both builds
write the same bytes, Python's gzip reads them, gdd_build_lengths meets its conditions, the stream writer without a device cuts
members as documented and the project's reader reads its file, and the match search and the dynamic codes each earn something."""
import gzip
import os
import re
import subprocess
import zlib
from fractions import Fraction

import numpy as np
import pytest

import bgzf_deflate_inputs as di
import bgzf_inputs as bi
from conftest import ROOT

TIMEOUT = 120  # seconds; a run takes well below one (W4 of csrc/bgzf_deflate.h: every loop ends)
CSRC = os.path.join(ROOT, "genome-on-diet_amd", "csrc")
SAN = ["-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build(exe, source, *flags):
    subprocess.check_call(["g++"] + SAN + list(flags) + ["-I", CSRC, os.path.join(ROOT, "tests", "emul", source), "-o", exe, "-lz"])
    return exe


@pytest.fixture(scope="module")
def emuls(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_deflate")
    return build(str(d / "up"), "bgzf_deflate_emul.cpp"), build(str(d / "down"), "bgzf_deflate_emul.cpp", "-DGDD_LANES_DOWN")


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=TIMEOUT)
    assert r.returncode == 0, (args, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout


def put(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def deflate(emuls, tmp_path, name, data):
    """the members of `data` from both builds (equal, or the test fails), and the first build's report"""
    src = put(tmp_path, name + ".in", data)
    outs = []
    for k, exe in enumerate(emuls):
        dst = str(tmp_path / ("%s.%d.gz" % (name, k)))
        outs.append((run(exe, "deflate", src, dst), open(dst, "rb").read()))
    assert outs[0] == outs[1], "%s: the members depend on the order of the lanes" % name
    return outs[0][1], outs[0][0]


@pytest.fixture(scope="module")
def deflated(emuls, tmp_path_factory):
    """name -> (input, file bytes, report), every input once"""
    d = tmp_path_factory.mktemp("members")
    return {name: (data,) + deflate(emuls, d, name, data) for name, data in di.inputs()}


@pytest.mark.parametrize("name", [n for n, _ in di.inputs()])
def test_members_are_valid_whatever_the_lane_order(name, deflated):
    data, z, report = deflated[name]
    n_members = -(-len(data) // bi.MAX_MEMBER_BYTES)
    assert report.endswith("ok members %d bytes_in %d bytes_out %d\n" % (n_members, len(data), len(z) - 28)), report
    assert z.endswith(bi.EOF_MARKER) and gzip.decompress(z) == data
    sizes = di.member_sizes(z)
    assert [i for _, i in sizes] == [min(bi.MAX_MEMBER_BYTES, len(data) - at) for at in range(0, len(data), bi.MAX_MEMBER_BYTES)] + [0]
    assert all(n <= 65536 and n <= 18 + 5 + i + 8 for n, i in sizes)


def test_edges(deflated):
    rep = {name: deflated[name][2] for name in deflated}
    line = lambda name: re.search(r"member 0 in (\d+) out (\d+) type (\d) maxdist (\d+)", rep[name]).groups()
    assert "empty member out 28 type 1" in rep["len0"]  # a member of no bytes: the end-of-block code of a fixed block
    # a stored member is exactly 18 + 5 + n + 8 bytes; random bytes take it, and a run does not
    assert line("random")[:3] == ("65280", "65311", "0")
    # (a run's matches reach back to the group of 64 positions before theirs: distances 1..64)
    assert int(line("run65280")[1]) < 400 and 1 <= int(line("run65280")[3]) <= 64
    # the longest distance: 32768 is found and used, 32769 is not (nor anything further than 32768, which no distance code could say);
    # a match of three bytes that far back costs more than its literals and is declined, as zlib does
    assert line("dist32768")[3] == "32768" and 1 <= int(line("dist32769")[3]) <= 64
    assert 1 <= int(line("dist32768_3")[3]) <= 64 and 1 <= int(line("dist32769_3")[3]) <= 64
    for n in (257, 258, 259, 260):
        assert 1 <= int(line("run%d" % n)[3]) <= 64
    assert line("one_distance")[3] == "2"
    assert line("one_value_1")[3] == "0" and line("one_value_2")[3] == "0"


def lengths(exe, max_bits, freq):
    out = run(exe, "lengths", max_bits, *freq).split()
    return [int(x) for x in out]


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def length_cases():
    rng = np.random.default_rng(5)
    cases = [("fib%d/%d" % (n, lim), lim, fib(n)) for n in (20, 25, 30) for lim in (15, 7)]
    cases += [("equal%d/%d" % (n, lim), lim, [7] * n) for n in (2, 3, 19, 30, 286) for lim in (15, 7) if n <= 1 << lim]
    cases += [("one", 15, [0, 0, 0, 9, 0, 0]), ("one/7", 7, [0] * 18 + [4]), ("two", 15, [0, 5, 0, 0, 1000000, 0]), ("none", 15, [0] * 30)]
    cases += [("random286", 15, rng.integers(0, 100000, size=286).tolist()), ("random286sparse", 15, (rng.integers(0, 3, size=286) * rng.integers(0, 1000, size=286)).tolist()),
              ("random19/7", 7, rng.integers(0, 300, size=19).tolist())]
    return cases


@pytest.mark.parametrize("case", length_cases(), ids=lambda c: c[0])
def test_build_lengths(case, emuls):
    name, lim, freq = case
    lens = lengths(emuls[0], lim, freq)
    assert lens == lengths(emuls[1], lim, freq), "the lengths depend on the order of the lanes"
    assert len(lens) == len(freq) and all(l <= lim for l in lens)
    assert all((l != 0) == (f != 0) for l, f in zip(lens, freq))
    used = [l for l in lens if l]
    if len(used) >= 2:
        assert sum(Fraction(1, 1 << l) for l in used) == 1
    elif used:
        assert used == [1]
    flat = max(1, (len(freq) - 1).bit_length())  # ceil(log2 n)
    assert sum(f * l for f, l in zip(freq, lens)) <= flat * sum(freq)
    if name.startswith("fib"):  # the limiter had to act: the plain Huffman code of Fibonacci frequencies is n - 1 deep
        assert len(freq) - 1 > lim and max(lens) == lim


WRITES = [1, 100, 65279, "f", 65281, 200000]


def test_stream_writer_without_a_device(emuls, tmp_path):
    """writes of 1, 100, 65279, 65281 and 200000 bytes with one flush in the middle: members of 65280 bytes except at the flush and at
    the close, the end-of-file member, the bytes back through gzip, and the project's own reader on the file (the BGZF route)"""
    total = sum(w for w in WRITES if w != "f")
    text = bi.fastq_text(np.random.default_rng(17), 1800)[:total]
    assert len(text) == total
    src = put(tmp_path, "w.fq", text)
    files = []
    for level, threads in ((1, 4), (-1, 1)):
        dst = str(tmp_path / ("w%d.fq.gz" % threads))
        out = run(emuls[0], "writer", src, dst, level, threads, *WRITES)
        z = open(dst, "rb").read()
        assert out == "ok members_device 0 members_host 7 bytes_in %d bytes_out %d\n" % (total, len(z)), out
        assert z.endswith(bi.EOF_MARKER) and gzip.decompress(z) == text
        assert [i for _, i in di.member_sizes(z)] == [65280, 100, 65280, 65280, 65280, 65280, total - 4 * 65280 - 65380, 0]
        files.append(dst)
    # the reader: the file takes the BGZF route and gives the records of the plain text
    reader = build(str(tmp_path / "bgzf_emul"), "bgzf_emul.cpp")
    assert run(reader, "scan", files[0]).rstrip().endswith("route 1")
    out = run(reader, "reader", files[0], src, 8 << 20, 1500, "host", 4)
    m = re.match(r"ok records (\d+) batches \d+ members_device 0 members_host 8 bytes_in (\d+) bytes_out (\d+) ", out)
    assert m and int(m.group(1)) == text.count(b"\n") // 4 and int(m.group(2)) == os.path.getsize(files[0]) and int(m.group(3)) == total, out


@pytest.mark.parametrize("which", ["sr", "hifi"])
def test_matches_and_dynamic_codes_each_earn_something(which, deflated, capsys):
    """summed over the members of a golden SAM text, the emulator's members are strictly smaller than zlib's at level 1 with
    Z_HUFFMAN_ONLY (no matches) and with Z_FIXED (no codes of its own), over the same 65280-byte blocks.  Its size against level 1
    itself is printed, not asserted."""
    data, z, _ = deflated[which + ".sam"]
    ours = len(z) - 28
    size = lambda level, strategy: sum(len(m) for m in bi.members_of(data, bi.MAX_MEMBER_BYTES, level, strategy))
    huffman, fixed, level1, level6 = size(1, zlib.Z_HUFFMAN_ONLY), size(1, zlib.Z_FIXED), size(1, zlib.Z_DEFAULT_STRATEGY), size(6, zlib.Z_DEFAULT_STRATEGY)
    with capsys.disabled():
        print("\n%s.golden.sam: raw %d, emulator %d, zlib level 1 %d (x%.3f), level 6 %d, Z_HUFFMAN_ONLY %d, Z_FIXED %d" % (which, len(data), ours, level1, ours / level1, level6, huffman, fixed))
    assert ours < huffman and ours < fixed


def test_python_writer_without_a_context(pkg, tmp_path):
    """BgzfWriter(ctx=None) through the C ABI: bytes, a bytearray, a slice of a read-only view and a ctypes buffer as one stream; the
    figures after the close; a failing write() is an error with its message"""
    import ctypes as C
    data = di.golden_text("sr")
    path = str(tmp_path / "w.sam.gz")
    with pkg.BgzfWriter(path, level=1, threads=3) as w:
        assert w.write(data[:100000]) == 100000 and w.write(bytearray(data[100000:300000])) == 200000
        w.flush()
        w.write(memoryview(data)[300000:])
        w.write(memoryview((C.c_char * 10).from_buffer_copy(b"0123456789")))
    z = open(path, "rb").read()
    assert z.endswith(bi.EOF_MARKER) and gzip.decompress(z) == data + b"0123456789"
    sizes = [i for _, i in di.member_sizes(z)]
    assert sizes[:4] == [65280] * 4 and sizes[4] == 300000 - 4 * 65280 and sizes[-1] == 0 and all(i == 65280 for i in sizes[5:-2])
    assert w.stats() == {"members_device": 0, "members_host": len(sizes) - 1, "bytes_in": len(data) + 10, "bytes_out": len(z)}
    with pytest.raises(pkg.GdietError) as e:
        pkg.BgzfWriter(str(tmp_path / "no" / "such" / "dir.gz"))
    assert "No such file" in str(e.value)
    if os.path.exists("/dev/full"):
        with pytest.raises(pkg.GdietError) as e:
            with pkg.BgzfWriter("/dev/full") as w:
                w.write(data)
        assert "BGZF writer: write" in str(e.value), str(e.value)

"""CPU: the decoder of csrc/bgzf_inflate.h on DEFLATE streams that zlib never writes (tests/deflate_streams.py), and the limiter of the
encoder's code builder inside a real block.  The reader of deflate_streams.py is held against zlib on every stream, the families are held
to their coverage conditions (what the old member matrix never reached is asserted as found), and the sanitized emulator
(tests/emul/bgzf_emul.cpp under AddressSanitizer / UBSan, as in tests/test_bgzf.py) decodes every valid stream to zlib's bytes and
refuses every invalid one with the listed class.  tests/test_deflate_streams_gpu.py sends the same streams to the kernel."""
import gzip
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_deflate_inputs as di
import bgzf_inputs as bi
import deflate_streams as ds
from conftest import ROOT

TIMEOUT = 120  # seconds; a run takes about one
CSRC = os.path.join(ROOT, "genome-on-diet_amd", "csrc")
SAN = ["-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
NAMES = list(ds.FAMILIES)


def build(exe, source, *flags):
    subprocess.check_call(["g++"] + SAN + list(flags) + ["-I", CSRC, os.path.join(ROOT, "tests", "emul", source), "-o", exe, "-lz"])
    return exe


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("deflate_streams") / "bgzf_emul"), "bgzf_emul.cpp")


@pytest.fixture(scope="module")
def deflate_emuls(tmp_path_factory):
    d = tmp_path_factory.mktemp("deflate_streams_writer")
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


def record_of(streams):
    rec = ds.Record()
    for s in streams:
        rec.merge(ds.walk(s)[1])
    return rec


@pytest.fixture(scope="module")
def records():
    """family -> Record; every stream through zlib, the reader and the family's own statement of its bytes on the way"""
    out = {}
    for fam in NAMES:
        rec = ds.Record()
        for name, stream, want in ds.family(fam):
            assert len(stream) <= ds.MAX_STREAM and len(want) <= ds.MAX_OUT, name
            assert zlib.decompress(stream, -15) == want, name
            got, r = ds.walk(stream)
            assert got == want, name
            rec.merge(r)
        out[fam] = rec
    return out


def test_reader_zlib_and_the_families_agree(records, capsys):
    assert sorted(records) == sorted(NAMES) and all(r.streams == len(ds.family(f)) for f, r in records.items())
    assert len({name for f in NAMES for name, _, _ in ds.family(f)}) == sum(len(ds.family(f)) for f in NAMES)  # a name names one stream
    with capsys.disabled():
        for f in NAMES:
            print("\n%s: %s" % (f, records[f].summary()))


def test_what_the_old_matrix_never_reached():
    """the record of what was missing: the member matrix of tests/bgzf_inputs.py, the whole input of test_inflate_the_member_matrix"""
    rec = ds.Record()
    for name, m, data in bi.matrix(np.random.default_rng(1)):
        got, r = ds.walk(m[18 + (m[10] - 6):-8])
        assert got == data, name
        rec.merge(r)
    assert sorted(rec.len_syms) == list(range(257, 267)) + [281, 285]  # 12 of 29: 267..280 and 282..284 never
    assert max(rec.lit_bits) == 14 and max(rec.dist_bits) == 12
    assert sum(rec.crossing.values()) == 0 and rec.rep16_zero == 0
    assert rec.max_blocks == 5


def test_coverage_conditions(records):
    """conditions on the inputs, with no margin: what the families are there to reach"""
    rec = ds.Record()
    for r in records.values():
        rec.merge(r)
    assert rec.len_syms == set(range(257, 286)) and rec.dist_syms == set(range(30))
    assert set(rec.lit_bits) == set(range(1, 16)) and set(rec.dist_bits) == set(range(1, 16)) and set(rec.clen_bits) == set(range(1, 8))
    assert {257, 286} <= rec.hlit and {1, 30} <= rec.hdist and {5, 19} <= rec.hclen
    assert all(rec.reps[s] and rec.crossing[s] for s in (16, 17, 18)) and rec.rep16_zero
    assert rec.no_dist_blocks and rec.one_dist_blocks
    assert rec.block_types[0] and rec.block_types[1] and rec.block_types[2]
    assert rec.max_blocks >= 300 and rec.max_out == 65536
    # ... and family by family, so that none leans on the random one
    r = records["symbols"]
    assert r.len_syms == set(range(257, 286)) and r.dist_syms == set(range(30)) and r.reach_first >= 2
    pairs = [(d, l) for d in ds.OVERLAP_DIST for l in ds.OVERLAP_LEN]
    r = records["overlap"]
    assert {p for p in pairs if p[0] < p[1]} | {(1, 3), (5, 10)} <= r.overlaps and r.copies >= 2 * len(pairs)
    r = records["long_codes"]
    assert set(r.lit_bits) >= set(range(1, 16)) and set(r.dist_bits) >= set(range(1, 16)) and set(r.clen_bits) == set(range(1, 8))
    r = records["header"]
    assert {257, 286} <= r.hlit and {1, 30} <= r.hdist and {5, 19} <= r.hclen
    assert all(r.crossing[s] == 1 for s in (16, 17, 18)) and r.rep16_zero == 2 and r.no_dist_blocks == 2 and r.one_dist_blocks == 2
    assert records["blocks"].max_blocks == 300 and records["blocks"].block_types[0] >= 8 + 3 + 6
    sizes = {len(s) for _, s, _ in ds.family("ring")}
    assert {1023, 1024, 1025, 2047, 2048, 2049} <= sizes
    r = records["random"]
    assert r.streams == 300 and set(r.lit_bits) == set(range(1, 16)) and set(r.dist_bits) == set(range(1, 16)) and r.crossing[16]
    # the placements of the full member: its output starts at every offset modulo 16
    at, starts = 0, set()
    for name, _, want in ds.family("full"):
        if name.startswith("full-behind"):
            assert len(want) == 65536
            starts.add(at % 16)
        at += len(want)
    assert starts == set(range(16))


def file_of(fam):
    return b"".join(ds.member(s, want) for _, s, want in ds.family(fam)) + bi.EOF_MARKER


@pytest.mark.parametrize("fam", NAMES)
def test_emulator_decodes_every_valid_stream(fam, emul, tmp_path):
    """a family as one BGZF file through the emulated kernel: every stream valid, the bytes zlib's, the sanitizers silent"""
    z = file_of(fam)
    assert gzip.decompress(z) == b"".join(want for _, _, want in ds.family(fam))
    n = len(ds.family(fam)) + 1
    out = run(emul, "decode", put(tmp_path, fam + ".bgzf", z))
    assert out == "ok members %d streams %d valid %d bytes %d\n" % (n, n, n, sum(len(want) for _, _, want in ds.family(fam))), out


def test_emulator_and_zlib_refuse_every_invalid_stream(emul, tmp_path):
    """every entry of invalid(): zlib refuses it, the emulated kernel refuses it with the listed class (and `agree` ends with status 1
    where the two differ), the sanitizers stay silent.  What the GPU test sends has passed here."""
    inv = ds.invalid()
    assert len({name for name, _, _, _ in inv}) == len(inv)
    assert {err for _, _, _, err in inv} == {ds.E_INPUT, ds.E_BTYPE, ds.E_STORED, ds.E_LENS, ds.E_CODE, ds.E_DIST, ds.E_OUTPUT}
    for name, stream, isize, err in inv:
        assert ds.zlib_refuses(stream, isize), name
        if err != ds.E_OUTPUT:
            with pytest.raises(ValueError):
                ds.walk(stream)
        else:  # valid deflate, one byte more than the trailer says
            assert len(ds.walk(stream)[0]) == isize + 1, name
    out = run(emul, "agree", put(tmp_path, "invalid.bgzf", b"".join(ds.member_with_trailer(s, isize) for _, s, isize, _ in inv)))
    lines = out.strip().split("\n")
    assert lines[-1] == "ok members %d streams %d valid 0 bytes 0" % (len(inv), len(inv)), out
    for k, (name, _, _, err) in enumerate(inv):
        m = re.match(r"member %d code (\d) \((.*)\) out \d+$" % k, lines[k])
        assert m and int(m.group(1)) != 0 and m.group(2) == err, (name, lines[k])
    # `agree` on valid members prints code 0
    out = run(emul, "agree", put(tmp_path, "valid.bgzf", file_of("overlap")))
    assert out.count(" code 0 (ok) ") == len(ds.family("overlap")) + 1 and " valid %d " % (len(ds.family("overlap")) + 1) in out, out


def deflate(exes, tmp_path, name, data):
    """(file bytes, report) of both builds of the writer's emulator: equal, or the test fails"""
    src = put(tmp_path, name + ".in", data)
    outs = []
    for k, exe in enumerate(exes):
        dst = str(tmp_path / ("%s.%d.gz" % (name, k)))
        outs.append((run(exe, "deflate", src, dst), open(dst, "rb").read()))
    assert outs[0] == outs[1], "%s: the members depend on the order of the lanes" % name
    return outs[0][1], outs[0][0]


def test_the_limiter_acts_inside_a_block(deflate_emuls, tmp_path):
    """the inputs of bgzf_deflate_inputs.limiter_inputs(): the code-length code's limiter (7 bits) cuts in at least one block, the members
    are those of both lane orders and inflate to the input (the emulator checks zlib, the scan and the project's decoder itself)"""
    for name, data in di.limiter_inputs():
        z, report = deflate(deflate_emuls, tmp_path, name, data)
        assert gzip.decompress(z) == data, name
        cuts = [tuple(int(x) for x in c) for c in re.findall(r" cut (\d+) (\d+) (\d+)$", report, re.M)]
        assert len(cuts) == -(-len(data) // bi.MAX_MEMBER_BYTES), report
        assert sum(c[2] for c in cuts) >= 1, (name, report)
        rec = record_of(m[18:-8] for m in members_of_file(z))
        assert max(rec.clen_bits) == 7 and rec.block_types[2] >= 1, rec.summary()  # the limited code is in the stream, and used


def members_of_file(z):
    out, at = [], 0
    for n, _ in di.member_sizes(z):
        out.append(z[at:at + n])
        at += n
    return out


def test_the_writers_streams_use_every_length_and_distance_symbol(deflate_emuls, tmp_path, capsys):
    """all 29 length symbols and all 30 distance symbols occur in what the writer's emulator makes of its test inputs (and so in what the
    kernel makes of them: tests/test_bgzf_deflate_gpu.py holds the two equal).  The inputs are walked until all have been seen."""
    rec = ds.Record()
    for name, data in di.inputs():
        if len(rec.len_syms) == 29 and len(rec.dist_syms) == 30:
            break
        src, dst = put(tmp_path, "w.in", data), str(tmp_path / "w.gz")
        run(deflate_emuls[0], "deflate", src, dst)
        for m in members_of_file(open(dst, "rb").read()):
            got, r = ds.walk(m[18:-8])
            assert len(got) == int.from_bytes(m[-4:], "little")
            rec.merge(r)
    with capsys.disabled():
        print("\nthe writer's streams: %s" % rec.summary())
    assert rec.len_syms == set(range(257, 286)) and rec.dist_syms == set(range(30))

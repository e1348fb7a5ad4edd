"""CPU: duplicate marking.  The oracle is tests/markdup_ref.py, an independent restatement of the section "Duplicate marking" of
include/gdiet_hip.h.  tests/emul/markdup_emul.cpp runs the statements of the kernels (bam_markdup.h) as a stand-alone program under
AddressSanitizer / UBSan on exact-size buffers, every record with the lanes running 0..63 and 63..0 and at every alignment of the buffer,
and GdqSorter with marking on over a host executor, on both compressor routes.
  * the restatement itself, on records whose answer is written down here;
  * the kernel-level boundary: every designed set (tests/markdup_inputs.py) gives the restatement's bytes and counts, and differs from its
    input in bit 0x400 alone; one bad record of each kind fails the run and names the record;
  * the sorter: run and chunk sizes and both routes give one file per route and one stream; its records are the restatement applied to
    the records of the file written with marking off, which is the file bam_sort_emul writes."""
import gzip
import os
import struct
import subprocess

import pytest

import bam_ref
import bam_sort_inputs as si
import bam_sort_ref as sr
import markdup_inputs as mi
import markdup_ref as md
from conftest import ROOT

DESIGNED = mi.designed()


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("markdup") / "markdup_emul")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "genome-on-diet_amd", "csrc"), "-I", os.path.join(ROOT, "tests", "emul"), os.path.join(ROOT, "tests", "emul", "markdup_emul.cpp"), "-o", exe,
                           "-lz", "-pthread"])
    return exe


def run(emul, args, status=0):
    r = subprocess.run([emul] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == status, (r.returncode, r.stderr[-2000:])
    return r.stdout if status == 0 else r.stderr


def emul_mark(emul, data, tmp_path, status=0):
    p = [str(tmp_path / n) for n in ("in.recs", "out.recs")]
    open(p[0], "wb").write(data)
    if os.path.exists(p[1]):
        os.remove(p[1])
    text = run(emul, ["mark"] + p, status=status)
    if status:
        assert not os.path.exists(p[1])  # nothing was written
        return text
    return open(p[1], "rb").read(), dict(zip(("examined", "eligible", "duplicates", "max_group"), (int(x) for x in text.split())))


def flags(data):
    return {r[36:36 + r[12] - 1].decode(): struct.unpack_from("<H", r, 18)[0] for r in md.split(data)}


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------
def test_restatement_on_the_clip_cases():
    apart, together = mi.clip_cases()
    assert [md.entry(r)[0] for r in apart] == [(0, 100, 0), (0, 97, 0), (0, 96, 0), (0, 95, 0), (0, 219, 1), (0, 222, 1), (0, 223, 1), (0, 224, 1)]
    assert [md.entry(r)[0] for r in together] == [(0, 100, 0)] * 4 + [(0, 219, 1)] * 5 + [(0, 219, 0)]
    out, st = md.markdup(b"".join(apart))
    assert out == b"".join(apart) and st == dict(examined=8, eligible=8, duplicates=0, max_group=1)
    out, st = md.markdup(b"".join(together))
    assert st == dict(examined=10, eligible=10, duplicates=7, max_group=5) and md.only_dup_bit_differs(out, b"".join(together))


def test_restatement_on_long_cigars_placeholder_and_scores():
    e = [md.entry(r) for r in mi.long_cigars()]
    assert all(e[k][0] == e[k + 1][0] for k in (0, 2, 4, 6)) and len({x[0] for x in e}) == 4
    assert e[4][0] == (1, 6998, 0) and e[6][0][1] == 8000 + 95 - 1 + 4
    p = [md.entry(r) for r in mi.placeholder()]
    assert p[0][0] == p[1][0] == (2, 1000 + 65534 - 1 + 3, 1)
    f = flags(md.markdup(b"".join(mi.qual_cases()))[0])
    assert [n for n, v in f.items() if not v & 0x400] == ["best"]
    by_name = {r[36:36 + r[12] - 1].decode(): md.entry(r)[1] for r in mi.qual_cases()}
    assert by_name["edge_a"] == by_name["edge_b_same_score"] == 86 and by_name["q4097_missing"] == 0 and by_name["best"] == 40 * 4097
    two = [r for r in mi.qual_cases() if r[36:40] == b"edge"]
    assert [v & 0x400 for v in flags(md.markdup(b"".join(two))[0]).values()] == [0, 0x400]  # equal scores: the first in the buffer wins
    assert [v & 0x400 for v in flags(md.markdup(b"".join(two[::-1]))[0]).values()] == [0, 0x400]


def test_restatement_on_eligibility_and_range():
    recs = mi.eligibility()
    before, after = flags(b"".join(recs)), flags(md.markdup(b"".join(recs))[0])
    assert after["winner_was_marked"] == 0 and after["loser_was_clear"] == 0x400 and after["paired_bits_do_not_matter"] == before["paired_bits_do_not_matter"]
    assert all(after[n] == before[n] for n in before if n.startswith(("in", "no_", "secondary")))
    assert md.markdup(b"".join(recs))[1] == dict(examined=len(recs), eligible=3, duplicates=1, max_group=2)
    e = [md.entry(r) for r in mi.range_edges()]
    assert e[0][0] == ((1 << 30) - 1, (1 << 32) - 2, 1) and e[2][0] == (0, -(1 << 32), 0) and md.key64(e[0][0]) == md.SENTINEL - 2 and md.key64(e[2][0]) == 0
    for name, (r, reason) in mi.BAD.items():
        assert md.entry(r) == reason, name
    with pytest.raises(md.Bad) as x:
        md.markdup(b"".join(mi.with_bad("op9")))
    assert (x.value.index, x.value.reason) == (5, "op")


# ---- the kernel-level boundary ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_designed_sets(name, emul, tmp_path):
    data = b"".join(DESIGNED[name])
    want, want_st = md.markdup(data)
    got, st = emul_mark(emul, data, tmp_path)
    assert got == want and st == want_st
    assert md.only_dup_bit_differs(got, data)
    if name == "groups":
        assert st["max_group"] == 65 and st["duplicates"] == 0 + 1 + 63 + 64
    if name == "one_group":
        assert st["max_group"] == 257 == st["duplicates"] + 1


@pytest.mark.parametrize("kind", ["sr", "hifi_sv"])
def test_doubled_goldens(kind, emul, tmp_path):
    recs, _ = si.golden_records(kind)
    data = b"".join(mi.doubled(recs))
    want, want_st = md.markdup(data)
    assert want_st["duplicates"] >= want_st["eligible"] // 2 > 10
    assert emul_mark(emul, data, tmp_path) == (want, want_st)


@pytest.mark.parametrize("name", sorted(mi.BAD))
def test_a_bad_record_fails_the_run(name, emul, tmp_path):
    text = emul_mark(emul, b"".join(mi.with_bad(name)), tmp_path, status=3)
    assert "record 5 of the buffer" in text and md.REASON_TEXT[mi.BAD[name][1]] in text


def test_a_truncated_buffer_is_refused(emul, tmp_path):
    assert "ends inside a record" in emul_mark(emul, b"".join(mi.counted(5))[:-1], tmp_path, status=3)


# ---- the sorter over the host executor -----------------------------------------------------------------------------------------------
def emul_sorter(emul, data, header, per_batch, run_bytes, chunk_bytes, device, markdup, tmp_path, status=0):
    spool = str(tmp_path / "spool")
    os.makedirs(spool, exist_ok=True)
    p = [str(tmp_path / n) for n in ("s.recs", "s.header", "s.bam")]
    open(p[0], "wb").write(data)
    open(p[1], "wb").write(header)
    text = run(emul, ["sorter", p[0], per_batch, run_bytes, chunk_bytes, spool, p[1], int(device), p[2], int(markdup)], status=status)
    if status:
        return text
    assert os.listdir(spool) == []
    v = [int(x) for x in text.split()]
    return open(p[2], "rb").read(), open(p[2] + ".bai", "rb").read(), dict(zip(("records", "runs", "spooled_bytes", "chunks"), v[:4])), dict(zip(("examined", "eligible", "duplicates", "max_group"), v[6:]))


def sorter_inputs(kind):
    if kind == "spread":
        return mi.spread_groups(), si.REFS
    recs, names = si.golden_records(kind)
    return mi.doubled(recs), names


@pytest.mark.parametrize("kind", ["spread", "sr", "hifi_sv"])
def test_sorter_marks_like_the_restatement(kind, emul, tmp_path):
    recs, names = sorter_inputs(kind)
    data = b"".join(recs)
    header = bam_ref.bam_header("@HD\tVN:1.6\tSO:coordinate\n", [(n, 1 << 28) for n in names])
    per_batch = max(1, len(recs) // 8)
    plain = sr.sort_records(data)
    want, want_st = md.markdup(plain)
    assert want_st["duplicates"] > 10 and md.only_dup_bit_differs(want, plain) and want != plain
    streams = set()
    for device in (0, 1):
        files = set()
        for run_bytes, chunk_bytes in ((1 << 29, 1 << 28), (4096, 1 << 28), (4096, 4096), (4096, 1), (len(data) // 3, 4096)):
            raw, bai, st, dup = emul_sorter(emul, data, header, per_batch, run_bytes, chunk_bytes, device, True, tmp_path)
            assert gzip.decompress(raw) == header + want and dup == want_st and st["records"] == len(recs)
            assert (st["runs"] == 1) == (run_bytes == 1 << 29) and (chunk_bytes != 1 or st["chunks"] == len(recs))
            assert bai == sr.bai(sr.rows(want), len(names), len(header), len(want), sr.members(raw))
            files.add(raw), streams.add(gzip.decompress(raw))
        assert len(files) == 1  # per route: a function of the input records alone
        if kind != "hifi_sv":
            off, _, _, dup = emul_sorter(emul, data, header, per_batch, 4096, 4096, device, False, tmp_path)
            assert gzip.decompress(off) == header + plain and dup == dict(examined=0, eligible=0, duplicates=0, max_group=0)
    assert len(streams) == 1
    if kind == "spread":  # every group's winner is its last member in input order, four runs behind its first
        assert all((v & 0x400 == 0) == n.endswith("_4") for n, v in flags(want).items() if n.startswith("sp"))


def test_sorter_fails_on_a_bad_record(emul, tmp_path):
    header = bam_ref.bam_header("@HD\tVN:1.6\tSO:coordinate\n", [("c%d" % k, 1 << 28) for k in range(4)])
    data = b"".join(mi.with_bad("op9"))
    for run_bytes in (1 << 29, 200):
        assert "operation code above 8" in emul_sorter(emul, data, header, 3, run_bytes, 4096, 0, True, tmp_path, status=5)
        assert not os.path.exists(str(tmp_path / "s.bam.bai"))
    raw = emul_sorter(emul, data, header, 3, 200, 4096, 0, False, tmp_path)[0]  # with marking off nobody looks at the CIGAR's codes
    assert gzip.decompress(raw) == header + sr.sort_records(data)

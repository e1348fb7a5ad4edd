"""GPU: duplicate marking on the device (dup_key_kernel, hipCUB's two stable radix sorts, dup_decide_kernel, dup_apply_kernel) through the
kernel-level boundary Context.bam_markdup_records, the sorter (BamSorter(markdup=True): one decision over runs and chunks, both compressors,
the .bai) and tools/map_file.py --bam --sort --markdup.  The oracle is the restatement tests/markdup_ref.py; the designed records are those
of the CPU tests (tests/markdup_inputs.py), where tests/emul/markdup_emul.cpp runs the same statements under the sanitizers."""
import ctypes as C
import gzip
import json
import os
import struct
import subprocess
import sys
import types

import numpy as np
import pytest

import bam_sort_inputs as si
import bam_sort_ref as sr
import markdup_inputs as mi
import markdup_ref as md
from conftest import ROOT
from fixture_io import OVERRIDES, SETS, read_fasta
import samopts_io as so

pytestmark = pytest.mark.gpu

DESIGNED = mi.designed()
NO_STATS = dict(examined=0, eligible=0, duplicates=0, max_group=0)


# ---- the kernel-level boundary ---------------------------------------------------------------------------------------------------------
def check(gpu_ctx, data):
    got, st = gpu_ctx.bam_markdup_records(data)
    want, want_st = md.markdup(data)
    assert len(got) == len(want) and got == want and st == want_st
    assert md.only_dup_bit_differs(got, data)  # only flag bytes differ from the input, and of those bit 0x400 alone
    return got, st


@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_designed_sets(name, gpu_ctx):
    """record counts around the blocks of four wavefronts and of 256 threads; groups of 1, 2, 64, 65 and of all records; record starts at
    all four alignments; the clip cases of both strands, apart, together and mixed; CIGARs of 130 operations whose clip runs end behind
    word 64 or have clips at the lanes' second words; a CG:B:I array of 65 536 operations; QUAL of 0 .. 4 097 bytes and missing, values
    on both sides of 15, equal scores; every ineligible flag on its own and the 0x400 bits that came in; the ends of the key's range"""
    _, st = check(gpu_ctx, b"".join(DESIGNED[name]))
    if name == "groups":
        assert st["max_group"] == 65 and st["duplicates"] == 128
    if name == "one_group":
        assert st["max_group"] == 257 and st["duplicates"] == 256
    if name == "clips_apart":
        assert st["duplicates"] == 0
    if name == "clips_together":
        assert (st["duplicates"], st["max_group"]) == (7, 5)


@pytest.mark.parametrize("kind", ["sr", "hifi_sv"])
def test_doubled_goldens(kind, gpu_ctx):
    recs, _ = si.golden_records(kind)
    _, st = check(gpu_ctx, b"".join(mi.doubled(recs)))
    assert st["duplicates"] >= st["eligible"] // 2 > 10


def test_the_buffers_order_breaks_ties(gpu_ctx):
    two = [r for r in mi.qual_cases() if r[36:40] == b"edge"]
    for pair in (two, two[::-1]):
        got, _ = check(gpu_ctx, b"".join(pair))
        assert [struct.unpack_from("<H", r, 18)[0] & 0x400 for r in md.split(got)] == [0, 0x400]


@pytest.mark.parametrize("name", sorted(mi.BAD))
def test_a_bad_record_fails_the_call_and_writes_nothing(name, pkg, gpu_ctx):
    data = b"".join(mi.with_bad(name))
    with pytest.raises(pkg.GdietError, match=r"error -3: .*record 5 of the buffer: .*" + md.REASON_TEXT[mi.BAD[name][1]]):
        gpu_ctx.bam_markdup_records(data)
    out = C.create_string_buffer(b"\xa5" * len(data), len(data))
    st = pkg.hip_abi.DupStats()
    assert gpu_ctx.lib.gdiet_hip_bam_markdup_records(gpu_ctx._h, data, len(data), C.cast(out, C.c_void_p), C.byref(st)) == -3
    assert out.raw == b"\xa5" * len(data) and st.as_dict() == NO_STATS
    check(gpu_ctx, b"".join(mi.counted(9)))  # the context marks on


def test_a_truncated_buffer_is_refused(pkg, gpu_ctx):
    with pytest.raises(pkg.GdietError, match="ends inside a record"):
        gpu_ctx.bam_markdup_records(b"".join(mi.counted(5))[:-1])


# ---- the sorter --------------------------------------------------------------------------------------------------------------------
LIMIT = {"sr": None, "hifi_sv": None}  # reads of the golden set that are mapped (None: all)
N_BATCHES = 8


class Batch:
    """C arrays of the reads picked by idx from a mapped set, under other names and with lowered qualities (0: as they are)"""

    def __init__(self, pkg, reads, res, idx, lower, tag):
        self.n = n = len(idx)
        low = lambda q: "".join(chr(max(ord(c) - lower, 33)) for c in q)
        self.names = (C.c_char_p * n)(*[(reads[i][0] + tag).encode() for i in idx])
        self.seqs = (C.c_char_p * n)(*[reads[i][1].encode() for i in idx])
        self.quals = (C.c_char_p * n)(*[low(reads[i][2]).encode() for i in idx])
        self.lens = np.array([len(reads[i][1]) for i in idx], np.int32)
        self.lens_p = self.lens.ctypes.data_as(C.POINTER(C.c_int32))
        self.res = types.SimpleNamespace(n_regs=(C.c_int32 * n)(*[res.n_regs[i] for i in idx]), regs=(C.POINTER(pkg.map_api.Reg) * n)(*[res.regs[i] for i in idx]))

    def args(self):
        return self.res, self.n, self.names, self.seqs, self.quals, self.lens_p


def sort_file(pkg, m, batches, path, tmp_dir, **kw):
    os.makedirs(tmp_dir, exist_ok=True)
    s = pkg.BamSorter(path, m, tmp_dir=tmp_dir, version=so.VERSION, argv=["x"], **kw)
    for b in batches:
        s.add(*b.args())
    st = s.close()
    assert os.listdir(tmp_dir) == []
    return open(path, "rb").read(), st


@pytest.fixture(scope="module")
def mapped(pkg, gpu_ctx, tmp_path_factory):
    """kind -> (mapper, batches, header, records of the file written with marking off, the restatement's marking of them and its
    counts), each kind mapped once for the module.  The batches: the golden reads in N_BATCHES batches; every batch a second time with
    changed names and qualities lowered by one, so that groups of two are certain; and one hand-built batch, every seventh read a third
    time with qualities lowered by two, whose groups have their other members in other batches -- with small runs in other runs, with
    chunks of one record in other chunks"""
    cache = {}

    def get(kind):
        if kind not in cache:
            base, _, preset = SETS[kind]
            names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
            reads = so.reads_with_comments(kind)[:LIMIT[kind]]
            m = pkg.Mapper(gpu_ctx, names, seqs, preset=preset, **OVERRIDES.get(kind, {}))
            res = m.map([r[1] for r in reads])
            cuts = [len(reads) * k // N_BATCHES for k in range(N_BATCHES + 1)]
            batches = [Batch(pkg, reads, res, range(a, b), 0, "") for a, b in zip(cuts, cuts[1:])]
            batches += [Batch(pkg, reads, res, range(a, b), 1, "_again") for a, b in zip(cuts, cuts[1:])]
            batches.append(Batch(pkg, reads, res, range(0, len(reads), 7), 2, "_third"))
            header = m.bam_header(so.VERSION, ["x"], sort_order="coordinate")
            d = tmp_path_factory.mktemp("plain_" + kind)
            raw, st = sort_file(pkg, m, batches, str(d / "plain.bam"), str(d / "spool"), markdup=False)
            assert "dup" not in st
            stream = gzip.decompress(raw)
            assert stream[:len(header)] == header
            plain = stream[len(header):]
            assert plain == sr.sort_records(b"".join(m.bam_batch_raw(*b.args()) for b in batches))
            want, want_st = md.markdup(plain)
            assert want_st["duplicates"] > 20 and want_st["max_group"] >= 3 and md.only_dup_bit_differs(want, plain) and want != plain
            cache[kind] = (m, batches, header, plain, want, want_st, res)  # (res: the batches point into the map result)
        return cache[kind]
    yield get
    for v in cache.values():
        v[0].close()


CHUNKS = (1, 4096, 1 << 40)
RUNS = (4096, 1 << 29)


@pytest.fixture(scope="module")
def marked(mapped, pkg, tmp_path_factory):
    """(kind, route, run_bytes) -> {chunk_bytes: (file, stats, .bai)} of the marking sorter, each written once for the module"""
    cache = {}

    def get(kind, route, run_bytes):
        if (kind, route, run_bytes) not in cache:
            m, batches = mapped(kind)[:2]
            d = tmp_path_factory.mktemp("marked")
            out = {}
            for chunk_bytes in CHUNKS:
                path = str(d / ("%d.bam" % chunk_bytes))
                raw, st = sort_file(pkg, m, batches, path, str(d / "spool"), bgzf=route, level=1, threads=2, run_bytes=run_bytes, chunk_bytes=chunk_bytes, markdup=True)
                out[chunk_bytes] = (raw, st, open(path + ".bai", "rb").read())
            cache[(kind, route, run_bytes)] = out
        return cache[(kind, route, run_bytes)]
    return get


@pytest.mark.parametrize("run_bytes", RUNS, ids=["runs_4096", "run_default"])
@pytest.mark.parametrize("route", ["device", "host"])
@pytest.mark.parametrize("kind", ["sr", "hifi_sv"])
def test_sorter_marks_like_the_restatement(kind, route, run_bytes, mapped, marked, gpu_ctx):
    """run size x chunk size (1, 4 096, unbounded) x compressor: the records are the restatement's marking of the records of the file
    written with marking off and differ from them in bit 0x400 alone, close()["dup"] is the restatement's counts, the .bai is the
    restatement's over the written file and region queries through it return the marked records"""
    m, batches, header, plain, want, want_st, _ = mapped(kind)
    for chunk_bytes, (raw, st, bai) in marked(kind, route, run_bytes).items():
        stream = gzip.decompress(raw)
        assert len(stream) == len(header) + len(want) and stream == header + want
        assert md.only_dup_bit_differs(stream[len(header):], plain)
        assert st["dup"] == want_st and st["records"] == len(md.split(want))
        if run_bytes == 4096:  # every batch is a run of its own; the chunks of one record are as many as the records
            assert st["runs"] == len(batches) and st["spooled_bytes"] == len(want) and (chunk_bytes != 1 or st["chunks"] == st["records"]) and (chunk_bytes != 1 << 40 or st["chunks"] == 1)
        else:
            assert (st["runs"], st["spooled_bytes"], st["chunks"]) == (1, 0, 0)
        assert bai == sr.bai(sr.rows(want), len(m.names), len(header), len(want), sr.members(raw))
    if route == "device":
        assert raw == gpu_ctx.bgzf_deflate(header + want, eof=True)
    # region queries through the written index return the marked records
    log, index = sr.members(raw), sr.parse_bai(bai)
    rws = [r for r in sr.rows(want) if r[2] >= 0]
    n_hits = n_marked = 0
    for ref in sorted({r[2] for r in rws}):
        mine = [r for r in rws if r[2] == ref]
        hi = max(r[4] for r in mine)
        for beg, end in ((0, hi + 1), (mine[len(mine) // 2][3], mine[len(mine) // 2][3] + 1), (hi - 1, hi)):
            hits = sr.brute(header + want, len(header), ref, beg, end)
            assert sr.query(index, stream, log, len(header), ref, beg, end) == hits, (ref, beg, end)
            n_hits += len(hits)
            n_marked += sum(1 for off in hits if struct.unpack_from("<H", stream, len(header) + off + 18)[0] & 0x400)  # (the file's own bytes at the offsets the index gave)
    assert n_hits > 20 and n_marked > 10


@pytest.mark.parametrize("kind", ["sr", "hifi_sv"])
def test_one_file_per_compressor_and_one_stream(kind, marked):
    """per compressor the file's bytes are identical across run and chunk sizes, and the decompressed file across all settings"""
    files = {route: {marked(kind, route, rb)[cb][0] for rb in RUNS for cb in CHUNKS} for route in ("device", "host")}
    assert len(files["device"]) == 1 and len(files["host"]) == 1
    assert gzip.decompress(files["device"].pop()) == gzip.decompress(files["host"].pop())


@pytest.mark.parametrize("route", ["device", "host"])
def test_marking_off_writes_what_the_sorter_wrote_before(route, mapped, pkg, gpu_ctx, tmp_path):
    """markdup=False, and a sorter that was never told about marking, write the same bytes: header + the restatement's sort of the records,
    on the device route Context.bgzf_deflate of that stream"""
    m, batches, header, plain, _, _, _ = mapped("sr")
    kw = dict(bgzf=route, level=1, threads=2, run_bytes=len(plain) // 3, chunk_bytes=65536)
    off, st = sort_file(pkg, m, batches, str(tmp_path / "off.bam"), str(tmp_path / "spool"), markdup=False, **kw)
    never, _ = sort_file(pkg, m, batches, str(tmp_path / "never.bam"), str(tmp_path / "spool"), **kw)
    assert off == never and gzip.decompress(off) == header + plain and "dup" not in st
    assert open(str(tmp_path / "off.bam.bai"), "rb").read() == open(str(tmp_path / "never.bam.bai"), "rb").read() == sr.bai(sr.rows(plain), len(m.names), len(header), len(plain), sr.members(off))
    if route == "device":
        assert off == gpu_ctx.bgzf_deflate(header + plain, eof=True)


def test_set_markdup_after_an_add_is_refused(mapped, pkg, tmp_path):
    m, batches, header, plain, _, _, _ = mapped("sr")
    os.makedirs(str(tmp_path / "spool"))
    with pkg.BamSorter(str(tmp_path / "late.bam"), m, tmp_dir=str(tmp_path / "spool"), version=so.VERSION, argv=["x"]) as s:
        s.set_markdup(True)
        s.set_markdup(False)  # before the first add the choice is open
        s.add(*batches[0].args())
        with pytest.raises(pkg.GdietError, match="error -3: .*before the first add"):
            s.set_markdup(True)
        st = s.close()  # the sorter sorts on, unmarked
    assert "dup" not in st and st["records"] > 0
    body = gzip.decompress(open(str(tmp_path / "late.bam"), "rb").read())[len(header):]
    assert body == sr.sort_records(m.bam_batch_raw(*batches[0].args()))


def test_the_old_close_drops_the_counts(mapped, pkg, tmp_path):
    """gdiet_hip_bam_sort_close on a marking sorter: the file is marked, the counts are simply not handed out"""
    m, batches, header, _, _, _, _ = mapped("sr")
    os.makedirs(str(tmp_path / "spool"))
    s = pkg.BamSorter(str(tmp_path / "old.bam"), m, tmp_dir=str(tmp_path / "spool"), version=so.VERSION, argv=["x"], markdup=True)
    for b in (batches[0], batches[N_BATCHES]):
        s.add(*b.args())
    h, s._h = s._h, C.c_void_p()
    assert s.lib.gdiet_hip_bam_sort_close(h, None) == 0
    body = gzip.decompress(open(str(tmp_path / "old.bam"), "rb").read())[len(header):]
    want, st = md.markdup(sr.sort_records(b"".join(m.bam_batch_raw(*b.args()) for b in (batches[0], batches[N_BATCHES]))))
    assert body == want and st["duplicates"] > 10


# ---- the tool ----------------------------------------------------------------------------------------------------------------------
def test_map_file_sort_markdup(tmp_path):
    """tools/map_file.py --bam --sort --markdup from file to file on 400 sr reads, each twice, against the same tool without --markdup"""
    fq = str(tmp_path / "reads.fq")
    reads = so.reads_with_comments("sr")[:400]
    with open(fq, "w") as f:
        for tag, lower in (("", 0), ("_again", 1)):
            for name, seq, qual, _ in reads:
                f.write("@%s%s\n%s\n+\n%s\n" % (name, tag, seq, "".join(chr(max(ord(c) - lower, 33)) for c in qual)))
    base = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "map_file.py"), "--preset", "sr", os.path.join(SETS["sr"][0], "ref.fa.gz"), fq, "--bam"]

    def run(extra, out, status=0):
        r = subprocess.run(base + extra + ["-o", out], capture_output=True, text=True)
        assert r.returncode == status, r.stderr[-3000:]
        return (json.loads(r.stdout.strip().split("\n")[-1]), open(out, "rb").read()) if status == 0 else r.stderr

    def records(raw):
        stream = gzip.decompress(raw)
        at = 8 + struct.unpack_from("<i", stream, 4)[0]
        n_ref = struct.unpack_from("<i", stream, at)[0]
        at += 4
        for _ in range(n_ref):
            at += 8 + struct.unpack_from("<i", stream, at)[0]
        return stream[at:], n_ref, at

    assert "--markdup needs --bam --sort" in run(["--markdup"], str(tmp_path / "no.bam"), status=2)
    rep, plain = run(["--sort", "--index", "--tmp-dir", str(tmp_path)], str(tmp_path / "plain.bam"))
    assert "dup" not in rep["bam_sort"]
    body, n_ref, at = records(plain)
    want, want_st = md.markdup(body)
    assert want_st["duplicates"] > 100
    rep, raw = run(["--sort", "--index", "--markdup", "--tmp-dir", str(tmp_path)], str(tmp_path / "marked.bam"))
    got, _, at2 = records(raw)
    assert got == want and rep["bam_sort"]["dup"] == want_st and md.only_dup_bit_differs(got, body)
    assert open(str(tmp_path / "marked.bam.bai"), "rb").read() == sr.bai(sr.rows(want), n_ref, at2, len(want), sr.members(raw))

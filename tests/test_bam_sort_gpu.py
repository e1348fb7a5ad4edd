"""GPU: BAM records put into coordinate order on the device (bam_key_kernel, hipCUB's radix sort and scan, bam_gather_kernel) through the
kernel-level boundary Context.bam_sort_records, the sorter (BamSorter: runs, spools, the merge in chunks, both compressors, the .bai) and
tools/map_file.py --bam --sort --index.  The oracle is the restatement tests/bam_sort_ref.py; the host emulator
tests/emul/bam_sort_emul.cpp is fed the same bytes."""
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

import bam_ref
import bam_sort_inputs as si
import bam_sort_ref as sr
from conftest import ROOT
from fixture_io import OVERRIDES, SETS, read_fasta
import samopts_io as so
from test_samopts_gpu import write_fastq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bam_sort_gpu") / "bam_sort_emul")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "genome-on-diet_amd", "csrc"), os.path.join(ROOT, "tests", "emul", "bam_sort_emul.cpp"), "-o", exe, "-lz", "-pthread"])
    return exe


def emul_sort(emul, data, tmp_path):
    p = [str(tmp_path / n) for n in ("in.recs", "out.recs", "out.rows")]
    open(p[0], "wb").write(data)
    r = subprocess.run([emul, "sort"] + p, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return open(p[1], "rb").read(), np.fromfile(p[2], sr_row_dtype())


def sr_row_dtype():
    return np.dtype([("key", "<u8"), ("out", "<u8"), ("refID", "<i4"), ("pos", "<i4"), ("end", "<i4"), ("bin", "<u2"), ("flag", "<u2")])


def check(gpu_ctx, data, emul=None, tmp_path=None):
    got, rows = gpu_ctx.bam_sort_records(data)
    want = sr.sort_records(data)
    assert len(got) == len(want) and got == want
    assert rows.dtype == sr_row_dtype() and [tuple(int(x) for x in r) for r in rows] == sr.rows(want)
    if emul:
        e_bytes, e_rows = emul_sort(emul, data, tmp_path)
        assert got == e_bytes and rows.tobytes() == e_rows.tobytes()
    return got, rows


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257])
def test_record_counts(n, gpu_ctx, emul, tmp_path):
    """one thread per record in blocks of 256, one wavefront per record in blocks of four: counts around both"""
    _, rows = check(gpu_ctx, b"".join(si.counted(n)), emul, tmp_path)
    assert len(rows) == n


def test_key_cases(gpu_ctx, emul, tmp_path):
    """equal position on both strands, fully equal keys (input order kept), refID -1 last, pos -1 first, three contigs interleaved"""
    got, rows = check(gpu_ctx, b"".join(si.key_cases()), emul, tmp_path)
    names = [bam_ref.bam_to_sam(r, si.REFS)[0].split("\t")[0] for r in sr.split(got)]
    assert names == ["c1_posm1", "c1_first", "c1_fwd", "equal_1", "equal_2", "equal_3", "c1_rev", "c1_unmapped_placed", "c2_x", "c2_y", "c3_early", "c3_late", "unplaced_a", "unplaced_b"]
    assert list(rows["refID"][-2:]) == [-1, -1] and rows["pos"][0] == -1 and rows["end"][0] == 0


def test_cigar_cases(gpu_ctx, emul, tmp_path):
    """n_cigar_op 0, 1, 64, 65: lane l sums the words l, l + 64; the placeholder's end comes from its N, not from CG"""
    recs = si.cigar_cases()
    got, rows = check(gpu_ctx, b"".join(recs), emul, tmp_path)
    by_name = {bam_ref.bam_to_sam(r, si.REFS)[0].split("\t")[0]: row for r, row in zip(sr.split(got), rows)}
    assert by_name["placeholder"]["end"] == 32768 + 40000 and by_name["ops0"]["end"] == by_name["ops0"]["pos"] + 1 and by_name["ops1"]["end"] == 16383 + 30
    for n in (64, 65):
        want = sum(1 + k % 3 for k in range(n) if "MIDN=X"[k % 6] in "MDN=X")
        assert by_name["ops%d" % n]["end"] - by_name["ops%d" % n]["pos"] == want


def test_sizes_and_alignments(gpu_ctx, emul, tmp_path):
    """from 38 bytes to more than 64 x 16, every size mod 16; the shuffles put sources and destinations at every alignment"""
    recs = si.size_cases()
    src_dst = set()
    for seed in (1, 2, 3):
        order = list(recs)
        np.random.default_rng(seed).shuffle(order)
        data = b"".join(order)
        got, rows = check(gpu_ctx, data, emul if seed == 1 else None, tmp_path)
        place = {bytes(r): int(o) for r, o in zip(sr.split(got), rows["out"])}
        at = 0
        for r in order:
            src_dst.add((at % 4, place[r] % 4))
            at += len(r)
    assert len(src_dst) == 16  # every pair of source and destination alignment mod 4, the unit of the copy


@pytest.mark.parametrize("kind", ["sr", "hifi_sv"])
def test_golden_records(kind, gpu_ctx, emul, tmp_path):
    recs, _ = si.golden_records(kind)
    check(gpu_ctx, b"".join(recs), emul, tmp_path)


def test_malformed_records_are_refused(pkg, gpu_ctx):
    data = b"".join(si.key_cases())
    with pytest.raises(pkg.GdietError, match="ends inside a record"):
        gpu_ctx.bam_sort_records(data[:-1])
    with pytest.raises(pkg.GdietError, match="block_size"):
        gpu_ctx.bam_sort_records(b"\x05\0\0\0" + data)


# ---- the sorter --------------------------------------------------------------------------------------------------------------------
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
N_BATCHES = 8
_mapped = {}


class Slice:
    """C arrays of reads[lo:hi] of a mapped set, and the view of the MapResult that goes with them"""

    def __init__(self, pkg, reads, res, lo, hi):
        rr = reads[lo:hi]
        self.n = n = len(rr)
        self.names = (C.c_char_p * n)(*[r[0].encode() for r in rr])
        self.seqs = (C.c_char_p * n)(*[r[1].encode() for r in rr])
        self.quals = (C.c_char_p * n)(*[r[2].encode() for r in rr])
        self.lens = np.array([len(r[1]) for r in rr], np.int32)
        self.lens_p = self.lens.ctypes.data_as(C.POINTER(C.c_int32))
        self.res = types.SimpleNamespace(n_regs=(C.c_int32 * n)(*res.n_regs[lo:hi]), regs=(C.POINTER(pkg.map_api.Reg) * n)(*[res.regs[i] for i in range(lo, hi)]))

    def args(self):
        return self.res, self.n, self.names, self.seqs, self.quals, self.lens_p


@pytest.fixture(scope="module")
def mapped(pkg, gpu_ctx):
    """kind -> (mapper, batches, their records in input order as bam_batch_raw gives them, the sorted file's uncompressed stream), each
    kind mapped once for the module; secondary and supplementary records are kept"""
    def get(kind):
        if kind not in _mapped:
            base, _, preset = SETS[kind]
            names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
            reads = so.reads_with_comments(kind)
            m = pkg.Mapper(gpu_ctx, names, seqs, preset=preset, **OVERRIDES.get(kind, {}))
            res = m.map([r[1] for r in reads])
            cuts = [len(reads) * k // N_BATCHES for k in range(N_BATCHES + 1)]
            batches = [Slice(pkg, reads, res, a, b) for a, b in zip(cuts, cuts[1:])]
            parts = [m.bam_batch_raw(*b.args()) for b in batches]
            header = m.bam_header(so.VERSION, ["x"], sort_order="coordinate")
            _mapped[kind] = (m, batches, parts, header, sr.sort_records(b"".join(parts)), res)
        return _mapped[kind][:5]
    yield get
    for v in _mapped.values():
        v[0].close()
    _mapped.clear()


def sort_file(pkg, m, batches, path, tmp_dir, **kw):
    os.makedirs(tmp_dir, exist_ok=True)
    s = pkg.BamSorter(path, m, tmp_dir=tmp_dir, version=so.VERSION, argv=["x"], **kw)
    for b in batches:
        s.add(*b.args())
    st = s.close()
    assert os.listdir(tmp_dir) == []  # the spools never had a name
    return open(path, "rb").read(), st


def plan_of(body, chunk_bytes):
    """the chunks of the sorted records: (number, whether a boundary falls between two records of one key)"""
    recs = sr.split(body)
    n, fill, inside = 1, 0, False
    for k, r in enumerate(recs):
        if fill and fill + len(r) > chunk_bytes:
            n, fill = n + 1, 0
            inside = inside or sr.key(recs[k - 1]) == sr.key(r)
        fill += len(r)
    return n, inside


def test_header_with_sort_order(mapped):
    m, _, _, header, _ = mapped("sr")
    plain = m.bam_header(so.VERSION, ["x"])
    text = b"@HD\tVN:1.6\tSO:coordinate\n"
    l_text = struct.unpack_from("<i", plain, 4)[0]
    assert header == plain[:4] + struct.pack("<i", l_text + len(text)) + text + plain[8:]
    assert m.bam_header(so.VERSION, ["x"]) == plain  # (gdiet_hip_bam_header itself does not change)


@pytest.mark.parametrize("route", ["device", "host"])
@pytest.mark.parametrize("kind", ["sr", "hifi_sv"])
def test_sorter_settings_give_one_file(kind, route, mapped, pkg, gpu_ctx, tmp_path):
    """run_bytes in {huge: one run, no spool; a quarter of the records: four runs} x chunk_bytes in {default; small: many chunks, on sr
    with a boundary inside the stretch of unplaced records}: the decompressed file is header + the restatement's sort of the records in
    input order, all settings give the same bytes, on the device route every member is Context.bgzf_deflate of its slice, the file ends
    with the end-of-file member, and the .bai is the restatement's over the written file"""
    m, batches, parts, header, body = mapped(kind)
    total = len(body)
    small_chunk = 4096 if kind == "sr" else 65536
    n_small, inside = plan_of(body, small_chunk)
    assert n_small >= 3 and (inside or kind != "sr") and len(sr.split(body)) > len(batches)
    assert kind == "sr" or sum(1 for r in sr.rows(body) if r[6] & 0x900) > 0  # secondary / supplementary records are in (sr maps to none)
    files = {}
    for run_bytes, chunk_bytes in ((1 << 29, 1 << 28), (1 << 29, small_chunk), (total // 4, 1 << 28), (total // 4, small_chunk)):
        path = str(tmp_path / ("%d_%d.bam" % (run_bytes, chunk_bytes)))
        raw, st = sort_file(pkg, m, batches, path, str(tmp_path / "spool"), bgzf=route, level=1, threads=2, run_bytes=run_bytes, chunk_bytes=chunk_bytes)
        stream = gzip.decompress(raw)
        assert len(stream) == len(header) + total and stream == header + body
        assert raw.endswith(EOF_MEMBER) and st["records"] == len(sr.split(body)) and st["members"] == len(sr.members(raw)) == (len(stream) + 65279) // 65280 + 1
        if run_bytes == 1 << 29:
            assert (st["runs"], st["spooled_bytes"], st["chunks"]) == (1, 0, 0)
        else:
            assert st["runs"] >= 3 and st["spooled_bytes"] == total and st["chunks"] == (1 if chunk_bytes == 1 << 28 else n_small)
        files[(run_bytes, chunk_bytes)] = raw
        bai = open(path + ".bai", "rb").read()
        assert bai == sr.bai(sr.rows(body), len(m.names), len(header), total, sr.members(raw))
        assert st["n_no_coor"] == sr.parse_bai(bai)[1] == sum(1 for r in sr.rows(body) if r[2] < 0)
    assert len(set(files.values())) == 1
    raw = next(iter(files.values()))
    if route == "device":
        assert raw == gpu_ctx.bgzf_deflate(header + body, eof=True)
    # region queries through the file: member offsets read from the file itself
    stream, log, index = header + body, sr.members(raw), sr.parse_bai(bai)
    rws = [r for r in sr.rows(body) if r[2] >= 0]
    n_hits = 0
    for ref in sorted({r[2] for r in rws}):
        mine = [r for r in rws if r[2] == ref]
        lo, hi = min(r[3] for r in mine), max(r[4] for r in mine)
        regions = [(ref, 0, hi + 1), (ref, hi + 5, hi + 50000), (ref, mine[len(mine) // 2][3], mine[len(mine) // 2][3] + 1), (ref, hi - 1, hi), (ref, hi, hi + 1)]
        for k in range(max(lo >> 14, 1), min((hi >> 14) + 2, (lo >> 14) + 4)):
            regions += [(ref, 16384 * k - 1, 16384 * k), (ref, 16384 * k, 16384 * k + 1), (ref, 16384 * k - 1, 16384 * k + 1), (ref, 16384 * k + 1, 16384 * k + 2)]
        for ref, beg, end in regions:
            hits = sr.brute(stream, len(header), ref, beg, end)
            assert sr.query(index, stream, log, len(header), ref, beg, end) == hits, (ref, beg, end)
            n_hits += len(hits)
    assert n_hits > 20


# ---- edges -------------------------------------------------------------------------------------------------------------------------
def test_sorter_closed_with_no_batch(mapped, pkg, tmp_path):
    m, _, _, header, _ = mapped("sr")
    raw, st = sort_file(pkg, m, [], str(tmp_path / "none.bam"), str(tmp_path / "spool"))
    assert gzip.decompress(raw) == header and raw.endswith(EOF_MEMBER) and len(sr.members(raw)) == 2
    assert (st["records"], st["runs"], st["chunks"], st["n_no_coor"]) == (0, 0, 0, 0)
    assert open(str(tmp_path / "none.bam.bai"), "rb").read() == b"BAI\1" + struct.pack("<i", len(m.names)) + struct.pack("<ii", 0, 0) * len(m.names) + struct.pack("<Q", 0)


def test_only_unmapped_reads(mapped, pkg, tmp_path):
    m, _, _, header, _ = mapped("sr")
    reads = [("u%d" % k, "ACGTN" * (1 + k), "IIIII" * (1 + k)) for k in range(7)]
    n = len(reads)
    none = types.SimpleNamespace(n_regs=(C.c_int32 * n)(), regs=(C.POINTER(pkg.map_api.Reg) * n)())
    path = str(tmp_path / "un.bam")
    os.makedirs(str(tmp_path / "spool"))
    with pkg.BamSorter(path, m, tmp_dir=str(tmp_path / "spool"), version=so.VERSION, argv=["x"]) as s:
        s.add_reads(none, reads)
        st = s.close()
    stream = gzip.decompress(open(path, "rb").read())
    assert [l.split("\t")[0] for l in bam_ref.bam_to_sam(stream)[-n:]] == [r[0] for r in reads]  # equal keys: input order
    index = sr.parse_bai(open(path + ".bai", "rb").read())
    assert st["n_no_coor"] == index[1] == n and all(not bins and pseudo is None and not lin for bins, pseudo, lin in index[0])


def test_one_batch_larger_than_run_bytes(mapped, pkg, tmp_path):
    m, batches, parts, header, body = mapped("sr")
    assert min(len(p) for p in parts) > 1000
    raw, st = sort_file(pkg, m, batches, str(tmp_path / "big.bam"), str(tmp_path / "spool"), run_bytes=1000, chunk_bytes=1 << 20)
    assert gzip.decompress(raw) == header + body and st["runs"] == len(batches) and st["chunks"] == 1 and st["spooled_bytes"] == len(body)


def test_a_tmp_dir_that_does_not_exist(mapped, pkg, tmp_path):
    """gdiet_hip_bam_sort_open: GDIET_E_PARAM naming the directory, and a handle that takes nothing but its close, which succeeds"""
    m, batches, _, header, body = mapped("sr")
    missing, out = str(tmp_path / "no_such_dir"), str(tmp_path / "x.bam")
    with pytest.raises(pkg.GdietError, match=r"error -3: .*no_such_dir"):
        pkg.BamSorter(out, m, tmp_dir=missing)
    probe = pkg.BamSorter(str(tmp_path / "probe.bam"), m, tmp_dir=str(tmp_path))  # (sets the argument types)
    probe.close()
    lib, h = probe.lib, C.c_void_p()
    rc = lib.gdiet_hip_bam_sort_open(m.ctx._h, out.encode(), header, len(header), 1, -1, 4, 0, 0, missing.encode(), 1, C.byref(h))
    assert rc == -3 and h.value and b"no_such_dir" in lib.gdiet_hip_strerror(m.ctx._h)  # GDIET_E_PARAM
    b = batches[0]
    cpp = C.POINTER(C.c_char_p)
    assert lib.gdiet_hip_bam_sort_add(h, m._idx, b.n, C.cast(b.names, cpp), C.cast(b.seqs, cpp), C.cast(b.quals, cpp), None, b.lens_p, b.res.n_regs, b.res.regs, m.opt.flag) == -3
    assert lib.gdiet_hip_bam_sort_close(h, None) == 0
    assert not os.path.exists(out) and not os.path.exists(out + ".bai")
    raw, _ = sort_file(pkg, m, batches[:2], out, str(tmp_path / "spool"))  # the context sorts on
    assert len(gzip.decompress(raw)) > len(header)


@pytest.mark.parametrize("route", ["device", "host"])
def test_a_file_whose_last_record_is_placed(route, mapped, pkg, tmp_path):
    """--sam-hit-only drops the unmapped reads, so the file ends in a placed record: the last chunk and the pseudo-bin of the last
    reference end at the virtual offset where the end-of-file member starts; one run and several"""
    m, batches, _, header, _ = mapped("sr")
    old = m.opt.flag
    m.opt.flag = old | so.F_SAM_HIT_ONLY
    try:
        parts = [m.bam_batch_raw(*b.args()) for b in batches]
        body = sr.sort_records(b"".join(parts))
        rws = sr.rows(body)
        assert len(rws) > 1000 and all(r[2] >= 0 for r in rws)
        for run_bytes in (1 << 29, len(body) // 4):
            path = str(tmp_path / ("placed_%d.bam" % run_bytes))
            raw, st = sort_file(pkg, m, batches, path, str(tmp_path / "spool"), bgzf=route, level=1, threads=2, run_bytes=run_bytes, chunk_bytes=65536)
            assert gzip.decompress(raw) == header + body and st["n_no_coor"] == 0
            bai = open(path + ".bai", "rb").read()
            assert bai == sr.bai(rws, len(m.names), len(header), len(body), sr.members(raw))
            last_ref = sr.parse_bai(bai)[0][rws[-1][2]]
            assert last_ref[1][0][1] == (len(raw) - 28) << 16
    finally:
        m.opt.flag = old


# ---- the tool ----------------------------------------------------------------------------------------------------------------------
def test_map_file_sort_index(tmp_path):
    """tools/map_file.py --bam --sort --index from file to file on sr, both compressors, against the same tool without --sort: the sorted
    file's records are the restatement's sort of the unsorted file's, its header gains the @HD line, its .bai is the restatement's"""
    fq = str(tmp_path / "reads.fq")
    write_fastq("sr", fq)
    base = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "map_file.py"), "--preset", "sr", os.path.join(SETS["sr"][0], "ref.fa.gz"), fq, "--bam"]

    def run(extra, out):
        r = subprocess.run(base + extra + ["-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads(r.stdout.strip().split("\n")[-1]), open(out, "rb").read()

    def split_stream(stream):
        l_text = struct.unpack_from("<i", stream, 4)[0]
        at = 8 + l_text
        n_ref = struct.unpack_from("<i", stream, at)[0]
        at += 4
        for _ in range(n_ref):
            at += 8 + struct.unpack_from("<i", stream, at)[0]
        return stream[8:8 + l_text].decode(), n_ref, at

    rep, plain = run([], str(tmp_path / "plain.bam"))
    assert "bam_sort" not in rep and rep["bam"] is True
    p_stream = gzip.decompress(plain)
    # without --sort the file is what test_bam_gpu.test_map_file_bam pins: the --header SAM output of the same configuration, line for line
    r = subprocess.run([a for a in base if a != "--bam"] + ["--header", "-o", str(tmp_path / "plain.sam")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    want_lines, got_lines = open(str(tmp_path / "plain.sam")).read().split("\n")[:-1], bam_ref.bam_to_sam(p_stream)
    assert len(got_lines) == len(want_lines)
    assert all(g.startswith("@PG\tID:minimap2") and "--bam" in g if w.startswith("@PG") else g == bam_ref.normal(w) for g, w in zip(got_lines, want_lines))
    p_text, n_ref, p_at = split_stream(p_stream)
    assert not p_text.startswith("@HD")
    want = sr.sort_records(p_stream[p_at:])
    for route in ("device", "host"):
        out = str(tmp_path / (route + ".bam"))
        rep, raw = run(["--sort", "--index", "--bgzf", route, "--tmp-dir", str(tmp_path)], out)
        stream = gzip.decompress(raw)
        text, n_ref2, at = split_stream(stream)
        assert text.startswith("@HD\tVN:1.6\tSO:coordinate\n@SQ") and n_ref2 == n_ref and stream[at:] == want and raw.endswith(EOF_MEMBER)
        assert [l for l in text.split("\n")[1:] if not l.startswith("@PG")] == [l for l in p_text.split("\n") if not l.startswith("@PG")]
        assert rep["bam_sort"]["records"] == len(sr.split(want)) and rep["bam_sort"]["route"] == route and rep["bam_sort"]["runs"] == 1
        assert open(out + ".bai", "rb").read() == sr.bai(sr.rows(want), n_ref, at, len(want), sr.members(raw))
    assert sorted(os.listdir(str(tmp_path))) == sorted(["reads.fq", "plain.bam", "plain.sam", "device.bam", "device.bam.bai", "host.bam", "host.bam.bai"])

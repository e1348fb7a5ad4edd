"""CPU: coordinate-sorted BAM and its BAI index.  The oracle is tests/bam_sort_ref.py, an independent restatement of the section "Sorted BAM
output" of include/gdiet_hip.h.  tests/emul/bam_sort_emul.cpp runs the statements of the sort kernels (bam_sort.h), the merge plan
(bam_sorter.h: gdq_plan_chunks) and the index builder (bam_index.h: gdx_bai_build) as a stand-alone program under AddressSanitizer /
UBSan on exact-size buffers, every gather with the lanes running 0..63 and 63..0 and at every alignment of the destination.
  * one pass: sorted bytes and index rows are the restatement's, on the goldens sr / hifi_sv / ont_sv as shuffled records and on hand-built
    records at the edges of the key, of the sizes and of the CIGAR field;
  * the merge: runs of several sizes and chunks of 1 byte, 4096 bytes and without bound give the same bytes and rows, the chunks
    concatenate to the global order, and every chunk takes one contiguous range of every run;
  * the sorter (GdqSorter) over an executor that runs these loops in host memory: runs, unnamed spools, the merge, both routes of the
    stream into the BGZF writer, the member log and the .bai, and what it refuses;
  * the index: its bytes are the restatement's for the member logs of a zlib and of a stored compression of the stream, and a BAI reader
    finds through it exactly the records an overlap scan finds."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_ref
import bam_sort_inputs as si
import bam_sort_ref as sr
from conftest import ROOT

ROW = np.dtype([("key", "<u8"), ("out", "<u8"), ("refID", "<i4"), ("pos", "<i4"), ("end", "<i4"), ("bin", "<u2"), ("flag", "<u2")])
INF = 1 << 62


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bam_sort") / "bam_sort_emul")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "genome-on-diet_amd", "csrc"), os.path.join(ROOT, "tests", "emul", "bam_sort_emul.cpp"), "-o", exe, "-lz", "-pthread"])
    return exe


def rows_of(path):
    return [tuple(int(x) for x in r) for r in np.fromfile(path, ROW)]


def run(emul, args, status=0):
    r = subprocess.run([emul] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == status, (r.returncode, r.stderr[-2000:])
    return r.stdout if status == 0 else r.stderr


def emul_sort(emul, data, tmp_path):
    p = [str(tmp_path / n) for n in ("in.recs", "out.recs", "out.rows")]
    open(p[0], "wb").write(data)
    run(emul, ["sort"] + p)
    return open(p[1], "rb").read(), rows_of(p[2])


def emul_merge(emul, data, per_run, chunk_bytes, tmp_path):
    """(sorted bytes, rows, plan): plan = [(j0, j1, bytes, [(lo, hi, byte_lo, byte_hi) per run])]"""
    p = [str(tmp_path / n) for n in ("in.recs", "m.recs", "m.rows")]
    open(p[0], "wb").write(data)
    text = run(emul, ["merge", p[0], per_run, chunk_bytes, p[1], p[2]])
    plan = []
    for l in text.split("\n")[:-1]:
        f = l.split()
        if f[0] == "CHUNK":
            plan.append((int(f[1]), int(f[2]), int(f[3]), []))
        else:
            assert f[0] == "RUN" and int(f[1]) == len(plan[-1][3])
            plan[-1][3].append(tuple(int(x) for x in f[2:]))
    return open(p[1], "rb").read(), rows_of(p[2]), plan


def emul_bai(emul, rows, n_ref, base, records_len, log, tmp_path):
    p = [str(tmp_path / n) for n in ("b.rows", "b.log", "b.bai")]
    np.array(rows, ROW).tofile(p[0]) if rows else open(p[0], "wb").close()
    open(p[1], "w").write("".join("%d %d\n" % m for m in log))
    n_no_coor = int(run(emul, ["bai", p[0], n_ref, base, records_len, p[1], p[2]]))
    return open(p[2], "rb").read(), n_no_coor


def inputs(kind):
    if kind == "hand":
        return si.hand_built(), si.REFS
    return si.golden_records(kind)


KINDS = ("hand", "sr", "hifi_sv", "ont_sv")


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------
def test_key_order_of_the_hand_built_records():
    got = [bam_ref.bam_to_sam(r, si.REFS)[0].split("\t")[0] for r in sr.split(sr.sort_records(b"".join(si.key_cases())))]
    assert got == ["c1_posm1", "c1_first", "c1_fwd", "equal_1", "equal_2", "equal_3", "c1_rev", "c1_unmapped_placed", "c2_x", "c2_y", "c3_early", "c3_late", "unplaced_a", "unplaced_b"]
    assert sr.key(si.key_cases()[0]) == 0xffffffff << 32 and sr.key(si.key_cases()[2]) == 100 << 1 | 1
    placeholder = si.cigar_cases()[-1]
    assert bam_ref.bam_to_sam(placeholder, si.REFS)[0].split("\t")[5] == "5S40000N" and sr.rows(placeholder)[0][4] == 32768 + 40000
    assert [sr.ref_len(r) for r in si.cigar_cases()[:2]] == [0, 30]


# ---- one pass ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_one_pass_sorts_like_the_restatement(kind, emul, tmp_path):
    recs, _ = inputs(kind)
    data = b"".join(recs)
    want = sr.sort_records(data)
    assert want != data and sorted(recs) == sorted(sr.split(want))
    got, rows = emul_sort(emul, data, tmp_path)
    assert got == want
    assert rows == sr.rows(want)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257])
def test_record_counts(n, emul, tmp_path):
    data = b"".join(si.counted(n))
    got, rows = emul_sort(emul, data, tmp_path)
    assert got == sr.sort_records(data) and rows == sr.rows(got) and len(rows) == n


def test_a_truncated_buffer_is_refused(emul, tmp_path):
    data = b"".join(si.key_cases())
    p = str(tmp_path / "bad.recs")
    open(p, "wb").write(data[:-1])
    assert "ends inside a record" in run(emul, ["sort", p, str(tmp_path / "o"), str(tmp_path / "r")], status=3)


# ---- the merge ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_bytes", [1, 4096, INF])
@pytest.mark.parametrize("kind,per_run", [("hand", 7), ("hand", 1000), ("sr", 700), ("hifi_sv", 40), ("ont_sv", 30)])
def test_merge_of_runs_is_the_one_pass_sort(kind, per_run, chunk_bytes, emul, tmp_path):
    recs, _ = inputs(kind)
    data = b"".join(recs)
    want = sr.sort_records(data)
    got, rows, plan = emul_merge(emul, data, per_run, chunk_bytes, tmp_path)
    assert got == want and rows == sr.rows(want)
    n_runs = (len(recs) + per_run - 1) // per_run
    sizes = [len(r) for r in sr.split(want)]
    # the chunks concatenate to the global order, each the longest prefix that fits (one record at least), one contiguous range per run
    at, nxt = 0, [(0, 0)] * n_runs
    for j0, j1, nbytes, runs in plan:
        assert j0 == at and j1 > j0 and nbytes == sum(sizes[j0:j1]) and len(runs) == n_runs
        assert nbytes <= chunk_bytes or j1 == j0 + 1
        assert j1 == len(sizes) or nbytes + sizes[j1] > chunk_bytes
        for r, (lo, hi, blo, bhi) in enumerate(runs):
            assert (lo, blo) == nxt[r] and hi >= lo and bhi >= blo
            nxt[r] = (hi, bhi)
        assert sum(hi - lo for lo, hi, _, _ in runs) == j1 - j0 and sum(bhi - blo for _, _, blo, bhi in runs) == nbytes
        at = j1
    assert at == len(sizes) and [hi for hi, _ in nxt] == [min(per_run, len(recs) - r * per_run) for r in range(n_runs)]
    if chunk_bytes == 1:
        assert len(plan) == len(recs)
    if chunk_bytes == INF:
        assert len(plan) == 1


def test_a_chunk_boundary_inside_a_stretch_of_equal_keys(emul, tmp_path):
    """twelve records of one key in three runs, chunks of two records: input order is kept across runs and chunks"""
    recs = [bam_ref.encode_record(si.line("r%02d" % k, 0, "c1", 100, "4M", "ACGT", "IIII"), si.REFS) for k in range(12)]
    data = b"".join(recs)
    got, rows, plan = emul_merge(emul, data, 5, 2 * len(recs[0]), tmp_path)
    assert got == data and len(plan) == 6 and len({r[0] for r in rows}) == 1


# ---- the index ---------------------------------------------------------------------------------------------------------------------
def regions_of(kind, names, stream, base):
    if kind == "hand":
        return si.REGIONS
    out = []
    rws = [r for r in sr.rows(stream[base:]) if r[2] >= 0]
    for ref in range(len(names)):
        mine = [r for r in rws if r[2] == ref]
        if not mine:
            continue
        lo, hi = min(r[3] for r in mine), max(r[4] for r in mine)
        out += [(ref, 0, hi + 1), (ref, hi + 5, hi + 50000), (ref, mine[len(mine) // 2][3], mine[len(mine) // 2][3] + 1), (ref, mine[-1][4] - 1, mine[-1][4]), (ref, mine[-1][4], mine[-1][4] + 1)]
        for k in range(max(lo >> 14, 1), min((hi >> 14) + 2, (lo >> 14) + 4)):
            out += [(ref, 16384 * k - 1, 16384 * k), (ref, 16384 * k, 16384 * k + 1), (ref, 16384 * k - 1, 16384 * k + 1), (ref, 16384 * k + 1, 16384 * k + 2)]
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_index_bytes_and_region_queries(kind, emul, tmp_path):
    recs, names = inputs(kind)
    header = bam_ref.bam_header("@HD\tVN:1.6\tSO:coordinate\n", [(n, 1 << 28) for n in names])
    body = sr.sort_records(b"".join(recs))
    stream, base = header + body, len(header)
    _, rows = emul_sort(emul, body, tmp_path)
    n_hits = 0
    for log in (sr.zlib_members(stream), sr.stored_members(stream)):
        want = sr.bai(sr.rows(body), len(names), base, len(body), log)
        got, n_no_coor = emul_bai(emul, rows, len(names), base, len(body), log, tmp_path)
        assert got == want
        index = sr.parse_bai(got)
        assert index[1] == n_no_coor == sum(1 for r in rows if r[2] < 0)
        for ref, beg, end in regions_of(kind, names, stream, base):
            hits = sr.brute(stream, base, ref, beg, end)
            assert sr.query(index, stream, log, base, ref, beg, end) == hits, (ref, beg, end)
            n_hits += len(hits)
        for ref, (bins, pseudo, lin) in enumerate(index[0]):
            mine = [r for r in rows if r[2] == ref]
            assert (pseudo is None) == (not mine) and (not mine or pseudo[1] == (sum(1 for r in mine if not r[6] & 4), sum(1 for r in mine if r[6] & 4)))
            assert list(bins) == sorted(bins)
    assert n_hits > 20
    if kind == "hand":  # an empty stretch, and the placeholder's 40000N found at its far end
        assert not sr.brute(stream, base, 0, 200000, 300000) and len(sr.brute(stream, base, 0, 72767, 72768)) == 1 and not sr.brute(stream, base, 0, 72768, 72769)


def placed_only(kind):
    recs, names = inputs(kind)
    return [r for r in recs if sr.fields(r)[0] >= 0], names


@pytest.mark.parametrize("kind", ["hand", "sr"])
def test_index_of_a_file_whose_last_record_is_placed(kind, emul, tmp_path):
    """no unplaced record behind the last reference: the last chunk and the pseudo-bin end where the stream ends, which is the file
    offset at which the end-of-file member STARTS (the member itself holds no offset), byte for byte for both member logs"""
    recs, names = placed_only(kind)
    header = bam_ref.bam_header("@HD\tVN:1.6\tSO:coordinate\n", [(n, 1 << 28) for n in names])
    body = sr.sort_records(b"".join(recs))
    assert sr.rows(body)[-1][2] >= 0
    _, rows = emul_sort(emul, body, tmp_path)
    for log in (sr.zlib_members(header + body), sr.stored_members(header + body), [(len(header) + len(body), 346), (0, 28)]):
        want = sr.bai(sr.rows(body), len(names), len(header), len(body), log)
        got, n_no_coor = emul_bai(emul, rows, len(names), len(header), len(body), log, tmp_path)
        assert got == want and n_no_coor == 0
        data_end = sum(f for _, f in log) - 28
        last = max(k for k, (bins, pseudo, lin) in enumerate(sr.parse_bai(got)[0]) if pseudo)
        bins, pseudo, _ = sr.parse_bai(got)[0][last]
        assert pseudo[0][1] == data_end << 16 == max(c[1] for ch in bins.values() for c in ch)


def test_index_of_no_record_and_of_unplaced_records_only(emul, tmp_path):
    header = bam_ref.bam_header("@HD\tVN:1.6\tSO:coordinate\n", list(zip(si.REFS, si.REF_LENS)))
    got, n = emul_bai(emul, [], 3, len(header), 0, sr.stored_members(header), tmp_path)
    assert got == b"BAI\1" + struct.pack("<i", 3) + struct.pack("<ii", 0, 0) * 3 + struct.pack("<Q", 0) == sr.bai([], 3, len(header), 0, sr.stored_members(header)) and n == 0
    body = b"".join(bam_ref.encode_record(si.line("u%d" % k, 4, "*", 0, "*", "ACGT", "IIII"), si.REFS) for k in range(5))
    log = sr.zlib_members(header + body)
    got, n = emul_bai(emul, sr.rows(body), 3, len(header), len(body), log, tmp_path)
    assert n == 5 and got == sr.bai(sr.rows(body), 3, len(header), len(body), log) and got[-8:] == struct.pack("<Q", 5) and len(got) == 8 + 24 + 8


def test_virtual_offsets_at_member_edges():
    log = [(65280, 100), (65280, 200), (10, 40), (0, 28)]
    assert sr.voffset(log, 0) == 0 and sr.voffset(log, 65279) == 65279 and sr.voffset(log, 65280) == 100 << 16
    assert sr.voffset(log, 2 * 65280 + 9) == 300 << 16 | 9 and sr.voffset(log, 2 * 65280 + 10) == 340 << 16
    assert [sr.stream_offset(log, sr.voffset(log, x)) for x in (0, 1, 65280, 130569, 130570)] == [0, 1, 65280, 130569, 130570]


# ---- the sorter over the host executor -----------------------------------------------------------------------------------------------
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def emul_sorter(emul, data, header, per_batch, run_bytes, chunk_bytes, device, tmp_path, status=0, tmp_dir=None):
    spool = tmp_dir or str(tmp_path / "spool")
    if tmp_dir is None:
        os.makedirs(spool, exist_ok=True)
    p = [str(tmp_path / n) for n in ("s.recs", "s.header", "s.bam")]
    open(p[0], "wb").write(data)
    open(p[1], "wb").write(header)
    for f in (p[2], p[2] + ".bai"):
        if os.path.exists(f):
            os.remove(f)
    text = run(emul, ["sorter", p[0], per_batch, run_bytes, chunk_bytes, spool, p[1], int(device), p[2]], status=status)
    if status:
        return text
    assert os.listdir(spool) == []
    st = dict(zip(("records", "runs", "spooled_bytes", "chunks", "members", "n_no_coor"), (int(x) for x in text.split())))
    return open(p[2], "rb").read(), open(p[2] + ".bai", "rb").read(), st


@pytest.mark.parametrize("device", [0, 1], ids=["host", "resident"])
@pytest.mark.parametrize("kind", ["hand", "sr", "hifi_sv", "sr_placed"])
def test_sorter_over_the_host_executor(kind, device, emul, tmp_path):
    recs, names = placed_only("sr") if kind == "sr_placed" else inputs(kind)  # (sr_placed: the file ends in a placed record)
    data = b"".join(recs)
    header = bam_ref.bam_header("@HD\tVN:1.6\tSO:coordinate\n", [(n, 1 << 28) for n in names])
    body = sr.sort_records(data)
    per_batch = max(1, len(recs) // 8)
    files = set()
    for run_bytes, chunk_bytes in ((1 << 29, 1 << 28), (len(data) // 4, 1 << 28), (len(data) // 4, 4096), (1, 1)):
        raw, bai, st = emul_sorter(emul, data, header, per_batch, run_bytes, chunk_bytes, device, tmp_path)
        assert gzip.decompress(raw) == header + body and raw.endswith(EOF_MEMBER)
        log = sr.members(raw)
        assert all(n_in == 65280 for n_in, _ in log[:-2]) and log[-1] == (0, 28) and st["members"] == len(log) and st["records"] == len(recs)
        assert bai == sr.bai(sr.rows(body), len(names), len(header), len(body), log)
        assert st["n_no_coor"] == sum(1 for r in sr.rows(body) if r[2] < 0)
        if run_bytes == 1 << 29:
            assert (st["runs"], st["spooled_bytes"], st["chunks"]) == (1, 0, 0)
        elif run_bytes == 1:  # every batch is larger than run_bytes: a run of its own; every record a chunk of its own
            assert (st["runs"], st["spooled_bytes"], st["chunks"]) == ((len(recs) + per_batch - 1) // per_batch, len(body), len(recs))
        else:
            assert st["runs"] >= 3 and st["spooled_bytes"] == len(body) and (st["chunks"] == 1 if chunk_bytes == 1 << 28 else st["chunks"] >= 3)
        files.add(raw)
    assert len(files) == 1  # a function of the input records alone


def test_sorter_edges(emul, tmp_path):
    header = bam_ref.bam_header("@HD\tVN:1.6\tSO:coordinate\n", list(zip(si.REFS, si.REF_LENS)))
    raw, bai, st = emul_sorter(emul, b"", header, 1, 0, 0, 0, tmp_path)
    assert gzip.decompress(raw) == header and len(sr.members(raw)) == 2 and st["runs"] == 0
    assert bai == b"BAI\1" + struct.pack("<i", 3) + struct.pack("<ii", 0, 0) * 3 + struct.pack("<Q", 0)
    data = b"".join(si.key_cases())
    assert "no_such_dir" in emul_sorter(emul, data, header, 3, 0, 0, 0, tmp_path, status=4, tmp_dir=str(tmp_path / "no_such_dir"))
    assert not os.path.exists(str(tmp_path / "s.bam")) and not os.path.exists(str(tmp_path / "s.bam.bai"))
    long_contig = bam_ref.bam_header("", [("fine", 1 << 29), ("giant", (1 << 29) + 1)])
    assert "giant" in emul_sorter(emul, data, long_contig, 3, 0, 0, 0, tmp_path, status=4)
    assert "no BAM header" in emul_sorter(emul, data, header[:-1], 3, 0, 0, 0, tmp_path, status=4)

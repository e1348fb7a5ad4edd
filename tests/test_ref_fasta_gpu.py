"""GPU: the reference input (csrc/ref_fasta*.h; gdiet_hip_index_open / _index_info / _index_open_stats / _ref_block).
  * the kernel-level boundary Context.ref_block against the host emulator (tests/emul/ref_fasta_emul.cpp, built here without
    sanitizers) on blocks around the tile edges, in each start state, with every disqualifying byte;
  * Mapper.from_file against Mapper(ctx, names, seqs) of the records the unattached FastxReader reads from the same file: export_index()
    array for array and dump_mmi byte for byte, for every input of tests/ref_fasta_inputs.py x block sizes {4 096, default} x {device
    route, GDIET_INDEX_BUILD=host}; the counters say who placed the bases, so that no case passes through the other route;
  * dump_mmi against the sha256 of `GDiet_avx -d` on the same file (tests/golden/reffile, tools/make_reffile_golden.py);
  * from_file on an .mmi that dump_mmi wrote, with other k / w in the arguments; tools/map_file.py with a FASTA and with -d and the .mmi.
tests/test_ref_fasta.py checks the same statements on the CPU."""
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import ref_fasta_inputs
from conftest import ROOT
from fixture_io import LR, SR, golden_sam, reads_of

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "reffile")
NONE = 0xffffffff
LS, HD, SQ = 0, 1, 2


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return ref_fasta_inputs.files(str(tmp_path_factory.mktemp("ref_inputs")))


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ref_fasta") / "ref_fasta_emul")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul", "ref_fasta_emul.cpp"), "-o", exe, "-lz"])
    return exe


@pytest.fixture(scope="module")
def host_ctx(pkg):
    """a context made under GDIET_INDEX_BUILD=host (the variable is read when a context is made)"""
    import torch  # noqa: F401
    old = os.environ.get("GDIET_INDEX_BUILD")
    os.environ["GDIET_INDEX_BUILD"] = "host"
    try:
        ctx = pkg.Context(0)
    finally:
        if old is None:
            del os.environ["GDIET_INDEX_BUILD"]
        else:
            os.environ["GDIET_INDEX_BUILD"] = old
    yield ctx
    ctx.close()


# ---- the kernel-level boundary ------------------------------------------------------------------------------------------------------
def block_cases():
    """[(label, text, state_in)]"""
    body = ref_fasta_inputs.contents()["odd_tiny_dup_longhdr.fa"] + b"\n" + ref_fasta_inputs.contents()["lr_w60_nl.fa"][:6000]
    seq = ref_fasta_inputs.contents()["lr_w0_nl.fa"][6:4000]  # one long line of bases, no newline
    assert b"\n" not in seq and b">" not in seq
    cases = []
    for n in (0, 1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049):  # sizes around the lane and tile edges
        for st in (LS, HD, SQ):
            cases.append(("size%d" % n, body[:n], st))
            cases.append(("size%d_mid" % n, body[37:37 + n], st))
    for st in (LS, HD, SQ):
        cases.append(("nl_last_of_tile", seq[:1023] + b"\n" + seq[:500], st))
        cases.append(("nl_first_of_next_tile", seq[:1024] + b"\n" + seq[:500], st))
        cases.append(("nl_both", seq[:1023] + b"\n\n>x\n" + seq[:500], st))
        cases.append(("no_newline_three_tiles", seq[:3000], st))
        cases.append(("tile_without_newline", seq[:900] + b"\n" + seq[:1500] + b"\n>h\n" + seq[:300], st))
        cases.append(("header_crosses_tile", seq[:1000] + b"\n>name " + b"c" * 100 + b"\n" + seq[:900], st))
        cases.append(("header_crosses_block", seq[:100] + b"\n>name " + b"c" * 50, st))
        cases.append(("header_runs_in", b"me comment\n" + seq[:100] + b"\n>second\n" + seq[:77], st))
        cases.append(("header_runs_through", b"no newline at all in this block", st))
        cases.append(("gt_is_last_byte", seq[:2047] + b"\n>", st))
        cases.append(("gt_inside_lines", b">a>b\nAC>GT\n>c\n", st))
        for bad in (b"\r", b"\n+", b"\n@"):
            cases.append(("bad%r_first_tile" % bad, seq[:10] + bad + seq[:2500] + b"\n", st))
            cases.append(("bad%r_last_tile" % bad, seq[:1000] + b"\n" + seq[:1400] + bad + seq[:5], st))
        for c in (b"+", b"@"):
            cases.append(("byte0_%r" % c, c + seq[:50] + b"\n", st))  # a line start only in state LS
            cases.append(("midline_%r" % c, seq[:20] + c + seq[:20] + b"\n" + seq[:5] + c + b"\n", st))  # never a line start: not disqualifying
    return cases


def test_ref_block_against_the_emulator(gpu_ctx, emul, tmp_path):
    cases = block_cases()
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for _, text, st in cases:
            f.write(struct.pack("<II", len(text), st) + text)
    r = subprocess.run([emul, "blocks", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    claimed = refused = 0
    for (label, text, st), line in zip(cases, lines):
        f = line.split(" ")
        assert f[0::2][:5] == ["claimed", "state", "run_nl", "bases", "rows"], line
        want = dict(claimed=int(f[1]), state_out=int(f[3]), run_nl=int(f[5]), nt4=[int(c, 16) for c in f[7]],
                    rows=[[int(x) for x in row.split(":")] for row in f[9].split(",")] if len(f) > 9 and f[9] else [])
        got = gpu_ctx.ref_block(text, st)
        assert got["claimed"] == want["claimed"] and got["state_out"] == want["state_out"] and got["run_nl"] == want["run_nl"], (label, st, got, want)
        assert got["nt4"].tolist() == want["nt4"], (label, st)
        assert got["rows"].tolist() == want["rows"], (label, st, got["rows"], want["rows"])
        # ... and against the text itself
        if label.startswith("bad") or (label.startswith("byte0") and st == LS):
            assert got["claimed"] == 0 and got["state_out"] == -1, (label, st)
            refused += 1
        else:
            assert got["claimed"] == len(text), (label, st)
            claimed += 1
            if text:
                assert got["state_out"] == (LS if text.endswith(b"\n") else got["state_out"]) and got["state_out"] in (HD, SQ, LS)
                for gt, nl, rank in got["rows"].tolist():
                    assert text[gt:gt + 1] == b">" and (st == LS if gt == 0 else text[gt - 1:gt] == b"\n") and (nl == NONE or text[nl:nl + 1] == b"\n")
    assert claimed > 100 and refused == 3 * 6 + 2


# ---- from_file against the sequences in memory --------------------------------------------------------------------------------------
def records_of(pkg, path):
    """names and sequences as the unattached reader returns them"""
    names, seqs = [], []
    with pkg.FastxReader(path) as r:
        while True:
            batch = r.read(1 << 28, with_qual=False)
            for name, seq, _, _ in batch:
                names.append(name.decode()), seqs.append(seq)
            if not batch and not r.truncated_now:
                return names, seqs


def by_key(f):
    """export_index() with the keys ascending: the export walks the table, and where colliding keys sit in it depends on which thread of
    the device build claimed its slot first (tests/fixture_io.py: flat_index orders them the same way)"""
    order = np.argsort(f["keys"], kind="stable")
    start = np.concatenate([[0], np.cumsum(f["cnt"].astype(np.int64))])
    pos = np.concatenate([f["pos"][start[j]:start[j + 1]] for j in order]) if len(order) else f["pos"]
    return dict(keys=f["keys"][order], cnt=f["cnt"][order], pos=pos, S=f["S"], offsets=f["offsets"])


_baseline = {}


def baseline(pkg, ctx, path, preset, tmp):
    """export_index() and the .mmi bytes of Mapper(ctx, names, seqs), once per distinct set of records"""
    names, seqs = records_of(pkg, path)
    key = (preset, hashlib.sha256(repr((names, seqs)).encode()).hexdigest())
    if key not in _baseline:
        if not names:
            _baseline[key] = None
        else:
            m = pkg.Mapper(ctx, names, seqs, preset=preset)
            try:
                mmi = os.path.join(tmp, "base.mmi")
                m.dump_mmi(mmi)
                with open(mmi, "rb") as f:
                    _baseline[key] = (names, [len(s) for s in seqs], by_key(m.export_index()), f.read())
            finally:
                m.close()
    return _baseline[key]


def groups():
    names = sorted(ref_fasta_inputs.contents())
    out = {}
    for n in names:
        g = ref_fasta_inputs.group(n)
        key = g if g != "canonical" else n.split("_")[0] + "." + n.rsplit(".", 1)[1]  # lr.fa, lr.gz, lr.bgz, sr.fa, ...
        out.setdefault(key, []).append(n)
    return out


@pytest.mark.parametrize("route", ["device", "host"])
@pytest.mark.parametrize("grp", sorted(groups()))
def test_from_file_builds_the_index_of_the_records(grp, route, gpu_ctx, host_ctx, pkg, inputs, tmp_path, monkeypatch):
    ctx = gpu_ctx if route == "device" else host_ctx
    preset = "sr" if grp.startswith("sr") else "hifi"
    tmp = str(tmp_path)
    for name in groups()[grp]:
        want = baseline(pkg, gpu_ctx, inputs[name], preset, tmp)
        for block in (4096, None):
            if block is None:
                monkeypatch.delenv("GDIET_FASTX_BLOCK", raising=False)
            else:
                monkeypatch.setenv("GDIET_FASTX_BLOCK", str(block))
            if want is None:  # no record: what gdiet_hip_index_build does with n_seq = 0
                with pytest.raises(pkg.GdietError):
                    pkg.Mapper(ctx, [], [], preset=preset)
                with pytest.raises(pkg.GdietError):
                    pkg.Mapper.from_file(ctx, inputs[name], preset=preset)
                continue
            names, lens, flat, mmi_bytes = want
            m = pkg.Mapper.from_file(ctx, inputs[name], preset=preset)
            try:
                assert m.names == names and m.lens.tolist() == lens, (name, block)
                got = by_key(m.export_index())
                for k in ("keys", "cnt", "pos", "S", "offsets"):
                    assert np.array_equal(got[k], flat[k]), (name, block, k)
                mmi = os.path.join(tmp, "got.mmi")
                m.dump_mmi(mmi)
                with open(mmi, "rb") as f:
                    assert f.read() == mmi_bytes, (name, block)
                st = m.open_stats()
                total = sum(lens)
                assert st["file_bytes"] == os.path.getsize(inputs[name]) and st["blocks"] >= 1, (name, st)
                if route == "host":
                    assert st["bases_device"] == 0 and st["blocks_host"] == st["blocks"] and st["bases_host"] == total, (name, block, st)
                elif ref_fasta_inputs.group(name) == "awkward":
                    assert st["blocks_host"] >= 1 and st["bases_host"] > 0, (name, block, st)
                else:  # canonical and odd files: every block is the device's
                    assert st["blocks_host"] == 0 and st["bases_host"] == 0 and st["bases_device"] == total, (name, block, st)
                    assert st["text_bytes"] == len(ref_fasta_inputs.contents()[name.rsplit(".", 1)[0] if name.endswith(("gz", "bgz")) else name]), (name, st)
                    assert st["device_peak_bytes"] >= total
            finally:
                m.close()


def test_small_blocks_go_back_to_the_device(gpu_ctx, pkg, inputs, monkeypatch):
    monkeypatch.setenv("GDIET_FASTX_BLOCK", "256")
    for name in ("awk_plus_at.fa", "awk_junk_front.fa"):
        m = pkg.Mapper.from_file(gpu_ctx, inputs[name])
        try:
            st = m.open_stats()
            assert 0 < st["blocks_host"] < st["blocks"] and st["bases_device"] > st["bases_host"] > 0, (name, st)
        finally:
            m.close()


def test_a_file_that_cannot_be_opened_is_named(gpu_ctx, pkg, tmp_path):
    missing = str(tmp_path / "no_such_reference.fa")
    with pytest.raises(pkg.GdietError, match="no_such_reference.fa"):
        pkg.Mapper.from_file(gpu_ctx, missing)
    with pytest.raises(pkg.GdietError, match="k must be in"):
        pkg.Mapper.from_file(gpu_ctx, os.path.join(LR, "ref.fa.gz"), k=29)


# ---- against the reference ----------------------------------------------------------------------------------------------------------
def test_device_route_mmi_is_the_reference_s(gpu_ctx, pkg, inputs, tmp_path):
    with open(os.path.join(GOLDEN, "mmi.sha256.json")) as f:
        g = json.load(f)
    assert len(g["files"]) >= 8
    for name, row in sorted(g["files"].items()):
        for preset, want in sorted(row["mmi_sha256"].items()):
            m = pkg.Mapper.from_file(gpu_ctx, inputs[name], preset=preset)
            try:
                out = str(tmp_path / "out.mmi")
                m.dump_mmi(out)
                with open(out, "rb") as f:
                    got = hashlib.sha256(f.read()).hexdigest()
                assert (got == want) == (name not in g["findings"]), (name, preset)
                assert m.open_stats()["bases_device" if ref_fasta_inputs.group(name) != "awkward" else "bases_host"] > 0
            finally:
                m.close()


# ---- .mmi by magic ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,base", [("hifi", LR), ("sr", SR)])
def test_mmi_round_trip_with_other_k_and_w_in_the_arguments(kind, base, gpu_ctx, pkg, tmp_path):
    path = str(tmp_path / "reference.fasta")  # (an index file is known by its magic, not by its name)
    m = pkg.Mapper.from_file(gpu_ctx, os.path.join(base, "ref.fa.gz"), preset=kind)
    try:
        info = m.index_info()
        m.dump_mmi(path)
    finally:
        m.close()
    reads = reads_of(kind)
    m = pkg.Mapper.from_file(gpu_ctx, path, preset=kind, k=info["k"] - 4, w=info["w"] + 3)
    try:
        got = m.index_info()
        assert (got["k"], got["w"], got["names"], got["lens"].tolist()) == (info["k"], info["w"], info["names"], info["lens"].tolist())
        assert m.names == info["names"] and m.open_stats()["file_bytes"] == os.path.getsize(path)
        res = m.map([r[1] for r in reads])
        assert m.sam_batch(res, reads) == "".join(l + "\n" for l in golden_sam(kind))
    finally:
        m.close()


def test_index_info_of_an_index_built_from_memory(gpu_ctx, pkg):
    m = pkg.Mapper(gpu_ctx, ["a", "b b", ""], ["ACGTACGTACGTACGTACGTAGCATCGACTAGCTACGACTAGC", "", "GGGTTTAAACCC"], preset="sr")
    try:
        info = m.index_info()
        assert (info["k"], info["w"], info["names"], info["lens"].tolist()) == (21, 11, ["a", "b b", ""], [43, 0, 12])
        assert m.open_stats()["blocks"] == 0
    finally:
        m.close()


# ---- the tool -----------------------------------------------------------------------------------------------------------------------
def test_map_file_with_a_fasta_and_with_the_mmi_it_dumped(tmp_path):
    fq, mmi = os.path.join(SR, "sr.fq.gz"), str(tmp_path / "ref.idx")
    want = "".join(l + "\n" for l in golden_sam("sr"))
    base = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "map_file.py"), "--preset", "sr"]
    for ref, extra in ((os.path.join(SR, "ref.fa.gz"), ["-d", mmi]), (mmi, [])):
        out = str(tmp_path / "out.sam")
        r = subprocess.run(base + extra + [ref, fq, "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        rep = json.loads(r.stdout.strip().split("\n")[-1])
        assert rep["reads"] == 2000 and rep["ref_open"]["file_bytes"] == os.path.getsize(ref)
        assert (rep["ref_open"]["bases_device"] > 0) == (ref != mmi)
        with open(out) as f:
            assert f.read() == want, ref
    with open(mmi, "rb") as f:
        assert f.read(4) == b"MMI\x02"

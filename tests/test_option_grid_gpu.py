"""The mapping kernels (seeding, voting, ShortReads boxes, post-processing, device index build) away from the README command lines:
every row of the option grid (tests/golden/opts/grid.json -- multi-1 / long / full-density patterns, k = 28 and k <= 12, w = 1, 8, 9, 64,
vote capacities up to the cap, gap / band / -i / -N options, --for-only / --rev-only, non-preset scorings) against what THE REFERENCE
printed for it (oracle/make_grid_golden.py): the SAM records through gdiet_hip_map_batch (B1) and the pattern phase and seed hits through
gdiet_hip_seed_batch (B4).  Rows tagged for a stage run it under both of its implementations."""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

from fixture_io import (OPTS, assert_seed_batch_matches_trace, flat_index, grid_golden_sam, grid_ids, grid_mapper_args, grid_reads, grid_row, grid_rows, grid_trace, read_fasta,
                        seed_trace_per_read, star_seq_qual)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _mapper(pkg, ctx, row):
    base, preset, ov = grid_mapper_args(row)
    names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
    return pkg.Mapper(ctx, names, seqs, preset=preset, **ov), names, seqs


def _check_sam(m, row):
    reads = grid_reads(row)
    assert len(reads) == row["n_reads"]
    got = [star_seq_qual(l) for l in m.sam_batch(m.map([r[1] for r in reads]), reads).rstrip("\n").split("\n")]
    want = grid_golden_sam(row)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a == b, (a[:300], b[:300])


def _check_seeds(m, names, row):
    reads = grid_reads(row)
    want = seed_trace_per_read(grid_trace(row))
    assert len(want) == len(reads)
    n_sd = assert_seed_batch_matches_trace(m.seed_batch([r[1] for r in reads]), want, names, True, flag=row["overrides"].get("flag", 0))
    assert n_sd > 100


@pytest.mark.parametrize("name", grid_ids())
def test_grid_map_batch_matches_the_reference_sam(gpu_ctx, pkg, name):
    """B1: Mapper.map + sam_batch == the row's golden SAM, byte for byte (SEQ and QUAL, echoes of the input, starred on both sides)"""
    row = grid_row(name)
    m, _, _ = _mapper(pkg, gpu_ctx, row)
    try:
        before = m.scratch_retries()
        _check_sam(m, row)
        if "retry" in row["tags"]:  # the dense pattern at w = 1 overflows the first per-read scratch estimate: the batch ran twice
            assert m.scratch_retries() > before
    finally:
        m.close()


@pytest.mark.parametrize("name", grid_ids())
def test_grid_seed_batch_matches_the_reference_trace(gpu_ctx, pkg, name):
    """B4: pattern phase, hit counts and seed hits of both strands of every read == the row's --print-seeds trace"""
    row = grid_row(name)
    m, names, _ = _mapper(pkg, gpu_ctx, row)
    try:
        _check_seeds(m, names, row)
    finally:
        m.close()


@pytest.mark.parametrize("seed_kernel", ["wave", "thread"])
@pytest.mark.parametrize("name", grid_ids("kw"))
def test_grid_pattern_rows_through_both_seed_executors(pkg, name, seed_kernel, monkeypatch):
    """every pattern / k / w row through the wavefront-per-read executor (gd_sketch_range's EXT_WIN form: aligned 8-byte loads, LDS
    windows, per-lane slices that start mid-read) and the thread-per-read one (plain form, with the thread vote kernel): both give the
    reference's seeds and SAM"""
    import torch  # noqa: F401
    monkeypatch.setenv("GDIET_SEED_KERNEL", seed_kernel)
    if seed_kernel == "thread":
        monkeypatch.setenv("GDIET_VOTE_WAVE", "0")
    row = grid_row(name)
    ctx = pkg.Context(0)  # the executor is chosen when the context is created
    try:
        m, names, _ = _mapper(pkg, ctx, row)
        try:
            _check_seeds(m, names, row)
            _check_sam(m, row)
        finally:
            m.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("name", grid_ids("kw"))
def test_grid_device_built_index_equals_host_built(pkg, name, monkeypatch):
    """gdiet_hip_index_build on the device against the host builder at every pattern / k / w row: same keys, counts, position lists, mid_occ"""
    import numpy as np
    import torch  # noqa: F401
    base, preset, ov = grid_mapper_args(grid_row(name))
    names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
    h, d = (flat_index(pkg, names, seqs, preset, ov, builder, monkeypatch) for builder in ("host", "device"))
    assert h[5] == d[5] > 1000 and h[4] == d[4]
    for a, b in zip(h[:4], d[:4]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", grid_ids("mmi"))
def test_grid_device_built_mmi_is_the_reference_s(gpu_ctx, pkg, tmp_path, name):
    """the index built on the device at a non-preset k / w / pattern, dumped: size and sha256 of the file `GDiet_avx -d` wrote"""
    want = json.load(open(os.path.join(OPTS, "mmi.sha256.json")))[name]
    m, _, _ = _mapper(pkg, gpu_ctx, grid_row(name))
    try:
        out = str(tmp_path / "built.mmi")
        m.dump_mmi(out)
        data = open(out, "rb").read()
        assert len(data) == want["size"] and hashlib.sha256(data).hexdigest() == want["sha256"]
    finally:
        m.close()


@pytest.mark.parametrize("env,tag", [({"GDIET_SR_BOXES": "host"}, "boxes"),  # ShortReads candidate geometry on host threads (the device form: the tests above)
                                     ({"GDIET_POST_WAVE": "0"}, "post"),       # mm_update_extra at other scorings: one thread per alignment ...
                                     ({"GDIET_POST_WAVE": "1"}, "post")])      # ... and one wavefront per alignment
def test_grid_rows_under_the_other_implementation_of_a_stage(env, tag):
    """the -r / AF_max_loc rows with the box stage on the host, the scoring rows through either post kernel (tests/grid_env_check.py, in
    a process of its own: the library reads these switches once)"""
    rows = grid_ids(tag)
    assert len(rows) >= 2
    r = subprocess.run([sys.executable, os.path.join(HERE, "grid_env_check.py")] + rows, capture_output=True, text=True, env=dict(os.environ, **env), timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_grid_limits_stay_refusals(gpu_ctx, pkg):
    """what the library does not take is refused with GDIET_E_PARAM (-3) and a message, not mapped with: a pattern of 64 positions, one
    without a 1, one with 41 ones, k = 29, w = 65 (index build); vt_nb_loc = 23, AF_max_loc = 25 (mapping: more candidates than a vote
    record holds)"""
    refused = re.compile(r"gdiet_hip error -3: \S")
    lr, sr = grid_row("lr_z110"), grid_row("sr_rep_af1_r3")
    base, preset, _ = grid_mapper_args(lr)
    names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
    for bad in (dict(Z="10" * 32, W=64), dict(Z="0000", W=4), dict(Z="1" * 41 + "0", W=42), dict(k=29), dict(w=65)):
        with pytest.raises(pkg.GdietError, match=refused):
            pkg.Mapper(gpu_ctx, names, seqs, preset=preset, **bad)
    for row, bad in ((lr, dict(vt_nb_loc=23)), (sr, dict(AF_max_loc=25))):
        base, preset, ov = grid_mapper_args(row)
        names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
        m = pkg.Mapper(gpu_ctx, names, seqs, preset=preset, **dict(ov, **bad))
        try:
            with pytest.raises(pkg.GdietError, match=refused):
                m.map([r[1] for r in grid_reads(row)[:4]])
        finally:
            m.close()
    assert len(grid_rows()) >= 20

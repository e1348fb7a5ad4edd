"""The mapping kernels (seeding, voting, ShortReads boxes, post-processing, device index build) away from the README command lines:
every row of the option grid (tests/golden/opts/grid.json -- multi-1 / long / full-density patterns, k = 28 and k <= 12, w = 1, 8, 9, 64,
vote capacities up to the cap, gap / band / -i / -N options, --for-only / --rev-only, non-preset scorings) against what THE REFERENCE
printed for it (oracle/make_grid_golden.py): the SAM records through gdiet_hip_map_batch (B1) and the pattern phase and seed hits through
gdiet_hip_seed_batch (B4).  Rows tagged for a stage run it under both of its implementations.  The scoring rows (tag "score": single
affine, the edge of the wave kernels' 120 bound, a = 16, e2 = 2 over Ns, scorings the wave kernels refuse) also report which DP kernels
ran, and go once more through every other route the library has for them: the generic kernel on the boxes the wave kernels took, the
pre-filter's diagonal shortcut off, no pipelines, groups of 16 lanes, the narrow band and the quarter rung off and on, submit / wait."""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

from fixture_io import (OPTS, assert_seed_batch_matches_trace, flat_index, grid_golden_sam, grid_ids, grid_mapper_args, grid_reads, grid_row, grid_rows, grid_trace,
                        grid_wave_scoring_ok, read_fasta, seed_trace_per_read, star_seq_qual)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _mapper(pkg, ctx, row):
    base, preset, ov = grid_mapper_args(row)
    names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
    return pkg.Mapper(ctx, names, seqs, preset=preset, **ov), names, seqs


WAVE_BITS = 1 | 4 | 8 | 16  # GdPlan::mask: 1 64-lane, 2 generic, 4 short-alignment, 8 wide-band, 16 pipelines


def _check_sam(m, row, ctx=None):
    """the row mapped synchronously == its golden SAM; with ctx: returns the kernel mask the mapping call left there"""
    reads = grid_reads(row)
    assert len(reads) == row["n_reads"]
    res = m.map([r[1] for r in reads])
    mask = ctx.last_kernel_mask() if ctx is not None else None
    got = [star_seq_qual(l) for l in m.sam_batch(res, reads).rstrip("\n").split("\n")]
    want = grid_golden_sam(row)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a == b, (a[:300], b[:300])
    return mask


def _check_mask(row, mask):
    """which DP kernels a scoring row's mapping call ran: the generic kernel alone at a scoring the wave forms refuse (every box of the
    batch, 15 kbp boxes at bw = 1000 and short-read boxes alike), a wave form otherwise -- and for short reads nothing but wave forms"""
    print("kernel mask of %s: %d" % (row["name"], mask))
    assert ("wave" in row["tags"]) == grid_wave_scoring_ok(row) != ("generic" in row["tags"]), row["name"]
    if "generic" in row["tags"]:
        assert mask == 2, (row["name"], mask)
    else:
        assert mask & WAVE_BITS, (row["name"], mask)
        if row["variant"] == "sr":
            assert not mask & 2, (row["name"], mask)


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
        mask = _check_sam(m, row, gpu_ctx)
        if "score" in row["tags"]:
            _check_mask(row, mask)
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


@pytest.mark.parametrize("name", grid_ids("wave"))
def test_grid_wave_rows_on_the_generic_kernel(gpu_ctx, pkg, name):
    """set_kernel_mode(1): the boxes the library gathered for a row the wave kernels take, all on ksw_extd2_generic_kernel -- the same SAM,
    and the mask says the generic kernel alone ran"""
    row = grid_row(name)
    m, _, _ = _mapper(pkg, gpu_ctx, row)
    try:
        gpu_ctx.set_kernel_mode(1)
        assert _check_sam(m, row, gpu_ctx) == 2
    finally:
        gpu_ctx.set_kernel_mode(0)
        m.close()


def _score_rows(variant, tag):
    return [r["name"] for r in grid_rows("score") if r["variant"] == variant and tag in r["tags"]]


@pytest.mark.parametrize("env,variant,tag", [({"GDIET_DIAG_SHORTCUT": "0"}, "sr", "score"),  # every short alignment through the DP and walked back, none answered from its diagonal
                                             ({"GDIET_SR_PIPE": "0"}, "sr", "score"),        # the grouped short-alignment kernels instead of the skewed pipelines
                                             ({"GDIET_GROUP_LANES": "16"}, "sr", "score"),   # always four alignments per wavefront
                                             ({"GDIET_NARROW_BAND": "0"}, "lr", "wave"),     # every box at its full band
                                             ({"GDIET_NARROW_QUARTER": "0"}, "lr", "wave"),  # the quarter rung never offered ...
                                             ({"GDIET_NARROW_QUARTER": "1"}, "lr", "wave")])  # ... and always
def test_grid_score_rows_through_the_other_dp_routes(env, variant, tag):
    """the scoring rows under the switches that send their boxes another way through the DP stage (tests/grid_env_check.py, in a process of
    its own: the library reads these switches once): every one gives the golden SAM"""
    rows = _score_rows(variant, tag)
    assert len(rows) >= 4
    r = subprocess.run([sys.executable, os.path.join(HERE, "grid_env_check.py")] + rows, capture_output=True, text=True, env=dict(os.environ, **env), timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("name", ["lr_score_b120first_sv", "sr_score_a16"])
def test_grid_score_rows_submit_and_wait_with_two_tickets_open(gpu_ctx, pkg, name):
    """gdiet_hip_map_submit / _wait at a non-preset scoring (one row on the generic kernel, one on the wave forms behind the widened
    pre-filter): the row in two resident batches, both tickets open at once -- the records of the synchronous call, i.e. the golden SAM"""
    row = grid_row(name)
    assert "score" in row["tags"]
    m, _, _ = _mapper(pkg, gpu_ctx, row)
    reads = grid_reads(row)
    half = len(reads) // 2
    parts = [reads[:half], reads[half:]]
    want = grid_golden_sam(row)
    wants = [[l for l in want if l.split("\t")[0] in {r[0] for r in p}] for p in parts]
    batches = [m.upload([r[1] for r in p]) for p in parts]
    lines = lambda res, p: [star_seq_qual(l) for l in m.sam_batch(res, p).rstrip("\n").split("\n")]
    try:
        sync = [lines(m.map_uploaded(b), p) for b, p in zip(batches, parts)]
        assert sync == wants
        m.set_inflight(2)
        ta, tb = m.submit(batches[0]), m.submit(batches[1])
        assert lines(m.wait(ta), parts[0]) == sync[0]
        assert lines(m.wait(tb), parts[1]) == sync[1]
    finally:
        for b in batches:
            m.free_batch(b)
        m.close()


def test_grid_limits_stay_refusals(gpu_ctx, pkg):
    """what the library does not take is refused with GDIET_E_PARAM (-3) and a message, not mapped with: a pattern of 64 positions, one
    without a 1, one with 41 ones, k = 29, w = 65 (index build); vt_nb_loc = 23, AF_max_loc = 25 (mapping: more candidates than a vote
    record holds); a scoring the reference's mm_check_opt refuses -- q or e not positive, a dual gap model without e > e2 and
    q + e < q2 + e2 (-O 24,12 -E 1,2: the larger model first, which the DP-level entry points do take), (q+e)+(q2+e2) > 127 -- or whose
    values the DP's int8_t parameters cannot hold.  After every refused scoring the same mapper maps four reads as recorded"""
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
    bad_scorings = [(dict(q=0), "positive"), (dict(e=0), "positive"), (dict(q=24, q2=12, e=1, e2=2), "dual gap"), (dict(q=6, q2=6, e=2, e2=1), "dual gap"),
                    (dict(q=40, e=3, q2=90, e2=2), "> 127"), (dict(a=200), "int8_t"), (dict(b=300), "int8_t"), (dict(q2=1000), "int8_t")]
    for row in (grid_row("lr_score_b120last_sv"), grid_row("sr_score_single")):
        base, preset, ov = grid_mapper_args(row)
        names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
        reads = grid_reads(row)[:4]
        want = [l for l in grid_golden_sam(row) if l.split("\t")[0] in {r[0] for r in reads}]
        assert sum(1 for l in want if l.split("\t")[2] != "*") >= 3
        m = pkg.Mapper(gpu_ctx, names, seqs, preset=preset, **ov)
        try:
            good = pkg.MapOpt.from_buffer_copy(m.opt)
            for bad, rule in bad_scorings:
                m.opt = pkg.MapOpt.from_buffer_copy(good)
                for key, v in bad.items():
                    setattr(m.opt, key, v)
                with pytest.raises(pkg.GdietError, match=r"gdiet_hip error -3: scoring: .*" + re.escape(rule)):
                    m.map([r[1] for r in reads])
                batch = m.upload([r[1] for r in reads])
                try:
                    with pytest.raises(pkg.GdietError, match=r"gdiet_hip error -3: scoring: .*" + re.escape(rule)):
                        m.submit(batch)
                finally:
                    m.free_batch(batch)
                m.opt = pkg.MapOpt.from_buffer_copy(good)
                got = [star_seq_qual(l) for l in m.sam_batch(m.map([r[1] for r in reads]), reads).rstrip("\n").split("\n")]
                assert got == want, (row["name"], bad)
        finally:
            m.close()
    assert len(grid_rows()) >= 20

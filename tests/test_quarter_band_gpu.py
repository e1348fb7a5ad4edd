"""GPU: the 239-wide rung of the 64-lane DP kernel's ladder through gdiet_hip_ksw_extd2_batch, in contexts created with
GDIET_NARROW_QUARTER=1 (always offered) and =0 (never).  A marked box whose band is wider than GD_W_QUARTER = 239 runs the quarter-block
rows at 239 first and keeps the result when the certificate holds; otherwise the same wavefront goes on with the half-block rows (at 495
or at its own band) and then the full band.  Scores and CIGARs against the oracle at the w given; the counters of
gdiet_hip_last_narrow_rungs and gdiet_hip_last_narrow_band against what the planner's mark, the rung function and the certificate say on
the oracle's scores at 239 and at 495 (quarter_pairs.expected_ladder)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import quarter_pairs
from narrow_pairs import W_NARROW, load_cert_shim, long_indels
from quarter_pairs import W_QUARTER, expected_ladder, load_quarter_shim

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    d = tmp_path_factory.mktemp("shims")
    return load_cert_shim(d), load_quarter_shim(d)


@pytest.fixture(scope="module")
def ctxs(pkg, gpu_ctx):
    """(context that always offers the 239 rung, context that never does): the switch is read when a context is created"""
    made = []
    old = os.environ.get("GDIET_NARROW_QUARTER")
    try:
        for v in ("1", "0"):
            os.environ["GDIET_NARROW_QUARTER"] = v
            made.append(pkg.Context(0))
    finally:
        if old is None:
            os.environ.pop("GDIET_NARROW_QUARTER", None)
        else:
            os.environ["GDIET_NARROW_QUARTER"] = old
    yield tuple(made)
    for c in made:
        c.close()


@pytest.fixture(scope="module")
def geometry():
    return quarter_pairs.geometry_pairs()


def _oracle_all(oracle, pairs, ws):
    gdo, lib = oracle
    a, b, q, e, q2, e2 = gdo.PRESETS["hifi"]
    mat = gdo.score_matrix(a, b)
    return [gdo.oracle_extd2(lib, qq, tt, mat, q, e, q2, e2, int(w)) for (qq, tt), w in zip(pairs, ws)]


def _check(sc, cg, want, what):
    bad = [i for i, o in enumerate(want) if sc[i] != o["score"] or not np.array_equal(cg[i], o["cigar"])]
    assert not bad, "%s: %d of %d differ from the oracle, first %s" % (what, len(bad), len(want), bad[:5])


def _run(ctx, pkg, pairs, w):
    sc, cg = ctx.ksw_extd2_batch([p[0] for p in pairs], [p[1] for p in pairs], w, pkg.KswScore.from_preset("hifi"))
    return sc, cg, ctx.last_narrow_band(), ctx.last_narrow_rungs()


@pytest.mark.gpu
def test_emulator_geometries_at_their_own_band(ctxs, pkg, oracle, shims, geometry):
    """bands up to 239: nothing to certify on any rung, whichever kernel the planner gives a pair to"""
    pairs, bands = geometry
    sc, cg, band, rungs = _run(ctxs[0], pkg, pairs, np.array(bands, np.int32))
    _check(sc, cg, _oracle_all(oracle, pairs, bands), "own band")
    want_band, want_rungs, _ = expected_ladder(*shims, oracle, pairs, bands)
    assert (band, rungs) == (want_band, want_rungs) == ((0, 0), (0, 0, 0, 0))


@pytest.mark.gpu
def test_emulator_geometries_at_w_1000_climb_the_ladder(ctxs, pkg, oracle, shims, geometry):
    pairs, _ = geometry
    ws = [1000] * len(pairs)
    full = _oracle_all(oracle, pairs, ws)
    sc, cg, band, rungs = _run(ctxs[0], pkg, pairs, 1000)
    _check(sc, cg, full, "w = 1000, rung offered")
    want_band, want_rungs, ends = expected_ladder(*shims, oracle, pairs, ws)
    print("ladder at w = 1000: %d pairs, band counters %s, rungs %s" % (len(pairs), band, rungs))
    assert band == want_band and rungs == want_rungs
    # the grid reaches both rungs: most pairs finish at 239; those with lengths w - 1 apart pay for a gap of that size and finish at 495
    # (the full band is reached by the pairs of test_two_opposite_600_base_indels_fail_both_rungs)
    assert min(sum(e == x for e in ends) for x in (W_QUARTER, W_NARROW)) >= 20 and rungs[0] >= 200
    # the same batch where the rung is never offered: same alignments, same counters of gdiet_hip_last_narrow_band, nothing at 239
    sc0, cg0, band0, rungs0 = _run(ctxs[1], pkg, pairs, 1000)
    _check(sc0, cg0, full, "w = 1000, rung not offered")
    off_band, off_rungs, _ = expected_ladder(*shims, oracle, pairs, ws, offered=False)
    assert band0 == band == off_band
    assert rungs0 == off_rungs and rungs0[:2] == (0, 0) and rungs0[2:] == band0


@pytest.mark.gpu
def test_paths_that_leave_239_but_not_495(ctxs, pkg, oracle, shims):
    """about 2 600 bases with a 300-base insertion and a 300-base deletion further on: the path is 300 off the diagonal in between, so the
    certificate fails at 239, holds at 495, and the alignment is the oracle's at 1000"""
    gdo, lib = oracle
    rng = np.random.default_rng(239495)
    pairs = [long_indels(rng, 2600 + 16 * k + k, [300 + k, -300] if k & 1 else [-300 - k, 300]) for k in range(12)]
    full = _oracle_all(oracle, pairs, [1000] * len(pairs))
    at239 = _oracle_all(oracle, pairs, [W_QUARTER] * len(pairs))
    assert all(not gdo.same(a, b, keys=("score",)) for a, b in zip(at239, full))  # built so that the band matters
    sc, cg, band, rungs = _run(ctxs[0], pkg, pairs, 1000)
    _check(sc, cg, full, "second rung")
    n = len(pairs)
    assert band == (n, n) and rungs == (n, 0, n, n)
    assert expected_ladder(*shims, oracle, pairs, [1000] * n)[:2] == ((n, n), (n, 0, n, n))


@pytest.mark.gpu
def test_two_opposite_600_base_indels_fail_both_rungs(ctxs, pkg, oracle, shims):
    """the pairs of tests/test_narrow_band_gpu.py whose path is 600 off the diagonal: quarter-block rows, half-block rows, full band"""
    rng = np.random.default_rng(77)
    pairs = [long_indels(rng, 4000 + 16 * k + k, [600, -600] if k & 1 else [-600, 600]) for k in range(6)]
    full = _oracle_all(oracle, pairs, [1000] * len(pairs))
    n = len(pairs)
    for ctx, want_rungs in ((ctxs[0], (n, 0, n, 0)), (ctxs[1], (0, 0, n, 0))):
        sc, cg, band, rungs = _run(ctx, pkg, pairs, 1000)
        _check(sc, cg, full, "full band")
        assert band == (n, 0) and rungs == want_rungs
    assert expected_ladder(*shims, oracle, pairs, [1000] * n)[:2] == ((n, 0), (n, 0, n, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("offered", ["0", "1"])
def test_goldens_with_the_rung_off_and_on(offered):
    """the hifi goldens mapped in a process of its own with GDIET_NARROW_QUARTER=0 / =1: every SAM record as recorded"""
    env = dict(os.environ, GDIET_NARROW_QUARTER=offered)
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden_env_check.py"), "hifi", "hifi_sv", "hifi_rep"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]

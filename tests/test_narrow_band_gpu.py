"""GPU: the narrow form of the 64-lane DP kernel through gdiet_hip_ksw_extd2_batch.  Boxes whose band is at most GD_W_NARROW = 495 run
on half-block rows at their own band; boxes at w = 1000 run the half-block rows at 495 first and keep the result when the certificate
holds, otherwise the same wavefront runs the full band.  Scores and CIGARs against the oracle at the w given, and the counters of
gdiet_hip_last_narrow_band against what the oracle's score at 495 makes the certificate say."""
import os
import subprocess
import sys

import numpy as np
import pytest

import narrow_pairs
from narrow_pairs import W_NARROW, expected_counters, load_cert_shim, long_indels, tandem

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return load_cert_shim(tmp_path_factory.mktemp("cert"))


@pytest.fixture(scope="module")
def geometry_pairs():
    return narrow_pairs.geometry_pairs()


def _oracle_all(oracle, pairs, ws):
    gdo, lib = oracle
    a, b, q, e, q2, e2 = gdo.PRESETS["hifi"]
    mat = gdo.score_matrix(a, b)
    return [gdo.oracle_extd2(lib, qq, tt, mat, q, e, q2, e2, int(w)) for (qq, tt), w in zip(pairs, ws)]


def _check(sc, cg, want, what):
    bad = [i for i, o in enumerate(want) if sc[i] != o["score"] or not np.array_equal(cg[i], o["cigar"])]
    assert not bad, "%s: %d of %d differ from the oracle, first %s" % (what, len(bad), len(want), bad[:5])


@pytest.mark.gpu
def test_own_narrow_bands_on_half_block_rows(gpu_ctx, pkg, oracle, shim, geometry_pairs):
    pairs, bands = geometry_pairs
    modes = [shim.cert_planned_mode(len(q), len(t), w) for (q, t), w in zip(pairs, bands)]
    assert sum(m == 2 for m in modes) >= len(pairs) * 4 // 7  # (|tlen - qlen| == w is not admitted, short ones go to the grouped kernels)
    sc, cg = gpu_ctx.ksw_extd2_batch([p[0] for p in pairs], [p[1] for p in pairs], np.array(bands, np.int32), pkg.KswScore.from_preset("hifi"))
    assert gpu_ctx.last_narrow_band() == (0, 0)  # nothing to certify at a box's own band
    _check(sc, cg, _oracle_all(oracle, pairs, bands), "own band")


@pytest.mark.gpu
def test_same_pairs_at_w_1000_try_the_narrow_band(gpu_ctx, pkg, oracle, shim, geometry_pairs):
    pairs, _ = geometry_pairs
    sc, cg = gpu_ctx.ksw_extd2_batch([p[0] for p in pairs], [p[1] for p in pairs], 1000, pkg.KswScore.from_preset("hifi"))
    got = gpu_ctx.last_narrow_band()
    _check(sc, cg, _oracle_all(oracle, pairs, [1000] * len(pairs)), "w = 1000")
    tried, cert, which = expected_counters(shim, oracle, pairs, 1000)
    print("narrow band at w = 1000: tried %d certified %d of %d pairs" % (tried, cert, len(pairs)))
    assert got == (tried, cert)
    # every pair whose lengths differ by at most one certifies: it loses a few dozen against a bound 1 500 below the perfect score
    small = [c for (q, t), c in zip(pairs, which) if abs(len(q) - len(t)) <= 1]
    assert len(small) >= 70 and all(c is True for c in small)


@pytest.mark.gpu
def test_paths_outside_the_narrow_band_fall_back_to_the_full_band(gpu_ctx, pkg, oracle, shim):
    """about 4 kbp each: two opposite 600-base indels; a tandem array of period above GD_W_NARROW / 2 with two copies more in the
    query and as many bases removed further on -- the true path is more than 495 off the diagonal in between"""
    gdo, lib = oracle
    rng = np.random.default_rng(77)
    pairs = []
    for k in range(6):
        pairs.append(long_indels(rng, 4000 + 16 * k + k, [600, -600] if k & 1 else [-600, 600]))
    for k in range(6):
        period = int(rng.integers(W_NARROW // 2 + 10, 400))
        q, t = tandem(rng, 4000 + 7 * k, period, 3, 5)
        cut = len(q) - 500 - 2 * period
        q = np.ascontiguousarray(np.concatenate([q[:cut], q[cut + 2 * period:]]))
        pairs.append((q, t))
    full = _oracle_all(oracle, pairs, [1000] * len(pairs))
    narrow = _oracle_all(oracle, pairs, [W_NARROW] * len(pairs))
    assert all(not gdo.same(a, b, keys=("score",)) for a, b in zip(narrow, full))  # built so that the band matters
    sc, cg = gpu_ctx.ksw_extd2_batch([p[0] for p in pairs], [p[1] for p in pairs], 1000, pkg.KswScore.from_preset("hifi"))
    got = gpu_ctx.last_narrow_band()
    _check(sc, cg, full, "fallback")
    assert got == (len(pairs), 0)
    assert expected_counters(shim, oracle, pairs, 1000)[:2] == (len(pairs), 0)


@pytest.mark.gpu
def test_goldens_with_the_narrow_band_switched_off():
    """GDIET_NARROW_BAND=0: every box at its full band, as before -- the hifi goldens, and the counters stay at zero"""
    env = dict(os.environ, GDIET_NARROW_BAND="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden_env_check.py"), "hifi", "hifi_sv", "hifi_rep"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    r = subprocess.run([sys.executable, os.path.join(HERE, "narrow_env_check.py")], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]

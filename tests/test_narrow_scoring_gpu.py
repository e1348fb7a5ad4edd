"""GPU: the narrow form of the 64-lane DP kernel (half-block rows, the certificate, the full band on failure) through
gdiet_hip_ksw_extd2_batch at every scoring of the oracle's table that reaches it, hifi apart (tests/test_narrow_band_gpu.py): the edges
of what the register-resident kernels accept -- the 120 bound, the S-key corner, e == e2, q == q2, a score for N, a = 8 and 16, the gap
models in the wrong order.  Per scoring: every fourth pair of the geometry grid (Ns in every fifth query, byte 4 and byte 7 in turn)
and the ten error-free pairs whose best path runs one diagonal beyond the band of 495 (narrow_pairs.band_edge_pairs), which the
certificate must refuse by a margin of 4 to 19.  Scores and CIGARs against the oracle at the band given; the counters of
gdiet_hip_last_narrow_band against what the certificate says on the oracle's UNSHIFTED score at 495."""
import gdo as _gdo
import numpy as np
import pytest

from narrow_pairs import W_NARROW, band_edge_pairs, expected_counters, geometry_pairs, load_cert_shim

NAMES = [k for k, v in _gdo.SCORINGS.items() if _gdo.wave_scoring_ok(*v) and k != "hifi"]
AVX = _gdo.EZ_APPROX_MAX | _gdo.EZ_AVX512_SC  # the score table the library follows: the oracle needs the flag for queries with byte 7


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return load_cert_shim(tmp_path_factory.mktemp("cert"))


@pytest.fixture(scope="module")
def batch():
    """(pairs, own bands, number of geometry pairs): the geometry pairs first, the ten band-edge pairs behind them"""
    pairs, bands = geometry_pairs()
    pairs, bands = pairs[::4], bands[::4]
    rng = np.random.default_rng(4)
    for j in range(0, len(pairs), 5):
        q = pairs[j][0].copy()
        q[rng.random(len(q)) < 0.01] = 7 if (j // 5) & 1 else 4  # (7: N of a reverse-complemented read)
        pairs[j] = (q, pairs[j][1])
    n_geo = len(pairs)
    edge = band_edge_pairs(5)
    assert all(abs(len(t) - len(q)) < W_NARROW for q, t in edge) and max(max(len(q), len(t)) for q, t in pairs + edge) <= 2100
    return pairs + edge, bands + [W_NARROW] * len(edge), n_geo


def _oracle_all(oracle, scoring, pairs, ws):
    gdo, lib = oracle
    a, b, q, e, q2, e2, amb = scoring
    mat = gdo.score_matrix(a, b, sc_ambi=amb)
    return [gdo.oracle_extd2(lib, qq, tt, mat, q, e, q2, e2, int(w), flag=AVX) for (qq, tt), w in zip(pairs, ws)]


def _check(sc, cg, want, what):
    bad = [i for i, o in enumerate(want) if sc[i] != o["score"] or not np.array_equal(cg[i], o["cigar"])]
    assert not bad, "%s: %d of %d differ from the oracle, first %s" % (what, len(bad), len(want), bad[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_narrow_band_at_a_table_scoring(gpu_ctx, pkg, oracle, shim, batch, name):
    gdo, _ = oracle
    pairs, bands, n_geo = batch
    scoring = gdo.SCORINGS[name]
    a, b, q, e, q2, e2, amb = scoring
    ksc = pkg.KswScore(a, -b, amb, q, e, q2, e2, 0, pkg.hip_abi.EZ_APPROX_MAX)  # the caller's order of the gap models
    qs, ts = [p[0] for p in pairs], [p[1] for p in pairs]

    # own band: half-block rows wherever the geometry is admitted, nothing to certify
    modes = [shim.cert_planned_mode(len(qq), len(tt), w) for (qq, tt), w in zip(pairs, bands)]
    assert sum(m == 2 for m in modes) >= len(pairs) // 2
    sc, cg = gpu_ctx.ksw_extd2_batch(qs, ts, np.array(bands, np.int32), ksc)
    assert gpu_ctx.last_narrow_band() == (0, 0)
    _check(sc, cg, _oracle_all(oracle, scoring, pairs, bands), "%s, own band" % name)

    # w = 1000: the band of 495 first; the result is kept where the certificate holds on the kernel's own (unshifted) score.  The reported
    # score carries the bias of a swapped scoring also where the certified early return answered.
    full = _oracle_all(oracle, scoring, pairs, [1000] * len(pairs))
    sc, cg = gpu_ctx.ksw_extd2_batch(qs, ts, 1000, ksc)
    got = gpu_ctx.last_narrow_band()
    _check(sc, cg, full, "%s, w = 1000" % name)
    tried, cert, which = expected_counters(shim, oracle, pairs, 1000, scoring, flag=AVX)
    print("narrow band at %s, w = 1000: tried %d certified %d of %d pairs" % (name, tried, cert, len(pairs)))
    assert got == (tried, cert)
    assert sum(c is False for c in which[n_geo:]) >= 8  # the band-edge pairs: tried, refused, the full band in the same backtrace slot
    small = [c for (qq, tt), c in zip(pairs[:n_geo], which) if abs(len(qq) - len(tt)) <= 1]
    assert len(small) >= 15 and all(c is True for c in small)

    # the generic LDS kernel on the same pairs: the same alignments, and no narrow band
    gpu_ctx.set_kernel_mode(1)
    try:
        sc, cg = gpu_ctx.ksw_extd2_batch(qs, ts, 1000, ksc)
        got = gpu_ctx.last_narrow_band()
    finally:
        gpu_ctx.set_kernel_mode(0)
    _check(sc, cg, full, "%s, generic kernel" % name)
    assert got == (0, 0)

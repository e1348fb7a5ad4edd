"""GPU: the paired steady rows of the quarter-block and half-block forms with the two-lane selector update (gdw_quarter_rows,
gdw_narrow_rows in ksw_wave.hip.h) through gdiet_hip_ksw_extd2_batch against the oracle's score and CIGAR, in contexts created with
GDIET_NARROW_QUARTER=1 (a marked box runs the quarter-block rows at 239 first) and =0 (it starts with the half-block rows at 495).
Lengths of 1 500 bases -- four times round the ring of 16 blocks -- and of 2 600, round the ring of 32; tlen mod 16 in {0, 1, 3, 4, 5, 15};
tlen - qlen in {0, 1, -1, 37, -37}; runs of N in every third target.  At w = 1000 the boxes climb the ladder (bands 239 and 495: two
lanes patched on 15 pairs of 16); own bands 401 (the same at a band of its own, in the context that does not offer 239) and 400 (a multiple of 16: the two rows of a pair
differ in `up` and every pair makes its selectors, the statements kept for such bands)."""
import os

import numpy as np
import pytest

from narrow_pairs import load_cert_shim, long_indels, pair_of_lengths
from quarter_pairs import expected_ladder, load_quarter_shim

MODS = (0, 1, 3, 4, 5, 15)
DELTAS = (0, 1, -1, 37, -37)


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
def pairs():
    """60 pairs: 2 lengths x 6 residues of tlen x 5 length differences, 1 % point errors; every third target with three runs of 2-12 Ns"""
    rng = np.random.default_rng(20261020)
    out = []
    for base in (1500, 2600):
        for mod in MODS:
            for delta in DELTAS:
                tlen = (base & ~15) + mod
                q, t = pair_of_lengths(rng, tlen - delta, tlen, 0.0)
                if len(out) % 3 == 0:
                    t = t.copy()
                    for at in rng.integers(50, tlen - 80, size=3):
                        t[at:at + int(rng.integers(2, 13))] = 4
                assert len(t) % 16 == mod and len(t) - len(q) == delta
                out.append((q, t))
    return out


def _oracle_all(oracle, pairs, w):
    gdo, lib = oracle
    a, b, q, e, q2, e2 = gdo.PRESETS["hifi"]
    mat = gdo.score_matrix(a, b)
    return [gdo.oracle_extd2(lib, qq, tt, mat, q, e, q2, e2, int(w)) for qq, tt in pairs]


def _check(sc, cg, want, what):
    bad = [i for i, o in enumerate(want) if sc[i] != o["score"] or not np.array_equal(cg[i], o["cigar"])]
    assert not bad, "%s: %d of %d differ from the oracle, first %s" % (what, len(bad), len(want), bad[:5])


def _run(ctx, pkg, pairs, w):
    sc, cg = ctx.ksw_extd2_batch([p[0] for p in pairs], [p[1] for p in pairs], w, pkg.KswScore.from_preset("hifi"))
    return sc, cg, ctx.last_narrow_band(), ctx.last_narrow_rungs()


@pytest.mark.gpu
def test_ladder_at_w_1000(ctxs, pkg, oracle, shims, pairs):
    """every pair certifies on the first rung it runs: the quarter-block rows at 239 where offered, the half-block rows at 495 where not"""
    full = _oracle_all(oracle, pairs, 1000)
    n = len(pairs)
    for ctx, offered in ((ctxs[0], True), (ctxs[1], False)):
        sc, cg, band, rungs = _run(ctx, pkg, pairs, 1000)
        _check(sc, cg, full, "w = 1000, rung %s" % ("offered" if offered else "not offered"))
        want_band, want_rungs, _ = expected_ladder(*shims, oracle, pairs, [1000] * n, offered=offered)
        assert (band, rungs) == (want_band, want_rungs)
        assert band == (n, n) and rungs == ((n, n, 0, 0) if offered else (0, 0, n, n))


@pytest.mark.gpu
@pytest.mark.parametrize("w", [400, 401])
def test_own_bands_on_both_sides_of_a_multiple_of_16(ctxs, pkg, oracle, shims, pairs, w):
    """where the 239 rung is not offered the boxes run the half-block rows at their own band, nothing to certify: 400 keeps every lane
    making its selectors on every pair, 401 patches two lanes; where it is offered a box with 239 < w <= 495 tries 239 first, and these
    certify there -- the alignment is the oracle's at w either way"""
    want = _oracle_all(oracle, pairs, w)
    n = len(pairs)
    assert all(shims[0].cert_planned_mode(len(q), len(t), w) == 2 for q, t in pairs)  # GD_NARROW_OWN
    for ctx, offered in ((ctxs[0], True), (ctxs[1], False)):
        sc, cg, band, rungs = _run(ctx, pkg, pairs, w)
        _check(sc, cg, want, "own band %d, rung %s" % (w, "offered" if offered else "not offered"))
        want_band, want_rungs, ends = expected_ladder(*shims, oracle, pairs, [w] * n, offered=offered)
        assert (band, rungs) == (want_band, want_rungs)
        assert band == (0, 0) and rungs == ((n, n, 0, 0) if offered else (0, 0, 0, 0))
        assert offered or ends == [w] * n  # the half-block rows at the box's own band did run


@pytest.mark.gpu
def test_300_base_insertion_and_deletion_walk_the_half_rows_at_495(ctxs, pkg, oracle, shims):
    """the path is 300 off the diagonal between the two: the certificate fails at 239 and holds at 495"""
    rng = np.random.default_rng(239495)
    pairs = [long_indels(rng, 2600 + 16 * k + k, [300 + k, -300] if k & 1 else [-300 - k, 300]) for k in range(6)]
    n = len(pairs)
    full = _oracle_all(oracle, pairs, 1000)
    for ctx, want_rungs in ((ctxs[0], (n, 0, n, n)), (ctxs[1], (0, 0, n, n))):
        sc, cg, band, rungs = _run(ctx, pkg, pairs, 1000)
        _check(sc, cg, full, "second rung")
        assert band == (n, n) and rungs == want_rungs
    assert expected_ladder(*shims, oracle, pairs, [1000] * n)[:2] == ((n, n), (n, 0, n, n))


@pytest.mark.gpu
def test_two_opposite_600_base_indels_run_the_full_band(ctxs, pkg, oracle, shims):
    """600 off the diagonal: quarter-block rows, half-block rows, then the full band in the same wavefront"""
    rng = np.random.default_rng(77)
    pairs = [long_indels(rng, 4000 + 16 * k + k, [600, -600] if k & 1 else [-600, 600]) for k in range(4)]
    n = len(pairs)
    full = _oracle_all(oracle, pairs, 1000)
    for ctx, want_rungs in ((ctxs[0], (n, 0, n, 0)), (ctxs[1], (0, 0, n, 0))):
        sc, cg, band, rungs = _run(ctx, pkg, pairs, 1000)
        _check(sc, cg, full, "full band")
        assert band == (n, 0) and rungs == want_rungs
    assert expected_ladder(*shims, oracle, pairs, [1000] * n)[:2] == ((n, 0), (n, 0, n, 0))

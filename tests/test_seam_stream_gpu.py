"""GPU: the paired steady rows of the quarter-block and half-block forms as they are now -- the row's fresh query byte from the seam stream
(GdwSeam, ksw_wave_core.h), the selector step from a shifted constant, the target-N term of the scores under a wave-uniform branch
(gdw_quarter_rows, gdw_narrow_rows in ksw_wave.hip.h) -- through gdiet_hip_ksw_extd2_batch against the oracle's score and CIGAR, in contexts
created with GDIET_NARROW_QUARTER=1 (a marked box runs the quarter-block rows at 239 first) and =0 (it starts with the half-block rows at 495).
Lengths of 1 500 bases -- four times round the ring of 16 blocks -- and of 2 600, round the ring of 32; tlen mod 16 in {0, 1, 3, 4, 5, 15};
tlen - qlen in {0, 1, -1, 37, -37}; the queries packed back to back, so that they start at every byte alignment of a dword (and of the
stream's 8-byte window); one batch with runs of N in every third target and the same batch with no N at all (both sides of the branch);
w = 1000 (the boxes climb the ladder) and own bands 400 / 401; the ladder's counters as expected_ladder predicts them."""
import os

import numpy as np
import pytest

from narrow_pairs import load_cert_shim, pair_of_lengths
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


def _make_pairs():
    """(60 pairs without N, the same with three runs of 2-12 Ns in every third target): 2 lengths x 6 residues of tlen x 5 length
    differences, 1 % point errors"""
    rng = np.random.default_rng(20261021)
    clean, with_n = [], []
    for base in (1500, 2600):
        for mod in MODS:
            for delta in DELTAS:
                tlen = (base & ~15) + mod
                q, t = pair_of_lengths(rng, tlen - delta, tlen, 0.0)
                assert len(t) % 16 == mod and len(t) - len(q) == delta
                clean.append((q, t))
                if len(with_n) % 3 == 0:
                    t = t.copy()
                    for at in rng.integers(50, tlen - 80, size=3):
                        t[at:at + int(rng.integers(2, 13))] = 4
                with_n.append((q, t))
    return clean, with_n


@pytest.fixture(scope="module")
def batches():
    return _make_pairs()


def test_queries_start_at_every_alignment():
    """the batch arena keeps the queries back to back (hip_abi.pack): their offsets take all 8 residues, so all four alignments of a dword"""
    clean, with_n = _make_pairs()
    off = np.concatenate([[0], np.cumsum([len(q) for q, _ in clean])[:-1]])
    assert set(int(x) for x in off % 8) == set(range(8))
    assert all(not (t == 4).any() for _, t in clean) and sum(bool((t == 4).any()) for _, t in with_n) == 20


@pytest.fixture(scope="module")
def wanted(oracle, batches):
    """the oracle's alignments, computed once: {(which batch, w)}"""
    gdo, lib = oracle
    a, b, q, e, q2, e2 = gdo.PRESETS["hifi"]
    mat = gdo.score_matrix(a, b)
    clean, with_n = batches
    out = {}
    for name, pairs, ws in (("clean", clean, (1000,)), ("n", with_n, (1000, 400, 401))):
        for w in ws:
            out[name, w] = [gdo.oracle_extd2(lib, qq, tt, mat, q, e, q2, e2, w) for qq, tt in pairs]
    return out


def _check(sc, cg, want, what):
    bad = [i for i, o in enumerate(want) if sc[i] != o["score"] or not np.array_equal(cg[i], o["cigar"])]
    assert not bad, "%s: %d of %d differ from the oracle, first %s" % (what, len(bad), len(want), bad[:5])


def _run(ctx, pkg, pairs, w):
    sc, cg = ctx.ksw_extd2_batch([p[0] for p in pairs], [p[1] for p in pairs], w, pkg.KswScore.from_preset("hifi"))
    return sc, cg, ctx.last_narrow_band(), ctx.last_narrow_rungs()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["n", "clean"])
def test_ladder_at_w_1000(ctxs, pkg, oracle, shims, batches, wanted, which):
    """every pair certifies on the first rung it runs: the quarter-block rows at 239 where offered, the half-block rows at 495 where not;
    with Ns in a third of the targets, and with none in the batch"""
    pairs = batches[1] if which == "n" else batches[0]
    n = len(pairs)
    for ctx, offered in ((ctxs[0], True), (ctxs[1], False)):
        sc, cg, band, rungs = _run(ctx, pkg, pairs, 1000)
        _check(sc, cg, wanted[which, 1000], "w = 1000, batch %s, rung %s" % (which, "offered" if offered else "not offered"))
        want_band, want_rungs, _ = expected_ladder(*shims, oracle, pairs, [1000] * n, offered=offered)
        assert (band, rungs) == (want_band, want_rungs)
        assert band == (n, n) and rungs == ((n, n, 0, 0) if offered else (0, 0, n, n))


@pytest.mark.gpu
@pytest.mark.parametrize("w", [400, 401])
def test_own_bands_on_both_sides_of_a_multiple_of_16(ctxs, pkg, oracle, shims, batches, wanted, w):
    """where the 239 rung is not offered the boxes run the half-block rows at their own band: at 400 every lane makes its selectors on
    every pair, at 401 two lanes are patched -- the stream feeds both; where it is offered these boxes certify at 239"""
    pairs = batches[1]
    n = len(pairs)
    assert all(shims[0].cert_planned_mode(len(q), len(t), w) == 2 for q, t in pairs)  # GD_NARROW_OWN
    for ctx, offered in ((ctxs[0], True), (ctxs[1], False)):
        sc, cg, band, rungs = _run(ctx, pkg, pairs, w)
        _check(sc, cg, wanted["n", w], "own band %d, rung %s" % (w, "offered" if offered else "not offered"))
        want_band, want_rungs, ends = expected_ladder(*shims, oracle, pairs, [w] * n, offered=offered)
        assert (band, rungs) == (want_band, want_rungs)
        assert band == (0, 0) and rungs == ((n, n, 0, 0) if offered else (0, 0, 0, 0))
        assert offered or ends == [w] * n  # the half-block rows at the box's own band did run

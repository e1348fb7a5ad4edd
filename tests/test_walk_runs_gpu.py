"""GPU: the wavefront walks (ksw_backtrack.hip.h: a fetched window of 64 cells consumed from ballots, a run of diagonal cells in one step)
through gdiet_hip_ksw_extd2_batch, on every backtrace layout they read, against the oracle at the same band.  The pairs are built for the
walk, not for the DP: indels planted so that the match runs between them are 62..66 and 126..130 cells long (on and next to the ends of
one and two windows), an insertion right behind a deletion, indels of 70 and 200 bases (gap runs longer than a window), indels in the
first and the last three bases, lengths that differ by 1 and by 200.
  * HiFi scoring, w = 1000, in contexts created with GDIET_NARROW_QUARTER=1 (most boxes walk the 256-byte rows of the 239-wide rung),
    GDIET_NARROW_QUARTER=0 (the 512-byte rows of the 495-wide band) and GDIET_NARROW_BAND=0 (the full-band rows, gd_bt_wave_walk); the
    batch also holds the 300 + 300 and the two-opposite-600 pairs of narrow_pairs.long_indels, so that in the first context one batch
    walks all three row formats;
  * ONT scoring, w = 1300, 2 000-4 000 bases at 8 % error: the checkpointed kernel (GDIET_WIDE_CKPT=1: walks of a recomputed cone, chunk
    by chunk, r0 > 0) and the stored-backtrace wide-band kernels (GDIET_WIDE_CKPT=0 with GDIET_WIDE_TWO_WAVES=0 and =1).
last_narrow_rungs() / last_narrow_band() / last_kernel_mask() say that each context took the route it is here for."""
import contextlib
import os

import numpy as np
import pytest

from narrow_pairs import long_indels

RUNS = (62, 63, 64, 65, 66, 126, 127, 128, 129, 130)


@contextlib.contextmanager
def _context(pkg, **env):
    """a context of its own: the switches are read when a context is created"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = pkg.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        yield ctx
    finally:
        ctx.close()


def _rand(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8)


def planted(rng, tlen, first=None, indel=None):
    """a query that copies the target in runs of RUNS bases (in turn, from a random one on) with an indel of 1-3 bases between two runs;
    first: the length of the first run; indel: a function k -> (bases inserted, target bases skipped) replacing the random choice"""
    t = _rand(rng, tlen)
    parts, pos, k = [], 0, int(rng.integers(0, len(RUNS)))
    run = RUNS[k % len(RUNS)] if first is None else first
    while pos + run < tlen:
        parts.append(t[pos:pos + run])
        pos += run
        ins, dele = indel(len(parts)) if indel else ((int(rng.integers(1, 4)), 0) if rng.random() < 0.5 else (0, int(rng.integers(1, 4))))
        if ins:
            parts.append(_rand(rng, ins))
        pos = min(tlen, pos + dele)
        k += 1
        run = RUNS[k % len(RUNS)]
    parts.append(t[pos:])
    return np.ascontiguousarray(np.concatenate(parts), np.uint8), t


def walk_pairs():
    rng = np.random.default_rng(20261019)
    pairs = [planted(rng, int(n)) for n in (700, 1111, 1600, 2048, 2500, 3000)]
    # an insertion immediately followed by a deletion: 60 Cs in the query where the target has 60 As (nothing to match: 60 mismatches
    # cost 240, the two long gaps 2 (26 + 60) = 172)
    t = _rand(rng, 1500)
    t[700:760] = 0
    pairs.append((np.ascontiguousarray(np.concatenate([t[:700], np.full(60, 1, np.uint8), t[760:]])), t))
    pairs.append(planted(rng, 2200, indel=lambda k: (70, 0) if k == 5 else (0, 70) if k == 11 else (1, 0)))   # 70-base indels
    pairs.append(planted(rng, 2900, indel=lambda k: (200, 0) if k == 4 else (0, 200) if k == 12 else (0, 1)))  # 200-base indels
    pairs.append(planted(rng, 1300, first=2))                                                  # an indel in the first three bases ...
    q, t = planted(rng, 1400)
    pairs.append((np.ascontiguousarray(np.concatenate([q[:-2], _rand(rng, 2), q[-2:]])), t))   # ... and in the last three: inserted,
    q, t = planted(rng, 1700)
    pairs.append((np.ascontiguousarray(np.concatenate([q[:-3], q[-1:]])), t))                  # ... and deleted
    q, t = planted(rng, 1800, indel=lambda k: (1, 0) if k & 1 else (0, 1))
    pairs.append((np.ascontiguousarray(q[:len(t) - 1] if len(q) >= len(t) else q), t))         # qlen != tlen by 1 ...
    pairs.append(planted(rng, 2600, indel=lambda k: (200, 0) if k == 7 else (1, 0) if k & 1 else (0, 1)))      # ... and by about 200
    q, t = pairs[-1]
    assert abs(len(q) - len(t)) >= 190 and abs(len(pairs[-2][0]) - len(pairs[-2][1])) == 1
    return pairs


@pytest.fixture(scope="module")
def hifi_batch(oracle):
    """(the walk pairs, the 300 + 300 pairs, the two-opposite-600 pairs) and the oracle's alignments at w = 1000, computed once"""
    gdo, lib = oracle
    own = walk_pairs()
    rng = np.random.default_rng(239495)
    second = [long_indels(rng, 2600 + 16 * k + k, [300 + k, -300] if k & 1 else [-300 - k, 300]) for k in range(4)]
    rng = np.random.default_rng(77)
    third = [long_indels(rng, 4000 + 16 * k + k, [600, -600] if k & 1 else [-600, 600]) for k in range(4)]
    pairs = own + second + third
    a, b, q, e, q2, e2 = gdo.PRESETS["hifi"]
    mat = gdo.score_matrix(a, b)
    want = [gdo.oracle_extd2(lib, qq, tt, mat, q, e, q2, e2, 1000) for qq, tt in pairs]
    return pairs, want, (len(own), len(second), len(third))


def _check(sc, cg, want, what):
    bad = [i for i, o in enumerate(want) if sc[i] != o["score"] or not np.array_equal(cg[i], o["cigar"])]
    assert not bad, "%s: %d of %d differ from the oracle, first %s" % (what, len(bad), len(want), bad[:5])


def test_planted_runs_sit_on_the_window_boundaries(hifi_batch):
    """(CPU) the oracle's own CIGARs of the walk pairs hold match runs of every length 62..66 and 126..130, and gaps of 70 and 200"""
    _, want, (n_own, _, _) = hifi_batch
    ms = {int(c) >> 4 for o in want[:n_own] for c in o["cigar"] if int(c) & 15 == 0}
    gaps = {int(c) >> 4 for o in want[:n_own] for c in o["cigar"] if int(c) & 15 in (1, 2)}
    assert set(RUNS) <= ms and {70, 200} <= gaps
    ops = [int(c) & 15 for c in want[6]["cigar"]]
    assert any({x, y} == {1, 2} for x, y in zip(ops, ops[1:]))  # an insertion and a deletion with no match between them


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["quarter", "half", "full"])
def test_hifi_walks_on_every_row_format(pkg, gpu_ctx, hifi_batch, route):
    pairs, want, (n_own, n_second, n_third) = hifi_batch
    n = len(pairs)
    env = {"quarter": dict(GDIET_NARROW_QUARTER="1"), "half": dict(GDIET_NARROW_QUARTER="0"), "full": dict(GDIET_NARROW_BAND="0")}[route]
    with _context(pkg, **env) as ctx:
        sc, cg = ctx.ksw_extd2_batch([p[0] for p in pairs], [p[1] for p in pairs], 1000, pkg.KswScore.from_preset("hifi"))
        band, rungs, mask = ctx.last_narrow_band(), ctx.last_narrow_rungs(), ctx.last_kernel_mask()
    print("route %s: narrow band %s, rungs %s, kernel mask %d" % (route, band, rungs, mask))
    _check(sc, cg, want, route)
    assert mask == 1  # every pair on the 64-lane kernel
    if route == "quarter":
        # tried at 239 / certified there (256-byte rows walked); the others tried at 495 / certified there (512-byte rows walked); the
        # two-opposite-600 pairs fail both and walk the full-band rows: all three formats in one batch
        assert rungs[0] == n and rungs[1] >= n_own - 3 and rungs[2] == n - rungs[1]
        assert rungs[3] >= n_second and rungs[2] - rungs[3] == n_third
        assert band == (n, n - n_third)
    elif route == "half":
        assert rungs[:2] == (0, 0) and rungs[2] == n and rungs[3] == n - n_third and band == (n, n - n_third)
    else:
        assert band == (0, 0) and rungs == (0, 0, 0, 0)


@pytest.fixture(scope="module")
def ont_batch(oracle):
    gdo, lib = oracle
    rng = np.random.default_rng(1300)
    pairs = [gdo.make_pair(rng, int(n), 0.03, 0.025, 0.025) for n in (2000, 2345, 2800, 3100, 3333, 3600, 3900, 4000)]
    a, b, q, e, q2, e2 = gdo.PRESETS["ont"]
    mat = gdo.score_matrix(a, b)
    want = [gdo.oracle_extd2(lib, qq, tt, mat, q, e, q2, e2, 1300, flag=gdo.EZ_APPROX_MAX | gdo.EZ_AVX512_SC) for qq, tt in pairs]
    return pairs, want


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["ckpt", "one_wave", "two_waves"])
def test_ont_walks_on_the_wide_band_kernels(pkg, gpu_ctx, ont_batch, route):
    pairs, want = ont_batch
    env = {"ckpt": dict(GDIET_WIDE_CKPT="1"), "one_wave": dict(GDIET_WIDE_CKPT="0", GDIET_WIDE_TWO_WAVES="0"),
           "two_waves": dict(GDIET_WIDE_CKPT="0", GDIET_WIDE_TWO_WAVES="1")}[route]
    with _context(pkg, **env) as ctx:
        sc, cg = ctx.ksw_extd2_batch([p[0] for p in pairs], [p[1] for p in pairs], 1300, pkg.KswScore.from_preset("ont"))
        mask = ctx.last_kernel_mask()
    _check(sc, cg, want, route)
    assert mask == 8  # every pair on a wide-band kernel (more than 64 blocks in flight)

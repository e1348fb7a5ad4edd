"""GPU: the compact backtrace arena of the 64-lane DP kernel through gdiet_hip_ksw_extd2_batch at w = 1000 with HiFi scoring.  The slot of a
box that tries the narrow band holds the 512-byte rows only; a box whose certificate fails at both rungs claims full-band rows from the
overflow pool behind the slots, and one that finds the pool used up is served by a drain launch.  Scores and CIGARs against the oracle at
1000 whatever the pool's size; the counters of gdiet_hip_last_arena against the arithmetic of the layout.  The switches are read when the
library is loaded, so every case runs tests/compact_arena_run.py in a process of its own; the oracle's alignments are computed once."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import compact_arena_run as car
from narrow_pairs import load_cert_shim
from quarter_pairs import expected_ladder, load_quarter_shim

HERE = os.path.dirname(os.path.abspath(__file__))
N_FALLBACK = 12


def _align256(x):
    return (x + 255) & ~255


def _full(p):
    return _align256((len(p[0]) + len(p[1]) - 1) * 1024 + 64)


def _half(p):
    return _align256((len(p[0]) + len(p[1]) - 1) * 512 + 64)


@pytest.fixture(scope="module")
def want(oracle, tmp_path_factory):
    """per batch: the pairs, the oracle's alignments at 1000, the ladder's counters as the certificate gives them on the oracle's scores"""
    gdo, lib = oracle
    a, b, q, e, q2, e2 = gdo.PRESETS["hifi"]
    mat = gdo.score_matrix(a, b)
    d = tmp_path_factory.mktemp("shims")
    cert, qshim = load_cert_shim(d), load_quarter_shim(d)

    def expect(pairs):  # (on eight threads, a slice of the pairs each: the oracle is a C function that releases the GIL)
        assert all(cert.cert_planned_mode(len(qq), len(tt), 1000) == 1 for qq, tt in pairs)  # every box tries the narrow band: half-size slots

        def part(k):
            mine = pairs[k::8]
            return [gdo.oracle_extd2(lib, qq, tt, mat, q, e, q2, e2, 1000) for qq, tt in mine], expected_ladder(cert, qshim, oracle, mine, [1000] * len(mine))

        with ThreadPoolExecutor(8) as pool:
            parts = list(pool.map(part, range(8)))
        full, ends = [None] * len(pairs), [None] * len(pairs)
        for k, (f, (_, _, en)) in enumerate(parts):
            full[k::8], ends[k::8] = f, en
        band = tuple(sum(p[1][0][i] for p in parts) for i in range(2))
        rungs = tuple(sum(p[1][1][i] for p in parts) for i in range(4))
        return full, band, rungs, ends

    mix, hard = car.mix_pairs(), car.fallback_pairs()  # ("fallback24" is the twelve, twice)
    full, band, rungs, ends = expect(hard)
    return {"mix": (mix,) + expect(mix), "fallback24": (hard * 2, full * 2, tuple(2 * x for x in band), tuple(2 * x for x in rungs), ends * 2)}


def _run(which, tmp_path, **env):
    out = str(tmp_path / ("%s_%s.npz" % (which, "_".join("%s%s" % kv for kv in sorted(env.items())) or "default")))
    e = {k: v for k, v in os.environ.items() if k not in ("GDIET_BT_COMPACT", "GDIET_BT_OVERFLOW_MB")}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "compact_arena_run.py"), "pairs", which, out], capture_output=True, text=True, env=e, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    return np.load(out)


def _check(got, want_of, what):
    pairs, full, band, rungs, _ = want_of
    off = np.concatenate([[0], np.cumsum(got["n_cigar"])])
    bad = [i for i, o in enumerate(full) if got["score"][i] != o["score"] or not np.array_equal(got["cigar"][off[i]:off[i + 1]], o["cigar"])]
    assert not bad, "%s: %d of %d differ from the oracle, first %s" % (what, len(bad), len(full), bad[:5])
    assert tuple(got["band"]) == band and tuple(got["rungs"]) == rungs, (what, tuple(got["band"]), band, tuple(got["rungs"]), rungs)


@pytest.fixture(scope="module")
def default_run(tmp_path_factory):
    return _run("mix", tmp_path_factory.mktemp("default"))


@pytest.mark.gpu
def test_default_pool_serves_the_fallbacks(default_run, want):
    pairs, full, band, rungs, ends = want["mix"]
    _check(default_run, want["mix"], "default pool")
    # the batch reaches every rung: the reads finish at 239, twelve boxes at 495, twelve in the full band
    assert band[0] - band[1] == N_FALLBACK and sum(e == 239 for e in ends) >= 400 and sum(e == 495 for e in ends) == 12
    claimed, drained, arena = (int(x) for x in default_run["arena"])
    slots = sum(_half(p) for p in pairs)
    assert _align256(slots // 16) >= sum(_full(p) for p, e in zip(pairs, ends) if e == 1000)  # the batch is large enough for its pool to hold the twelve
    assert (claimed, drained) == (N_FALLBACK, 0)
    assert arena == slots + _align256(slots // 16)
    print("arena: compact %d bytes, full-size %d" % (arena, sum(_full(p) for p in pairs)))


@pytest.mark.gpu
def test_full_size_slots_give_the_same(default_run, want, tmp_path):
    pairs = want["mix"][0]
    got = _run("mix", tmp_path, GDIET_BT_COMPACT="0")
    _check(got, want["mix"], "GDIET_BT_COMPACT=0")
    for k in ("score", "cigar", "n_cigar", "band", "rungs"):
        assert np.array_equal(got[k], default_run[k]), k
    claimed, drained, arena = (int(x) for x in got["arena"])
    assert (claimed, drained) == (0, 0) and arena == sum(_full(p) for p in pairs)
    assert int(default_run["arena"][2]) < 0.6 * arena


@pytest.mark.gpu
def test_without_a_pool_the_drain_launches_serve_them(want, tmp_path):
    got = _run("mix", tmp_path, GDIET_BT_OVERFLOW_MB="0")
    _check(got, want["mix"], "pool 0")
    claimed, drained, arena = (int(x) for x in got["arena"])
    assert (claimed, drained) == (0, N_FALLBACK) and arena == sum(_half(p) for p in want["mix"][0])


@pytest.mark.gpu
def test_a_pool_for_five_of_the_twelve(want, tmp_path):
    pairs, _, _, _, ends = want["mix"]
    sizes = sorted(_full(p) for p, e in zip(pairs, ends) if e == 1000)
    assert len(sizes) == N_FALLBACK and 6 * sizes[0] > 5 * sizes[-1]  # whichever five claim first fit, no sixth does
    pool = sum(sizes[-5:])
    got = _run("mix", tmp_path, GDIET_BT_OVERFLOW_MB=repr(pool / 1048576.0))
    _check(got, want["mix"], "pool for five")
    claimed, drained, _ = (int(x) for x in got["arena"])
    assert claimed + drained == N_FALLBACK and claimed > 0 and drained > 0
    assert claimed == 5


@pytest.mark.gpu
def test_an_arena_of_half_the_need_takes_more_than_one_drain_launch(want, tmp_path):
    pairs, _, band, _, _ = want["fallback24"]
    assert band == (24, 0)
    got = _run("fallback24", tmp_path, GDIET_BT_OVERFLOW_MB="0")
    _check(got, want["fallback24"], "24 fall-backs, pool 0")
    claimed, drained, arena = (int(x) for x in got["arena"])
    assert (claimed, drained) == (0, 24) and arena == sum(_half(p) for p in pairs)
    # a launch serves what fits the arena: fewer than all 24, so at least two drain launches did real work
    assert arena // min(_full(p) for p in pairs) < 24


@pytest.mark.gpu
@pytest.mark.parametrize("pool", ["default", "0"])
def test_goldens(pool):
    """the hifi goldens mapped in a process of its own, with the default pool and with none: every SAM record as recorded"""
    env = {k: v for k, v in os.environ.items() if k not in ("GDIET_BT_COMPACT", "GDIET_BT_OVERFLOW_MB")}
    if pool != "default":
        env["GDIET_BT_OVERFLOW_MB"] = pool
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden_env_check.py"), "hifi", "hifi_sv", "hifi_rep"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_two_batches_in_flight_with_private_arenas():
    """hifi_sv as two batches in flight (submit, submit, wait, wait): each lane's small batch has an arena of its own"""
    env = {k: v for k, v in os.environ.items() if k not in ("GDIET_BT_COMPACT", "GDIET_BT_OVERFLOW_MB")}
    r = subprocess.run([sys.executable, os.path.join(HERE, "compact_arena_run.py"), "inflight", "hifi_sv"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]

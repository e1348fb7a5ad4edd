"""Seeded pairs and expectations for the tests of the 239-wide rung (tests/test_quarter_certificate.py, tests/test_quarter_band_gpu.py):
reads drawn by the benchmark's rules, the geometry grid of tests/emul/quarter_emul.cpp at GPU-test sizes, and what the ladder's counters
must be for a batch according to the planner's mark, the rung function and the certificate on the oracle's scores."""
import ctypes as C
import os
import subprocess

import numpy as np

from narrow_pairs import W_NARROW, pair_of_lengths

W_QUARTER = 239
BANDS = (239, 238, 237, 223, 119, 55)
MODS = (0, 1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15)


def bench_like_read(rng, mean=15000, sd=2000, lo=5000, hi=25000, sub=0.002, ins=0.001, dele=0.001):
    """a read against its origin window, by the rules of bench.py's HiFi reads: length N(15000, 2000) clipped to [5000, 25000],
    0.2 % substitutions, 0.1 % insertions, 0.1 % deletions"""
    n = int(min(max(rng.normal(mean, sd), lo), hi))
    t = rng.integers(0, 4, size=n, dtype=np.uint8)
    r = rng.random(n)
    out = t.copy()
    s = r < sub
    out[s] = (out[s] + rng.integers(1, 4, size=int(s.sum()))) & 3
    keep = ~((r >= sub) & (r < sub + dele))
    add = (r >= sub + dele) & (r < sub + dele + ins)
    pieces = np.where(add, 2, 1) * keep
    q = np.repeat(out, pieces)
    at = (np.cumsum(pieces) - pieces)[add & keep]
    q[at] = rng.integers(0, 4, size=len(at))
    return np.ascontiguousarray(q, np.uint8), t


def geometry_pairs():
    """the emulator's grid at 300-3000 bases: the six bands, tlen on and next to every quarter boundary, |tlen - qlen| in {0, 1, w - 1}
    (both signs), lengths a little above the band and at least 2 w + 200; Ns in every third target"""
    rng = np.random.default_rng(20261018)
    pairs, bands = [], []
    k = 0
    for w in BANDS:
        for mod in MODS:
            for delta in (0, 1, -1, w - 1, -(w - 1)):
                base = int(rng.integers(w + 80, w + 300)) if k % 2 else int(rng.integers(2 * w + 200, 2 * w + 900))
                tlen = (max(base, 300 + max(0, delta)) & ~15) + 16 + mod
                qlen = tlen - delta
                if qlen < 300:
                    tlen += (300 - qlen + 15) & ~15
                    qlen = tlen - delta
                assert 300 <= qlen <= 3000 and 300 <= tlen <= 3000 and tlen % 16 == mod
                pairs.append(pair_of_lengths(rng, qlen, tlen, 0.01 if k % 3 == 0 else 0.0))
                bands.append(w)
                k += 1
    return pairs, bands


def load_quarter_shim(tmpdir):
    """tests/emul/quarter_shim.cpp: the rung function and the planner's mark, compiled from the headers the kernel is compiled from"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(str(tmpdir), "libquarter_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(root, "genome-on-diet_amd", "csrc"),
                           os.path.join(root, "tests", "emul", "quarter_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.quarter_planned_rung.argtypes = [C.c_int] * 3
    assert lib.quarter_w() == W_QUARTER
    return lib


def expected_ladder(cert, qshim, oracle, pairs, ws, offered=True):
    """((tried, certified) of gdiet_hip_last_narrow_band, (tried 239, certified 239, tried 495, certified 495) of
    gdiet_hip_last_narrow_rungs, the band each pair finishes in) as the planner's mark, gd_quarter_rung and gd_band_certified on the
    oracle's scores at 239 and 495 give them (hifi scoring).  cert: narrow_pairs.load_cert_shim; offered: the launch offers the 239 rung"""
    gdo, lib = oracle
    a, b, q, e, q2, e2, amb = gdo.SCORINGS["hifi"]
    mat = gdo.score_matrix(a, b, sc_ambi=amb)
    band = [0, 0]
    rungs = [0, 0, 0, 0]
    ends = []
    for (qq, tt), w in zip(pairs, ws):
        w = int(w)
        mode = cert.cert_planned_mode(len(qq), len(tt), w)
        if mode == 0:
            ends.append(w)
            continue
        done = 0
        wq = qshim.quarter_planned_rung(len(qq), len(tt), w) if offered else 0
        if wq == w and wq:
            done = wq
        elif wq:
            s = gdo.oracle_extd2(lib, qq, tt, mat, q, e, q2, e2, wq)["score"]
            ok = bool(cert.cert_certified_for(wq, a, -b, amb, q, e, q2, e2, len(qq), len(tt), s))
            rungs[0] += 1
            rungs[1] += ok
            done = wq if ok else 0
        if not done:
            if mode == 2:
                done = w
            else:
                s = gdo.oracle_extd2(lib, qq, tt, mat, q, e, q2, e2, W_NARROW)["score"]
                ok = bool(cert.cert_certified_for(W_NARROW, a, -b, amb, q, e, q2, e2, len(qq), len(tt), s))
                rungs[2] += 1
                rungs[3] += ok
                done = W_NARROW if ok else 0
        if mode == 1:
            band[0] += 1
            band[1] += done > 0
        ends.append(done if done else w)
    return tuple(band), tuple(rungs), ends

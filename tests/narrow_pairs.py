"""Seeded query / target pairs for the narrow-band tests (tests/test_band_certificate.py, tests/test_narrow_band_gpu.py,
tests/test_narrow_scoring_gpu.py): the kinds of pair on which an alignment in a narrow band can differ from the one in the full band, and
the ordinary ones on which it cannot; the certificate of the 64-lane kernel behind ctypes, and what it predicts for a batch."""
import ctypes as C
import os
import subprocess

import numpy as np

W_NARROW = 495


def point_errors(rng, seq, err):
    """substitutions, single-base insertions and deletions, a third of `err` each (vectorised: the pairs are up to 9 kbp)"""
    seq = np.asarray(seq, np.uint8)
    r = rng.random(len(seq))
    sub = r < err / 3
    out = seq.copy()
    out[sub] = (out[sub] + rng.integers(1, 4, size=int(sub.sum()))) & 3
    keep = ~((r >= err / 3) & (r < 2 * err / 3))
    ins = (r >= 2 * err / 3) & (r < err)
    pieces = np.where(ins, 2, 1) * keep
    res = np.repeat(out, pieces)
    starts = np.cumsum(pieces) - pieces
    at = starts[ins & keep]
    res[at] = rng.integers(0, 4, size=len(at))
    return np.ascontiguousarray(res, np.uint8)


def hifi_like(rng, tlen, err, alphabet=4):
    t = rng.integers(0, alphabet, size=tlen, dtype=np.uint8)
    q = point_errors(rng, t, err)
    if alphabet < 4:
        q = np.minimum(q, alphabet - 1).astype(np.uint8)
    return q, t


def long_indels(rng, tlen, sizes, err=0.01):
    """the query with a block inserted (size > 0) or removed (size < 0) at spread-out places: two opposite ones of more than the band
    take the true path out of the band and back"""
    t = rng.integers(0, 4, size=tlen, dtype=np.uint8)
    q = point_errors(rng, t, err)
    n = len(sizes)
    for k, s in reversed(list(enumerate(sizes))):
        pos = int(len(q) * (k + 1) / (n + 1)) + int(rng.integers(-20, 21))
        if s > 0:
            q = np.concatenate([q[:pos], rng.integers(0, 4, size=s, dtype=np.uint8), q[pos:]])
        else:
            q = np.concatenate([q[:pos], q[pos - s:]])
    return np.ascontiguousarray(q, np.uint8), t


def tandem(rng, tlen, period, copies_t, copies_q, err=0.01):
    """a tandem array in the middle of the target with another copy number in the query: the gap can sit at either end of the array, or
    be split, and a band decides which placements exist"""
    unit = rng.integers(0, 4, size=period, dtype=np.uint8)
    flank = max(60, (tlen - period * copies_t) // 2)
    a, b = rng.integers(0, 4, size=flank, dtype=np.uint8), rng.integers(0, 4, size=flank, dtype=np.uint8)
    t = np.concatenate([a, np.tile(unit, copies_t), b])
    q = np.concatenate([point_errors(rng, a, err), point_errors(rng, np.tile(unit, copies_q), err), point_errors(rng, b, err)])
    return np.ascontiguousarray(q, np.uint8), np.ascontiguousarray(t, np.uint8)


def with_ns(rng, q, t, frac=0.01):
    q, t = q.copy(), t.copy()
    t[rng.random(len(t)) < frac] = 4
    q[rng.random(len(q)) < frac / 2] = 4
    return q, t


def certificate_mix(seed, n):
    """n pairs of 600-9000 bases: HiFi-like at 1-6 % error, one or two long indels of up to 450, tandem copy-number changes of period
    20-450, two-letter sequences, Ns"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        kind = i % 8
        tlen = int(rng.integers(600, 9001))
        if kind in (0, 1):
            q, t = hifi_like(rng, tlen, float(rng.choice([0.004, 0.01, 0.02, 0.04, 0.06])))
        elif kind == 2:
            q, t = long_indels(rng, tlen, [int(rng.integers(20, 451)) * int(rng.choice([-1, 1]))])
        elif kind == 3:
            s = int(rng.integers(60, 451))
            q, t = long_indels(rng, max(tlen, 1500), [s, -s + int(rng.integers(-10, 11))] if i & 8 else [-s, s + int(rng.integers(-10, 11))])
        elif kind == 4:
            period = int(rng.integers(20, 451))
            ct = int(rng.integers(2, 7))
            q, t = tandem(rng, tlen, period, ct, max(1, ct + int(rng.choice([-2, -1, 1, 2]))))
        elif kind == 5:
            period = int(rng.integers(130, 451))  # more than half of the middle band: a copy more or less moves the path by a band's worth
            ct = int(rng.integers(3, 6))
            q, t = tandem(rng, max(tlen, 2500), period, ct, ct + int(rng.choice([-2, -1, 1, 2])), err=0.02)
        elif kind == 6:
            q, t = hifi_like(rng, tlen, float(rng.choice([0.01, 0.03])), alphabet=2)
        else:
            q, t = with_ns(rng, *hifi_like(rng, tlen, 0.01), frac=float(rng.choice([0.005, 0.02])))
        out.append((q, t))
    return out


def band_edge_pair(rng, D, delta, insertion_first, tlen=1400, flank=8):
    """error-free, tlen - qlen == delta: the query lacks D + 1 target bases right after the first flank and carries D + 1 - delta random
    ones right before the last flank, so the best full-band path runs on diagonal t - q = D + 1 in between -- one beyond the band D --
    and comes back.  insertion_first: the mirror image (query and target change roles), diagonal -(D + 1)."""
    if insertion_first:
        t, q = band_edge_pair(rng, D, -delta, False, tlen, flank)
        return q, t
    t = rng.integers(0, 4, size=tlen, dtype=np.uint8)
    q = np.concatenate([t[:flank], t[flank + D + 1:tlen - flank], rng.integers(0, 4, size=D + 1 - delta, dtype=np.uint8), t[tlen - flank:]])
    assert len(t) - len(q) == delta
    return np.ascontiguousarray(q, np.uint8), t


def band_edge_pairs(seed, D=W_NARROW, deltas=(0, 37, -37, 300, -300)):
    """the ten pairs the bound of the certificate is measured on: each delta in both orientations (the mirror of a pair has a sequence of
    1400 - delta bases on the other side: nothing is longer than 1700)"""
    rng = np.random.default_rng(seed)
    return [band_edge_pair(rng, D, d, m) for d in deltas for m in (False, True)]


def max_off_diagonal(cigar):
    """the largest |t - q| along the path of a CIGAR (len << 4 | op; 1: insertion to the query, 2: deletion)"""
    d = far = 0
    for c in cigar:
        op, n = int(c) & 15, int(c) >> 4
        d += n if op == 2 else -n if op == 1 else 0
        far = max(far, abs(d))
    return far


def pair_of_lengths(rng, qlen, tlen, n_frac):
    """a target of tlen bases and a query of exactly qlen: 1 % point errors, then one block inserted or removed"""
    t = rng.integers(0, 4, size=tlen, dtype=np.uint8)
    q = point_errors(rng, t, 0.01)
    if len(q) < qlen:
        pos = int(rng.integers(0, len(q)))
        q = np.concatenate([q[:pos], rng.integers(0, 4, size=qlen - len(q), dtype=np.uint8), q[pos:]])
    elif len(q) > qlen:
        pos = int(rng.integers(0, qlen))
        q = np.concatenate([q[:pos], q[pos + len(q) - qlen:]])
    if n_frac:
        t = t.copy()
        t[rng.random(tlen) < n_frac] = 4
    return np.ascontiguousarray(q, np.uint8), t


def geometry_pairs():
    """bands at the admission limit and 1-2 below (and 247), tlen mod 16 in {0, 1, 7, 8, 9, 15}, |tlen - qlen| in {0, 1, w - 1, w},
    lengths 500-2100: around the band, and long enough for the paired steady rows; Ns in every third target"""
    rng = np.random.default_rng(20261018)
    pairs, bands = [], []
    k = 0
    for w in (W_NARROW, W_NARROW - 1, W_NARROW - 2, 247):
        for mod in (0, 1, 7, 8, 9, 15):
            for delta in (0, 1, -1, w - 1, -(w - 1), w, -w):
                base = int(rng.integers(w + 20, w + 200)) if k % 2 else int(rng.integers(max(2 * w + 200, 700), 2000))
                tlen = (base & ~15) + mod + (max(0, delta) if k % 2 == 0 else 0)
                tlen = min(max(tlen, abs(delta) + 120), 2100)
                tlen = (tlen & ~15) + mod if (tlen & ~15) + mod <= 2100 else ((tlen - 16) & ~15) + mod
                qlen = tlen - delta
                if qlen < 100 or qlen > 2100:
                    tlen = ((abs(delta) + 600) & ~15) + mod
                    qlen = tlen - delta
                pairs.append(pair_of_lengths(rng, qlen, tlen, 0.01 if k % 3 == 0 else 0.0))
                bands.append(w)
                k += 1
    return pairs, bands


def load_cert_shim(tmpdir):
    """tests/emul/cert_shim.cpp: gd_band_certified and the planner's mark, compiled from the headers the kernel is compiled from"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(str(tmpdir), "libcert_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(root, "genome-on-diet_amd", "csrc"),
                           os.path.join(root, "tests", "emul", "cert_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.cert_band_certified.argtypes = [C.c_int] * 11
    lib.cert_certified_for.argtypes = [C.c_int] * 11
    lib.cert_score_bias.argtypes = [C.c_int] * 7
    assert lib.cert_w_narrow() == W_NARROW
    return lib


def expected_counters(shim, oracle, pairs, w_full, scoring=None, flag=None):
    """(tried, certified) as the planner's mark and the certificate on the oracle's score at GD_W_NARROW give them.  scoring:
    (a, b, q, e, q2, e2, sc_ambi) as the caller passes it, default the hifi preset; the certificate sees the score the kernel computes,
    which is the oracle's minus the bias of a scoring whose larger gap model comes first; flag: the oracle's (queries with byte 7 need
    EZ_AVX512_SC, the score table of the kernel the library follows)"""
    gdo, lib = oracle
    a, b, q, e, q2, e2, amb = scoring if scoring is not None else gdo.SCORINGS["hifi"]
    mat = gdo.score_matrix(a, b, sc_ambi=amb)
    bias = shim.cert_score_bias(a, -b, amb, q, e, q2, e2)
    tried = cert = 0
    which = []
    for qq, tt in pairs:
        if shim.cert_planned_mode(len(qq), len(tt), w_full) != 1:  # (short ones go to the grouped kernels)
            which.append(None)
            continue
        tried += 1
        s = gdo.oracle_extd2(lib, qq, tt, mat, q, e, q2, e2, W_NARROW, flag=gdo.EZ_APPROX_MAX if flag is None else flag)["score"]
        c = bool(shim.cert_certified_for(W_NARROW, a, -b, amb, q, e, q2, e2, len(qq), len(tt), s - bias))
        cert += c
        which.append(c)
    return tried, cert, which

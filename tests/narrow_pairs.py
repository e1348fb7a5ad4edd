"""Seeded query / target pairs for the narrow-band tests (tests/test_band_certificate.py, tests/test_narrow_band_gpu.py): the kinds of
pair on which an alignment in a narrow band can differ from the one in the full band, and the ordinary ones on which it cannot."""
import numpy as np


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

"""Designed inputs for P1 -- mm_fix_cigar + mm_update_extra (LR/align.c:93-172,259-318; csrc/map_post.h and the two kernels
map_post_kernel / map_post_wave_kernel of csrc/map_kernels.hip.h) -- shared by oracle/pin_post.py, tests/test_post.py and
tests/test_post_gpu.py.

  cases()        the designed families: a list of dicts {family, q, t, cigar (raw uint32 words), n_cigar, score, sc (index into SCORINGS)}
  random_cases() fresh seeded alignments: random CIGARs over random sequences with about 10 % N, not produced by an aligner
  restate(case)  a plain restatement of the reference's two loops (Python float accumulator, numpy float32 mg_log2) that returns the
                 results and counts which branch a case takes, in the terms of the wave kernel's 64-base chunks where a condition is
                 about them
  coverage(...)  the counters of a set of cases summed: what tests/test_post.py asserts on the golden file

A slot is the raw CIGAR followed by one guard word.  Dead slots (score -0x40000000, n_cigar 0, n_cigar above the slot) must come back
untouched with an all-zero result.
"""
import numpy as np

NEG_INF = -0x40000000
GUARD = 0x5afe5afe
M, I, D, N = 0, 1, 2, 3
FIELDS = ("qshift", "tshift", "mlen", "blen", "dp_max", "n_ambi")


def matrix(a, b):
    m = np.zeros(25, np.int8)
    for i in range(4):
        for j in range(4):
            m[i * 5 + j] = a if i == j else -b
    return m


def _nonuniform():
    m = matrix(3, 5)
    v = [[5, -7, -2, -9], [-6, 4, -8, -3], [-1, -9, 6, -5], [-8, -2, -4, 3]]  # [target][query], not symmetric
    for i in range(4):
        for j in range(4):
            m[i * 5 + j] = v[i][j]
    return m


# (name, mat, q, e, log_gap): the presets' (a, b, q, e) -- hifi (1,4,6,2), ont (2,4,4,2), sr (2,8,12,2) -- each with and without the
# logarithmic gap cost; one large pair inside int8; a non-uniform 4 x 4 part; e = 0
SCORINGS = [("hifi_log", matrix(1, 4), 6, 2, 1), ("hifi_lin", matrix(1, 4), 6, 2, 0), ("ont_log", matrix(2, 4), 4, 2, 1), ("ont_lin", matrix(2, 4), 4, 2, 0),
            ("sr_lin", matrix(2, 8), 12, 2, 0), ("sr_log", matrix(2, 8), 12, 2, 1), ("large_log", matrix(100, 120), 90, 30, 1),
            ("large_lin", matrix(100, 120), 90, 30, 0), ("nonuni_lin", _nonuniform(), 7, 3, 0), ("nonuni_log", _nonuniform(), 7, 3, 1),
            ("e0_log", matrix(1, 4), 6, 0, 1), ("e0_lin", matrix(2, 4), 5, 0, 0), ("step_e1", matrix(1, 4), 4, 1, 1), ("step_e3", matrix(1, 4), 4, 3, 1)]
SC = {s[0]: i for i, s in enumerate(SCORINGS)}


def mg_log2(x):
    """LR/mmpriv.h:146-157 in float32 operations, one rounding each"""
    z = np.array([x], np.float32).view(np.uint32)
    log_2 = np.float32(int((z[0] >> 23) & 255) - 128)
    z[0] = (int(z[0]) & ~(255 << 23) & 0xffffffff) + (127 << 23)
    f = z.view(np.float32)[0]
    t = np.float32(-0.34484843) * f
    t = t + np.float32(2.02466578)
    t = t * f
    t = t - np.float32(0.67487759)
    return np.float32(log_2 + t)


_gap_memo = {}


def gap_cost(q, e, log_gap, length):
    key = (q, e, log_gap, length)
    if key not in _gap_memo:
        _gap_memo[key] = float(q) + float(e) * float(mg_log2(np.float32(1.0) + np.float32(length))) if log_gap else float(q + e)
    return _gap_memo[key]


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def restate_fix(cg, q, t, cnt):
    """mm_fix_cigar on a list of words; returns (words, qshift, tshift) and counts its branches in cnt"""
    cg = [int(c) for c in cg]
    n = len(cg)
    if n <= 1:
        cnt["fix_early_n%d" % n] += 1
        return cg, 0, 0
    if cg[0] & 0xf == I:
        cnt["fix_lead_I_input"] += 1
    if cg[0] & 0xf == D:
        cnt["fix_lead_D_input"] += 1
    for k in range(n):
        if cg[k] >> 4 == 0:
            cnt["fix_zero_" + ("front" if k == 0 else "last" if k == n - 1 else "inside")] += 1
    for k in range(1, n - 1):
        if cg[k] & 0xf == N and cg[k - 1] & 0xf in (I, D) and cg[k + 1] & 0xf in (I, D):
            cnt["fix_N_between_indels"] += 1
    toff = qoff = 0
    shrink = False
    for k in range(n):
        op, ln = cg[k] & 0xf, cg[k] >> 4
        if ln == 0:
            shrink = True
        if op == M:
            toff += ln
            qoff += ln
        elif op in (I, D):
            if 0 < k < n - 1 and cg[k - 1] & 0xf == M and cg[k + 1] & 0xf == M:
                prev = cg[k - 1] >> 4
                s, o = (q, qoff) if op == I else (t, toff)
                l = 0
                while l < prev and s[o - 1 - l] == s[o + ln - 1 - l]:
                    l += 1
                if l > 0:
                    cg[k - 1] -= l << 4
                    cg[k + 1] += l << 4
                    qoff -= l
                    toff -= l
                if ln > 0 and prev > 0:
                    if 0 < l < prev:
                        cnt["fix_shift_part_" + "MID"[op]] += 1
                    if l == prev:
                        cnt["fix_shift_full_" + "MID"[op]] += 1
                        if k == 1:
                            cnt["fix_shift_empties_first_M_" + "MID"[op]] += 1
                if l == prev:
                    shrink = True
            if op == I:
                qoff += ln
            else:
                toff += ln
        elif op == N:
            toff += ln
    k = 0
    while k + 2 < n:
        if cg[k] & 0xf > 0 and (cg[k] & 0xf) + (cg[k + 1] & 0xf) == 3:
            s = [0, 0, 0]
            l = k
            zero_inside = False
            while l < n:
                op = cg[l] & 0xf
                if op in (I, D) or cg[l] >> 4 == 0:
                    assert op < 3, "a zero-length operation above D inside an indel run writes past s[] in the reference"
                    s[op] += cg[l] >> 4
                    zero_inside |= cg[l] >> 4 == 0 and l > k
                else:
                    break
                l += 1
            if s[1] > 0 and s[2] > 0 and l - k > 2:
                cnt["fix_merge_" + ("IDI" if cg[k] & 0xf == I else "DID")] += 1
                if l - k > 3:
                    cnt["fix_merge_longer"] += 1
                if zero_inside:
                    cnt["fix_merge_zero_inside"] += 1
                cg[k], cg[k + 1] = s[1] << 4 | I, s[2] << 4 | D
                for j in range(k + 2, l):
                    cg[j] &= 0xf
                shrink = True
            elif l - k == 2:
                cnt["fix_pair_not_merged"] += 1
            k = l
        k += 1
    if shrink:
        cg = [c for c in cg if c >> 4]
        out = []
        for k in range(len(cg)):
            if k == len(cg) - 1 or cg[k] & 0xf != cg[k + 1] & 0xf:
                out.append(cg[k])
            else:
                cnt["fix_equal_neighbours"] += 1
                cg[k + 1] += cg[k] >> 4 << 4
        cg = out
    qshift = tshift = 0
    if cg and cg[0] & 0xf in (I, D):
        if cg[0] & 0xf == I:
            qshift = cg[0] >> 4
            cnt["fix_lead_I_removed"] += 1
        else:
            tshift = cg[0] >> 4
            cnt["fix_lead_D_removed"] += 1
        cg = cg[1:]
    return cg, qshift, tshift


class Counter(dict):
    def __missing__(self, k):
        return 0


def restate(case, scoring=None):
    """(result dict, Counter) of one live case: the reference's loops, and what happened in them"""
    _, mat, gq, ge, log_gap = scoring if scoring is not None else SCORINGS[case["sc"]]
    cnt = Counter()
    q, t = case["q"], case["t"]
    cg, qshift, tshift = restate_fix(case["cigar"][:case["n_cigar"]], q, t, cnt)
    q, t = q[qshift:], t[tshift:]
    matl = [int(x) for x in mat]
    s = mx = 0.0
    qoff = toff = blen = mlen = n_ambi_tot = 0
    attain = []  # (run, chunk, lane) of every base at which the running score equals the maximum so far and is positive
    n_runs = sum(1 for c in cg if c & 0xf == M)
    run = -1
    prev_odd = None
    for k, c in enumerate(cg):
        op, ln = c & 0xf, c >> 4
        if op == M:
            run += 1
            cnt["run_len_%d" % ln] += 1
            if prev_odd is not None:
                cnt["run_len_%d_behind_odd_%s" % (ln, prev_odd)] += 1
            prev_odd = None
            n_ambi = n_diff = 0
            qs, ts = q[qoff:qoff + ln].tolist(), t[toff:toff + ln].tolist()
            clamp_chunks = set()
            for base in range(0, ln, 64):
                # the chunk as the wave kernel sees it: S and MX at its entry, the peak in front of its first clamp and the peak behind one
                s_in, mx_in = s, mx
                clamped = False
                pre_peak = post_peak = None
                for l in range(base, min(base + 64, ln)):
                    cq, ct = qs[l], ts[l]
                    if ct > 3 or cq > 3:
                        n_ambi += 1
                    elif ct != cq:
                        n_diff += 1
                    a = matl[ct * 5 + cq] if ct * 5 + cq < 25 else 0  # (query byte 7 against a target N: past the matrix, taken as 0)
                    s += a
                    if s < 0:
                        s = 0.0
                        clamped = True
                        cnt["clamp_lane_%d" % (l - base)] += 1
                        clamp_chunks.add(base // 64)
                    else:
                        if s == 0 and a < 0:
                            cnt["exact_zero"] += 1
                        if s >= mx and s > 0:
                            if s > mx:
                                attain = []
                            attain.append((run, base // 64, l - base))
                        mx = max(mx, s)
                        if clamped:
                            post_peak = s if post_peak is None else max(post_peak, s)
                        else:
                            pre_peak = s if pre_peak is None else max(pre_peak, s)
                    if s_in != int(s_in) and l - base in (0, 63):
                        cnt["frac_state_at_seam"] += 1
                m1 = mx_in
                if pre_peak is not None and int(pre_peak) == int(mx_in) and (pre_peak != int(pre_peak) or mx_in != int(mx_in)):
                    cnt["tie_frac_" + ("larger" if pre_peak > mx_in else "smaller" if pre_peak < mx_in else "equal")] += 1
                if pre_peak is not None:
                    m1 = max(m1, pre_peak)
                if post_peak is not None and post_peak == int(m1) and m1 != int(m1):
                    cnt["tie_restart_reaches_int_of_frac_max"] += 1
            for c0 in clamp_chunks:
                if c0 + 1 in clamp_chunks:
                    cnt["clamps_in_consecutive_chunks"] += 1
            blen += ln - n_ambi
            mlen += ln - n_ambi - n_diff
            n_ambi_tot += n_ambi
            cnt["ambi_in_M_q"] += sum(1 for x, y in zip(qs, ts) if x > 3 and y <= 3)
            cnt["ambi_in_M_t"] += sum(1 for x, y in zip(qs, ts) if y > 3 and x <= 3)
            cnt["ambi_in_M_both"] += sum(1 for x, y in zip(qs, ts) if x > 3 and y > 3)
            toff += ln
            qoff += ln
        elif op in (I, D):
            src = q[qoff:qoff + ln] if op == I else t[toff:toff + ln]
            na = int((src > 3).sum())
            if ln and src[0] > 3:
                cnt["ambi_first_of_%s_%d" % ("MID"[op], ln)] += 1
            if ln and src[-1] > 3:
                cnt["ambi_last_of_%s_%d" % ("MID"[op], ln)] += 1
            blen += ln - na
            n_ambi_tot += na
            s -= gap_cost(gq, ge, log_gap, ln)
            if s < 0:
                s = 0.0
                cnt["clamp_at_gap"] += 1
            if op == I:
                qoff += ln
            else:
                toff += ln
            prev_odd = "MID"[op] if ln & 1 else None
        elif op == N:
            toff += ln
            prev_odd = None
    assert qoff <= len(q) and toff <= len(t)
    for r, ch, lane in attain:
        cnt["max_lane_%d" % lane] += 1
        if r < n_runs - 1:
            cnt["max_in_run_not_last"] += 1
    if len(attain) >= 2:
        cnt["max_attained_twice"] += 1
    for (r0, c0, l0), (r1, c1, l1) in zip(attain, attain[1:]):
        if r0 == r1 and c1 == c0 + 1 and l0 == 63 and l1 == 0:
            cnt["max_on_both_sides_of_a_seam"] += 1
    frac = mx - int(mx)
    if frac:
        cnt["final_frac"] += 1
        if 0.496 <= frac < 0.501:
            cnt["final_frac_just_below_step"] += 1
        if 0.501 <= frac <= 0.506:
            cnt["final_frac_just_above_step"] += 1
    cnt["ops_%s" % ("ge1000" if len(cg) >= 1000 else "lt1000")] += 1
    res = dict(cigar=np.array(cg, np.uint32), qshift=qshift, tshift=tshift, mlen=mlen, blen=blen, dp_max=int(mx + .499), n_ambi=n_ambi_tot, max=mx)
    return res, cnt


def is_dead(case):
    return case["score"] == NEG_INF or case["n_cigar"] <= 0 or case["n_cigar"] > len(case["cigar"])


def coverage(cases, scorings=None):
    tot = Counter()
    for c in cases:
        if is_dead(c):
            tot["dead"] += 1
            continue
        _, cnt = restate(c, None if scorings is None else scorings[c["sc"]])
        for k, v in cnt.items():
            tot[k] += v
    return tot


# ---- building alignments ---------------------------------------------------------------------------------------------------------------
class Builder:
    """query, target and raw CIGAR grown operation by operation.  An M is a string over = (match) X (mismatch) q / t / b (code 4 in the
    query / the target / both); an indel takes its length, the places of code 4 inside it, and the left shift mm_fix_cigar is to find for
    it: 0 unless asked for (the run's last base is made to differ from the base in front of it)"""

    def __init__(self, rng):
        self.rng, self.q, self.t, self.cg = rng, [], [], []

    def m(self, sym):
        if isinstance(sym, (int, np.integer)):
            sym = "=" * int(sym)
        for ch in sym:
            b = int(self.rng.integers(0, 4))
            o = (b + 1 + int(self.rng.integers(0, 3))) & 3
            cq, ct = {"=": (b, b), "X": (b, o), "q": (4, b), "t": (b, 4), "b": (4, 4)}[ch]
            self.q.append(cq)
            self.t.append(ct)
        self.cg.append(len(sym) << 4 | M)
        return self

    def gap(self, op, n, ambi=(), shift=0):
        own, other = (self.q, self.t) if op == I else (self.t, self.q)
        P = len(own)
        run = [int(x) for x in self.rng.integers(0, 4, n)]
        own.extend(run)
        if n:
            if shift:  # own[i] == own[i + n] for the `shift` bases in front of the run, and not one further
                prev = self.cg[-1] >> 4
                assert self.cg[-1] & 0xf == M and shift <= prev and not ambi
                for i in range(P - shift + n, P + n):
                    own[i] = own[i - n]
                if shift < prev:
                    j = P - shift - 1 + n
                    if own[j] == own[P - shift - 1]:
                        own[j] = (own[j] + 1) & 3 if own[P - shift - 1] < 4 else 0
                    for i in range(j + n, P + n, n):
                        own[i] = own[i - n]
                for i in range(P - shift, P):  # the M in front stays a run of matches
                    other[len(other) - (P - i)] = own[i]
            elif P and own[P + n - 1] == own[P - 1]:
                own[P + n - 1] = (own[P - 1] + 1) & 3 if own[P - 1] < 4 else 0
            for a in ambi:
                own[P + a] = 4
        self.cg.append(n << 4 | op)
        return self

    def i(self, n, **kw):
        return self.gap(I, n, **kw)

    def d(self, n, **kw):
        return self.gap(D, n, **kw)

    def skip(self, n):
        self.t.extend(int(x) for x in self.rng.integers(0, 4, n))
        self.cg.append(n << 4 | N)
        return self

    def case(self, family, sc="hifi_log", score=100):
        return dict(family=family, q=np.array(self.q, np.uint8), t=np.array(self.t, np.uint8), cigar=np.array(self.cg, np.uint32), n_cigar=len(self.cg),
                    score=score, sc=SC[sc] if isinstance(sc, str) else sc)


def walk(a, b, length, clamps=(), peak=None, rng=None):
    """an M string of `length` for the uniform matrix (a, -b) from score 0: the score stays within [0, b], dips below 0 exactly at the
    places in `clamps` (each an X at a score below b), touches 0 only by an X at score exactly b; with peak = p, everything up to p is a
    match and nothing behind p reaches the score at p again"""
    out, s = [], 0
    if peak is not None:
        out = ["="] * (peak + 1)
        s = (peak + 1) * a
        top = s
        while len(out) < length:
            if s - b >= 0 and s + a >= top or len(out) == peak + 1:
                out.append("X")
                s = max(s - b, 0)
            elif s + a < top:
                out.append("=")
                s += a
            else:
                out.append("X")
                s = max(s - b, 0)
        return "".join(out)
    for p in range(length):
        if p in clamps:
            assert s < b, (p, s)
            out.append("X")
            s = 0
        elif p + 1 in clamps and s < b and s + a >= b:
            out.append("b")  # (hold: the next place must find a score below b)
        elif s + a <= b:
            out.append("=")
            s += a
        elif s == b:
            out.append("X")
            s = 0
        else:
            out.append("b")
    return "".join(out)


SEAM_LENS = (1, 2, 63, 64, 65, 127, 128, 129, 192, 193)
GAP_LENS = (1, 63, 64, 65, 130)


def find_gap(q, e, want, lo=1, hi=400):
    """the gap length in [lo, hi] whose cost under the logarithmic model leaves 1 - frac(cost) nearest to `want` from the named side:
    want = (low, high): the first length with low <= 1 - frac < high"""
    for n in range(lo, hi):
        c = gap_cost(q, e, 1, n)
        f = 1.0 - (c - int(c))
        if want[0] <= f < want[1]:
            return n
    raise ValueError("no gap length leaves a fraction in %r" % (want,))


def cases():
    rng = np.random.default_rng(20260101)
    out = []
    B = lambda: Builder(rng)  # noqa: E731

    def rnd_m(n, px=0.08, pn=0.0):
        r = rng.random(n)
        return "".join("X" if x < px else ("qtb"[int(x * 1e6) % 3] if x < px + pn else "=") for x in r)

    # -- chunk seams: every length alone, behind an odd I and behind an odd D (qoff / toff unaligned), at more than one scoring
    for sc in ("hifi_log", "ont_lin", "nonuni_log", "large_log", "sr_lin", "e0_log", "hifi_lin", "e0_lin"):
        for n in SEAM_LENS:
            out.append(B().m(rnd_m(n)).case("seam_alone", sc))
            out.append(B().m(rnd_m(7)).i(3).m(rnd_m(n)).case("seam_behind_I", sc))
            out.append(B().m(rnd_m(9)).d(5).m(rnd_m(n)).case("seam_behind_D", sc))
            out.append(B().m(rnd_m(n)).i(1).m(rnd_m(n)).d(7).m(rnd_m(n)).case("seam_chain", sc))
    # -- the clamp at every lane of a chunk, in the first and in a later chunk; exact zeros come with the walk
    for sc, a, b in (("hifi_log", 1, 4), ("ont_lin", 2, 4), ("sr_log", 2, 8)):
        for lane in range(64):
            for chunk in (0, 1, 2):
                if (lane + chunk) % 3 and sc != "hifi_log":
                    continue
                p = 64 * chunk + lane
                out.append(B().m(walk(a, b, p + 1 + (lane * 7) % 50, clamps=(p,)) + "=" * 5).case("clamp_lane", sc))
        for l0, l1 in ((5, 70), (63, 64), (0, 127), (40, 100), (63, 127), (10, 64)):
            out.append(B().m(walk(a, b, 140, clamps=(l0, l1)) + "===").case("clamp_two_chunks", sc))
            out.append(B().m(20).d(3).m(walk(a, b, 200, clamps=(l0, l1, l1 + 64))).case("clamp_two_chunks", sc))
    # -- the maximum at every lane; on both sides of a seam; in a run that is not the last; twice
    for sc, a, b in (("hifi_log", 1, 4), ("ont_log", 2, 4), ("large_lin", 100, 120)):
        for lane in range(64):
            for chunk in (0, 1, 2):
                if (lane + chunk) % 3 and sc != "hifi_log":
                    continue
                p = 64 * chunk + lane
                out.append(B().m(walk(a, b, p + 2 + (lane * 11) % 70, peak=p)).case("max_lane", sc))
                if lane % 8 == chunk:
                    out.append(B().m(walk(a, b, p + 20, peak=p)).i(2).m(walk(a, b, 30, clamps=(3,))).case("max_not_last_run", sc))
        for p in (63, 127, 191):  # the last base of a chunk, then a base of score 0 on the first of the next: attained on both
            out.append(B().m("=" * (p + 1) + "b" + "X" * 9).case("max_seam_both", sc))
            out.append(B().m("=" * (p + 1) + "q" + "X" * 3 + "=" * 2).case("max_seam_both", sc))
            out.append(B().m("=" * (p + 2) + "X" * 5).case("max_seam_first", sc))
        per = "X" + "=" * (b // a) if b % a == 0 else None
        for k in (5, 60, 64, 100, 130) if per else ():  # attained, lost by one mismatch, attained again by b / a matches
            out.append(B().m("=" * k + per * 2 + "X" * 4).case("max_twice", sc))
            out.append(B().m("=" * k + "X").d(2).m("=" * 70 + "X" * 3).case("max_twice_runs", sc))
    # -- fractional ties under the logarithmic gap cost
    for sc, a, b in (("hifi_log", 1, 4), ("ont_log", 2, 4), ("step_e3", 1, 4)):
        _, _, gq, ge, _ = SCORINGS[SC[sc]]
        g_hi = find_gap(gq, ge, (0.55, 0.98))   # leaves a fraction well above the .501 step
        g_hi2 = find_gap(gq, ge, (0.55, 0.98), g_hi + 1)
        g_lo = find_gap(gq, ge, (0.02, 0.45))
        for rep in range(6):
            k = 40 + 2 * rep + (64 if rep % 2 else 0)
            k += k % a
            for op in (I, D):
                def up(g):  # matches that bring the score behind a gap of length g back to the integer part it had in front of it
                    c = gap_cost(gq, ge, 1, g)
                    return -(-int(np.ceil(c)) // a) if a > 1 else int(np.ceil(c))
                pad = "b" * (3 + 9 * rep)
                # larger: the standing maximum k (no fraction) met again with the fraction the gap left
                out.append(B().m(k).gap(op, g_hi).m("=" * up(g_hi) + "X" * 3).case("tie_larger", sc))
                out.append(B().m(k).gap(op, g_lo).m(pad + "=" * up(g_lo) + "X" * 3).case("tie_larger", sc))
                # smaller: a maximum with a large fraction, then a second gap that leaves a smaller one
                x = B().m(k).gap(op, g_hi).m("=" * up(g_hi) + pad).gap(op, g_lo)
                c2 = gap_cost(gq, ge, 1, g_lo) + gap_cost(gq, ge, 1, g_hi)
                f1 = 1 - (gap_cost(gq, ge, 1, g_hi) % 1)
                # the score is now k + f1 - cost(g_lo): climb to integer part k again
                s_now = k * a + up(g_hi) * a - c2 if a == 1 else None
                if a == 1:
                    need = int(np.floor(k + f1)) - int(np.floor(s_now))
                    f2 = s_now % 1
                    out.append(x.m("=" * need + "X" * 4).case("tie_smaller" if f2 < f1 else "tie_larger", sc))
                # equal: down by one mismatch and up again by b / a matches, in the next chunk or run
                if b % a == 0:
                    out.append(B().m(k).gap(op, g_hi).m("=" * up(g_hi) + "b" * (64 - up(g_hi) % 64) + "X" + "=" * (b // a) + "X" * 3).case("tie_equal", sc))
                    out.append(B().m(k).gap(op, g_hi2).m("=" * up(g_hi2) + "X").skip(5).m("=" * (b // a) + "X" * 2).case("tie_equal", sc))
                # a clamp drops the fraction the gap left: a new maximum behind it is an integer, whatever the fraction was
                out.append(B().m(k).gap(op, g_hi).m("X" * (k * a // b + 2) + "=" * (70 + k + 9 * rep)).case("clamp_drops_fraction", sc))
                # a restart from a clamp reaches the integer part of a maximum that carries a fraction: clamp and climb inside one chunk
                c = gap_cost(gq, ge, 1, g_hi)
                for kr in range(int(np.ceil(c)) + 1 + rep, int(np.ceil(c)) + 3 + rep):
                    kr += (kr * a) % a
                    top = kr * a + up(g_hi) * a - c
                    if int(top) % a == 0 and up(g_hi) + int(top) // b + 2 + int(top) // a <= 60:
                        out.append(B().m(kr).gap(op, g_hi).m("=" * up(g_hi) + "X" * (int(top) // b + 2) + "=" * (int(top) // a) + "X" * 3).case("tie_restart", sc))
                        out.append(B().m(kr).gap(op, g_hi).m("=" * up(g_hi) + "X" * (int(top) // b + 2)).gap(op, 1).m("=" * (int(top) // a) + "X").case("tie_restart_run", sc))
    # -- the .499 step: a final maximum whose fraction lies just below and just above .501 (one long deletion; the generator searches)
    for sc in ("step_e1", "step_e3", "hifi_log", "ont_log"):
        _, _, gq, ge, _ = SCORINGS[SC[sc]]
        a = int(SCORINGS[SC[sc]][1][0])
        below, above = [], []
        for n in range(1, 4000):
            c = gap_cost(gq, ge, 1, n)
            f = 1.0 - (c - int(c))
            if 0.496 <= f < 0.501:
                below.append((0.501 - f, n))
            elif 0.501 <= f <= 0.506:
                above.append((f - 0.501, n))
        for lst in (sorted(below)[:3], sorted(above)[:3]):
            for _, n in lst:
                out.append(B().m(60).d(n).m(60).case("step_499", sc))
        for _, n in sorted(below)[:1] + sorted(above)[:1]:
            if n < 700:
                out.append(B().m(70).i(n).m(66).case("step_499", sc))
    # -- ambiguous bases: in M (query, target, both) and at the first and last base of I / D runs (the ballot loops)
    for sc in ("hifi_log", "sr_lin", "nonuni_lin"):
        for n in (5, 64, 65, 130):
            out.append(B().m(rnd_m(n, 0.1, 0.3)).case("ambi_M", sc))
            out.append(B().m("q" + rnd_m(n, 0.1, 0.1) + "t").i(2).m("b" + rnd_m(n) + "b").case("ambi_M", sc))
        for g in GAP_LENS:
            for op in (I, D):
                for am in ((0,), (g - 1,), (0, g - 1), tuple(range(0, g, 3))):
                    out.append(B().m(rnd_m(20)).gap(op, g, ambi=am).m(rnd_m(30)).case("ambi_gap", sc))
    # -- mm_fix_cigar
    for rep in range(6):
        sc = ("hifi_log", "ont_lin", "sr_lin", "large_log", "nonuni_log", "e0_log")[rep]
        r = 3 + 5 * rep
        out.append(B().m(rnd_m(r + 60 * (rep % 3))).case("fix_n1", sc))
        out.append(B().m(0).m(rnd_m(r)).i(2).m(rnd_m(r)).case("fix_zero_front", sc))
        out.append(B().i(0).m(rnd_m(r)).d(2).m(rnd_m(9)).case("fix_zero_front", sc))
        out.append(B().m(rnd_m(r)).i(0).m(rnd_m(r)).case("fix_zero_inside", sc))
        out.append(B().m(rnd_m(r)).d(0).m(rnd_m(70)).i(3).m(0).m(5).case("fix_zero_inside", sc))
        out.append(B().m(rnd_m(r)).d(4).m(rnd_m(r)).i(0).case("fix_zero_last", sc))
        out.append(B().m(rnd_m(r)).i(1).m(rnd_m(r)).m(0).case("fix_zero_last", sc))
        for op in (I, D):
            g = 1 + rep
            out.append(B().m(r + 10).gap(op, g, shift=1 + rep).m(rnd_m(r)).case("fix_shift_part", sc))
            out.append(B().m(r + 70).gap(op, g, shift=r + 3).m(rnd_m(64)).case("fix_shift_part", sc))
            # l == prev_len: the M vanishes; in front of it an indel of the same kind (the neighbours merge), of the other kind, or nothing
            out.append(B().m(rnd_m(r)).gap(op, 2).m(r).gap(op, g, shift=r).m(rnd_m(r)).case("fix_shift_full_merge", sc))
            out.append(B().m(rnd_m(r)).gap(3 - op, 2).m(r).gap(op, g, shift=r).m(rnd_m(r)).case("fix_shift_full_other", sc))
            out.append(B().m(r).gap(op, g, shift=r).m(rnd_m(r + 60)).case("fix_shift_empties_first", sc))
            out.append(B().m(r + 1).gap(op, g + 64, shift=r + 1).m(rnd_m(r)).d(1).m(4).case("fix_shift_empties_first", sc))
            # runs of I and D
            o = 3 - op
            out.append(B().m(rnd_m(r)).gap(op, 5).gap(o, 6).gap(op, 7).m(rnd_m(r)).case("fix_merge3", sc))
            out.append(B().m(rnd_m(r)).gap(op, 1).gap(o, 2).gap(op, 3).gap(o, 4).gap(o, 1).m(rnd_m(r)).case("fix_merge_longer", sc))
            out.append(B().m(rnd_m(r)).gap(op, 2).gap(o, 3).gap(op, 0).gap(o, 65).m(rnd_m(r)).case("fix_merge_zero_inside", sc))
            out.append(B().m(rnd_m(r)).gap(op, 2).m(0).gap(o, 3).gap(op, 1).m(rnd_m(r)).case("fix_merge_zero_inside", sc))
            out.append(B().m(rnd_m(r)).gap(op, 2 + rep).gap(o, 3).m(rnd_m(r)).case("fix_pair", sc))
            out.append(B().m(rnd_m(r)).gap(op, 2).gap(op, 3 + rep).m(rnd_m(r)).m(rnd_m(4)).case("fix_equal_neighbours", sc))
            out.append(B().m(rnd_m(r)).gap(op, 2).skip(7 + rep).gap(o, 3).m(rnd_m(r)).case("fix_N_between", sc))
            out.append(B().m(rnd_m(r)).gap(op, 2).skip(7).gap(op, 3).gap(o, 1).m(rnd_m(r)).case("fix_N_between", sc))
            out.append(B().gap(op, 1 + rep).m(rnd_m(r + 64)).case("fix_lead_input", sc))
            out.append(B().gap(op, 3).m(rnd_m(r)).gap(o, 2).m(rnd_m(r)).case("fix_lead_input", sc))
    # -- length: ~20 kbp with ~2 000 operations, and one perfect 40 000-base match at the large a
    for sc in ("hifi_log", "ont_log", "large_log"):
        x = B()
        for j in range(1000):
            x.m(rnd_m(int(rng.integers(1, 40)), 0.05, 0.01))
            if j < 999:
                x.gap(I if rng.random() < 0.5 else D, int(rng.integers(1, 6)) if rng.random() < 0.95 else int(rng.integers(60, 140)))
        out.append(x.case("long_20k", sc))
    x = B().m(40000)
    x.t = list(x.q)
    out.append(x.case("long_perfect_40k", "large_log"))
    # -- dead slots
    for rep in range(5):
        live = B().m(rnd_m(10 + rep)).i(2).m(rnd_m(70))
        out.append(live.case("dead_neg_inf", "hifi_log", score=NEG_INF))
        c = B().m(rnd_m(10 + rep)).d(2).m(rnd_m(5)).case("dead_over_cap", "hifi_log")
        c["n_cigar"] = len(c["cigar"]) + 2 + rep  # (above the slot: raw words + the guard word)
        out.append(c)
        c = B().m(rnd_m(10 + rep)).case("dead_n0", "hifi_log")
        c["n_cigar"] = 0
        out.append(c)
        c = B().case("fix_n0", ("hifi_log", "ont_lin", "sr_lin", "large_log", "nonuni_log")[rep])  # (the reference returns early; a dead slot on the device)
        out.append(c)
    return out


def random_cases(n=2000, seed=77):
    """random CIGARs over random sequences, about 10 % code 4, with the odd zero-length operation, N operation and indel run"""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(n):
        x = Builder(rng)
        n_ops = int(rng.integers(1, 14))
        for k in range(n_ops):
            r = rng.random()
            ln = int(rng.integers(0, 4)) if rng.random() < 0.05 else int(rng.choice((1, 2, 3, 5, 17, 40, 63, 64, 65, 100, 129, 200)))
            if k == n_ops - 1 or r < 0.5:
                x.q.extend(int(v) for v in rng.integers(0, 4, ln))
                if rng.random() < 0.5:  # related sequences, 10 % mismatches
                    x.t.extend((v + (int(rng.integers(1, 4)) if rng.random() < 0.1 else 0)) & 3 for v in x.q[len(x.q) - ln:])
                else:
                    x.t.extend(int(v) for v in rng.integers(0, 2, ln))
                x.cg.append(ln << 4 | M)
            elif r < 0.72:
                x.q.extend(int(v) for v in rng.integers(0, 2, min(ln, 70)))  # (two letters: left shifts are common)
                x.cg.append(min(ln, 70) << 4 | I)
            elif r < 0.94:
                x.t.extend(int(v) for v in rng.integers(0, 2, min(ln, 70)))
                x.cg.append(min(ln, 70) << 4 | D)
            elif ln:
                x.skip(ln)
        c = x.case("random", int(rng.integers(0, len(SCORINGS))))
        for s in (c["q"], c["t"]):
            s[rng.random(len(s)) < 0.1] = 4
        if sum(w >> 4 for w in c["cigar"] if w & 0xf == M) == 0:
            continue  # (nothing but gaps: the CIGAR would vanish)
        try:
            restate_fix(c["cigar"], c["q"], c["t"], Counter())
        except AssertionError:
            continue  # (a zero-length N inside an indel run: undefined in the reference)
        out.append(c)
    return out


# ---- the emulator's file formats (tests/emul/post_emul.cpp) and the layout of a batch --------------------------------------------------
def write_emul_input(path, cases, scorings=None):
    scorings = SCORINGS if scorings is None else scorings
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for c in cases:
            _, mat, gq, ge, lg = scorings[c["sc"]]
            cap = len(c["cigar"])
            f.write(np.array([c["n_cigar"], cap, len(c["q"]), len(c["t"]), c["score"], gq, ge, lg], np.int32).tobytes())
            f.write(np.asarray(mat, np.int8).tobytes() + b"\0\0\0")
            f.write(np.asarray(c["cigar"], np.uint32).tobytes())
            f.write(c["q"].tobytes() + c["t"].tobytes())


def read_emul_output(path, cases):
    """per case three dicts -- thread form, wave form lanes 0..63, wave form lanes 63..0 -- of n_cigar, the six fields, slot (all its words)"""
    a = np.fromfile(path, np.int32)
    out, p = [], 0
    for c in cases:
        cap = len(c["cigar"])
        rec = []
        for _ in range(3):
            h = a[p:p + 7]
            rec.append(dict(n_cigar=int(h[0]), slot=a[p + 7:p + 7 + cap].view(np.uint32).copy(), **{k: int(v) for k, v in zip(FIELDS, h[1:])}))
            p += 7 + cap
        out.append(rec)
    assert p == len(a), "the emulator's output has another length than its input asks for"
    return out


def layout(cases):
    """the arrays of one gdiet_hip_post_batch call: slots back to back, each the raw words and one guard word"""
    qoff = np.zeros(len(cases) + 1, np.int64)
    toff, coff = qoff.copy(), qoff.copy()
    for i, c in enumerate(cases):
        qoff[i + 1], toff[i + 1], coff[i + 1] = qoff[i] + len(c["q"]), toff[i] + len(c["t"]), coff[i] + len(c["cigar"]) + 1
    cat = lambda k, dt: np.concatenate([c[k] for c in cases]).astype(dt) if cases else np.zeros(0, dt)  # noqa: E731
    pool = np.full(int(coff[-1]), GUARD, np.uint32)
    for i, c in enumerate(cases):
        pool[coff[i]:coff[i] + len(c["cigar"])] = c["cigar"]
    return dict(qseq=cat("q", np.uint8), qoff=qoff, tseq=cat("t", np.uint8), toff=toff, cigar=pool, coff=coff,
                n_cigar=np.array([c["n_cigar"] for c in cases], np.int32), score=np.array([c["score"] for c in cases], np.int32))


def read_emul_input(path):
    """(cases, scorings) of a file in the emulator's input format, e.g. what tests/emul/map_host_main.cpp --dump-post writes"""
    raw = open(path, "rb").read()
    n = int(np.frombuffer(raw, np.int32, 1)[0])
    p, cases, scorings, index = 4, [], [], {}
    for _ in range(n):
        h = np.frombuffer(raw, np.int32, 8, p)
        mat = np.frombuffer(raw, np.int8, 25, p + 32)
        p += 60
        nc, cap, ql, tl = (int(x) for x in h[:4])
        cg = np.frombuffer(raw, np.uint32, cap, p).copy()
        p += 4 * cap
        q, t = np.frombuffer(raw, np.uint8, ql, p).copy(), np.frombuffer(raw, np.uint8, tl, p + ql).copy()
        p += ql + tl
        key = (mat.tobytes(), int(h[5]), int(h[6]), int(h[7]))
        if key not in index:
            index[key] = len(scorings)
            scorings.append(("dump%d" % len(scorings), mat.copy(), int(h[5]), int(h[6]), int(h[7])))
        cases.append(dict(family="dump", q=q, t=t, cigar=cg, n_cigar=nc, score=int(h[4]), sc=index[key]))
    assert p == len(raw)
    return cases, scorings


def load_golden(path):
    """(cases, refs, scorings) of tests/golden/update_extra.npz: refs[i] = the reference's dict(cigar, qshift, ...) for cases[i]"""
    with np.load(path) as f:
        z = {k: f[k] for k in f.files}
    fam, scn = [str(x) for x in z["family_names"]], [str(x) for x in z["sc_names"]]
    scorings = [(scn[i], z["sc_mat"][i].copy(), int(z["sc_qel"][i][0]), int(z["sc_qel"][i][1]), int(z["sc_qel"][i][2])) for i in range(len(scn))]
    cases, refs = [], []
    for i in range(len(z["n_cigar"])):
        cases.append(dict(family=fam[int(z["family"][i])], q=z["q"][z["qo"][i]:z["qo"][i + 1]], t=z["t"][z["to"][i]:z["to"][i + 1]],
                          cigar=z["cigar"][z["co"][i]:z["co"][i + 1]], n_cigar=int(z["n_cigar"][i]), score=int(z["score"][i]), sc=int(z["sc"][i])))
        refs.append(dict(cigar=z["ref_cigar"][z["ref_co"][i]:z["ref_co"][i + 1]], **{k: int(v) for k, v in zip(FIELDS, z["ref_out"][i])}))
    return cases, refs, scorings

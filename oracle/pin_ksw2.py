#!/usr/bin/env python3
"""Pin the ksw2 oracle (oracle/gdo_ksw2.c) against the reference itself and (re)generate the committed golden
vectors tests/golden/ksw2_extd2.npz, ksw2_extz2.npz, exact_match.npz and, over gdo.SCORINGS, ksw2_scoring.npz.

Runs only where oracle/_ref has been built from /root/reference (this container).  The golden vectors hold
inputs + the REFERENCE's outputs (ksw_extd2_sse / ksw_extz2_sse / exact_match_sse called through ctypes), so the
GPU box and later rounds can re-check both the oracle and the HIP kernels without the reference.

    python oracle/pin_ksw2.py --fuzz 3000          # differential fuzz only (oracle vs SSE vs AVX-512)
    python oracle/pin_ksw2.py --write-golden       # also rewrite tests/golden/*.npz
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gdo  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(gdo.HERE), "tests", "golden")


def cases(rng, n, heavy=True):
    """yield (tag, query, target, preset, w, zdrop, end_bonus, flag)"""
    for i in range(n):
        kind = i % 12
        preset = ("sr", "hifi", "ont")[i % 3]
        flag = gdo.EZ_APPROX_MAX
        zdrop, end_bonus = -1, 0
        if kind == 0:  # SR shape: 150x150, w=150
            q, t = gdo.make_pair(rng, 150, 0.01, 0.0005, 0.0005)
            preset, w = "sr", 150
        elif kind == 1:  # long-ish, moderate band
            tl = int(rng.integers(300, 2500 if heavy else 900))
            q, t = gdo.make_pair(rng, tl, 0.002, 0.001, 0.001)
            w = int(rng.integers(20, 400))
        elif kind == 2:  # band-edge stress: one indel of 0.4-0.6 w
            tl = int(rng.integers(400, 2000 if heavy else 900))
            w = int(rng.integers(40, 300))
            sz = int(w * rng.uniform(0.4, 0.62)) * (1 if rng.random() < 0.5 else -1)
            q, t = gdo.make_pair(rng, tl, 0.01, 0.002, 0.002, big_indel=sz)
        elif kind == 3:  # Ns in both
            tl = int(rng.integers(100, 1200))
            q, t = gdo.make_pair(rng, tl, 0.02, 0.005, 0.005, n_frac=0.02)
            w = int(rng.integers(10, 300))
        elif kind == 4:  # tiny
            tl = int(rng.integers(1, 40))
            q, t = gdo.make_pair(rng, tl, 0.05, 0.03, 0.03)
            w = int(rng.integers(0, 40))
        elif kind == 5:  # qlen != tlen, band may be exhausted (st > en)
            tl = int(rng.integers(50, 600))
            q, t = gdo.make_pair(rng, tl, 0.02, 0.01, 0.01, trim=int(rng.integers(0, tl // 2 + 1)))
            w = int(rng.integers(1, 120))
        elif kind == 6:  # unrelated sequences (path wanders to band edges)
            q = rng.integers(0, 4, size=int(rng.integers(20, 700)), dtype=np.uint8)
            t = rng.integers(0, 4, size=int(rng.integers(20, 700)), dtype=np.uint8)
            w = int(rng.integers(5, 200))
        elif kind == 7:  # w multiple of 16 and lengths multiple of 16 (alignment corner cases)
            tl = 16 * int(rng.integers(1, 60))
            q, t = gdo.make_pair(rng, tl, 0.01, 0.0, 0.0)
            w = 16 * int(rng.integers(1, 20))
        elif kind == 8:  # exact-max + z-drop / extension-only flags (oracle generality; not on the live path)
            tl = int(rng.integers(30, 500))
            q, t = gdo.make_pair(rng, tl, 0.05, 0.02, 0.02)
            w = int(rng.integers(10, 200))
            flag = int(rng.choice([0, gdo.EZ_EXTZ_ONLY, gdo.EZ_RIGHT, gdo.EZ_REV_CIGAR, gdo.EZ_SCORE_ONLY,
                                   gdo.EZ_APPROX_MAX | gdo.EZ_APPROX_DROP, gdo.EZ_APPROX_MAX | gdo.EZ_RIGHT,
                                   gdo.EZ_EXTZ_ONLY | gdo.EZ_RIGHT | gdo.EZ_REV_CIGAR, gdo.EZ_GENERIC_SC]))
            zdrop = int(rng.choice([-1, 20, 100, 400]))
            end_bonus = int(rng.choice([0, 5]))
        elif kind == 9:  # HiFi-like geometry at reduced length: w close to the length
            tl = int(rng.integers(800, 3000 if heavy else 1200))
            q, t = gdo.make_pair(rng, tl, 0.002, 0.001, 0.001)
            preset, w = "hifi", 1000
        elif kind == 10:  # ONT-like noise
            tl = int(rng.integers(300, 2000 if heavy else 900))
            q, t = gdo.make_pair(rng, tl, 0.03, 0.02, 0.02)
            preset, w = "ont", int(rng.integers(100, 1300))
        else:  # full matrix (w < 0)
            tl = int(rng.integers(10, 300))
            q, t = gdo.make_pair(rng, tl, 0.03, 0.02, 0.02)
            w = -1
        yield ("k%d" % kind, q, t, preset, w, zdrop, end_bonus, flag)


WIDE_AT = ("sr", "ont", "bound120_last", "skey_corner", "a16", "wrap_2_8_60_3", "k3_2_32_40_2")
SC_CLASSES = ("sr", "group", "lane64", "wide", "misc", "k3")


def scoring_cases(rng, name):
    """yield (class, query, target, w) for one scoring of gdo.SCORINGS: the shapes each kernel form takes -- short-read 150 x 150
    (one exact copy among them), the grouped widths (targets around 128 / 160 / 256), 64-lane lengths, for a few scorings the wide
    ONT band, and band-edge / N stress"""
    for i in range(4):
        q, t = gdo.make_pair(rng, 150, 0.02, 0.003, 0.003, n_frac=0.01 if i == 2 else 0.0)
        n = min(len(q), len(t))
        q, t = (t[:150].copy(), t[:150]) if i == 0 else (q[:n], t[:n])
        yield "sr", q, t, 150
    for tl in (120, 155, 250):
        q, t = gdo.make_pair(rng, tl, 0.03, 0.006, 0.006)
        yield "group", q, t, 150
    for _ in range(2):
        tl = int(rng.integers(300, 3000))
        q, t = gdo.make_pair(rng, tl, 0.01, 0.003, 0.003)
        yield "lane64", q, t, int(rng.integers(100, 500))
    if name in WIDE_AT:
        q, t = gdo.make_pair(rng, int(rng.integers(1500, 2500)), 0.03, 0.02, 0.02)
        yield "wide", q, t, 1300
    tl = int(rng.integers(300, 900))
    w = int(rng.integers(40, 200))
    q, t = gdo.make_pair(rng, tl, 0.01, 0.002, 0.002, big_indel=int(w * rng.uniform(0.4, 0.62)) * (1 if rng.random() < 0.5 else -1))
    yield "misc", q, t, w
    q, t = gdo.make_pair(rng, int(rng.integers(60, 600)), 0.05, 0.02, 0.02, n_frac=0.03)
    yield "misc", q, t, int(rng.integers(10, 300))


SC_KEYS = ("score", "zdropped", "max", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "reach_end")


def k3_cases(ref, rng, name, want=3, tries=3000):
    """yield ("k3", query, target, w): divergent pairs in narrow bands at one of the table's k3_* scorings on which the reference's own
    ksw_extz2_sse and ksw_extd2_sse(q,e,q,e) differ (they differ in a few pairs in a hundred, so a fixed shape set would miss them)"""
    a, b, go, ge, _, _, amb = gdo.SCORINGS[name]
    mat = gdo.score_matrix(a, b, sc_ambi=amb)
    n = 0
    for _ in range(tries):
        tl, w = int(rng.integers(30, 400)), int(rng.integers(10, 200))
        q, t = gdo.make_pair(rng, tl, 0.05, 0.03, 0.03)
        if not gdo.same(gdo.ref_extz2(ref, q, t, mat, go, ge, w), gdo.ref_extd2(ref, q, t, mat, go, ge, go, ge, w)):
            yield "k3", q, t, w
            n += 1
            if n == want:
                return


def pin_scorings(ora, ref, seed):
    """every scoring of gdo.SCORINGS: the reference's ksw_extd2_sse, ksw_extd2_avx512 (byte-7 queries), ksw_extz2_sse in APPROX_MAX and in
    exact mode against the oracle; returns (mismatches, golden records, pairs where ksw_extz2 != ksw_extd2(q,e,q,e))"""
    rng = np.random.default_rng(seed + 2000)
    n_bad = n_k3 = n_avx_k3 = 0
    gold = []
    for si, (name, (a, b, go, ge, go2, ge2, amb)) in enumerate(gdo.SCORINGS.items()):
        mat = gdo.score_matrix(a, b, sc_ambi=amb)
        shapes = list(scoring_cases(rng, name))
        if name.startswith("k3_"):
            k3 = list(k3_cases(ref, rng, name))
            if not k3:
                n_bad += 1
                print("NO PAIR where ksw_extz2 != ksw_extd2(q,e,q,e) found at", name)
            shapes += k3
        for ci, (cls, q, t, w) in enumerate(shapes):
            r = gdo.ref_extd2(ref, q, t, mat, go, ge, go2, ge2, w)
            o = gdo.oracle_extd2(ora, q, t, mat, go, ge, go2, ge2, w)
            q7 = q.copy()
            if ci % 2 and len(q7) > 4 and cls != "k3":  # (k3 pairs: no byte-7 queries, see DESIGN.md "Scorings")
                q7[rng.integers(0, len(q7), size=max(1, len(q7) // 100))] = 7
            v = gdo.ref_extd2(ref, q7, t, mat, go, ge, go2, ge2, w, fn="ksw_extd2_avx512")
            o7 = gdo.oracle_extd2(ora, q7, t, mat, go, ge, go2, ge2, w, flag=gdo.EZ_APPROX_MAX | gdo.EZ_AVX512_SC)
            rz = gdo.ref_extz2(ref, q, t, mat, go, ge, w)
            oz = gdo.oracle_extz2(ora, q, t, mat, go, ge, w)
            flag_x, zdrop_x, eb_x = (0, gdo.EZ_EXTZ_ONLY)[ci % 2], (-1, 100, 400)[ci % 3], (0, 5)[ci % 2]
            rx = gdo.ref_extz2(ref, q, t, mat, go, ge, w, zdrop_x, eb_x, flag_x)
            ox = gdo.oracle_extz2(ora, q, t, mat, go, ge, w, zdrop_x, eb_x, flag_x)
            for what, x, y in (("extd2", o, r), ("extd2_avx512", o7, v), ("extz2", oz, rz), ("extz2_exact", ox, rx)):
                if what == "extd2_avx512" and cls == "k3":
                    # the pairs picked because the band-edge padding cells decide them: there ksw_extd2_avx512, whose windows are
                    # 64-cell aligned, can differ from ksw_extd2_sse (16-cell), and the oracle models the SSE windows only
                    n_avx_k3 += not gdo.same(x, y, SC_KEYS)
                    continue
                if not gdo.same(x, y, SC_KEYS):
                    n_bad += 1
                    if n_bad <= 5:
                        print("MISMATCH scoring", name, what, cls, len(q), len(t), w, {k: (x[k], y[k]) for k in SC_KEYS if x[k] != y[k]})
            n_k3 += not gdo.same(rz, gdo.ref_extd2(ref, q, t, mat, go, ge, go, ge, w))
            gold.append((si, cls, q, q7, t, w, flag_x, zdrop_x, eb_x, r, v, rz, rx))
    print("k3 pairs where ksw_extd2_avx512 differs from the oracle (SSE windows): %d" % n_avx_k3)
    return n_bad, gold, n_k3


def write_scoring_golden(path, gold):
    def pack(seqs, dt=np.uint8):
        offs = np.zeros(len(seqs) + 1, np.int64)
        offs[1:] = np.cumsum([len(x) for x in seqs])
        return (np.concatenate(seqs).astype(dt) if seqs else np.zeros(0, dt)), offs
    out = {}
    out["q"], out["qo"] = pack([g[2] for g in gold])
    out["q7"], _ = pack([g[3] for g in gold])
    out["t"], out["to"] = pack([g[4] for g in gold])
    out["params"] = np.array([[g[0], SC_CLASSES.index(g[1]), g[5], g[6], g[7], g[8]] for g in gold], np.int32)
    out["scorings"] = np.array(list(gdo.SCORINGS.values()), np.int32)
    out["scoring_names"] = np.array(list(gdo.SCORINGS.keys()))
    for key, k in (("extd2", 9), ("extd2_avx512", 10), ("extz2", 11), ("extz2_exact", 12)):
        out[key + "_cigar"], out[key + "_cigar_off"] = pack([g[k]["cigar"].view(np.uint8) for g in gold])
        out[key + "_scalars"] = np.array([[g[k][f] for f in SC_KEYS] for g in gold], np.int64)
    np.savez_compressed(path, **out)


def identity_sweep(ref, pairs=24, seed=11):
    """ksw_extz2_sse(q,e) against ksw_extd2_sse(q,e,q,e) on `pairs` pairs at every single-affine scoring with a <= 16, b <= 40,
    q <= 40, e <= 20 that gd_consts accepts, split by gdo.wave_scoring_ok: (scorings taken, of them differing), (refused, differing)"""
    rng = np.random.default_rng(seed)
    ps = []
    for i in range(pairs):
        q, t = gdo.make_pair(rng, int(rng.integers(30, 400)), 0.05, 0.03, 0.03, n_frac=0.01 if i % 5 == 0 else 0)
        ps.append((q, t, int(rng.integers(10, 200)) if i % 4 else -1))
    cnt = {True: [0, 0], False: [0, 0]}
    for a in range(1, 17):
        for b in range(1, 41):
            for go in range(0, 41):
                for ge in range(1, 21):
                    if 2 * (go + ge) > 127 or b > 2 * (go + ge):
                        continue
                    ok = gdo.wave_scoring_ok(a, b, go, ge, go, ge)
                    mat = gdo.score_matrix(a, b)
                    bad = any(not gdo.same(gdo.ref_extz2(ref, q, t, mat, go, ge, w), gdo.ref_extd2(ref, q, t, mat, go, ge, go, ge, w)) for q, t, w in ps)
                    cnt[ok][0] += 1
                    cnt[ok][1] += bad
    return cnt[True], cnt[False]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--identity-sweep", action="store_true", help="only the ksw_extz2 / ksw_extd2(q,e,q,e) sweep (minutes)")
    ap.add_argument("--fuzz", type=int, default=1200)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--write-golden", action="store_true")
    args = ap.parse_args()

    gdo.build_oracle()
    ora = gdo.load_oracle()
    ref = gdo.load_ref("lr_avx")
    if args.identity_sweep:
        (n_ok, bad_ok), (n_no, bad_no) = identity_sweep(ref)
        print("single-affine scorings the wave forms take: %d, ksw_extz2 != ksw_extd2(q,e,q,e) at %d; refused: %d, differing at %d"
              % (n_ok, bad_ok, n_no, bad_no))
        return 1 if bad_ok else 0
    rng = np.random.default_rng(args.seed)

    n_bad_sse = n_bad_avx = n_sse_vs_avx = 0
    gold = []
    gold_avx = []
    for idx, (tag, q, t, preset, w, zdrop, end_bonus, flag) in enumerate(cases(rng, args.fuzz)):
        a, b, go, ge, go2, ge2 = gdo.PRESETS[preset]
        mat = gdo.score_matrix(a, b)
        o = gdo.oracle_extd2(ora, q, t, mat, go, ge, go2, ge2, w, zdrop, end_bonus, flag)
        r = gdo.ref_extd2(ref, q, t, mat, go, ge, go2, ge2, w, zdrop, end_bonus, flag)
        keys = ("score", "zdropped", "max", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "reach_end")
        if not gdo.same(o, r, keys):
            n_bad_sse += 1
            if n_bad_sse <= 5:
                print("MISMATCH oracle vs SSE", idx, tag, len(q), len(t), preset, w, flag, zdrop,
                      {k: (o[k], r[k]) for k in keys if o[k] != r[k]}, len(o["cigar"]), len(r["cigar"]))
        if flag == gdo.EZ_APPROX_MAX:  # the AVX-512 port is only used (and only valid) in the live-path mode
            # the parity target's kernel; the oracle reproduces its score table with GDO_EZ_AVX512_SC.  Every third
            # pair gets some query bytes 7 (= N of a reverse-complemented read, LR/map.c:1634), where SSE and AVX-512 differ.
            q7 = q.copy()
            if idx % 3 == 0 and len(q7) > 4:
                pos7 = rng.integers(0, len(q7), size=max(1, len(q7) // 100))
                q7[pos7] = 7
                run = int(rng.integers(0, len(q7) - 3))
                q7[run:run + int(rng.integers(1, 40))] = 7
            v = gdo.ref_extd2(ref, q7, t, mat, go, ge, go2, ge2, w, zdrop, end_bonus, flag, fn="ksw_extd2_avx512")
            o7 = gdo.oracle_extd2(ora, q7, t, mat, go, ge, go2, ge2, w, zdrop, end_bonus, flag | gdo.EZ_AVX512_SC)
            if not gdo.same(o7, v):
                n_bad_avx += 1
                if n_bad_avx <= 5:
                    print("MISMATCH oracle(AVX512_SC) vs ksw_extd2_avx512", idx, tag, len(q), len(t), preset, w, o7["score"], v["score"])
            r7 = gdo.ref_extd2(ref, q7, t, mat, go, ge, go2, ge2, w, zdrop, end_bonus, flag)
            if not gdo.same(r7, v):
                n_sse_vs_avx += 1
            if idx < 360:
                gold_avx.append((q7, t, preset, w, zdrop, end_bonus, flag, v))
        # extz2 (single affine) on the same pair
        oz = gdo.oracle_extz2(ora, q, t, mat, go, ge, w, zdrop, end_bonus, flag)
        rz = gdo.ref_extz2(ref, q, t, mat, go, ge, w, zdrop, end_bonus, flag)
        if not gdo.same(oz, rz, keys):
            n_bad_sse += 1
            if n_bad_sse <= 5:
                print("MISMATCH extz2 oracle vs SSE", idx, tag, len(q), len(t), preset, w, flag,
                      {k: (oz[k], rz[k]) for k in keys if oz[k] != rz[k]})
        if idx < 360:
            gold.append((q, t, preset, w, zdrop, end_bonus, flag, r, rz))
    # exact match
    n_bad_em = 0
    em = []
    for i in range(400):
        n = int(rng.integers(1, 300))
        t = rng.integers(0, 5, size=n, dtype=np.uint8)
        q = t.copy()
        if i % 3:
            q[int(rng.integers(0, n))] ^= 1
        mat = gdo.score_matrix(2, 8)
        if gdo.oracle_exact_match(ora, q, t) != gdo.ref_exact_match(ref, q, t, mat):
            n_bad_em += 1
        if i < 60:
            em.append((q, t, gdo.ref_exact_match(ref, q, t, mat)))
    # exact-maximum mode of ksw_extz2 (flag 0 / KSW_EZ_EXTZ_ONLY, with and without z-drop): what gdiet_hip_ksw_extz2_batch_ex answers
    n_bad_exact = 0
    gold_exact = []
    rng = np.random.default_rng(args.seed + 1000)  # (a stream of its own: these vectors do not depend on --fuzz)
    for i in range(1200 if args.fuzz >= 1000 else 300):
        preset = ("sr", "hifi", "ont")[i % 3]
        a, b, go, ge, _, _ = gdo.PRESETS[preset]
        mat = gdo.score_matrix(a, b)
        tlen = int(rng.integers(20, 420))
        t = rng.integers(0, 4, size=tlen, dtype=np.uint8)
        if i % 9 == 0:
            t[rng.integers(0, tlen, size=max(1, tlen // 50))] = 4
        q = t.copy()
        m = rng.random(tlen) < (0.02 if i % 2 else 0.08)
        q[m] = (q[m] + rng.integers(1, 4, size=int(m.sum()))) & 3
        q = q[rng.random(len(q)) >= 0.01]
        if i % 4 == 1 and len(q) > 60:  # a long indel or an unrelated tail: z-drop / a maximum inside the matrix
            cut = int(rng.integers(20, len(q) - 20))
            q = np.concatenate([q[:cut], rng.integers(0, 4, size=int(rng.integers(5, 80)), dtype=np.uint8), q[cut:]]) if i % 8 == 1 else \
                np.concatenate([q[:cut], rng.integers(0, 4, size=len(q) - cut, dtype=np.uint8)])
        if len(q) == 0:
            q = t[:1].copy()
        w = int(rng.integers(8, 200)) if i % 5 else -1
        zdrop = (-1, 20, 100, 400)[(i // 3) % 4]
        end_bonus = (0, 5)[(i // 12) % 2]
        flag = (0, gdo.EZ_EXTZ_ONLY)[(i // 24) % 2]
        oz = gdo.oracle_extz2(ora, q, t, mat, go, ge, w, zdrop, end_bonus, flag)
        rz = gdo.ref_extz2(ref, q, t, mat, go, ge, w, zdrop, end_bonus, flag)
        keys = ("score", "zdropped", "max", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "reach_end")
        if not gdo.same(oz, rz, keys):
            n_bad_exact += 1
            if n_bad_exact <= 5:
                print("MISMATCH extz2 exact mode oracle vs SSE", i, len(q), len(t), preset, w, flag, zdrop, {k: (oz[k], rz[k]) for k in keys if oz[k] != rz[k]})
        if i < 300:
            gold_exact.append((q, t, preset, w, zdrop, end_bonus, flag, rz))
    n_bad_sse += n_bad_exact
    n_bad_sc, gold_sc, n_k3 = pin_scorings(ora, ref, args.seed)
    n_bad_sse += n_bad_sc
    print("scoring table: %d scorings, %d pairs, oracle_vs_reference_mismatch=%d (ksw_extz2 != ksw_extd2(q,e,q,e) in %d pairs)"
          % (len(gdo.SCORINGS), len(gold_sc), n_bad_sc, n_k3))
    print("extz2 exact-maximum mode: pairs=%d oracle_vs_sse_mismatch=%d (z-dropped in %d of the %d golden pairs)"
          % (1200 if args.fuzz >= 1000 else 300, n_bad_exact, sum(1 for g in gold_exact if g[7]["zdropped"]), len(gold_exact)))
    print("pairs=%d oracle_vs_sse_mismatch=%d oracle_vs_avx512_mismatch=%d sse_vs_avx512_differ_on_byte7_inputs=%d exact_match_mismatch=%d"
          % (args.fuzz, n_bad_sse, n_bad_avx, n_sse_vs_avx, n_bad_em))

    if args.write_golden:
        os.makedirs(GOLDEN, exist_ok=True)

        def pack(seqs):
            offs = np.zeros(len(seqs) + 1, np.int64)
            offs[1:] = np.cumsum([len(s) for s in seqs])
            return (np.concatenate(seqs).astype(np.uint8) if seqs else np.zeros(0, np.uint8)), offs

        qs, qo = pack([g[0] for g in gold])
        ts, to = pack([g[1] for g in gold])
        params = np.array([[("sr", "hifi", "ont").index(g[2]), g[3], g[4], g[5], g[6]] for g in gold], np.int32)
        for name, k in (("ksw2_extd2", 7), ("ksw2_extz2", 8)):
            cg, co = pack([g[k]["cigar"].view(np.uint8) for g in gold])
            scal = np.array([[g[k][f] for f in ("score", "zdropped", "max", "max_q", "max_t", "mqe", "mqe_t", "mte",
                                                  "mte_q", "reach_end")] for g in gold], np.int64)
            np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), q=qs, qo=qo, t=ts, to=to, params=params,
                                cigar_bytes=cg, cigar_off=co, scalars=scal)
        qs7, qo7 = pack([g[0] for g in gold_avx])
        ts7, to7 = pack([g[1] for g in gold_avx])
        params7 = np.array([[("sr", "hifi", "ont").index(g[2]), g[3], g[4], g[5], g[6]] for g in gold_avx], np.int32)
        cg7, co7 = pack([g[7]["cigar"].view(np.uint8) for g in gold_avx])
        scal7 = np.array([[g[7][f] for f in ("score", "zdropped", "max", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q",
                                             "reach_end")] for g in gold_avx], np.int64)
        np.savez_compressed(os.path.join(GOLDEN, "ksw2_extd2_avx512.npz"), q=qs7, qo=qo7, t=ts7, to=to7, params=params7,
                            cigar_bytes=cg7, cigar_off=co7, scalars=scal7)
        qsx, qox = pack([g[0] for g in gold_exact])
        tsx, tox = pack([g[1] for g in gold_exact])
        paramsx = np.array([[("sr", "hifi", "ont").index(g[2]), g[3], g[4], g[5], g[6]] for g in gold_exact], np.int32)
        cgx, cox = pack([g[7]["cigar"].view(np.uint8) for g in gold_exact])
        scalx = np.array([[g[7][f] for f in ("score", "zdropped", "max", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q",
                                             "reach_end")] for g in gold_exact], np.int64)
        np.savez_compressed(os.path.join(GOLDEN, "ksw2_extz2_exact.npz"), q=qsx, qo=qox, t=tsx, to=tox, params=paramsx,
                            cigar_bytes=cgx, cigar_off=cox, scalars=scalx)
        eq, eqo = pack([e[0] for e in em])
        et, eto = pack([e[1] for e in em])
        np.savez_compressed(os.path.join(GOLDEN, "exact_match.npz"), q=eq, qo=eqo, t=et, to=eto,
                            expect=np.array([e[2] for e in em], np.int32))
        write_scoring_golden(os.path.join(GOLDEN, "ksw2_scoring.npz"), gold_sc)
        print("golden vectors written to", GOLDEN)
    return 1 if (n_bad_sse or n_bad_em) else 0


if __name__ == "__main__":
    sys.exit(main())

"""CPU: the oracle (oracle/gdo_ksw2.c) reproduces the reference's outputs stored in tests/golden/."""
import numpy as np

from golden_io import SCALARS, SCORING_OUTPUTS, load_exact, load_ksw, load_scoring


def test_extd2_oracle_matches_reference_golden(oracle):
    gdo, lib = oracle
    cases = load_ksw("ksw2_extd2")
    assert len(cases) >= 300
    for c in cases:
        a, b, q, e, q2, e2 = gdo.PRESETS[c["preset"]]
        o = gdo.oracle_extd2(lib, c["q"], c["t"], gdo.score_matrix(a, b), q, e, q2, e2, c["w"], c["zdrop"], c["end_bonus"], c["flag"])
        for k in SCALARS:
            assert o[k] == c[k], (k, o[k], c[k], c["preset"], c["w"], c["flag"])
        assert np.array_equal(o["cigar"], c["cigar"])


def test_extz2_oracle_matches_reference_golden(oracle):
    gdo, lib = oracle
    for c in load_ksw("ksw2_extz2"):
        a, b, q, e, q2, e2 = gdo.PRESETS[c["preset"]]
        o = gdo.oracle_extz2(lib, c["q"], c["t"], gdo.score_matrix(a, b), q, e, c["w"], c["zdrop"], c["end_bonus"], c["flag"])
        for k in SCALARS:
            assert o[k] == c[k], (k, o[k], c[k])
        assert np.array_equal(o["cigar"], c["cigar"])


def test_extz2_exact_mode_oracle_matches_reference_golden(oracle):
    """flag 0 / KSW_EZ_EXTZ_ONLY with and without z-drop (tests/golden/ksw2_extz2_exact.npz): the oracle the exact-maximum GPU
    kernel is fuzzed against reproduces ksw_extz2_sse's scalars and CIGARs"""
    gdo, lib = oracle
    cases = load_ksw("ksw2_extz2_exact")
    assert len(cases) >= 300 and sum(c["zdropped"] for c in cases) >= 20
    for c in cases:
        a, b, q, e, q2, e2 = gdo.PRESETS[c["preset"]]
        o = gdo.oracle_extz2(lib, c["q"], c["t"], gdo.score_matrix(a, b), q, e, c["w"], c["zdrop"], c["end_bonus"], c["flag"])
        for k in SCALARS:
            assert o[k] == c[k], (k, o[k], c[k])
        assert np.array_equal(o["cigar"], c["cigar"])


def test_exact_match_oracle_matches_reference_golden(oracle):
    gdo, lib = oracle
    cases = load_exact()
    assert any(e for _, _, e in cases) and any(not e for _, _, e in cases)
    for q, t, expect in cases:
        assert gdo.oracle_exact_match(lib, q, t) == expect


def test_cigar_consumes_both_sequences(oracle):
    """size-independent property: a reported global alignment consumes exactly qlen and tlen"""
    gdo, lib = oracle
    rng = np.random.default_rng(99)
    for _ in range(60):
        q, t = gdo.make_pair(rng, int(rng.integers(50, 900)), 0.02, 0.01, 0.01)
        a, b, go, ge, go2, ge2 = gdo.PRESETS["hifi"]
        o = gdo.oracle_extd2(lib, q, t, gdo.score_matrix(a, b), go, ge, go2, ge2, 200)
        if o["score"] == gdo.NEG_INF:
            assert len(o["cigar"]) == 0
            continue
        ops, lens = o["cigar"] & 0xf, o["cigar"] >> 4
        assert lens[(ops == 0) | (ops == 1)].sum() == len(q)
        assert lens[(ops == 0) | (ops == 2)].sum() == len(t)


def test_self_alignment_is_all_match(oracle):
    gdo, lib = oracle
    rng = np.random.default_rng(5)
    for n in (1, 15, 16, 17, 150, 1000):
        t = rng.integers(0, 4, size=n, dtype=np.uint8)
        a, b, go, ge, go2, ge2 = gdo.PRESETS["sr"]
        o = gdo.oracle_extd2(lib, t, t, gdo.score_matrix(a, b), go, ge, go2, ge2, 150)
        assert o["score"] == n * a and list(o["cigar"]) == [n << 4]


def test_extz2_equals_extd2_with_equal_gap_models(oracle):
    """the identity K3 rests on (include/gdiet_hip.h): in APPROX_MAX mode ksw_extz2(q,e) and ksw_extd2(q,e,q,e) give the same
    score, CIGAR and band-exhaustion status -- checked on the oracle (pinned to the reference) and, for the golden extz2
    vectors, on ksw_extz2_sse's own outputs"""
    gdo, lib = oracle
    import pin_ksw2
    rng = np.random.default_rng(31)
    n = 0
    for tag, q, t, preset, w, zdrop, eb, flag in pin_ksw2.cases(rng, 900, heavy=False):
        if flag != gdo.EZ_APPROX_MAX or zdrop != -1:
            continue
        a, b, go, ge, _, _ = gdo.PRESETS[preset]
        mat = gdo.score_matrix(a, b)
        z = gdo.oracle_extz2(lib, q, t, mat, go, ge, w)
        d = gdo.oracle_extd2(lib, q, t, mat, go, ge, go, ge, w)
        assert z["score"] == d["score"] and z["zdropped"] == d["zdropped"] and np.array_equal(z["cigar"], d["cigar"]), (tag, len(q), len(t), w)
        n += 1
    assert n > 700
    for c in load_ksw("ksw2_extz2"):
        if c["flag"] != 8 or c["zdrop"] != -1:
            continue
        a, b, go, ge, _, _ = gdo.PRESETS[c["preset"]]
        d = gdo.oracle_extd2(lib, c["q"], c["t"], gdo.score_matrix(a, b), go, ge, go, ge, c["w"])
        assert d["score"] == c["score"] and np.array_equal(d["cigar"], c["cigar"])


def _diag_cases(rng, n_cases, a, b, thr):
    """N-free pairs of equal length whose only differences are m substitutions with m (a + b) <= thr: random, tandem-repeat and two-letter
    targets (where a gapped path re-aligns the most), scattered and adjacent mismatches"""
    mmax = thr // (a + b)
    for it in range(n_cases):
        n = int(rng.integers(17, 260))
        kind = it % 4
        if kind == 0:
            t = rng.integers(0, 4, size=n, dtype=np.uint8)
        elif kind == 1:
            t = np.resize(rng.integers(0, 4, size=int(rng.integers(1, 7)), dtype=np.uint8), n).astype(np.uint8)
        elif kind == 2:
            t = rng.integers(0, 2, size=n, dtype=np.uint8)
        else:
            t = np.resize(rng.integers(0, 4, size=int(rng.integers(2, 9)), dtype=np.uint8), n).astype(np.uint8)
            t[rng.integers(0, n, size=3)] = rng.integers(0, 4, size=3)
        m = int(rng.integers(0, mmax + 1))
        q = t.copy()
        pos = [int(x) for x in rng.choice(n, size=m, replace=False)] if m else []
        if it % 3 == 0 and m >= 2:
            pos[1] = min(n - 1, pos[0] + 1)
        for p in set(pos):
            q[p] = (q[p] + 1 + rng.integers(0, 3)) & 3
        mm = int((q != t).sum())
        if mm * (a + b) <= thr:
            yield q, t, mm


def test_few_mismatches_mean_the_main_diagonal(oracle):
    """what the library's widened pre-filter rests on (ksw_exact_match_kernel, csrc/ksw_backtrack.hip.h): an N-free pair of equal length
    with m substitutions and m (a + b) <= a + 2 (q + e) aligns along its main diagonal -- score (n - m) a - m b, CIGAR "<n>M" -- because any
    other corner-to-corner path pays two gap opens and scores one pair less (at equality a gapped path may tie; the backtrack's priority
    order still walks the diagonal).  Checked on the oracle for every scoring of gdo.SCORINGS the short-alignment kernels take (the
    pre-filter only answers for those), wide and narrow bands, and on the reference's own ksw_extd2_sse where oracle/_ref is built.
    (Passed the larger gap model first, the reference reports every DP score shifted by the difference of the two q+e: ksw_score_bias_kernel.)"""
    gdo, lib = oracle
    ref = gdo.load_ref() if gdo.have_ref() else None
    rng = np.random.default_rng(2025)
    n = 0
    for name, (a, b, go, ge, go2, ge2, amb) in gdo.SCORINGS.items():
        if not gdo.wave_scoring_ok(a, b, go, ge, go2, ge2, amb):
            continue
        bias = min(go + ge, go2 + ge2) - (go + ge)
        mat = gdo.score_matrix(a, b, sc_ambi=amb)
        for q, t, mm in _diag_cases(rng, 700 if name in gdo.PRESETS else 150, a, b, a + 2 * min(go + ge, go2 + ge2)):
            ln = len(q)
            for w in (ln, ln // 3 + 20):
                o = gdo.oracle_extd2(lib, q, t, mat, go, ge, go2, ge2, w)
                assert o["score"] == (ln - mm) * a - mm * b + bias and list(o["cigar"]) == [ln << 4], (name, ln, mm, w)
                if ref is not None and n % 5 == 0:
                    r = gdo.ref_extd2(ref, q, t, mat, go, ge, go2, ge2, w)
                    assert r["score"] == o["score"] and np.array_equal(r["cigar"], o["cigar"]), (name, ln, mm, w)
                n += 1
    assert n > 3000


def test_oracle_matches_reference_golden_at_every_table_scoring(oracle):
    """tests/golden/ksw2_scoring.npz: at every scoring of gdo.SCORINGS (presets, both sides of the wave forms' limits, single affine,
    the gap models swapped, large match scores, the mismatch limit, a score for N, scorings where the 8-bit recurrence wraps, those where
    ksw_extz2 != ksw_extd2(q,e,q,e)) the oracle reproduces ksw_extd2_sse, ksw_extd2_avx512, and ksw_extz2_sse in both modes"""
    gdo, lib = oracle
    cases = load_scoring()
    assert {c["scoring"] for c in cases} == set(gdo.SCORINGS) and len(cases) >= 200
    assert {c["scoring"]: c["sc"] for c in cases} == dict(gdo.SCORINGS)
    for c in cases:
        a, b, q, e, q2, e2, amb = c["sc"]
        mat = gdo.score_matrix(a, b, sc_ambi=amb)
        got = dict(extd2=gdo.oracle_extd2(lib, c["q"], c["t"], mat, q, e, q2, e2, c["w"]),
                   extd2_avx512=gdo.oracle_extd2(lib, c["q7"], c["t"], mat, q, e, q2, e2, c["w"], flag=gdo.EZ_APPROX_MAX | gdo.EZ_AVX512_SC),
                   extz2=gdo.oracle_extz2(lib, c["q"], c["t"], mat, q, e, c["w"]),
                   extz2_exact=gdo.oracle_extz2(lib, c["q"], c["t"], mat, q, e, c["w"], c["zdrop_x"], c["end_bonus_x"], c["flag_x"]))
        for k in SCORING_OUTPUTS:
            if k == "extd2_avx512" and c["cls"] == "k3":
                continue  # (decided by the band-edge padding cells, whose width differs in the AVX-512 build: DESIGN.md, K3)
            for f in SCALARS:
                assert got[k][f] == c[k][f], (c["scoring"], c["cls"], k, f, got[k][f], c[k][f])
            assert np.array_equal(got[k]["cigar"], c[k]["cigar"]), (c["scoring"], c["cls"], k)


def test_extz2_is_extd2_where_the_wave_forms_run_and_not_everywhere(oracle):
    """gdiet_hip_ksw_extz2_batch runs ksw_extz2(q,e) as ksw_extd2(q,e,q,e) only at scorings the register-resident kernels take
    (gdo.wave_scoring_ok); there the two agree on every golden pair and on a sweep of single-affine scorings.  At the table's K3 scorings
    they do not -- which is why the library runs ksw_extz2's own recurrence there"""
    gdo, lib = oracle
    cases = load_scoring()
    differ = set()
    for c in cases:
        a, b, q, e, _, _, amb = c["sc"]
        mat = gdo.score_matrix(a, b, sc_ambi=amb)
        d = gdo.oracle_extd2(lib, c["q"], c["t"], mat, q, e, q, e, c["w"])
        if gdo.wave_scoring_ok(a, b, q, e, q, e, amb):
            assert gdo.same(d, c["extz2"]), (c["scoring"], c["cls"])
        elif not gdo.same(d, c["extz2"]):
            differ.add(c["scoring"])
    assert {"wrap_2_8_60_3", "wrap_10_20_40_20"} | {k for k in gdo.SCORINGS if k.startswith("k3_")} <= differ, differ
    assert all(not gdo.wave_scoring_ok(*gdo.SCORINGS[k]) for k in differ)
    rng = np.random.default_rng(99)
    pairs = [gdo.make_pair(rng, int(rng.integers(30, 300)), 0.05, 0.03, 0.03) + (int(rng.integers(10, 150)),) for _ in range(6)]
    n = 0
    for a in (1, 2, 4):
        for q in range(0, 15, 2):
            for e in (1, 2, 3):
                for b in range(2, 2 * (q + e) + 1, 3):
                    if not gdo.wave_scoring_ok(a, b, q, e, q, e):
                        continue
                    mat = gdo.score_matrix(a, b)
                    for qs, ts, w in pairs:
                        assert gdo.same(gdo.oracle_extz2(lib, qs, ts, mat, q, e, w), gdo.oracle_extd2(lib, qs, ts, mat, q, e, q, e, w)), (a, b, q, e)
                        n += 1
    assert n > 1000

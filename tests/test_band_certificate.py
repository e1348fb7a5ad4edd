"""CPU: the certificate of the 64-lane DP kernel's narrow band (gd_band_certified in ksw_wave_core.h, compiled from that header by
tests/emul/cert_shim.cpp -- the function the kernel evaluates, not a restatement).  A box whose band is wider than GD_W_NARROW is
aligned in the narrow band first and the result kept when the certificate holds, so: whenever it holds, the oracle's score and CIGAR
at the narrow band must be its score and CIGAR at w = 1000.  The pairs are those on which the two bands can differ -- long indels,
tandem copy-number changes, two-letter sequences, Ns, besides HiFi-like reads at 1-6 % error -- and the test is not vacuous: at least
40 % of the (pair, band) cases certify and at least 10 uncertified ones do differ between the bands."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import gdo as _gdo
from narrow_pairs import band_edge_pairs, certificate_mix, load_cert_shim, max_off_diagonal

W_FULL = 1000
SCORINGS = ("hifi", "sr", "ont")
N_PAIRS = 264
# the scorings of the oracle's table that the register-resident kernels take in dual-affine form: those that can reach the narrow band
WAVE_SCORINGS = [k for k, v in _gdo.SCORINGS.items() if _gdo.wave_scoring_ok(*v)]
OFF_PRESET = [k for k in WAVE_SCORINGS if k not in SCORINGS]
AVX = _gdo.EZ_APPROX_MAX | _gdo.EZ_AVX512_SC


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return load_cert_shim(tmp_path_factory.mktemp("cert"))


def _certified(shim, gdo, scoring, wn, qlen, tlen, score):
    mch, mis, n, q, e, q2, e2 = gdo.abi_consts(*gdo.PRESETS[scoring])
    return bool(shim.cert_band_certified(wn, mch, mis, n, q, e, q2, e2, qlen, tlen, score))


@pytest.fixture(scope="module")
def cases(shim, oracle):
    """every pair at w = 1000 and at the three narrow bands, once (the oracle releases the GIL: a few threads side by side)"""
    gdo, lib = oracle
    bands = (119, 247, shim.cert_w_narrow())
    pairs = certificate_mix(20261018, N_PAIRS)

    def one(k):
        q, t = pairs[k]
        scoring = SCORINGS[k % 3]
        a, b, gq, ge, gq2, ge2 = gdo.PRESETS[scoring]
        mat = gdo.score_matrix(a, b)
        full = gdo.oracle_extd2(lib, q, t, mat, gq, ge, gq2, ge2, W_FULL)
        rows = []
        for wn in bands:
            if abs(len(t) - len(q)) > wn:  # the corner is outside the band: nothing to run, the certificate must refuse
                rows.append((k, scoring, wn, None, full))
                continue
            rows.append((k, scoring, wn, gdo.oracle_extd2(lib, q, t, mat, gq, ge, gq2, ge2, wn), full))
        return rows

    with ThreadPoolExecutor(max_workers=max(1, min(8, (os.cpu_count() or 2) - 1))) as pool:
        out = [r for rows in pool.map(one, range(N_PAIRS)) for r in rows]
    return pairs, out


def test_w_narrow_is_what_the_planner_uses(shim):
    assert shim.cert_w_narrow() == 495
    assert shim.cert_narrow_mode(9000, 9010, 1000) == 1 and shim.cert_narrow_mode(9000, 9010, 300) == 2
    assert shim.cert_narrow_mode(9000, 9000 + 496, 1000) == 0 and shim.cert_narrow_mode(9000, 9000 - 496, 1000) == 0


def test_certified_alignments_are_those_of_the_full_band(shim, oracle, cases):
    gdo, _ = oracle
    pairs, rows = cases
    n_cert = n_differ_uncert = 0
    bad = []
    per_band = {}
    for k, scoring, wn, narrow, full in rows:
        q, t = pairs[k]
        if narrow is None:
            assert not _certified(shim, gdo, scoring, wn, len(q), len(t), full["score"]), (k, wn)
            continue
        cert = _certified(shim, gdo, scoring, wn, len(q), len(t), narrow["score"])
        same = gdo.same(narrow, full, keys=("score",))
        st = per_band.setdefault(wn, [0, 0, 0])
        st[0] += 1
        st[1] += cert
        st[2] += (not cert) and (not same)
        n_cert += cert
        n_differ_uncert += (not cert) and (not same)
        if cert and not same:
            bad.append((k, scoring, wn, len(q), len(t), narrow["score"], full["score"]))
    print("certificate: %d cases, %d certified, %d uncertified and different; per band (cases, certified, differing): %s"
          % (len(rows), n_cert, n_differ_uncert, per_band))
    assert not bad, "certified, yet the full band aligns differently: %s" % bad[:5]
    assert n_cert >= 0.4 * len(rows), (n_cert, len(rows))
    assert n_differ_uncert >= 10, n_differ_uncert


def test_certificate_against_the_reference_build(shim, oracle, cases):
    """the same on the reference's own ksw_extd2_sse, where it has been built, for a subset"""
    gdo, _ = oracle
    if not gdo.have_ref("lr_avx"):
        pytest.skip("oracle/_ref not built")
    ref = gdo.load_ref("lr_avx")
    pairs, rows = cases
    n_cert = 0
    for k, scoring, wn, narrow, full in rows[::5]:
        if narrow is None:
            continue
        q, t = pairs[k]
        a, b, gq, ge, gq2, ge2 = gdo.PRESETS[scoring]
        mat = gdo.score_matrix(a, b)
        rn = gdo.ref_extd2(ref, q, t, mat, gq, ge, gq2, ge2, wn)
        rf = gdo.ref_extd2(ref, q, t, mat, gq, ge, gq2, ge2, W_FULL)
        if _certified(shim, gdo, scoring, wn, len(q), len(t), rn["score"]):
            n_cert += 1
            assert gdo.same(rn, rf, keys=("score",)), (k, scoring, wn)
    assert n_cert >= 10


# ---- at every scoring of the table that reaches the narrow band (the presets above; here the others) ----------------------------------
# The certificate's constants come from the scoring (gd_narrow_arg on gd_derive_consts), and it is evaluated on the score the KERNEL
# computes.  Passed the larger gap model first ("swapped"), the reference -- and so the oracle and the library -- reports every DP score
# shifted by cert_score_bias = -11; the certificate must see the oracle's score MINUS that bias.

def _certified_for(shim, gdo, name, wn, qlen, tlen, unshifted):
    a, b, q, e, q2, e2, amb = gdo.SCORINGS[name]
    return bool(shim.cert_certified_for(wn, a, -b, amb, q, e, q2, e2, qlen, tlen, unshifted))


def _bias(shim, gdo, name):
    a, b, q, e, q2, e2, amb = gdo.SCORINGS[name]
    return shim.cert_score_bias(a, -b, amb, q, e, q2, e2)


def _oracle_at(gdo, lib, name, q, t, w):
    a, b, gq, ge, gq2, ge2, amb = gdo.SCORINGS[name]
    return gdo.oracle_extd2(lib, q, t, gdo.score_matrix(a, b, sc_ambi=amb), gq, ge, gq2, ge2, w)


def test_the_table_has_the_eleven_wave_scorings(shim, oracle):
    gdo, _ = oracle
    assert WAVE_SCORINGS == ["sr", "hifi", "ont", "bound120_last", "skey_corner", "single_affine", "swapped", "equal_e", "a8", "a16", "ambi"]
    assert [_bias(shim, gdo, k) for k in WAVE_SCORINGS] == [0, 0, 0, 0, 0, 0, -11, 0, 0, 0, 0]


@pytest.fixture(scope="module")
def mix48():
    return certificate_mix(99, 48)


@pytest.mark.parametrize("name", OFF_PRESET)
def test_certified_alignments_are_those_of_the_full_band_off_preset(shim, oracle, mix48, name):
    """48 pairs of the mix at bands 247 and 495 against w = 1000: certified (on the unshifted score) => score and CIGAR of the full band.
    Not vacuous per scoring: at least a quarter of the cases certify and at least 3 uncertified ones differ between the bands.
    Oracle alone, seed 99: 78 cases per scoring, 25 (skey_corner) to 66 certified, 5 uncertified and different."""
    gdo, lib = oracle
    bias = _bias(shim, gdo, name)

    def one(k):
        q, t = mix48[k]
        full = _oracle_at(gdo, lib, name, q, t, W_FULL)
        return [(k, wn, _oracle_at(gdo, lib, name, q, t, wn) if abs(len(t) - len(q)) <= wn else None, full) for wn in (247, shim.cert_w_narrow())]

    with ThreadPoolExecutor(max_workers=max(1, min(8, (os.cpu_count() or 2) - 1))) as pool:
        rows = [r for rs in pool.map(one, range(len(mix48))) for r in rs]
    n = n_cert = n_differ_uncert = 0
    bad = []
    for k, wn, narrow, full in rows:
        q, t = mix48[k]
        if narrow is None:  # the corner is outside the band: nothing to run, the certificate must refuse
            assert not _certified_for(shim, gdo, name, wn, len(q), len(t), full["score"] - bias), (k, wn)
            continue
        cert = _certified_for(shim, gdo, name, wn, len(q), len(t), narrow["score"] - bias)
        same = gdo.same(narrow, full, keys=("score",))
        n += 1
        n_cert += cert
        n_differ_uncert += (not cert) and (not same)
        if cert and not same:
            bad.append((k, wn, len(q), len(t), narrow["score"], full["score"]))
    print("certificate at %s: %d cases, %d certified, %d uncertified and different, %d certified and different" % (name, n, n_cert, n_differ_uncert, len(bad)))
    assert not bad, "certified, yet the full band aligns differently: %s" % bad[:5]
    assert 4 * n_cert >= n, (n_cert, n)
    assert n_differ_uncert >= 3, n_differ_uncert


def _smallest_certifying_score(shim, gdo, name, wn, qlen, tlen):
    """by bisection on the function the kernel evaluates (monotone in the score)"""
    a = max(gdo.SCORINGS[name][0], 1)
    lo, hi = -(1 << 24), a * min(qlen, tlen) + 1  # hi: above any score, and above both bounds
    assert not _certified_for(shim, gdo, name, wn, qlen, tlen, lo) and _certified_for(shim, gdo, name, wn, qlen, tlen, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _certified_for(shim, gdo, name, wn, qlen, tlen, mid):
            hi = mid
        else:
            lo = mid
    return hi


@pytest.fixture(scope="module")
def edge10():
    return band_edge_pairs(5)


@pytest.mark.parametrize("name", WAVE_SCORINGS)
def test_paths_one_diagonal_outside_the_band_score_below_the_bound(shim, oracle, edge10, name):
    """The bound itself, on error-free pairs whose best full-band path runs ONE diagonal beyond D = 495 and comes back
    (narrow_pairs.band_edge_pair): such a path must score strictly below the smallest score the certificate accepts for the pair's
    lengths -- a bound a little too low would accept it.  Tight per scoring: at least 8 of the 10 pairs do leave the band and at least 4
    come within 24 of the bound.  Oracle alone, seed 5: the nearest pair is 4 (hifi, skey_corner), 5 (sr, ont, bound120_last, swapped,
    ambi), 7 (single_affine), 11 (a8) and 19 (equal_e, a16) below the smallest certifying score."""
    gdo, lib = oracle
    D = shim.cert_w_narrow()
    bias = _bias(shim, gdo, name)
    n_out = n_tight = 0
    nearest = None
    for q, t in edge10:
        full = _oracle_at(gdo, lib, name, q, t, W_FULL)
        if max_off_diagonal(full["cigar"]) <= D:
            continue
        n_out += 1
        need = _smallest_certifying_score(shim, gdo, name, D, len(q), len(t))
        gap = need - (full["score"] - bias)
        assert gap > 0, "%s: a path outside the band scores %d (unshifted), and %d would certify (qlen %d tlen %d)" % (name, full["score"] - bias, need, len(q), len(t))
        n_tight += gap <= 24
        nearest = gap if nearest is None else min(nearest, gap)
    print("bound at %s: %d of %d pairs leave the band, %d within 24 of the bound, the nearest %s below it" % (name, n_out, len(edge10), n_tight, nearest))
    assert n_out >= 8 and n_tight >= 4, (n_out, n_tight)

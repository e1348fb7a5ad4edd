"""CPU: the certificate of the 64-lane DP kernel's narrow band (gd_band_certified in ksw_wave_core.h, compiled from that header by
tests/emul/cert_shim.cpp -- the function the kernel evaluates, not a restatement).  A box whose band is wider than GD_W_NARROW is
aligned in the narrow band first and the result kept when the certificate holds, so: whenever it holds, the oracle's score and CIGAR
at the narrow band must be its score and CIGAR at w = 1000.  The pairs are those on which the two bands can differ -- long indels,
tandem copy-number changes, two-letter sequences, Ns, besides HiFi-like reads at 1-6 % error -- and the test is not vacuous: at least
40 % of the (pair, band) cases certify and at least 10 uncertified ones do differ between the bands."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT
from narrow_pairs import certificate_mix

W_FULL = 1000
SCORINGS = ("hifi", "sr", "ont")
N_PAIRS = 264


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cert") / "libcert_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul", "cert_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.cert_band_certified.argtypes = [C.c_int] * 11
    return lib


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

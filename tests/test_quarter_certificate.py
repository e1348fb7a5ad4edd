"""CPU: the certificate at the 239-wide rung (gd_band_certified with D = GD_W_QUARTER, compiled from the kernel's header by
tests/emul/cert_shim.cpp).  A box whose band is wider runs the quarter-block rows at 239 first and keeps the result when the certificate
holds, so: whenever it holds, the oracle's score and CIGAR at 239 must be its score and CIGAR at w = 1000.  On the pairs where the two
bands can differ -- long indels, tandem copy-number changes, two-letter sequences, Ns (narrow_pairs.certificate_mix) -- and on 60 reads
drawn by the benchmark's rules, of which at least 58 must certify (1200 of 1200 such reads did when the rung was designed)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from narrow_pairs import certificate_mix, load_cert_shim
from quarter_pairs import W_QUARTER, bench_like_read, load_quarter_shim

W_FULL = 1000
N_MIX = 120
N_BENCH = 60


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return load_cert_shim(tmp_path_factory.mktemp("cert"))


def _both_bands(oracle, pairs):
    gdo, lib = oracle
    a, b, q, e, q2, e2 = gdo.PRESETS["hifi"]
    mat = gdo.score_matrix(a, b)

    def one(p):
        qq, tt = p
        full = gdo.oracle_extd2(lib, qq, tt, mat, q, e, q2, e2, W_FULL)
        narrow = gdo.oracle_extd2(lib, qq, tt, mat, q, e, q2, e2, W_QUARTER) if abs(len(tt) - len(qq)) <= W_QUARTER else None
        return narrow, full

    with ThreadPoolExecutor(max_workers=max(1, min(8, (os.cpu_count() or 2) - 1))) as pool:
        return list(pool.map(one, pairs))


def _certified(shim, gdo, qlen, tlen, score):
    mch, mis, n, q, e, q2, e2 = gdo.abi_consts(*gdo.PRESETS["hifi"])
    return bool(shim.cert_band_certified(W_QUARTER, mch, mis, n, q, e, q2, e2, qlen, tlen, score))


def test_the_constant_and_the_break_even_share(tmp_path):
    q = load_quarter_shim(tmp_path)
    assert q.quarter_w() == 239
    assert 0 < q.quarter_break_even_num() < q.quarter_break_even_den()


def test_certified_at_239_is_the_alignment_of_the_full_band(shim, oracle):
    gdo, _ = oracle
    pairs = certificate_mix(20261019, N_MIX)
    n_cert = n_differ_uncert = 0
    bad = []
    for (qq, tt), (narrow, full) in zip(pairs, _both_bands(oracle, pairs)):
        if narrow is None:  # the corner is outside the band: nothing to run, the certificate must refuse
            assert not _certified(shim, gdo, len(qq), len(tt), full["score"])
            continue
        cert = _certified(shim, gdo, len(qq), len(tt), narrow["score"])
        same = gdo.same(narrow, full, keys=("score",))
        n_cert += cert
        n_differ_uncert += (not cert) and (not same)
        if cert and not same:
            bad.append((len(qq), len(tt), narrow["score"], full["score"]))
    print("certificate at 239: %d pairs, %d certified, %d uncertified and different" % (len(pairs), n_cert, n_differ_uncert))
    assert not bad, "certified at 239, yet the full band aligns differently: %s" % bad[:5]
    # not vacuous: a good share certifies, and pairs that do differ between the bands are among the refused ones
    assert n_cert >= N_MIX // 4 and n_differ_uncert >= 5, (n_cert, n_differ_uncert)


def test_reads_like_the_benchmarks_certify_at_239(shim, oracle):
    gdo, _ = oracle
    rng = np.random.default_rng(239)
    pairs = [bench_like_read(rng) for _ in range(N_BENCH)]
    n_cert = 0
    losses = []
    for (qq, tt), (narrow, full) in zip(pairs, _both_bands(oracle, pairs)):
        assert narrow is not None
        cert = _certified(shim, gdo, len(qq), len(tt), narrow["score"])
        n_cert += cert
        losses.append(min(len(qq), len(tt)) * gdo.PRESETS["hifi"][0] - narrow["score"])
        if cert:
            assert gdo.same(narrow, full, keys=("score",)), (len(qq), len(tt))
    print("bench-like reads at 239: %d of %d certified; loss against a perfect match %.0f +- %.0f, largest %d (the certificate holds below about 769)"
          % (n_cert, N_BENCH, np.mean(losses), np.std(losses), max(losses)))
    assert n_cert >= 58, n_cert

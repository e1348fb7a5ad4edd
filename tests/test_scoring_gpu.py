"""GPU parity at every scoring of gdo.SCORINGS (not only the three presets): ksw_extd2_batch (automatic dispatch and the generic kernel
alone), ksw_extz2_batch and ksw_extz2_batch_ex against the reference's outputs in tests/golden/ksw2_scoring.npz, and which kernel form
took each scoring (last_kernel_mask: 1 = 64-lane, 2 = generic LDS / literal extz2, 4 = short-alignment groups, 8 = wide band,
16 = pipelines)."""
import numpy as np
import pytest

from golden_io import load_scoring

pytestmark = pytest.mark.gpu

WAVE_BIT = {"sr": 4, "group": 1 | 4, "lane64": 1 | 4, "wide": 8}  # (a 64-lane length with a narrow band can fit the 16-lane form)


def _by_scoring():
    out = {}
    for c in load_scoring():
        out.setdefault(c["scoring"], []).append(c)
    return out


def _score(pkg, sc, single=False, flag=None):
    a, b, q, e, q2, e2, amb = sc
    if single:
        q2, e2 = q, e
    return pkg.KswScore(a, -b, amb, q, e, q2, e2, 0, pkg.hip_abi.EZ_APPROX_MAX if flag is None else flag)


def _check(got_sc, got_cg, cases, key, tag):
    for i, c in enumerate(cases):
        want = c[key]
        assert got_sc[i] == want["score"], (tag, c["cls"], i, len(c["q"]), len(c["t"]), c["w"], got_sc[i], want["score"])
        assert np.array_equal(got_cg[i], want["cigar"]), (tag, c["cls"], i, len(c["q"]), len(c["t"]), c["w"])


@pytest.mark.parametrize("name", list(_by_scoring()))
def test_dp_kernels_match_reference_at_scoring(gpu_ctx, pkg, oracle, name):
    gdo, lib = oracle
    cases = _by_scoring()[name]
    sc = cases[0]["sc"]
    dual_ok = gdo.wave_scoring_ok(*sc)
    single_ok = gdo.wave_scoring_ok(sc[0], sc[1], sc[2], sc[3], sc[2], sc[3], sc[6])
    classes = sorted({c["cls"] for c in cases})
    # ksw_extd2, automatic dispatch: one batch per shape class, so that each one's kernel form is asserted
    for cls in classes:
        cs = [c for c in cases if c["cls"] == cls]
        # an exact_score column at this scoring's match score: the copies among the short-read pairs are answered by the pre-filter
        ex = np.array([len(c["q"]) * sc[0] if len(c["q"]) == len(c["t"]) else pkg.hip_abi.NEG_INF for c in cs], np.int32)
        s, cg = gpu_ctx.ksw_extd2_batch([c["q"] for c in cs], [c["t"] for c in cs], [c["w"] for c in cs], _score(pkg, sc), exact_score=ex)
        mask = gpu_ctx.last_kernel_mask()
        for i, c in enumerate(cs):
            if len(c["q"]) == len(c["t"]) and np.array_equal(c["q"], c["t"]):
                assert s[i] == ex[i] and list(cg[i]) == [len(c["q"]) << 4], (name, cls, i)
                s[i] = c["extd2"]["score"]
                cg[i] = c["extd2"]["cigar"]
        _check(s, cg, cs, "extd2", (name, "extd2"))
        if not dual_ok:
            assert mask == 2, (name, cls, mask)
        elif cls in WAVE_BIT:
            assert mask & WAVE_BIT[cls], (name, cls, mask)
            # at a scoring the wave forms take, the form depends on the geometry alone: the same pairs at the sr preset take exactly the
            # same kernels (bits 0-3; a pair whose band geometry no wave form fits goes to the generic kernel at every scoring)
            gpu_ctx.ksw_extd2_batch([c["q"] for c in cs], [c["t"] for c in cs], [c["w"] for c in cs], pkg.KswScore.from_preset("sr"))
            assert mask & 15 == gpu_ctx.last_kernel_mask() & 15, (name, cls, mask, gpu_ctx.last_kernel_mask())
            if cls == "sr":
                assert not mask & 2, (name, cls, mask)
        # the same pairs with byte-7 query Ns (a reverse-complemented read's N) against ksw_extd2_avx512 (k3 pairs: no byte 7, and the AVX-512
        # build's wider windows decide some of them differently)
        if cls != "k3":
            s, cg = gpu_ctx.ksw_extd2_batch([c["q7"] for c in cs], [c["t"] for c in cs], [c["w"] for c in cs], _score(pkg, sc))
            _check(s, cg, cs, "extd2_avx512", (name, "extd2 byte-7"))
    # ... the generic LDS kernel alone (mode 1), the whole table's pairs in one batch
    gpu_ctx.set_kernel_mode(1)
    try:
        s, cg = gpu_ctx.ksw_extd2_batch([c["q"] for c in cases], [c["t"] for c in cases], [c["w"] for c in cases], _score(pkg, sc))
        assert gpu_ctx.last_kernel_mask() == 2
    finally:
        gpu_ctx.set_kernel_mode(0)
    _check(s, cg, cases, "extd2", (name, "extd2 generic"))
    # ksw_extz2 (APPROX_MAX): ksw_extd2(q,e,q,e) on the wave forms where they take the scoring, ksw_extz2's own recurrence elsewhere
    for cls in classes:
        cs = [c for c in cases if c["cls"] == cls]
        s, cg = gpu_ctx.ksw_extz2_batch([c["q"] for c in cs], [c["t"] for c in cs], [c["w"] for c in cs], _score(pkg, sc, single=True))
        mask = gpu_ctx.last_kernel_mask()
        _check(s, cg, cs, "extz2", (name, "extz2"))
        if not single_ok:
            assert mask == 2, (name, cls, mask)
        elif cls in WAVE_BIT:
            assert mask & WAVE_BIT[cls], (name, cls, mask)
    # ksw_extz2, exact-maximum mode (flag 0 / EXTZ_ONLY; zdrop, end_bonus per case)
    for c in cases:
        ez, cg = gpu_ctx.ksw_extz2_batch_ex([c["q"]], [c["t"]], [c["w"]], _score(pkg, sc, single=True, flag=c["flag_x"]), c["zdrop_x"], c["end_bonus_x"])
        assert gpu_ctx.last_kernel_mask() == 2
        for f in ("score", "zdropped", "max", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "reach_end"):
            assert ez[0][f] == c["extz2_exact"][f], (name, c["cls"], f, ez[0][f], c["extz2_exact"][f])
        assert np.array_equal(cg[0], c["extz2_exact"]["cigar"]), (name, c["cls"])


@pytest.mark.parametrize("env", ["GDIET_GROUP_LANES=16", "GDIET_SR_PIPE=0", "GDIET_DIAG_SHORTCUT=0"])
def test_dispatch_variants_match_reference_at_every_scoring(env):
    """the dispatch switches read once per process, in a process of their own (tests/scoring_variant_check.py): four alignments per
    wavefront instead of 8 / 6, the grouped kernels instead of the pipelines, every short alignment through the DP and the walk instead
    of the pre-filter's diagonal answer -- at every table scoring against the reference's golden"""
    import os
    import subprocess
    import sys
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scoring_variant_check.py")
    k, v = env.split("=")
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, env=dict(os.environ, **{k: v}), timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("two_waves", ["0", "1", "ckpt"])
def test_wide_band_variants_match_reference_at_scoring(pkg, oracle, monkeypatch, two_waves):
    """the wide-band pairs of the table (w = 1300) through each wide-band form: one wavefront, two wavefronts, checkpointed"""
    if two_waves == "ckpt":
        monkeypatch.setenv("GDIET_WIDE_CKPT", "1")
    else:
        monkeypatch.setenv("GDIET_WIDE_TWO_WAVES", two_waves)
        monkeypatch.setenv("GDIET_WIDE_CKPT", "0")
    gdo, _ = oracle
    ctx = pkg.Context(0)
    try:
        n = 0
        for name, cases in _by_scoring().items():
            cs = [c for c in cases if c["cls"] == "wide"]
            if not cs:
                continue
            s, cg = ctx.ksw_extd2_batch([c["q"] for c in cs], [c["t"] for c in cs], [c["w"] for c in cs], _score(pkg, cs[0]["sc"]))
            assert ctx.last_kernel_mask() == (8 if gdo.wave_scoring_ok(*cs[0]["sc"]) else 2), (name, ctx.last_kernel_mask())
            _check(s, cg, cs, "extd2", (name, "wide", two_waves))
            n += len(cs)
        assert n >= 5
    finally:
        ctx.close()

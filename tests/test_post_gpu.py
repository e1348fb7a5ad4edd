"""GPU: the two P1 kernels at their own boundary (Context.post_batch = gdiet_hip_post_batch: the map_post_kernel<false> /
map_post_wave_kernel the mapping path launches) on the designed families of tests/post_inputs.py.
  * the golden set (tests/golden/update_extra.npz: the reference's mm_update_extra on every case) through form 0 and 1, each with the
    results copied back and with the kernel's own stores to page-locked memory: n_cigar, the six result fields and every word of the
    pool -- the CIGAR, the words behind the new n_cigar, the guard word between two slots, the dead slots -- are equal to the
    reference's / the host emulator's (tests/emul/post_emul.cpp, built here without sanitizers; tests/test_post.py holds it to the
    reference under ASan and UBSan);
  * 2 000 fresh random alignments the same way, against the emulator;
  * batches of 1, 63, 64 and 65 alignments.
A call has one scoring, so a set goes up as one call per scoring it uses: all cases of that scoring in one batch.  Equality is exact."""
import os
import subprocess

import numpy as np
import pytest

import post_inputs as P
from conftest import ROOT

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "update_extra.npz")
MODES = [(0, False), (0, True), (1, False), (1, True)]
MODE_IDS = ["thread", "thread_exported", "wave", "wave_exported"]


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    d = tmp_path_factory.mktemp("post_gpu")
    exe = str(d / "post_emul")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"), os.path.join(ROOT, "tests", "emul", "post_emul.cpp"), "-o", exe])

    def run(tag, cases, scorings):
        fin, fout = str(d / (tag + ".in")), str(d / (tag + ".out"))
        P.write_emul_input(fin, cases, scorings)
        subprocess.run([exe, fin, fout], check=True)
        return P.read_emul_output(fout, cases)
    return run


@pytest.fixture(scope="module")
def golden(emul):
    cases, refs, scorings = P.load_golden(GOLDEN)
    return cases, refs, scorings, emul("golden", cases, scorings)


@pytest.fixture(scope="module")
def fresh(emul):
    cases = P.random_cases()
    return cases, P.SCORINGS, emul("random", cases, P.SCORINGS)


def check_batch(ctx, cases, want, scoring, form, exported):
    """one call; want[i] = the emulator's three results for cases[i] (the thread form's is the expectation for either kernel)"""
    _, mat, gq, ge, lg = scoring
    L = P.layout(cases)
    pool, nc, post = ctx.post_batch(L["qseq"], L["qoff"], L["tseq"], L["toff"], L["cigar"], L["coff"], L["n_cigar"], L["score"], mat, gq, ge, lg, form, exported)
    exp_pool = L["cigar"].copy()
    for i, w in enumerate(want):
        exp_pool[L["coff"][i]:L["coff"][i + 1] - 1] = w[0]["slot"]
    assert np.all(exp_pool[L["coff"][1:] - 1] == P.GUARD)
    exp_nc = np.array([w[0]["n_cigar"] for w in want], np.int32)
    exp_post = np.array([[w[0][k] for k in P.FIELDS] for w in want], np.int64).astype(np.int32)
    bad = np.nonzero((nc != exp_nc) | np.any(post != exp_post, axis=1))[0]
    assert len(bad) == 0, (scoring[0], form, exported, [(cases[i]["family"], int(nc[i]), int(exp_nc[i]), post[i].tolist(), exp_post[i].tolist()) for i in bad[:5]])
    badw = np.nonzero(pool != exp_pool)[0]
    assert len(badw) == 0, (scoring[0], form, exported, [(int(w), cases[int(np.searchsorted(L["coff"], w, "right")) - 1]["family"]) for w in badw[:5]])


def by_scoring(cases, want):
    groups = {}
    for c, w in zip(cases, want):
        groups.setdefault(c["sc"], ([], []))
        groups[c["sc"]][0].append(c), groups[c["sc"]][1].append(w)
    return groups


def test_emulator_expectation_is_the_reference(golden):
    """(what the CPU suite checks under the sanitizers, here on the plain build the GPU results are held to)"""
    cases, refs, _, want = golden
    for c, r, w in zip(cases, refs, want):
        if P.is_dead(c):
            assert w[0]["n_cigar"] == c["n_cigar"] and all(w[0][k] == 0 for k in P.FIELDS) and np.array_equal(w[0]["slot"], c["cigar"])
        else:
            assert w[0]["n_cigar"] == len(r["cigar"]) and all(w[0][k] == r[k] for k in P.FIELDS) and np.array_equal(w[0]["slot"][:len(r["cigar"])], r["cigar"])


@pytest.mark.parametrize("form,exported", MODES, ids=MODE_IDS)
def test_golden_set(gpu_ctx, golden, form, exported):
    cases, _, scorings, want = golden
    groups = by_scoring(cases, want)
    assert len(groups) == len(scorings)
    for sc, (cs, ws) in groups.items():
        check_batch(gpu_ctx, cs, ws, scorings[sc], form, exported)


@pytest.mark.parametrize("form,exported", MODES, ids=MODE_IDS)
def test_fresh_random_alignments(gpu_ctx, fresh, form, exported):
    cases, scorings, want = fresh
    for sc, (cs, ws) in by_scoring(cases, want).items():
        check_batch(gpu_ctx, cs, ws, scorings[sc], form, exported)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_shapes(gpu_ctx, golden, n):
    """1, 63, 64 and 65 alignments: one block and its edge in the thread form, so many wavefronts in the other; live and dead slots mixed"""
    cases, _, scorings, want = golden
    cs, ws = by_scoring(cases, want)[P.SC["hifi_log"]]
    live = [i for i, c in enumerate(cs) if c["family"].startswith(("fix_", "tie_", "seam_"))]
    dead = [i for i, c in enumerate(cs) if P.is_dead(c)]
    assert len(dead) >= 15 and len(live) >= 140
    for start in (0, 1):
        idx = live[start::2][:n]
        if n > 1:  # dead slots in front, inside and last
            idx[0], idx[n // 2], idx[-1] = dead[start], dead[5 + start], dead[10 + start]
        assert len(idx) == n
        for form, exported in MODES:
            check_batch(gpu_ctx, [cs[i] for i in idx], [ws[i] for i in idx], scorings[P.SC["hifi_log"]], form, exported)


def test_a_cigar_past_its_windows_is_refused(gpu_ctx, pkg):
    """the boundary checks what a live CIGAR consumes against its windows before anything is launched"""
    c = P.Builder(np.random.default_rng(1)).m(10).i(2).m(5).case("x")
    L = P.layout([c])
    with pytest.raises(pkg.GdietError):
        gpu_ctx.post_batch(L["qseq"][:-1], L["qoff"] - np.array([0, 1]), L["tseq"], L["toff"], L["cigar"], L["coff"], L["n_cigar"], L["score"], P.matrix(1, 4), 6, 2, 1, 1)

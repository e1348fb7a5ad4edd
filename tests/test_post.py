"""CPU: P1 -- mm_fix_cigar + mm_update_extra (csrc/map_post.h; the kernels map_post_kernel / map_post_wave_kernel) -- at its own boundary.
  * tests/golden/update_extra.npz holds the designed families of tests/post_inputs.py and what the REFERENCE's mm_update_extra made of
    them (oracle/pin_post.py; --check where oracle/_ref exists);
  * the plain restatement of the reference's loops agrees with the golden on every case, and its branch counters show that the families
    reach what they were designed for (asserted, no margin);
  * tests/emul/post_emul.cpp under AddressSanitizer and UBSan: the thread form's code and the lock-step restatement of the wave kernel, in
    both lane orders, equal the reference on every golden case and each other on 2 000 fresh random alignments;
  * eight seeded one-line mistakes in the wave form's helpers (-DGDP_MISTAKE=n, the emulator's build only): the families notice each; what
    the P1 inputs of the golden read sets (hifi, ont, hifi_sv, hifi_edge; dumped by the host driver) notice is printed beside it, with how
    often those inputs reach each condition.  DESIGN.md section 3 (P1) holds both tables.
tests/test_post_gpu.py runs the same cases through the kernels."""
import gzip
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import post_inputs as P
from conftest import ROOT
from fixture_io import LR, cmd_of, reads_of

GOLDEN = os.path.join(ROOT, "tests", "golden", "update_extra.npz")
CSRC = os.path.join(ROOT, "genome-on-diet_amd", "csrc")
EMUL = os.path.join(ROOT, "tests", "emul", "post_emul.cpp")
MISTAKES = {1: "join: B without + Ay", 2: "join: P without Ax +", 3: "join: Q without the Bx + Py term", 4: "fold: no tie on the fraction",
            5: "fold: Qm >= MXi for Qm > MXi", 6: "fold: Sf kept after a clamp", 7: "gap: the borrow forgotten", 8: "round: .5 for .499"}
OLD_SETS = ("hifi", "ont", "hifi_sv", "hifi_edge")


@pytest.fixture(scope="module")
def golden():
    return P.load_golden(GOLDEN)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return str(tmp_path_factory.mktemp("post"))


@pytest.fixture(scope="module")
def emul(work):
    exe = os.path.join(work, "post_emul")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, EMUL, "-o", exe])
    return exe


def run_emul(exe, work, tag, cases, scorings):
    fin, fout = os.path.join(work, tag + ".in"), os.path.join(work, tag + "." + os.path.basename(exe) + ".out")
    if not os.path.exists(fin):
        P.write_emul_input(fin, cases, scorings)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    return P.read_emul_output(fout, cases)


def expected(case, ref):
    """what either kernel must leave for a golden case: (n_cigar, the six fields, the CIGAR words that are defined)"""
    if P.is_dead(case):
        return case["n_cigar"], {k: 0 for k in P.FIELDS}, case["cigar"]
    return len(ref["cigar"]), {k: ref[k] for k in P.FIELDS}, ref["cigar"]


def differs(got, want):
    n, f, cg = want
    return got["n_cigar"] != n or any(got[k] != f[k] for k in P.FIELDS) or not np.array_equal(got["slot"][:len(cg)], cg)


def test_pin_script_check():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import gdo
    if not gdo.have_ref("lr_avx"):
        pytest.skip("oracle/_ref not built (no reference sources on this machine)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "pin_post.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.getsize(GOLDEN) < 400 * 1000


def test_golden_is_what_the_module_generates(golden):
    cases, _, scorings = golden
    mine = P.cases()
    assert len(mine) == len(cases)
    for a, b in zip(mine, cases):
        assert a["family"] == b["family"] and a["n_cigar"] == b["n_cigar"] and a["score"] == b["score"] and a["sc"] == b["sc"]
        assert np.array_equal(a["q"], b["q"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["cigar"], b["cigar"])
    for a, b in zip(P.SCORINGS, scorings):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


def test_restatement_agrees_with_the_reference(golden):
    cases, refs, scorings = golden
    for c, r in zip(cases, refs):
        if P.is_dead(c):
            assert all(r[k] == 0 for k in P.FIELDS) and len(r["cigar"]) == 0
            continue
        mine, _ = P.restate(c, scorings[c["sc"]])
        assert np.array_equal(mine["cigar"], r["cigar"]) and all(mine[k] == r[k] for k in P.FIELDS), (c["family"], mine, r)


def coverage_rows(cov):
    """the coverage table: (condition, count) -- a list of counters stands for its minimum"""
    def least(keys):
        return min(cov[k] for k in keys)
    rows = [("every M length of %s" % (P.SEAM_LENS,), least("run_len_%d" % n for n in P.SEAM_LENS)),
            ("... behind an I of odd length", least("run_len_%d_behind_odd_I" % n for n in P.SEAM_LENS)),
            ("... behind a D of odd length", least("run_len_%d_behind_odd_D" % n for n in P.SEAM_LENS)),
            ("clamp at every lane 0..63 (least)", least("clamp_lane_%d" % i for i in range(64))),
            ("score exactly 0 by a negative base", cov["exact_zero"]),
            ("clamps in two consecutive chunks", cov["clamps_in_consecutive_chunks"]),
            ("maximum at every lane 0..63 (least)", least("max_lane_%d" % i for i in range(64))),
            ("maximum on lane 63 and lane 0 of the next chunk", cov["max_on_both_sides_of_a_seam"]),
            ("maximum in a run that is not the last", cov["max_in_run_not_last"]),
            ("maximum attained twice", cov["max_attained_twice"]),
            ("tie on the integer part, larger fraction", cov["tie_frac_larger"]),
            ("tie on the integer part, smaller fraction", cov["tie_frac_smaller"]),
            ("tie on the integer part, equal fraction", cov["tie_frac_equal"]),
            ("restart from a clamp reaches the integer part of a fractional maximum", cov["tie_restart_reaches_int_of_frac_max"]),
            ("final fraction in [.496, .501)", cov["final_frac_just_below_step"]),
            ("final fraction in [.501, .506]", cov["final_frac_just_above_step"]),
            ("code 4 in M: query / target / both (least)", least(("ambi_in_M_q", "ambi_in_M_t", "ambi_in_M_both"))),
            ("code 4 first and last in I / D of %s (least)" % (P.GAP_LENS,), least("ambi_%s_of_%s_%d" % (w, o, g) for w in ("first", "last") for o in "ID" for g in P.GAP_LENS)),
            ("n_cigar 1", cov["fix_early_n1"]),
            ("zero-length operation in front / inside / last (least)", least("fix_zero_" + w for w in ("front", "inside", "last"))),
            ("left shift 0 < l < prev_len, I / D (least)", least(("fix_shift_part_I", "fix_shift_part_D"))),
            ("left shift l == prev_len, I / D (least)", least(("fix_shift_full_I", "fix_shift_full_D"))),
            ("shift empties the first M, I / D (least)", least(("fix_shift_empties_first_M_I", "fix_shift_empties_first_M_D"))),
            ("leading I / D removed (least)", least(("fix_lead_I_removed", "fix_lead_D_removed"))),
            ("I D I / D I D merged (least)", least(("fix_merge_IDI", "fix_merge_DID"))),
            ("longer run merged", cov["fix_merge_longer"]),
            ("run with a zero-length operation inside merged", cov["fix_merge_zero_inside"]),
            ("pair I D alone, not merged", cov["fix_pair_not_merged"]),
            ("equal neighbours merged", cov["fix_equal_neighbours"]),
            ("N between indels", cov["fix_N_between_indels"]),
            ("leading I / D in the input (least)", least(("fix_lead_I_input", "fix_lead_D_input"))),
            ("CIGARs of 1 000 operations or more", cov["ops_ge1000"])]
    return rows


FIVE = ("tie on", "restart from", "n_cigar 1", "zero-length", "left shift", "shift empties", "leading I", "I D I", "longer run", "run with a zero", "pair I D",
        "equal neighbours", "N between")


def test_families_reach_what_they_were_designed_for(golden):
    cases, refs, scorings = golden
    cov = P.coverage(cases, scorings)
    print("\ncoverage of the designed families (golden file):")
    for name, n in coverage_rows(cov):
        print("  %-75s %d" % (name, n))
        assert n >= (5 if name.startswith(FIVE) else 1), name
    assert cov["ops_ge1000"] >= 3
    # n_cigar 0 through the reference; the three kinds of dead slot
    assert sum(1 for c in cases if c["n_cigar"] == 0 and len(c["q"]) == 0) >= 5
    assert all(sum(1 for c in cases if c["family"] == f) >= 1 for f in ("dead_neg_inf", "dead_n0", "dead_over_cap"))
    assert all(P.is_dead(c) for c in cases if c["family"].startswith("dead_"))
    # the .499 step: both sides present; the nearest distances
    fr = []
    for c in cases:
        if not P.is_dead(c) and c["family"] == "step_499":
            mx = P.restate(c, scorings[c["sc"]])[0]["max"]
            fr.append(mx - int(mx))
    below, above = [0.501 - f for f in fr if f < 0.501], [f - 0.501 for f in fr if f >= 0.501]
    print("  nearest final fractions to .501: %.6f below, %.6f above" % (min(below), min(above)))
    assert min(below) < 0.005 and min(above) < 0.005
    # scoring: the presets' pairs, a large pair, a non-uniform 4 x 4 part, log_gap 0 and 1, e = 0 -- each used by live cases
    used = {scorings[c["sc"]][0] for c in cases if not P.is_dead(c)}
    assert {"hifi_log", "ont_log", "ont_lin", "sr_lin", "sr_log", "large_log", "large_lin", "nonuni_lin", "nonuni_log", "e0_log"} <= used
    by = {s[0]: s for s in scorings}
    assert by["large_log"][1][0] == 100 and by["large_log"][1][1] == -120 and by["e0_log"][3] == 0 and by["nonuni_lin"][4] == 0 and by["nonuni_log"][4] == 1
    m = by["nonuni_lin"][1]
    assert len({int(m[i * 5 + i]) for i in range(4)}) > 1 and len({int(m[i * 5 + j]) for i in range(4) for j in range(4) if i != j}) > 1
    # length
    long_ = [r for c, r in zip(cases, refs) if c["family"] == "long_perfect_40k"]
    assert len(long_) == 1 and long_[0]["mlen"] == 40000 and long_[0]["dp_max"] == 40000 * 100
    assert all(18000 <= len(c["q"]) <= 26000 for c in cases if c["family"] == "long_20k")
    assert sum(len(c["q"]) > 700 or len(c["t"]) > 4200 for c in cases) <= 4 + sum(c["family"] == "step_499" for c in cases)


def test_emulator_equals_the_reference_under_the_sanitizers(golden, emul, work):
    cases, refs, scorings = golden
    out = run_emul(emul, work, "golden", cases, scorings)
    for c, r, o in zip(cases, refs, out):
        want = expected(c, r)
        for v, name in enumerate(("thread form", "wave form, lanes 0..63", "wave form, lanes 63..0")):
            assert not differs(o[v], want), (c["family"], name, {k: o[v][k] for k in P.FIELDS}, r)
            assert np.array_equal(o[v]["slot"], o[0]["slot"]), (c["family"], name, "the words behind the CIGAR differ between the forms")
        if P.is_dead(c):
            assert np.array_equal(o[0]["slot"], c["cigar"])


def test_forms_agree_on_fresh_random_alignments(emul, work):
    cases = P.random_cases()
    assert len(cases) >= 1950
    n4 = sum(int((c["q"] > 3).sum() + (c["t"] > 3).sum()) for c in cases) / sum(len(c["q"]) + len(c["t"]) for c in cases)
    assert 0.08 < n4 < 0.12
    out = run_emul(emul, work, "random", cases, P.SCORINGS)
    for c, o in zip(cases, out):
        for v in (1, 2):
            assert o[v]["n_cigar"] == o[0]["n_cigar"] and all(o[v][k] == o[0][k] for k in P.FIELDS) and np.array_equal(o[v]["slot"], o[0]["slot"]), \
                (c["cigar"], {k: (o[v][k], o[0][k]) for k in P.FIELDS})
        mine, _ = P.restate(c)
        assert all(mine[k] == o[0][k] for k in P.FIELDS) and np.array_equal(mine["cigar"], o[0]["slot"][:o[0]["n_cigar"]])


@pytest.fixture(scope="module")
def old_inputs(work):
    """the P1 inputs of the golden read sets, dumped by the host driver: {set: (cases, scorings)}"""
    exe = os.path.join(work, "map_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-w", "-I", CSRC, "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "emul", "map_host_main.cpp"),
                           "-x", "c", os.path.join(ROOT, "oracle", "gdo_ksw2.c"), "-o", exe])
    ref = os.path.join(work, "ref.fa")
    with gzip.open(os.path.join(LR, "ref.fa.gz"), "rb") as src, open(ref, "wb") as dst:
        shutil.copyfileobj(src, dst)
    out = {}
    for kind in OLD_SETS:
        fq, dump = os.path.join(work, kind + ".fq"), os.path.join(work, kind + ".in")
        with open(fq, "w") as f:
            for name, seq, qual in reads_of(kind):
                f.write("@%s\n%s\n+\n%s\n" % (name, seq, qual))
        subprocess.run([exe, "-t", str(min(8, os.cpu_count() or 1))] + cmd_of(kind) + ["--dump-post=" + dump, ref, fq], capture_output=True, check=True)
        out[kind] = P.read_emul_input(dump)
        assert len(out[kind][0]) > 0
    return out


def test_golden_read_sets_through_both_forms_and_what_they_reach(old_inputs, emul, work):
    """the wave form's restatement equals the thread form's code on everything the golden read sets feed to P1; prints the "old" column
    of the coverage table"""
    tot = P.Counter()
    for kind, (cases, scorings) in old_inputs.items():
        out = run_emul(emul, work, kind, cases, scorings)
        for c, o in zip(cases, out):
            for v in (1, 2):
                assert o[v]["n_cigar"] == o[0]["n_cigar"] and all(o[v][k] == o[0][k] for k in P.FIELDS) and np.array_equal(o[v]["slot"], o[0]["slot"]), kind
        for k, v in P.coverage(cases, scorings).items():
            tot[k] += v
    print("\nwhat the P1 inputs of %s reach (%d alignments):" % (", ".join(OLD_SETS), sum(len(v[0]) for v in old_inputs.values())))
    for name, n in coverage_rows(tot):
        print("  %-75s %d" % (name, n))


def test_seeded_mistakes(golden, old_inputs, work):
    """each one-line mistake in the wave form's helpers changes the emulator's answer on some golden case; whether the P1 inputs of the
    golden read sets would have noticed is printed"""
    cases, refs, scorings = golden
    exes, procs = {}, []
    for m in [0] + sorted(MISTAKES):
        exes[m] = os.path.join(work, "post_emul_m%d" % m)
        procs.append(subprocess.Popen(["g++", "-O1", "-std=c++17", "-DGDP_MISTAKE=%d" % m, "-I", CSRC, EMUL, "-o", exes[m]]))
    assert all(p.wait() == 0 for p in procs)
    right = {kind: run_emul(exes[0], work, kind, cs, sc) for kind, (cs, sc) in old_inputs.items()}
    print("\nseeded mistake                               families: cases that differ   golden read sets: alignments that differ")
    for m in sorted(MISTAKES):
        out = run_emul(exes[m], work, "golden", cases, scorings)
        fam = sorted({c["family"] for c, r, o in zip(cases, refs, out) if differs(o[1], expected(c, r)) or differs(o[2], expected(c, r))})
        n_fam = sum(1 for c, r, o in zip(cases, refs, out) if differs(o[1], expected(c, r)))
        assert all(not differs(o[0], expected(c, r)) for c, r, o in zip(cases, refs, out)), "the thread form shares none of the helpers"
        n_old = 0
        for kind, (cs, sc) in old_inputs.items():
            got = run_emul(exes[m], work, kind, cs, sc)
            n_old += sum(1 for a, b in zip(got, right[kind]) if any(a[1][k] != b[1][k] for k in P.FIELDS))
        print("  %d %-40s %5d (%s)   %5d" % (m, MISTAKES[m], n_fam, ", ".join(fam[:4]) + (" ..." if len(fam) > 4 else ""), n_old))
        assert n_fam > 0, MISTAKES[m]


def test_mistake_switch_is_not_reachable_from_the_library(work):
    """GDP_MISTAKE without the emulator's own define does not compile"""
    src = os.path.join(work, "lib_like.cpp")
    open(src, "w").write('#include "map_post.h"\nint main() { return 0; }\n')
    assert subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", CSRC, src], capture_output=True).returncode == 0
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-DGDP_MISTAKE=3", "-I", CSRC, src], capture_output=True, text=True)
    assert r.returncode != 0 and "GDP_MISTAKE" in r.stderr

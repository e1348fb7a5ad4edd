"""CPU: the shared core of the wavefront walks (genome-on-diet_amd/csrc/ksw_walk_core.h: a window of 64 fetched cells consumed from
wave-uniform masks, a run of diagonal cells in one step) in a 64-lane emulation of the device loop (tests/emul/walk_emul.cpp) against the
oracle's gdo_backtrack on synthetic backtrace matrices: lengths 1..400, bands 8, 50, 239, 1000 and -1, direction 0 in 90 %, 99 % and
100 % of the cells, planted match runs of 1, 63, 64, 65, 127, 128, 129 cells ended by each gap state, gaps longer than a window, walks
that start in a forced state, runs that end at the matrix's edge; every matrix in one piece and in chunks of 32 and 192 anti-diagonals,
each at a CIGAR capacity of 0, 1, 3 and ample.  On matrices of direction 0 only a walk of L cells takes at most ceil(L / 64) + 2 loop
iterations.  Once more as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

from conftest import ROOT

STATS = (r"walk_emul cases=(\d+) mismatches=(\d+) planted=(\d+) forced_start=(\d+) edge_end=(\d+) capped=(\d+) max_ops=(\d+) "
         r"counted=(\d+) worst_step_excess=(-?\d+)")


def _build(exe, flags):
    subprocess.check_call(["g++", "-w", *flags, "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"), "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "emul", "walk_emul.cpp"), "-x", "c", os.path.join(ROOT, "oracle", "gdo_ksw2.c"), "-o", exe])


def _check(out):
    assert out.returncode == 0, out.stdout + out.stderr
    cases, bad, planted, forced, edge, capped, max_ops, counted, excess = (int(x) for x in re.search(STATS, out.stdout).groups())
    assert bad == 0
    assert cases >= 20000
    # every kind of input is really there: planted paths, walks whose first cell lies outside the stored window of its row, walks that
    # reach the edge of the matrix before its corner, CIGARs longer than the capacity (counted, not stored) and long ones that fit
    assert planted >= 500 and forced >= 100 and edge >= 500 and capped >= 5000 and max_ops >= 30
    # direction 0 everywhere: at most ceil(L / 64) + 2 iterations for L cells (the cell-at-a-time loop takes L)
    assert counted >= 100 and excess <= 0


def test_walk_windows_match_oracle_backtrack(tmp_path):
    exe = str(tmp_path / "walk_emul")
    _build(exe, ["-O2"])
    _check(subprocess.run([exe, "1"], capture_output=True, text=True))


def test_walk_windows_under_address_and_ub_sanitizers(tmp_path):
    """the same program and cases, compiled with -fsanitize=address,undefined: any report aborts the run (the CIGAR buffers are exactly
    as long as the capacity)"""
    exe = str(tmp_path / "walk_emul_san")
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    _check(subprocess.run([exe, "1"], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")))

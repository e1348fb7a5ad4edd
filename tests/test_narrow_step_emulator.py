"""CPU: the half-block rows of the 64-lane DP kernel's narrow form with the two-lane selector update of their paired steady rows
(gdw_narrow_rows, ksw_wave.hip.h; gdw_sel_step_half, ksw_wave_core.h) in a lock-step emulator of 64 lanes
(tests/emul/narrow_step_emul.cpp) against the oracle at the band they run, over the grid of tests/emul/narrow_emul.cpp -- which stays as
the record of the statements before the update: bands 495, 494, 493, 479, 247 and 119, tlen mod 16 in {0, 1, 7, 8, 9, 15},
|tlen - qlen| in {0, 1, w - 1, w}, lengths around the band and long enough for the paired steady rows.  Every cell of every in-band row
must have been stored, the ring must hold 64 distinct half blocks on every row, and most first rows of a pair must have taken the
two-lane path."""
import os
import re
import subprocess

from conftest import ROOT


def test_half_block_rows_with_selector_steps_match_oracle(tmp_path):
    exe = str(tmp_path / "narrow_step_emul")
    subprocess.check_call(["g++", "-O2", "-w", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"), "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "emul", "narrow_step_emul.cpp"), "-x", "c", os.path.join(ROOT, "oracle", "gdo_ksw2.c"), "-o", exe])
    out = subprocess.run([exe, "1"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"pairs_run=(\d+) skipped=(\d+) mismatches=(\d+) rows=(\d+) paired_rows=(\d+) patched_pairs=(\d+)", out.stdout)
    run, skipped, bad, rows, paired, patched = (int(x) for x in m.groups())
    # |tlen - qlen| == w is never admitted: those 2 of 7 length differences are the skipped ones, as in narrow_emul.cpp
    assert bad == 0 and run >= 500 and skipped * 7 == (run + skipped) * 2
    assert paired > rows // 4
    # no band of the grid is a multiple of 16: of the pairs (paired // 2) all but the first of an alignment and one in 16 are patched
    assert paired // 2 * 14 // 16 < patched < paired // 2 * 15 // 16

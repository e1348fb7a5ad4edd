"""CPU: the quarter-block rows of the 64-lane DP kernel with the two-lane selector update of their paired steady rows (gdw_quarter_rows,
ksw_wave.hip.h; gdw_sel_step_quarter, ksw_wave_core.h) in a lock-step emulator of 64 lanes (tests/emul/quarter_step_emul.cpp) against the
oracle at the band they run, over the grid of tests/emul/quarter_emul.cpp -- which stays as the record of the statements before the
update: bands 239, 238, 237, 223, 119 and 55; tlen mod 16 on and next to every quarter boundary; |tlen - qlen| in {0, 1, w - 1}; lengths
around the band and at least 2 w + 200.  Every cell of every in-band row must have been stored, the ring must hold 64 distinct quarter
blocks on every row, and most first rows of a pair must have taken the two-lane path."""
import os
import re
import subprocess

from conftest import ROOT

STATS = (r"by_delta (\d+) (\d+) (\d+) by_length (\d+) (\d+) (\d+)\nquarter_step_emul pairs_run=(\d+) skipped=(\d+) mismatches=(\d+) rows=(\d+) "
         r"paired_rows=(\d+) patched_pairs=(\d+)")


def test_quarter_block_rows_with_selector_steps_match_oracle(tmp_path):
    exe = str(tmp_path / "quarter_step_emul")
    subprocess.check_call(["g++", "-w", "-O2", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"), "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "emul", "quarter_step_emul.cpp"), "-x", "c", os.path.join(ROOT, "oracle", "gdo_ksw2.c"), "-o", exe])
    out = subprocess.run([exe, "1"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    d0, d1, dw, l0, l1, l2, run, skipped, bad, rows, paired, patched = (int(x) for x in re.search(STATS, out.stdout).groups())
    assert bad == 0 and "mismatches=0" in out.stdout
    # the grid of quarter_emul.cpp: 6 bands x 12 residues x 5 length differences x 3 length classes, a fifth of it not admitted
    assert run + skipped == 1080 and skipped * 5 == run + skipped
    assert (d0, d1, dw) == (216, 432, 216) and l0 == l1 == l2 == 288
    assert paired > rows // 4
    # no band of the grid is a multiple of 16: of the pairs (paired // 2) all but the first of an alignment and one in 16 are patched
    assert paired // 2 * 14 // 16 < patched < paired // 2 * 15 // 16

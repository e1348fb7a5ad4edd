"""CPU: the half-block rows of the 64-lane DP kernel's narrow form (gdw_narrow_rows, ksw_wave.hip.h) in a lock-step emulator of 64 lanes
(tests/emul/narrow_emul.cpp) against the oracle at the band they run: bands at the admission limit GD_W_NARROW and one and two below
it (and narrower ones), tlen mod 16 in {0, 1, 7, 8, 9, 15}, |tlen - qlen| in {0, 1, w - 1, w}, lengths around the band and long enough
for the paired steady rows, Ns in target and query.  The emulator also requires every cell of every in-band row to have been stored and
the ring to hold 64 distinct half blocks on every row."""
import os
import re
import subprocess

from conftest import ROOT


def test_half_block_rows_match_oracle_at_their_band(tmp_path):
    exe = str(tmp_path / "narrow_emul")
    subprocess.check_call(["g++", "-O2", "-w", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"), "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "emul", "narrow_emul.cpp"), "-x", "c", os.path.join(ROOT, "oracle", "gdo_ksw2.c"), "-o", exe])
    out = subprocess.run([exe, "1"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"pairs_run=(\d+) skipped=(\d+) mismatches=(\d+) rows=(\d+) paired_rows=(\d+)", out.stdout)
    run, skipped, bad, rows, paired = (int(x) for x in m.groups())
    # |tlen - qlen| == w is never admitted (the last cell sits on the band's edge): those 2 of 7 length differences are the skipped ones
    assert bad == 0 and run >= 500 and skipped * 7 == (run + skipped) * 2
    assert paired > rows // 4  # the paired steady rows are well represented beside the general ones

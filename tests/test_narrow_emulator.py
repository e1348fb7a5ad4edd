"""CPU: the half-block rows of the 64-lane DP kernel's narrow form (gdw_narrow_rows, ksw_wave.hip.h) in a lock-step emulator of 64 lanes
(tests/emul/narrow_emul.cpp) against the oracle at the band they run: bands at the admission limit GD_W_NARROW and one and two below
it (and narrower ones), tlen mod 16 in {0, 1, 7, 8, 9, 15}, |tlen - qlen| in {0, 1, w - 1, w}, lengths around the band and long enough
for the paired steady rows, Ns in target and query.  The emulator also requires every cell of every in-band row to have been stored and
the ring to hold 64 distinct half blocks on every row."""
import os
import re
import subprocess

import gdo
import pytest

from conftest import ROOT

PRESETS = ("sr", "hifi", "ont")
# the other scorings of the oracle's table that reach the narrow band (dual-affine, taken by the register-resident kernels)
OFF_PRESET = [k for k, v in gdo.SCORINGS.items() if gdo.wave_scoring_ok(*v) and k not in PRESETS]


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


@pytest.fixture(scope="module")
def scoring_runs(tmp_path_factory):
    """the whole geometry grid once per off-preset scoring, every pair at that scoring: the runs (17 s each) side by side"""
    from concurrent.futures import ThreadPoolExecutor
    exe = str(tmp_path_factory.mktemp("emul") / "narrow_emul")
    subprocess.check_call(["g++", "-O2", "-w", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"), "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "emul", "narrow_emul.cpp"), "-x", "c", os.path.join(ROOT, "oracle", "gdo_ksw2.c"), "-o", exe])
    pool = ThreadPoolExecutor(max_workers=max(1, min(8, (os.cpu_count() or 2) - 1)))
    runs = {k: pool.submit(subprocess.run, [exe, "1", "scoring"] + [str(x) for x in gdo.SCORINGS[k]], capture_output=True, text=True) for k in OFF_PRESET}
    yield runs
    pool.shutdown(wait=True)


@pytest.mark.parametrize("name", OFF_PRESET)
def test_half_block_rows_match_oracle_off_preset(scoring_runs, name):
    """the constants from the driver's own derivation (gd_derive_consts), the oracle with the caller's order of the gap models and the
    score of N in its matrix; at "swapped" the emulator's score plus the bias is the oracle's"""
    out = scoring_runs[name].result()
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"pairs_run=(\d+) skipped=(\d+) mismatches=(\d+) rows=(\d+) paired_rows=(\d+)", out.stdout)
    run, skipped, bad, rows, paired = (int(x) for x in m.groups())
    assert bad == 0 and "mismatches=0" in out.stdout
    assert run >= 500
    assert paired > rows // 4

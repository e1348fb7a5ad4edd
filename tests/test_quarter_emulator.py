"""CPU: the quarter-block rows of the 64-lane DP kernel (gdw_quarter_rows, ksw_wave.hip.h) in a lock-step emulator of 64 lanes
(tests/emul/quarter_emul.cpp) against the oracle at the band they run: bands 239 (the admission limit GD_W_QUARTER), 238, 237, 223, 119
and 55; tlen mod 16 in {0, 1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15} -- on and next to every quarter boundary; |tlen - qlen| in {0, 1, w - 1};
lengths around the band and at least 2 w + 200, so that the ring of 16 blocks wraps several times; Ns in target and query.  The emulator
also requires every cell of every in-band row to have been stored and the ring to hold 64 distinct quarter blocks on every row.  Once
more as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

import gdo
import pytest

from conftest import ROOT

PRESETS = ("sr", "hifi", "ont")
# the other scorings of the oracle's table that reach the narrow bands (dual-affine, taken by the register-resident kernels)
OFF_PRESET = [k for k, v in gdo.SCORINGS.items() if gdo.wave_scoring_ok(*v) and k not in PRESETS]
STATS = r"by_delta (\d+) (\d+) (\d+) by_length (\d+) (\d+) (\d+)\nquarter_emul pairs_run=(\d+) skipped=(\d+) mismatches=(\d+) rows=(\d+) paired_rows=(\d+)"


def _build(exe, flags):
    subprocess.check_call(["g++", "-w", *flags, "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"), "-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "emul", "quarter_emul.cpp"), "-x", "c", os.path.join(ROOT, "oracle", "gdo_ksw2.c"), "-o", exe])


def _check(out):
    assert out.returncode == 0, out.stdout + out.stderr
    d0, d1, dw, l0, l1, l2, run, skipped, bad, rows, paired = (int(x) for x in re.search(STATS, out.stdout).groups())
    assert bad == 0 and "mismatches=0" in out.stdout
    # 6 bands x 12 residues x 5 length differences x 3 length classes; tlen - qlen == w - 1 is not admitted (the last block would hold
    # fewer than 17 cells of the band), qlen - tlen == w - 1 is: that fifth is the skipped one
    assert run + skipped == 1080 and skipped * 5 == run + skipped
    assert (d0, d1, dw) == (216, 432, 216) and l0 == l1 == l2 == 288
    assert paired > rows // 4  # the paired steady rows are well represented beside the general ones


def test_quarter_block_rows_match_oracle_at_their_band(tmp_path):
    exe = str(tmp_path / "quarter_emul")
    _build(exe, ["-O2"])
    _check(subprocess.run([exe, "1"], capture_output=True, text=True))


def test_quarter_block_rows_under_address_and_ub_sanitizers(tmp_path):
    """the same program and grid, compiled with -fsanitize=address,undefined: any report aborts the run"""
    exe = str(tmp_path / "quarter_emul_san")
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    _check(subprocess.run([exe, "1"], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")))


@pytest.fixture(scope="module")
def scoring_runs(tmp_path_factory):
    """the whole geometry grid once per off-preset scoring, every pair at that scoring: the runs side by side"""
    from concurrent.futures import ThreadPoolExecutor
    exe = str(tmp_path_factory.mktemp("emul") / "quarter_emul")
    _build(exe, ["-O2"])
    pool = ThreadPoolExecutor(max_workers=max(1, min(8, (os.cpu_count() or 2) - 1)))
    runs = {k: pool.submit(subprocess.run, [exe, "1", "scoring"] + [str(x) for x in gdo.SCORINGS[k]], capture_output=True, text=True) for k in OFF_PRESET}
    yield runs
    pool.shutdown(wait=True)


def test_eight_off_preset_scorings():
    assert len(OFF_PRESET) == 8


@pytest.mark.parametrize("name", OFF_PRESET)
def test_quarter_block_rows_match_oracle_off_preset(scoring_runs, name):
    """the constants from the driver's own derivation (gd_derive_consts), the oracle with the caller's order of the gap models and the
    score of N in its matrix; at "swapped" the emulator's score plus the bias is the oracle's"""
    _check(scoring_runs[name].result())

"""CPU: the two-lane update of the score selectors in the paired steady rows of the quarter-block and half-block forms of the 64-lane DP
kernel (gdw_sel_step_quarter / gdw_sel_step_half, ksw_wave_core.h; the pair rows of gdw_quarter_rows / gdw_narrow_rows, ksw_wave.hip.h).
tests/emul/sel_step_test.cpp keeps 64 lanes' (blk, quarter | half, SEL, m_lowest) through the device's row loop with its statements and
compares every lane, after the first row of every pair, with what gdw_make_sel_quarter / gdw_make_sel_half and the m_lowest expression
give outright: quarter bands 239, 238, 237, 223, own bands 224 | 225 on both sides of a multiple of 16, and 119 and 55 of the emulator's
grid; half bands 495, 494, 479 | 480 | 481, 400 | 401, 247 and 119; tlen mod 16 on and next to every quarter and half boundary;
|tlen - qlen| in {0, 1, w - 1, w}; lengths from just below the band to 5 w + 700.  Plain, and the same stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

from conftest import ROOT

LINE = r"(quarter|half) band (\d+) geometries (\d+) rows (\d+) full_pairs (\d+) patched_pairs (\d+) ring_wraps (\d+)"
QUARTER = (239, 238, 237, 223, 224, 225, 119, 55)
HALF = (495, 494, 479, 480, 481, 400, 401, 247, 119)


def _build(exe, flags):
    subprocess.check_call(["g++", "-w", *flags, "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul", "sel_step_test.cpp"), "-o", exe])


def _check(out):
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.rstrip().endswith("sel_step_test ok")
    got = {(k, int(w)): tuple(int(x) for x in rest) for k, w, *rest in re.findall(LINE, out.stdout)}
    assert sorted(got) == sorted([("quarter", w) for w in QUARTER] + [("half", w) for w in HALF])
    for (kind, w), (geoms, rows, full, patched, wraps) in got.items():
        assert geoms >= 300 and wraps >= geoms // 4  # (the ring goes round several times in the long alignments)
        if w % 16 == 0:  # the two rows of a pair differ in `up`: the kept statements, every pair
            assert patched == 0 and full > rows // 8
        else:  # the first pair of an alignment and one pair in 16 make the selectors, every other pair patches two lanes
            assert full > geoms // 2 and 13 * full < patched < 15 * full


def test_selector_steps_equal_selectors_made_outright(tmp_path):
    exe = str(tmp_path / "sel_step_test")
    _build(exe, ["-O2"])
    _check(subprocess.run([exe], capture_output=True, text=True))


def test_selector_steps_under_address_and_ub_sanitizers(tmp_path):
    """the same program and grid, compiled with -fsanitize=address,undefined: any report aborts the run"""
    exe = str(tmp_path / "sel_step_test_san")
    _build(exe, ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    _check(subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")))

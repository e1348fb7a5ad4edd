"""CPU: the seam stream of the paired steady rows of the quarter-block and half-block forms of the 64-lane DP kernel (GdwSeam, gdw_seam_init /
gdw_seam_next in ksw_wave_core.h; the pair rows of gdw_quarter_rows / gdw_narrow_rows in ksw_wave.hip.h), as stand-alone programs, plain and
under AddressSanitizer and UndefinedBehaviorSanitizer.
tests/emul/seam_stream_test.cpp: on every paired row of the geometry grid of sel_step_test.cpp (quarter bands 239 ... 55, half bands
495 ... 119, 12 residues of tlen, 7 length differences, 7 lengths), with the query at each byte place of an aligned 8-byte window and with
query lengths at which j reaches qlen - 1, qlen and qlen + 14 inside the paired rows, the stream's byte equals gdw_qbyte and a host copy of
gdw_seam_byte, and every dword the stream loads is 4-aligned and holds a byte of the query.
tests/emul/quarter_seam_emul.cpp, narrow_seam_emul.cpp: the step emulators with the pair rows as they are now (stream, selector step,
target-N term under its branch), statement by statement against the oracle over the emulators' grids, every in-band cell stored."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "genome-on-diet_amd", "csrc")
PLAIN = ["-O2"]
SAN = ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
QUARTER = (239, 238, 237, 223, 224, 225, 119, 55)
HALF = (495, 494, 479, 480, 481, 400, 401, 247, 119)


def _run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))


@pytest.mark.parametrize("flags", [PLAIN, SAN], ids=["plain", "asan_ubsan"])
def test_stream_equals_seam_byte_on_every_paired_row(tmp_path, flags):
    exe = str(tmp_path / "seam_stream_test")
    subprocess.check_call(["g++", "-w", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "emul", "seam_stream_test.cpp"), "-o", exe])
    out = _run(exe)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.rstrip().endswith("seam_stream_test ok")
    got = {(k, int(w)): (int(g), int(r)) for k, w, g, r in re.findall(r"(quarter|half) band (\d+) geometries (\d+) paired_rows (\d+)", out.stdout)}
    assert sorted(got) == sorted([("quarter", w) for w in QUARTER] + [("half", w) for w in HALF])
    # 8 places of the query for every geometry: those of sel_step_test.cpp (at least 300 a band) and the 16 lengths that end by the query
    assert all(g >= 8 * 300 and r > 100 * g for g, r in got.values())
    tot = dict((k, int(v)) for k, v in re.findall(r"(\w+)=(\d+)", out.stdout.rstrip().split("\n")[-2]))
    assert tot["j_qlen_m1"] > 0 and tot["j_qlen"] > 0 and tot["j_qlen_p14"] > 0 and tot["past_end"] > tot["j_qlen"]
    # one block taken over in 16 pairs (32 rows); a window of 8 bytes serves 8 rows and is read as at most two dwords
    assert tot["paired_rows"] // 40 < tot["steps_back"] < tot["paired_rows"] // 30
    assert tot["paired_rows"] // 10 < tot["refills"] and tot["loads"] < tot["paired_rows"] // 2


@pytest.mark.parametrize("flags", [PLAIN, SAN], ids=["plain", "asan_ubsan"])
@pytest.mark.parametrize("name", ["quarter_seam_emul", "narrow_seam_emul"])
def test_pair_rows_with_the_stream_match_oracle(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-w", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "emul", name + ".cpp"),
                           "-x", "c", os.path.join(ROOT, "oracle", "gdo_ksw2.c"), "-o", exe])
    out = _run(exe, "1")
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(name + r" pairs_run=(\d+) skipped=(\d+) mismatches=(\d+) rows=(\d+) paired_rows=(\d+) patched_pairs=(\d+) seam_loads=(\d+)", out.stdout)
    run, skipped, bad, rows, paired, patched, loads = (int(x) for x in m.groups())
    # the grids of the step emulators (tests/test_quarter_step_emulator.py, tests/test_narrow_step_emulator.py)
    if name == "quarter_seam_emul":
        assert run + skipped == 1080 and skipped * 5 == run + skipped
    else:
        assert run >= 500 and skipped * 7 == (run + skipped) * 2
    assert bad == 0 and paired > rows // 4
    assert paired // 2 * 14 // 16 < patched < paired // 2 * 15 // 16
    assert paired // 8 < loads < paired // 2  # every paired row took its byte from the stream

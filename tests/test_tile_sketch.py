"""CPU: the position-parallel sketch of the wave seed kernel (map_tile_sketch.h) on 64 emulated lock-step lanes against the sequential
automaton gd_sketch_core (tests/emul/tile_sketch_test.cpp): every (x, y) in order, the count, the cut at a cap and tmp_extracted_len,
over patterns 10 / 1 / 110 / 0001 / 40 ones at every shift, k in {11, 15, 19, 21, 28}, w in {1, 8, 10, 19, 33, 64}; plain and under
ASan / UBSan."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

# how often the rare paths must fire in one run: steps with a tie enumeration (on leaving the window / in the first full window), N flushes,
# capped lists cut at the cap, lists that do not fit -- counted by the program from gd_sketch_core / gd_sketch_slice alone
MIN_FIRED = {"tie_leave": 200, "tie_first": 400, "n_flush": 500, "cap_cut": 10000, "overflow_checks": 1000}


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_tile_sketch_equals_sequential_sketch(tmp_path, flags):
    exe = str(tmp_path / "tile_sketch_test")
    subprocess.check_call(["g++", "-std=c++17", "-w"] + flags + ["-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul", "tile_sketch_test.cpp"), "-o", exe])
    for seed in ("1", "2"):
        out = subprocess.run([exe, seed], capture_output=True, text=True)
        print(out.stdout)
        assert out.returncode == 0 and " mismatches=0 " in out.stdout, out.stdout + out.stderr
        got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.stdout)}
        assert got["runs"] > 40000
        for k, v in MIN_FIRED.items():
            assert got[k] >= v, (k, got[k], v)

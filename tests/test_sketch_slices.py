"""CPU: exact slicing of the winnowing automaton (the property the wave-parallel seed kernel relies on):
concatenated gd_sketch_slice() outputs == sequential gd_sketch_core() output, incl. Ns, tandem repeats, homopolymers."""
import os
import subprocess

import pytest

from conftest import ROOT
from fixture_io import PRESET_PATTERN, grid_ids, grid_row


@pytest.fixture(scope="module")
def slice_test(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slices") / "slice_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul", "sketch_slice_test.cpp"), "-o", exe])
    return exe


def test_slices_equal_sequential_sketch(slice_test):
    exe = slice_test
    for seed in ("1", "2"):
        out = subprocess.run([exe, seed, "400"], capture_output=True, text=True)
        assert out.returncode == 0 and "mismatches=0" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("name", grid_ids("kw"))
def test_slices_equal_sequential_sketch_at_grid_settings(slice_test, name):
    """the same property at every pattern / k / w row of the option grid: a slice that starts in the middle of a pattern period (the
    iq / ir carry of gd_sketch_range from i_begin / ones, i_begin % ones), patterns of up to 50 positions and 40 ones, k = 28, w = 1, 64"""
    row = grid_row(name)
    o = row["overrides"]
    base = PRESET_PATTERN[row["variant"] if row["variant"] == "sr" else row["kind"].split("_")[0]]
    k, w, z = o.get("k", base[0]), o.get("w", base[1]), o.get("Z", "10")
    out = subprocess.run([slice_test, "3", "150", str(k), str(w), z], capture_output=True, text=True)
    assert out.returncode == 0 and "iters=150 mismatches=0" in out.stdout, out.stdout + out.stderr

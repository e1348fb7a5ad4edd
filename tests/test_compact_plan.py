"""CPU: the compact backtrace arena of the DP planner (ksw_plan.h, tests/emul/compact_plan_test.cpp) on random batch geometries: slot
sizes and order, the overflow pool behind the last slot, the layout without the option, and a host model of the kernel's claim that
confirms the planner's number of drain launches when every box falls back and the pool is empty.  The program ends with status 1 at the
first property that does not hold; here the batches are checked to have been of the kinds they were built as.  Built plain and under
ASan / UBSan."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.parametrize("sanitize", [False, True])
def test_compact_layout_and_drain_launches(tmp_path, sanitize):
    exe = str(tmp_path / "compact_plan_test")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"),
           os.path.join(ROOT, "tests", "emul", "compact_plan_test.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in r.stdout.splitlines():
        name, *fields = line.split()
        got[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    hifi = [v for k, v in got.items() if k.startswith("hifi")]
    assert len(hifi) == 12 and all(v["try"] > 0 for v in hifi)
    # a batch of mostly whole reads needs clearly less than the full-size layout, and the model never took more launches than planned
    assert any(v["n"] >= 200 and v["bt"] < 0.7 * v["full_bt"] for v in hifi)
    assert all(1 <= v["model"] <= v["drain"] for v in got.values() if v["try"])
    # pool 0: the arena is the slots alone; one box, two boxes: grown to the largest box
    assert any(v["pool"] == 0 for v in hifi)
    assert got["one"]["drain"] == 1 and got["one"]["bt"] == got["one"]["full_bt"] and got["two"]["drain"] == 2
    # 24 equal boxes in half of what they need: 11 fit a launch beside the room kept for the largest
    assert got["twentyfour"]["bt"] * 2 > got["twentyfour"]["full_bt"] * 0.99 and got["twentyfour"]["drain"] == 3 and got["twentyfour"]["model"] >= 2
    # nothing to compact: the full-size layout
    for name in ("short", "single"):
        assert got[name]["try"] == 0 and got[name]["bt"] == got[name]["full_bt"]

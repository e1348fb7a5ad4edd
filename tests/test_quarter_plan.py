"""CPU: admission, rung decision and auto mode of the 64-lane DP kernel's quarter form (tests/emul/quarter_plan_test.cpp): GD_W_QUARTER = 239
is the widest band that fits 16 blocks for every geometry; the O(1) admission test the kernel evaluates equals its loop form on random
geometries and what it admits satisfies what the quarter-block rows need anti-diagonal by anti-diagonal (gd_quarter_rows_ok); the rung the
kernel decides on from the planner's mark and the geometry (gd_quarter_rung) is its definition on the hifi / own / mix batches of the
planner test; the auto mode stops offering the rung below break-even, probes again after its hold and ignores launches with fewer than
64 tries."""
import os
import subprocess

from conftest import ROOT


def test_quarter_admission_rung_and_auto_mode(tmp_path):
    exe = str(tmp_path / "quarter_plan_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul", "quarter_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe, "300000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    head = lines[0].split()
    f = dict(zip(head[0::2], (int(x) for x in head[1::2])))
    assert f["w_quarter"] == 239 and f["cases"] == 300000 and f["differ"] == 0 and f["rows_bad"] == 0
    assert 0.2 * f["cases"] < f["admitted"] < 0.8 * f["cases"] and f["rows_checked"] > 20000
    rungs = {}
    for line in lines[1:4]:
        _, name, *fields = line.split()
        rungs[name] = {k: int(v) for k, v in (x.split("=") for x in fields)}
    # every box of a HiFi batch, and every box at its own band between 300 and 495, tries the 239 rung first
    assert rungs["hifi"]["at239"] == rungs["hifi"]["n"] == 3000
    assert rungs["own"]["at239"] == rungs["own"]["n"] == 3000
    assert rungs["mix"]["at239"] > 2000 and rungs["mix"]["none"] > 1500
    assert lines[4].startswith("auto ok")

"""CPU: admission and planning of the 64-lane DP kernel's narrow form (tests/emul/narrow_plan_test.cpp): GD_W_NARROW is the widest band
that fits 32 blocks for every geometry; the O(1) admission test equals its loop form on random geometries and what it admits satisfies
what the half-block rows need anti-diagonal by anti-diagonal; gd_plan_batch marks the boxes that try the narrow band first (band wider
than GD_W_NARROW, lengths no further apart than it), those that run their own narrow band, and nothing else -- none in a single-affine
batch -- while the arena keeps a full-band slot for every alignment."""
import os
import subprocess

from conftest import ROOT


def test_narrow_admission_and_marks(tmp_path):
    exe = str(tmp_path / "narrow_plan_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul", "narrow_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe, "300000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    head = lines[0].split()
    f = dict(zip(head[0::2], (int(x) for x in head[1::2])))
    assert f["w_narrow"] == 495 and f["cases"] == 300000 and f["differ"] == 0 and f["rows_bad"] == 0
    assert 0.2 * f["cases"] < f["admitted"] < 0.8 * f["cases"] and f["rows_checked"] > 20000
    plans = {}
    for line in lines[1:]:
        _, name, *fields = line.split()
        plans[name] = {k: int(v) for k, v in (x.split("=") for x in fields)}
    assert plans["hifi"]["try"] == plans["hifi"]["n"] == 3000
    assert plans["own"]["own"] == plans["own"]["n"] == 3000
    assert min(plans["mix"][k] for k in ("try", "own", "no")) > 500
    assert plans["hifi_single"]["no"] == 3000 and plans["hifi_single"]["bt"] == plans["hifi"]["bt"]

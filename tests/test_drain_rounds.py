"""CPU: the rounds of the drain launches over a pending list (ksw_plan.h: gd_drain_rounds and the replay of the kernel's claim,
tests/emul/drain_rounds_test.cpp): nothing pending, one box in an arena of its size, every box pending, an arena of the largest box, and
200 random sets of up to 64 boxes of 256 B .. 64 KB in arenas between the largest box and the total.  The program checks by brute force
that every box is served exactly once in slots that are disjoint within a round and inside the arena, in six orders of arrival, and ends
with status 1 at the first property that does not hold; here the cases are checked to have been what they were built as.  Built plain
and under ASan / UBSan."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.parametrize("sanitize", [False, True])
def test_drain_rounds(tmp_path, sanitize):
    exe = str(tmp_path / "drain_rounds_test")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"),
           os.path.join(ROOT, "tests", "emul", "drain_rounds_test.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", r.stdout[-2000:] + r.stderr[-2000:]
    got = {}
    for line in r.stdout.splitlines()[:-1]:
        name, *fields = line.split()
        got[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    assert len(got) == 204
    assert got["none"]["rounds"] == 0 and got["none"]["used"] == 0 and got["none"]["planned"] > 0  # the batch had planned some: none is enqueued
    assert got["one"]["rounds"] == 1 and got["one"]["used"] == 1
    assert got["all"]["n"] == 40 and 2 <= got["all"]["used"] <= got["all"]["rounds"] == got["all"]["planned"]
    assert got["one_per_round"]["used"] == got["one_per_round"]["rounds"] == got["one_per_round"]["n"] == 17
    draws = [v for k, v in got.items() if k.startswith("draw")]
    assert len(draws) == 200 and all(1 <= v["used"] <= v["own"] <= v["allowed"] and v["own"] <= v["rounds"] <= v["planned"] for v in draws)
    # the draws reach both ends: sets served in one round, and sets that need several
    assert any(v["used"] == 1 and v["n"] > 1 for v in draws) and any(v["used"] >= 3 for v in draws)
    # a set inside a larger batch gets fewer rounds than the batch had planned
    assert any(v["rounds"] < v["planned"] for v in draws)

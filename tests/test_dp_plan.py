"""CPU: the planner of a DP batch (gd_plan_batch, ksw_plan.h) on seeded batches shaped like those of the mapping modes
(tests/emul/dp_plan_test.cpp).  Every batch of every mode goes through it: which kernel takes an alignment, where its backtrace lies,
the groups and pipeline runs the short-alignment kernels are launched over.  The program checks each plan against what the kernels
need and ends with status 1 at the first property that does not hold; here the batches are checked to have reached the paths they
were built for."""
import os
import subprocess

from conftest import ROOT


def test_plans_of_seeded_batches_hold_what_the_kernels_need(tmp_path):
    exe = str(tmp_path / "dp_plan_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul", "dp_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in r.stdout.splitlines():
        name, *fields = line.split()
        got[name] = {k: [int(x) for x in v.split(",")] for k, v in (f.split("=") for f in fields)}
    one = lambda name, key: got[name][key][0]
    generic, wave64, wave16, wave128 = range(4)

    # short reads: at least 100 000 pairs, all on the pipelines, as a root context and as a lane (whose pipes are longer: fewer wavefronts)
    for name in ("sr_root", "sr_lane"):
        assert one(name, "n") >= 100000 and one(name, "err") == 0
        assert got[name]["kinds"][wave16] == one(name, "n") == one(name, "pipe_ids") and one(name, "runs") >= 1
    assert one("sr_lane", "pipes") < one("sr_root", "pipes")
    # without pipelines the same batch fills the 10- and 8-lane groups; forced to 16 lanes, those
    assert one("sr_nopipe", "runs") == 0 and got["sr_nopipe"]["groups"][0] == 0 and min(got["sr_nopipe"]["groups"][1:]) > 0
    assert got["sr_lanes16_nopipe"]["groups"][0] >= one("sr_lanes16_nopipe", "n") and got["sr_lanes16_nopipe"]["groups"][1:] == [0, 0]
    # 241..256 bases, full matrix: nothing but the pipelines takes them, however few share a geometry
    assert one("pipe_only", "pipe_ids") == one("pipe_only", "n") and got["pipe_only"]["groups"] == [0, 0, 0]
    # HiFi: the 64-lane kernel; ONT: wide bands, checkpointed from 1 024 alignments on (5 120 wavefront slots), both ring forms in use
    assert got["hifi"]["kinds"][wave64] == one("hifi", "n") >= 2000
    assert got["ont"]["kinds"][wave128] == one("ont", "n") >= 1024 and one("ont", "wide_ck") == 1 and 0 < one("ont", "ring96") < one("ont", "n")
    assert got["ont_few"]["kinds"][wave128] == one("ont_few", "n") < 1024 and one("ont_few", "wide_ck") == 0
    assert one("ont_nockpt", "wide_ck") == 0 and one("ont_few_ckpt", "wide_ck") == 1 and one("ont_single", "wide_ck") == 0
    # the mix: every kernel at once
    for name in ("mix_root", "mix_lane"):
        assert one(name, "mask") == 31 and min(got[name]["kinds"]) > 0 and min(got[name]["groups"]) > 0 and one(name, "runs") > 0
        assert one(name, "wide_ck") == 1 and 0 < one(name, "ring96") < got[name]["kinds"][wave128]
    for name in ("mix_generic", "mix_scoring"):
        assert got[name]["kinds"] == [one(name, "n"), 0, 0, 0]
    # errors and their precedence: empty sequence (1), no wave kernel in wave-only mode (2), beyond the generic kernel's LDS window (4)
    assert one("sr_waveonly", "err") == 0 and one("mix_waveonly", "err") == 2
    assert [one(k, "err") for k in ("big", "big_generic", "big_waveonly", "big_empty", "big_empty_waveonly", "sr_empty")] == [4, 4, 2, 1, 1, 1]

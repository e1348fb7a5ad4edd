"""CPU: the host tables of a mapping call (map_plan.h) on seeded synthetic batches (tests/emul/map_plan_test.cpp): the capacity
classes of the seed kernel, the scratch layout, the box tables of the host box stage and the reads it fails.  On a GPU this code runs
inside every mapping call; here it runs alone.  The program checks each table against what the kernels and the later stages need and
ends with status 1 at the first property that does not hold; here the scenarios are checked to have reached the cases they were
built for."""
import os
import subprocess

from conftest import ROOT


def test_host_tables_of_seeded_batches_hold_what_the_stages_need(tmp_path):
    exe = str(tmp_path / "map_plan_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul", "map_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for line in r.stdout.splitlines():
        name, *fields = line.split()
        got[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}

    # capacity classes: the ONT mix spreads over every capacity, longest first; one capacity for all reads, or one read, gives no list
    assert got["classes_ont"]["n"] == 3000 and got["classes_ont"]["classes"] == got["classes_ont"]["caps_used"] == 4
    assert got["classes_ont"]["sort_cap"] == 16384
    assert got["classes_hifi"] == dict(n=3000, classes=0, caps_used=1, sort_cap=2048)
    assert got["classes_hifi_long"] == dict(n=500, classes=0, caps_used=1, sort_cap=8192)
    assert got["classes_one_read"] == dict(n=1, classes=0, caps_used=1, sort_cap=16384)
    assert got["classes_two_reads"] == dict(n=2, classes=2, caps_used=2, sort_cap=16384)
    # layouts: both forms were laid out
    for name in ("layout_ont", "layout_sr"):
        assert got[name]["tot_full"] > got[name]["tot"] > 0
    # the host box stage on seeded votes, both variants: boxes on both strands, reads without candidates, contigs that do not exist
    for name, n in (("votes_sr", 6000), ("votes_lr", 1500)):
        g = got[name]
        assert g["n"] == n and g["boxes"] > n and g["rev"] > 0 and g["rev"] < g["boxes"] and g["empty"] > 0 and g["no_contig"] > 0
    assert got["votes_lr"]["hanging"] > 0  # (the ShortReads geometry clips its boxes at the contig's end itself)
    assert got["votes_sr"]["bw_lo"] > 0 and got["votes_sr"]["bw_hi"] > 0 and got["votes_sr"]["failed"] > 0
    # ... and on seeded boxes: every kind of window the reference reads stale memory for is there, and none fails its read
    for name in ("tables_sr", "tables_lr"):
        g = got[name]
        assert g["n"] == 400 and g["failed"] == 0 and g["last"] == -1
        assert min(g["boxes"], g["hanging"], g["beyond"], g["no_contig"], g["rev"], g["empty"]) > 0
    assert got["tables_sr"]["bw_lo"] > 0 and got["tables_sr"]["bw_hi"] > 0 and got["tables_lr"]["bw_lo"] == got["tables_lr"]["bw_hi"] == 0
    # failed reads: one per term of the predicate (terms = 0b11111) and the fault-injected one, which must own boxes to fail
    assert got["failed"] == dict(n=12, boxes=15, failed=6, last=8, terms=31, warned=1)
    for name in ("failed_no_fault", "failed_fault_on_empty_read", "failed_fault_on_failed_read"):
        assert got[name] == dict(n=12, boxes=18, failed=5, last=5, terms=31, warned=1)

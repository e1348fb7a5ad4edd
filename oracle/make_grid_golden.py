#!/usr/bin/env python3
"""Test infrastructure: (re)makes the fixtures of the option grid (tests/golden/opts/, table: grid.json, read by
tests/fixture_io.py::grid_rows) with THE REFERENCE ITSELF, as oracle/make_golden.py does for the kinds of SETS.

    python oracle/make_grid_golden.py            # check: every committed file equals what the reference prints today
    python oracle/make_grid_golden.py --write    # rewrite them
    python oracle/make_grid_golden.py --only lr_z110,sr_r3 [--write]

Per row of grid.json (n_reads reads of the row's kind from first_read on, the kind's .cmd plus the row's extra options):
  <name>.golden.sam.gz   the SAM body of `gdiet_{lr,sr}_avx -t 4 ...` -- of scalar `gdiet_{lr,sr}` for rows with "build": "scalar" --,
                         SEQ and QUAL printed as "*" (echoes of the input; the full goldens of SETS pin them)
  <name>.trace.gz        the --print-seeds stage trace of the same run, reduced to the lines that start with one of TRACE_PREFIXES,
                         every read's SD lines replaced by their count and sha1 (fixture_io.digest_sd)
  mmi.sha256.json        size and sha256 of the index file `-d` writes, for the rows tagged "mmi"
What keeps a row from passing vacuously is asserted here (and again by tests/test_map_host.py on the committed files): the reference
maps at least the row's min_mapped share of the reads; --for-only / --rev-only rows hold mapped and unmapped reads; leaving out any one of
the row's option groups ("sensitive": every option of "extra") changes the reference's SAM or trace, so no option rides along inert; for a
"scalar" row the two builds of the reference really print different traces; a "score" row holds what fixture_io.assert_score_row_conditions
asks of it (records on both sides of the pre-filter's bound, Ns inside alignments at e2 = 2, a wave / generic tag that is true).
Nothing of the product is involved in what is written."""
import argparse
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from fixture_io import OPTS, SETS, TRACE_PREFIXES, assert_score_row_conditions, digest_sd, grid_cmd, grid_reads, grid_rows, mapped_share, star_seq_qual  # noqa: E402
from make_golden import _gunzip_to, _write_gz  # noqa: E402


def ref_bin(row, build=None):
    return os.path.join(ROOT, "oracle", "_ref", "gdiet_%s%s" % (row["variant"], "_avx" if (build or row["build"]) == "avx" else ""))


def row_inputs(row, tmp):
    """(ref.fa, reads.fq) of a row, unpacked under tmp"""
    d = SETS[row["kind"]][0]
    ref_fa = os.path.join(tmp, os.path.basename(d) + "_ref.fa")
    if not os.path.exists(ref_fa):
        _gunzip_to(os.path.join(d, "ref.fa.gz"), ref_fa)
    fq = os.path.join(tmp, row["name"] + ".fq")
    with open(fq, "w") as f:
        for name, seq, qual in grid_reads(row):
            f.write("@%s\n%s\n+\n%s\n" % (name, seq, qual))
    return ref_fa, fq


def reference_run(row, tmp, build=None, without=None):
    """(SAM body with SEQ / QUAL starred, reduced trace) of the reference on a row; without: an option group of the row left out"""
    ref_fa, fq = row_inputs(row, tmp)
    exe = ref_bin(row, build)
    cmd = grid_cmd(row, without)
    run = subprocess.run([exe] + cmd + ["--print-seeds", ref_fa, fq], capture_output=True, text=True, check=True)
    body = [l for l in run.stdout.split("\n") if l and not l.startswith("@")]
    if without is None:
        par = subprocess.run([exe, "-t", "4"] + cmd + [ref_fa, fq], capture_output=True, text=True, check=True)
        assert [l for l in par.stdout.split("\n") if l and not l.startswith("@")] == body
    lines = digest_sd([l for l in run.stderr.split("\n") if l.startswith(TRACE_PREFIXES)])
    return "".join(star_seq_qual(l) + "\n" for l in body), "".join(l + "\n" for l in lines)


def check_row(row, sam, trace, tmp):
    """the conditions under which a row tests something (see the module text)"""
    lines = sam.rstrip("\n").split("\n")
    mapped, n = mapped_share(lines)
    assert n == row["n_reads"], (row["name"], n)
    assert mapped >= row["min_mapped"] * n, "%s: the reference maps only %d of %d reads" % (row["name"], mapped, n)
    if "strand" in row["tags"]:
        assert 0 < mapped < n, (row["name"], mapped, n)
    assert trace.count("Final shift") == n and trace.count("SDX\t") > 0
    if "score" in row["tags"]:
        assert_score_row_conditions(row, lines)
    for group in row["sensitive"]:  # every option the row names changes what the reference itself prints
        assert reference_run(row, tmp, without=group) != (sam, trace), "%s: the reference prints the same without %s" % (row["name"], group)
    if row["build"] == "scalar":
        other = reference_run(row, tmp, "avx")
        assert other[1] != trace, "%s: both builds of the reference print the same trace" % row["name"]
    return mapped, n


def mmi_digest(row, tmp):
    ref_fa, _ = row_inputs(row, tmp)
    mmi = os.path.join(tmp, row["name"] + ".mmi")
    subprocess.run([ref_bin(row), "-t", "4"] + grid_cmd(row) + ["-d", mmi, ref_fa], capture_output=True, check=True)
    data = open(mmi, "rb").read()
    return dict(size=len(data), sha256=hashlib.sha256(data).hexdigest())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    only = [x for x in a.only.split(",") if x]
    rows = [r for r in grid_rows() if not only or r["name"] in only]
    for r in rows:
        if not os.path.exists(ref_bin(r)):
            sys.exit("oracle/_ref is not built (make -f oracle/Makefile.ref needs the reference's sources)")
    bad = 0

    def put(path, text, gz):
        nonlocal bad
        same = os.path.exists(path) and (gzip.open(path, "rt").read() if gz else open(path).read()) == text
        if not same and a.write:
            _write_gz(path, text) if gz else open(path, "w").write(text)
        bad += not same
        print("%-50s %s" % (os.path.relpath(path, ROOT), "ok" if same else ("WRITTEN" if a.write else "DIFFERS")))

    with tempfile.TemporaryDirectory() as tmp:
        digests = {}
        for row in rows:
            sam, trace = reference_run(row, tmp)
            mapped, n = check_row(row, sam, trace, tmp)
            put(os.path.join(OPTS, row["name"] + ".golden.sam.gz"), sam, True)
            put(os.path.join(OPTS, row["name"] + ".trace.gz"), trace, True)
            print("    %s build, %d of %d reads mapped, %d SAM lines, %d CONQ events" % (row["build"], mapped, n, sam.count("\n"), trace.count("CONQ[")))
            if "mmi" in row["tags"]:
                digests[row["name"]] = mmi_digest(row, tmp)
        if not only:
            put(os.path.join(OPTS, "mmi.sha256.json"), json.dumps(digests, indent=1, sort_keys=True) + "\n", False)
    sys.exit(0 if a.write or not bad else 1)


if __name__ == "__main__":
    main()

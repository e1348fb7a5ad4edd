"""CPU: coverage and depth from BAM records.  The oracle is tests/cov_ref.py, an independent restatement of the section "Coverage" of
include/gdiet_hip.h with a plain depth array.  tests/emul/cov_emul.cpp runs the statements of the kernels (csrc/cov.h) as a stand-alone
program under AddressSanitizer / UBSan on exact-size buffers, with the lanes running 0..63 and 63..0.
  * the emulator equals the restatement, integer for integer -- summary, per-contig counters, windows and the depth of every position --
    on every designed set of tests/cov_inputs.py, at every filter, chunk and window;
  * every kind of bad record is named with its place and reason and contributes nothing;
  * a second, independent oracle ties the rules to the reference's own output: the committed golden SAM text is parsed line by line and
    accumulated one position at a time, and must equal the restatement on the BAM bytes bam_ref makes from the same lines."""
import os
import subprocess

import numpy as np
import pytest

import cov_inputs as ci
import cov_ref as cr
from conftest import ROOT


def build_emul(tmp_path_factory, tag):
    exe = str(tmp_path_factory.mktemp(tag) / "cov_emul")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "genome-on-diet_amd", "csrc"), os.path.join(ROOT, "tests", "emul", "cov_emul.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory, "cov")


def run_emul(emul, data, ref_lens, tmp_path, excl_flags=0x704, min_mapq=0, window=0, chunk=0):
    """the emulator's output as a cov_ref.Cov (bad: (index, reason name) or None)"""
    p = str(tmp_path / "in.recs")
    with open(p, "wb") as f:
        f.write(data)
    r = subprocess.run([emul, p, str(excl_flags), str(min_mapq), str(window), str(chunk), str(len(ref_lens))] + [str(n) for n in ref_lens], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = cr.Cov()
    out.bad, out.contigs, out.depth, out.windows = None, [], [], [] if window else None
    for line in r.stdout.split("\n")[:-1]:
        f = line.split(" ")
        if f[0] == "BAD":
            out.bad = (int(f[1]), cr.REASONS[int(f[2])])
        elif f[0] == "SUMMARY":
            out.summary = dict(zip(cr.SUMMARY, (int(x) for x in f[1:])))
        elif f[0] == "CONTIG":
            out.contigs.append(dict(zip(cr.CONTIG, (int(x) for x in f[2:]))))
        elif f[0] == "WIN":
            v = [int(x) for x in f[3:]]
            assert len(v) == 2 * int(f[2])
            out.windows.append((np.array(v[0::2], np.uint32), np.array(v[1::2], np.uint64)))
        elif f[0] == "DEPTH":
            out.depth.append(np.array([int(x) for x in f[2:]], np.uint32))
    return out


def same(got, want, what=""):
    """two Cov agree in every integer"""
    assert got.summary == want.summary, (what, got.summary, want.summary)
    assert got.contigs == want.contigs, (what, got.contigs, want.contigs)
    assert len(got.depth) == len(want.depth)
    for rid, (a, b) in enumerate(zip(got.depth, want.depth)):
        assert a.dtype == b.dtype == np.uint32 and np.array_equal(a, b), (what, rid, np.nonzero(a != b)[0][:5] if len(a) == len(b) else (len(a), len(b)))
    assert (got.windows is None) == (want.windows is None)
    for rid, (a, b) in enumerate(zip(got.windows or [], want.windows or [])):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (what, "windows", rid)
    assert got.bad == want.bad, (what, got.bad, want.bad)


DESIGNED = ci.designed()


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------
def test_restatement_on_records_read_by_eye():
    """three records whose depth can be written down: 3M at 0 and 20M to the end of a 300-base contig, 1M on the one-base contig"""
    c = cr.coverage(b"".join(ci.edge_set(True)[:2] + ci.edge_set(True)[-1:]), ci.REF_LENS, window=100)
    assert list(c.depth[0][:4]) == [1, 1, 1, 0] and list(c.depth[0][279:]) == [0] + [1] * 20 and list(c.depth[1]) == [1] and not c.depth[2].any()
    assert c.contigs[0] == dict(n_reads=2, cov_bases=23, sum_depth=23, sum_mapq=60, sum_baseq=c.contigs[0]["sum_baseq"], n_baseq=23) and c.contigs[1]["cov_bases"] == 1
    assert [list(x) for x in c.windows[0]] == [[3, 0, 20], [3, 0, 20]] and [len(w[0]) for w in c.windows] == [3, 1, 3, 5, 60]
    assert c.summary == dict(records=3, unmapped=0, secondary=0, supplementary=0, primary_mapped=3, reverse=0, excluded_by_flag=0, excluded_by_mapq=0, counted=3, bad=0)


def test_designed_sets_hold_what_they_are_for():
    assert sorted(len(DESIGNED["count%d" % n]) for n in (0, 1, 3, 4, 5, 63, 64, 65, 257)) == [0, 1, 3, 4, 5, 63, 64, 65, 257]
    for k in (0, 1, 63, 64, 65, 129):
        f, why = cr.parse(DESIGNED["ops%d" % k][0])
        assert why is None and len(f["ops"]) == k and {op for op, _ in f["ops"]} == set(range(min(k, 9)))
    c = cr.coverage(b"".join(DESIGNED["copies"]), ci.REF_LENS)
    assert c.depth[0].max() == 1000 and c.contigs[0]["n_reads"] == 1000
    f, _ = cr.parse(DESIGNED["long_quality_run"][0])
    assert len(f["ops"]) == 129 and f["ops"][-1] == (0, 5000) and f["qual"] is not None
    f, why = cr.parse(DESIGNED["placeholder"][0])
    assert why is None and [op for op, _ in f["ops"]] == [4, 0, 1, 2, 7, 3, 8, 4]
    assert cr.parse(DESIGNED["placeholder"][2])[0]["ops"] == [(4, 30), (2, 40)]
    # every chunk border of 7 and 256 slots, on every contig, lies inside a run of the border set
    d = np.concatenate(cr.coverage(b"".join(DESIGNED["borders"]), ci.REF_LENS).depth)
    assert all(d[k - 1] > 0 and d[k] > 0 for c in (7, 256) for k in range(c, len(d), c))


# ---- the emulator against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DESIGNED))
def test_emulator_equals_restatement(name, emul, tmp_path):
    data = b"".join(DESIGNED[name])
    want = cr.coverage(data, ci.REF_LENS, window=64)
    assert want.bad is None and (want.summary["counted"] > 0 or name == "count0")
    same(run_emul(emul, data, ci.REF_LENS, tmp_path, window=64, chunk=7), want, name)


@pytest.mark.parametrize("excl,mapq", ci.FILTERS)
def test_filters(excl, mapq, emul, tmp_path):
    data = b"".join(ci.filter_set())
    want = cr.coverage(data, ci.REF_LENS, excl_flags=excl, min_mapq=mapq)
    same(run_emul(emul, data, ci.REF_LENS, tmp_path, excl_flags=excl, min_mapq=mapq), want, (excl, mapq))
    s = want.summary
    assert s["records"] == 20 and s["bad"] == 0
    assert (s["unmapped"], s["secondary"], s["supplementary"], s["primary_mapped"], s["reverse"]) == (4, 5, 3, 10, 3)  # of the set's list of flags, whatever the filter


def test_filter_counters_by_hand():
    """the default filter on the filter set, counted by eye from its list of (flag, mapq)"""
    s = cr.coverage(b"".join(ci.filter_set()), ci.REF_LENS).summary
    assert (s["excluded_by_flag"], s["excluded_by_mapq"], s["counted"]) == (10, 0, 9)  # 4, 4|16, 0x100 x2, 0x900, 0x200, 0x400 x2, 4|0x100, unmapped; unplaced_passing is none
    s = cr.coverage(b"".join(ci.filter_set()), ci.REF_LENS, excl_flags=0, min_mapq=61).summary
    assert (s["excluded_by_flag"], s["excluded_by_mapq"], s["counted"]) == (0, 17, 2)  # 61 and 255 are counted, 70 passes but is unplaced


@pytest.mark.parametrize("window", ci.WINDOWS)
def test_chunks_and_windows(window, emul, tmp_path):
    data = b"".join(ci.border_set())
    want = cr.coverage(data, ci.REF_LENS, window=window)
    for chunk in ci.CHUNKS if window in (1, 64) else (7,):
        same(run_emul(emul, data, ci.REF_LENS, tmp_path, window=window, chunk=chunk), want, (window, chunk))


@pytest.mark.parametrize("name", sorted(ci.BAD))
def test_bad_records(name, emul, tmp_path):
    """named with its place and reason, counted in `bad`, and nothing else: the other counters and arrays are those of the set without it"""
    recs = ci.with_bad(name)
    want = cr.coverage(b"".join(recs), ci.REF_LENS, window=64)
    assert want.bad == (3, ci.BAD[name][1]) and want.summary["bad"] == 1
    same(run_emul(emul, b"".join(recs), ci.REF_LENS, tmp_path, window=64), want, name)
    clean = cr.coverage(b"".join(recs[:3] + recs[4:]), ci.REF_LENS, window=64)
    assert want.contigs == clean.contigs and all(np.array_equal(a, b) for a, b in zip(want.depth, clean.depth)) and want.summary["counted"] == clean.summary["counted"]


def test_order_freedom(emul, tmp_path):
    recs = DESIGNED["borders"] + DESIGNED["quality"] + DESIGNED["placeholder"]
    want = cr.coverage(b"".join(recs), ci.REF_LENS, window=65)
    shuffled = list(recs)
    np.random.default_rng(3).shuffle(shuffled)
    same(run_emul(emul, b"".join(shuffled), ci.REF_LENS, tmp_path, window=65, chunk=256), want)


# ---- the second oracle: the reference's own SAM text ---------------------------------------------------------------------------------------
HOLDS = {"hifi_sv": "D rev supp sec deep", "ont_sv": "D rev supp sec deep", "sr": "D rev deep", "hifi_edge": "D rev sec"}


@pytest.mark.parametrize("kind", ci.GOLDEN)
def test_golden_sam_text_by_brute_force(kind, emul, tmp_path):
    """FLAG, RNAME, POS, MAPQ, CIGAR and QUAL of every golden line, accumulated one base at a time, equal the restatement on the BAM bytes of
    the same lines (and the emulator equals both).  What the sets hold is asserted: deletions and reverse strands in all four;
    supplementary records in hifi_sv and ont_sv only, secondary records in all but sr, and overlapping reads (depth > 1) in all but
    hifi_edge, whose six mapped reads lie apart.  What a set lacks the designed records cover: the filter set holds secondary and
    supplementary records on both strands, `copies` and `strands` overlapping reads (test_emulator_equals_restatement, test_filters)."""
    recs, names, lens, lines = ci.golden_records(kind)
    data = b"".join(recs)
    for excl, mapq in ((0x704, 0), (0x900, 0), (0, 20)):
        want = cr.coverage(data, lens, excl_flags=excl, min_mapq=mapq)
        depth, contigs, counted = cr.sam_depth(lines, names, lens, excl_flags=excl, min_mapq=mapq)
        assert want.bad is None and want.summary["counted"] == counted > 0 and want.contigs == contigs
        assert all(np.array_equal(a, b) for a, b in zip(want.depth, depth))
    want = cr.coverage(data, lens, window=1000)
    same(run_emul(emul, data, lens, tmp_path, window=1000, chunk=65536), want, kind)
    flags = [int(l.split("\t")[1]) for l in lines]
    holds = dict(D=any("D" in l.split("\t")[5] for l in lines), rev=any(f & 16 and not f & 4 for f in flags), supp=any(f & 0x800 for f in flags), sec=any(f & 0x100 for f in flags),
                 deep=max(int(d.max()) for d in want.depth) > 1)
    assert " ".join(k for k in ("D", "rev", "supp", "sec", "deep") if holds[k]) == HOLDS[kind]


def test_text_files_from_integers():
    """the layout of the two files, on numbers that can be checked by eye"""
    c = cr.coverage(b"".join(ci.edge_set(True)[:2]), ci.REF_LENS, window=100)
    tsv = cr.coverage_tsv(c, ci.REFS, ci.REF_LENS).split("\n")
    assert tsv[0] == "#rname\tstartpos\tendpos\tnumreads\tcovbases\tcoverage\tmeandepth\tmeanbaseq\tmeanmapq"
    assert tsv[1].split("\t")[:7] == ["c0", "1", "300", "2", "23", "7.66667", "0.0766667"] and tsv[1].split("\t")[8] == "30" and tsv[2] == "one\t1\t1\t0\t0\t0\t0\t0\t0"
    assert tsv[6].startswith("#summary\trecords=2\tunmapped=0") and tsv[7] == ""
    bed = cr.regions_bed(c, ci.REFS, ci.REF_LENS, 100).split("\n")
    assert bed[:4] == ["c0\t0\t100\t0.03", "c0\t100\t200\t0.00", "c0\t200\t300\t0.20", "one\t0\t1\t0.00"]

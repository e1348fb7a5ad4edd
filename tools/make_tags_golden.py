#!/usr/bin/env python3
"""Test infrastructure: (re)makes the fixtures of the per-base difference tags (tests/golden/tags/) with THE REFERENCE ITSELF, in
the style of oracle/make_golden.py and oracle/make_grid_golden.py.

    python tools/make_tags_golden.py            # check: every committed file equals what the reference prints today
    python tools/make_tags_golden.py --write    # rewrite them

SAM, per kind of SAM_KINDS and mode (md: --MD, cs: --cs, cs_long: --cs=long), `gdiet_{lr,sr}_avx -t 4 <kind's .cmd> <mode>`:
  <kind>.<mode>.tsv.gz      one line per SAM record in output order: qname, flag, rname, pos, the tag's text without its "cs:Z:" /
                            "MD:Z:" prefix (nothing for a record without an alignment).  For cs_long of the long-read kinds the text is
                            stored as "#<length>:<sha1>" (fixture_io.SD_DIGESTED does the same for seed hits): spelled out it is 350-440 KB
                            per kind.
PAF, under fixture_io.paf_cmd_of (`-c --paf-no-hit`):
  <kind>.paf.<name>.tsv.gz  one line per PAF line: qname, query start, strand, tag text; hifi_sv with --cs, --qstrand --cs and
                            --qstrand --MD, sr with --cs.  Under --qstrand the tag of a reverse-strand line is nearly all mismatches
                            (the reference pairs the read with the mirrored target interval: LR/index.c:168-181), 3-5 KB each: those
                            90 tags are stored as "#<length>:<sha1>" as well.
What is asserted on the way (and again on the committed files by tests/test_diffstr.py where it can be): with the tag field removed,
every line is the committed golden SAM / PAF line of the kind -- the tag is a pure insertion, behind SA:Z: and in front of rl:i:0 in
SAM, at the end of the line in PAF; every record with an alignment has a tag (TAGGED counts); --MD --cs prints what --MD prints;
--qstrand changes the tag of every reverse-strand line of hifi_sv and of no other; every kind holds records on the reverse strand,
with a deletion, with an insertion and with an N on either side, as far as its read set has them (COVER).
Nothing of the product is involved in what is written."""
import argparse
import gzip
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from fixture_io import SETS, cmd_of, golden_paf, golden_sam, paf_cmd_of, reads_of, variant_of  # noqa: E402
from make_golden import REF, _gunzip_to, _write_gz  # noqa: E402

TAGS = os.path.join(ROOT, "tests", "golden", "tags")
SAM_KINDS = ("hifi_sv", "ont_sv", "hifi_edge", "sr", "sr_edge")
MODES = {"md": ["--MD"], "cs": ["--cs"], "cs_long": ["--cs=long"]}
DIGESTED = {("hifi_sv", "cs_long"), ("ont_sv", "cs_long"), ("hifi_edge", "cs_long")}
PAF_ROWS = (("hifi_sv", "cs", ["--cs"]), ("hifi_sv", "qstrand_cs", ["--qstrand", "--cs"]), ("hifi_sv", "qstrand_md", ["--qstrand", "--MD"]),
            ("sr", "cs", ["--cs"]))
TAGGED = {"hifi_sv": (187, 193), "ont_sv": (65, 71), "sr": (1693, 2000), "hifi_edge": (7, 17), "sr_edge": (13, 20)}  # (tagged, lines)
# what every kind must hold at least one record of (what the read sets give: hifi_edge has a single reverse record and no insertion;
# of the reverse-strand reads over the reference's N run only ont_sv_3's final record still covers it)
COVER = {"hifi_sv": ("rev", "deletion", "insertion", "with_N"), "ont_sv": ("rev", "deletion", "insertion", "with_N", "rev_with_N"),
         "hifi_edge": ("rev", "deletion", "with_N"), "sr": ("rev", "deletion", "insertion", "with_N", "rev_with_N"),
         "sr_edge": ("rev", "deletion", "insertion", "with_N", "rev_with_N")}


def digest(text):
    return "#%d:%s" % (len(text), hashlib.sha1(text.encode()).hexdigest())


def split_tag(line):
    """(line without its cs:Z: / MD:Z: field, the field's text or "")"""
    f = line.split("\t")
    hit = [i for i, x in enumerate(f) if x.startswith(("cs:Z:", "MD:Z:"))]
    assert len(hit) <= 1, line[:200]
    if not hit:
        return line, ""
    return "\t".join(f[:hit[0]] + f[hit[0] + 1:]), f[hit[0]][5:]


def inputs(kind, tmp):
    d = SETS[kind][0]
    ref_fa = os.path.join(tmp, os.path.basename(d) + "_ref.fa")
    if not os.path.exists(ref_fa):
        _gunzip_to(os.path.join(d, "ref.fa.gz"), ref_fa)
    fq = os.path.join(tmp, kind + ".fq")
    if not os.path.exists(fq):
        with open(fq, "w") as f:
            for name, seq, qual in reads_of(kind):
                f.write("@%s\n%s\n+\n%s\n" % (name, seq, qual))
    return ref_fa, fq


def run(kind, cmd, tmp):
    ref_fa, fq = inputs(kind, tmp)
    out = subprocess.run([REF[variant_of(kind)], "-t", "4"] + cmd + [ref_fa, fq], capture_output=True, text=True, check=True).stdout
    return [l for l in out.split("\n") if l and not l.startswith("@")]


def sam_rows(kind, mode, tmp):
    """[(qname, flag, rname, pos, tag text)] of the reference's SAM under the mode, after the checks of the module text"""
    lines = run(kind, cmd_of(kind) + MODES[mode], tmp)
    plain = golden_sam(kind)
    assert len(lines) == len(plain), (kind, mode, len(lines), len(plain))
    rows = []
    for l, g in zip(lines, plain):
        bare, tag = split_tag(l)
        assert bare == g, (kind, mode, l.split("\t")[0])
        f = l.split("\t")
        if tag:  # behind SA:Z: (if any), in front of rl:i:0
            i = next(i for i, x in enumerate(f) if x.startswith(("cs:Z:", "MD:Z:")))
            assert f[i + 1] == "rl:i:0" and f[i][:2] == ("MD" if mode == "md" else "cs"), (kind, mode, f[0])
        assert bool(tag) == (f[5] != "*"), (kind, mode, f[0])
        rows.append((f[0], f[1], f[2], f[3], tag))
    assert (sum(1 for r in rows if r[4]), len(rows)) == TAGGED[kind], (kind, mode, sum(1 for r in rows if r[4]), len(rows))
    return rows


def check_cover(kind, rows_by_mode):
    cs, plain = rows_by_mode["cs"], golden_sam(kind)
    rev = sum(1 for r in cs if r[4] and int(r[1]) & 16)
    dele = sum(1 for r in cs if "-" in r[4])
    ins = sum(1 for r in cs if "+" in r[4])
    n_any = sum(1 for r in cs if "n" in r[4])
    n_rev = sum(1 for r in cs if "n" in r[4] and int(r[1]) & 16)
    assert len(plain) == len(cs)
    got = dict(rev=rev, deletion=dele, insertion=ins, with_N=n_any, rev_with_N=n_rev)
    for what in COVER[kind]:
        assert got[what] > 0, (kind, what)
    return got


def paf_rows(kind, extra, tmp):
    lines = run(kind, paf_cmd_of(kind) + extra, tmp)
    plain = golden_paf(kind)
    assert len(lines) == len(plain), (kind, extra)
    rows = []
    for l, g in zip(lines, plain):
        bare, tag = split_tag(l)
        f, fg = bare.split("\t"), g.split("\t")
        if "--qstrand" in extra and f[4] == "-":  # mm_write_paf3 prints the target interval on the read's strand (LR/format.c:340-341)
            tl = int(f[6])
            assert (tl - int(f[8]), tl - int(f[7])) == (int(fg[7]), int(fg[8])), (kind, f[0])
            f[7], f[8] = fg[7], fg[8]
        assert f == fg, (kind, extra, f[0])
        assert bool(tag) == (f[4] != "*") and (not tag or l.split("\t")[-1][5:] == tag), (kind, extra, f[0])  # the last field, behind cg:Z:
        rows.append((f[0], f[2], f[4], tag))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    for b in REF.values():
        if not os.path.exists(b):
            sys.exit("oracle/_ref is not built (make -f oracle/Makefile.ref needs the reference's sources)")
    os.makedirs(TAGS, exist_ok=True)
    bad = 0

    def put(name, rows, dig=False):
        nonlocal bad
        text = "".join("\t".join(r[:-1] + ((digest(r[-1]) if dig and r[-1] else r[-1]),)) + "\n" for r in rows)
        path = os.path.join(TAGS, name)
        same = os.path.exists(path) and gzip.open(path, "rt").read() == text
        if not same and a.write:
            _write_gz(path, text)
        bad += not same
        print("%-44s %s" % (os.path.relpath(path, ROOT), "ok" if same else ("WRITTEN" if a.write else "DIFFERS")))

    with tempfile.TemporaryDirectory() as tmp:
        for kind in SAM_KINDS:
            by_mode = {mode: sam_rows(kind, mode, tmp) for mode in MODES}
            both = run(kind, cmd_of(kind) + ["--MD", "--cs"], tmp)
            assert both == run(kind, cmd_of(kind) + ["--MD"], tmp), kind  # the two flags together mean MD
            print("    %s: %s" % (kind, check_cover(kind, by_mode)))
            for mode, rows in by_mode.items():
                put("%s.%s.tsv.gz" % (kind, mode), rows, (kind, mode) in DIGESTED)
        paf = {(kind, name): paf_rows(kind, extra, tmp) for kind, name, extra in PAF_ROWS}
        for (kind, name), rows in paf.items():
            if name.startswith("qstrand"):
                rows = [r[:3] + ((digest(r[3]) if r[2] == "-" else r[3]),) for r in rows]
            put("%s.paf.%s.tsv.gz" % (kind, name), rows)
        plain_cs, q_cs = paf[("hifi_sv", "cs")], paf[("hifi_sv", "qstrand_cs")]
        n_rev = 0
        for p, q in zip(plain_cs, q_cs):  # --qstrand changes the tag of every reverse-strand line and of no other
            assert (p[3] != q[3]) == (p[2] == "-"), p[0]
            n_rev += p[2] == "-"
        assert n_rev == 90, n_rev
    sys.exit(0 if a.write or not bad else 1)


if __name__ == "__main__":
    main()

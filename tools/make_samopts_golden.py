#!/usr/bin/env python3
"""Test infrastructure: (re)makes the fixtures of the SAM / PAF output options (tests/golden/samopts/) with THE REFERENCE ITSELF, in the
style of tools/make_tags_golden.py.

    python tools/make_samopts_golden.py            # check: every committed file equals what the reference prints today
    python tools/make_samopts_golden.py --write    # rewrite them

Per kind of samopts_io.KINDS and mode of samopts_io.MODES (Y: -Y, hit: --sam-hit-only, Q: -Q, y: -y, R: -R <line>, all: -Y -y -R <line>
--sam-hit-only), `gdiet_{lr,sr}_avx -t 4 <kind's .cmd> <mode> ref.fa reads.fq`, run inside a temporary directory so that the CL: field
of @PG holds no path.  reads.fq is written here from the committed read set, with samopts_io.comment_of's comment on two reads of
every three.  Files: see tests/samopts_io.py.
What is asserted on the way, against the committed plain goldens (EXPECT holds the counts):
  -Y              changes the CIGAR column of every supplementary record (H -> S) and SEQ / QUAL of every supplementary and every
                  secondary record (the whole read), and nothing else;
  --sam-hit-only  drops the unmapped lines and changes no other;
  -Q              makes QUAL "*" and changes nothing else;
  -y              appends the read's comment as the last field of every line of a read that has one, unmapped lines included;
  -R              puts RG:Z:<id> in front of the first tag of every line, and one @RG line into the header;
  -L              changes nothing: no CIGAR of these sets comes near 65 534 operations;
  every mode      the values of NM:i: and de:f: are the plain golden's on every line; the header is the @SQ lines of the reference FASTA,
                  the @RG line where -R is given, and @PG with VN: and CL:;
  PAF, -y         appends the comment to mapped lines only, not to the lines of --paf-no-hit.
One value is not the run's own: ms:i: of a reverse-strand record over reference Ns is an out-of-bounds read in the reference (DESIGN.md §5,
item 2; tests/test_map_host.py:_norm_ms) and can change from run to run, so on those records (a few per long-read set) the value of the
committed plain golden, another run of the same binary, is written and compared.
Nothing of the product is involved in what is written."""
import argparse
import gzip
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from fixture_io import SETS, cmd_of, golden_paf, golden_sam, read_fasta, variant_of  # noqa: E402
from make_golden import REF, _gunzip_to, _write_gz  # noqa: E402
import samopts_io as so  # noqa: E402

# kind: (lines, unmapped lines, supplementary records, secondary records) of the plain golden
EXPECT = {"hifi_sv": (193, 6, 39, 4), "ont_sv": (71, 6, 9, 2), "sr": (2000, 307, 0, 0)}
MAX_BYTES = 200 * 1000


def tag_value(fields, tag):
    hit = [x[len(tag):] for x in fields[11:] if x.startswith(tag)]
    assert len(hit) <= 1
    return hit[0] if hit else None


def pin_ms(line, plain_line, rev):
    """line with the plain golden's ms:i: value if the record is one whose ms:i: the reference reads out of bounds (see the module text)"""
    f = line.split("\t")
    if not rev or "nn:i:0" in f or not any(x.startswith("nn:i:") for x in f):
        return line
    ms = [x for x in plain_line.split("\t") if x.startswith("ms:i:")]
    assert len(ms) == 1
    return "\t".join(ms[0] if x.startswith("ms:i:") else x for x in f)


def run(kind, mode, tmp, extra=None):
    """the reference's standard output, as lines, for the mode (or for cmd_of + extra)"""
    d = os.path.join(tmp, kind)
    if not os.path.isdir(d):
        os.makedirs(d)
        _gunzip_to(os.path.join(SETS[kind][0], "ref.fa.gz"), os.path.join(d, "ref.fa"))
        with open(os.path.join(d, "reads.fq"), "w") as f:
            for name, seq, qual, cm in so.reads_with_comments(kind):
                f.write("@%s%s\n%s\n+\n%s\n" % (name, "" if cm is None else " " + cm, seq, qual))
    argv = so.ref_argv(kind, mode) if extra is None else ["minimap2"] + so.THREADS + cmd_of(kind) + extra + ["ref.fa", "reads.fq"]
    out = subprocess.run([REF[variant_of(kind)]] + argv[1:], cwd=d, capture_output=True, text=True, check=True).stdout
    assert out.endswith("\n")
    return out.split("\n")[:-1]


def check_header(kind, mode, hdr):
    names, seqs = read_fasta(os.path.join(SETS[kind][0], "ref.fa.gz"))
    want = ["@SQ\tSN:%s\tLN:%d" % (n, len(s)) for n, s in zip(names, seqs)]
    if mode in so.MODE_RG:
        want.append(so.RG_LINE)
    want.append("@PG\tID:minimap2\tPN:minimap2\tVN:%s\tCL:%s" % (so.VERSION, " ".join(so.ref_argv(kind, mode))))
    assert hdr == want, (kind, mode, hdr[-2:], want[-2:])


def check_mode(kind, mode, body):
    plain = golden_sam(kind)
    n_lines, n_unmapped, n_supp, n_sec = EXPECT[kind]
    assert len(plain) == n_lines
    comment = {r[0]: r[3] for r in so.reads_with_comments(kind)}
    assert len(comment) == len(so.reads_with_comments(kind))  # (names are unique: a line finds its read by QNAME)
    if mode in ("hit", "all"):
        kept = [g for g in plain if not int(g.split("\t")[1]) & 4]
        assert len(plain) - len(kept) == n_unmapped, (kind, mode)
        plain = kept
    assert len(body) == len(plain), (kind, mode, len(body), len(plain))
    changed = cigar_changed = seq_changed = 0
    for l, g in zip(body, plain):
        f, fg = l.split("\t"), g.split("\t")
        flag = int(fg[1])
        assert f[:5] == fg[:5] and f[6:9] == fg[6:9], (kind, mode, f[0])
        assert tag_value(f, "NM:i:") == tag_value(fg, "NM:i:") and tag_value(f, "de:f:") == tag_value(fg, "de:f:"), (kind, mode, f[0])
        want = list(fg)
        if mode in ("Y", "all"):
            read = next(r for r in so.reads_with_comments(kind) if r[0] == f[0]) if flag & 0x900 else None
            if flag & 0x800:
                want[5] = fg[5].replace("H", "S")
                assert want[5] != fg[5], (kind, f[0])  # every supplementary record is clipped
            if flag & 0x900:  # the whole read, on the record's strand; SEQ / QUAL of the primary line of the same strand show it
                assert len(f[9]) == len(read[1]) == len(f[10]) and f[9] != fg[9], (kind, f[0])
                want[9], want[10] = f[9], f[10]
                seq_changed += 1
        if mode == "Q":
            assert fg[10] != "*" or flag & 0x100  # (a secondary record has neither SEQ nor QUAL)
            want[10] = "*"
        if mode in ("R", "all"):
            want.insert(11, "RG:Z:" + so.RG_ID)
        if mode in ("y", "all") and comment[f[0]] is not None:
            want += comment[f[0]].split("\t")
        assert f == want, (kind, mode, f[0])
        changed += l != g
        cigar_changed += f[5] != fg[5]
    if mode == "Y":
        assert (changed, cigar_changed, seq_changed) == (n_supp + n_sec, n_supp, n_supp + n_sec), (kind, changed, cigar_changed, seq_changed)
        assert sum(1 for g in plain if int(g.split("\t")[1]) & 0x800) == n_supp and sum(1 for g in plain if int(g.split("\t")[1]) & 0x100) == n_sec
    if mode == "hit":
        assert changed == 0
    if mode == "y":
        assert changed == sum(1 for g in plain if comment[g.split("\t")[0]] is not None) > 0
        assert any(int(g.split("\t")[1]) & 4 and comment[g.split("\t")[0]] is not None for g in plain), kind  # an unmapped line with a comment


def check_whole_read_under_Y(kind, body):
    """under -Y the SEQ / QUAL of a 0x100 / 0x800 record are those of the read's primary line when the strands agree"""
    pri = {}
    for l in body:
        f = l.split("\t")
        if not int(f[1]) & 0x904:
            pri[f[0]] = f
    n = 0
    for l in body:
        f = l.split("\t")
        if int(f[1]) & 0x900 and (int(f[1]) & 16) == (int(pri[f[0]][1]) & 16):
            assert f[9:11] == pri[f[0]][9:11], (kind, f[0])
            n += 1
    return n


def check_paf_y(kind, lines):
    plain = golden_paf(kind)
    comment = {r[0]: r[3] for r in so.reads_with_comments(kind)}
    assert len(lines) == len(plain), kind
    n_mapped = n_nohit = 0
    for l, g in zip(lines, plain):
        name, mapped = g.split("\t")[0], g.split("\t")[4] != "*"
        assert l == (g + "\t" + comment[name] if mapped and comment[name] is not None else g), (kind, name)
        n_mapped += mapped and comment[name] is not None
        n_nohit += (not mapped) and comment[name] is not None
    assert n_mapped > 0 and n_nohit > 0, (kind, n_mapped, n_nohit)  # both rules are exercised


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    for b in REF.values():
        if not os.path.exists(b):
            sys.exit("oracle/_ref is not built (make -f oracle/Makefile.ref needs the reference's sources)")
    os.makedirs(so.SAMOPTS, exist_ok=True)
    bad = 0

    def put(name, lines):
        nonlocal bad
        text = "".join(l + "\n" for l in lines)
        path = os.path.join(so.SAMOPTS, name)
        same = os.path.exists(path) and gzip.open(path, "rt").read() == text
        if not same and a.write:
            _write_gz(path, text)
            assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
        bad += not same
        print("%-44s %s" % (os.path.relpath(path, ROOT), "ok" if same else ("WRITTEN" if a.write else "DIFFERS")))

    with tempfile.TemporaryDirectory() as tmp:
        for kind in so.KINDS:
            for extra in ([], ["-L"]):  # comments in the FASTQ change nothing without -y; -L changes nothing
                lines = [l for l in run(kind, None, tmp, extra=extra) if not l.startswith("@")]
                assert len(lines) == len(golden_sam(kind)), (kind, extra)
                assert [pin_ms(l, g, int(g.split("\t")[1]) & 16) for l, g in zip(lines, golden_sam(kind))] == golden_sam(kind), (kind, extra)
            for mode in so.MODES:
                out = run(kind, mode, tmp)
                n_hdr = next(i for i, l in enumerate(out) if not l.startswith("@"))
                hdr, body = out[:n_hdr], out[n_hdr:]
                kept = [g for g in golden_sam(kind) if not (mode in ("hit", "all") and int(g.split("\t")[1]) & 4)]
                assert len(kept) == len(body), (kind, mode)
                body = [pin_ms(l, g, int(g.split("\t")[1]) & 16) for l, g in zip(body, kept)]
                out = hdr + body
                check_header(kind, mode, hdr)
                check_mode(kind, mode, body)
                if mode == "Y":
                    print("    %s: -Y: %d clipped records carry their primary line's SEQ / QUAL" % (kind, check_whole_read_under_Y(kind, body)))
                put("%s.%s.sam.gz" % (kind, mode), [so.digest_line(l) for l in out])
        for kind in so.PAF_KINDS:
            lines = run(kind, "paf_y", tmp)
            assert len(lines) == len(golden_paf(kind)), kind
            lines = [pin_ms(l, g, g.split("\t")[4] == "-") for l, g in zip(lines, golden_paf(kind))]
            check_paf_y(kind, lines)
            put("%s.paf_y.paf.gz" % kind, lines)
    sys.exit(0 if a.write or not bad else 1)


if __name__ == "__main__":
    main()

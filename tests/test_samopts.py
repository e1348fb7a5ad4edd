"""CPU: the SAM / PAF output options -Y, -L, -Q, -y, -R and --sam-hit-only of the record writers (map_host.h: gd_write_sam, gd_write_paf,
gd_parse_rg_line, gd_sam_header), as a stand-alone program under AddressSanitizer and UBSan (tests/emul/samopts_emul.cpp).
  * tools/make_samopts_golden.py in check mode: the committed fixtures (tests/golden/samopts/) are what the reference prints;
  * the records are rebuilt from the committed PLAIN golden lines (records_of below) and printed again: with no option the program
    prints the plain golden, with each mode of samopts_io.MODES the reference's output under that mode, header included;
  * -L on hand-built records around the 65 535-operation limit;
  * the read-group parser: refusals, escapes, the 255-byte limit of the id."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from fixture_io import SETS, golden_paf, golden_sam, read_fasta, reads_of
import samopts_io as so

F_OUT_MD, F_OUT_CG, F_PAF_NO_HIT = 0x1000000, 0x20, 0x8000000
# Records whose NM:i: / de:f: values cannot be rebuilt from their own line: primaries made by concatenate_cigars keep the blen of their
# first part, so blen is not the sum of the CIGAR's M/I/D, and the line shows only blen - mlen.  (records, of how many with a CIGAR)
STALE = {"hifi_sv": (74, 187), "ont_sv": (21, 65), "sr": (2, 1693)}
_CG = re.compile(r"(\d+)([MIDNSHP=XB])")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("samopts") / "samopts_emul")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "genome-on-diet_amd", "csrc"), os.path.join(ROOT, "tests", "emul", "samopts_emul.cpp"), "-o", exe])
    return exe


def run_emul(emul, what, text, tmp_path, status=0):
    path = os.path.join(str(tmp_path), "in.txt")
    with open(path, "w") as f:
        f.write(text)
    r = subprocess.run([emul, what, path], capture_output=True, text=True)
    assert r.returncode == status, (r.returncode, r.stderr[-2000:])
    return r.stdout


def test_samopts_goldens_are_what_the_reference_prints():
    """tools/make_samopts_golden.py in check mode (skipped where the reference's sources, hence oracle/_ref, do not exist)"""
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "gdiet_sr_avx")):
        pytest.skip("oracle/_ref not built (no reference sources on this machine)")
    r = subprocess.run(["python3", os.path.join(ROOT, "tools", "make_samopts_golden.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" ok\n") == len(so.KINDS) * len(so.MODES) + len(so.PAF_KINDS), r.stdout


# ---- records out of the plain golden ---------------------------------------------------------------------------------------------
def records_of(kind):
    """[(qname, seq, qual, comment, [REG field strings])] rebuilt from the plain golden SAM of the kind:
         qs / qe / rev        clips and FLAG 0x10           re       rs + lengths of M/D/N
         has_p                CIGAR != *                    parent   != id on 0x100 records
         sam_pri              mapped, neither 0x100 nor 0x800
         cnt / score / subsc / dp_max / dp_score / n_ambi   cm / s1 / s2 / ms / AS / nn
         blen                 sum of M/I/D                  mlen     blen + nn - NM"""
    names, _ = read_fasta(os.path.join(SETS[kind][0], "ref.fa.gz"))
    rid_of = {n: i for i, n in enumerate(names)}
    by_read = {}
    for l in golden_sam(kind):
        by_read.setdefault(l.split("\t")[0], []).append(l.split("\t"))
    out = []
    for qname, seq, qual, cm in so.reads_with_comments(kind):
        regs = []
        for j, f in enumerate(by_read[qname]):
            flag = int(f[1])
            if flag & 4:
                assert len(by_read[qname]) == 1
                break
            tag = {x[:5]: x[5:] for x in f[11:]}
            cg = [(int(n), op) for n, op in _CG.findall(f[5])]
            assert "".join("%d%s" % x for x in cg) == f[5] and f[5] != "*"
            clip0 = cg[0][0] if cg[0][1] in "SH" else 0
            clip1 = cg[-1][0] if cg[-1][1] in "SH" else 0
            core = [x for x in cg if x[1] not in "SH"]
            rev = 1 if flag & 16 else 0
            qs, qe = (clip1, len(seq) - clip0) if rev else (clip0, len(seq) - clip1)
            rs = int(f[3]) - 1
            re_ = rs + sum(n for n, op in core if op in "MDN=X")
            blen = sum(n for n, op in core if op in "MID=X")
            nn = int(tag["nn:i:"])
            mlen = blen + nn - int(tag["NM:i:"])
            parent = j if not flag & 0x100 else (j + 1 if j == 0 else 0)
            assert ("s2:i:" in tag) == (parent == j) and tag["tp:A:"] == ("P" if parent == j else "S")
            nums = [j, int(tag["cm:i:"]), rid_of[f[2]], int(tag["s1:i:"]), qs, qe, rs, re_, parent, int(tag.get("s2:i:", 0)), mlen, blen, int(f[4]), rev,
                    0 if flag & 0x900 else 1, int(tag["AS:i:"]), int(tag["ms:i:"]), nn, 1]
            regs.append("REG\t%s\t%s\t-" % (" ".join(str(x) for x in nums), "".join("%d%s" % x for x in core)))
        out.append((qname, seq, qual, cm, regs))
    return out


def dump(kind, mode, flag, rg=None, hdr=None, with_qual=True):
    names, seqs = read_fasta(os.path.join(SETS[kind][0], "ref.fa.gz"))
    t = ["MODE\t" + mode, "FLAG\t%d" % flag]
    if rg is not None:
        t.append("RG\t" + rg)
    if hdr is not None:
        t.append("HDR\t" + "\t".join(hdr))
    t += ["SQ\t%s\t%d" % (n, len(s)) for n, s in zip(names, seqs)]
    for qname, seq, qual, cm, regs in _records(kind):
        t.append("READ\t%s\t%s\t%s" % (qname, seq, qual if with_qual else "*"))
        if cm is not None:
            t.append("COMMENT\t" + cm)
        t += regs
    return "\n".join(t) + "\n"


_rec = {}


def _records(kind):
    if kind not in _rec:
        _rec[kind] = records_of(kind)
    return _rec[kind]


def mask_nm_de(line):
    return "\t".join("NM:i:?" if x.startswith("NM:i:") else "de:f:?" if x.startswith("de:f:") else x for x in line.split("\t"))


_stale = {}


def stale_keys(kind, emul, tmp_path):
    """(qname, FLAG, POS) of the records whose NM / de values the plain line does not determine, found by the self-check: with no option
    the program prints the plain golden line, but for these, and for these only in the values of NM:i: and de:f:"""
    if kind not in _stale:
        got = run_emul(emul, "fmt", dump(kind, "sam", 0), tmp_path).split("\n")[:-1]
        want = golden_sam(kind)
        assert len(got) == len(want)
        keys = set()
        for g, w in zip(got, want):
            if g != w:
                assert mask_nm_de(g) == mask_nm_de(w), w.split("\t")[:4]
                assert not int(w.split("\t")[1]) & 0x900, w.split("\t")[:4]  # the records -Y changes are exact
                f = w.split("\t")
                keys.add((f[0], f[1], f[3]))
        _stale[kind] = keys
    return _stale[kind]


def same_lines(kind, got, want, stale):
    assert len(got) == len(want), (kind, len(got), len(want))
    for g, w in zip(got, want):
        f = w.split("\t")
        if (f[0], f[1], f[3]) in stale:
            g, w = mask_nm_de(g), mask_nm_de(w)
        assert g == w, (kind, f[:4])


@pytest.mark.parametrize("kind", so.KINDS)
def test_no_option_prints_the_plain_golden(kind, emul, tmp_path):
    """the self-check of the rebuilt records, with the counts of STALE; the flag-off path of the writers is the committed plain golden"""
    stale = stale_keys(kind, emul, tmp_path)
    n_cigar = sum(1 for l in golden_sam(kind) if l.split("\t")[5] != "*")
    assert (len(stale), n_cigar) == STALE[kind]
    # PAF, mapped and unmapped lines (the PAF goldens exist for two kinds)
    if kind in so.PAF_KINDS:
        got = run_emul(emul, "fmt", dump(kind, "paf", F_OUT_CG | F_PAF_NO_HIT), tmp_path).split("\n")[:-1]
        want = golden_paf(kind)
        assert len(got) == len(want)
        n_masked = 0
        for g, w in zip(got, want):
            if g != w:  # the same records: PAF prints mlen and blen themselves (columns 10 and 11) next to NM and de
                fg, fw = mask_nm_de(g).split("\t"), mask_nm_de(w).split("\t")
                assert fg[:9] + fg[11:] == fw[:9] + fw[11:], fw[:6]
                n_masked += 1
        assert n_masked <= len(stale)


@pytest.mark.parametrize("mode", list(so.MODES))
@pytest.mark.parametrize("kind", so.KINDS)
def test_mode_equals_the_reference(kind, mode, emul, tmp_path):
    """header and every record under the mode, line for line (SEQ / QUAL digested as in the fixture; NM / de values ignored on the records
    of STALE and nowhere else)"""
    hdr, body = so.golden(kind, mode)
    text = dump(kind, "sam", so.MODE_FLAG[mode], rg=so.RG_ARG if mode in so.MODE_RG else None, hdr=[so.VERSION] + so.ref_argv(kind, mode),
                with_qual=mode != "Q")  # (-Q: the reference does not read the qualities; the flag alone is test_no_qual_ignores_quals)
    out = run_emul(emul, "fmt", text, tmp_path)
    lines = out.split("\n")[:-1]
    assert lines[:len(hdr)] == hdr  # byte for byte: @SQ, @RG, @PG with VN: and CL:
    same_lines(kind, [so.digest_line(l) for l in lines[len(hdr):]], body, stale_keys(kind, emul, tmp_path))


def test_no_qual_ignores_quals(emul, tmp_path):
    """MM_F_NO_QUAL prints * whatever the caller passes as qualities"""
    _, body = so.golden("hifi_sv", "Q")
    lines = run_emul(emul, "fmt", dump("hifi_sv", "sam", so.F_NO_QUAL), tmp_path).split("\n")[:-1]
    same_lines("hifi_sv", [so.digest_line(l) for l in lines], body, stale_keys("hifi_sv", emul, tmp_path))


def test_comment_needs_the_flag(emul, tmp_path):
    """a comment handed to the writers is printed under MM_F_COPY_COMMENT only, and a read group needs no flag"""
    got = run_emul(emul, "fmt", dump("sr", "sam", 0), tmp_path).split("\n")[:-1]
    same_lines("sr", got, golden_sam("sr"), stale_keys("sr", emul, tmp_path))


@pytest.mark.parametrize("kind", so.PAF_KINDS)
def test_paf_copy_comment(kind, emul, tmp_path):
    """-y in PAF: the comment ends every mapped line and no --paf-no-hit line (LR/format.c:329-333, :357)"""
    got = run_emul(emul, "fmt", dump(kind, "paf", F_OUT_CG | F_PAF_NO_HIT | so.F_COPY_COMMENT), tmp_path).split("\n")[:-1]
    want = so.golden_paf_y(kind)
    plain = run_emul(emul, "fmt", dump(kind, "paf", F_OUT_CG | F_PAF_NO_HIT), tmp_path).split("\n")[:-1]
    assert len(got) == len(want) == len(plain)
    n = 0
    for g, w, p, pw in zip(got, want, plain, golden_paf(kind)):
        if p == pw:
            assert g == w, w.split("\t")[:6]
        else:  # a record of STALE: what -y adds to the line is still the reference's
            assert g[len(p):] == w[len(pw):], w.split("\t")[:6]
        n += g != p
    assert n > 0


# ---- -L ---------------------------------------------------------------------------------------------------------------------------
def long_cigar_case(n_ops, clip0, clip1, kind, flag, md=None):
    """One read with a short primary record and, as its second record, an alignment of n_ops operations 1M1I1M1I... on the forward
    strand behind clip0 and in front of clip1 read bases; kind: "only" (the read's only record, its primary), "supp" (0x800) or "sec"
    (0x100), both behind a short primary record.  Returns (dump text, the expected line of that record, whether its CIGAR goes to the tag),
    the expectation spelled out from LR/format.c:476-490 and :394-400."""
    n_m, n_i = (n_ops + 1) // 2, n_ops // 2
    qlen = clip0 + n_ops + clip1
    seq = ("ACGT" * (qlen // 4 + 1))[:qlen]
    qs, qe, rs = clip0, clip0 + n_ops, 1000
    re_ = rs + n_m
    blen = mlen = n_ops  # NM 0; de 0: blen + n_ambi - n_gap + n_gapo = blen with gaps of length 1
    cigar = "1M1I" * n_i + ("1M" if n_ops & 1 else "")
    t = ["MODE\tsam", "FLAG\t%d" % flag, "SQ\tchrL\t100000", "READ\tlong\t%s\t*" % seq]
    regs = []
    if kind != "only":
        regs.append("REG\t0 5 0 50 0 20 10 30 0 0 20 20 60 0 1 40 40 0 1\t20M\t%s" % ("20" if md else "-"))
    j = len(regs)
    parent = 0 if kind == "sec" else j
    sam_pri = 1 if kind == "only" else 0
    regs.append("REG\t%d 7 0 70 %d %d %d %d %d 3 %d %d 33 0 %d 90 91 0 1\t%s\t%s" % (j, qs, qe, rs, re_, parent, mlen, blen, sam_pri, cigar, md or "-"))
    text = "\n".join(t + regs) + "\n"
    sam_flag = {"only": 0, "supp": 0x800, "sec": 0x100}[kind]
    softclip = bool(flag & so.F_SOFTCLIP)
    in_tag = bool(flag & so.F_LONG_CIGAR) and n_ops > 65533 and n_ops + (qs != 0) + (qe != qlen) > 65535
    hard = sam_flag == 0x800 and not softclip
    if in_tag:
        slen = qlen if sam_flag == 0 or softclip else (0 if sam_flag == 0x100 else qe - qs)
        col = "%dS%dN" % (slen, re_ - rs)
    else:
        c = "H" if hard else "S"
        col = ("%d%s" % (clip0, c) if clip0 else "") + cigar + ("%d%s" % (clip1, c) if clip1 else "")
    if sam_flag == 0 or softclip:
        sq = seq
    elif sam_flag == 0x100:
        sq = "*"
    else:
        sq = seq[qs:qe]
    tags = ["NM:i:0", "ms:i:91", "AS:i:90", "nn:i:0", "tp:A:%s" % ("S" if kind == "sec" else "P"), "cm:i:7", "s1:i:70"]
    if kind != "sec":
        tags.append("s2:i:3")
    tags.append("de:f:0")
    if kind == "supp":  # the other record that is no secondary one: the short primary (LR/format.c:565-590)
        tags.append("SA:Z:chrL,11,+,20M%dS,60,0;" % (qlen - 20))
    if md:
        tags.append("MD:Z:" + md)
    if in_tag:
        code = 5 if hard else 4
        words = ([clip0 << 4 | code] if clip0 else []) + [1 << 4 | (k & 1) for k in range(n_ops)] + ([clip1 << 4 | code] if clip1 else [])
        tags.append("CG:B:I," + ",".join(str(w) for w in words))
    tags.append("rl:i:0")
    line = "\t".join(["long", str(sam_flag), "chrL", str(rs + 1), "33", col, "*", "0", "0", sq, "*"] + tags)
    return text, line, in_tag


L = so.F_LONG_CIGAR
Y = so.F_SOFTCLIP
LONG_CASES = [  # (operations, clip0, clip1, kind, flag, MD text, in the tag?)
    (65533, 3, 5, "only", L, None, False),          # n_cigar > 65533 fails, whatever the clips add
    (65534, 0, 0, "only", L, None, False),          # 65 534 operations in all
    (65534, 3, 0, "only", L, None, False),          # 65 535: the most BAM holds
    (65534, 0, 5, "only", L, None, False),
    (65534, 3, 5, "only", L, None, True),           # 65 536
    (65534, 3, 5, "only", 0, None, False),          # the same without -L
    (65535, 3, 0, "only", L, None, True),
    (65533, 3, 5, "supp", L | Y, None, False),      # the boundaries again on a supplementary record under -Y
    (65534, 3, 0, "supp", L | Y, None, False),
    (65534, 3, 5, "supp", L | Y, None, True),       # clip code 4, the whole read as SEQ and as <slen>S
    (65534, 3, 5, "supp", L, None, True),           # clip code 5, the aligned part as SEQ and as <slen>S
    (65534, 3, 5, "sec", L, None, True),            # 0x100: SEQ * and 0S
    (65534, 3, 5, "sec", L | Y, None, True),        # 0x100 under -Y: the whole read
    (65534, 3, 5, "only", L | F_OUT_MD, "1A2^C3", True),  # behind the MD string, in front of rl:i:0
]


@pytest.mark.parametrize("case", LONG_CASES, ids=lambda c: "%d_%d_%d_%s_%x%s" % (c[0], c[1], c[2], c[3], c[4], "_md" if c[5] else ""))
def test_long_cigar(case, emul, tmp_path):
    """MM_F_LONG_CIGAR on hand-built records: no committed read set comes near 65 534 operations (the longest CIGAR of any golden has
    1 627), so NO REFERENCE RUN backs this test; the expectation is written out in long_cigar_case from the reference's text
    (LR/format.c:476-490: the rule and the <slen>S<span>N placeholder; :394-400: the CG:B:I words and the clip code)."""
    n_ops, clip0, clip1, kind, flag, md, want_tag = case
    text, line, in_tag = long_cigar_case(n_ops, clip0, clip1, kind, flag, md)
    assert in_tag == want_tag
    got = run_emul(emul, "fmt", text, tmp_path).split("\n")[:-1]
    assert got[-1] == line
    assert ("\tCG:B:I," in got[-1]) == want_tag and len(got) == (1 if kind == "only" else 2)
    if want_tag:
        f = got[-1].split("\t")
        i = next(i for i, x in enumerate(f) if x.startswith("CG:B:I,"))
        assert f[i + 1] == "rl:i:0" and i + 2 == len(f) and (md is None or f[i - 1] == "MD:Z:" + md)


# ---- read group -------------------------------------------------------------------------------------------------------------------
def test_read_group_parser(emul, tmp_path):
    """sam_write_rg_line + mm_escape (LR/format.c:74-126): the reference's four refusals with its messages, the lone trailing backslash
    (refused here; the reference reads past the terminator), the three escapes, the id's end, and ids of 255 and 256 bytes"""
    cases = [
        (so.RG_ARG, "ok\t%s\t%s" % (so.RG_ID, so.RG_LINE)),
        ("RG\\tID:a", "err\tthe read group line is not started with @RG"),
        (" @RG\\tID:a", "err\tthe read group line is not started with @RG"),
        ("@RG\tID:a", "err\tthe read group line contained literal <tab> characters -- replace with escaped tabs: \\t"),
        ("@RG\\tSM:a", "err\tno ID within the read group line"),
        ("@RG ID:a", "err\tno ID within the read group line"),
        ("@RG\\tID:" + "i" * 256, "err\t@RG:ID is longer than 255 characters"),
        ("@RG\\tID:" + "i" * 255, "ok\t%s\t@RG\tID:%s" % ("i" * 255, "i" * 255)),
        ("@RG\\tID:" + "i" * 255 + "\\tSM:x", "ok\t%s\t@RG\tID:%s\tSM:x" % ("i" * 255, "i" * 255)),
        ("@RG\\tID:a\\", "err\tthe read group line ends in a lone backslash"),
        ("@RG\\tID:a\\\\", "ok\ta\\\t@RG\tID:a\\"),             # an escaped backslash at the end is fine
        ("@RG\\tID:a\\qb\\tPL:x", "ok\tab\t@RG\tID:ab\tPL:x"),   # backslash-q: both characters vanish
        ("@RG\\tSM:s\\tID:z", "ok\tz\t@RG\tSM:s\tID:z"),         # the id ends with the line
        ("@RGX\\tID:a", "ok\ta\t@RGX\tID:a"),                    # only the first three characters are looked at
    ]
    out = run_emul(emul, "rg", "".join(c[0] + "\n" for c in cases), tmp_path).split("\n")[:-1]
    assert out == [c[1] for c in cases]


def test_refused_read_group_stops_the_formatter(emul, tmp_path):
    run_emul(emul, "fmt", "MODE\tsam\nFLAG\t0\nRG\t@RG\\tSM:a\nSQ\tc\t10\n", tmp_path, status=4)


def test_header_without_read_group_version_or_arguments(emul, tmp_path):
    """mm_write_sam_hdr's optional parts (LR/format.c:137-144): no VN: without a version, no CL: with argc <= 1"""
    base = "MODE\tsam\nFLAG\t0\nSQ\tc1\t10\nSQ\tc2\t4000000000\n"
    assert run_emul(emul, "fmt", base + "HDR\t-\tprog\n", tmp_path) == "@SQ\tSN:c1\tLN:10\n@SQ\tSN:c2\tLN:-294967296\n@PG\tID:minimap2\tPN:minimap2\n"
    assert run_emul(emul, "fmt", base + "HDR\t2.0\tprog\ta b\t-c\n", tmp_path).split("\n")[2] == "@PG\tID:minimap2\tPN:minimap2\tVN:2.0\tCL:minimap2 a b -c"

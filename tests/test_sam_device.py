"""CPU: SAM text as the device formatter writes it.  The oracle is gd_write_sam, which the SAM tests pin to the reference byte for byte:
the host's flattening (sam_flatten.h) and the 64-lane line code (sam_record.h, the statements of sam_encode_kernel) must give exactly
the text the existing writer prints for the same records, and gds_line_size must be every line's length.  tests/emul/sam_emul.cpp runs
both as a stand-alone program under AddressSanitizer / UBSan on exact-size buffers, with the lanes running 0..63 and 63..0.
  * the goldens hifi_sv / ont_sv / sr rebuilt as records (test_samopts.records_of), plain and under every mode of samopts_io.MODES (there
    the text must also be the committed output of the reference), with MD / cs strings attached, and with = / X CIGARs;
  * test_samopts.long_cigar_case under -L: the placeholder, and CG:B:I behind the difference tag;
  * hand-built records at the edges of every field."""
import gzip
import os
import subprocess

import pytest

from conftest import ROOT
from diffstr_ref import tag_rows as golden_rows
from fixture_io import golden_sam
import samopts_io as so
from test_bam import with_strings
from test_samopts import LONG_CASES, dump, long_cigar_case, mask_nm_de

GOLDEN = os.path.join(ROOT, "tests", "golden")
F_OUT_CS, F_OUT_MD = 0x40, 0x1000000


def build_emul(directory):
    exe = os.path.join(str(directory), "sam_emul")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "genome-on-diet_amd", "csrc"), os.path.join(ROOT, "tests", "emul", "sam_emul.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    return build_emul(tmp_path_factory.mktemp("sam_device"))


def run_emul(emul, text, tmp_path, status=0):
    """(the text the existing writer prints, the text the 64 lanes write, gds_line_size of every row) of a dump, all as bytes / ints; with
    another status: the message on stderr.  text: str (written as latin-1, so that a dump can carry any byte) or bytes"""
    path, out = os.path.join(str(tmp_path), "in.txt"), os.path.join(str(tmp_path), "out.sam")
    with open(path, "wb") as f:
        f.write(text if isinstance(text, bytes) else text.encode("latin-1"))
    for p in (out, out + ".sizes"):
        if os.path.exists(p):
            os.remove(p)
    r = subprocess.run([emul, "fmt", path, out], capture_output=True)
    assert r.returncode == status, (r.returncode, r.stderr[-2000:])
    if status:
        assert not os.path.exists(out)
        return r.stderr.decode("latin-1")
    return r.stdout, open(out, "rb").read(), [int(x) for x in open(out + ".sizes").read().split()]


def check(emul, text, tmp_path):
    """the lanes' text is the existing writer's, and every row's size is its line's length; returns the record lines as str (latin-1)"""
    host, dev, sizes = run_emul(emul, text, tmp_path)
    assert len(dev) == len(host)
    assert dev == host
    lines = host.split(b"\n")[:-1]
    body = [l for l in lines if not l.startswith(b"@")] if b"\nHDR\t" in (text if isinstance(text, bytes) else text.encode("latin-1")) else lines
    assert sizes == [len(l) + 1 for l in body]
    return [l.decode("latin-1") for l in body]


# ---- the goldens as records -------------------------------------------------------------------------------------------------------
_plain = {}


def stale_keys(kind, emul, tmp_path):
    """(qname, FLAG, POS) of the records whose NM / de values their plain golden line does not determine (test_samopts.STALE)"""
    if kind not in _plain:
        got, want = check(emul, dump(kind, "sam", 0), tmp_path), golden_sam(kind)
        assert len(got) == len(want)
        keys = set()
        for g, w in zip(got, want):
            if g != w:
                assert mask_nm_de(g) == mask_nm_de(w), w.split("\t")[:4]
                f = w.split("\t")
                keys.add((f[0], f[1], f[3]))
        _plain[kind] = keys
    return _plain[kind]


@pytest.mark.parametrize("kind", so.KINDS)
def test_goldens_plain(kind, emul, tmp_path):
    """with no option the lanes write the committed plain golden (but for NM / de of the stale records, whose number test_samopts pins)"""
    from test_samopts import STALE
    assert len(stale_keys(kind, emul, tmp_path)) == STALE[kind][0]


@pytest.mark.parametrize("mode", list(so.MODES))
@pytest.mark.parametrize("kind", so.KINDS)
def test_goldens_under_every_mode(kind, mode, emul, tmp_path):
    """the lanes' text is the host writer's AND the reference's committed output under the mode (tests/golden/samopts, SEQ / QUAL as digests)"""
    hdr, body = so.golden(kind, mode)
    text = dump(kind, "sam", so.MODE_FLAG[mode], rg=so.RG_ARG if mode in so.MODE_RG else None, hdr=[so.VERSION] + so.ref_argv(kind, mode), with_qual=mode != "Q")
    lines = check(emul, text, tmp_path)
    stale = stale_keys(kind, emul, tmp_path)
    assert len(lines) == len(body)
    for g, w in zip(lines, body):
        g, f = so.digest_line(g), w.split("\t")
        if (f[0], f[1], f[3]) in stale:
            g, w = mask_nm_de(g), mask_nm_de(w)
        assert g == w, (kind, f[:4])


@pytest.mark.parametrize("tag", ["md", "cs", "cs_long"])
@pytest.mark.parametrize("kind", so.KINDS)
def test_goldens_with_difference_strings(kind, tag, emul, tmp_path):
    """the reference's own MD / cs strings (tests/golden/tags) attached to the records: the tag sits behind SA and in front of rl"""
    flag = F_OUT_MD if tag == "md" else F_OUT_CS
    rows = golden_rows("%s.%s" % (kind, tag))
    assert len(rows) == len(golden_sam(kind))
    lines = check(emul, with_strings(dump(kind, "sam", flag), kind, rows), tmp_path)
    key = "\tMD:Z:" if tag == "md" else "\tcs:Z:"
    assert sum(key in l for l in lines) == sum(1 for r in rows if r[-1]) > 0


def test_sr_with_eqx_cigars(emul, tmp_path):
    """the = / X CIGARs the reference prints under --eqx (tests/golden/eqx/sr.sam.tsv.gz) in place of the M ones: letters 7 and 8"""
    rows = [l.rstrip("\n").split("\t") for l in gzip.open(os.path.join(GOLDEN, "eqx", "sr.sam.tsv.gz"), "rt")]
    mapped = [r for r in rows if not int(r[1]) & 4]
    lines = check(emul, with_strings(dump("sr", "sam", 0), "sr", mapped, cigars=True), tmp_path)
    assert sum("=" in l.split("\t")[5] for l in lines) > 1000 and any("X" in l.split("\t")[5] for l in lines)


# ---- -L ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LONG_CASES, ids=lambda c: "%d_%d_%d_%s_%x%s" % (c[0], c[1], c[2], c[3], c[4], "_md" if c[5] else ""))
def test_long_cigar(case, emul, tmp_path):
    """MM_F_LONG_CIGAR around the 65 535-operation limit: 1 024 rounds of the scan with a carry; the placeholder <slen>S<re - rs>N, and
    CG:B:I behind the difference tag and in front of rl:i:0"""
    n_ops, clip0, clip1, kind, flag, md, want_tag = case
    text, line, in_tag = long_cigar_case(n_ops, clip0, clip1, kind, flag, md)
    assert in_tag == want_tag
    lines = check(emul, text, tmp_path)
    assert lines[-1] == line and ("\tCG:B:I," in lines[-1]) == want_tag


# ---- hand-built records -----------------------------------------------------------------------------------------------------------
HEAD = "MODE\tsam\nFLAG\t%d\nSQ\tc1\t100000\nSQ\tc2\t300000000\nSQ\t%s\t5\n" % (0, "contig_with_a_long_name." * 4)


def head(flag):
    return HEAD.replace("FLAG\t0", "FLAG\t%d" % flag)


def reg(j=0, cnt=5, rid=0, score=50, qs=0, qe=1, rs=10, re_=None, parent=None, subsc=0, mlen=None, blen=None, mapq=60, rev=0, pri=1, as_=40, ms=40, nn=0, cigar=None, ds="-"):
    n = qe - qs
    cigar = cigar if cigar is not None else "%dM" % n
    re_ = rs + n if re_ is None else re_
    nums = [j, cnt, rid, score, qs, qe, rs, re_, j if parent is None else parent, subsc, n if mlen is None else mlen, n if blen is None else blen, mapq, rev, pri, as_, ms, nn, 1]
    return "REG\t%s\t%s\t%s\n" % (" ".join(str(x) for x in nums), cigar, ds)


NUMBERS = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000, 999999999, 1000000000, 2147483646]
SIGNED = NUMBERS + [-1, -9, -10, -99, -100, -2147483647, -2147483648]


def test_numbers_of_every_width(emul, tmp_path):
    """every decimal width, with and without a sign, in POS, MAPQ and the numeric tags (NM = blen - mlen + nn is kept inside an int)"""
    t = head(0)
    n = len(SIGNED)
    for k, v in enumerate(SIGNED):
        u = NUMBERS[k % len(NUMBERS)]
        t += "READ\tv%d\tACGT\tIIII\n" % k + reg(qe=4, score=v, as_=SIGNED[(k + 1) % n], ms=SIGNED[(k + 3) % n], subsc=SIGNED[(k + 5) % n], cnt=SIGNED[(k + 7) % n], nn=u, blen=0,
                                                 mlen=k * 37 % 200, rs=u, re_=u + 4 if u < 2147483640 else u, mapq=(0, 9, 10, 99, 100, 255)[k % 6])
    lines = check(emul, t, tmp_path)
    assert ["s1:i:%d" % v in l.split("\t") for l, v in zip(lines, SIGNED)] == [True] * n
    assert [l.split("\t")[3] for l in lines] == [str(NUMBERS[k % len(NUMBERS)] + 1) for k in range(n)]
    assert any("\tNM:i:-" in l for l in lines) and any("\tnn:i:2147483646\t" in l for l in lines)


def cigar_of(n_ops, widths=False):
    """n_ops operations MIMD... of 1 to 3 bases; widths: M of 1 to 3 bases and D of 1, 10, ... 100 000 000 in turn, so that lengths of
    every width from 1 to 9 digits mix within the CIGAR while the read stays short"""
    if widths:
        return [(1 + k % 3, "M") if k % 2 == 0 else (10 ** (k // 2 % 9), "D") for k in range(n_ops)]
    return [(1 + k % 3, "MIMD"[k % 4]) for k in range(n_ops)]


@pytest.mark.parametrize("n_ops", [0, 1, 63, 64, 65, 128, 129])
def test_operation_counts_around_the_rounds_of_the_scan(n_ops, emul, tmp_path):
    """0 .. 129 operations with 0, 1 and 2 clips: the carry crosses no round, one round and two rounds; on both strands, on a primary
    (S clips) and a supplementary (H clips) record; once with lengths of every width from 1 to 9 digits mixed within the CIGAR"""
    t = head(0)
    for widths in (False, True):
        ops = cigar_of(n_ops, widths)
        q = sum(n for n, op in ops if op in "MI")
        ref = sum(n for n, op in ops if op in "MD")
        cg = "".join("%d%s" % x for x in ops)
        for c0, c1 in ((0, 0), (3, 0), (0, 12), (123, 4567)):
            L = c0 + q + c1
            if L == 0:
                continue
            for rev in (0, 1):
                qs, qe = (c1, c1 + q) if rev else (c0, c0 + q)
                t += "READ\tr%d_%d_%d\t%s\t%s\n" % (c0, c1, rev, ("ACGTN" * L)[:L], ("IJKLMNO" * L)[:L])
                t += reg(0, qs=qs, qe=qe, rev=rev, cigar=cg, re_=10 + ref, mlen=q, blen=q + ref) + reg(1, qs=qs, qe=qe, rev=rev, pri=0, rid=1, cigar=cg, re_=10 + ref, mlen=q, blen=q + ref)
    if n_ops == 0:  # (a CIGAR of no operation is printed as its clips alone, or as nothing)
        lines = check(emul, t, tmp_path)
        assert {l.split("\t")[5] for l in lines} >= {"3S", "3H", "12S", "123H4567H"}
        return
    lines = check(emul, t, tmp_path)
    cols = {l.split("\t")[5] for l in lines}
    plain = "".join("%d%s" % x for x in cigar_of(n_ops))
    assert {plain, "3S" + plain, plain + "12S", "123H" + plain + "4567H"} <= cols
    if n_ops >= 18:  # (the generator's mixed lengths do cover every width from 1 to 9 digits, and the lanes printed them)
        assert {len(str(n)) for n, _ in cigar_of(n_ops, True)} == set(range(1, 10))
        assert any("100000000D" in c and "10000D" in c for c in cols)


def test_names_comments_and_read_groups(emul, tmp_path):
    """names of 1 and 300 bytes; a free-text comment, an empty one and none, with and without -y; RG:Z: on mapped and unmapped lines"""
    for flag, rg in ((0, None), (so.F_COPY_COMMENT, None), (so.F_COPY_COMMENT, so.RG_ARG)):
        t = head(flag).replace("SQ\tc1", ("RG\t%s\n" % rg if rg else "") + "SQ\tc1")
        t += "READ\tx\tAC\tII\nCOMMENT\tfree text, with\ttabs and : colons\n" + reg(qe=2)
        t += "READ\t%s\tACG\tIII\nCOMMENT\t\n" % ("n" * 300) + reg(qe=3, rid=2)
        t += "READ\tun\tACGTN\tIIIII\nCOMMENT\tXX:i:1\n"
        t += "READ\tplain\tACGTN\tIIIII\n" + reg(qe=5)
        lines = check(emul, t, tmp_path)
        assert len(lines) == 4 and lines[1].startswith("n" * 300 + "\t0\tcontig_with_a_long_name.contig_")
        assert lines[0].endswith("\trl:i:0\tfree text, with\ttabs and : colons") == bool(flag) and lines[1].endswith("rl:i:0\t") == bool(flag)
        assert all(("\tRG:Z:%s\t" % so.RG_ID in l) == bool(rg) for l in lines)


def test_seq_and_qual_bytes_on_both_strands(emul, tmp_path):
    """lower case, IUPAC letters, '*', '.', '=' and bytes >= 128 in SEQ: complemented through comp_tab with their case kept on the reverse
    strand, every other byte unchanged; QUAL reversed; lengths around one and two rounds of 64"""
    alphabet = "ACGTNacgtnRYKMSWBDHVrykmswbdhvUuXxZz*.=-\x80\xe9\xff@[`{"
    t = head(0).encode("latin-1")
    for L in (1, 2, 63, 64, 65, 127, 128, 129, len(alphabet)):
        sq = (alphabet * 4)[:L] if L != len(alphabet) else alphabet
        ql = "".join(chr(33 + (7 * i) % 94) for i in range(L))
        for rev in (0, 1):
            t += ("READ\ts%d_%d\t%s\t%s\n" % (L, rev, sq, ql) + reg(qe=L, rev=rev)).encode("latin-1")
    lines = check(emul, t, tmp_path)
    comp = dict(zip("ABCDEFGHIJKLMNOPQRSTUVWXYZ", "TVGHEFCDIJMLKNOPQYSAABWXRZ"))
    comp.update({k.lower(): v.lower() for k, v in comp.items()})
    f = lines[-1].split("\t")
    assert f[1] == "16" and f[9] == "".join(comp.get(c, c) for c in reversed(alphabet)) and "\xff" in f[9] and f[10] == "".join(chr(33 + (7 * i) % 94) for i in range(len(alphabet)))[::-1]


def test_missing_pieces_under_the_flags(emul, tmp_path):
    """no qualities; SEQ * on a secondary record; an unmapped read; -Q; a supplementary record's slice, hard- and (-Y) soft-clipped;
    --sam-hit-only; secondary records dropped; a record without a CIGAR"""
    for flag in (0, so.F_NO_QUAL, so.F_SOFTCLIP, so.F_SAM_HIT_ONLY, 0x4000, so.F_SOFTCLIP | so.F_NO_QUAL | 0x4000):
        t = head(flag)
        t += "READ\tnoq\tACGTACGTAC\t*\n" + reg(qe=10)
        t += "READ\ttwo\tACGTACGTACGT\tABCDEFGHIJKL\n" + reg(0, qs=0, qe=8, score=90) + reg(1, qs=2, qe=9, parent=0, score=20, rid=1, rs=268435450, rev=1)
        t += "READ\tun\tACGTN\tIIIII\n"
        t += "READ\tempty\t\t*\n"
        t += "READ\tsup\tACGTACGTACGT\tABCDEFGHIJKL\n" + reg(0, qs=0, qe=5, score=90) + reg(1, qs=6, qe=11, score=20, pri=0, rid=2, rs=0, rev=1, cigar="2M1D3M", re_=6)
        t += "READ\tnop\tACGT\tIIII\n" + reg(qe=4)[:-1].rsplit("\t", 2)[0].rsplit(" ", 1)[0] + " 0\t*\t-\n"
        lines = check(emul, t, tmp_path)
        if flag == 0:
            f = [l.split("\t") for l in lines]
            assert [x[1] for x in f] == ["0", "0", "272", "4", "4", "0", "2064", "0"] and f[2][9:11] == ["*", "*"] and f[0][10] == "*" and f[6][5] == "1H2M1D3M6H" and "SA:Z:" in lines[5]
            assert f[4][9:11] == ["", "*"] and f[7][5] == "*" and "NM:i:" not in lines[7] and "de:f:" not in lines[7]


def test_de_texts(emul, tmp_path):
    """de:f: as the host formats it: 0 (exact identity), 0.0000 (a divergence that rounds to nothing), 1.0000, and a negative one"""
    t = head(0)
    for k, (mlen, blen) in enumerate([(100, 100), (99999, 100000), (0, 100), (150, 100), (1, 3)]):
        t += "READ\td%d\tACGT\tIIII\n" % k + reg(qe=4, mlen=mlen, blen=blen)
    lines = check(emul, t, tmp_path)
    assert [[x for x in l.split("\t") if x.startswith("de:f:")][0][5:] for l in lines] == ["0", "0.0000", "1.0000", "-0.5000", "0.6667"]


def test_empty_batches(emul, tmp_path):
    """no read at all; --sam-hit-only with nothing mapped: no line, no byte, and no failure"""
    assert run_emul(emul, head(0), tmp_path) == (b"", b"", [])
    assert run_emul(emul, head(so.F_SAM_HIT_ONLY) + "READ\tu1\tACGT\tIIII\nREAD\tu2\tAC\t*\n", tmp_path) == (b"", b"", [])
    assert len(check(emul, head(0) + "READ\tu1\tACGT\tIIII\nREAD\tu2\tAC\t*\n", tmp_path)) == 2


def test_a_record_outside_its_read_is_refused(emul, tmp_path):
    """the emulator's parser refuses such a dump itself (status 3), as bam_emul does: the rows' offsets are the host's to check"""
    run_emul(emul, head(0) + "READ\tbad\tACGT\tIIII\n" + reg(qe=5), tmp_path, status=3)

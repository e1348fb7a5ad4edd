"""GPU: the SAM / PAF output options through every entry point that carries them -- Mapper.sam_batch / sam_batch_raw / paf_batch_seqs /
sam_header / set_read_group on whole mapped read sets, and tools/map_file.py from file to file -- against what the reference printed
under -Y, --sam-hit-only, -Q, -y, -R and all of them together (tests/golden/samopts/, tools/make_samopts_golden.py).  SEQ and QUAL are
digested as in the fixtures; nothing is masked."""
import io
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from fixture_io import OVERRIDES, SETS, golden_sam, read_fasta
import samopts_io as so

pytestmark = pytest.mark.gpu

F_CG, F_PAF_NO_HIT = 0x20, 0x8000000
_mapped = {}


@pytest.fixture(scope="module")
def mapped(pkg, gpu_ctx):
    """kind -> (mapper, reads with comments, MapResult), each kind mapped once for the module"""
    def get(kind):
        if kind not in _mapped:
            base, _, preset = SETS[kind]
            names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
            reads = so.reads_with_comments(kind)
            m = pkg.Mapper(gpu_ctx, names, seqs, preset=preset, **OVERRIDES.get(kind, {}))
            _mapped[kind] = (m, reads, m.map([r[1] for r in reads]))
        return _mapped[kind]
    yield get
    for m, _, _ in _mapped.values():
        m.close()
    _mapped.clear()


class under:
    """the mapper's flag and the context's read group set for a mode, and put back"""

    def __init__(self, m, mode, extra=0):
        self.m, self.mode, self.extra = m, mode, extra

    def __enter__(self):
        self.flag = self.m.opt.flag
        self.m.opt.flag = self.flag | so.MODE_FLAG[self.mode] | self.extra
        if self.mode in so.MODE_RG:
            self.m.set_read_group(so.RG_ARG)

    def __exit__(self, *a):
        self.m.opt.flag = self.flag
        self.m.set_read_group(None)  # (the context is shared by the whole session)


def write_fastq(kind, path):
    with open(path, "w") as f:
        for name, seq, qual, cm in so.reads_with_comments(kind):
            f.write("@%s%s\n%s\n+\n%s\n" % (name, "" if cm is None else " " + cm, seq, qual))


def digested(text):
    assert text == "" or text.endswith("\n")
    return [so.digest_line(l) for l in text.split("\n")[:-1]]


def test_constants(pkg):
    assert (pkg.map_api.F_SOFTCLIP, pkg.map_api.F_LONG_CIGAR, pkg.map_api.F_COPY_COMMENT, pkg.map_api.F_NO_QUAL, pkg.map_api.F_SAM_HIT_ONLY) == \
        (0x80000, 0x10000, 0x2000000, 0x10, 0x40000000)


@pytest.mark.parametrize("mode", list(so.MODES))
@pytest.mark.parametrize("kind", so.KINDS)
def test_sam_batch_under_mode(kind, mode, mapped):
    """Mapper.sam_batch: the reference's records under the mode, and Mapper.sam_header its header"""
    m, reads, res = mapped(kind)
    hdr, body = so.golden(kind, mode)
    with under(m, mode):
        got = digested(m.sam_batch(res, reads))
        head = m.sam_header(so.VERSION, so.ref_argv(kind, mode))
    assert len(got) == len(body)
    for g, w in zip(got, body):
        assert g == w, w.split("\t")[:4]
    assert head == "".join(l + "\n" for l in hdr)
    # the options are gone again: the plain golden
    assert m.sam_batch(res, reads) == "".join(l + "\n" for l in golden_sam(kind))


def test_long_cigar_flag_changes_nothing_here(mapped):
    m, reads, res = mapped("hifi_sv")
    flag = m.opt.flag
    m.opt.flag = flag | so.F_LONG_CIGAR
    try:
        assert m.sam_batch(res, reads) == "".join(l + "\n" for l in golden_sam("hifi_sv"))
    finally:
        m.opt.flag = flag


def test_sam_record_honours_softclip_and_no_qual(mapped):
    """gdiet_hip_sam_record has no context: -Y and -Q through the flag, no RG:Z: and no comment"""
    m, reads, res = mapped("hifi_sv")
    _, body = so.golden("hifi_sv", "Y")
    _, body_q = so.golden("hifi_sv", "Q")
    with under(m, "all"):
        m.opt.flag &= ~(so.F_SAM_HIT_ONLY | so.F_COPY_COMMENT)
        got = [so.digest_line(l) for i, r in enumerate(reads) for l in m.sam(res, i, r[0], r[1], r[2])]
    assert got == body
    with under(m, "Q"):
        got = [so.digest_line(l) for i, r in enumerate(reads) for l in m.sam(res, i, r[0], r[1], r[2])]
    assert got == body_q


@pytest.mark.parametrize("mode,with_sink", [("y", True), ("all", True), ("all", False), ("Q", True)])
def test_sam_batch_raw_with_comments(mode, with_sink, mapped, pkg, tmp_path):
    """the route of tools/map_file.py on sr: the reader's C arrays (names, comments, sequences, qualities) into gdiet_hip_sam_batch_comments_into,
    into the mapper's own buffer (sink) or a fresh one"""
    m, _, _ = mapped("sr")
    fq = str(tmp_path / "reads.fq")
    write_fastq("sr", fq)
    _, body = so.golden("sr", mode)
    fx = pkg.FastxReader(fq)
    try:
        n, names, comments, seqs, quals, lens, _ = fx.read_raw(1 << 30, with_qual=mode != "Q", with_comment=True)
        assert n == 2000
        batch = m.upload_raw(n, seqs, lens)
        try:
            res = m.map_uploaded(batch)
            with under(m, mode):
                if with_sink:
                    sink = io.BytesIO()
                    length = m.sam_batch_raw(res, n, names, seqs, quals, lens, sink, comments)
                    text = sink.getvalue()
                    assert length == len(text)
                else:
                    text = m.sam_batch_raw(res, n, names, seqs, quals, lens, comments=comments)
            assert digested(text.decode()) == body
            # the comments are there, the flag is not: the plain golden
            sink = io.BytesIO()
            m.sam_batch_raw(res, n, names, seqs, quals, lens, sink, comments)
            if mode != "Q":
                assert sink.getvalue().decode() == "".join(l + "\n" for l in golden_sam("sr"))
        finally:
            m.free_batch(batch)
    finally:
        fx.close()


@pytest.mark.parametrize("kind", so.PAF_KINDS)
def test_paf_batch_seqs_copy_comment(kind, mapped):
    m, reads, res = mapped(kind)
    want = so.golden_paf_y(kind)
    got = m.paf_batch_seqs(res, reads, flag=F_CG | F_PAF_NO_HIT | so.F_COPY_COMMENT)
    assert got == "".join(l + "\n" for l in want)
    from fixture_io import golden_paf
    assert m.paf_batch_seqs(res, reads, flag=F_CG | F_PAF_NO_HIT) == "".join(l + "\n" for l in golden_paf(kind))  # no flag, no comment


def test_read_group_through_the_abi(mapped, pkg):
    """gdiet_hip_set_read_group: a refusal is GDIET_E_PARAM with the reference's message and leaves no read group behind"""
    m, reads, res = mapped("ont_sv")
    plain_head = m.sam_header(so.VERSION, ["x"])
    assert "@RG" not in plain_head and plain_head.endswith("@PG\tID:minimap2\tPN:minimap2\tVN:%s\n" % so.VERSION)
    try:
        m.set_read_group(so.RG_ARG)
        assert so.RG_LINE + "\n" in m.sam_header(so.VERSION, ["x"])
        for bad, msg in (("RG\\tID:a", "not started with @RG"), ("@RG\tID:a", "literal <tab>"), ("@RG\\tSM:a", "no ID within"),
                         ("@RG\\tID:" + "i" * 256, "longer than 255"), ("@RG\\tID:a\\", "lone backslash")):
            m.set_read_group(so.RG_ARG)
            with pytest.raises(pkg.GdietError, match=msg):
                m.set_read_group(bad)
            assert m.sam_header(so.VERSION, ["x"]) == plain_head
        assert m.sam_batch(res, reads) == "".join(l + "\n" for l in golden_sam("ont_sv"))
        m.set_read_group("@RG\\tID:" + "i" * 255)
        assert m.sam_batch(res, reads[:1]).split("\t")[11] == "RG:Z:" + "i" * 255
    finally:
        m.set_read_group(None)


def test_map_file_end_to_end_with_every_option(tmp_path):
    """tools/map_file.py as a program, from the FASTQ with comments to a SAM file with header: the reference's whole standard output of
    mode `all`, except the @PG line, which names this tool's version and command line"""
    fq, out = str(tmp_path / "reads.fq"), str(tmp_path / "out.sam")
    write_fastq("hifi_sv", fq)
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "map_file.py"), "--preset", "hifi", "--header", "-R", so.RG_ARG, "-Y", "-y",
           "--sam-hit-only", os.path.join(SETS["hifi_sv"][0], "ref.fa.gz"), fq, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    hdr, body = so.golden("hifi_sv", "all")
    got = open(out).read()
    assert got.endswith("\n")
    lines = got.split("\n")[:-1]
    assert len(lines) == len(hdr) + len(body)
    pg = [i for i, l in enumerate(hdr) if l.startswith("@PG")]
    assert pg == [len(hdr) - 1]
    assert lines[:pg[0]] == hdr[:pg[0]]
    assert lines[pg[0]].startswith("@PG\tID:minimap2\tPN:minimap2\tVN:") and "\tCL:minimap2 --preset hifi --header -R " in lines[pg[0]]
    assert [so.digest_line(l) for l in lines[len(hdr):]] == body


def test_map_file_without_new_options_writes_the_plain_body(tmp_path, monkeypatch, capsys):
    """no new option: what the tool always wrote -- the plain golden body, no header, whatever comments the FASTQ holds"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import map_file
    fq, out = str(tmp_path / "reads.fq"), str(tmp_path / "out.sam")
    write_fastq("hifi_sv", fq)
    monkeypatch.setattr(sys, "argv", ["map_file.py", "--preset", "hifi", os.path.join(SETS["hifi_sv"][0], "ref.fa.gz"), fq, "-o", out])
    map_file.main()
    assert open(out).read() == "".join(l + "\n" for l in golden_sam("hifi_sv"))

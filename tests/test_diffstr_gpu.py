"""GPU: the cs / cs=long / MD difference strings computed on the device (map_diffstr.hip.h) through every entry point that carries them:
gdiet_hip_diffstr_batch on the hand-built synthetic set (tests/diffstr_ref.py: expected values from the restatement that
tests/test_diffstr.py pins on the reference's own tags), gdiet_hip_sam_batch and gdiet_hip_paf_batch_seqs on whole mapped read sets
against what the reference printed under --MD / --cs / --cs=long (tests/golden/tags/, tools/make_tags_golden.py)."""
import ctypes as C
import os

import pytest

import diffstr_ref as dr
from fixture_io import OVERRIDES, SETS, golden_paf, golden_sam, read_fasta, reads_of
from test_map_host import _norm_ms

pytestmark = pytest.mark.gpu

F_CG, F_PAF_NO_HIT = 0x20, 0x8000000
SAM_KINDS = ("hifi_sv", "sr", "sr_edge", "hifi_edge")
PAF_ROWS = (("hifi_sv", "cs", dr.MODE_FLAG["cs"]), ("hifi_sv", "qstrand_cs", dr.MODE_FLAG["cs"] | dr.F_QSTRAND),
            ("hifi_sv", "qstrand_md", dr.MODE_FLAG["md"] | dr.F_QSTRAND), ("sr", "cs", dr.MODE_FLAG["cs"]))


class HandRes:
    """hand-built records in the arrays a MapResult holds (n_regs / regs of gdiet_hip_map_batch); recs: dicts of diffstr_ref"""

    def __init__(self, pkg, n_reads, recs):
        from genome_on_diet_amd.map_api import Reg
        per = [[r for r in recs if r["read"] == i] for i in range(n_reads)]
        self.n_regs = (C.c_int32 * n_reads)(*[len(p) for p in per])
        self.regs = (C.POINTER(Reg) * n_reads)()
        self._keep = []
        for i, p in enumerate(per):
            if not p:
                continue
            arr = (Reg * len(p))()
            for j, r in enumerate(p):
                words = (C.c_uint32 * len(r["cigar"]))(*[n << 4 | o for o, n in r["cigar"]])
                self._keep.append(words)
                arr[j].id = arr[j].parent = j
                arr[j].rid, arr[j].qs, arr[j].qe, arr[j].rs, arr[j].re, arr[j].rev = r["rid"], r["qs"], r["qe"], r["rs"], r["re"], r["rev"]
                arr[j].n_cigar, arr[j].cigar = len(r["cigar"]), C.cast(words, C.POINTER(C.c_uint32))
            self._keep.append(arr)
            self.regs[i] = C.cast(arr, C.POINTER(Reg))


def ascii_of(codes):
    return dr._UP[codes].tobytes().decode()


@pytest.fixture(scope="module")
def synth(pkg, gpu_ctx):
    contigs4, reads4, recs, notes = dr.synthetic_set()
    m = pkg.Mapper(gpu_ctx, ["c%d" % i for i in range(len(contigs4))], [ascii_of(c) for c in contigs4], preset="hifi")
    reads = [ascii_of(r) for r in reads4]
    yield dict(m=m, contigs4=contigs4, reads4=reads4, reads=reads, recs=recs, notes=notes, res=HandRes(pkg, len(reads), recs))
    m.close()


_mapped = {}


@pytest.fixture(scope="module")
def mapped(pkg, gpu_ctx):
    """kind -> (mapper, reads, MapResult), each kind mapped once for the module"""
    def get(kind):
        if kind not in _mapped:
            base, _, preset = SETS[kind]
            names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
            reads = reads_of(kind)
            m = pkg.Mapper(gpu_ctx, names, seqs, preset=preset, **OVERRIDES.get(kind, {}))
            _mapped[kind] = (m, reads, m.map([r[1] for r in reads]))
        return _mapped[kind]
    yield get
    for m, _, _ in _mapped.values():
        m.close()
    _mapped.clear()


def tagged_sam(m, res, reads, bits):
    flag = m.opt.flag
    m.opt.flag = flag | bits
    try:
        return m.sam_batch(res, reads)
    finally:
        m.opt.flag = flag


def check_lines(got, plain, rows, col, where, prefix):
    """got: our lines; plain: the golden lines without a tag; rows[i][col]: the golden tag of line i ("" = none, "#..." = digest).  Every
    line is the plain one with "\\t<prefix><tag>" inserted at where(line)"""
    assert len(got) == len(plain) == len(rows)
    for g, p, r in zip(got, plain, rows):
        want_tag = r[col]
        if not want_tag:
            assert _norm_ms(g) == _norm_ms(p)
            continue
        bare, tag = g, None
        f = g.split("\t")
        hit = [i for i, x in enumerate(f) if x.startswith(prefix)]
        assert len(hit) == 1, (g[:200], prefix)
        tag = f[hit[0]][len(prefix):]
        bare = "\t".join(f[:hit[0]] + f[hit[0] + 1:])
        assert _norm_ms(bare) == _norm_ms(p), r[:3]
        assert where(f, hit[0]), r[:3]
        assert dr.same_tag(tag, want_tag), (r[:3], tag[:120], want_tag[:120])


@pytest.mark.parametrize("qstrand", [False, True])
@pytest.mark.parametrize("mode", dr.MODES)
def test_synthetic_set_through_diffstr_batch(synth, mode, qstrand):
    """hand-built records through gdiet_hip_diffstr_batch, once with host sequences (encoded and uploaded by the call) and once with a
    resident batch, against the pinned restatement"""
    m, recs = synth["m"], synth["recs"]
    flag = dr.MODE_FLAG[mode] | (dr.F_QSTRAND if qstrand else 0)
    want = [dr.expected(mode, r, synth["reads4"], synth["contigs4"], qstrand).encode() for r in recs]
    got = m.diffstr(synth["res"], synth["reads"], flag)
    assert [s for per in got for s in per] == want, [n for n, a, b in zip(synth["notes"], [s for per in got for s in per], want) if a != b]
    batch = m.upload(synth["reads"])
    try:
        got = m.diffstr(synth["res"], synth["reads"], flag, batch=batch)
    finally:
        m.free_batch(batch)
    assert [s for per in got for s in per] == want


def test_flags_of_diffstr_batch(synth):
    """both flags together mean MD; neither gives empty strings; the long bit alone gives nothing"""
    m, res, reads = synth["m"], synth["res"], synth["reads"]
    md = m.diffstr(res, reads, dr.MODE_FLAG["md"])
    assert m.diffstr(res, reads, dr.MODE_FLAG["md"] | dr.MODE_FLAG["cs_long"]) == md
    assert all(s == b"" for per in m.diffstr(res, reads, 0) for s in per)
    assert all(s == b"" for per in m.diffstr(res, reads, 0x800) for s in per)
    assert sum(len(per) for per in md) == len(synth["recs"])


@pytest.mark.parametrize("mode", dr.MODES)
@pytest.mark.parametrize("kind", SAM_KINDS)
def test_whole_path_sam_carries_the_reference_s_tag(mapped, kind, mode):
    """map, then gdiet_hip_sam_batch with the mode's bits: every line is the golden SAM line with the golden tag in front of rl:i:0"""
    m, reads, res = mapped(kind)
    got = tagged_sam(m, res, reads, dr.MODE_FLAG[mode]).rstrip("\n").split("\n")
    prefix = "MD:Z:" if mode == "md" else "cs:Z:"
    check_lines(got, golden_sam(kind), dr.tag_rows("%s.%s" % (kind, mode)), 4, lambda f, i: f[i + 1] == "rl:i:0" and i + 2 == len(f), prefix)
    assert sum(1 for g in got if "\t" + prefix in g) == sum(1 for r in dr.tag_rows("%s.%s" % (kind, mode)) if r[4]) > 0


@pytest.mark.parametrize("kind,name,bits", PAF_ROWS)
def test_whole_path_paf_carries_the_reference_s_tag(mapped, kind, name, bits):
    """gdiet_hip_paf_batch_seqs under -c --paf-no-hit: the golden PAF line (target interval on the read's strand under --qstrand, as
    mm_write_paf3 prints it) with the golden tag behind cg:Z:"""
    m, reads, res = mapped(kind)
    got = m.paf_batch_seqs(res, reads, flag=F_CG | F_PAF_NO_HIT | bits).rstrip("\n").split("\n")
    plain = []
    for line in golden_paf(kind):
        f = line.split("\t")
        if bits & dr.F_QSTRAND and f[4] == "-":
            f[7], f[8] = str(int(f[6]) - int(f[8])), str(int(f[6]) - int(f[7]))
        plain.append("\t".join(f))
    prefix = "MD:Z:" if bits & dr.MODE_FLAG["md"] else "cs:Z:"
    check_lines(got, plain, dr.tag_rows("%s.paf.%s" % (kind, name)), 3, lambda f, i: i + 1 == len(f) and f[i - 1].startswith("cg:Z:"), prefix)
    # the entry point without reads keeps ignoring the bits
    assert m.paf_batch(res, reads, flag=F_CG | F_PAF_NO_HIT | (bits & ~dr.F_QSTRAND)) == "".join(l + "\n" for l in golden_paf(kind))


def test_without_the_bits_the_sam_text_is_what_it_was(mapped):
    for kind in ("hifi_sv", "sr_edge"):
        m, reads, res = mapped(kind)
        assert m.sam_batch(res, reads) == "".join(l + "\n" for l in golden_sam(kind))
        assert tagged_sam(m, res, reads, 0x800) == "".join(l + "\n" for l in golden_sam(kind))  # the long bit alone selects nothing


def test_tagged_sam_while_a_ticket_is_open(pkg, mapped):
    """the tag pass works on a stream and buffers of its own: issued while another batch is in flight it gives the same text"""
    m, reads, _ = mapped("hifi_sv")
    ra, rb = reads[:60], reads[60:]
    ba, bb = m.upload([r[1] for r in ra]), m.upload([r[1] for r in rb])
    try:
        res_a = m.map_uploaded(ba)
        bits = dr.MODE_FLAG["cs"]
        want = tagged_sam(m, res_a, ra, bits)
        assert want.count("\tcs:Z:") > 50
        ticket = m.submit(bb)
        try:
            got = tagged_sam(m, res_a, ra, bits)
            per_read = m.diffstr(res_a, ra, dr.MODE_FLAG["md"], batch=ba)
        finally:
            res_b = m.wait(ticket)
        assert got == want
        assert sum(len(p) for p in per_read) == sum(res_a.n_regs[i] for i in range(len(ra)))
        want_b = [l for l in golden_sam("hifi_sv") if l.split("\t")[0] in {r[0] for r in rb}]
        assert m.sam_batch(res_b, rb) == "".join(l + "\n" for l in want_b)
    finally:
        m.free_batch(ba), m.free_batch(bb)


def test_a_bad_record_is_refused_and_the_context_goes_on(pkg, synth, mapped):
    """a CIGAR whose query sum disagrees with qe - qs: GDIET_E_PARAM from the host check (nothing is launched), one line of text; the
    same context then maps and tags the next batch"""
    m, reads = synth["m"], synth["reads"]
    recs = [dict(r) for r in synth["recs"]]
    recs[7]["qe"] -= 1
    with pytest.raises(pkg.GdietError) as e:
        m.diffstr(HandRes(pkg, len(reads), recs), reads, dr.MODE_FLAG["cs"])
    assert "error -3" in str(e.value) and "read 7 record 0" in str(e.value) and "\n" not in str(e.value)
    got = m.diffstr(synth["res"], reads, dr.MODE_FLAG["cs"])
    assert [s.decode() for per in got for s in per] == [dr.expected("cs", r, synth["reads4"], synth["contigs4"]) for r in synth["recs"]]
    # ... and through the SAM formatter: no text, the reason in strerror; then a mapped batch, tagged
    mh, hreads, _ = mapped("hifi_sv")
    sub = hreads[:12]
    res = mh.map([r[1] for r in sub])
    first = next(i for i in range(len(sub)) if res.n_regs[i] > 0)
    res.regs[first][0].qe -= 1
    try:
        with pytest.raises(pkg.GdietError):
            tagged_sam(mh, res, sub, dr.MODE_FLAG["md"])
    finally:
        res.regs[first][0].qe += 1
    res2 = mh.map([r[1] for r in sub])
    got = tagged_sam(mh, res2, sub, dr.MODE_FLAG["md"]).rstrip("\n").split("\n")
    names = {r[0] for r in sub}
    keep = [i for i, l in enumerate(golden_sam("hifi_sv")) if l.split("\t")[0] in names]
    plain, rows = golden_sam("hifi_sv"), dr.tag_rows("hifi_sv.md")
    check_lines(got, [plain[i] for i in keep], [rows[i] for i in keep], 4, lambda f, i: f[i + 1] == "rl:i:0", "MD:Z:")


def test_each_thread_reads_the_text_of_its_own_refusal(pkg, synth):
    """two writer threads on one context, each refused by the host check (nothing is launched) at another record: gdiet_hip_strerror
    answers every thread with the text of its own failure, and a thread that did not fail with neither"""
    import threading
    m, reads = synth["m"], synth["reads"]
    m.diffstr(synth["res"], reads, dr.MODE_FLAG["cs"])  # (the main thread's last call on the context succeeded)
    step = threading.Barrier(2)
    seen, raised = {}, {}

    def writer(name, k, first):
        recs = [dict(r) for r in synth["recs"]]
        recs[k]["qe"] -= 1
        res = HandRes(pkg, len(reads), recs)
        if not first:
            step.wait()  # B fails after A has
        try:
            m.diffstr(res, reads, dr.MODE_FLAG["cs"])
        except pkg.GdietError as e:
            raised[name] = str(e)
        if first:
            step.wait()
        step.wait()  # both have failed
        if not first:
            step.wait()  # B reads after A has
        seen[name] = m.lib.gdiet_hip_strerror(m.ctx._h).decode()
        if first:
            step.wait()

    ta, tb = threading.Thread(target=writer, args=("a", 7, True)), threading.Thread(target=writer, args=("b", 3, False))
    ta.start(), tb.start()
    ta.join(60), tb.join(60)
    assert not ta.is_alive() and not tb.is_alive()
    assert "read 7 record 0" in raised["a"] and "read 3 record 0" in raised["b"]
    assert "read 7 record 0" in seen["a"] and "read 3 record 0" not in seen["a"], seen
    assert "read 3 record 0" in seen["b"] and "read 7 record 0" not in seen["b"], seen
    mine = m.lib.gdiet_hip_strerror(m.ctx._h).decode()
    assert "read 7 record 0" not in mine and "read 3 record 0" not in mine, mine

"""GPU: --eqx of the ShortReads variant (MM_F_EQX next to MM_F_SR; the EQX form of map_post_kernel, map_kernels.hip.h) through every entry
point that maps, against what the reference printed under --eqx (tests/golden/eqx/, tools/make_eqx_golden.py): the committed golden SAM
with column 6 from the fixture, line for line."""
import os

import pytest

import diffstr_ref as dr
import eqx_ref as er
from fixture_io import OVERRIDES, SETS, golden_paf, golden_sam, read_fasta, reads_of

pytestmark = pytest.mark.gpu

F_CG = 0x20


def text(lines):
    return "".join(l + "\n" for l in lines)


def sr_mapper(pkg, ctx, kind, eqx=True):
    from genome_on_diet_amd.map_api import F_EQX, F_FRAG_MODE, F_SR
    names, seqs = er.reference_of(kind)
    ov = dict(OVERRIDES.get(kind, {}))
    return pkg.Mapper(ctx, names, seqs, preset="sr", flag=F_SR | F_FRAG_MODE | (F_EQX if eqx else 0), **ov)


_mapped = {}


@pytest.fixture(scope="module")
def mapped(pkg, gpu_ctx):
    """(kind, eqx) -> (mapper, reads, MapResult of Mapper.map), each mapped once for the module"""
    def get(kind, eqx=True):
        if (kind, eqx) not in _mapped:
            m = sr_mapper(pkg, gpu_ctx, kind, eqx)
            reads = er.reads_of_kind(kind)
            _mapped[(kind, eqx)] = (m, reads, m.map([r[1] for r in reads]))
        return _mapped[(kind, eqx)]
    yield get
    for m, _, _ in _mapped.values():
        m.close()
    _mapped.clear()


@pytest.mark.parametrize("kind", er.KINDS)
def test_whole_path_sam_is_the_reference_s_under_eqx(mapped, kind):
    """gdiet_hip_map_batch + gdiet_hip_sam_batch"""
    m, reads, res = mapped(kind)
    assert m.sam_batch(res, reads) == text(er.eqx_sam(kind))


@pytest.mark.parametrize("kind", er.KINDS)
def test_submit_and_wait_with_two_tickets_open(mapped, kind):
    """gdiet_hip_map_uploaded and gdiet_hip_map_submit / _wait: the read set in two resident batches, both tickets open at once"""
    m, reads, _ = mapped(kind)
    want = er.eqx_sam(kind)
    half = len(reads) // 2
    parts = [reads[:half], reads[half:]]
    names = [{r[0] for r in p} for p in parts]
    wants = [text([l for l in want if l.split("\t")[0] in ns]) for ns in names]
    batches = [m.upload([r[1] for r in p]) for p in parts]
    try:
        assert m.sam_batch(m.map_uploaded(batches[0]), parts[0]) == wants[0]
        m.set_inflight(2)
        ta, tb = m.submit(batches[0]), m.submit(batches[1])
        assert m.sam_batch(m.wait(ta), parts[0]) == wants[0]
        assert m.sam_batch(m.wait(tb), parts[1]) == wants[1]
    finally:
        for b in batches:
            m.free_batch(b)


def test_map_frag_on_the_synthetic_set(mapped):
    """gdiet_hip_map_frag, read by read"""
    m, reads, _ = mapped("syn")
    got = []
    for qn, sq, ql in reads:
        got += m.sam(m.map_frag([sq]), 0, qn, sq, ql)
    assert got == er.eqx_sam("syn")


@pytest.mark.parametrize("kind", er.KINDS)
def test_fan_out_over_the_devices_present(pkg, kind):
    """gdiet_hip_map_batch_multi: one context per device (two contexts on the one device of a single-GPU box)"""
    import torch
    n_dev = torch.cuda.device_count()
    devs = list(range(min(n_dev, 4))) if n_dev > 1 else [0, 0]
    reads = er.reads_of_kind(kind)
    ctxs = [pkg.Context(d) for d in devs]
    ms = [sr_mapper(pkg, c, kind) for c in ctxs]
    try:
        for m in ms:
            m.set_host_threads(max(1, pkg.effective_cpus() // len(ms)))
        res = pkg.map_multi(ms, [r[1] for r in reads])
        assert ms[0].sam_batch(res, reads) == text(er.eqx_sam(kind))
        del res
    finally:
        for m in ms:
            m.close()
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("kind", ["sr", "syn"])
def test_records_carry_the_rewritten_cigar_and_nothing_else_moves(mapped, kind):
    """Reg.cigar holds operations 7 and 8 and no 0, n_cigar is the rewritten length (the fixture's, clips aside); every other field of
    every record is that of the run without the bit"""
    m, reads, res = mapped(kind)
    _, _, plain = mapped(kind, eqx=False)
    rws = {}
    for r in er.rows(kind + ".sam"):
        rws.setdefault(r[0], []).append([x for x in er.parse_cigar(r[3]) if x[0] not in (4, 5)] if r[3] != "*" else None)
    n_rec = n_grown = 0
    for i, (qn, _, _) in enumerate(reads):
        assert res.n_regs[i] == plain.n_regs[i]
        for j in range(res.n_regs[i]):
            a, b = res.regs[i][j], plain.regs[i][j]
            for fld in ("id", "cnt", "rid", "score", "qs", "qe", "rs", "re", "parent", "subsc", "mlen", "blen", "mapq", "rev", "sam_pri", "dp_score", "dp_max", "n_ambi"):
                assert getattr(a, fld) == getattr(b, fld), (qn, j, fld)
            cg = [(a.cigar[k] & 0xf, a.cigar[k] >> 4) for k in range(a.n_cigar)]
            assert cg == rws[qn][j], (qn, j)
            assert all(o in (1, 2, 7, 8) for o, _ in cg) and any(b.cigar[k] & 0xf == 0 for k in range(b.n_cigar))
            assert a.n_cigar >= b.n_cigar
            n_rec += 1
            n_grown += a.n_cigar > b.n_cigar
    assert n_rec == sum(1 for v in rws.values() for c in v if c is not None) and n_grown > 0


@pytest.mark.parametrize("mode", dr.MODES)
@pytest.mark.parametrize("kind", ["sr", "sr_edge"])
def test_difference_tags_under_eqx(mapped, kind, mode):
    """F_EQX with F_OUT_MD / F_OUT_CS / F_OUT_CS_LONG: the --eqx line with the tag of tests/golden/tags/ in front of rl:i:0 (the
    difference-string kernel reads = and X as it reads M)"""
    m, reads, res = mapped(kind)
    flag = m.opt.flag
    m.opt.flag = flag | dr.MODE_FLAG[mode]
    try:
        got = m.sam_batch(res, reads).rstrip("\n").split("\n")
    finally:
        m.opt.flag = flag
    want = []
    for line, tg in zip(er.eqx_sam(kind), dr.tag_rows("%s.%s" % (kind, mode))):
        f = line.split("\t")
        if tg[4]:
            assert f[-1] == "rl:i:0" and not tg[4].startswith("#")
            f.insert(len(f) - 1, ("MD:Z:" if mode == "md" else "cs:Z:") + tg[4])
        want.append("\t".join(f))
    assert got == want and sum(1 for l in got if "\tMD:Z:" in l or "\tcs:Z:" in l) > 0


def test_paf_cg_tag_under_eqx(mapped):
    """gdiet_hip_paf_batch with MM_F_OUT_CG: the mapped lines of the golden PAF with cg:Z: from the fixture (the reference moves no other
    column under --eqx: tools/make_eqx_golden.py)"""
    m, reads, res = mapped("sr")
    want = []
    for line, r in zip(golden_paf("sr"), er.rows("sr.paf")):
        f = line.split("\t")
        if f[4] == "*":  # (a line of --paf-no-hit)
            continue
        at = [i for i, x in enumerate(f) if x.startswith("cg:Z:")]
        assert len(at) == 1 and (f[0], f[2], f[4]) == tuple(r[:3])
        f[at[0]] = "cg:Z:" + r[3]
        want.append("\t".join(f))
    assert m.paf_batch(res, reads, flag=F_CG) == text(want)


@pytest.mark.parametrize("kind", ["sr_edge", "syn"])
def test_without_the_bit_the_sam_text_is_what_it_was(mapped, kind):
    m, reads, res = mapped(kind, eqx=False)
    assert m.sam_batch(res, reads) == text(er.plain_sam(kind))


def test_the_long_read_variant_does_not_interpret_the_bit(pkg, gpu_ctx):
    """a hifi mapper with MM_F_EQX set prints what it prints without it: the golden SAM"""
    base = SETS["hifi_sv"][0]
    names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
    reads = reads_of("hifi_sv")[:40]
    keep = {r[0] for r in reads}
    want = text([l for l in golden_sam("hifi_sv") if l.split("\t")[0] in keep])
    for flag in (0, er.F_EQX):
        m = pkg.Mapper(gpu_ctx, names, seqs, preset="hifi", flag=flag)
        try:
            assert m.sam_batch(m.map([r[1] for r in reads]), reads) == want, flag
        finally:
            m.close()

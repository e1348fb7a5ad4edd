"""The two finer levels of the drop-in boundary on the GPU:
B4 -- gdiet_hip_seed_batch (mm_sketch2 + mm_get_shift, mm_sketch3, mm_seed_mz_flt, mm_collect_matches2, LR/mmpriv.h:65-76) against THE
      REFERENCE's --print-seeds trace (committed as <kind>.trace.gz by oracle/make_golden.py): the pattern phase of every read ("Final
      shift" lines) and -- expanding every kept seed's occurrences as collect_seed_hits does (LR/map.c:861-955) -- its seed hits on both
      strands ("RS" counts and the SD lines, as a multiset; for the repeat-rich sets their count and sha1);
B2 -- gdiet_hip_map_frag (mm_map_frag's call shape, LR/minimap.h:390) against the golden SAM, read by read."""
import os

import pytest

from fixture_io import OVERRIDES, SD_DIGESTED, SETS, assert_seed_batch_matches_trace, golden_sam, read_fasta, reads_of, seed_trace_per_read, trace_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["hifi", "ont", "sr", "hifi_sv", "hifi_rep", "ont_rep", "sr_rep"])
def test_seed_batch_matches_the_reference_trace(gpu_ctx, pkg, kind):
    base, stem, preset = SETS[kind]
    names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
    reads = reads_of(kind)
    want = seed_trace_per_read(trace_of(kind))
    assert len(want) == len(reads)
    m = pkg.Mapper(gpu_ctx, names, seqs, preset=preset, **OVERRIDES.get(kind, {}))
    try:
        got = m.seed_batch([r[1] for r in reads])
    finally:
        m.close()
    n_sd = assert_seed_batch_matches_trace(got, want, names, kind in SD_DIGESTED)
    assert n_sd > 1000


@pytest.mark.parametrize("kind", ["hifi", "sr_edge"])
def test_map_frag_matches_golden_sam(gpu_ctx, pkg, kind):
    base, stem, preset = SETS[kind]
    names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
    reads = reads_of(kind)[:40]
    want = [l for l in golden_sam(kind) if l.split("\t")[0] in {r[0] for r in reads}]
    m = pkg.Mapper(gpu_ctx, names, seqs, preset=preset, **OVERRIDES.get(kind, {}))
    try:
        got = []
        for qn, sq, ql in reads:
            res = m.map_frag([sq])
            got += m.sam(res, 0, qn, sq, ql)
        if len({r[0] for r in reads}) == len(reads):  # (a read name that occurs twice would be counted twice in `want`)
            assert got == want
        res2 = m.map_frag([reads[0][1], reads[1][1]])  # two segments: only segment 0 is mapped, as in the reference
        assert res2.n_regs[1] == 0 and m.sam(res2, 0, *reads[0]) == m.sam(m.map_frag([reads[0][1]]), 0, *reads[0])
    finally:
        m.close()

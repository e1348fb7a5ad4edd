"""A Coverage and a Pileup attached together (csrc/accum_driver.hip.h: one hold over both, one table of record starts, both scatters
behind it) to one BgzfWriter with a context, or to one BamSorter: what they accumulate equals, integer for integer, a fresh Coverage
and a fresh Pileup fed the same records through add_bam -- the bytes Mapper.bam_batch_raw returns for the same batches."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from test_coverage import same as same_cov
from test_coverage_gpu import as_cov, mapped  # noqa: F401  (fixture: the mapped golden reads)
from test_pileup import golden_regions, same as same_pile
from test_pileup_gpu import as_got

pytestmark = pytest.mark.gpu

KIND = "sr"
CALLS = dict(min_depth=2, min_alt=2, frac=(1, 5))
WINDOW = 1000


def cut(pkg, b, lo, hi):
    """reads [lo, hi) of the batch b, as a batch"""
    n = hi - lo
    out = types.SimpleNamespace(n=n, names=(C.c_char_p * n)(*b.names[lo:hi]), seqs=(C.c_char_p * n)(*b.seqs[lo:hi]), quals=(C.c_char_p * n)(*b.quals[lo:hi]),
                                lens=np.array(b.lens[lo:hi], np.int32))
    out.res = types.SimpleNamespace(n_regs=(C.c_int32 * n)(*b.res.n_regs[lo:hi]), regs=(C.POINTER(pkg.map_api.Reg) * n)(*[b.res.regs[i] for i in range(lo, hi)]))
    out.args = lambda: (out.res, out.n, out.names, out.seqs, out.quals, out.lens.ctypes.data_as(C.POINTER(C.c_int32)))
    return out


def batches_of(pkg, batches, which):
    if which == "all":
        return batches
    if which == "empty":
        return [cut(pkg, batches[0], 0, 0)]
    i = next(i for i in range(batches[0].n) if batches[0].res.n_regs[i] > 0)  # one read, a mapped one
    return [cut(pkg, batches[0], i, i + 1)]


def pair(pkg, m):
    lens = [int(x) for x in m.index_info()["lens"]]
    return pkg.Coverage(m, window=WINDOW), pkg.Pileup(m, regions=golden_regions(lens), min_baseq=20)


def said(cov, pile):
    return as_cov(cov), as_got(pile, **CALLS)


def feed(pkg, gpu_ctx, m, route, path, batches, cov, pile):
    """the batches through one writer or one sorter with cov and pile (either may be None) attached; the exception of a refused batch leaves"""
    if route == "writer":
        with pkg.BgzfWriter(path, ctx=gpu_ctx) as w:
            w.set_coverage(cov), w.set_pileup(pile)
            w.write(m.bam_header("v", ["x"]))
            for b in batches:
                w.write_bam(m, *b.args())
    else:
        s = pkg.BamSorter(path, m, tmp_dir=os.path.dirname(path), version="v", argv=["x"])
        try:
            s.set_coverage(cov), s.set_pileup(pile)
            for b in batches:
                s.add(*b.args())
        finally:
            try:
                s.close()
            except pkg.GdietError:
                pass  # (a sorter whose add was refused says so again at close)


@pytest.fixture(scope="module")
def fresh(pkg, mapped):  # noqa: F811
    """which -> what a fresh Coverage and a fresh Pileup say after add_bam of bam_batch_raw's bytes: once per set of batches"""
    cache = {}

    def get(which):
        if which not in cache:
            m, batches = mapped(KIND)
            cov, pile = pair(pkg, m)
            with cov, pile:
                for b in batches_of(pkg, batches, which):
                    data = m.bam_batch_raw(*b.args())
                    cov.add_bam(data), pile.add_bam(data)
                cache[which] = said(cov, pile)
        return cache[which]
    return get


@pytest.mark.parametrize("which", ["all", "empty", "one"])
@pytest.mark.parametrize("route", ["writer", "sorter"])
def test_both_attached_equal_fresh_pair(route, which, mapped, fresh, pkg, gpu_ctx, tmp_path):  # noqa: F811
    m, batches = mapped(KIND)
    want_cov, want_pile = fresh(which)
    assert (want_cov.summary["counted"] > 0) == (which != "empty") and want_pile.summary["records"] == want_cov.summary["records"]
    cov, pile = pair(pkg, m)
    with cov, pile:
        feed(pkg, gpu_ctx, m, route, str(tmp_path / "out.bam"), batches_of(pkg, batches, which), cov, pile)
        got_cov, got_pile = said(cov, pile)
    same_cov(got_cov, want_cov, (route, which))
    same_pile(got_pile, want_pile, (route, which))


@pytest.mark.parametrize("route", ["writer", "sorter"])
def test_finished_pileup_beside_live_coverage(route, mapped, fresh, pkg, gpu_ctx, tmp_path):  # noqa: F811
    """the pileup of the set is finished: the call is refused with its text before anything is encoded, and the coverage accumulator
    beside it is neither fed nor poisoned -- the same batches through a holder without the pileup give it the fresh pair's integers"""
    m, batches = mapped(KIND)
    cov, pile = pair(pkg, m)
    with cov, pile:
        pile.finish()
        with pytest.raises(pkg.GdietError, match="pileup: finished, the accumulator is read-only"):
            feed(pkg, gpu_ctx, m, route, str(tmp_path / "refused.bam"), batches, cov, pile)
        feed(pkg, gpu_ctx, m, route, str(tmp_path / "out.bam"), batches, cov, None)
        same_cov(as_cov(cov), fresh("all")[0], route)

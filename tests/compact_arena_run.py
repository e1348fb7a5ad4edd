"""run by tests/test_compact_arena_gpu.py in a process of its own, with GDIET_BT_COMPACT / GDIET_BT_OVERFLOW_MB in the environment (the
library reads them once, when it is loaded).
    python compact_arena_run.py pairs <mix|fallback24> <out.npz>   aligns the batch at w = 1000 with HiFi scoring through
        gdiet_hip_ksw_extd2_batch and writes scores, CIGARs, the ladder's counters and gdiet_hip_last_arena; the caller compares
    python compact_arena_run.py inflight <kind>   maps the kind's reads as two batches in flight (submit, submit, wait, wait) and compares
        every SAM record with the golden SAM"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from narrow_pairs import W_NARROW, long_indels, tandem  # noqa: E402
from quarter_pairs import bench_like_read  # noqa: E402


def fallback_pairs():
    """the twelve pairs of test_paths_outside_the_narrow_band_fall_back_to_the_full_band (tests/test_narrow_band_gpu.py): about 4 kbp,
    the true path more than 495 off the diagonal in between"""
    rng = np.random.default_rng(77)
    pairs = []
    for k in range(6):
        pairs.append(long_indels(rng, 4000 + 16 * k + k, [600, -600] if k & 1 else [-600, 600]))
    for k in range(6):
        period = int(rng.integers(W_NARROW // 2 + 10, 400))
        q, t = tandem(rng, 4000 + 7 * k, period, 3, 5)
        cut = len(q) - 500 - 2 * period
        q = np.ascontiguousarray(np.concatenate([q[:cut], q[cut + 2 * period:]]))
        pairs.append((q, t))
    return pairs


def mix_pairs():
    """reads drawn by the benchmark's error rates at about 4 kbp (they certify at 239), twelve pairs with a 300-base insertion and a
    300-base deletion further on (only at 495), the twelve fall-back pairs -- interleaved, so that the claims come from all over the grid.
    420 of the first kind, not a few dozen: the default pool is a sixteenth of the slots, a slot is half of a box's full-band rows, so
    twelve fall-backs find room in it only among at least 12 x 32 = 384 boxes of their size"""
    rng = np.random.default_rng(20261019)
    easy = [bench_like_read(rng, mean=4000, sd=300, lo=3200, hi=4800) for _ in range(420)]
    mid = [long_indels(rng, 4000 + 16 * k + k, [300 + k, -300] if k & 1 else [-300 - k, 300]) for k in range(12)]
    hard = fallback_pairs()
    out = []
    for k in range(12):
        out += easy[3 * k:3 * k + 3] + [mid[k], hard[k]]
    return out + easy[36:]


def pairs_of(which):
    return mix_pairs() if which == "mix" else fallback_pairs() * 2


def main():
    import torch  # noqa: F401  (first: one HIP runtime)
    from conftest import load_pkg
    pkg = load_pkg()
    ctx = pkg.Context(0)
    if sys.argv[1] == "pairs":
        pairs = pairs_of(sys.argv[2])
        sc, cg = ctx.ksw_extd2_batch([p[0] for p in pairs], [p[1] for p in pairs], 1000, pkg.KswScore.from_preset("hifi"))
        band, rungs, arena = ctx.last_narrow_band(), ctx.last_narrow_rungs(), ctx.last_arena()
        np.savez(sys.argv[3], score=np.asarray(sc, np.int64), cigar=np.concatenate([np.asarray(c, np.uint32) for c in cg]),
                 n_cigar=np.array([len(c) for c in cg], np.int64), band=np.array(band, np.int64), rungs=np.array(rungs, np.int64), arena=np.array(arena, np.int64))
    else:
        from fixture_io import OVERRIDES, SETS, golden_sam, read_fasta, reads_of
        kind = sys.argv[2]
        base, stem, preset = SETS[kind]
        names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
        reads = reads_of(kind)
        m = pkg.Mapper(ctx, names, seqs, preset=preset, **OVERRIDES.get(kind, {}))
        m.set_inflight(2)
        halves = [reads[:len(reads) // 2], reads[len(reads) // 2:]]
        batches = [m.upload([r[1] for r in h]) for h in halves]
        tickets = [m.submit(b) for b in batches]
        got = "".join(m.sam_batch(m.wait(t), h) for t, h in zip(tickets, halves))
        print("pool claims, drained, arena bytes of the second batch:", ctx.last_arena())  # (the call also reports a box left without rows)
        for b in batches:
            m.free_batch(b)
        want = "".join(l + "\n" for l in golden_sam(kind))
        if got != want:
            g, w = got.split("\n"), want.split("\n")
            bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
            print("DIFF", kind, len(g), len(w), bad[:3])
            sys.exit(1)
        m.close()
    ctx.close()
    print("ok")


if __name__ == "__main__":
    main()

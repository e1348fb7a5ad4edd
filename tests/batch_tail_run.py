"""run by tests/test_batch_tail_gpu.py in a process of its own, with GDIET_BT_OVERFLOW_MB in the environment (the library reads it once,
when it is loaded).
    python batch_tail_run.py pairs <mix|fallback24> <host|dev> <out.npz>   aligns the batch at w = 1000 with HiFi scoring -- host:
        gdiet_hip_ksw_extd2_batch, which waits for its stream and decides on the drain launches when the main launch has ended; dev:
        gdiet_hip_ksw_extd2_batch_dev on a stream of the caller's, which never waits -- and writes scores, CIGARs, gdiet_hip_last_arena
        and gdiet_hip_last_drain_launches
    python batch_tail_run.py inflight <kind>   maps the kind's reads as two batches in flight (submit, submit, wait, wait), compares every
        SAM record with the golden SAM and prints what the two batches drained"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from compact_arena_run import pairs_of  # noqa: E402


def align_dev(pkg, ctx, pairs):
    import torch
    qs, ts = [p[0] for p in pairs], [p[1] for p in pairs]
    qbuf, qoff = pkg.pack(qs)
    tbuf, toff = pkg.pack(ts)
    coff = np.zeros(len(qs) + 1, np.int64)
    coff[1:] = np.cumsum([len(q) + len(t) for q, t in zip(qs, ts)])
    dev = torch.device("cuda", 0)
    d_q, d_t, d_coff = torch.from_numpy(qbuf).to(dev), torch.from_numpy(tbuf).to(dev), torch.from_numpy(coff).to(dev)
    d_sc = torch.zeros(len(qs), dtype=torch.int32, device=dev)
    d_nc = torch.zeros(len(qs), dtype=torch.int32, device=dev)
    d_cg = torch.zeros(int(coff[-1]) + 1, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        ctx.ksw_extd2_batch_dev(len(qs), d_q.data_ptr(), d_t.data_ptr(), None, pkg.KswScore.from_preset("hifi"), d_sc.data_ptr(), d_nc.data_ptr(),
                                d_cg.data_ptr(), d_coff.data_ptr(), qoff, toff, np.full(len(qs), 1000, np.int32), stream=st.cuda_stream)
    st.synchronize()
    sc, nc, cg = d_sc.cpu().numpy(), d_nc.cpu().numpy(), d_cg.cpu().numpy().view(np.uint32)
    return sc, [cg[coff[i]:coff[i] + nc[i]] for i in range(len(qs))]


def main():
    import torch  # noqa: F401  (first: one HIP runtime)
    from conftest import load_pkg
    pkg = load_pkg()
    ctx = pkg.Context(0)
    if sys.argv[1] == "pairs":
        pairs = pairs_of(sys.argv[2])
        if sys.argv[3] == "host":
            sc, cg = ctx.ksw_extd2_batch([p[0] for p in pairs], [p[1] for p in pairs], 1000, pkg.KswScore.from_preset("hifi"))
        else:
            sc, cg = align_dev(pkg, ctx, pairs)
        band, rungs, arena, launches = ctx.last_narrow_band(), ctx.last_narrow_rungs(), ctx.last_arena(), ctx.last_drain_launches()
        np.savez(sys.argv[4], score=np.asarray(sc, np.int64), cigar=np.concatenate([np.asarray(c, np.uint32) for c in cg]),
                 n_cigar=np.array([len(c) for c in cg], np.int64), band=np.array(band, np.int64), rungs=np.array(rungs, np.int64),
                 arena=np.array(arena, np.int64), launches=np.array(launches, np.int64))
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
        got, drained, launches = "", 0, 0
        for t, h in zip(tickets, halves):
            got += m.sam_batch(m.wait(t), h)
            drained += ctx.last_arena()[1]  # (the lane's counters of this batch, copied to the context by the wait)
            launches += ctx.last_drain_launches()
        print("IN_FLIGHT drained %d launches %d" % (drained, launches))
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

#!/usr/bin/env python3
"""The shader clock the 64-lane DP kernel sustains (GPU box only):  python tools/clock_probe.py [n_pairs] [len]

Every wavefront of ksw_extd2_wave_kernel<64> stamps s_memtime and s_memrealtime around its DP rows (gdiet_hip_last_dp_clock reduces them;
this tool reads the raw table through a measurement build, build_ab/libgdiet_clk.so = the library with -DGD_CLOCK_STAMP, which exports it).
s_memrealtime ticks at the constant 100 MHz reference (tools/clock_probe.hip checks that against HIP events), so per wavefront
    sclk = (s_memtime ticks / s_memrealtime ticks) x 100 MHz
and, with the instruction counts of the kernel (PMC: profiles/r02_pmc_valu.json), cycles per VALU instruction follow."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "build_ab", "libgdiet_clk.so")

if "--build" in sys.argv:
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread", "-mllvm", "-amdgpu-sched-strategy=max-ilp",
                           "-DGD_CLOCK_STAMP", "-o", LIB, os.path.join(ROOT, "genome-on-diet_amd", "csrc", "gdiet_hip.hip"), "-lz"])
    print(LIB)
    sys.exit(0)

os.environ["GDIET_HIP_LIB"] = LIB
import numpy as np  # noqa: E402
import torch  # noqa: F401,E402

sys.path.insert(0, ROOT)
from __graft_entry__ import _load_pkg  # noqa: E402

pkg = _load_pkg()


def occupancy(out_path):
    """--occupancy [out.json]: resident DP wavefronts over time of ONE launch of a bench batch (bench.py's reference and first 5 120 reads, one
    batch in flight), from the per-box s_memrealtime stamps around the DP rows (the walk that follows them, 0.5 ms per launch in all, is not
    inside).  Share of slot-time that is empty between the first start and the last end = 1 - sum(box durations) / (slots x span)."""
    import bench
    names, contigs = bench.synth_reference(float(os.environ.get("GDIET_BENCH_REF_MBP", "3088")), seed=2)
    reads = bench.synth_hifi_reads(np.random.default_rng(pkg.rank_seed(5, 0)), contigs, 5120)
    ctx = pkg.Context(0)
    cores = pkg.effective_cpus()
    mapper = pkg.Mapper(ctx, names, contigs, preset="hifi", n_threads=cores)
    mapper.set_host_threads(cores)
    batch = mapper.upload([s for _, s in reads])
    lib = pkg.load_library()
    lib.gdiet_hip_debug_clock_stamps.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    slots = 5120
    res = {}
    for rep in range(3):
        mapper.map_uploaded(batch)
        dp_ms, _ = ctx.last_kernel_ms()
        n = 16384
        buf = (C.c_ulonglong * (4 * n))()
        got = lib.gdiet_hip_debug_clock_stamps(buf, n)
        st = np.frombuffer(buf, np.uint64).reshape(-1, 4)[:got].astype(np.float64)
        t0, t1 = st[:, 1], st[:, 3]
        ok = t1 > t0
        ok &= t0 > t1[ok].max() - (dp_ms + 5.0) * 1e5  # this launch's boxes only: the table keeps the stamps of the launch before in unused entries
        t0, t1 = (t0[ok] - t0[ok].min()) * 1e-5, (t1[ok] - t0[ok].min()) * 1e-5  # ms
        span = float(t1.max())
        ev = np.concatenate([np.stack([t0, np.ones_like(t0)], 1), np.stack([t1, -np.ones_like(t1)], 1)])
        ev = ev[np.argsort(ev[:, 0], kind="mergesort")]
        resident = np.cumsum(ev[:, 1])
        grid = np.linspace(0, span, 41)
        curve = [int(resident[max(0, np.searchsorted(ev[:, 0], g, side="right") - 1)]) for g in grid]
        full_until = float(ev[np.nonzero(resident >= slots - 8)[0][-1], 0]) if (resident >= slots - 8).any() else 0.0
        below = lambda k: float(span - ev[np.nonzero(resident >= k)[0][-1], 0])  # ms at the end with fewer than k resident  # noqa: E731
        res = {"boxes": int(ok.sum()), "slots": slots, "kernel_ms_events": dp_ms, "span_ms": span, "box_ms_sum": float((t1 - t0).sum()),
               "empty_share": 1.0 - float((t1 - t0).sum()) / (slots * span), "full_until_ms": full_until,
               "tail_ms_below_4096": below(4096), "tail_ms_below_2048": below(2048), "tail_ms_below_1024": below(1024), "tail_ms_below_256": below(256),
               "box_ms_max": float((t1 - t0).max()), "box_ms_median": float(np.median(t1 - t0)),
               "curve_t_ms": [round(float(g), 2) for g in grid], "curve_resident": curve}
        print(json.dumps(res))
    if hasattr(ctx, "last_arena"):
        # the compact arena's counters over the bench's batches (--batches K: the first K of bench.py's 40, this one included)
        k = int(sys.argv[sys.argv.index("--batches") + 1]) if "--batches" in sys.argv else 1
        rng = np.random.default_rng(pkg.rank_seed(5, 0))
        tot, arenas = [0, 0], []
        for b in range(k):
            rb = bench.synth_hifi_reads(rng, contigs, 5120, first=b * 5120)
            if b:
                mapper.free_batch(batch)
                batch = mapper.upload([s for _, s in rb])
                mapper.map_uploaded(batch)
            a = ctx.last_arena()
            tot[0] += a[0]
            tot[1] += a[1]
            arenas.append(a[2])
        res.update({"batches": k, "pool_claims": tot[0], "drained": tot[1], "arena_bytes_min": min(arenas), "arena_bytes_max": max(arenas), "narrow_rungs_last": list(ctx.last_narrow_rungs())})
        print(json.dumps({k_: v for k_, v in res.items() if not k_.startswith("curve")}))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f)
    mapper.close()
    ctx.close()


if "--occupancy" in sys.argv:
    rest = [a for a in sys.argv[1:] if not a.startswith("--")]
    occupancy(rest[0] if rest else None)
    sys.exit(0)
args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 9400
ln = int(args[1]) if len(args) > 1 else 15000
w = 1000
rng = np.random.default_rng(1)
qs, ts = [], []
for i in range(n):
    L = int(np.clip(rng.normal(ln, ln * 0.13), ln // 3, ln * 5 // 3))
    t = rng.integers(0, 4, size=L, dtype=np.uint8)
    pos = np.sort(rng.choice(L, size=max(1, L // 300), replace=False))
    q = t.copy()
    q[pos] = (q[pos] + 1) & 3
    q = np.delete(q, pos[::4])
    qs.append(q), ts.append(t)
cells = sum((len(q) + len(t) - 1) * min(w + 1, len(q), len(t)) for q, t in zip(qs, ts))
ctx = pkg.Context(0)
ctx.set_kernel_mode(0)
lib = pkg.load_library()
lib.gdiet_hip_debug_clock_stamps.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
out = {}
for rep in range(3):
    sc, cg = ctx.ksw_extd2_batch(qs, ts, w, pkg.KswScore.from_preset("hifi"))
    dp_ms, _ = ctx.last_kernel_ms()
    buf = (C.c_ulonglong * (4 * n))()
    got = lib.gdiet_hip_debug_clock_stamps(buf, n)
    st = np.frombuffer(buf, np.uint64).reshape(-1, 4)[:got].astype(np.float64)
    mt, rt = st[:, 2] - st[:, 0], st[:, 3] - st[:, 1]
    ok = rt > 0
    f = mt[ok] / rt[ok] * 100.0
    span_ms = (st[ok, 3].max() - st[ok, 1].min()) * 1e-5
    # instructions per cell of this kernel, from the committed PMC summary
    valu_per_cell = None
    for name in ("r03_pmc_valu.json", "r02_pmc_valu.json"):
        p = os.path.join(ROOT, "profiles", name)
        if os.path.exists(p):
            valu_per_cell = json.load(open(p)).get("valu_insts_per_cell")
            break
    out = {"pairs": n, "mean_len": ln, "dp_cells": int(cells), "kernel_ms_events": dp_ms, "kernel_ms_by_s_memrealtime": span_ms, "wavefronts_stamped": int(ok.sum()),
           "sclk_mhz_min": float(f.min()), "sclk_mhz_p10": float(np.percentile(f, 10)), "sclk_mhz_median": float(np.median(f)), "sclk_mhz_p90": float(np.percentile(f, 90)),
           "sclk_mhz_max": float(f.max()), "wavefront_ms_median": float(np.median(rt[ok]) * 1e-5)}
    if valu_per_cell:
        insts_per_simd = valu_per_cell * cells / 1024.0
        out["valu_insts_per_cell_pmc"] = valu_per_cell
        out["ns_per_valu_inst_per_simd"] = dp_ms * 1e6 / insts_per_simd
        out["sclk_cycles_per_valu_inst"] = dp_ms * 1e-3 * out["sclk_mhz_median"] * 1e6 / insts_per_simd
    print(json.dumps(out))
ctx.close()

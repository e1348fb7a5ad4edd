#!/usr/bin/env python3
"""The tail of every HiFi batch in a rocprofv3 kernel trace: what passes between the end of a batch's main DP launch and its results.

usage: batch_tail.py TRACE_DIR [--json OUT.json]
TRACE_DIR holds the *_kernel_trace.csv of one
    rocprofv3 --kernel-trace --stats --output-format csv -d TRACE_DIR -- python3 bench.py --gpus 1 --steps 20 --warmup 5
run (a run of its own, no counters).

A batch's DP stage is a chain on one stream: ksw_exact_match_kernel, the main launch of ksw_extd2_wave_kernel<64, 0, true>, its drain
launches (the same kernel again, if any were enqueued), ksw_backtrack_wave_kernel, map_fix_cigar_kernel (builds that still have it
as a kernel of its own), map_post_wave_kernel and the runtime's copy kernels, where the copies are kernels; map_pack_cigar_kernel follows on the lane's other stream once the host has summed the CIGAR lengths.  The trace
has no enqueue time, so "queued" is the end of the kernel before it on the same stream: from then on nothing but a free wavefront slot
(or, where the host decides in between, the host) keeps the kernel from starting.  Every figure is in ms, per batch, relative to the
end of the main launch unless it says otherwise; printed as mean / median / max over the batches."""
import csv
import glob
import json
import os
import statistics
import sys

MAIN = "ksw_extd2_wave_kernel<64, 0, true>"


def load(trace_dir):
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*_kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            stream = r.get("Stream_Id") or "0"
            key = (r.get("Agent_Id", ""), stream if stream not in ("", "0") else "q" + r.get("Queue_Id", ""))
            rows.append(dict(name=r["Kernel_Name"], t0=int(r["Start_Timestamp"]), t1=int(r["End_Timestamp"]), key=key))
    rows.sort(key=lambda r: r["t0"])
    return rows


def short(name):
    for k in ("ksw_exact_match_kernel", "ksw_backtrack_wave_kernel", "map_fix_cigar_kernel", "map_post_wave_kernel", "map_pack_cigar_kernel",
              "map_seed_wave_kernel", "map_vote_wave_kernel"):
        if k in name:
            return k
    if MAIN in name or "ksw_extd2_wave_kernelILi64ELi0ELb1E" in name:
        return "main"
    if "copy" in name.lower():
        return "copy"
    return name


def batches(rows):
    """one dict per batch: the kernels of its DP chain, in stream order"""
    by_stream = {}
    for r in rows:
        by_stream.setdefault(r["key"], []).append(r)
    out = []
    for chain in by_stream.values():
        cur = None
        for i, r in enumerate(chain):
            k = short(r["name"])
            r = dict(r, queued=chain[i - 1]["t1"] if i else r["t0"])
            if k == "ksw_exact_match_kernel":
                cur = dict(main=None, drains=[], copies=[])
                out.append(cur)
            elif cur is None:
                continue
            elif k == "main":
                if cur["main"] is None:
                    cur["main"] = r
                elif "ksw_backtrack_wave_kernel" not in cur:
                    cur["drains"].append(r)
            elif k in ("ksw_backtrack_wave_kernel", "map_fix_cigar_kernel", "map_post_wave_kernel") and k not in cur:
                cur[k] = r
            elif k == "copy" and "map_post_wave_kernel" in cur:
                cur["copies"].append(r)
    out = [b for b in out if b["main"] is not None and "map_post_wave_kernel" in b]
    out.sort(key=lambda b: b["main"]["t1"])
    packs = [r for r in rows if short(r["name"]) == "map_pack_cigar_kernel"]
    for b in out:  # the first pack kernel not yet taken that starts behind this batch's post-processing
        for p in packs:
            if not p.get("taken") and p["t0"] >= b["map_post_wave_kernel"]["t1"]:
                p["taken"] = True
                b["map_pack_cigar_kernel"] = p
                break
    return out


def stat(v):
    v = [x / 1e6 for x in v]
    return dict(n=len(v), mean=statistics.mean(v), median=statistics.median(v), max=max(v)) if v else dict(n=0)


def summarise(rows):
    B = batches(rows)
    res = {"batches": len(B), "drain_launches": sum(len(b["drains"]) for b in B), "batches_with_drain_launches": sum(1 for b in B if b["drains"])}
    iv = {}

    def add(name, val):
        iv.setdefault(name, []).append(val)
    for b in B:
        e = b["main"]["t1"]
        add("main launch, duration", b["main"]["t1"] - b["main"]["t0"])
        for k, d in enumerate(b["drains"]):
            add("-> end of drain launch %d" % (k + 1), d["t1"] - e)
        for k in ("ksw_backtrack_wave_kernel", "map_fix_cigar_kernel", "map_post_wave_kernel", "map_pack_cigar_kernel"):
            if k in b:
                add("-> %s starts" % k, b[k]["t0"] - e)
                add("-> %s ends" % k, b[k]["t1"] - e)
                if k != "map_pack_cigar_kernel":
                    add("%s: queued -> start" % k, b[k]["t0"] - b[k]["queued"])
                    add("%s: start -> end" % k, b[k]["t1"] - b[k]["t0"])
        first = b["drains"][0] if b["drains"] else b.get("ksw_backtrack_wave_kernel")
        if first:
            add("first kernel behind the main launch: queued -> start", first["t0"] - first["queued"])
        if b["copies"]:
            add("-> last copy kernel ends", b["copies"][-1]["t1"] - e)
    res["intervals_ms"] = {k: stat(v) for k, v in iv.items()}
    mains = sorted((b["main"] for b in B), key=lambda r: r["t0"])
    ov = [a["t1"] - b["t0"] for a, b in zip(mains, mains[1:]) if b["t0"] < a["t1"]]
    res["consecutive_main_launches"] = len(mains) - 1 if mains else 0
    res["of_them_overlapping"] = len(ov)
    res["overlap_ms"] = stat(ov)
    # the seed and vote kernels wait for a retiring DP wavefront as well (67 and 46 VGPRs): queued -> start, for a later change
    by_stream = {}
    for r in rows:
        by_stream.setdefault(r["key"], []).append(r)
    for k in ("map_seed_wave_kernel", "map_vote_wave_kernel"):
        w = [c[i]["t0"] - c[i - 1]["t1"] for c in by_stream.values() for i in range(1, len(c)) if short(c[i]["name"]) == k]
        res[k + ": queued -> start, ms"] = stat(w)
        res[k + ": start -> end, ms"] = stat([r["t1"] - r["t0"] for r in rows if short(r["name"]) == k])
    return res


def main():
    args = sys.argv[1:]
    out = None
    if "--json" in args:
        i = args.index("--json")
        out = args[i + 1]
        del args[i:i + 2]
    res = summarise(load(args[0]))
    if out:
        json.dump(res, open(out, "w"), indent=1)
    print("batches %d, drain launches %d (in %d batches)" % (res["batches"], res["drain_launches"], res["batches_with_drain_launches"]))
    print("consecutive main launches that overlap: %d of %d" % (res["of_them_overlapping"], res["consecutive_main_launches"]), res["overlap_ms"])
    print("| interval | n | mean | median | max |\n|---|---|---|---|---|")
    for k, s in res["intervals_ms"].items():
        if s["n"]:
            print("| %s | %d | %.2f | %.2f | %.2f |" % (k, s["n"], s["mean"], s["median"], s["max"]))
    for k, s in res.items():
        if k.startswith("map_"):
            print(k, s)


if __name__ == "__main__":
    main()

"""BgzfWriter on about 100 MB of SAM text (the golden short-read SAM repeated 120 times, 1543 members) to a file in /dev/shm: the device
route against zlib on 4 host threads at level 1 and 6 and against a plain write, three rounds; one JSON line per run with seconds, MB/s,
file size and the device's own H2D / kernel / D2H seconds (HIP events).  The text alone: no mapping runs beside it.

    python tools/bench_bgzf_out.py [--dir /dev/shm] [--repeat 120] [--rounds 3]"""
import argparse
import gzip
import json
import os
import sys
import time

import torch  # noqa: F401  (first: one HIP runtime for torch and libgdiet_hip.so)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import _load_pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--repeat", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    pkg = _load_pkg()
    ctx = pkg.Context(0)
    with gzip.open(os.path.join(ROOT, "tests", "golden", "sr", "sr.golden.sam.gz")) as f:
        data = f.read() * a.repeat
    for rnd in range(a.rounds):
        for route in ("device", "host1", "host6", "plain"):
            path = os.path.join(a.dir, "gd_bgzf_out_bench.%s" % route)
            s0, t0 = ctx.bgzf_deflate_seconds(), time.perf_counter()
            if route == "plain":
                with open(path, "wb") as f:
                    f.write(data)
                st = {}
            else:
                with pkg.BgzfWriter(path, ctx=ctx if route == "device" else None, level={"host1": 1, "host6": 6}.get(route, -1), threads=4) as w:
                    w.write(data)
                st = w.stats()
            dt = time.perf_counter() - t0
            print(json.dumps({"round": rnd, "route": route, "bytes_in": len(data), "seconds": round(dt, 4), "MB_per_s": round(len(data) / dt / 1e6, 1),
                              "file_bytes": os.path.getsize(path), "device_seconds_h2d_kernel_d2h": [round(y - x, 4) for x, y in zip(s0, ctx.bgzf_deflate_seconds())], **st}), flush=True)
            os.remove(path)
    ctx.close()


if __name__ == "__main__":
    main()

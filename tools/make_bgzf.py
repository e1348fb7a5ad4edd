#!/usr/bin/env python3
"""Plain or gzip file in, BGZF out: the writer of tests/bgzf_inputs.py behind a command line, for the files of measurements.

    python tools/make_bgzf.py reads.fq reads.fq.gz [--level 6] [--member-bytes 65280] [--workers 8]

Every member holds --member-bytes input bytes (the last one what is left) and the file ends with the 28-byte end-of-file member, so any
gzip tool reads it and the reader of this library takes its BGZF route.  Members are compressed by up to 16 worker processes."""
import argparse
import gzip
import multiprocessing
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import bgzf_inputs  # noqa: E402

GROUP = 256  # members per task


def _pack(task):
    data, member_bytes, level = task
    return b"".join(bgzf_inputs.members_of(data, member_bytes, level))


def _tasks(f, member_bytes, level):
    while True:
        data = f.read(member_bytes * GROUP)
        if not data:
            return
        yield data, member_bytes, level


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--level", type=int, default=6, choices=range(0, 10))
    ap.add_argument("--member-bytes", type=int, default=bgzf_inputs.MAX_MEMBER_BYTES)
    ap.add_argument("--workers", type=int, default=8)
    a = ap.parse_args()
    if not 1 <= a.member_bytes <= bgzf_inputs.MAX_MEMBER_BYTES:
        ap.error("--member-bytes must be 1 .. %d" % bgzf_inputs.MAX_MEMBER_BYTES)
    workers = max(1, min(16, a.workers))
    with open(a.src, "rb") as probe:
        gz = probe.read(2) == b"\x1f\x8b"
    n_in = n_out = 0
    with (gzip.open(a.src, "rb") if gz else open(a.src, "rb")) as f, open(a.dst, "wb") as out:
        if workers == 1:
            chunks = map(_pack, _tasks(f, a.member_bytes, a.level))
            pool = None
        else:
            pool = multiprocessing.Pool(workers)
            chunks = pool.imap(_pack, _tasks(f, a.member_bytes, a.level))
        for c in chunks:
            out.write(c)
            n_out += len(c)
        out.write(bgzf_inputs.EOF_MARKER)
        n_out += len(bgzf_inputs.EOF_MARKER)
        n_in = f.tell()
        if pool is not None:
            pool.close()
            pool.join()
    print("%s: %d bytes -> %s: %d bytes, members of %d input bytes at level %d" % (a.src, n_in, a.dst, n_out, a.member_bytes, a.level))


if __name__ == "__main__":
    main()

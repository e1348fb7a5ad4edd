#!/usr/bin/env python3
"""reads with a few Ns inside: the first N_READS reads of a committed read set with 1 to 3 bases each replaced by N, at positions drawn
from SEED and at least MARGIN bases away from both ends (so that the Ns lie inside the alignment, where the DP scores them as -e2).
    synth_n.py SEED N_READS in.fq[.gz] out.fq
tests/golden/lr/hifi_n.fq.gz = synth_n.py 21 12 tests/golden/lr/hifi.fq.gz; tests/golden/sr/sr_n.fq.gz = synth_n.py 22 200 tests/golden/sr/sr.fq.gz"""
import gzip
import sys

import numpy as np

MARGIN = 25

seed, n_reads, src, dst = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
rng = np.random.default_rng(seed)
lines = [l.rstrip("\n") for l in (gzip.open if src.endswith(".gz") else open)(src, "rt")]
with open(dst, "w") as out:
    for i in range(0, 4 * n_reads, 4):
        name, seq, qual = lines[i][1:].split()[0], list(lines[i + 1]), lines[i + 3]
        for p in rng.choice(np.arange(MARGIN, len(seq) - MARGIN), size=int(rng.integers(1, 4)), replace=False):
            seq[int(p)] = "N"
        out.write("@%s_n\n%s\n+\n%s\n" % (name, "".join(seq), qual))

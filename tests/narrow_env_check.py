"""run by tests/test_narrow_band_gpu.py in a process of its own with GDIET_NARROW_BAND=0 (read once per context): a few pairs at
w = 1000 must then not try the narrow band at all, and still give the oracle's alignments."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import torch  # noqa: F401,E402  (first: one HIP runtime)
import gdo  # noqa: E402
from conftest import load_pkg  # noqa: E402
from narrow_pairs import hifi_like  # noqa: E402

pkg = load_pkg()
lib = gdo.load_oracle()
ctx = pkg.Context(0)
rng = np.random.default_rng(5)
pairs = [hifi_like(rng, n, 0.01) for n in (700, 1500, 2100, 3000)]
a, b, q, e, q2, e2 = gdo.PRESETS["hifi"]
sc, cg = ctx.ksw_extd2_batch([p[0] for p in pairs], [p[1] for p in pairs], 1000, pkg.KswScore.from_preset("hifi"))
tried, cert = ctx.last_narrow_band()
for i, (qq, tt) in enumerate(pairs):
    o = gdo.oracle_extd2(lib, qq, tt, gdo.score_matrix(a, b), q, e, q2, e2, 1000)
    assert sc[i] == o["score"] and np.array_equal(cg[i], o["cigar"]), i
assert (tried, cert) == (0, 0), (tried, cert)
ctx.close()
print("ok")

"""run by a GPU test in a process of its own (GDIET_GROUP_LANES / GDIET_SR_PIPE / GDIET_DIAG_SHORTCUT are read once per process):
every pair of tests/golden/ksw2_scoring.npz through gdiet_hip_ksw_extd2_batch at its scoring (default dispatch, an exact_score column
at the scoring's match score), against the reference's outputs; prints one line per scoring and "ok" at the end."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401,E402  (first: one HIP runtime)
from conftest import load_pkg  # noqa: E402
from golden_io import load_scoring  # noqa: E402

pkg = load_pkg()
ctx = pkg.Context(0)
by = {}
for c in load_scoring():
    by.setdefault(c["scoring"], []).append(c)
bad = 0
for name, cs in by.items():
    a, b, q, e, q2, e2, amb = cs[0]["sc"]
    ex = np.array([len(c["q"]) * a if len(c["q"]) == len(c["t"]) else pkg.hip_abi.NEG_INF for c in cs], np.int32)
    s, cg = ctx.ksw_extd2_batch([c["q"] for c in cs], [c["t"] for c in cs], [c["w"] for c in cs],
                                pkg.KswScore(a, -b, amb, q, e, q2, e2, 0, pkg.hip_abi.EZ_APPROX_MAX), exact_score=ex)
    for i, c in enumerate(cs):
        if len(c["q"]) == len(c["t"]) and np.array_equal(c["q"], c["t"]):
            ok = s[i] == ex[i] and list(cg[i]) == [len(c["q"]) << 4]
        else:
            ok = s[i] == c["extd2"]["score"] and np.array_equal(cg[i], c["extd2"]["cigar"])
        if not ok:
            bad += 1
            print("DIFFERS", name, c["cls"], i, len(c["q"]), len(c["t"]), c["w"], s[i], c["extd2"]["score"])
    print(name, len(cs), "mask", ctx.last_kernel_mask())
ctx.close()
print("ok" if bad == 0 else "%d differ" % bad)
sys.exit(1 if bad else 0)

"""run by tests/test_option_grid_gpu.py in a process of its own, with switches of the library in the environment (they are read once
per process): maps the rows of the option grid named on the command line and compares every SAM record (SEQ / QUAL starred) with the
row's golden SAM.  python grid_env_check.py row..."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401,E402  (first: one HIP runtime)
from conftest import load_pkg  # noqa: E402
from fixture_io import grid_golden_sam, grid_mapper_args, grid_reads, grid_row, read_fasta, star_seq_qual  # noqa: E402

pkg = load_pkg()
ctx = pkg.Context(0)
for name in sys.argv[1:]:
    row = grid_row(name)
    base, preset, ov = grid_mapper_args(row)
    names, seqs = read_fasta(os.path.join(base, "ref.fa.gz"))
    reads = grid_reads(row)
    m = pkg.Mapper(ctx, names, seqs, preset=preset, **ov)
    g = [star_seq_qual(l) for l in m.sam_batch(m.map([r[1] for r in reads]), reads).rstrip("\n").split("\n")]
    w = grid_golden_sam(row)
    if g != w:
        bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
        print("DIFF", name, len(g), len(w), bad[:3], (g[bad[0]][:300], w[bad[0]][:300]) if bad else "")
        sys.exit(1)
    m.close()
ctx.close()
print("ok")

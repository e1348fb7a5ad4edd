#!/usr/bin/env python3
"""Pin P1 against the reference's own mm_update_extra (LR/align.c:259-318, which calls mm_fix_cigar, :93-172; an external symbol of
oracle/_ref/libgdiet_lr_avx.so, built from /root/reference by oracle/Makefile.ref) on the designed families of tests/post_inputs.py,
and (re)generate tests/golden/update_extra.npz: the inputs and the REFERENCE's CIGAR, shifts, mlen, blen, n_ambi and dp_max.
Runs only where oracle/_ref exists; TEST INFRASTRUCTURE.

    python oracle/pin_post.py            # run the reference on every case, compare with the restatement, write the golden file
    python oracle/pin_post.py --check    # regenerate in memory and compare with the committed file

An mm_reg1_t + mm_extra_t is built per case through ctypes: rev = 0, qs = rs = 0 and qe / re the bases the CIGAR consumes (the
reference asserts that, :126 and :314), is_eqx = 0, codes 0..4 only.  The shifts are read back from the moved qs / rs.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import gdo  # noqa: E402
import post_inputs as P  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(HERE), "tests", "golden", "update_extra.npz")


class Reg1(C.Structure):  # mm_reg1_t, LR/minimap.h:115-131
    _fields_ = [(n, C.c_int32) for n in ("id", "cnt", "rid", "score", "qs", "qe", "rs", "re", "parent", "subsc", "as_", "mlen", "blen", "n_sub", "score0")] + \
               [("bits", C.c_uint32), ("hash", C.c_uint32), ("div", C.c_float), ("p", C.c_void_p)]


EXTRA_WORDS = 6  # mm_extra_t, :105-113: capacity, dp_score, dp_max, dp_max2, n_ambi : 30 | trans_strand : 2, n_cigar, cigar[]


def run_reference(lib, case):
    """the reference on one case -> dict(cigar, qshift, tshift, mlen, blen, dp_max, n_ambi)"""
    _, mat, gq, ge, log_gap = P.SCORINGS[case["sc"]]
    cg = np.asarray(case["cigar"][:case["n_cigar"]], np.uint32)
    assert case["q"].max(initial=0) <= 4 and case["t"].max(initial=0) <= 4
    ql = int(sum(w >> 4 for w in cg if w & 0xf in (0, 1)))
    tl = int(sum(w >> 4 for w in cg if w & 0xf in (0, 2, 3)))
    assert ql == len(case["q"]) and tl == len(case["t"])
    ex = np.zeros(EXTRA_WORDS + max(len(cg), 1), np.uint32)
    ex[0], ex[5] = len(cg), len(cg)
    ex[EXTRA_WORDS:EXTRA_WORDS + len(cg)] = cg
    r = Reg1()
    r.qs, r.qe, r.rs, r.re = 0, ql, 0, tl
    r.p = ex.ctypes.data
    q = np.concatenate([case["q"], np.zeros(8, np.uint8)])  # (the reference reads inside the windows only; the slack is never looked at)
    t = np.concatenate([case["t"], np.zeros(8, np.uint8)])
    m = np.ascontiguousarray(mat, np.int8)
    lib.mm_update_extra(C.byref(r), q.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), C.c_int8(gq), C.c_int8(ge), 0, log_gap)
    n = int(ex[5])
    assert r.qe == ql and r.re == tl
    return dict(cigar=ex[EXTRA_WORDS:EXTRA_WORDS + n].copy(), qshift=int(r.qs), tshift=int(r.rs), mlen=int(r.mlen), blen=int(r.blen), dp_max=int(ex[2].view(np.int32)),
                n_ambi=int(ex[4] & 0x3fffffff))


def generate():
    lib = gdo.load_ref("lr_avx")
    lib.mm_update_extra.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int8, C.c_int8, C.c_int, C.c_int]
    lib.mm_update_extra.restype = None
    cases = P.cases()
    refs, bad = [], 0
    for c in cases:
        if c["score"] == P.NEG_INF or c["n_cigar"] > len(c["cigar"]) or (c["n_cigar"] == 0 and len(c["q"])):
            refs.append(dict(cigar=np.zeros(0, np.uint32), **{k: 0 for k in P.FIELDS}))  # dead by the kernels' rule: never shown to the reference
            continue
        r = run_reference(lib, c)
        refs.append(r)
        if c["n_cigar"] == 0:
            assert all(r[k] == 0 for k in P.FIELDS)
            continue
        mine, _ = P.restate(c)
        if not (np.array_equal(mine["cigar"], r["cigar"]) and all(mine[k] == r[k] for k in P.FIELDS)):
            bad += 1
            if bad <= 5:
                print("MISMATCH restatement vs reference:", c["family"], {k: (mine[k], r[k]) for k in P.FIELDS if mine[k] != r[k]})
    return cases, refs, bad


def pack(cases, refs):
    def cat(arrs, dt):
        off = np.zeros(len(arrs) + 1, np.int64)
        off[1:] = np.cumsum([len(a) for a in arrs])
        return (np.concatenate(arrs).astype(dt) if arrs else np.zeros(0, dt)), off

    q, qo = cat([c["q"] for c in cases], np.uint8)
    t, to = cat([c["t"] for c in cases], np.uint8)
    cg, co = cat([c["cigar"] for c in cases], np.uint32)
    rc, ro = cat([r["cigar"] for r in refs], np.uint32)
    fams = sorted(set(c["family"] for c in cases))
    return dict(q=q, qo=qo, t=t, to=to, cigar=cg, co=co, n_cigar=np.array([c["n_cigar"] for c in cases], np.int32),
                score=np.array([c["score"] for c in cases], np.int32), sc=np.array([c["sc"] for c in cases], np.int16),
                family=np.array([fams.index(c["family"]) for c in cases], np.int16), family_names=np.array(fams),
                sc_names=np.array([s[0] for s in P.SCORINGS]), sc_mat=np.array([s[1] for s in P.SCORINGS], np.int8),
                sc_qel=np.array([s[2:] for s in P.SCORINGS], np.int32),
                ref_cigar=rc, ref_co=ro, ref_out=np.array([[r[k] for k in P.FIELDS] for r in refs], np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    cases, refs, bad = generate()
    new = pack(cases, refs)
    print("update_extra: %d cases through mm_update_extra, restatement_vs_reference_mismatch=%d" % (len(cases), bad))
    if args.check:
        old = np.load(GOLDEN)
        diff = [k for k in new if k not in old.files or not np.array_equal(old[k], new[k])] + [k for k in old.files if k not in new]
        print("golden file:", "identical" if not diff else "DIFFERS in %s" % diff)
        return 1 if (bad or diff) else 0
    np.savez_compressed(GOLDEN, **new)
    print("written %s (%d bytes)" % (GOLDEN, os.path.getsize(GOLDEN)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

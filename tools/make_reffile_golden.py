#!/usr/bin/env python3
"""Test infrastructure: (re)makes the digests of the reference-input tests (tests/golden/reffile/mmi.sha256.json) with THE REFERENCE
ITSELF, in the style of tools/make_samopts_golden.py.

    python tools/make_reffile_golden.py            # check: every committed digest equals what the reference writes today
    python tools/make_reffile_golden.py --write    # rewrite them

For a handful of the inputs of tests/ref_fasta_inputs.py (FILES: canonical, odd and awkward ones, plain, gzip and BGZF) the reference
builds its index from the file and dumps it -- `gdiet_lr_avx <hifi.cmd> -d out.mmi FILE` and `gdiet_sr_avx <sr.cmd> -d out.mmi FILE`, so k,
w, -Z and -W are those of the two canonical command lines -- and the sha256 of the .mmi is written next to the sha256 of the input.
Only digests are committed: small data, no program text.  tests/test_ref_fasta.py compares the host route's .mmi with them on the CPU,
tests/test_ref_fasta_gpu.py the device route's dump_mmi on the GPU.
Where the reference's own reader makes something else of a file than this library's sequential grammar does, the file is listed under
"findings" with what was seen, its digest is still the reference's, and the tests skip nothing: they compare.
Nothing of the product is involved in what is written."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from fixture_io import cmd_of  # noqa: E402
from make_golden import REF  # noqa: E402
import ref_fasta_inputs  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reffile", "mmi.sha256.json")
FILES = ["lr_w60_nl.fa", "lr_w1024_nonl.fa.gz", "lr_w0_nl.fa.bgz", "sr_w70_nl.fa", "sr_w1025_nonl.fa.bgz", "odd_blank_space_iupac.fa", "odd_tiny_dup_longhdr.fa",
         "awk_crlf.fa", "awk_ref.fq", "awk_plus_at.fa", "awk_junk_front.fa"]
KINDS = {"hifi": "lr", "sr": "sr"}  # preset -> variant of the reference


def digests():
    data = ref_fasta_inputs.contents()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in FILES:
            path = os.path.join(tmp, name)
            with open(path, "wb") as f:
                f.write(data[name])
            row = {"input_sha256": hashlib.sha256(data[name]).hexdigest(), "mmi_sha256": {}}
            for kind, variant in KINDS.items():
                mmi = os.path.join(tmp, "out.mmi")
                subprocess.run([REF[variant], "-t", "4"] + cmd_of(kind) + ["-d", mmi, path], capture_output=True, check=True)
                with open(mmi, "rb") as f:
                    row["mmi_sha256"][kind] = hashlib.sha256(f.read()).hexdigest()
                os.remove(mmi)
            out[name] = row
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    if not all(os.path.exists(p) for p in REF.values()):
        sys.exit("oracle/_ref is not built (python __graft_entry__.py build compiles it where the reference's sources are present)")
    have = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            have = json.load(f)
    new = {"files": digests(), "findings": have.get("findings", {})}
    text = json.dumps(new, indent=1, sort_keys=True) + "\n"
    if a.write:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, "w") as f:
            f.write(text)
        print("wrote", OUT)
    elif have.get("files") != new["files"]:
        sys.exit("tests/golden/reffile/mmi.sha256.json differs from what the reference writes today (run with --write and look at the diff)")
    else:
        print("ok: %d files x %d command lines" % (len(FILES), len(KINDS)))


if __name__ == "__main__":
    main()

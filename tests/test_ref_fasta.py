"""CPU: the device stage of the reference input (csrc/ref_fasta.h) on the host emulator tests/emul/ref_fasta_emul.cpp, built as a
stand-alone program under AddressSanitizer / UBSan.  For every input of tests/ref_fasta_inputs.py, at block sizes 256, 1 024, 4 096 and one
block for the whole file, the emulator itself checks the bases, names and lengths against read_record, every block's end against the
next block's start, and the packed S against gd_index_pack_S; it ends with status 1 on any difference.  The tests add what the
counters must be, so that no input passes through the other route: a canonical or odd file hands no block to the host grammar, an
awkward one at least one (the empty file has no block at all)."""
import hashlib
import json
import os
import re
import subprocess

import pytest

import ref_fasta_inputs
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "reffile")
LINE = re.compile(r"ok (\S+) block (\d+) blocks (\d+) handed (\d+) device (\d+) host (\d+) seqs (\d+)$")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return ref_fasta_inputs.files(str(tmp_path_factory.mktemp("ref_inputs")))


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ref_fasta") / "ref_fasta_emul")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "genome-on-diet_amd", "csrc"), os.path.join(ROOT, "tests", "emul", "ref_fasta_emul.cpp"), "-o", exe, "-lz"])
    return exe


@pytest.fixture(scope="module")
def results(emul, inputs):
    """{(name, block size): counters}, one emulator process per group of inputs"""
    out = {}
    names = sorted(inputs)
    for i in range(0, len(names), 16):
        r = subprocess.run([emul, "files"] + [inputs[n] for n in names[i:i + 16]], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        for line in r.stdout.splitlines():
            m = LINE.match(line)
            assert m, line
            out[(os.path.basename(m.group(1)), int(m.group(2)))] = dict(zip(("blocks", "handed", "device", "host", "seqs"), map(int, m.groups()[2:])))
    assert len(out) == 4 * len(names)
    return out


def total_bases(data):
    """of a canonical or odd file: the bytes of the lines that do not start with '>', without the line ends"""
    return sum(len(l) for l in data.split(b"\n") if not l.startswith(b">"))


@pytest.mark.parametrize("grp", ["canonical", "odd"])
def test_the_device_places_every_base_of_a_claimed_file(grp, results):
    data = ref_fasta_inputs.contents()
    for (name, block), st in sorted(results.items()):
        if ref_fasta_inputs.group(name) != grp:
            continue
        text = data[name]
        if name.endswith((".gz", ".bgz")):
            text = data[name.rsplit(".", 1)[0]]
        assert st["handed"] == 0 and st["host"] == 0, (name, block, st)
        assert st["device"] == total_bases(text), (name, block, st)
        assert st["seqs"] == text.count(b"\n>") + 1, (name, block, st)


def test_awkward_files_hand_blocks_to_the_host_grammar(results):
    seen = 0
    for (name, block), st in sorted(results.items()):
        if ref_fasta_inputs.group(name) != "awkward":
            continue
        seen += 1
        if name == "awk_empty.fa":
            assert st == dict(blocks=0, handed=0, device=0, host=0, seqs=0), (block, st)
        else:
            assert st["handed"] >= 1 and st["host"] > 0, (name, block, st)
    assert seen == 4 * 5


def test_small_blocks_return_to_the_device_behind_an_awkward_stretch(results):
    """a block that disqualifies costs its own bytes and what follows up to a line boundary, not the rest of the file"""
    for name in ("awk_plus_at.fa", "awk_junk_front.fa"):
        st = results[(name, 256)]
        assert 0 < st["handed"] < st["blocks"] and st["device"] > st["host"], (name, st)
    st = results[("awk_crlf.fa", 256)]  # ("\r" in every line: nothing for the device)
    assert st["handed"] == st["blocks"] and st["device"] == 0, st


def test_what_the_grammar_makes_of_the_awkward_files(results):
    """the records kseq_read returns, worked out by hand from LR/kseq.h:191-232 (tests/ref_fasta_inputs.py says how each file is made)"""
    want = {"awk_crlf.fa": 4, "awk_ref.fq": 3, "awk_plus_at.fa": 8, "awk_junk_front.fa": 3}
    for name, n in want.items():
        for block in (256, 1024, 4096, 64 << 20):
            assert results[(name, block)]["seqs"] == n, (name, block, results[(name, block)])


PRESET_KWZ = {"hifi": (19, 19, "10"), "sr": (21, 11, "10")}  # k, w, -Z of lr/hifi.cmd and sr/sr.cmd (-W 2 is the pattern's length)
# files the reference's own reader reads differently from this library's grammar (tests/golden/reffile: "findings")
KNOWN_FINDINGS = set()


def test_host_route_mmi_is_the_reference_s(emul, inputs, tmp_path):
    """reader records -> gd_index_build -> .mmi on the CPU (what GDIET_INDEX_BUILD=host runs), against the sha256 of `GDiet_avx -d` on
    the same file at hifi.cmd's and sr.cmd's k, w, -Z, -W (tools/make_reffile_golden.py)"""
    with open(os.path.join(GOLDEN, "mmi.sha256.json")) as f:
        g = json.load(f)
    data = ref_fasta_inputs.contents()
    assert len(g["files"]) >= 8 and set(g["findings"]) == KNOWN_FINDINGS, g["findings"]
    for name, row in sorted(g["files"].items()):
        assert hashlib.sha256(data[name]).hexdigest() == row["input_sha256"], name
        assert set(row["mmi_sha256"]) == set(PRESET_KWZ), name
        for preset, (k, w, z) in PRESET_KWZ.items():
            out = str(tmp_path / "out.mmi")
            subprocess.run([emul, "mmi", inputs[name], str(k), str(w), z, out], check=True, timeout=300)
            with open(out, "rb") as f:
                got = hashlib.sha256(f.read()).hexdigest()
            assert (got == row["mmi_sha256"][preset]) == (name not in g["findings"]), (name, preset)

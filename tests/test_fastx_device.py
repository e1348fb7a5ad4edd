"""CPU: the device mode of the reader (csrc/fastx_dev.h) on the host emulator tests/emul/fastx_dev_emul.cpp, built as a stand-alone
program under AddressSanitizer / UBSan.  The emulator installs an executor that runs the device's passes as loops in a real GdFastx,
checks every accepted record and every hand-over position against GdFastxParser inside each block, and compares the attached
reader's batches with the unattached reader's; it ends with status 1 on any difference.  The tests add what the counts must be."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from fastx_device_inputs import mixed_file, newline_geometry, strict_prefix, sweep_file
from fastx_inputs import awkward_inputs

BLOCKS = [256, 1000, 4096, 8 << 20]  # 1000: not a multiple of the 16-byte lane
# strict prefixes of the awkward inputs, counted with a line-based restatement of the predicate (strict_prefix below checks them again)
STRICT = {"plain.fq": 40, "broken_mid.fq": 12, "truncated.fq": 3, "multiline.fq": 0, "crlf.fq": 0, "multi.fa": 0}


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fastx_dev") / "fastx_dev_emul")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "genome-on-diet_amd", "csrc"), os.path.join(ROOT, "tests", "emul", "fastx_dev_emul.cpp"), "-o", exe, "-lz"])
    return exe


def run(emul, path, block, chunk):
    r = subprocess.run([emul, path, str(block), str(chunk)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (block, chunk, r.stdout[-2000:], r.stderr[-2000:])
    m = re.match(r"ok device (\d+) host (\d+) total (\d+) early (\d+) blocks (\d+) handed (\d+)\n$", r.stdout)
    assert m, r.stdout
    return dict(zip(("device", "host", "total", "early", "blocks", "handed"), map(int, m.groups())))


def test_strict_prefixes_of_the_awkward_inputs():
    files = awkward_inputs(np.random.default_rng(31))
    assert {k: strict_prefix(v) for k, v in files.items()} == STRICT


@pytest.mark.parametrize("name", sorted(STRICT))
def test_awkward_inputs(name, emul, tmp_path):
    data = awkward_inputs(np.random.default_rng(31))[name]
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    for block in BLOCKS:
        st = run(emul, path, block, 1500)
        assert st["early"] == (1 if name in ("truncated.fq", "broken_mid.fq") else 0)
        if block == 8 << 20:  # the whole file is one block: the device's share is the strict prefix of the file
            assert st["device"] == STRICT[name], st
        if name == "plain.fq":
            assert (st["device"], st["host"]) == (40, 0), (block, st)
        if STRICT[name] == 0:
            assert st["device"] == 0, (block, st)  # (the multi-line records always wrap: none is strict by accident)


def test_geometry_sweep_is_all_the_devices(emul, tmp_path):
    data, n = sweep_file()
    mod16, mod1024 = newline_geometry(data)
    assert mod16 == set(range(16)) and {0, 1023} <= mod1024  # every residue of the lane, both sides of a tile edge
    assert strict_prefix(data) == n
    path = str(tmp_path / "sweep.fq")
    with open(path, "wb") as f:
        f.write(data)
    for block in BLOCKS:
        st = run(emul, path, block, 20000)
        assert (st["device"], st["host"], st["total"]) == (n, 0, n), (block, st)


@pytest.mark.parametrize("block", [4096, 65536])
def test_mixed_file(block, emul, tmp_path):
    path = str(tmp_path / "mixed.fq")
    with open(path, "wb") as f:
        f.write(mixed_file())
    for chunk in (3000, 10 ** 7):
        st = run(emul, path, block, chunk)
        assert st["total"] == 6000 and st["early"] == 1, st
        assert st["device"] > 0 and st["host"] > 0 and st["handed"] > 0, st

"""CPU: the thread's error mark behind gdiet_hip_strerror (csrc/err_mark.h) -- two threads fail on one context and each reads its own
text, a third reads none -- plain and under ThreadSanitizer."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.parametrize("tsan", [False, True])
def test_every_thread_reads_its_own_text(tmp_path, tsan):
    exe = str(tmp_path / "err_mark_test")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "genome-on-diet_amd", "csrc"),
           os.path.join(ROOT, "tests", "emul", "err_mark_test.cpp"), "-o", exe]
    if tsan:
        cmd.insert(1, "-fsanitize=thread")
    subprocess.check_call(cmd)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bad 0" in r.stdout
    assert "WARNING: ThreadSanitizer" not in r.stderr

"""GPU: the drain launches of the compact backtrace arena run over the pending list, and only where there is one.  A box of the main
launch that finds the overflow pool used up appends its id to a list on the device.  gdiet_hip_ksw_extd2_batch and the mapping path wait
for their stream anyway: the host reads the list's length when the main launch has ended and enqueues no drain launch for an empty
list.  gdiet_hip_ksw_extd2_batch_dev never waits: the planner's worst case is enqueued up front.  Scores and CIGARs against the oracle at
w = 1000 either way (the pairs, the oracle's alignments and the comparison are those of test_compact_arena_gpu.py); the decision through
gdiet_hip_last_drain_launches.  mm_fix_cigar is now the prologue of map_post_wave_kernel: the goldens through it.  The switches are read
when the library is loaded, so every case runs in a process of its own."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_compact_arena_gpu import _align256, _check, _full, _half, want  # noqa: F401  (want: the fixture, computed once for this module)

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("GDIET_BT_COMPACT", "GDIET_BT_OVERFLOW_MB", "GDIET_POST_WAVE")


def _env(**env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    return e


def _run(which, entry, tmp_path, **env):
    out = str(tmp_path / ("%s_%s.npz" % (which, entry)))
    r = subprocess.run([sys.executable, os.path.join(HERE, "batch_tail_run.py"), "pairs", which, entry, out], capture_output=True, text=True, env=_env(**env), timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    return np.load(out)


def _planned_drain_launches(pairs, pool):
    """gd_drain_launches (ksw_plan.h) for a batch whose boxes all have half-size slots: what is enqueued where nobody waits"""
    slots, total, largest = sum(_half(p) for p in pairs), sum(_full(p) for p in pairs), max(_full(p) for p in pairs)
    if pool is None:
        pool = max(_align256(slots // 16), min(total, 64 << 20))
    arena = max(slots + pool, largest)
    per = arena - largest + 256
    return min(len(pairs), (total + per - 1) // per)


CASES = [("mix", None, (12, 0)), ("mix", "0", (0, 12)), ("fallback24", "0", (0, 24))]


@pytest.mark.gpu
@pytest.mark.parametrize("which,pool,served", CASES, ids=["mix-default", "mix-pool0", "fallback24-pool0"])
def test_the_host_drains_only_what_is_pending(which, pool, served, want, tmp_path):
    got = _run(which, "host", tmp_path, **({} if pool is None else {"GDIET_BT_OVERFLOW_MB": pool}))
    _check(got, want[which], "%s, pool %s, host entry" % (which, pool))
    claimed, drained, _ = (int(x) for x in got["arena"])
    launches = int(got["launches"])
    print("claimed %d drained %d drain launches %d (planned for the whole batch: %d)" % (claimed, drained, launches, _planned_drain_launches(want[which][0], None if pool is None else 0)))
    assert (claimed, drained) == served
    if drained == 0:
        assert launches == 0  # nothing pending: nothing enqueued
    elif which == "mix":
        assert launches >= 1
    else:
        assert launches >= 2  # (the arena holds fewer than 24 full-size boxes: test_compact_arena_gpu.py asserts the arithmetic)
    assert launches <= _planned_drain_launches(want[which][0], None if pool is None else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("which,pool,served", CASES, ids=["mix-default", "mix-pool0", "fallback24-pool0"])
def test_a_callers_stream_gets_them_up_front(which, pool, served, want, tmp_path):
    got = _run(which, "dev", tmp_path, **({} if pool is None else {"GDIET_BT_OVERFLOW_MB": pool}))
    _check(got, want[which], "%s, pool %s, device entry" % (which, pool))
    claimed, drained, _ = (int(x) for x in got["arena"])
    launches, planned = int(got["launches"]), _planned_drain_launches(want[which][0], None if pool is None else 0)
    print("claimed %d drained %d drain launches %d, planned %d" % (claimed, drained, launches, planned))
    assert (claimed, drained) == served
    assert launches == planned and launches >= (2 if which == "fallback24" else 1)  # no decision on the host: the worst case, also for an empty list


@pytest.mark.gpu
def test_two_batches_in_flight_decide_per_lane():
    """hifi_sv as two batches in flight (submit, submit, wait, wait) without an overflow pool: each lane waits for its own main launch
    and enqueues drain launches for what that launch left pending.  The reads are hifi_sv's own: its structural variants leave boxes whose
    certificate fails at both rungs, so with no pool the two batches drain at least one box between them (asserted)."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "batch_tail_run.py"), "inflight", "hifi_sv"], capture_output=True, text=True,
                       env=_env(GDIET_BT_OVERFLOW_MB="0"), timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    m = re.search(r"IN_FLIGHT drained (\d+) launches (\d+)", r.stdout)
    print(m.group(0))
    assert int(m.group(1)) >= 1 and int(m.group(2)) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("post_wave", ["default", "1"])
def test_goldens_through_the_fused_post_kernel(post_wave):
    """hifi, hifi_sv and hifi_rep: every SAM record as recorded, with the kernel chosen by the batch and with the wave form forced"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden_env_check.py"), "hifi", "hifi_sv", "hifi_rep"], capture_output=True, text=True,
                       env=_env(**({} if post_wave == "default" else {"GDIET_POST_WAVE": post_wave})), timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]

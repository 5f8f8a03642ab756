"""Host-only side of StepPlan's host push: step_push_ranges (who copies
which byte of an H2D copy) and the worker pool run alone on host memory by
bin/hpk_push_pool. No GPU."""

import subprocess
from pathlib import Path

import numpy as np
import pytest

from hpc_patterns_amd._native import native

ROOT = Path(__file__).resolve().parent.parent

SIZES = [0, 1, 63, 64, 4096, 4096 + 68, (1 << 20) + 68]
THREADS = [1, 3, 8]
FRACTIONS = [0, 0.01, 0.25, 0.5, 1]


@pytest.mark.parametrize("g", FRACTIONS)
@pytest.mark.parametrize("nthreads", THREADS)
@pytest.mark.parametrize("nbytes", SIZES)
def test_ranges_cover_each_byte_once_and_are_aligned(nbytes, nthreads, g):
    head, ranges = native().step_push_ranges(nbytes, g, nthreads)
    assert len(ranges) == nthreads
    assert 0 <= head <= nbytes
    if g == 0:
        assert head == nbytes
    else:
        assert head % 4096 == 0
        # rounded down to 4 KiB: never more than asked stays on the engine
        want_tail = int(nbytes * g + 0.5)
        assert nbytes - want_tail - 4096 < head <= nbytes - want_tail
    if g == 1:
        assert head == 0
    covered = np.zeros(nbytes, dtype=np.int32)
    covered[:head] += 1
    for begin, end in ranges:
        assert head <= begin <= end <= nbytes
        covered[begin:end] += 1
        if end > begin:
            assert begin % 64 == 0
            assert end % 64 == 0 or end == nbytes
    assert (covered == 1).all()
    # in order, and empty ranges only after the last byte is dealt out
    nonempty = [(b, e) for b, e in ranges if e > b]
    assert nonempty == sorted(nonempty)
    for (_, e0), (b1, _) in zip(nonempty, nonempty[1:]):
        assert e0 == b1
    # as even as whole lines allow
    lines = [-(-(e - b) // 64) for b, e in ranges]
    assert max(lines) - min(lines) <= 1


def test_ranges_clamp_bad_arguments():
    hpk = native()
    assert hpk.step_push_ranges(8192, -1.0, 2) == hpk.step_push_ranges(8192, 0, 2)
    assert hpk.step_push_ranges(8192, 7.0, 2) == hpk.step_push_ranges(8192, 1, 2)
    assert hpk.step_push_ranges(8192, float("nan"), 2)[0] == 8192
    assert len(hpk.step_push_ranges(8192, 0.5, 0)[1]) == 1


def test_worker_pool_alone_on_host_memory():
    """The stand-alone program checks payloads, guard bytes, wake-up from
    sleep and stop() with a kick in flight; here only its verdict."""
    exe = ROOT / "bin" / "hpk_push_pool"
    assert exe.exists(), "bin/hpk_push_pool not built (make bins)"
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "push_pool OK" in res.stdout

"""StepPlan host push (native/step.hip, include/push_pool.h): the tail of
H2D stored by host threads through the PCIe BAR. h2d_dev must hold the
source bytes whatever the split, seen by a copy engine and by a kernel, round
after round; the other three outputs must not notice; the submit/join/close
contract must hold with workers in play."""

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MIB = 1 << 20


def _host_view(ptr, nbytes):
    return np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(ptr))


class _Rig:
    """Raw buffers + a plan over them, shaped like FlagshipPatternStep's at
    SMOKE_CONFIG size."""

    def __init__(self, h2d_bytes, push_fraction=-1.0, d2h_bytes=MIB,
                 d2d_floats=1 << 20, globalsize=1 << 14, time_copies=False):
        from hpc_patterns_amd._native import native

        self.hpk = hpk = native()
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        self.h2d_bytes, self.d2h_bytes = h2d_bytes, d2h_bytes
        self.h2d_host = hpk.host_malloc(h2d_bytes)
        self.h2d_dev = hpk.hip_malloc(h2d_bytes)
        self.d2h_dev = hpk.hip_malloc(d2h_bytes)
        self.d2h_host = hpk.host_malloc(d2h_bytes)
        self.h2d_copy = torch.zeros(h2d_bytes, dtype=torch.uint8, device=dev)
        self.d2d_src = torch.empty(d2d_floats, dtype=torch.float32, device=dev)
        self.d2d_dst = torch.zeros_like(self.d2d_src)
        self.busy_out = torch.zeros(globalsize, dtype=torch.float32, device=dev)
        self.streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        self.h2d_src = _host_view(self.h2d_host, h2d_bytes)
        self.d2h_dst = _host_view(self.d2h_host, d2h_bytes)
        torch.cuda.synchronize()
        self.plan = hpk.StepPlan(
            0, (self.h2d_dev, self.h2d_host, h2d_bytes),
            (self.d2h_host, self.d2h_dev, d2h_bytes),
            (self.d2d_dst.data_ptr(), self.d2d_src.data_ptr(), d2d_floats * 4),
            self.busy_out.data_ptr(), globalsize,
            self.streams[0].cuda_stream, self.streams[1].cuda_stream,
            time_copies=time_copies, push_fraction=push_fraction)

    def read_dev(self, ptr, nbytes):
        """hipMemcpy readback of a raw device buffer."""
        out = np.empty(nbytes, dtype=np.uint8)
        self.hpk.memcpy_async(out.ctypes.data, ptr, nbytes, 0)
        self.hpk.stream_synchronize(0)
        return out

    def read_h2d_by_kernel(self):
        """h2d_dev through the shader copy kernel into a second device
        buffer, then hipMemcpy."""
        self.hpk.copy_kernel(self.h2d_copy.data_ptr(), self.h2d_dev,
                             self.h2d_bytes, 0)
        self.hpk.stream_synchronize(0)
        return self.read_dev(self.h2d_copy.data_ptr(), self.h2d_bytes)

    def write_dev(self, ptr, arr):
        arr = np.ascontiguousarray(arr).view(np.uint8)
        self.hpk.memcpy_async(ptr, arr.ctypes.data, arr.nbytes, 0)
        self.hpk.stream_synchronize(0)

    def close(self):
        self.plan.close()
        torch.cuda.synchronize()
        self.hpk.host_free(self.h2d_host)
        self.hpk.hip_free(self.h2d_dev)
        self.hpk.hip_free(self.d2h_dev)
        self.hpk.host_free(self.d2h_host)


def _expected_fraction(hpk, nbytes, g, nthreads=8):
    head, _ = hpk.step_push_ranges(nbytes, g, nthreads)
    return (nbytes - head) / nbytes


# (h2d_bytes, threads): 1 MiB; a tail that is no multiple of 64 or of the
# thread count; 4 KiB over 8 threads (512-byte ranges); 4 KiB + 68 over 8
# threads, whose tail at small g is one line and a 4-byte rest, so six
# threads get nothing.
SHAPES = [(MIB, None), (MIB + 68, "3"), (4096, "8"), (4096 + 68, "8")]
# 0/0.25/0.5 through HPK_STEP_PUSH, 0.01 and 1.0 through the constructor
FRACTIONS = [("env", "0"), ("env", "0.25"), ("env", "0.5"), ("arg", 0.01),
             ("arg", 1.0)]


@pytest.mark.parametrize("how,g", FRACTIONS)
@pytest.mark.parametrize("h2d_bytes,threads", SHAPES)
def test_h2d_dev_holds_the_source(monkeypatch, h2d_bytes, threads, how, g):
    """Three rounds, a different seeded payload each: a stale write-combine
    buffer or HDP line would show as bytes of the round before."""
    if threads is None:
        monkeypatch.delenv("HPK_STEP_PUSH_THREADS", raising=False)
    else:
        monkeypatch.setenv("HPK_STEP_PUSH_THREADS", threads)
    if how == "env":
        monkeypatch.setenv("HPK_STEP_PUSH", g)
        rig = _Rig(h2d_bytes)
    else:
        monkeypatch.delenv("HPK_STEP_PUSH", raising=False)
        rig = _Rig(h2d_bytes, push_fraction=g)
    try:
        plan = rig.plan
        want = float(g)
        if want > 0 and not plan.push_access:
            # the machine refuses CPU access or has no HDP flush register:
            # the plan must say so and run without a push
            assert plan.push_fraction == 0 and plan.push_threads == 0
        else:
            nthreads = int(threads or 8)
            assert plan.push_fraction == pytest.approx(
                _expected_fraction(rig.hpk, h2d_bytes, want, nthreads))
            assert plan.push_threads == (nthreads if plan.push_fraction else 0)
        for rnd in range(3):
            payload = np.random.default_rng(100 + rnd).integers(
                0, 256, h2d_bytes, dtype=np.uint8)
            rig.h2d_src[:] = payload
            plan.submit(64)
            plan.join()
            assert np.array_equal(rig.read_dev(rig.h2d_dev, h2d_bytes),
                                  payload), f"hipMemcpy readback, round {rnd}"
            assert np.array_equal(rig.read_h2d_by_kernel(), payload), \
                f"kernel readback, round {rnd}"
    finally:
        rig.close()


def _outputs(g):
    rig = _Rig(MIB, push_fraction=g)
    try:
        rng = np.random.default_rng(5)
        rig.h2d_src[:] = rng.integers(0, 256, MIB, dtype=np.uint8)
        rig.write_dev(rig.d2h_dev, rng.integers(0, 256, MIB, dtype=np.uint8))
        rig.write_dev(rig.d2d_src.data_ptr(),
                      rng.integers(0, 256, 4 << 20, dtype=np.uint8))
        rig.d2h_dst[:] = 0
        for _ in range(2):
            rig.plan.submit(64)
            rig.plan.join()
        torch.cuda.synchronize()
        return (rig.plan.push_fraction, rig.d2h_dst.copy(),
                rig.d2d_dst.cpu(), rig.busy_out.cpu(),
                rig.read_dev(rig.h2d_dev, MIB))
    finally:
        rig.close()


def test_other_outputs_unchanged_against_no_push():
    g0, d2h0, d2d0, busy0, h2d0 = _outputs(0.0)
    assert g0 == 0
    for g in (0.25, 0.5, 1.0):
        _, d2h, d2d, busy, h2d = _outputs(g)
        assert np.array_equal(d2h, d2h0), g
        # random bytes make NaNs as float32: compare the bits
        assert torch.equal(d2d.view(torch.int32), d2d0.view(torch.int32)), g
        assert torch.equal(busy.view(torch.int32), busy0.view(torch.int32)), g
        assert np.array_equal(h2d, h2d0), g
    assert d2h0.any() and h2d0.any()


def test_contract_with_workers():
    rig = _Rig(MIB, push_fraction=0.5, time_copies=True)
    try:
        plan = rig.plan
        rig.h2d_src[:] = 7
        plan.submit(64)
        with pytest.raises(RuntimeError, match="not joined"):
            plan.submit(64)
        assert plan.pending
        plan.join()
        assert not plan.pending
        assert np.array_equal(rig.read_dev(rig.h2d_dev, MIB),
                              np.full(MIB, 7, dtype=np.uint8))
        assert len(plan.copy_times()) == 2
        wake_ns, done_ns = plan.push_times()
        print(f"workers: first store {wake_ns} ns, done {done_ns} ns "
              f"after submit")
        if plan.push_threads:
            assert 0 < wake_ns <= done_ns

        # close() with a submission pending completes it and joins the
        # workers (a worker left running would write after the free below)
        rig.h2d_src[:] = 9
        plan.submit(64)
        plan.close()
        assert not plan.pending
        assert np.array_equal(rig.read_dev(rig.h2d_dev, MIB),
                              np.full(MIB, 9, dtype=np.uint8))
        plan.close()
        with pytest.raises(RuntimeError, match="after close"):
            plan.submit(64)
    finally:
        rig.close()


def test_push_off_and_small_copies_do_not_push(monkeypatch):
    """HPK_STEP_PUSH=0 stands in for a machine that refuses access or has no
    flush register: the plan runs with push_fraction == 0. So does a plan
    left to choose for itself below the size where a push can pay."""
    monkeypatch.setenv("HPK_STEP_PUSH", "0")
    rig = _Rig(MIB)
    try:
        assert rig.plan.push_fraction == 0 and rig.plan.push_threads == 0
        rig.h2d_src[:] = 3
        rig.plan.submit(64)
        rig.plan.join()
        assert np.array_equal(rig.read_dev(rig.h2d_dev, MIB),
                              np.full(MIB, 3, dtype=np.uint8))
        assert rig.plan.push_times() == (0, 0)
    finally:
        rig.close()
    monkeypatch.delenv("HPK_STEP_PUSH")
    rig = _Rig(MIB)
    try:
        assert rig.plan.push_fraction == 0
    finally:
        rig.close()
    monkeypatch.setenv("HPK_STEP_PUSH", "1.5")
    with pytest.raises(RuntimeError, match="HPK_STEP_PUSH"):
        _Rig(MIB)

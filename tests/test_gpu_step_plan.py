"""StepPlan (native/step.hip): the flagship step's four local commands behind
one native submit and one join — completion, signal re-arming, odd sizes,
the submit/join/close contract, agreement with the one-call-per-command
path, and the opt-in copy-timestamp diagnostic."""

import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MIB = 1 << 20


def _host_view(ptr, nbytes, dtype=np.uint8):
    raw = np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(ptr))
    return raw.view(dtype)


class _Rig:
    """Raw buffers + a plan over them, shaped like FlagshipPatternStep's."""

    def __init__(self, h2d_bytes, d2h_bytes, d2d_floats, globalsize=1 << 14,
                 time_copies=False):
        from hpc_patterns_amd._native import native

        self.hpk = hpk = native()
        torch.cuda.set_device(0)
        self.dev = torch.device("cuda", 0)
        self.h2d_bytes, self.d2h_bytes = h2d_bytes, d2h_bytes
        self.h2d_host = hpk.host_malloc(h2d_bytes)
        self.h2d_dev = hpk.hip_malloc(h2d_bytes)
        self.d2h_dev = hpk.hip_malloc(d2h_bytes)
        self.d2h_host = hpk.host_malloc(d2h_bytes)
        self.d2d_src = torch.empty(d2d_floats, dtype=torch.float32,
                                   device=self.dev)
        self.d2d_dst = torch.zeros_like(self.d2d_src)
        self.busy_out = torch.zeros(globalsize, dtype=torch.float32,
                                    device=self.dev)
        self.streams = [torch.cuda.Stream(device=self.dev) for _ in range(2)]
        self.h2d_src = _host_view(self.h2d_host, h2d_bytes)
        self.d2h_dst = _host_view(self.d2h_host, d2h_bytes)
        self.d2h_dst[:] = 0
        torch.cuda.synchronize()
        self.plan = hpk.StepPlan(
            0, (self.h2d_dev, self.h2d_host, h2d_bytes),
            (self.d2h_host, self.d2h_dev, d2h_bytes),
            (self.d2d_dst.data_ptr(), self.d2d_src.data_ptr(), d2d_floats * 4),
            self.busy_out.data_ptr(), globalsize,
            self.streams[0].cuda_stream, self.streams[1].cuda_stream,
            time_copies=time_copies)

    def read_dev(self, ptr, nbytes):
        """Blocking device->host readback of a raw device buffer."""
        out = np.empty(nbytes, dtype=np.uint8)
        self.hpk.memcpy_async(out.ctypes.data, ptr, nbytes, 0)
        self.hpk.stream_synchronize(0)
        return out

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


def test_join_waits_and_signals_rearm():
    """32 MiB copies (~0.6 ms each): a join() that returned early, or a
    signal left at 0 from the round before, leaves the previous round's
    value in the tail of a buffer."""
    n = 32 * MIB
    rig = _Rig(n, n, MIB // 4)
    try:
        rig.d2d_src.fill_(3.0)
        h2d_src_f = rig.h2d_src.view(np.float32)
        d2h_dst_f = rig.d2h_dst.view(np.float32)
        for rnd in range(20):
            val = float(rnd + 1)
            h2d_src_f[:] = val
            rig.hpk.fill_f32(rig.d2h_dev, val + 0.5, n // 4, 0)
            torch.cuda.synchronize()
            rig.plan.submit(64)
            rig.plan.join()
            assert not rig.plan.pending
            got = torch.from_numpy(rig.read_dev(rig.h2d_dev, n).view(np.float32))
            assert torch.equal(got, torch.full((n // 4,), val)), f"H2D round {rnd}"
            assert np.array_equal(
                d2h_dst_f, np.full(n // 4, val + 0.5, dtype=np.float32)), \
                f"D2H round {rnd}"
        torch.cuda.synchronize()
        assert torch.equal(rig.d2d_dst, rig.d2d_src)
    finally:
        rig.close()


def test_sizes_with_remainders():
    """4-byte H2D, 1 MiB + 4 byte D2H, 2^20 + 3 float D2D (16-byte body plus
    the byte-tail kernel): byte for byte equal to the sources."""
    h2d_bytes, d2h_bytes, d2d_floats = 4, MIB + 4, (1 << 20) + 3
    rig = _Rig(h2d_bytes, d2h_bytes, d2d_floats)
    try:
        rng = np.random.default_rng(7)
        h2d_payload = rng.integers(0, 256, h2d_bytes, dtype=np.uint8)
        d2h_payload = rng.integers(0, 256, d2h_bytes, dtype=np.uint8)
        d2d_payload = rng.integers(0, 256, d2d_floats * 4, dtype=np.uint8)
        rig.h2d_src[:] = h2d_payload
        rig.write_dev(rig.d2h_dev, d2h_payload)
        rig.write_dev(rig.d2d_src.data_ptr(), d2d_payload)
        rig.write_dev(rig.h2d_dev, np.zeros(h2d_bytes, dtype=np.uint8))
        torch.cuda.synchronize()
        rig.plan.submit(64)
        rig.plan.join()
        assert np.array_equal(rig.read_dev(rig.h2d_dev, h2d_bytes), h2d_payload)
        assert np.array_equal(rig.d2h_dst, d2h_payload)
        assert np.array_equal(
            rig.read_dev(rig.d2d_dst.data_ptr(), d2d_floats * 4), d2d_payload)
    finally:
        rig.close()


def test_submit_join_close_contract():
    n = 32 * MIB
    rig = _Rig(n, n, MIB // 4)
    try:
        rig.plan.join()  # nothing pending: returns
        assert not rig.plan.pending

        rig.h2d_src.view(np.float32)[:] = 11.0
        rig.hpk.fill_f32(rig.d2h_dev, 12.0, n // 4, 0)
        torch.cuda.synchronize()
        rig.plan.submit(64)
        with pytest.raises(RuntimeError, match="not joined"):
            rig.plan.submit(64)
        assert rig.plan.pending  # the first submission is still joinable
        rig.plan.join()
        assert not rig.plan.pending
        assert np.array_equal(rig.read_dev(rig.h2d_dev, n).view(np.float32),
                              np.full(n // 4, 11.0, dtype=np.float32))
        assert np.array_equal(rig.d2h_dst.view(np.float32),
                              np.full(n // 4, 12.0, dtype=np.float32))

        # close() with a submission pending completes it
        rig.h2d_src.view(np.float32)[:] = 21.0
        rig.hpk.fill_f32(rig.d2h_dev, 22.0, n // 4, 0)
        torch.cuda.synchronize()
        rig.plan.submit(64)
        rig.plan.close()
        assert not rig.plan.pending
        assert np.array_equal(rig.read_dev(rig.h2d_dev, n).view(np.float32),
                              np.full(n // 4, 21.0, dtype=np.float32))
        assert np.array_equal(rig.d2h_dst.view(np.float32),
                              np.full(n // 4, 22.0, dtype=np.float32))
        rig.plan.close()  # second close: no-op
        with pytest.raises(RuntimeError, match="after close"):
            rig.plan.submit(64)
    finally:
        rig.close()


def _run_flagship(monkeypatch, plan_env):
    from hpc_patterns_amd.models import SMOKE_CONFIG, FlagshipPatternStep

    if plan_env is None:
        monkeypatch.delenv("HPK_STEP_PLAN", raising=False)
    else:
        monkeypatch.setenv("HPK_STEP_PLAN", plan_env)
    dev = torch.device("cuda", 0)
    step = FlagshipPatternStep(device=dev, rank=0, world_size=1,
                               config=dict(SMOKE_CONFIG))
    try:
        cfg = step.config
        rng = np.random.default_rng(20240517)
        rng.random(out=_host_view(step.h2d_host, cfg["h2d_bytes"], np.float32),
                   dtype=np.float32)
        for _ in range(3):
            step.step()
        torch.cuda.synchronize()
        h2d = np.empty(cfg["h2d_bytes"], dtype=np.uint8)
        step.hpk.memcpy_async(h2d.ctypes.data, step.h2d_dev,
                              cfg["h2d_bytes"], 0)
        step.hpk.stream_synchronize(0)
        return {
            "has_plan": step.plan is not None,
            "d2d_dst": step.d2d_dst.cpu(),
            "h2d_dev": h2d,
            "d2h_host": _host_view(step.d2h_host, cfg["d2h_bytes"]).copy(),
            "compute_out": step.compute_out[:cfg["compute_globalsize"]].cpu(),
        }
    finally:
        step.close()


def test_plan_and_per_command_paths_agree(monkeypatch):
    on = _run_flagship(monkeypatch, None)
    off = _run_flagship(monkeypatch, "0")
    assert on["has_plan"], "step fell back silently with HPK_STEP_PLAN unset"
    assert not off["has_plan"]
    assert torch.equal(on["d2d_dst"], off["d2d_dst"])
    assert np.array_equal(on["h2d_dev"], off["h2d_dev"])
    assert np.array_equal(on["d2h_host"], off["d2h_host"])
    assert torch.equal(on["compute_out"], off["compute_out"])
    # and the copies carried the payloads, not zeros on both sides
    assert on["h2d_dev"].any() and on["d2h_host"].any()


def test_copy_time_diagnostic():
    n = 32 * MIB
    rig = _Rig(n, n, MIB // 4, time_copies=True)
    try:
        rig.plan.submit(64)  # first touch of the buffers
        rig.plan.join()
        assert len(rig.plan.copy_times()) == 2
        rig.plan.clear_copy_times()
        assert rig.plan.copy_times() == []
        rig.plan.submit(64)
        rig.plan.join()
        times = rig.plan.copy_times()
        assert len(times) == 2
        ideal_ns = n / 57e9 * 1e9
        for start, end in times:
            print(f"copy {start}..{end}: {(end - start) / 1e6:.3f} ms")
            assert start < end
            assert ideal_ns / 4 <= end - start <= ideal_ns * 4
    finally:
        rig.close()

    rig = _Rig(n, n, MIB // 4)  # timing off: nothing recorded
    try:
        rig.plan.submit(64)
        rig.plan.join()
        assert rig.plan.copy_times() == []
    finally:
        rig.close()

"""GPU numerics tests: every hand-written HIP kernel vs a plain PyTorch fp32
reference (SURVEY.md §4 oracle style — exact where the math is exact)."""

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    from hpc_patterns_amd import ops as _ops
    from hpc_patterns_amd._native import native

    native()  # fail loudly, not skip: on a GPU box the extension must exist
    return _ops


@pytest.mark.parametrize("n", [1, 3, 4, 255, 1 << 20, (1 << 20) + 7])
def test_fill(ops, dev, n):
    t = torch.empty(n, dtype=torch.float32, device=dev)
    ops.fill(t, 3.5)
    torch.cuda.synchronize()
    assert torch.equal(t, torch.full((n,), 3.5, device=dev))


@pytest.mark.parametrize("n", [1, 17, 1 << 20])
def test_iota(ops, dev, n):
    t = torch.empty(n, dtype=torch.float32, device=dev)
    ops.iota(t)
    torch.cuda.synchronize()
    assert torch.equal(t, torch.arange(n, dtype=torch.float32, device=dev))


@pytest.mark.parametrize("n", [4, 1023, 1 << 22, (1 << 24) + 3])
def test_accumulate(ops, dev, n):
    a = torch.rand(n, device=dev)
    b = torch.rand(n, device=dev)
    ref = a + b
    ops.accumulate(a, b)
    torch.cuda.synchronize()
    assert torch.equal(a, ref)  # fp32 add is exact vs torch's fp32 add


@pytest.mark.parametrize("nbytes", [16, 4096, (1 << 22) + 36])
def test_copy_kernel(ops, dev, nbytes):
    n = nbytes // 4
    src = torch.rand(n, device=dev)
    dst = torch.empty_like(src)
    ops.copy_kernel(dst, src)
    torch.cuda.synchronize()
    assert torch.equal(dst, src)


def test_copy_kernel_aligned_pointer_odd_length(ops, dev):
    base = torch.rand(1029, device=dev)  # odd length -> 16B body + tail
    dst = torch.empty_like(base)
    ops.copy_kernel(dst, base)
    torch.cuda.synchronize()
    assert torch.equal(dst, base)


# ---------------------------------------------------------------------------
# Streaming kernels at their edges: misaligned pointers (the scalar
# fallbacks of every launcher), vector-body tails, the unrolled copy body,
# and a second grid-stride iteration at the benchmark's size regime. Every
# write target sits inside one larger allocation between 64-byte canaries.
# ---------------------------------------------------------------------------

_CANARY = 64      # bytes on each side of a write target
_CANARY_BYTE = 0xA5
_MISALIGNED_NS = [1, 3, 4, 5, 17, 255, 1025, (1 << 20) + 3]
_TAIL_NS = [4 * q + r for q in (1, 64, 257) for r in (1, 2, 3)]


def _window(dev, nbytes, misalign, dtype):
    """(base, win): `win` views `nbytes` of the uint8 allocation `base`
    starting `misalign` bytes past a 16-byte boundary, with >= 64 canary
    bytes before and after it."""
    base = torch.full((_CANARY + misalign + nbytes + _CANARY,), _CANARY_BYTE,
                      dtype=torch.uint8, device=dev)
    start = _CANARY + misalign
    win = base[start:start + nbytes].view(dtype)
    assert win.data_ptr() % 16 == misalign and win.is_contiguous()
    return base, win


def _canaries_intact(base, win):
    start = win.data_ptr() - base.data_ptr()
    end = start + win.numel() * win.element_size()
    assert start >= _CANARY and base.numel() - end >= _CANARY
    return bool((base[:start] == _CANARY_BYTE).all()) and \
        bool((base[end:] == _CANARY_BYTE).all())


@pytest.mark.parametrize("n,misalign",
                         [(n, 4) for n in _MISALIGNED_NS] +
                         [(n, 0) for n in _TAIL_NS])
def test_fill_misaligned_and_tails(ops, dev, n, misalign):
    base, t = _window(dev, 4 * n, misalign, torch.float32)
    ops.fill(t, 3.5)
    torch.cuda.synchronize()
    assert torch.equal(t, torch.full((n,), 3.5, device=dev))
    assert _canaries_intact(base, t)


@pytest.mark.parametrize("which", ["dst", "src", "both"])
@pytest.mark.parametrize("n", _MISALIGNED_NS)
def test_accumulate_misaligned(ops, dev, n, which):
    a0 = torch.rand(n, device=dev)
    b0 = torch.rand(n, device=dev)
    base, a = _window(dev, 4 * n, 4 if which in ("dst", "both") else 0,
                      torch.float32)
    _, b = _window(dev, 4 * n, 4 if which in ("src", "both") else 0,
                   torch.float32)
    a.copy_(a0)
    b.copy_(b0)
    ops.accumulate(a, b)
    torch.cuda.synchronize()
    assert torch.equal(a, a0 + b0)
    assert torch.equal(b, b0)
    assert _canaries_intact(base, a)


@pytest.mark.parametrize("n", _TAIL_NS)
def test_accumulate_aligned_tails(ops, dev, n):
    a0 = torch.rand(n, device=dev)
    b0 = torch.rand(n, device=dev)
    base, a = _window(dev, 4 * n, 0, torch.float32)
    a.copy_(a0)
    ops.accumulate(a, b0)
    torch.cuda.synchronize()
    assert torch.equal(a, a0 + b0)
    assert _canaries_intact(base, a)


@pytest.mark.parametrize("n", _MISALIGNED_NS)
def test_copy_kernel_misaligned_f32(ops, dev, n):
    src0 = torch.rand(n, device=dev)
    _, src = _window(dev, 4 * n, 4, torch.float32)
    base, dst = _window(dev, 4 * n, 4, torch.float32)
    src.copy_(src0)
    ops.copy_kernel(dst, src)
    torch.cuda.synchronize()
    assert torch.equal(dst, src0)
    assert _canaries_intact(base, dst)


@pytest.mark.parametrize("which", ["dst", "src", "both"])
@pytest.mark.parametrize("nbytes", [1, 15, 16, 17, 4099])
def test_copy_kernel_byte_misaligned(ops, dev, nbytes, which):
    g = torch.Generator(device="cpu").manual_seed(nbytes)
    src0 = torch.randint(0, 256, (nbytes,), generator=g,
                         dtype=torch.uint8).to(dev)
    _, src = _window(dev, nbytes, 1 if which in ("src", "both") else 0,
                     torch.uint8)
    base, dst = _window(dev, nbytes, 1 if which in ("dst", "both") else 0,
                        torch.uint8)
    src.copy_(src0)
    ops.copy_kernel(dst, src)
    torch.cuda.synchronize()
    assert torch.equal(dst, src0)
    assert _canaries_intact(base, dst)


@pytest.mark.parametrize("misalign", [0, 4])
@pytest.mark.parametrize("n", [2, 3, 5, 6, 7, 1026, 1027, (1 << 20) + 2,
                               (1 << 20) + 3])
def test_reduce_sum_tails_and_misaligned(ops, dev, n, misalign):
    """Integer-valued addends: every partial sum is an exact double, so the
    device reduction must EQUAL the float64 sum in any order. n % 4 in
    {2, 3} with n4 > 0 reaches the float4 body's tail lanes; the misaligned
    base reaches the scalar branch."""
    import numpy as np

    g = torch.Generator(device="cpu").manual_seed(n)
    host = torch.randint(-1000, 1001, (n,), generator=g).float()
    _, t = _window(dev, 4 * n, misalign, torch.float32)
    t.copy_(host)
    got = ops.reduce_sum(t)
    assert got == float(host.numpy().astype(np.float64).sum())


def test_reduce_sum_uniform_random_bound(ops, dev):
    """Non-integer addends: every float32 is an exact double and the
    reduction only ever adds doubles, so for ANY summation tree
    |got - exact| <= (n - 1) * u * sum|x| with u = 2^-53."""
    import math

    n = (1 << 20) + 3
    g = torch.Generator(device="cpu").manual_seed(20)
    host = torch.rand(n, generator=g)
    got = ops.reduce_sum(host.to(dev))
    xs = host.double().tolist()
    ref = math.fsum(xs)
    bound = n * 2.0 ** -53 * math.fsum(abs(x) for x in xs)
    print(f"reduce_sum err {abs(got - ref):.3e} bound {bound:.3e}")
    assert abs(got - ref) <= bound


@pytest.mark.parametrize("src_offset", [0, 4])
@pytest.mark.parametrize("cap", [1, 16])
@pytest.mark.parametrize("unroll", [1, 4, 5])
def test_copy_kernel_tuned_unrolled_body(ops, dev, unroll, cap, src_offset):
    """n16 = 9 * stride + 37 with stride = cap * 256 threads: the 4x body
    of the unrolled kernel runs twice (8 strides), then the remainder loop
    takes the ninth stride and the 37 leftovers; 5 tail bytes follow. A
    source 4 bytes off a 16-byte boundary takes the tuned launcher's
    fallback to the generic copy."""
    from hpc_patterns_amd._native import native

    hpk = native()
    n16 = 9 * (cap * 256) + 37
    nbytes = 16 * n16 + 5
    g = torch.Generator(device="cpu").manual_seed(unroll * 100 + cap)
    src0 = torch.randint(0, 256, (nbytes,), generator=g,
                         dtype=torch.uint8).to(dev)
    _, src = _window(dev, nbytes, src_offset, torch.uint8)
    base, dst = _window(dev, nbytes, 0, torch.uint8)
    src.copy_(src0)
    torch.cuda.synchronize()
    hpk.copy_kernel_tuned(dst.data_ptr(), src.data_ptr(), nbytes,
                          torch.cuda.current_stream().cuda_stream, unroll, cap)
    torch.cuda.synchronize()
    assert torch.equal(dst, src0)
    assert _canaries_intact(base, dst)


@pytest.mark.parametrize("nbytes", [1, 15])
def test_copy_kernel_aligned_tail_only(ops, dev, nbytes):
    """16-byte-aligned pointers and fewer than 16 bytes: no 16-byte item,
    so the generic launcher skips the body and launches the tail alone."""
    g = torch.Generator(device="cpu").manual_seed(nbytes)
    src0 = torch.randint(0, 256, (nbytes,), generator=g,
                         dtype=torch.uint8).to(dev)
    _, src = _window(dev, nbytes, 0, torch.uint8)
    base, dst = _window(dev, nbytes, 0, torch.uint8)
    src.copy_(src0)
    ops.copy_kernel(dst, src)
    torch.cuda.synchronize()
    assert torch.equal(dst, src0)
    assert _canaries_intact(base, dst)


@pytest.mark.parametrize("unroll", [1, 4, 5])
@pytest.mark.parametrize("nbytes", [5, 16, 21])
def test_copy_kernel_tuned_small_aligned(ops, dev, nbytes, unroll):
    """Aligned, grid_cap=1: 5 bytes is an empty body launch (n16 == 0, which
    the tuned launcher does not skip) plus a tail, 16 one item and no tail,
    21 both."""
    from hpc_patterns_amd._native import native

    g = torch.Generator(device="cpu").manual_seed(nbytes * 10 + unroll)
    src0 = torch.randint(0, 256, (nbytes,), generator=g,
                         dtype=torch.uint8).to(dev)
    _, src = _window(dev, nbytes, 0, torch.uint8)
    base, dst = _window(dev, nbytes, 0, torch.uint8)
    src.copy_(src0)
    torch.cuda.synchronize()
    native().copy_kernel_tuned(dst.data_ptr(), src.data_ptr(), nbytes,
                               torch.cuda.current_stream().cuda_stream,
                               unroll, 1)
    torch.cuda.synchronize()
    assert torch.equal(dst, src0)
    assert _canaries_intact(base, dst)


# Smallest size at which the reductions' clamp to 4096 blocks changes the
# grid (one block's worth past 4096 * 256 * 8) and a ragged end remains.
_REDUCE_CLAMP_N = 4096 * 256 * 8 + 256 * 8 + 3


def test_reduce_sum_i32_above_block_cap(ops, dev):
    from hpc_patterns_amd._native import native

    n = _REDUCE_CLAMP_N
    g = torch.Generator(device="cpu").manual_seed(7)
    host = torch.randint(-2 ** 30, 2 ** 30 + 1, (n,), generator=g,
                         dtype=torch.int32)
    t = host.to(dev)
    got = native().reduce_sum_i32(t.data_ptr(), n,
                                  torch.cuda.current_stream().cuda_stream)
    assert got == int(host.long().sum())


def test_reduce_sum_above_block_cap(ops, dev):
    """Integer-valued addends, as in test_reduce_sum_tails_and_misaligned:
    every partial sum is an exact double, so the result must be equal."""
    n = _REDUCE_CLAMP_N
    g = torch.Generator(device="cpu").manual_seed(8)
    host = torch.randint(-1000, 1001, (n,), generator=g)
    got = ops.reduce_sum(host.float().to(dev))
    assert got == float(int(host.sum()))


# The nontemporal streaming kernels (copy, fill, accumulate) cap their grid
# at 131072 blocks of 256 threads, one 16-byte item per thread per
# iteration — so they grid-stride only above 512 MiB, the regime of the
# flagship's 1 GiB D2D copy. This size gives SOME threads (3 blocks + 1) a
# second iteration, the rest one, plus a 12-byte tail.
_NT_GRID_CAP = 131072
_WRAP_NBYTES = _NT_GRID_CAP * 256 * 16 + 16 * (3 * 256 + 1) + 12


def test_copy_kernel_grid_stride_wrap(ops, dev):
    n = _WRAP_NBYTES // 4
    src = torch.rand(n, device=dev)
    base, dst = _window(dev, _WRAP_NBYTES, 0, torch.float32)
    ops.copy_kernel(dst, src)
    torch.cuda.synchronize()
    assert torch.equal(dst, src)
    assert _canaries_intact(base, dst)


def test_fill_grid_stride_wrap(ops, dev):
    n = _WRAP_NBYTES // 4
    base, t = _window(dev, _WRAP_NBYTES, 0, torch.float32)
    ops.fill(t, -2.25)
    torch.cuda.synchronize()
    assert bool((t == -2.25).all())
    assert t.numel() == n and _canaries_intact(base, t)


def test_accumulate_nt_grid_stride_wrap(ops, dev):
    from hpc_patterns_amd._native import native

    hpk = native()
    n = _WRAP_NBYTES // 4
    a0 = torch.rand(n, device=dev)
    b = torch.rand(n, device=dev)
    base, a = _window(dev, _WRAP_NBYTES, 0, torch.float32)
    a.copy_(a0)
    torch.cuda.synchronize()
    hpk.acc_f32_nt(a.data_ptr(), b.data_ptr(), n,
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    a0 += b  # the reference, in place: three 512 MiB buffers, not four
    assert torch.equal(a, a0)
    assert _canaries_intact(base, a)


# int32 twins (fill_i32 / acc_i32 / reduce_sum_i32): the miniapps' int
# instantiation, same size, alignment and tail grid as the float kernels.

@pytest.mark.parametrize("n,misalign",
                         [(n, 4) for n in _MISALIGNED_NS] +
                         [(n, 0) for n in _TAIL_NS])
def test_fill_i32(ops, dev, n, misalign):
    from hpc_patterns_amd._native import native

    base, t = _window(dev, 4 * n, misalign, torch.int32)
    native().fill_i32(t.data_ptr(), -123456789, n,
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(t, torch.full((n,), -123456789, dtype=torch.int32,
                                     device=dev))
    assert _canaries_intact(base, t)


@pytest.mark.parametrize("n,dst_mis,src_mis",
                         [(n, d, s) for n in _MISALIGNED_NS
                          for d, s in ((4, 0), (0, 4), (4, 4))] +
                         [(n, 0, 0) for n in _TAIL_NS])
def test_acc_i32(ops, dev, n, dst_mis, src_mis):
    from hpc_patterns_amd._native import native

    g = torch.Generator(device="cpu").manual_seed(n)
    a0 = torch.randint(-2 ** 30, 2 ** 30, (n,), generator=g,
                       dtype=torch.int32).to(dev)
    b0 = torch.randint(-2 ** 30, 2 ** 30, (n,), generator=g,
                       dtype=torch.int32).to(dev)
    base, a = _window(dev, 4 * n, dst_mis, torch.int32)
    _, b = _window(dev, 4 * n, src_mis, torch.int32)
    a.copy_(a0)
    b.copy_(b0)
    torch.cuda.synchronize()
    native().acc_i32(a.data_ptr(), b.data_ptr(), n,
                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(a, a0 + b0)  # |a0 + b0| < 2^31: no wrap either side
    assert _canaries_intact(base, a)


def test_reduce_sum_i32_needs_64bit_accumulator(ops, dev):
    from hpc_patterns_amd._native import native

    n = 1 << 20
    t = torch.full((n,), 2 ** 31 - 1, dtype=torch.int32, device=dev)
    got = native().reduce_sum_i32(t.data_ptr(), n,
                                  torch.cuda.current_stream().cuda_stream)
    assert got == n * (2 ** 31 - 1)


@pytest.mark.parametrize("n,misalign", [(1, 0), (1027, 4), ((1 << 20) + 3, 0)])
def test_reduce_sum_i32_random(ops, dev, n, misalign):
    from hpc_patterns_amd._native import native

    g = torch.Generator(device="cpu").manual_seed(n)
    host = torch.randint(-2 ** 30, 2 ** 30 + 1, (n,), generator=g,
                         dtype=torch.int32)
    _, t = _window(dev, 4 * n, misalign, torch.int32)
    t.copy_(host)
    got = native().reduce_sum_i32(t.data_ptr(), n,
                                  torch.cuda.current_stream().cuda_stream)
    assert got == int(host.long().sum())


@pytest.mark.parametrize("n", [1, 1000, 1 << 24])
def test_reduce_sum_exact_iota(ops, dev, n):
    t = torch.empty(n, dtype=torch.float32, device=dev)
    ops.iota(t)
    got = ops.reduce_sum(t)
    expected = ops.iota_checksum(n)
    assert got == expected  # exact: integer-valued addends in double


def test_reduce_sum_vs_torch(ops, dev):
    t = torch.rand(1 << 20, device=dev)
    got = ops.reduce_sum(t)
    ref = float(t.to(torch.float64).sum())
    assert abs(got - ref) < 1e-6 * max(abs(ref), 1.0)


def test_busy_wait_runs_and_scales(ops, dev):
    import time

    out = torch.empty(256, dtype=torch.float32, device=dev)
    # correctness: writes a finite value everywhere in [0, globalsize)
    ops.busy_wait(out, tripcount=10, globalsize=256)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()

    def timed(trip):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.busy_wait(out, tripcount=trip, globalsize=256)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    timed(1000)  # warm
    t1 = min(timed(2000) for _ in range(3))
    t4 = min(timed(8000) for _ in range(3))
    # linearity within 2x slack (the autotuner's model)
    assert 2.0 < t4 / t1 < 8.0, (t1, t4)


def test_busy_wait_mfma_runs(ops, dev):
    out = torch.empty(256, dtype=torch.float32, device=dev)
    ops.busy_wait_mfma(out, tripcount=1000, n_waves=4)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


def test_ops_reject_wrong_dtype(ops, dev):
    t = torch.empty(8, dtype=torch.float64, device=dev)
    with pytest.raises(TypeError):
        ops.fill(t, 0.0)


def test_interop_torch_allocator_shared_with_hip_kernels(ops, dev):
    """The suite's runtime-interop capability (reference
    sycl_omp_ze_interopt): torch's caching allocator, torch streams and the
    raw HIP kernels drive the same memory with no copies."""
    s = torch.cuda.Stream()
    t = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    with torch.cuda.stream(s):
        ops.fill(t, 7.0, stream=s)        # native kernel on torch stream
        u = t * 2.0                        # torch op, same stream, same memory
    s.synchronize()
    assert torch.equal(u, torch.full_like(t, 14.0))


@pytest.mark.parametrize("unroll,cap", [(1, 4096), (4, 65536)])
def test_copy_kernel_tuned(ops, dev, unroll, cap):
    from hpc_patterns_amd._native import native

    hpk = native()
    n = (1 << 20) + 5
    src = torch.rand(n, device=dev)
    dst = torch.zeros_like(src)
    torch.cuda.synchronize()
    hpk.copy_kernel_tuned(dst.data_ptr(), src.data_ptr(), n * 4,
                          torch.cuda.current_stream().cuda_stream, unroll, cap)
    torch.cuda.synchronize()
    assert torch.equal(dst, src)


def test_roctx_markers_noop_safe(ops, dev):
    from hpc_patterns_amd._native import native

    hpk = native()
    hpk.trace_push("test_range")
    hpk.trace_mark("test_mark")
    hpk.trace_pop()


def test_sdma_explicit_engine_copy(ops, dev):
    """Explicit SDMA-engine copies: correctness + handle lifecycle."""
    from hpc_patterns_amd._native import native

    hpk = native()
    n_engines = hpk.sdma_num_engines(0)
    assert n_engines >= 1, "MI355X should expose SDMA engines"
    nbytes = 32 << 20
    host = hpk.host_malloc(nbytes)
    dev_buf = hpk.hip_malloc(nbytes)
    host2 = hpk.host_malloc(nbytes)
    # pattern into host via a device round-trip
    t = torch.arange(nbytes // 4, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    hpk.memcpy_async(host, t.data_ptr(), nbytes, 0)
    hpk.stream_synchronize(0)
    # H2D on engine 0, D2H on engine 1 (or 0 if single-engine)
    h1 = hpk.sdma_copy_begin(dev_buf, host, nbytes, 0, 0)
    hpk.sdma_wait(h1)
    h2 = hpk.sdma_copy_begin(host2, dev_buf, nbytes, 0,
                             1 if n_engines >= 2 else 0)
    hpk.sdma_wait(h2)
    out = torch.empty_like(t)
    hpk.memcpy_async(out.data_ptr(), host2, nbytes, 0)
    hpk.stream_synchronize(0)
    assert torch.equal(out, t)
    for p in (host, host2):
        hpk.host_free(p)
    hpk.hip_free(dev_buf)


def test_fill_large_nontemporal_path(ops, dev):
    # >32 MB exercises the nontemporal-store fill variant
    n = (64 << 20) // 4 + 3
    t = torch.empty(n, dtype=torch.float32, device=dev)
    ops.fill(t, -2.25)
    torch.cuda.synchronize()
    assert torch.all(t == -2.25)


def test_copy_large_nontemporal_path(ops, dev):
    n = (64 << 20) // 4 + 5
    src = torch.rand(n, device=dev)
    dst = torch.zeros_like(src)
    ops.copy_kernel(dst, src)
    torch.cuda.synchronize()
    assert torch.equal(dst, src)


def test_sdma_engine_pair_query(ops, dev):
    from hpc_patterns_amd._native import native

    hpk = native()
    # same-device pair: must not crash; >=0 engines
    n = hpk.sdma_num_engines_pair(0, 0)
    assert n >= 0


def test_accumulate_nt_variant(ops, dev):
    from hpc_patterns_amd._native import native

    hpk = native()
    n = (48 << 20) // 4  # beyond-L3 class size, 16B aligned
    a = torch.rand(n, device=dev)
    b = torch.rand(n, device=dev)
    ref = a + b
    torch.cuda.synchronize()
    hpk.acc_f32_nt(a.data_ptr(), b.data_ptr(), n,
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(a, ref)


@pytest.mark.parametrize("mb", [40, 64])
def test_nt_kernels_coherence_stress(ops, dev, mb):
    """Hunt cache-hint staleness in the NT performance kernels: write fresh
    data with NORMAL stores (dirty L2), immediately run the NT copy /
    accumulate on it, verify exactly. Repeated at L2-window sizes — if NT
    loads/stores bypassed coherence this flakes (cf. the reverted NT
    reduction, profiles/README r24 note)."""
    from hpc_patterns_amd._native import native

    hpk = native()
    n = (mb << 20) // 4
    s = torch.cuda.current_stream().cuda_stream
    for trial in range(4):
        src = torch.rand(n, device=dev)          # normal stores
        dst = torch.zeros(n, device=dev)         # normal stores (dirty zeros)
        torch.cuda.synchronize()
        ops.copy_kernel(dst, src)                # NT path at these sizes
        torch.cuda.synchronize()
        assert torch.equal(dst, src), f"NT copy stale data (trial {trial})"

        a = torch.rand(n, device=dev)
        b = torch.rand(n, device=dev)
        ref = a + b
        torch.cuda.synchronize()
        hpk.acc_f32_nt(a.data_ptr(), b.data_ptr(), n, s)
        torch.cuda.synchronize()
        assert torch.equal(a, ref), f"NT accumulate stale data (trial {trial})"
        del src, dst, a, b, ref


def test_staged_pageable_copy_roundtrip(ops, dev):
    """Pipelined pinned-staging copies for pageable memory (staged.hip):
    pageable->device on engine 0, device->pageable on engine 1, exact."""
    import numpy as np

    from hpc_patterns_amd._native import native

    hpk = native()
    n = (40 << 20) // 4 + 13  # 40MB + odd tail, several 8MB chunks
    src = np.random.rand(n).astype(np.float32)  # pageable numpy memory
    out = np.zeros_like(src)
    dbuf = hpk.hip_malloc(n * 4)
    hpk.staged_copy(dbuf, src.ctypes.data, n * 4, 0, 0, True)
    hpk.staged_copy(out.ctypes.data, dbuf, n * 4, 0,
                    1 if hpk.sdma_num_engines(0) >= 2 else 0, False)
    assert np.array_equal(out, src)
    hpk.hip_free(dbuf)


@pytest.mark.parametrize("nbytes", [1024, 8 << 20, (8 << 20) + 4,
                                    (16 << 20) - 4, 65 << 20])
def test_staged_copy_chunk_boundaries(ops, dev, nbytes):
    """staged.hip chunk/thread-split logic at boundary sizes (8 MiB chunks,
    4-way threading beyond 64 MiB)."""
    import numpy as np

    from hpc_patterns_amd._native import native

    hpk = native()
    n = nbytes // 4
    src = np.random.rand(n).astype(np.float32)
    out = np.zeros_like(src)
    dbuf = hpk.hip_malloc(nbytes)
    hpk.staged_copy(dbuf, src.ctypes.data, nbytes, 0, 0, True)
    hpk.staged_copy(out.ctypes.data, dbuf, nbytes, 0, 0, False)
    assert np.array_equal(out, src), nbytes
    hpk.hip_free(dbuf)


# ---------------------------------------------------------------------------
# K7 (r2): LDS-tiled bf16 MFMA GEMM
# ---------------------------------------------------------------------------

def test_gemm_bf16_identity_asymmetric():
    """A = I with an ASYMMETRIC B catches any row/col-swapped fragment or
    epilogue mapping (the guide's A=I-check): C = I @ B^T = B^T exactly."""
    from hpc_patterns_amd import ops

    torch.manual_seed(7)
    m = n = k = 128
    a = torch.eye(m, k, device="cuda").to(torch.bfloat16)
    b = torch.randn(n, k, device="cuda").to(torch.bfloat16)
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_bf16(c, a, b)
    torch.cuda.synchronize()
    assert torch.equal(c, b.t().float()), (c - b.t().float()).abs().max()


def test_gemm_bf16_exact_integers():
    """Small-integer payloads make every product and partial sum exactly
    representable in fp32, so the MFMA result must EQUAL the torch fp32
    reference bit for bit regardless of summation order."""
    from hpc_patterns_amd import ops

    g = torch.Generator(device="cpu").manual_seed(11)
    m, n, k = 256, 384, 512
    a = torch.randint(-4, 5, (m, k), generator=g).to(torch.bfloat16).cuda()
    b = torch.randint(-4, 5, (n, k), generator=g).to(torch.bfloat16).cuda()
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_bf16(c, a, b)
    ref = torch.matmul(a.float(), b.float().t())
    torch.cuda.synchronize()
    assert torch.equal(c, ref), (c - ref).abs().max()


@pytest.mark.parametrize("swizzle", [True, False])
def test_gemm_bf16_large_close(swizzle):
    """1024^3 random normal: products of bf16 values are exact in fp32, so
    the only divergence from the torch fp32 reference is summation order —
    tight allclose."""
    from hpc_patterns_amd import ops

    torch.manual_seed(3)
    m = n = k = 1024
    a = torch.randn(m, k, device="cuda").to(torch.bfloat16)
    b = torch.randn(n, k, device="cuda").to(torch.bfloat16)
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_bf16(c, a, b, xcd_swizzle=swizzle)
    ref = torch.matmul(a.float(), b.float().t())
    torch.cuda.synchronize()
    assert torch.allclose(c, ref, rtol=1e-4, atol=1e-3), \
        (c - ref).abs().max()


def test_gemm_bf16_shape_guards():
    from hpc_patterns_amd import ops

    a = torch.zeros(128, 64, dtype=torch.bfloat16, device="cuda")
    b = torch.zeros(128, 64, dtype=torch.bfloat16, device="cuda")
    c = torch.zeros(128, 128, dtype=torch.float32, device="cuda")
    ops.gemm_bf16(c, a, b)  # minimal legal shape
    with pytest.raises((RuntimeError, ValueError)):
        ops.gemm_bf16(c, a[:, :32].contiguous(), b[:, :32].contiguous())
    with pytest.raises(TypeError):
        ops.gemm_bf16(c, a.float(), b)


def test_gemm_bf16_db_variant_exact():
    """HPK_GEMM_VARIANT=db (double-buffered LDS + raw barriers + counted
    vmcnt) must be bitwise-identical to the reference on integer payloads
    — race-screened 30x at two shapes in profiles/gemm_db_r2.log; this
    keeps one exact check in CI."""
    import os

    from hpc_patterns_amd import ops

    os.environ["HPK_GEMM_VARIANT"] = "db"
    try:
        g = torch.Generator(device="cpu").manual_seed(23)
        m, n, k = 256, 256, 640
        a = torch.randint(-4, 5, (m, k), generator=g).to(torch.bfloat16).cuda()
        b = torch.randint(-4, 5, (n, k), generator=g).to(torch.bfloat16).cuda()
        c = torch.empty(m, n, dtype=torch.float32, device="cuda")
        ops.gemm_bf16(c, a, b)
        ref = torch.matmul(a.float(), b.float().t())
        torch.cuda.synchronize()
        assert torch.equal(c, ref)
    finally:
        del os.environ["HPK_GEMM_VARIANT"]


def test_gemm_fp8_exact_integers():
    """fp8 e4m3 twin: {-4..4} are exactly representable in e4m3, so the
    result must EQUAL the torch fp32 reference bitwise."""
    from hpc_patterns_amd import ops

    g = torch.Generator(device="cpu").manual_seed(17)
    m, n, k = 256, 384, 512
    a = torch.randint(-4, 5, (m, k), generator=g).to(torch.float8_e4m3fn).cuda()
    b = torch.randint(-4, 5, (n, k), generator=g).to(torch.float8_e4m3fn).cuda()
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_fp8(c, a, b)
    ref = torch.matmul(a.float(), b.float().t())
    torch.cuda.synchronize()
    assert torch.equal(c, ref), (c - ref).abs().max()


def test_gemm_fp8_identity_asymmetric():
    from hpc_patterns_amd import ops

    torch.manual_seed(5)
    m = n = k = 128
    a = torch.eye(m, k, device="cuda").to(torch.float8_e4m3fn)
    b = (torch.randint(-4, 5, (n, k)).float()).to(torch.float8_e4m3fn).cuda()
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_fp8(c, a, b)
    torch.cuda.synchronize()
    assert torch.equal(c, b.float().t())


def test_gemm_bf16_8phase_exact_integers():
    """The deep-pipelined 256^2 8-phase kernel (default for shapes with
    M,N % 256 == 0 and K % 128 == 0): bitwise equality on integer payloads
    at an eligible shape — plus the identity check at 256^2."""
    from hpc_patterns_amd import ops

    g = torch.Generator(device="cpu").manual_seed(29)
    m, n, k = 512, 256, 640
    a = torch.randint(-3, 4, (m, k), generator=g).to(torch.bfloat16).cuda()
    b = torch.randint(-3, 4, (n, k), generator=g).to(torch.bfloat16).cuda()
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_bf16(c, a, b)
    ref = torch.matmul(a.float(), b.float().t())
    torch.cuda.synchronize()
    assert torch.equal(c, ref), (c - ref).abs().max()
    ai = torch.eye(256, 256, device="cuda").to(torch.bfloat16)
    bi = torch.randn(256, 256, device="cuda").to(torch.bfloat16)
    ci = torch.empty(256, 256, dtype=torch.float32, device="cuda")
    ops.gemm_bf16(ci, ai, bi)
    torch.cuda.synchronize()
    assert torch.equal(ci, bi.t().float())


def test_gemm_fp8_8phase_exact_integers(monkeypatch):
    """fp8 8-phase pipeline (pinned via HPK_GEMM_VARIANT — 256-divisible
    shapes now default to the 32x32x64 kernel): bitwise equality."""
    from hpc_patterns_amd import ops

    monkeypatch.setenv("HPK_GEMM_VARIANT", "8ph")

    g = torch.Generator(device="cpu").manual_seed(37)
    m, n, k = 256, 512, 640
    a = torch.randint(-3, 4, (m, k), generator=g).to(torch.float8_e4m3fn).cuda()
    b = torch.randint(-3, 4, (n, k), generator=g).to(torch.float8_e4m3fn).cuda()
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_fp8(c, a, b)
    ref = torch.matmul(a.float(), b.float().t())
    torch.cuda.synchronize()
    assert torch.equal(c, ref), (c - ref).abs().max()


def _mx_ref(a, b, a_scale, b_scale):
    """fp32 reference of the MX semantics: dequant per 32-block, matmul."""
    af = a.float() * (2.0 ** (a_scale.float() - 127)).repeat_interleave(32, 1)
    bf = b.float() * (2.0 ** (b_scale.float() - 127)).repeat_interleave(32, 1)
    return torch.matmul(af, bf.t())


def test_gemm_mxfp8_unit_scales_exact():
    """All scales 127 (=1.0): must equal the plain-fp8 exact result."""
    from hpc_patterns_amd import ops

    g = torch.Generator(device="cpu").manual_seed(41)
    m, n, k = 128, 256, 384
    a = torch.randint(-4, 5, (m, k), generator=g).to(torch.float8_e4m3fn).cuda()
    b = torch.randint(-4, 5, (n, k), generator=g).to(torch.float8_e4m3fn).cuda()
    sa = torch.full((m, k // 32), 127, dtype=torch.uint8, device="cuda")
    sb = torch.full((n, k // 32), 127, dtype=torch.uint8, device="cuda")
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_mxfp8(c, a, b, sa, sb)
    ref = torch.matmul(a.float(), b.float().t())
    torch.cuda.synchronize()
    assert torch.equal(c, ref), (c - ref).abs().max()


def test_gemm_mxfp8_power_of_two_scales_exact():
    """Random per-block power-of-2 scales: products stay exact in fp32, so
    the HW-dequant result must EQUAL the fp32 reference bitwise."""
    from hpc_patterns_amd import ops

    g = torch.Generator(device="cpu").manual_seed(43)
    m, n, k = 256, 128, 512
    a = torch.randint(-3, 4, (m, k), generator=g).to(torch.float8_e4m3fn).cuda()
    b = torch.randint(-3, 4, (n, k), generator=g).to(torch.float8_e4m3fn).cuda()
    sa = torch.randint(124, 131, (m, k // 32), generator=g,
                       dtype=torch.uint8).cuda()
    sb = torch.randint(124, 131, (n, k // 32), generator=g,
                       dtype=torch.uint8).cuda()
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_mxfp8(c, a, b, sa, sb)
    ref = _mx_ref(a, b, sa, sb)
    torch.cuda.synchronize()
    assert torch.equal(c, ref), (c - ref).abs().max()


def test_gemm_mxfp8_identity():
    from hpc_patterns_amd import ops

    m = n = k = 128
    a = torch.eye(m, k, device="cuda").to(torch.float8_e4m3fn)
    b = torch.randint(-4, 5, (n, k)).float().to(torch.float8_e4m3fn).cuda()
    sa = torch.full((m, k // 32), 127, dtype=torch.uint8, device="cuda")
    sb = torch.full((n, k // 32), 127, dtype=torch.uint8, device="cuda")
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_mxfp8(c, a, b, sa, sb)
    torch.cuda.synchronize()
    assert torch.equal(c, b.float().t())


def test_gemm_mxfp8_large_square_exact():
    """256-divisible shape with random power-of-2 scales (covers the tile
    shapes the removed deep-pipelined variant used to take)."""
    from hpc_patterns_amd import ops

    g = torch.Generator(device="cpu").manual_seed(47)
    m, n, k = 256, 256, 512
    a = torch.randint(-3, 4, (m, k), generator=g).to(torch.float8_e4m3fn).cuda()
    b = torch.randint(-3, 4, (n, k), generator=g).to(torch.float8_e4m3fn).cuda()
    sa = torch.randint(124, 131, (m, k // 32), generator=g,
                       dtype=torch.uint8).cuda()
    sb = torch.randint(124, 131, (n, k // 32), generator=g,
                       dtype=torch.uint8).cuda()
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_mxfp8(c, a, b, sa, sb)
    ref = _mx_ref(a, b, sa, sb)
    torch.cuda.synchronize()
    assert torch.equal(c, ref), (c - ref).abs().max()


def test_gemm_i8_exact():
    """int8 GEMM: int32 accumulate is exact by construction — full-range
    payloads must EQUAL the int64 torch reference."""
    from hpc_patterns_amd import ops

    g = torch.Generator(device="cpu").manual_seed(53)
    m, n, k = 256, 384, 512
    a = torch.randint(-128, 128, (m, k), generator=g, dtype=torch.int8).cuda()
    b = torch.randint(-128, 128, (n, k), generator=g, dtype=torch.int8).cuda()
    c = torch.empty(m, n, dtype=torch.int32, device="cuda")
    ops.gemm_i8(c, a, b)
    # torch has no int CUDA matmul — exact reference on host
    ref = torch.matmul(a.cpu().long(), b.cpu().long().t()).to(torch.int32).cuda()
    torch.cuda.synchronize()
    assert torch.equal(c, ref), (c - ref).abs().max()


def test_gemm_i8_identity():
    from hpc_patterns_amd import ops

    m = n = k = 128
    a = torch.eye(m, k).to(torch.int8).cuda()
    b = torch.randint(-5, 6, (n, k), dtype=torch.int8).cuda()
    c = torch.empty(m, n, dtype=torch.int32, device="cuda")
    ops.gemm_i8(c, a, b)
    torch.cuda.synchronize()
    assert torch.equal(c, b.int().t())


def test_gemm_i8_8phase_exact(monkeypatch):
    """The 8-phase 16x16x64 i8 pipeline (pinned via HPK_GEMM_VARIANT —
    256-divisible shapes now default to the 32x32x32 kernel)."""
    from hpc_patterns_amd import ops

    monkeypatch.setenv("HPK_GEMM_VARIANT", "8ph")

    g = torch.Generator(device="cpu").manual_seed(61)
    m, n, k = 256, 512, 512
    ah = torch.randint(-128, 128, (m, k), generator=g, dtype=torch.int8)
    bh = torch.randint(-128, 128, (n, k), generator=g, dtype=torch.int8)
    c = torch.empty(m, n, dtype=torch.int32, device="cuda")
    ops.gemm_i8(c, ah.cuda(), bh.cuda())
    ref = torch.matmul(ah.long(), bh.long().t()).to(torch.int32).cuda()
    torch.cuda.synchronize()
    assert torch.equal(c, ref)


# ---------------------------------------------------------------------------
# matmul_nt — arbitrary-shape front door (zero-padding dispatch)
# ---------------------------------------------------------------------------

def test_matmul_nt_bf16_odd_shapes_exact():
    """Odd (non-tile-multiple) shapes through the padding path: small
    integers keep everything exact, so the sliced result must EQUAL the
    torch fp32 reference."""
    from hpc_patterns_amd import ops

    g = torch.Generator(device="cpu").manual_seed(71)
    for m, n, k in ((300, 520, 736), (1, 1, 64), (257, 129, 192)):
        a = torch.randint(-4, 5, (m, k), generator=g).to(torch.bfloat16).cuda()
        b = torch.randint(-4, 5, (n, k), generator=g).to(torch.bfloat16).cuda()
        c = ops.matmul_nt(a, b)
        ref = torch.matmul(a.float(), b.float().t())
        torch.cuda.synchronize()
        assert c.shape == (m, n) and c.dtype == torch.float32
        assert torch.equal(c, ref), (m, n, k)


def test_matmul_nt_i8_odd_shapes_exact():
    from hpc_patterns_amd import ops

    g = torch.Generator(device="cpu").manual_seed(73)
    m, n, k = 100, 300, 700
    ah = torch.randint(-128, 128, (m, k), generator=g, dtype=torch.int8)
    bh = torch.randint(-128, 128, (n, k), generator=g, dtype=torch.int8)
    c = ops.matmul_nt(ah.cuda(), bh.cuda())
    ref = torch.matmul(ah.long(), bh.long().t()).to(torch.int32).cuda()
    torch.cuda.synchronize()
    assert c.shape == (m, n) and c.dtype == torch.int32
    assert torch.equal(c, ref)


def test_matmul_nt_fp8_and_mx_odd_shapes():
    from hpc_patterns_amd import ops

    g = torch.Generator(device="cpu").manual_seed(79)
    m, n, k = 200, 136, 160
    a = torch.randint(-4, 5, (m, k), generator=g).float() \
        .to(torch.float8_e4m3fn).cuda()
    b = torch.randint(-4, 5, (n, k), generator=g).float() \
        .to(torch.float8_e4m3fn).cuda()
    ref = torch.matmul(a.float(), b.float().t())
    c = ops.matmul_nt(a, b)
    torch.cuda.synchronize()
    assert torch.equal(c, ref)
    # mx path: unit scales (127 = 2^0) must reproduce the plain result
    s_a = torch.full((m, k // 32), 127, dtype=torch.uint8, device="cuda")
    s_b = torch.full((n, k // 32), 127, dtype=torch.uint8, device="cuda")
    cmx = ops.matmul_nt(a, b, a_scale=s_a, b_scale=s_b)
    torch.cuda.synchronize()
    assert torch.equal(cmx, ref)


def test_matmul_nt_aligned_no_copy():
    """Tile-multiple shapes skip padding entirely: result tensor IS the
    kernel's output buffer (no slice copy)."""
    from hpc_patterns_amd import ops

    torch.manual_seed(83)
    a = torch.randn(256, 128, device="cuda").to(torch.bfloat16)
    b = torch.randn(256, 128, device="cuda").to(torch.bfloat16)
    c = ops.matmul_nt(a, b)
    torch.cuda.synchronize()
    ref = torch.matmul(a.float(), b.float().t())
    assert c.is_contiguous() and c.shape == (256, 256)
    assert torch.allclose(c, ref, rtol=1e-3, atol=1e-3)


def test_gemm_grouped_order_exact(monkeypatch):
    """The L2-aware grouped tile order (HPK_GEMM_GROUP) is a pure launch
    reordering: results must stay bitwise identical, including grids whose
    tiles_n is not a multiple of the band width (partial last band)."""
    from hpc_patterns_amd import ops

    g = torch.Generator(device="cpu").manual_seed(89)
    m, n, k = 768, 1792, 512  # 8ph grid: 3 x 7 tiles
    a = torch.randint(-4, 5, (m, k), generator=g).to(torch.bfloat16).cuda()
    b = torch.randint(-4, 5, (n, k), generator=g).to(torch.bfloat16).cuda()
    ref = torch.matmul(a.float(), b.float().t())
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    for grp in ("2", "4", "8", "16", "64"):
        monkeypatch.setenv("HPK_GEMM_GROUP", grp)
        ops.gemm_bf16(c, a, b)
        torch.cuda.synchronize()
        assert torch.equal(c, ref), grp


def test_gemm_mxfp8_grouped_order_exact(monkeypatch):
    from hpc_patterns_amd import ops

    g = torch.Generator(device="cpu").manual_seed(97)
    m, n, k = 384, 1152, 256  # 128-tile grid: 3 x 9
    a = torch.randint(-4, 5, (m, k), generator=g).float() \
        .to(torch.float8_e4m3fn).cuda()
    b = torch.randint(-4, 5, (n, k), generator=g).float() \
        .to(torch.float8_e4m3fn).cuda()
    sa = torch.full((m, k // 32), 127, dtype=torch.uint8, device="cuda")
    sb = torch.full((n, k // 32), 127, dtype=torch.uint8, device="cuda")
    ref = torch.matmul(a.float(), b.float().t())
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    for grp in ("4", "16", "32"):
        monkeypatch.setenv("HPK_GEMM_GROUP", grp)
        ops.gemm_mxfp8(c, a, b, sa, sb)
        torch.cuda.synchronize()
        assert torch.equal(c, ref), grp


# ---------------------------------------------------------------------------
# K7-mx4: block-scaled OCP MX-fp4 GEMM (4x rate class)
# ---------------------------------------------------------------------------

def _mx4_operands(m, n, k, seed):
    """Random exactly-representable e2m1 payloads + packed forms."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    from hpc_patterns_amd import ops

    vals = torch.tensor([0., 0.5, -0.5, 1., -1., 1.5, -1.5, 2., -2.])
    fa = vals[torch.randint(0, 9, (m, k), generator=g)]
    fb = vals[torch.randint(0, 9, (n, k), generator=g)]
    return fa, fb, ops.e2m1_pack(fa).cuda(), ops.e2m1_pack(fb).cuda()


def test_gemm_mxfp4_unit_scales_exact():
    """Products/sums of e2m1 values at these magnitudes are exact in fp32:
    the result must EQUAL the fp32 reference bitwise."""
    from hpc_patterns_amd import ops

    m, n, k = 128, 256, 384
    fa, fb, pa, pb = _mx4_operands(m, n, k, 113)
    sa = torch.full((m, k // 32), 127, dtype=torch.uint8, device="cuda")
    sb = torch.full((n, k // 32), 127, dtype=torch.uint8, device="cuda")
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_mxfp4(c, pa, pb, sa, sb)
    ref = torch.matmul(fa, fb.t()).cuda()
    torch.cuda.synchronize()
    assert torch.equal(c, ref), (c - ref).abs().max()


def test_gemm_mxfp4_identity():
    """A = packed identity with an ASYMMETRIC B: C = B^T exactly."""
    from hpc_patterns_amd import ops

    m = n = k = 128
    fa = torch.eye(m, k)
    g = torch.Generator(device="cpu").manual_seed(127)
    vals = torch.tensor([0., 0.5, -0.5, 1., -1., 1.5, -1.5, 2., -2.])
    fb = vals[torch.randint(0, 9, (n, k), generator=g)]
    pa, pb = ops.e2m1_pack(fa).cuda(), ops.e2m1_pack(fb).cuda()
    sa = torch.full((m, k // 32), 127, dtype=torch.uint8, device="cuda")
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_mxfp4(c, pa, pb, sa, sa.clone())
    torch.cuda.synchronize()
    assert torch.equal(c, fb.t().cuda()), (c - fb.t().cuda()).abs().max()


def test_gemm_mxfp4_power_of_two_scales_exact():
    """Random e8m0 scales near 127: dequant is exact power-of-2 scaling,
    still bitwise-equal to the fp32 reference."""
    from hpc_patterns_amd import ops

    m, n, k = 256, 128, 256
    fa, fb, pa, pb = _mx4_operands(m, n, k, 131)
    g = torch.Generator(device="cpu").manual_seed(137)
    sa = torch.randint(124, 131, (m, k // 32), generator=g,
                       dtype=torch.int16).to(torch.uint8)
    sb = torch.randint(124, 131, (n, k // 32), generator=g,
                       dtype=torch.int16).to(torch.uint8)
    da = fa * torch.pow(2.0, sa.float() - 127).repeat_interleave(32, dim=1)
    db = fb * torch.pow(2.0, sb.float() - 127).repeat_interleave(32, dim=1)
    ref = torch.matmul(da, db.t()).cuda()
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_mxfp4(c, pa, pb, sa.cuda(), sb.cuda())
    torch.cuda.synchronize()
    assert torch.equal(c, ref), (c - ref).abs().max()


def test_gemm_mxfp4_large_square_exact():
    from hpc_patterns_amd import ops

    m = n = k = 1024
    fa, fb, pa, pb = _mx4_operands(m, n, k, 139)
    sa = torch.full((m, k // 32), 127, dtype=torch.uint8, device="cuda")
    sb = torch.full((n, k // 32), 127, dtype=torch.uint8, device="cuda")
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_mxfp4(c, pa, pb, sa, sb)
    ref = torch.matmul(fa, fb.t()).cuda()
    torch.cuda.synchronize()
    assert torch.equal(c, ref)


def test_gemm_mxfp4_grouped_order_exact(monkeypatch):
    from hpc_patterns_amd import ops

    m, n, k = 384, 1152, 256  # 3 x 9 tile grid (partial bands)
    fa, fb, pa, pb = _mx4_operands(m, n, k, 149)
    sa = torch.full((m, k // 32), 127, dtype=torch.uint8, device="cuda")
    sb = torch.full((n, k // 32), 127, dtype=torch.uint8, device="cuda")
    ref = torch.matmul(fa, fb.t()).cuda()
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    for grp in ("4", "16", "32"):
        monkeypatch.setenv("HPK_GEMM_GROUP", grp)
        ops.gemm_mxfp4(c, pa, pb, sa, sb)
        torch.cuda.synchronize()
        assert torch.equal(c, ref), grp


def test_gemm_mxfp4_256tile_power_of_two_scales_exact():
    """256-divisible shapes take the 256^2-tile 32x32x64 kernel (the
    default fast path): full exactness incl. its size-4 glds scale
    staging with non-uniform scales."""
    from hpc_patterns_amd import ops

    m, n, k = 256, 512, 384
    fa, fb, pa, pb = _mx4_operands(m, n, k, 151)
    g = torch.Generator(device="cpu").manual_seed(157)
    sa = torch.randint(124, 131, (m, k // 32), generator=g,
                       dtype=torch.int16).to(torch.uint8)
    sb = torch.randint(124, 131, (n, k // 32), generator=g,
                       dtype=torch.int16).to(torch.uint8)
    da = fa * torch.pow(2.0, sa.float() - 127).repeat_interleave(32, dim=1)
    db = fb * torch.pow(2.0, sb.float() - 127).repeat_interleave(32, dim=1)
    ref = torch.matmul(da, db.t()).cuda()
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_mxfp4(c, pa, pb, sa.cuda(), sb.cuda())
    torch.cuda.synchronize()
    assert torch.equal(c, ref), (c - ref).abs().max()


def test_matmul_nt_mxfp4_odd_shapes_exact():
    """Packed-fp4 through the matmul_nt padding path: zero nibbles pad
    exactly, scales pad with 127."""
    from hpc_patterns_amd import ops

    m, n, k = 200, 136, 192  # odd vs the 256/128 fast-path multiples
    fa, fb, pa, pb = _mx4_operands(m, n, k, 167)
    sa = torch.full((m, k // 32), 127, dtype=torch.uint8, device="cuda")
    sb = torch.full((n, k // 32), 127, dtype=torch.uint8, device="cuda")
    c = ops.matmul_nt(pa, pb, a_scale=sa, b_scale=sb)
    ref = torch.matmul(fa, fb.t()).cuda()
    torch.cuda.synchronize()
    assert c.shape == (m, n) and torch.equal(c, ref)


def test_gemm_mxfp8_256tile_power_of_two_scales_exact():
    """256-divisible shapes take the 256^2-tile 32x32x64 mx8 kernel (the
    r2-follow-up default): full exactness incl. non-uniform scales."""
    from hpc_patterns_amd import ops

    g = torch.Generator(device="cpu").manual_seed(173)
    m, n, k = 256, 512, 384
    fa = torch.randint(-4, 5, (m, k), generator=g).float()
    fb = torch.randint(-4, 5, (n, k), generator=g).float()
    a = fa.to(torch.float8_e4m3fn).cuda()
    b = fb.to(torch.float8_e4m3fn).cuda()
    sa = torch.randint(124, 131, (m, k // 32), generator=g,
                       dtype=torch.int16).to(torch.uint8)
    sb = torch.randint(124, 131, (n, k // 32), generator=g,
                       dtype=torch.int16).to(torch.uint8)
    da = fa * torch.pow(2.0, sa.float() - 127).repeat_interleave(32, dim=1)
    db = fb * torch.pow(2.0, sb.float() - 127).repeat_interleave(32, dim=1)
    ref = torch.matmul(da, db.t()).cuda()
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_mxfp8(c, a, b, sa.cuda(), sb.cuda())
    torch.cuda.synchronize()
    assert torch.equal(c, ref), (c - ref).abs().max()


def test_gemm_fp8_32x32_default_exact():
    """Plain fp8 at 256-divisible shapes defaults to the 256^2 32x32x64
    scaled-MFMA kernel with hardcoded x1.0 scales: bitwise equality."""
    from hpc_patterns_amd import ops

    g = torch.Generator(device="cpu").manual_seed(179)
    m, n, k = 256, 512, 640
    a = torch.randint(-3, 4, (m, k), generator=g).to(torch.float8_e4m3fn).cuda()
    b = torch.randint(-3, 4, (n, k), generator=g).to(torch.float8_e4m3fn).cuda()
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_fp8(c, a, b)
    ref = torch.matmul(a.float(), b.float().t())
    torch.cuda.synchronize()
    assert torch.equal(c, ref), (c - ref).abs().max()


def test_gemm_i8_32x32_variant_exact(monkeypatch):
    """The selectable 256^2 32x32x32 i8 kernel (HPK_GEMM_VARIANT=32 — a
    measured perf negative, kept for the design-space record): full-range
    int8, exact int32, bitwise vs the int64 host reference."""
    from hpc_patterns_amd import ops

    monkeypatch.setenv("HPK_GEMM_VARIANT", "32")

    g = torch.Generator(device="cpu").manual_seed(181)
    m, n, k = 256, 512, 384
    ah = torch.randint(-128, 128, (m, k), generator=g, dtype=torch.int8)
    bh = torch.randint(-128, 128, (n, k), generator=g, dtype=torch.int8)
    c = torch.empty(m, n, dtype=torch.int32, device="cuda")
    ops.gemm_i8(c, ah.cuda(), bh.cuda())
    ref = torch.matmul(ah.long(), bh.long().t()).to(torch.int32).cuda()
    torch.cuda.synchronize()
    assert torch.equal(c, ref)


def test_gemm_mxfp4_32h_variant_exact(monkeypatch):
    """The 256x128 occupancy-experiment kernel (HPK_MX4_WAVES=32h, a
    measured perf negative kept as the design-space record): exactness
    with random power-of-2 scales."""
    from hpc_patterns_amd import ops

    monkeypatch.setenv("HPK_MX4_WAVES", "32h")
    m, n, k = 512, 384, 256
    fa, fb, pa, pb = _mx4_operands(m, n, k, 191)
    g = torch.Generator(device="cpu").manual_seed(193)
    sa = torch.randint(124, 131, (m, k // 32), generator=g,
                       dtype=torch.int16).to(torch.uint8)
    sb = torch.randint(124, 131, (n, k // 32), generator=g,
                       dtype=torch.int16).to(torch.uint8)
    da = fa * torch.pow(2.0, sa.float() - 127).repeat_interleave(32, dim=1)
    db = fb * torch.pow(2.0, sb.float() - 127).repeat_interleave(32, dim=1)
    ref = torch.matmul(da, db.t()).cuda()
    c = torch.empty(m, n, dtype=torch.float32, device="cuda")
    ops.gemm_mxfp4(c, pa, pb, sa.cuda(), sb.cuda())
    torch.cuda.synchronize()
    assert torch.equal(c, ref)

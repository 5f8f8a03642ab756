"""The MX quantize kernel (native/quant.hip) against its pure-torch oracle
ops.quantize_mx_reference, bit for bit on both output tensors, and
ops.matmul_mx end to end. The oracle itself is pinned to the written
contract on the CPU by tests/test_mx_quant_reference.py.

Shapes are the smallest at which the kernel can go wrong. A quad of lanes
owns a tile of 4 consecutive MX blocks, lane 0 stores the tile's 4 scale
bytes as one dword, and a ragged last tile stores bytes instead:
  (1, 32)       1 block: one ragged tile, three lanes of the quad idle
  (3, 96)       9 blocks: odd rows, odd blocks per row, tail of 1
  (5, 32*33)    165 blocks: no multiple of any lane-group size
  (2043, 8224)  525,051 blocks > _hpk.QUANT_MAX_GRID (2048 workgroups) *
                256 blocks per workgroup pass = 524,288: the grid stride
                runs a second pass, the tail is 3 blocks, and at 64 MiB of
                fp32 (32.05 MiB of bf16) the input is past the 32 MiB
                threshold from which the nontemporal kernels run; all the
                smaller shapes run the plain ones.
"""

import functools

import pytest
import torch

import mx_quant_cases as cases

pytestmark = pytest.mark.gpu

FMTS = ("mxfp8", "mxfp4")
DTYPES = (torch.float32, torch.bfloat16)
SHAPES = [(1, 32), (3, 96), (5, 32 * 33), (2043, 8224)]
_BLOCKS_PER_WORKGROUP_PASS = 256    # 64 quads of 4 blocks


def _ops():
    from hpc_patterns_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def _randn(shape):
    return cases.wide_randn(*shape)     # built once per shape, never written


def _check(x, fmt):
    """Kernel == oracle on the scale bytes everywhere, and on the element
    codes of every block whose scale is not 255 (Inf/NaN blocks: codes are
    unspecified). Returns (q, scale) of the kernel."""
    ops = _ops()
    q, s = ops.quantize_mx(x, fmt)
    torch.cuda.synchronize()
    q_ref, s_ref = ops.quantize_mx_reference(x, fmt)
    assert s.dtype == torch.uint8 and s.shape == s_ref.shape
    assert q.dtype == q_ref.dtype and q.shape == q_ref.shape
    bad = (s != s_ref).nonzero()
    assert bad.numel() == 0, (
        f"{len(bad)} scale bytes differ; first at {bad[0].tolist()}: kernel "
        f"{int(s[tuple(bad[0])])} oracle {int(s_ref[tuple(bad[0])])}")
    c, c_ref = cases.codes(q, fmt), cases.codes(q_ref, fmt)
    finite = (s_ref != 255).repeat_interleave(32, dim=1)
    bad = ((c != c_ref) & finite).nonzero()
    if bad.numel():
        i = tuple(bad[0])
        raise AssertionError(
            f"{len(bad)} element codes differ; first at {bad[0].tolist()}: "
            f"x {float(x[i])!r} scale {int(s_ref[i[0], i[1] // 32])} kernel "
            f"{int(c[i]):#x} oracle {int(c_ref[i]):#x}")
    return q, s


def test_shape_list_crosses_the_grid_cap():
    from hpc_patterns_amd import _hpk
    assert _hpk.QUANT_MAX_GRID == 2048
    one_pass = _hpk.QUANT_MAX_GRID * _BLOCKS_PER_WORKGROUP_PASS
    rows, k = SHAPES[-1]
    assert rows * k // 32 > one_pass and (rows * k // 32) % 4 != 0
    assert all(r * k // 32 <= one_pass for r, k in SHAPES[:-1])


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_reference_randn(shape, fmt, dtype):
    x = _randn(shape).cuda().to(dtype)
    _check(x, fmt)


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("fmt", FMTS)
def test_kernel_equals_reference_edge_blocks(fmt, dtype):
    """Zero, -0, subnormal, saturating, FLT_MAX, scale-0 and non-finite
    blocks, once one block per row and once all in one row (so that they
    share quads and tiles with each other)."""
    names, blocks = cases.edge_blocks()
    for x in (blocks, blocks.view(1, -1)):
        x = x.cuda().to(dtype)
        _, s = _check(x, fmt)
        s = s.view(-1).tolist()
        for name in ("one_inf", "one_neg_inf", "one_nan"):
            assert s[names.index(name)] == 255, name
        assert s[names.index("all_zero")] == 0
        if dtype == torch.float32:      # FLT_MAX rounds to Inf in bf16
            assert s[names.index("flt_max")] == 254 - (8 if fmt == "mxfp8" else 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("fmt", FMTS)
def test_kernel_equals_reference_on_every_rounding_boundary(fmt, dtype):
    """Every finite code of the element format and every midpoint between
    adjacent codes, at scale 1.0 (exact in fp32 and in bf16)."""
    x = cases.sweep(fmt).cuda().to(dtype)
    assert torch.equal(x.float().cpu(), cases.sweep(fmt))
    _, s = _check(x, fmt)
    assert bool((s == 127).all())


@pytest.mark.parametrize("fmt,emax", [("mxfp8", 8), ("mxfp4", 2)])
def test_block_max_does_not_leak_across_blocks(fmt, emax):
    """Blocks of 1e-3 (exponent field 117) alternate with blocks of 1e3
    (field 136) along a row of 9 blocks, 3 rows."""
    x = torch.full((3, 9, 32), 1e-3)
    x[:, 1::2] = 1e3
    _, s = _check(x.view(3, 288).cuda(), fmt)
    want = torch.tensor([117 - emax, 136 - emax] * 4 + [117 - emax],
                        dtype=torch.uint8).expand(3, 9)
    assert torch.equal(s.cpu(), want)


@pytest.mark.parametrize("fmt", FMTS)
def test_matmul_mx_exact_on_lossless_payload(fmt):
    """Payloads MX holds exactly (scales 124..130, K = 128 < 256: every
    partial sum is exact in fp32 in any order, the condition
    tests/test_gpu_gemm_matrix.py derives), so the product is bitwise the
    float64 one."""
    from hpc_patterns_amd import _hpk
    ops = _ops()
    a = cases.lossless(fmt, 128, 128, seed=2).cuda()
    b = cases.lossless(fmt, 128, 128, seed=3).cuda()
    c = ops.matmul_mx(a, b, fmt)
    torch.cuda.synchronize()
    assert c.dtype == torch.float32 and c.shape == (128, 128)
    assert torch.equal(c, (a.double() @ b.double().T).float())
    assert _hpk.gemm_variant(fmt, *ops.gemm_pad_shapes(fmt, 128, 128, 128)) \
        .startswith(fmt)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_matmul_mx_ragged_pads_k_and_tiles(fmt, dtype):
    """(100, 72, 80): K is zero-padded to 96, then M, N, K to the tile.
    Integers -4..4 at unit scale (halves for mxfp4) are exact in MX."""
    from hpc_patterns_amd import _hpk
    ops = _ops()
    m, n, k = 100, 72, 80
    g = torch.Generator().manual_seed(4)
    unit = 1.0 if fmt == "mxfp8" else 0.5
    a = (torch.randint(-4, 5, (m, k), generator=g) * unit).cuda().to(dtype)
    b = (torch.randint(-4, 5, (n, k), generator=g) * unit).cuda().to(dtype)
    c = ops.matmul_mx(a, b, fmt)
    torch.cuda.synchronize()
    assert c.shape == (m, n) and c.is_contiguous()
    assert torch.equal(c, (a.double() @ b.double().T).float())
    assert _hpk.gemm_variant(fmt, *ops.gemm_pad_shapes(fmt, m, n, 96)) \
        .startswith(fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_matmul_mx_randn_within_fp32_accumulation_bound(fmt):
    """The kernel's operands are the oracle's (the tests above), so against
    the float64 product of the dequantized oracle operands only the fp32
    accumulation differs: |c - ref| <= K * 2^-23 * (|a| @ |b|^T), the
    running-sum bound with the unit roundoff taken as a full ulp."""
    ops = _ops()
    m, n, k = 128, 128, 256
    g = torch.Generator().manual_seed(5)
    a = torch.randn(m, k, generator=g).cuda()
    b = torch.randn(n, k, generator=g).cuda()
    c = ops.matmul_mx(a, b, fmt)
    torch.cuda.synchronize()
    ad = ops.dequantize_mx(*ops.quantize_mx_reference(a, fmt), fmt)
    bd = ops.dequantize_mx(*ops.quantize_mx_reference(b, fmt), fmt)
    ref = ad @ bd.T
    bound = k * 2.0 ** -23 * (ad.abs() @ bd.abs().T)
    err = (c.double() - ref).abs()
    worst = float((err / bound).max())
    print(f"{fmt}: max |c - ref| / bound = {worst:.3e}")
    assert bool((err <= bound).all()), f"worst error / bound = {worst}"


def test_quantize_mx_error_paths():
    ops = _ops()
    x = torch.zeros(4, 64, device="cuda")
    with pytest.raises(TypeError):
        ops.quantize_mx(x.cpu(), "mxfp8")
    with pytest.raises(TypeError):
        ops.quantize_mx(x.half(), "mxfp8")
    with pytest.raises(TypeError):
        ops.quantize_mx(x.view(-1), "mxfp8")
    with pytest.raises(TypeError):
        ops.quantize_mx(x.t(), "mxfp8")                # not contiguous
    with pytest.raises(ValueError):
        ops.quantize_mx(torch.zeros(4, 48, device="cuda"), "mxfp8")
    with pytest.raises(ValueError):
        ops.quantize_mx(x, "mxfp6")
    off = torch.zeros(4 * 64 + 1, device="cuda")[1:].view(4, 64)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    with pytest.raises(ValueError):
        ops.quantize_mx(off, "mxfp8")
    # ... and matmul_mx copes with such a view by copying it
    one = torch.ones(4 * 64 + 1, device="cuda")[1:].view(4, 64)
    c = ops.matmul_mx(one, one, "mxfp8")
    torch.cuda.synchronize()
    assert torch.equal(c, torch.full((4, 4), 64.0, device="cuda"))

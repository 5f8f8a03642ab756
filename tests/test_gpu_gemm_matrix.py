"""Every GEMM variant at its edge shapes, bitwise against a float64 reference.

One table (ROWS) names the 18 kernels the five launchers in native/gemm.hip
can dispatch to, with the environment that selects each, its output tile and
its K quantum. Every test first asserts `_hpk.gemm_variant(...)` names the
row's kernel, so a silently-taken fallback fails instead of passing on the
wrong code. Cases per row:

  single_k           (TM, TN, Kq): one workgroup, ONE trip of the K loop —
                     prologue and epilogue of the pipelined kernels coincide
  ragged_grid        (3TM, 5TN, 3Kq): 15 workgroups (XCD remap q=1, r=7, the
                     uneven arm), odd K-trip count; x xcd_swizzle x
                     HPK_GEMM_GROUP in {unset, 2}
  tiny_grid_swizzle  (TM, 3TN, Kq) with the XCD remap at q=0
  k_gather           (TM, TN, Kq): one operand is one-hot per row at
                     k = (5i+3) mod K with weight in {1,-1,2,0.5}, so every
                     output is ONE product and the other operand can carry
                     the whole number format (all finite e4m3 codes, all 16
                     e2m1 nibbles, full int8, bf16 across the exponent
                     range, e8m0 scales 87..167) and still be exact

All payloads are built on the CPU, the reference is a float64 (int64 for i8)
matmul of the dequantised operands, and test_matrix_payloads_are_exact (no
GPU needed) checks the conditions under which "bitwise equal" is the right
expectation rather than assuming them.
"""

import functools
import os
from collections import namedtuple

import pytest
import torch

Row = namedtuple("Row", "name kind env tm tn kq")

_V, _W = "HPK_GEMM_VARIANT", "HPK_GEMM_WAVES"
ROWS = [
    Row("bf16_plain8", "bf16", {_V: "plain"}, 128, 128, 64),
    Row("bf16_plain4", "bf16", {_V: "plain", _W: "4"}, 128, 128, 64),
    Row("bf16_db8", "bf16", {_V: "db"}, 128, 128, 64),
    Row("bf16_db4", "bf16", {_V: "db", _W: "4"}, 128, 128, 64),
    Row("bf16_8ph", "bf16", {}, 256, 256, 128),
    Row("fp8_plain", "fp8", {_V: "plain"}, 128, 128, 64),
    Row("fp8_8ph", "fp8", {_V: "8ph"}, 256, 256, 128),
    Row("fp8_32", "fp8", {}, 256, 256, 128),
    Row("i8_plain", "i8", {_V: "plain"}, 128, 128, 64),
    Row("i8_8ph", "i8", {}, 256, 256, 256),
    Row("i8_32", "i8", {_V: "32"}, 256, 256, 128),
    Row("mxfp8_plain", "mxfp8", {"HPK_MX8_VARIANT": "plain"}, 128, 128, 128),
    Row("mxfp8_32", "mxfp8", {}, 256, 256, 128),
    Row("mxfp4_w8", "mxfp4", {"HPK_MX4_WAVES": "8"}, 128, 128, 128),
    Row("mxfp4_w4", "mxfp4", {"HPK_MX4_WAVES": "4"}, 128, 128, 128),
    Row("mxfp4_db", "mxfp4", {"HPK_MX4_WAVES": "db"}, 128, 128, 128),
    Row("mxfp4_32", "mxfp4", {}, 256, 256, 128),
    Row("mxfp4_32h", "mxfp4", {"HPK_MX4_WAVES": "32h"}, 256, 128, 128),
]
_ROW_IDS = [r.name for r in ROWS]
_MX = ("mxfp8", "mxfp4")

# Payload of the sum cases: the ranges tests/test_gpu_kernels.py uses per
# dtype — integers -4..4 (bf16, fp8, mxfp8), the e2m1 set up to +-2 in
# halves (mxfp4), full-range int8.
_E2M1_SUM_VALUES = [0., 0.5, -0.5, 1., -1., 1.5, -1.5, 2., -2.]
# MX scales of the sum cases, inclusive. 124..130 (the range the existing
# tests use) wherever the exactness condition of
# test_matrix_payloads_are_exact holds for it: per operand max/granule is
# 4 * 2^6, so K * (2^8)^2 < 2^24 needs K < 256 — true for the single-trip
# shapes (K = 128). ragged_grid has K = 384, where 125..130 (max/granule
# 4 * 2^5, K * 2^14 = 1.5 * 2^22) is the widest range that keeps every
# partial sum exact in any summation order.
_SCALES_SINGLE = (124, 130)
_SCALES_RAGGED = (125, 130)
# k_gather: one product per output, so the scales can roam. 87..167 keeps
# every product a NORMAL fp32: |c| <= 448 * 2 * 2^80, >= 2^-9 * 2^-1 * 2^-80.
_SCALES_GATHER = (87, 167)

# e4m3 codes fed to the fp8/mxfp8 k_gather: every byte except the two NaNs
# (0x7F, 0xFF) — subnormals (0x01-0x07, 0x81-0x87), +-0 and +-448 included.
_E4M3_GATHER_CODES = [c for c in range(256) if c not in (0x7F, 0xFF)]

Payload = namedtuple(
    "Payload", "kind a b sa sb ref ref_wide a_deq b_deq unit_a unit_b")


# ---------------------------------------------------------------------------
# payloads and references (CPU only, built once per (kind, case, shape))
# ---------------------------------------------------------------------------

def _gen(*key):
    # Python's hash() of a str is salted per process; spell the seed out
    s = 0
    for part in key:
        for ch in str(part):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator(device="cpu").manual_seed(s)


def _dequant(kind, x, scale):
    """float64 value of an operand as the kernel is specified to read it."""
    from hpc_patterns_amd import ops

    if kind == "mxfp4":
        v = ops.e2m1_decode(x).to(torch.float64)
    else:
        v = x.to(torch.float64)
    if scale is not None:
        v = v * (2.0 ** (scale.to(torch.float64) - 127)) \
            .repeat_interleave(32, dim=1)
    return v


def _finish(kind, a, b, sa, sb, unit_a, unit_b):
    a_deq, b_deq = _dequant(kind, a, sa), _dequant(kind, b, sb)
    if kind == "i8":
        wide = torch.matmul(a.long(), b.long().t())
        ref = wide.to(torch.int32)
    else:
        wide = torch.matmul(a_deq, b_deq.t())
        ref = wide.to(torch.float32)
    return Payload(kind, a, b, sa, sb, ref, wide, a_deq, b_deq,
                   unit_a, unit_b)


def _sum_operand(kind, rows, k, g):
    """(tensor as the kernel takes it, spacing of its values before scaling)"""
    from hpc_patterns_amd import ops

    if kind == "i8":
        return torch.randint(-128, 128, (rows, k), generator=g,
                             dtype=torch.int8), 1.0
    if kind == "mxfp4":
        vals = torch.tensor(_E2M1_SUM_VALUES)
        f = vals[torch.randint(0, len(vals), (rows, k), generator=g)]
        return ops.e2m1_pack(f), 0.5
    f = torch.randint(-4, 5, (rows, k), generator=g).float()
    dt = torch.bfloat16 if kind == "bf16" else torch.float8_e4m3fn
    return f.to(dt), 1.0


def _scales(rows, k, lo_hi, g):
    lo, hi = lo_hi
    return torch.randint(lo, hi + 1, (rows, k // 32), generator=g,
                         dtype=torch.int16).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def sum_payload(kind, m, n, k, scale_range):
    g = _gen("sum", kind, m, n, k)
    a, ua = _sum_operand(kind, m, k, g)
    b, ub = _sum_operand(kind, n, k, g)
    sa = sb = None
    if kind in _MX:
        sa, sb = _scales(m, k, scale_range, g), _scales(n, k, scale_range, g)
        ua *= 2.0 ** (scale_range[0] - 127)
        ub *= 2.0 ** (scale_range[0] - 127)
    return _finish(kind, a, b, sa, sb, ua, ub)


def _full_range_operand(kind, rows, k, g):
    """An operand that carries the whole number format (k_gather)."""
    n = rows * k
    if kind == "i8":
        codes = (torch.arange(n) % 256 - 128).to(torch.int8)
        return codes[torch.randperm(n, generator=g)].view(rows, k)
    if kind == "bf16":
        # random finite bit patterns, exponent field 2..253: every product
        # with a weight in {+-1, 2, 0.5} then stays a normal, finite fp32
        # (field 254 times 2 overflows, which the float64 reference does
        # not survive; field 1 times 0.5 is an fp32 subnormal). Those ends,
        # bf16 SUBNORMAL inputs (field 0) and NaN/Inf have a reference and
        # a comparison rule of their own: tests/test_gpu_gemm_specials.py.
        sign = torch.randint(0, 2, (n,), generator=g)
        exp = torch.randint(2, 254, (n,), generator=g)
        man = torch.randint(0, 128, (n,), generator=g)
        bits = (sign << 15) | (exp << 7) | man
        bits = torch.where(bits >= 32768, bits - 65536, bits)
        return bits.to(torch.int16).view(torch.bfloat16).view(rows, k)
    if kind == "mxfp4":
        # raw bytes, not e2m1_pack: all 16 nibble codes in both nibble
        # positions, so -0, +-3, +-4 and +-6 reach the kernel
        codes = (torch.arange(n // 2) % 256).to(torch.uint8)
        return codes[torch.randperm(n // 2, generator=g)].view(rows, k // 2)
    table = torch.tensor(_E4M3_GATHER_CODES, dtype=torch.uint8)
    codes = table[torch.arange(n) % len(table)]
    return codes[torch.randperm(n, generator=g)] \
        .view(torch.float8_e4m3fn).view(rows, k)


def _one_hot_operand(kind, rows, k):
    """H[i, (5i+3) mod k] = w(i), zero elsewhere; w cycles {1,-1,2,0.5}
    (+-1, +-2 for i8). i -> (5i+3) mod k is a bijection on k for i < k
    (gcd(5, k) = 1 for every K quantum) and wraps for i >= k."""
    from hpc_patterns_amd import ops

    w = [1., -1., 2., -2.] if kind == "i8" else [1., -1., 2., 0.5]
    h = torch.zeros(rows, k)
    i = torch.arange(rows)
    h[i, (5 * i + 3) % k] = torch.tensor(w)[i % 4]
    if kind == "i8":
        return h.to(torch.int8)
    if kind == "mxfp4":
        return ops.e2m1_pack(h)
    return h.to(torch.bfloat16 if kind == "bf16" else torch.float8_e4m3fn)


@functools.lru_cache(maxsize=None)
def gather_payload(kind, m, n, k, full_side):
    g = _gen("gather", kind, m, n, k, full_side)
    if full_side == "a":
        a, b = _full_range_operand(kind, m, k, g), _one_hot_operand(kind, n, k)
    else:
        a, b = _one_hot_operand(kind, m, k), _full_range_operand(kind, n, k, g)
    sa = sb = None
    if kind in _MX:
        sa = _scales(m, k, _SCALES_GATHER, g)
        sb = _scales(n, k, _SCALES_GATHER, g)
    return _finish(kind, a, b, sa, sb, None, None)


def _case_payloads(row):
    """Every payload the matrix feeds this row: (case id, payload, is_sum)."""
    tm, tn, kq, kind = row.tm, row.tn, row.kq, row.kind
    yield "single_k", sum_payload(kind, tm, tn, kq, _SCALES_SINGLE), True
    yield "ragged_grid", sum_payload(kind, 3 * tm, 5 * tn, 3 * kq,
                                     _SCALES_RAGGED), True
    yield "tiny_grid_swizzle", sum_payload(kind, tm, 3 * tn, kq,
                                           _SCALES_SINGLE), True
    for side in ("a", "b"):
        yield f"k_gather[{side}]", gather_payload(kind, tm, tn, kq, side), \
            False


# ---------------------------------------------------------------------------
# CPU-runnable guard: "bitwise equal" is a checked condition
# ---------------------------------------------------------------------------

def test_matrix_table_is_complete():
    assert len(ROWS) == 18 and len(set(_ROW_IDS)) == 18
    for row in ROWS:
        assert row.kq <= row.tn  # one k_gather pass reaches every k
        assert all(k.startswith(("HPK_GEMM_", "HPK_MX4_", "HPK_MX8_"))
                   for k in row.env)


@pytest.mark.parametrize("row", ROWS, ids=_ROW_IDS)
def test_matrix_payloads_are_exact(row):
    """1. every float64 reference element is an fp32 value (int32 for i8),
    so the cast to the output dtype loses nothing; 2. in the sum cases every
    partial sum, in ANY order, is exact in fp32: all products are multiples
    of min_granule and K * max|a| * max|b| / min_granule < 2^24."""
    for case, p, is_sum in _case_payloads(row):
        k = p.a_deq.shape[1]
        if p.kind == "i8":
            assert p.ref_wide.abs().max() < 2 ** 31, case
            assert torch.equal(p.ref.long(), p.ref_wide), case
            assert k * 128 * 128 < 2 ** 31, case  # any partial sum
            continue
        assert torch.isfinite(p.ref_wide).all(), case
        assert torch.equal(p.ref_wide.float().double(), p.ref_wide), case
        if not is_sum:
            # one product per output; it must be a NORMAL fp32 or zero
            nz = p.ref_wide[p.ref_wide != 0].abs()
            assert nz.min() >= 2.0 ** -126, case
            # ... and really a single product: <= 1 nonzero term per output
            terms = (p.a_deq != 0).double() @ (p.b_deq != 0).double().t()
            assert terms.max() <= 1, case
            continue
        for deq, unit in ((p.a_deq, p.unit_a), (p.b_deq, p.unit_b)):
            q = deq / unit
            assert torch.equal(q, q.round()), case  # multiples of the unit
        min_granule = p.unit_a * p.unit_b
        bound = k * float(p.a_deq.abs().max()) * float(p.b_deq.abs().max())
        assert bound / min_granule < 2 ** 24, (case, bound / min_granule)


def test_gather_payloads_cover_the_formats():
    """The k_gather operands carry what they claim to."""
    fp8 = gather_payload("fp8", 128, 128, 64, "a").a.view(torch.uint8)
    assert sorted(set(fp8.flatten().tolist())) == _E4M3_GATHER_CODES
    mx4 = gather_payload("mxfp4", 128, 128, 128, "a").a
    assert set((mx4 & 0xF).flatten().tolist()) == set(range(16))
    assert set((mx4 >> 4).flatten().tolist()) == set(range(16))
    i8 = gather_payload("i8", 128, 128, 64, "b").b
    assert set(i8.flatten().tolist()) == set(range(-128, 128))
    bf = gather_payload("bf16", 128, 128, 64, "a").a.view(torch.int16).int()
    exps = set(((bf >> 7) & 0xFF).flatten().tolist())
    assert min(exps) == 2 and max(exps) == 253
    for kind in _MX:
        p = gather_payload(kind, 128, 128, 128, "a")
        for s in (p.sa, p.sb):
            assert int(s.min()) >= 87 and int(s.max()) <= 167
            assert len(set(s.flatten().tolist())) > 40


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------

@pytest.fixture
def hpk():
    from hpc_patterns_amd._native import native

    torch.cuda.set_device(0)
    return native()  # fail loudly, not skip: on a GPU box it must exist


@pytest.fixture
def row_env(request, monkeypatch):
    """Start from NO dispatch variable, then set exactly the row's."""
    row = request.node.callspec.params["row"]
    for name in list(os.environ):
        if name.startswith(("HPK_GEMM_", "HPK_MX4_", "HPK_MX8_")):
            monkeypatch.delenv(name)
    for name, value in row.env.items():
        monkeypatch.setenv(name, value)
    return row


def _run_and_compare(hpk, row, p, xcd_swizzle):
    from hpc_patterns_amd import ops

    m, n = p.ref.shape
    k = p.a_deq.shape[1]
    assert hpk.gemm_variant(row.kind, m, n, k) == row.name
    a, b = p.a.cuda(), p.b.cuda()
    # poison C: a tile nobody writes must not pass by luck
    if row.kind == "i8":
        c = torch.full((m, n), -(2 ** 31), dtype=torch.int32, device="cuda")
    else:
        c = torch.full((m, n), float("nan"), device="cuda")
    if row.kind == "bf16":
        ops.gemm_bf16(c, a, b, xcd_swizzle=xcd_swizzle)
    elif row.kind == "fp8":
        ops.gemm_fp8(c, a, b, xcd_swizzle=xcd_swizzle)
    elif row.kind == "i8":
        ops.gemm_i8(c, a, b, xcd_swizzle=xcd_swizzle)
    elif row.kind == "mxfp8":
        ops.gemm_mxfp8(c, a, b, p.sa.cuda(), p.sb.cuda(),
                       xcd_swizzle=xcd_swizzle)
    else:
        ops.gemm_mxfp4(c, a, b, p.sa.cuda(), p.sb.cuda(),
                       xcd_swizzle=xcd_swizzle)
    torch.cuda.synchronize()
    got = c.cpu()
    if torch.equal(got, p.ref):
        return
    idx = (got != p.ref).nonzero()  # NaN poison compares unequal too
    head = []
    for i, j in idx[:8]:
        # the largest-magnitude term of the output names the culprit operands
        kk = int((p.a_deq[i] * p.b_deq[j]).abs().argmax())
        head.append((int(i), int(j), got[i, j].item(), p.ref[i, j].item(),
                     f"a[{kk}]={p.a_deq[i, kk].item()!r}",
                     f"b[{kk}]={p.b_deq[j, kk].item()!r}"))
    pytest.fail(f"{row.name} {m}x{n}x{k}: {len(idx)} of {m * n} outputs "
                f"differ; first (row, col, got, ref, top term): {head}")


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=_ROW_IDS)
def test_single_k(hpk, row_env, row):
    p = sum_payload(row.kind, row.tm, row.tn, row.kq, _SCALES_SINGLE)
    _run_and_compare(hpk, row, p, xcd_swizzle=False)


@pytest.mark.gpu
@pytest.mark.parametrize("group", [None, "2"], ids=["rowmajor", "group2"])
@pytest.mark.parametrize("xcd_swizzle", [False, True],
                         ids=["linear", "swizzle"])
@pytest.mark.parametrize("row", ROWS, ids=_ROW_IDS)
def test_ragged_grid(hpk, row_env, monkeypatch, row, xcd_swizzle, group):
    if group is not None:
        monkeypatch.setenv("HPK_GEMM_GROUP", group)
    p = sum_payload(row.kind, 3 * row.tm, 5 * row.tn, 3 * row.kq,
                    _SCALES_RAGGED)
    _run_and_compare(hpk, row, p, xcd_swizzle=xcd_swizzle)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=_ROW_IDS)
def test_tiny_grid_swizzle(hpk, row_env, row):
    p = sum_payload(row.kind, row.tm, 3 * row.tn, row.kq, _SCALES_SINGLE)
    _run_and_compare(hpk, row, p, xcd_swizzle=True)


@pytest.mark.gpu
@pytest.mark.parametrize("full_side", ["a", "b"])
@pytest.mark.parametrize("row", ROWS, ids=_ROW_IDS)
def test_k_gather(hpk, row_env, row, full_side):
    p = gather_payload(row.kind, row.tm, row.tn, row.kq, full_side)
    _run_and_compare(hpk, row, p, xcd_swizzle=False)

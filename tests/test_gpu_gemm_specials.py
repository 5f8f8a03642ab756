"""The GEMM family on NaN, Inf, bf16 subnormals, products that leave fp32
at either end, e8m0 scales 0..2 / 252..254 and the e8m0 NaN 255: every NT
variant by name, the nn/tn/tt layout kernels, split-K and the front doors
(matmul_mx, matmul_nt, linear_bf16).

Payloads, reference and the comparison rule live in
tests/gemm_special_cases.py and are guarded on the CPU by
tests/test_gemm_special_cases.py. In short: got and reference must be NaN
at the same places and equal everywhere else (+-Inf included); an output in
the two-outcome class (exact value an fp32 subnormal, or its only non-zero
term has a bf16-subnormal input) may instead be a zero of the exact value's
sign. Rows and columns without a planted special must equal the clean
payload's reference: a NaN that smears is a kernel bug.

The discipline is the matrix's (tests/test_gpu_gemm_matrix.py): clear every
HPK_GEMM_*, HPK_MX4_* and HPK_MX8_* variable, set the row's, assert
_hpk.gemm_variant names the row. C is prefilled with a FINITE sentinel,
NaN being a legitimate answer here. Each test is one single-tile launch.

int8 has no special values; its extremes (-128, 127) are in the matrix, so
there is nothing to add for it here.
"""

import functools

import pytest
import torch

import gemm_special_cases as sc
import mx_quant_cases as cases
from test_gpu_gemm_matrix import hpk, row_env  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

_ids = lambda rows: [r.name for r in rows]  # noqa: E731
_NAN, _INF = float("nan"), float("inf")


def _ops():
    from hpc_patterns_amd import ops
    return ops


def _sentinel(shape):
    return torch.full(shape, sc.SENTINEL, device="cuda")


def _launch(kind, c, p):
    ops = _ops()
    a, b = p.a.cuda(), p.b.cuda()
    if kind == "bf16":
        ops.gemm_bf16(c, a, b)
    elif kind == "fp8":
        ops.gemm_fp8(c, a, b)
    elif kind == "mxfp8":
        ops.gemm_mxfp8(c, a, b, p.sa.cuda(), p.sb.cuda())
    else:
        ops.gemm_mxfp4(c, a, b, p.sa.cuda(), p.sb.cuda())
    torch.cuda.synchronize()


def _judge(got, p, what):
    """Print the two-outcome tally, then fail on anything not accepted."""
    got = got.cpu()
    if bool(p.two.any()):
        exact, flushed = sc.outcome_counts(got, p)
        print(f"{what} {p.name}: two-outcome class of {int(p.two.sum())}: "
              f"{exact} exact, {flushed} flushed to zero")
    count, head = sc.describe_mismatches(got, p)
    if count:
        pytest.fail(f"{what} {p.name}: {count} of {got.numel()} outputs are "
                    f"wrong; first (row, col, got, ref, top term): {head}")
    return got


def _run_row(hpk, row, p):
    m, n = p.ref.shape
    assert hpk.gemm_variant(row.kind, m, n, p.a_deq.shape[1]) == row.name
    c = _sentinel((m, n))
    _launch(row.kind, c, p)
    return _judge(c, p, row.name)


# ---------------------------------------------------------------------------
# every NT variant, by name
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("side", sc.SIDES)
@pytest.mark.parametrize("row", sc.NONFINITE_ROWS,
                         ids=_ids(sc.NONFINITE_ROWS))
def test_nonfinite(hpk, row_env, row, side):
    _run_row(hpk, row, sc.nonfinite(row.kind, side, row.tm, row.tn, row.kq))


@pytest.mark.parametrize("side", sc.SIDES)
@pytest.mark.parametrize("row", sc.BF16_ROWS, ids=_ids(sc.BF16_ROWS))
def test_overflow_and_underflow(hpk, row_env, row, side):
    _run_row(hpk, row, sc.overflow_and_underflow(row.kind, side, row.tm,
                                                 row.tn, row.kq))


@pytest.mark.parametrize("side", sc.SIDES)
@pytest.mark.parametrize("row", sc.BF16_ROWS, ids=_ids(sc.BF16_ROWS))
def test_subnormal_inputs(hpk, row_env, row, side):
    _run_row(hpk, row, sc.subnormal_inputs(row.kind, side, row.tm, row.tn,
                                           row.kq))


@pytest.mark.parametrize("side", sc.SIDES)
@pytest.mark.parametrize("row", sc.MX_ROWS, ids=_ids(sc.MX_ROWS))
def test_extreme_scales(hpk, row_env, row, side):
    _run_row(hpk, row, sc.extreme_scales(row.kind, side, row.tm, row.tn,
                                         row.kq))


@pytest.mark.parametrize("side", sc.SIDES)
@pytest.mark.parametrize("row", sc.MX_ROWS, ids=_ids(sc.MX_ROWS))
def test_nan_scale(hpk, row_env, row, side):
    _run_row(hpk, row, sc.nan_scale(row.kind, side, row.tm, row.tn, row.kq))


# ---------------------------------------------------------------------------
# layout kernels: bit-identical to bf16_db8, on specials too
# ---------------------------------------------------------------------------

@pytest.fixture
def no_dispatch_env(monkeypatch):
    import os
    for name in list(os.environ):
        if name.startswith(("HPK_GEMM_", "HPK_MX4_", "HPK_MX8_")):
            monkeypatch.delenv(name)


def _bits_equal(x, y):
    return torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("side", sc.SIDES)
@pytest.mark.parametrize("builder", [sc.nonfinite, sc.subnormal_inputs],
                         ids=["nonfinite", "subnormal_inputs"])
@pytest.mark.parametrize("layout", ["nn", "tn", "tt"])
def test_layout_kernels(hpk, no_dispatch_env, monkeypatch, layout, builder,
                        side):
    ops = _ops()
    m, n, k = sc.LAYOUT_SHAPE
    p = builder("bf16", side, m, n, k)
    a = (p.a.t().contiguous() if layout[0] == "t" else p.a).cuda()
    b = (p.b if layout[1] == "t" else p.b.t().contiguous()).cuda()
    c = _sentinel((m, n))
    ops.gemm_bf16_layout(c, a, b, layout)
    torch.cuda.synchronize()
    got = _judge(c, p, layout)

    monkeypatch.setenv("HPK_GEMM_VARIANT", "db")
    assert hpk.gemm_variant("bf16", m, n, k) == "bf16_db8"
    c_nt = _sentinel((m, n))
    _launch("bf16", c_nt, p)
    c_nt = c_nt.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(c_nt))
    assert _bits_equal(torch.nan_to_num(got, nan=0.0),
                       torch.nan_to_num(c_nt, nan=0.0)), \
        f"{layout} differs from bf16_db8 on {p.name}"


# ---------------------------------------------------------------------------
# split-K: the fold carries the specials of one split into C
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("side", sc.SIDES)
@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_splitk_fold_carries_specials(hpk, no_dispatch_env, kind, side):
    ops = _ops()
    p = sc.splitk_payload(kind, side)
    m, n = p.ref.shape
    a, b = p.a.cuda(), p.b.cuda()
    got = {}
    for splits in (1, 4):
        c = _sentinel((m, n))
        ops.gemm_splitk(c, a, b, splits)
        torch.cuda.synchronize()
        got[splits] = _judge(c, p, f"splitk[{splits}]")
    assert torch.equal(torch.isnan(got[1]), torch.isnan(got[4]))
    assert torch.equal(torch.isinf(got[1]), torch.isinf(got[4]))
    clean = torch.ones(m, n, dtype=torch.bool)
    clean[list(p.rows), :] = False
    clean[:, list(p.cols)] = False
    assert torch.equal(got[4][clean], p.clean_ref[clean])
    assert not bool(torch.isfinite(got[4][~clean]).any())


@pytest.mark.parametrize("side", sc.SIDES)
def test_splitk_subnormal_inputs(hpk, no_dispatch_env, side):
    """One product per output: the other split's partial is a zero, and the
    fold must neither flush nor lose the product."""
    ops = _ops()
    p = sc.subnormal_inputs("bf16", side, 128, 128, 128)
    c = _sentinel((128, 128))
    ops.gemm_splitk(c, p.a.cuda(), p.b.cuda(), 2)
    torch.cuda.synchronize()
    _judge(c, p, "splitk[2]")


# ---------------------------------------------------------------------------
# front doors (never xfail)
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _mx_front_payload(fmt, m, n, k):
    """(a, b, clean fp32 reference): exact in the format. K % 32 == 0 takes
    cases.lossless (scales 124..130, K = 128: exact in any order, the
    condition tests/test_gpu_gemm_matrix.py derives); the ragged shape the
    integers -4..4 at unit scale (halves for mxfp4)."""
    if k % 32 == 0:
        a = cases.lossless(fmt, m, k, seed=2)
        b = cases.lossless(fmt, n, k, seed=3)
    else:
        g = torch.Generator().manual_seed(4)
        unit = 1.0 if fmt == "mxfp8" else 0.5
        a = torch.randint(-4, 5, (m, k), generator=g) * unit
        b = torch.randint(-4, 5, (n, k), generator=g) * unit
    wide = sc.reference(a.double(), b.double())
    ref = wide.float()
    assert torch.equal(ref.double(), wide)
    assert torch.equal(a.to(torch.bfloat16).float(), a)
    assert torch.equal(b.to(torch.bfloat16).float(), b)
    return a, b, ref


def _check_lines(got, ref, rows, cols, what):
    """rows / cols entirely NaN, every other output equal to ref."""
    got = got.cpu()
    want = ref.clone()
    want[list(rows), :] = _NAN
    want[:, list(cols)] = _NAN
    bad = (torch.isnan(got) != torch.isnan(want)) \
        | (~torch.isnan(want) & (got != want))
    if bool(bad.any()):
        idx = bad.nonzero()
        head = [(int(i), int(j), got[i, j].item(), want[i, j].item())
                for i, j in idx[:8]]
        pytest.fail(f"{what}: {len(idx)} of {got.numel()} outputs are wrong; "
                    f"first (row, col, got, want): {head}")


@pytest.mark.parametrize("shape", [(128, 128, 128), (100, 72, 80)],
                         ids=["tile", "ragged"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
def test_matmul_mx_nonfinite_inputs(hpk, no_dispatch_env, fmt, dtype, shape):
    """+Inf at a[3, 79] (for K = 80 the block that the K padding completes),
    NaN at a[50, 0], -Inf at b[7, 40]: rows 3 and 50 and column 7 of the
    result are entirely NaN, the rest is the clean product."""
    ops = _ops()
    a, b, ref = _mx_front_payload(fmt, *shape)
    a, b = a.clone(), b.clone()
    a[3, 79] = _INF
    a[50, 0] = _NAN
    b[7, 40] = -_INF
    c = ops.matmul_mx(a.cuda().to(dtype), b.cuda().to(dtype), fmt)
    torch.cuda.synchronize()
    assert c.shape == ref.shape and c.dtype == torch.float32
    _check_lines(c, ref, (3, 50), (7,), f"matmul_mx {fmt} {shape}")


@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
@pytest.mark.parametrize("side", sc.SIDES)
def test_matmul_nt_scale_255(hpk, no_dispatch_env, fmt, side):
    """Scaled matmul_nt on operands whose scale rows hold the e8m0 NaN."""
    ops = _ops()
    p = sc.nan_scale(fmt, side, 128, 128, 128)
    c = ops.matmul_nt(p.a.cuda(), p.b.cuda(), p.sa.cuda(), p.sb.cuda())
    torch.cuda.synchronize()
    _check_lines(c, p.clean_ref, p.rows, p.cols, f"matmul_nt {p.name}")


def test_matmul_nt_bf16_nan_row(hpk, no_dispatch_env):
    ops = _ops()
    m, n, k = 100, 130, 70
    g = torch.Generator().manual_seed(6)
    a = torch.randint(-4, 5, (m, k), generator=g).float()
    b = torch.randint(-4, 5, (n, k), generator=g).float()
    ref = sc.reference(a.double(), b.double()).float()
    a[41, 13] = _NAN
    c = ops.matmul_nt(a.to(torch.bfloat16).cuda(), b.to(torch.bfloat16).cuda())
    torch.cuda.synchronize()
    assert c.shape == (m, n)
    _check_lines(c, ref, (41,), (), "matmul_nt bf16 ragged")


def test_linear_bf16_inf_gradient(hpk, no_dispatch_env):
    """One Inf in dy: row m0 of dx and row n0 of dw are non-finite, the rest
    is the float64 autograd result of the clean dy, cast to bf16."""
    ops = _ops()
    m, n, k = 100, 130, 70
    m0, n0 = 17, 101
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-1, 2, (m, k), generator=g).float()
    w = torch.randint(-1, 2, (n, k), generator=g).float()
    dy = torch.randint(-1, 2, (m, n), generator=g).float()
    dy[m0, n0] = 0.0        # the clean gradient; Inf goes here below

    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    (x64 @ w64.t()).backward(dy.double())
    for t in (x64.grad, w64.grad):  # integers <= 256: exact in bf16
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 256

    dy[m0, n0] = _INF
    xd = x.to(torch.bfloat16).cuda().requires_grad_()
    wd = w.to(torch.bfloat16).cuda().requires_grad_()
    y = ops.linear_bf16(xd, wd)
    y.backward(dy.to(torch.bfloat16).cuda())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    for got, ref, line, what in ((xd.grad, x64.grad, m0, "dx"),
                                 (wd.grad, w64.grad, n0, "dw")):
        got = got.float().cpu()
        assert not bool(torch.isfinite(got[line]).any()), what
        keep = torch.ones(got.shape[0], dtype=torch.bool)
        keep[line] = False
        bad = (got[keep] != ref.float()[keep]).nonzero()
        assert bad.numel() == 0, (what, len(bad), bad[:8].tolist())

"""The bf16-output GEMM epilogue with bias (native/gemm_epilogue.hip) on the
GPU: bitwise against float64 on exact payloads and against the oracle
everywhere — the fp32 C of the kernel that existed (gemm_bf16 under
HPK_GEMM_VARIANT=db, gemm_bf16_layout, gemm_splitk,
gemm_bf16_layout_splitk), taken to the CPU, one fp32 add of the bias, one
cast (gemm_epilogue_cases.oracle). C and a caller's workspace are NaN
before every call; the bias is distinct per column and asymmetric."""

import pytest
import torch

import gemm_epilogue_cases as cases

pytestmark = pytest.mark.gpu

LAYOUTS = cases.LAYOUTS
BF16 = torch.bfloat16


@pytest.fixture
def ops():
    from hpc_patterns_amd import ops as _ops
    from hpc_patterns_amd._native import native

    torch.cuda.set_device(0)
    native()  # fail loudly, not skip: on a GPU box it must exist
    return _ops


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("HPK_GEMM_GROUP", raising=False)
    monkeypatch.delenv("HPK_GEMM_VARIANT", raising=False)


def _poison(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device="cuda", dtype=dtype)


def _same(got, ref, what):
    """equal where neither is NaN, and NaN in the same places"""
    got, ref = got.cpu(), ref.cpu()
    gn, rn = torch.isnan(got), torch.isnan(ref)
    bad = (gn != rn) | (~gn & ~rn & (got != ref))
    if not bool(bad.any()):
        return
    idx = bad.nonzero()
    head = [(int(i), int(j), got[i, j].item(), ref[i, j].item())
            for i, j in idx[:8]]
    pytest.fail(f"{what}: {len(idx)} of {got.numel()} outputs differ; "
                f"first (row, col, got, ref): {head}")


def _exact(got, ref, what):
    assert not bool(torch.isnan(ref).any())
    _same(got, ref, what)


def _fused(ops, p, layout, bias=True, splits=1, workspace=None, **kw):
    a, b = (t.cuda() for t in cases.stored(p, layout))
    m, n = p.a.shape[0], p.b.shape[1]
    c = _poison((m, n), BF16)
    ops.gemm_bf16_epilogue(c, a, b, layout,
                           bias=p.bias.cuda() if bias else None,
                           splits=splits, workspace=workspace, **kw)
    torch.cuda.synchronize()
    return c


def _parent32(ops, p, layout):
    """fp32 C of the kernel that existed, on the CPU"""
    a, b = (t.cuda() for t in cases.stored(p, layout))
    m, n = p.a.shape[0], p.b.shape[1]
    c = _poison((m, n))
    if layout == "nt":
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("HPK_GEMM_VARIANT", "db")
            from hpc_patterns_amd._native import native
            assert native().gemm_variant("bf16", m, n, p.a.shape[1]) \
                == "bf16_db8"
            ops.gemm_bf16(c, a, b)
    else:
        ops.gemm_bf16_layout(c, a, b, layout)
    torch.cuda.synchronize()
    return c.cpu()


# ---------------------------------------------------------------------------
# exact payloads: float64 and the oracle, all four layouts
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", cases.EXACT,
                         ids=["x".join(map(str, s)) for s in cases.EXACT])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_exact(ops, layout, shape):
    p = cases.exact_payload(*shape)
    got = _fused(ops, p, layout)
    _exact(got.double(), p.wide, f"{layout} {shape} vs float64")
    _exact(got, cases.oracle(_parent32(ops, p, layout), p.bias),
           f"{layout} {shape} vs oracle")
    nob = _fused(ops, p, layout, bias=False)
    _exact(nob, cases.oracle(_parent32(ops, p, layout)),
           f"{layout} {shape} no bias")


@pytest.mark.parametrize("group", [None, "2"])
@pytest.mark.parametrize("swizzle", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ragged_grid(ops, monkeypatch, layout, swizzle, group):
    if group is not None:
        monkeypatch.setenv("HPK_GEMM_GROUP", group)
    p = cases.exact_payload(*cases.RAGGED_GRID)
    got = _fused(ops, p, layout, xcd_swizzle=swizzle)
    _exact(got.double(), p.wide, f"{layout} swizzle={swizzle} group={group}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_identity_shows_a_transposed_store(ops, layout):
    p = cases.identity_payload()
    assert not torch.equal(p.b.float()[:128, :128], p.b.float()[:128, :128].t())
    got = _fused(ops, p, layout)
    _exact(got.double(), p.wide, f"{layout} identity")
    _exact(got, cases.oracle(_parent32(ops, p, layout), p.bias),
           f"{layout} identity vs oracle")


# ---------------------------------------------------------------------------
# rounding and specials (nt and tn)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["nt", "tn"])
def test_rounding(ops, layout):
    p, want = cases.rounding_payload()
    got = _fused(ops, p, layout)
    _exact(got.double(), want, f"{layout} rounding vs float64 RNE")
    _exact(got, cases.oracle(_parent32(ops, p, layout), p.bias),
           f"{layout} rounding vs oracle")
    assert bool(torch.isinf(got[:, -cases.OVERFLOW_COLS:]).all())


@pytest.mark.parametrize("layout", ["nt", "tn"])
def test_inf_bias_column_and_nan_row(ops, layout):
    base = cases.exact_payload(*cases.EXACT[1])
    a = base.a.clone()
    a[37, 5] = float("nan")
    bias = base.bias.clone()
    bias[70] = float("inf")
    p = cases.Payload(a, base.b, bias, None)
    got = _fused(ops, p, layout).cpu()
    ref = cases.oracle(_parent32(ops, p, layout), bias)
    _same(got, ref, f"{layout} specials")
    nan = torch.isnan(got)
    assert bool(nan[37].all()) and int(nan.sum()) == got.shape[1]
    inf = torch.isinf(got)
    want_inf = torch.zeros_like(inf)
    want_inf[:, 70] = True
    want_inf[37, 70] = False
    assert torch.equal(inf, want_inf) and bool((got[inf] > 0).all())
    # and everything else is the clean payload's
    clean = (base.wide).to(BF16)
    keep = ~nan & ~inf
    assert torch.equal(got[keep], clean[keep])


# ---------------------------------------------------------------------------
# randn: the accumulators are the parents'
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_randn_equals_parent(ops, layout):
    p = cases.randn_payload(*cases.RANDN)
    c32 = _parent32(ops, p, layout)
    with_bias = cases.oracle(c32, p.bias)
    first = _fused(ops, p, layout)
    _exact(first, with_bias, f"{layout} randn + bias")
    _exact(_fused(ops, p, layout, bias=False), cases.oracle(c32),
           f"{layout} randn")
    assert not torch.equal(with_bias, cases.oracle(c32))
    for i in range(cases.REPEATS):
        assert torch.equal(_fused(ops, p, layout), first), f"repeat {i}"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    a, b = (t.cuda() for t in cases.stored(p, layout))
    bias = p.bias.cuda()
    c = _poison(c32.shape, BF16)
    torch.cuda.synchronize()
    ops.gemm_bf16_epilogue(c, a, b, layout, bias=bias, stream=side)
    side.synchronize()
    _exact(c, with_bias, f"{layout} randn side stream")


# ---------------------------------------------------------------------------
# split-K
# ---------------------------------------------------------------------------

def _parent_split32(ops, p, layout, splits):
    a, b = (t.cuda() for t in cases.stored(p, layout))
    c = _poison((p.a.shape[0], p.b.shape[1]))
    ops.gemm_bf16_layout_splitk(c, a, b, layout, splits)  # nt: gemm_splitk
    torch.cuda.synchronize()
    return c.cpu()


@pytest.mark.parametrize("splits", cases.SPLITK_SPLITS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_splitk(ops, layout, splits):
    p = cases.exact_payload(*cases.SPLITK)
    m, n = p.wide.shape
    ws = _poison((splits * m * n,))
    got = _fused(ops, p, layout, splits=splits, workspace=ws)
    _exact(got.double(), p.wide, f"{layout} S={splits} vs float64")
    _exact(got, cases.oracle(_parent_split32(ops, p, layout, splits), p.bias),
           f"{layout} S={splits} vs oracle")
    if splits == 1:  # written by the GEMM kernel: the workspace is untouched
        assert bool(torch.isnan(ws).all())
    else:
        assert not bool(torch.isnan(ws).any())
    r = cases.randn_payload(m, n, cases.SPLITK[2])
    _exact(_fused(ops, r, layout, splits=splits),
           cases.oracle(_parent_split32(ops, r, layout, splits), r.bias),
           f"{layout} S={splits} randn vs oracle")


@pytest.mark.parametrize("splits", cases.RAGGED_SPLITS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_splitk_ragged_grid(ops, layout, splits):
    p = cases.exact_payload(*cases.RAGGED_GRID)
    got = _fused(ops, p, layout, splits=splits)
    _exact(got.double(), p.wide, f"{layout} ragged S={splits}")
    _exact(_fused(ops, p, layout, splits=splits, bias=False),
           cases.oracle(_parent_split32(ops, p, layout, splits)),
           f"{layout} ragged S={splits} no bias")


def test_splitk_workspace(ops):
    p = cases.exact_payload(*cases.SPLITK)
    m, n = p.wide.shape
    ws = _poison((5 * m * n + 64,))
    got = _fused(ops, p, "tn", splits=3, workspace=ws)     # oversized
    _exact(got.double(), p.wide, "oversized workspace")
    assert bool(torch.isnan(ws[3 * m * n:]).all())
    got = _fused(ops, p, "tn", splits=5, workspace=ws)     # reused
    _exact(got.double(), p.wide, "reused workspace")
    assert bool(torch.isnan(ws[5 * m * n:]).all())
    got = _fused(ops, p, "tn", splits=5)                   # absent
    _exact(got.double(), p.wide, "allocated workspace")


@pytest.mark.parametrize("layout", ["nt", "tn"])
def test_fold_grid_stride(ops, layout):
    m, n, k, splits = cases.GRID_STRIDE
    p = cases.exact_payload(m, n, k)
    got = _fused(ops, p, layout, splits=splits)
    _exact(got.double(), p.wide, f"{layout} grid-stride fold")


# ---------------------------------------------------------------------------
# colsum_bf16
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", cases.COLSUM_N)
@pytest.mark.parametrize("m", cases.COLSUM_M)
def test_colsum_exact(ops, m, n):
    x = cases.colsum_payload(m, n)
    want = x.double().sum(0)
    assert float(x.double().abs().sum(0).max()) < 2 ** 24
    got = ops.colsum_bf16(x.cuda())
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == (n,)
    assert torch.equal(got.cpu().double(), want)
    out = _poison((n,))
    assert ops.colsum_bf16(x.cuda(), out=out) is out
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().double(), want)


def test_colsum_chunks(ops):
    """the launcher's R == 1 and R > 1 both run above"""
    plans = {(m, n): ops.colsum_plan(m, -(-n // 8) * 8)
             for m in cases.COLSUM_M for n in cases.COLSUM_N}
    assert plans[(7, 136)] == 1 and plans[(4099, 1000)] > 1


def test_colsum_randn(ops):
    m, n = cases.COLSUM_RANDN
    g = cases._gen("colsum-randn")
    x = torch.randn(m, n, generator=g).to(BF16)
    xd = x.cuda()
    first = ops.colsum_bf16(xd)
    torch.cuda.synchronize()
    err = (first.cpu().double() - x.double().sum(0)).abs()
    bound = (m - 1) * 2.0 ** -24 * x.double().abs().sum(0)
    print(f"colsum randn: max err {float(err.max()):.3e}, "
          f"min bound {float(bound.min()):.3e}")
    assert bool((err <= bound).all())
    for i in range(cases.REPEATS):
        assert torch.equal(ops.colsum_bf16(xd), first), f"repeat {i}"


# ---------------------------------------------------------------------------
# front doors
# ---------------------------------------------------------------------------

def _logical(p, layout):
    a = p.a.cuda() if layout[0] == "n" else p.a.t().contiguous().cuda().t()
    b = p.b.cuda() if layout[1] == "n" else p.b.t().contiguous().cuda().t()
    return a, b


@pytest.mark.parametrize("layout", LAYOUTS)
def test_matmul_front_door(ops, layout):
    m, n, k = cases.FRONT_DOOR
    p = cases.exact_payload(m, n, k)
    a, b = _logical(p, layout)
    assert ops.matmul_layout(a, b)[0] == layout
    for bias in (p.bias, p.bias.to(BF16)):      # the half units are bf16
        assert torch.equal(bias.float(), p.bias)
        got = ops.matmul(a, b, out_dtype=BF16, bias=bias.cuda())
        torch.cuda.synchronize()
        assert got.dtype == BF16 and got.shape == (m, n)
        assert got.is_contiguous()
        _exact(got.double(), p.wide, f"matmul {layout}")
    got = ops.matmul(a, b, out_dtype=BF16, bias=p.bias.cuda(), split_k=2)
    _exact(got.double(), p.wide, f"matmul {layout} split_k=2")
    got = ops.matmul(a, b, out_dtype=BF16)
    _exact(got.double(), p.wide - p.bias.double(), f"matmul {layout} no bias")


def _linear_payload():
    """integers with y, dx, dw and dbias all bf16 values: x, w, dy sparse"""
    tokens, n_out, n_in = cases.LINEAR
    g = cases._gen("linear-epilogue")
    x = torch.zeros(tokens, n_in)
    rows = torch.arange(tokens)
    x[rows, (3 * rows) % n_in] = ((rows % 5) - 2).float()
    w = torch.randint(-3, 4, (n_out, n_in), generator=g).float()
    bias = ((torch.arange(n_out) % 101) - 50.5).float()
    # dy: one non-zero per column block of rows, so dw = dy^T x and
    # dbias = sum dy stay small integers
    dy = torch.zeros(tokens, n_out)
    cols = torch.arange(n_out)
    for j in range(3):
        dy[(17 * cols + 601 * j) % tokens, cols] = float(j - 1) + (cols % 2).float()
    return x, w, bias, dy


def _linear_ref(x, w, bias, dy):
    xd = x.double().requires_grad_()
    wd = w.double().requires_grad_()
    bd = bias.double().requires_grad_()
    y = xd @ wd.t() + bd
    y.backward(dy.double())
    return y.detach(), xd.grad, wd.grad, bd.grad


def _run_linear(ops, x, w, bias, dy, **kw):
    xg = x.to(BF16).cuda().requires_grad_()
    wg = w.to(BF16).cuda().requires_grad_()
    bg = None if bias is None else bias.cuda().requires_grad_()
    y = ops.linear_bf16(xg, wg, bias=bg, **kw)
    y.backward(dy.to(BF16).cuda())
    torch.cuda.synchronize()
    return y.detach(), xg.grad, wg.grad, None if bg is None else bg.grad


@pytest.mark.parametrize("split_k", [None, "auto"])
def test_linear_bias_against_autograd(ops, split_k):
    x, w, bias, dy = _linear_payload()
    ref = _linear_ref(x, w, bias, dy)
    for r in ref:   # every result is a bf16 value
        assert torch.equal(r.float().to(BF16).double(), r)
    tokens, n_out, n_in = cases.LINEAR
    if split_k == "auto":
        assert ops.gemm_splitk_plan(n_out, n_in, tokens) > 1   # dw splits
    got = _run_linear(ops, x, w, bias, dy, split_k=split_k)
    for g, r, name in zip(got, ref, ("y", "dx", "dw", "dbias")):
        assert g.dtype == (torch.float32 if name == "dbias" else BF16)
        assert torch.equal(g.cpu().double(), r), name
    # fused=False with a bias: the composition, same numbers here
    unf = _run_linear(ops, x, w, bias, dy, split_k=split_k, fused=False)
    for g, u, name in zip(got, unf, ("y", "dx", "dw", "dbias")):
        assert torch.equal(g, u), name
    # a bf16 bias gets a bf16 gradient
    gb = _run_linear(ops, x, w, bias.to(BF16), dy, split_k=split_k)
    assert gb[3].dtype == BF16 and torch.equal(gb[3].cpu().double(), ref[3])


def test_linear_fused_without_bias_equals_default(ops):
    x, w, _, dy = _linear_payload()
    default = _run_linear(ops, x, w, None, dy)
    fused = _run_linear(ops, x, w, None, dy, fused=True)
    for d, f, name in zip(default[:3], fused[:3], ("y", "dx", "dw")):
        assert torch.equal(d, f), name


def test_linear_frozen_operand_skips_its_product(ops, monkeypatch):
    x, w, bias, dy = _linear_payload()
    calls = []
    real = ops.matmul

    def spy(a, b, **kw):
        calls.append(ops.matmul_layout(a, b)[0])
        return real(a, b, **kw)

    monkeypatch.setattr(ops, "matmul", spy)
    xg = x.to(BF16).cuda()
    wg = w.to(BF16).cuda().requires_grad_()
    ops.linear_bf16(xg, wg, bias=bias.cuda()).backward(dy.to(BF16).cuda())
    assert calls == ["nt", "tn"] and wg.grad is not None
    calls.clear()
    xg = x.to(BF16).cuda().requires_grad_()
    wg = w.to(BF16).cuda()
    bg = bias.cuda().requires_grad_()
    ops.linear_bf16(xg, wg, bias=bg).backward(dy.to(BF16).cuda())
    assert calls == ["nt", "nn"] and xg.grad is not None and bg.grad is not None


def test_error_paths(ops):
    p = cases.exact_payload(*cases.EXACT[0])
    a, b = p.a.cuda(), p.b.t().contiguous().cuda()
    c = _poison((128, 128), BF16)
    bias = p.bias.cuda()
    with pytest.raises(TypeError):
        ops.gemm_bf16_epilogue(_poison((128, 128)), a, b)         # fp32 c
    with pytest.raises(TypeError):
        ops.gemm_bf16_epilogue(c, a.float(), b)
    with pytest.raises(TypeError):
        ops.gemm_bf16_epilogue(c, a, b, bias=bias.to(BF16))
    with pytest.raises(TypeError):
        ops.gemm_bf16_epilogue(c, a, b, bias=bias.cpu())
    with pytest.raises(TypeError):
        ops.gemm_bf16_epilogue(c, a.t(), b)                       # strided
    with pytest.raises(ValueError):
        ops.gemm_bf16_epilogue(c, a, b, bias=bias[:64])
    with pytest.raises(ValueError):
        ops.gemm_bf16_epilogue(c, a, b, layout="tx")
    with pytest.raises(ValueError):
        ops.gemm_bf16_epilogue(c, a, b, splits=2)                 # K/64 = 1
    with pytest.raises(ValueError):
        ops.gemm_bf16_epilogue(c, a, b[:64])
    with pytest.raises(ValueError):
        ops.gemm_bf16_epilogue(c, a[:100], b)
    with pytest.raises(TypeError):
        ops.colsum_bf16(a.float())
    with pytest.raises(ValueError):
        ops.colsum_bf16(a, out=_poison((65,)))
    assert bool(torch.isnan(c).all())                             # untouched

"""The activation epilogues (native/gemm_act.hip) on the GPU. ReLU is judged
bit for bit; GELU by the interval rule of gemm_act_cases (docs/gemm.md,
"Activations") against float64 of the fp32 C of the kernels that existed
(gemm_bf16 under HPK_GEMM_VARIANT=db, gemm_bf16_layout, the split-K pair),
taken to the CPU. C, aux_out and a caller's workspace are NaN before every
call."""

import pytest
import torch

import gemm_act_cases as act
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


def _ruled(got, ref, delta, what):
    """the acceptance rule, with the share of ambiguous intervals capped"""
    got = got.cpu()
    share = act.ambiguous_share(ref, delta)
    ok = act.accepted(got, ref, delta)
    print(f"{what}: ambiguous intervals {share:.4%}, outside "
          f"{int((~ok).sum())} of {ok.numel()}")
    assert share <= act.AMBIGUOUS_CAP, f"{what}: ambiguous share {share}"
    if bool(ok.all()):
        return
    idx = (~ok).nonzero()
    head = [(int(i), int(j), got[i, j].item(), ref[i, j].item())
            for i, j in idx[:8]]
    pytest.fail(f"{what}: {len(idx)} of {got.numel()} outputs outside their "
                f"interval; first (row, col, got, ref): {head}")


def _dev(p, layout):
    return tuple(t.cuda() for t in cases.stored(p, layout))


def _fwd(ops, p, layout, activation, bias=True, aux=False, splits=1,
         workspace=None, **kw):
    a, b = _dev(p, layout)
    m, n = p.a.shape[0], p.b.shape[1]
    c = _poison((m, n), BF16)
    z = _poison((m, n), BF16) if aux else None
    ops.gemm_bf16_act(c, a, b, layout, activation=activation,
                      bias=p.bias.cuda() if bias else None, aux_out=z,
                      splits=splits, workspace=workspace, **kw)
    torch.cuda.synchronize()
    return (c, z) if aux else c


def _grad(ops, p, layout, activation, aux, splits=1, workspace=None, **kw):
    a, b = _dev(p, layout)
    c = _poison((p.a.shape[0], p.b.shape[1]), BF16)
    ops.gemm_bf16_act(c, a, b, layout, activation=activation,
                      grad_aux=aux.cuda(), splits=splits, workspace=workspace,
                      **kw)
    torch.cuda.synchronize()
    return c


def _epilogue(ops, p, layout, bias=True, splits=1):
    """bf16 output of the kernel that existed"""
    a, b = _dev(p, layout)
    c = _poison((p.a.shape[0], p.b.shape[1]), BF16)
    ops.gemm_bf16_epilogue(c, a, b, layout,
                           bias=p.bias.cuda() if bias else None,
                           splits=splits)
    torch.cuda.synchronize()
    return c


def _parent32(ops, p, layout, splits=1):
    """fp32 C of the kernel that existed, on the CPU"""
    a, b = _dev(p, layout)
    m, n = p.a.shape[0], p.b.shape[1]
    c = _poison((m, n))
    if splits > 1:
        ops.gemm_bf16_layout_splitk(c, a, b, layout, splits)  # nt: gemm_splitk
    elif layout == "nt":
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


def _relu16(t):
    return torch.relu(t.float()).to(BF16)


# ---------------------------------------------------------------------------
# ReLU: exact
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", cases.EXACT,
                         ids=["x".join(map(str, s)) for s in cases.EXACT])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_relu_forward_exact(ops, layout, shape):
    p = cases.exact_payload(*shape)
    neg = float((p.bias < 0).double().mean())
    assert 0.3 < neg < 0.7
    c32 = _parent32(ops, p, layout)
    got = _fwd(ops, p, layout, "relu")
    _exact(got.double(), torch.relu(p.wide), f"{layout} {shape} vs float64")
    _exact(got, _relu16(cases.oracle(c32, p.bias)), f"{layout} {shape}")
    assert bool((got == 0).any()) and bool((got > 0).any())
    nob = _fwd(ops, p, layout, "relu", bias=False)
    _exact(nob.double(), torch.relu(p.wide - p.bias.double()),
           f"{layout} {shape} no bias vs float64")
    _exact(nob, _relu16(cases.oracle(c32)), f"{layout} {shape} no bias")
    # aux_out with relu: the pre-activation, the epilogue kernel's bits
    y, z = _fwd(ops, p, layout, "relu", aux=True)
    _exact(y, got, "relu with aux_out")
    _exact(z, cases.oracle(c32, p.bias), "relu aux_out")


@pytest.mark.parametrize("group", [None, "2"])
@pytest.mark.parametrize("swizzle", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ragged_grid(ops, monkeypatch, layout, swizzle, group):
    if group is not None:
        monkeypatch.setenv("HPK_GEMM_GROUP", group)
    p = cases.exact_payload(*cases.RAGGED_GRID)
    what = f"{layout} swizzle={swizzle} group={group}"
    got = _fwd(ops, p, layout, "relu", xcd_swizzle=swizzle)
    _exact(got.double(), torch.relu(p.wide), what)
    m, n = p.wide.shape
    aux = act.hash_sign_aux(m, n)
    acc = p.wide - p.bias.double()              # exact, a bf16 value
    d = _grad(ops, p, layout, "relu", aux, xcd_swizzle=swizzle)
    _exact(d.double(), acc * (aux.double() > 0), what + " gradient")


@pytest.mark.parametrize("activation", ["relu", "gelu"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_identity_shows_a_transposed_aux(ops, layout, activation):
    p = cases.identity_payload()
    m, n = p.wide.shape
    acc = p.wide - p.bias.double()              # = b
    aux = act.hash_sign_aux(m, n)
    d = _grad(ops, p, layout, activation, aux)
    if activation == "relu":
        _exact(d.double(), acc * (aux.double() > 0), f"{layout} identity")
        return
    acc32 = _parent32(ops, p, layout)
    assert torch.equal(acc32.double(), acc)
    _ruled(d, *act.grad_ref(ops, acc32, aux), f"{layout} identity gelu")


# ---------------------------------------------------------------------------
# GELU
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", act.GELU_SHAPES,
                         ids=["x".join(map(str, s)) for s in act.GELU_SHAPES])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gelu_forward(ops, layout, shape):
    p = act.gelu_payload(*shape)
    z32 = _parent32(ops, p, layout) + p.bias
    assert float(z32.abs().max()) <= act.Z_MAX
    y, z = _fwd(ops, p, layout, "gelu", aux=True)
    _ruled(y, *act.forward_ref(ops, z32), f"{layout} {shape} gelu")
    _exact(z, _epilogue(ops, p, layout), f"{layout} {shape} aux_out")
    _exact(_fwd(ops, p, layout, "gelu"), y, f"{layout} {shape} no aux_out")
    nob = _fwd(ops, p, layout, "gelu", bias=False)
    _ruled(nob, *act.forward_ref(ops, z32 - p.bias),
           f"{layout} {shape} gelu no bias")


@pytest.mark.parametrize("shape", act.GELU_SHAPES,
                         ids=["x".join(map(str, s)) for s in act.GELU_SHAPES])
@pytest.mark.parametrize("layout", ["nn", "tn"])
def test_gelu_gradient(ops, layout, shape):
    p = act.gelu_payload(*shape)
    acc32 = _parent32(ops, p, layout)
    d = _grad(ops, p, layout, "gelu", p.aux)
    _ruled(d, *act.grad_ref(ops, acc32, p.aux), f"{layout} {shape} dgelu")
    # gelu'(0) = 0.5 exactly: E = 1, R = 0.5, s = 0.5, the second term 0
    half = _grad(ops, p, layout, "gelu", torch.zeros_like(p.aux))
    _exact(half, (0.5 * acc32).to(BF16), f"{layout} {shape} gelu'(0)")
    # relu on the same accumulators, aux = z or y alike
    mask = p.aux.double() > 0
    for aux in (p.aux, torch.relu(p.aux.float()).to(BF16)):
        r = _grad(ops, p, layout, "relu", aux)
        _exact(r, (acc32.double() * mask).float().to(BF16),
               f"{layout} {shape} drelu")


@pytest.mark.parametrize("layout", ["nt", "tn"])
def test_specials(ops, layout):
    inf, nan = float("inf"), float("nan")
    base = act.gelu_payload(*act.GELU_SHAPES[0])
    m, n = base.a.shape[0], base.b.shape[1]
    rows = {37: inf, 38: -inf, 39: nan}
    a = base.a.clone()
    b = base.b.clone()
    b[5] = b[5].abs() + 1.0         # a[r, 5] = +-Inf: row r is +-Inf, no NaN
    for r, v in rows.items():
        a[r, 5] = v
    p = act.GeluPayload(a, b, base.bias, None)
    z32 = _parent32(ops, p, layout) + p.bias
    assert bool((z32[37] == inf).all()) and bool((z32[38] == -inf).all())
    assert bool(torch.isnan(z32[39]).all())
    clean = torch.ones(m, dtype=torch.bool)
    clean[list(rows)] = False
    assert bool(torch.isfinite(z32[clean]).all())
    y, z = _fwd(ops, p, layout, "gelu", aux=True)
    y, z = y.cpu(), z.cpu()
    _same(z, z32.to(BF16), f"{layout} specials aux_out")
    assert bool((y[37] == inf).all())
    assert bool(torch.isnan(y[38]).all()) and bool(torch.isnan(y[39]).all())
    assert bool(torch.isfinite(y[clean]).all())
    ref, delta = act.forward_ref(ops, z32[clean])
    assert bool(act.accepted(y[clean], ref, delta).all())
    r = _fwd(ops, p, layout, "relu").cpu()
    assert bool((r[37] == inf).all()) and bool((r[38] == 0).all())
    assert bool(torch.isnan(r[39]).all())
    _same(r[clean], torch.relu(z32[clean]).to(BF16), f"{layout} relu rest")
    # z >= 16: gelu returns z; z <= -20: -0 or a tiny negative; +-0
    bias = torch.zeros(n)
    bias[:32] = 16.0 + torch.arange(32.0)
    bias[32:64] = -20.0 - torch.arange(32.0)
    q = act.GeluPayload(torch.zeros_like(base.a), base.b, bias, None)
    y = _fwd(ops, q, layout, "gelu").cpu().float()
    assert torch.equal(y[:, :32], bias[:32].to(BF16).float().expand(m, 32))
    assert bool((y[:, 32:64] <= 0).all()) and bool((y[:, 32:64] > -1e-30).all())
    assert bool((y[:, 64:] == 0).all())
    neg = act.GeluPayload(-q.a, base.b, None, None)     # acc = -0
    y0 = _fwd(ops, neg, layout, "gelu", bias=False).cpu()
    assert bool((y0 == 0).all())


# ---------------------------------------------------------------------------
# split-K
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("splits", (2, 3, 5))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_splitk(ops, layout, splits):
    m, n, k = cases.SPLITK
    e = cases.exact_payload(m, n, k)
    ws = _poison((splits * m * n,))
    got = _fwd(ops, e, layout, "relu", splits=splits, workspace=ws)
    _exact(got, _relu16(_epilogue(ops, e, layout, splits=splits)),
           f"{layout} S={splits} relu")
    _exact(got.double(), torch.relu(e.wide), f"{layout} S={splits} float64")
    assert not bool(torch.isnan(ws).any())
    aux = act.hash_sign_aux(m, n)
    d = _grad(ops, e, layout, "relu", aux, splits=splits)
    _exact(d.double(), (e.wide - e.bias.double()) * (aux.double() > 0),
           f"{layout} S={splits} drelu")
    p = act.gelu_payload(m, n, k)
    c32 = _parent32(ops, p, layout, splits)
    y, z = _fwd(ops, p, layout, "gelu", aux=True, splits=splits)
    _ruled(y, *act.forward_ref(ops, c32 + p.bias), f"{layout} S={splits} gelu")
    _exact(z, _epilogue(ops, p, layout, splits=splits),
           f"{layout} S={splits} aux_out")
    _exact(_fwd(ops, p, layout, "gelu", splits=splits), y, "no aux_out")
    d = _grad(ops, p, layout, "gelu", p.aux, splits=splits)
    _ruled(d, *act.grad_ref(ops, c32, p.aux), f"{layout} S={splits} dgelu")


@pytest.mark.parametrize("layout", ["nt", "tn"])
def test_fold_grid_stride(ops, layout):
    m, n, k, splits = cases.GRID_STRIDE
    e = cases.exact_payload(m, n, k)
    got = _fwd(ops, e, layout, "relu", splits=splits)
    _exact(got.double(), torch.relu(e.wide), f"{layout} grid-stride relu")
    aux = act.hash_sign_aux(m, n)
    d = _grad(ops, e, layout, "relu", aux, splits=splits)
    _exact(d.double(), (e.wide - e.bias.double()) * (aux.double() > 0),
           f"{layout} grid-stride drelu")
    p = act.gelu_payload(m, n, k)
    c32 = _parent32(ops, p, layout, splits)
    y = _fwd(ops, p, layout, "gelu", splits=splits)
    _ruled(y, *act.forward_ref(ops, c32 + p.bias), f"{layout} grid-stride gelu")
    d = _grad(ops, p, layout, "gelu", p.aux, splits=splits)
    _ruled(d, *act.grad_ref(ops, c32, p.aux), f"{layout} grid-stride dgelu")


# ---------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("activation", ["relu", "gelu"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_repeats_give_the_same_bits(ops, layout, activation):
    p = act.gelu_payload(*cases.RANDN)
    y0, z0 = _fwd(ops, p, layout, activation, aux=True)
    d0 = _grad(ops, p, layout, activation, p.aux)
    s0 = _fwd(ops, p, layout, activation, splits=3)
    for i in range(cases.REPEATS):
        y, z = _fwd(ops, p, layout, activation, aux=True)
        assert torch.equal(y, y0) and torch.equal(z, z0), f"repeat {i}"
        assert torch.equal(_grad(ops, p, layout, activation, p.aux), d0)
        assert torch.equal(_fwd(ops, p, layout, activation, splits=3), s0)
    assert not bool(torch.isnan(y0).any()) and not bool(torch.isnan(d0).any())


# ---------------------------------------------------------------------------
# front doors
# ---------------------------------------------------------------------------

def _logical(a, b, layout):
    a = a.cuda() if layout[0] == "n" else a.t().contiguous().cuda().t()
    b = b.cuda() if layout[1] == "n" else b.t().contiguous().cuda().t()
    return a, b


@pytest.mark.parametrize("layout", LAYOUTS)
def test_matmul_front_door(ops, layout):
    m, n, k = cases.FRONT_DOOR
    e = cases.exact_payload(m, n, k)
    a, b = _logical(e.a, e.b, layout)
    assert ops.matmul_layout(a, b)[0] == layout
    bias = e.bias.cuda()
    got = ops.matmul(a, b, out_dtype=BF16, bias=bias, activation="relu")
    assert got.dtype == BF16 and got.shape == (m, n) and got.is_contiguous()
    _exact(got.double(), torch.relu(e.wide), f"matmul {layout} relu")
    y, z = ops.matmul(a, b, out_dtype=BF16, bias=bias, activation="relu",
                      return_aux=True, split_k=2)
    assert z.shape == (m, n) and z.is_contiguous()
    _exact(y.double(), torch.relu(e.wide), f"matmul {layout} relu split")
    _exact(z.double(), e.wide, f"matmul {layout} aux")
    aux = act.hash_sign_aux(m, n)
    acc = e.wide - e.bias.double()
    for kw in ({}, {"split_k": 2}):
        d = ops.matmul(a, b, out_dtype=BF16,
                       activation_grad=("relu", aux.cuda()), **kw)
        assert d.shape == (m, n) and d.is_contiguous()
        _exact(d.double(), acc * (aux.double() > 0), f"matmul {layout} drelu")
    # gelu through the padding: the existing front door gives z32's bf16
    # only, so the fp32 reference is the padded parent kernel's
    p = act.gelu_payload(128, 256, 128)
    pa, pb = p.a[:m, :k], p.b[:k, :n]
    q = act.GeluPayload(torch.zeros(128, 128, dtype=BF16),
                        torch.zeros(128, 256, dtype=BF16), p.bias, None)
    q.a[:m, :k] = pa
    q.b[:k, :n] = pb
    c32 = _parent32(ops, q, layout)[:m, :n]
    z32 = c32 + p.bias[:n]
    la, lb = _logical(pa.contiguous(), pb.contiguous(), layout)
    y, z = ops.matmul(la, lb, out_dtype=BF16, bias=p.bias[:n].cuda(),
                      activation="gelu", return_aux=True)
    _ruled(y, *act.forward_ref(ops, z32), f"matmul {layout} gelu")
    _exact(z, ops.matmul(la, lb, out_dtype=BF16, bias=p.bias[:n].cuda()),
           f"matmul {layout} gelu aux")
    gaux = p.aux[:m, :n].contiguous()
    d = ops.matmul(la, lb, out_dtype=BF16,
                   activation_grad=("gelu", gaux.cuda()))
    _ruled(d, *act.grad_ref(ops, c32, gaux),
           f"matmul {layout} dgelu")


# ---------------------------------------------------------------------------
# mlp_bf16
# ---------------------------------------------------------------------------

NAMES = ("y", "dx", "dw1", "db1", "dw2", "db2")


def _mlp_tensors(tokens, requires=(True,) * 5):
    x, w1, b1, w2, b2, dy = act.mlp_payload(tokens, *act.MLP[1:])
    leaves = [t.cuda().requires_grad_(r)
              for t, r in zip((x, w1, b1, w2, b2), requires)]
    return leaves, dy.cuda()


def _run(fn, leaves, dy):
    y = fn(*leaves)
    y.backward(dy)
    torch.cuda.synchronize()
    x, w1, b1, w2, b2 = leaves
    return (y.detach(), x.grad, w1.grad, b1.grad, w2.grad, b2.grad)


@pytest.mark.parametrize("tokens,split_k", [(act.MLP[0], None),
                                            (cases.LINEAR[0], "auto")])
def test_mlp_relu_equals_the_composition(ops, tokens, split_k):
    if split_k == "auto":
        assert ops.gemm_splitk_plan(act.MLP[2], act.MLP[1], tokens) > 1

    def composed(x, w1, b1, w2, b2):
        h = torch.relu(ops.linear_bf16(x, w1, bias=b1, fused=True,
                                       split_k=split_k))
        return ops.linear_bf16(h, w2, bias=b2, fused=True, split_k=split_k)

    ref = _run(composed, *_mlp_tensors(tokens))
    got = _run(lambda *t: ops.mlp_bf16(*t, activation="relu",
                                       split_k=split_k),
               *_mlp_tensors(tokens))
    for g, r, name in zip(got, ref, NAMES):
        assert g.dtype == r.dtype and g.shape == r.shape, name
        assert not bool(torch.isnan(g).any()), name
        assert torch.equal(g, r), name
    assert bool((got[1] != 0).any()) and bool((got[3] != 0).any())


@pytest.mark.parametrize("tokens,split_k", [(act.MLP[0], None),
                                            (cases.LINEAR[0], "auto")])
def test_mlp_gelu_chain_of_custody(ops, monkeypatch, tokens, split_k):
    leaves, dy = _mlp_tensors(tokens)
    calls = []
    real = ops.matmul

    def spy(a, b, **kw):
        out = real(a, b, **kw)
        calls.append((a, b, kw, out))
        return out

    monkeypatch.setattr(ops, "matmul", spy)
    got = _run(lambda *t: ops.mlp_bf16(*t, activation="gelu",
                                       split_k=split_k), leaves, dy)
    monkeypatch.setattr(ops, "matmul", real)
    assert [ops.matmul_layout(c[0], c[1])[0] for c in calls] \
        == ["nt", "nt", "nn", "nn", "tn", "tn"]
    h, z = calls[0][3]
    dz = calls[2][3]
    x, w1, b1, w2, b2 = (t.detach() for t in leaves)
    kw = dict(out_dtype=BF16, split_k=split_k)
    # h and dz by the rule, from fp32 results of the existing kernels
    z_old = real(x, w1.t(), bias=b1, **kw)
    _exact(z, z_old, "z")
    xp = act.GeluPayload(x.cpu(), w1.t().cpu(), b1.cpu(), None)
    plan1 = ops.gemm_splitk_plan(tokens, act.MLP[2], act.MLP[1]) \
        if split_k else 1
    z32 = _parent32(ops, xp, "nt", plan1) + b1.cpu()
    assert float(z32.abs().max()) <= act.Z_MAX
    _ruled(h, *act.forward_ref(ops, z32), "h")
    dp = act.GeluPayload(dy.cpu(), w2.cpu(), None, None)
    plan2 = ops.gemm_splitk_plan(tokens, act.MLP[2], act.MLP[3]) \
        if split_k else 1
    acc32 = _parent32(ops, dp, "nn", plan2)
    _ruled(dz, *act.grad_ref(ops, acc32, z_old.cpu()), "dz")
    # everything downstream: the existing calls on that h and that dz
    want = (real(h, w2.t(), bias=b2, **kw), real(dz, w1, **kw),
            real(dz.t(), x, **kw), ops.colsum_bf16(dz),
            real(dy.t(), h, **kw), ops.colsum_bf16(dy))
    torch.cuda.synchronize()
    for g, r, name in zip(got, want, NAMES):
        assert g.dtype == r.dtype and g.shape == r.shape, name
        assert torch.equal(g, r), name


def test_mlp_computes_only_the_gradients_asked_for(ops, monkeypatch):
    calls = []
    real = ops.matmul
    monkeypatch.setattr(ops, "matmul", lambda a, b, **kw: calls.append(
        ops.matmul_layout(a, b)[0]) or real(a, b, **kw))
    leaves, dy = _mlp_tensors(act.MLP[0], (False, False, False, True, True))
    got = _run(lambda *t: ops.mlp_bf16(*t, activation="gelu"), leaves, dy)
    assert calls == ["nt", "nt", "tn"]              # no dz at all
    assert [g is None for g in got] == [False, True, True, True, False, False]
    calls.clear()
    leaves, dy = _mlp_tensors(act.MLP[0], (False, False, True, False, False))
    got = _run(lambda *t: ops.mlp_bf16(*t, activation="relu"), leaves, dy)
    assert calls == ["nt", "nt", "nn"]              # dz for db1 alone
    assert [g is None for g in got] == [False, True, True, False, True, True]
    calls.clear()
    x, w1, b1, w2, b2, dyc = act.mlp_payload(act.MLP[0], *act.MLP[1:])
    xg = x.cuda().requires_grad_()
    y = ops.mlp_bf16(xg, w1.cuda(), None, w2.cuda(), None)
    y.backward(dyc.cuda())
    assert calls == ["nt", "nt", "nn", "nn"] and xg.grad is not None


def test_error_paths(ops):
    p = cases.exact_payload(*cases.EXACT[0])
    a, b = p.a.cuda(), p.b.t().contiguous().cuda()
    c = _poison((128, 128), BF16)
    aux = _poison((128, 128), BF16)
    bias = p.bias.cuda()
    with pytest.raises(ValueError, match="activation must be one of"):
        ops.gemm_bf16_act(c, a, b)
    with pytest.raises(ValueError, match="neither bias nor aux_out"):
        ops.gemm_bf16_act(c, a, b, activation="relu", grad_aux=aux, bias=bias)
    with pytest.raises(ValueError, match="neither bias nor aux_out"):
        ops.gemm_bf16_act(c, a, b, activation="relu", grad_aux=aux,
                          aux_out=aux)
    with pytest.raises(TypeError):
        ops.gemm_bf16_act(c, a, b, activation="gelu", aux_out=aux.float())
    with pytest.raises(ValueError):
        ops.gemm_bf16_act(c, a, b, activation="gelu", grad_aux=aux[:64])
    with pytest.raises(ValueError, match="same memory"):
        ops.gemm_bf16_act(c, a, b, activation="gelu", grad_aux=c)
    with pytest.raises(TypeError):
        ops.gemm_bf16_act(_poison((128, 128)), a, b, activation="relu")
    with pytest.raises(ValueError):
        ops.gemm_bf16_act(c, a, b, activation="relu", splits=2)   # K/64 = 1
    with pytest.raises(ValueError):
        ops.gemm_bf16_act(c, a, b, layout="tx", activation="relu")
    assert bool(torch.isnan(c).all()) and bool(torch.isnan(aux).all())

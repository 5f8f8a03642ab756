"""Split-K for the nn/tn/tt layouts (native/gemm_layout_splitk.hip) on the
GPU: bitwise against a float64 CPU reference on exact payloads for every
split count, `torch.equal` with both parents (gemm_splitk, gemm_bf16_layout)
on random operands, the workspace contract, specials, ops.matmul(split_k=)
and ops.linear_bf16(split_k=), and the error paths.

Payloads are built on the CPU in LOGICAL form a [M,K], b [K,N] (integers
-4..4 unless a test says otherwise) and laid out per layout by _stored;
_assert_exact checks the condition under which every summation order is
exact, so that "bitwise equal for every S" is the right expectation. C and
a caller's workspace are NaN before every call."""

import functools
from collections import namedtuple

import pytest
import torch

import gemm_layout_splitk_cases as cases

pytestmark = pytest.mark.gpu

LAYOUTS = ["nn", "tn", "tt"]

Payload = namedtuple("Payload", "a b ref ref_wide")


def _gen(*key):
    # Python's hash() of a str is salted per process; spell the seed out
    s = 0
    for part in key:
        for ch in str(part):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator(device="cpu").manual_seed(s)


def _make(a, b):
    """a [M,K], b [K,N] float tensors holding bf16-exact values"""
    wide = torch.matmul(a.double(), b.double())
    return Payload(a.to(torch.bfloat16), b.to(torch.bfloat16), wide.float(),
                   wide)


@functools.lru_cache(maxsize=None)
def payload(m, n, k, tag=""):
    g = _gen("layout-splitk", m, n, k, tag)
    a = torch.randint(-4, 5, (m, k), generator=g).float()
    b = torch.randint(-4, 5, (k, n), generator=g).float()
    return _make(a, b)


def _assert_exact(p):
    """Integer operands, every partial sum over any subset of k exact in
    fp32 in any order, and the wide reference survives the cast to fp32."""
    k = p.a.shape[1]
    av, bv = p.a.double(), p.b.double()
    assert torch.equal(av, av.round()) and torch.equal(bv, bv.round())
    assert k * float(av.abs().max()) * float(bv.abs().max()) < 2 ** 24
    assert torch.equal(p.ref.double(), p.ref_wide)


def _stored(p, layout):
    """the operands as layout stores them, on the GPU, contiguous"""
    a = p.a.t().contiguous() if layout[0] == "t" else p.a
    b = p.b.t().contiguous() if layout[1] == "t" else p.b
    return a.cuda(), b.cuda()


def _poison(shape):
    return torch.full(shape, float("nan"), device="cuda")


def _check(got, ref, what):
    got = got.cpu()
    if torch.equal(got, ref):
        return
    idx = (got != ref).nonzero()  # NaN poison compares unequal too
    head = [(int(i), int(j), got[i, j].item(), ref[i, j].item())
            for i, j in idx[:8]]
    pytest.fail(f"{what}: {len(idx)} of {got.numel()} outputs differ; "
                f"first (row, col, got, ref): {head}")


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


def _run(ops, p, layout, splits, ws_extra=0, **kw):
    """gemm_bf16_layout_splitk into a poisoned C with a poisoned caller
    workspace of splits*M*N + ws_extra elements; returns (c, workspace)."""
    a, b = _stored(p, layout)
    m, n = p.ref.shape
    c = _poison((m, n))
    ws = _poison((splits * m * n + ws_extra,))
    ops.gemm_bf16_layout_splitk(c, a, b, layout, splits, workspace=ws, **kw)
    torch.cuda.synchronize()
    return c, ws


# ---------------------------------------------------------------------------
# bitwise on exact payloads
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", cases.BITWISE,
                         ids=["x".join(map(str, s[:3])) + f"-S{s[3]}"
                              for s in cases.BITWISE])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_bitwise(ops, layout, shape):
    m, n, k, splits = shape
    p = payload(m, n, k)
    _assert_exact(p)
    c, ws = _run(ops, p, layout, splits)
    _check(c, p.ref, f"{layout} {shape}")
    if splits == 1:  # C is written directly: the workspace is not touched
        assert bool(torch.isnan(ws).all())
    else:            # every partial is written
        assert not bool(torch.isnan(ws).any())


@pytest.mark.parametrize("group", [None, "2"], ids=["rowmajor", "group2"])
@pytest.mark.parametrize("xcd_swizzle", [False, True],
                         ids=["linear", "swizzle"])
@pytest.mark.parametrize("splits", cases.RAGGED_SPLITS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ragged_grid(ops, monkeypatch, layout, splits, xcd_swizzle, group):
    """15 tiles x S splits of T = 3: the uneven arm of the XCD remap."""
    if group is not None:
        monkeypatch.setenv("HPK_GEMM_GROUP", group)
    p = payload(*cases.RAGGED_GRID)
    _assert_exact(p)
    c, _ = _run(ops, p, layout, splits, xcd_swizzle=xcd_swizzle)
    _check(c, p.ref, f"{layout} ragged S={splits} swizzle={xcd_swizzle} "
                     f"group={group}")


@functools.lru_cache(maxsize=None)
def _row_start_payload(layout):
    """The operand stored [K, X] — A for tn and tt, B for nn — holds
    1 + (k // 64) + 5 * (x % 3): an integer that names the k-row block.
    The other operand is random and asymmetric. A split that starts at
    another split's rows, or steps from row to row by the wrong stride,
    weights the blocks differently and changes C."""
    m, n, k, _ = cases.ROW_START
    g = _gen("row-start", layout)
    block = 1 + torch.arange(k) // 64
    if layout == "nn":
        a = torch.randint(-4, 5, (m, k), generator=g).float()
        b = (block[:, None] + 5 * (torch.arange(n)[None, :] % 3)).float()
    else:
        a = (block[None, :] + 5 * (torch.arange(m)[:, None] % 3)).float()
        b = torch.randint(-4, 5, (k, n), generator=g).float()
    return _make(a, b)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_row_start_of_each_split(ops, layout):
    m, n, k, splits = cases.ROW_START
    p = _row_start_payload(layout)
    _assert_exact(p)
    # the payload tells the blocks apart: swapping two of them changes C
    perm = torch.arange(k)
    perm[0:64], perm[256:320] = torch.arange(256, 320), torch.arange(0, 64)
    a64, b64 = p.a.double(), p.b.double()
    wrong = a64 @ b64[perm] if layout == "nn" else a64[:, perm] @ b64
    assert not torch.equal(wrong, p.ref_wide)
    c, _ = _run(ops, p, layout, splits)
    _check(c, p.ref, f"{layout} row start")


def test_reduce_walks_grid_stride(ops):
    """M*N/4 vectors need more workgroups than the shared fold launches."""
    from hpc_patterns_amd._native import native

    m, n, k, splits = cases.GRID_STRIDE
    assert m * n // 4 // 256 > native().SPLITK_REDUCE_MAX_GRID
    p = payload(m, n, k)
    _assert_exact(p)
    c, _ = _run(ops, p, "tn", splits)
    _check(c, p.ref, "tn grid-stride reduce")


# ---------------------------------------------------------------------------
# random operands: the parents' bits, and the family's analytic bound
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _randn_payload():
    m, n, k = cases.PARENTS
    g = _gen("randn", m, n, k)
    a = torch.randn(m, k, generator=g).to(torch.bfloat16)
    b = torch.randn(k, n, generator=g).to(torch.bfloat16)
    ref = torch.matmul(a.double(), b.double())
    # running-sum bound of an fp32 accumulation of K terms; a fold of S
    # partials of K/S terms stays inside it
    bound = k * 2.0 ** -23 * torch.matmul(a.double().abs(), b.double().abs())
    return Payload(a, b, ref, ref), bound


@pytest.mark.parametrize("splits", cases.PARENT_SPLITS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_random_operands_bit_identical_to_the_parents(ops, layout, splits):
    """Same partition, same MFMA order inside a split, same fold order as
    gemm_splitk on materialised transposes; for S = 1 the layout kernel's
    own bits too."""
    p, _ = _randn_payload()
    m, n = p.ref.shape
    c, _ = _run(ops, p, layout, splits)
    assert not bool(torch.isnan(c).any())
    c_nt = _poison((m, n))
    ops.gemm_splitk(c_nt, p.a.cuda().contiguous(),
                    p.b.cuda().t().contiguous(), splits)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(c_nt).any())
    assert torch.equal(c, c_nt), f"{layout} S={splits} differs from gemm_splitk"
    if splits == 1:
        a, b = _stored(p, layout)
        c_lay = _poison((m, n))
        ops.gemm_bf16_layout(c_lay, a, b, layout)
        torch.cuda.synchronize()
        assert torch.equal(c, c_lay), f"{layout} differs from gemm_bf16_layout"


@pytest.mark.parametrize("splits", cases.PARENT_SPLITS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_random_operands_within_the_family_bound(ops, layout, splits):
    p, bound = _randn_payload()
    c, _ = _run(ops, p, layout, splits)
    err = (c.cpu().double() - p.ref).abs()
    m, n, k = cases.PARENTS
    print(f"layout split-K {layout} randn {m}x{n}x{k} S={splits}: worst "
          f"|err|/bound = {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())


# ---------------------------------------------------------------------------
# workspace contract, streams, determinism
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_oversized_workspace_keeps_its_tail(ops, layout):
    m, n, k = cases.WORKSPACE
    p = payload(m, n, k)
    splits, extra = 3, 4096 + 4
    c, ws = _run(ops, p, layout, splits, ws_extra=extra)
    _check(c, p.ref, f"{layout} oversized workspace")
    assert not bool(torch.isnan(ws[:splits * m * n]).any())
    assert ws[splits * m * n:].numel() == extra
    assert bool(torch.isnan(ws[splits * m * n:]).all())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_partials_are_fresh_on_reuse(ops, layout):
    """Two products with different operands through the same workspace."""
    m, n, k = cases.WORKSPACE
    p1, p2 = payload(m, n, k), payload(m, n, k, "second")
    _assert_exact(p2)
    assert not torch.equal(p1.ref, p2.ref)
    ws = _poison((5 * m * n,))
    for p in (p1, p2):
        a, b = _stored(p, layout)
        c = _poison((m, n))
        ops.gemm_bf16_layout_splitk(c, a, b, layout, 5, workspace=ws)
        torch.cuda.synchronize()
        _check(c, p.ref, f"{layout} workspace reuse")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_workspace_none(ops, layout):
    m, n, k = cases.WORKSPACE
    p = payload(m, n, k)
    a, b = _stored(p, layout)
    c = _poison((m, n))
    ops.gemm_bf16_layout_splitk(c, a, b, layout, 3)
    torch.cuda.synchronize()
    _check(c, p.ref, f"{layout} workspace=None")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_side_stream(ops, layout):
    """Tile kernel and fold both run on the stream given, with a workspace
    allocated inside: synchronizing that stream alone must be enough."""
    m, n, k, splits = cases.SIDE_STREAM
    p = payload(m, n, k)
    a, b = _stored(p, layout)
    c = _poison((m, n))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())  # the poison fill, copies
    ops.gemm_bf16_layout_splitk(c, a, b, layout, splits, stream=side)
    side.synchronize()
    _check(c, p.ref, f"{layout} side stream")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_deterministic(ops, layout):
    """Ten runs, one result; stops at the first difference."""
    p = payload(*cases.RAGGED_GRID)
    a, b = _stored(p, layout)
    m, n = p.ref.shape
    ws = _poison((3 * m * n,))
    first = None
    for i in range(cases.REPEATS):
        c = _poison((m, n))
        ops.gemm_bf16_layout_splitk(c, a, b, layout, 3, workspace=ws)
        if first is None:
            first = c
        else:
            assert torch.equal(c, first), f"{layout}: run {i} differs"
    _check(first, p.ref, f"{layout} repeated")


# ---------------------------------------------------------------------------
# specials (tn)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("side", ["a", "b"])
def test_inf_of_one_split_reaches_its_row_or_column_only(ops, side):
    """An Inf at a k that the LAST split owns (its only tile) meets
    non-zero factors only: row i0 (Inf in a) or column j0 (Inf in b) of C
    is +-Inf by the factor's sign, and every other output is exact."""
    m, n, k, splits = cases.SPECIALS
    from hpc_patterns_amd._native import native
    first, count = native().gemm_splitk_ktiles(k // 64, splits, splits - 1)
    k0, i0, j0 = 64 * first + 17, 37, 90
    assert count == 1 and first * 64 <= k0 < k
    clean = payload(m, n, k, "specials")
    _assert_exact(clean)
    a, b = clean.a.float().clone(), clean.b.float().clone()
    expect = None
    if side == "a":
        b[k0] = torch.where(b[k0] == 0, torch.ones(()), b[k0])
        a[i0, k0] = 0
        expect = torch.matmul(a.double(), b.double()).float()
        expect[i0] = torch.sign(b[k0]) * float("inf")
        a[i0, k0] = float("inf")
    else:
        a[:, k0] = torch.where(a[:, k0] == 0, torch.ones(()), a[:, k0])
        b[k0, j0] = 0
        expect = torch.matmul(a.double(), b.double()).float()
        expect[:, j0] = torch.sign(a[:, k0]) * float("inf")
        b[k0, j0] = float("inf")
    assert int(torch.isinf(expect).sum()) == (n if side == "a" else m)
    p = Payload(a.to(torch.bfloat16), b.to(torch.bfloat16), expect, None)
    c, _ = _run(ops, p, "tn", splits)
    _check(c, expect, f"tn Inf in {side}")


def test_bf16_subnormal_input_is_not_flushed(ops):
    """One product per output of row i0: 2^-133 (a bf16 subnormal) times
    2^100 is the normal fp32 2^-33; the other splits' partials are zeros.
    Neither the MFMA nor the fold may lose it."""
    m, n, k, splits = cases.SPECIALS
    k0, i0 = 150, 37
    a = torch.zeros(m, k)
    a[i0, k0] = 2.0 ** -133
    b = torch.randint(-4, 5, (k, n), generator=_gen("subnormal")).float()
    b[k0] = 2.0 ** 100
    a16, b16 = a.to(torch.bfloat16), b.to(torch.bfloat16)
    assert float(a16[i0, k0].double()) == 2.0 ** -133   # kept by the cast
    assert 0 < float(a16[i0, k0].double()) < 2.0 ** -126
    expect = torch.zeros(m, n)
    expect[i0] = 2.0 ** -33
    assert torch.equal(torch.matmul(a16.double(), b16.double()).float(),
                       expect)
    p = Payload(a16, b16, expect, None)
    c, _ = _run(ops, p, "tn", splits)
    _check(c, expect, "tn bf16 subnormal")


# ---------------------------------------------------------------------------
# front doors
# ---------------------------------------------------------------------------

def _views(p, layout):
    """logical a [M,K], b [K,N] as views of the tensors layout stores"""
    a_st, b_st = _stored(p, layout)
    return (a_st.t() if layout[0] == "t" else a_st,
            b_st.t() if layout[1] == "t" else b_st)


@pytest.mark.parametrize("split_k", [cases.FRONT_DOOR_SPLITS, "auto"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_matmul_split_k_on_a_ragged_shape(ops, layout, split_k):
    m, n, k = cases.FRONT_DOOR
    p = payload(m, n, k)
    _assert_exact(p)
    a, b = _views(p, layout)
    assert a.shape == (m, k) and b.shape == (k, n)
    assert ops.matmul_layout(a, b)[0] == layout
    if split_k == "auto":
        plan = ops.gemm_splitk_plan(m, n, k)
        print(f"plan{cases.FRONT_DOOR} = {plan}")
        assert plan > 1      # the split path is what this case is about
    c = ops.matmul(a, b, split_k=split_k)
    torch.cuda.synchronize()
    assert c.shape == (m, n) and c.dtype == torch.float32
    _check(c, p.ref, f"matmul {layout} split_k={split_k}")


def test_matmul_nt_gets_split_k_passed_on(ops):
    m, n, k = cases.FRONT_DOOR
    p = payload(m, n, k)
    a, b = p.a.cuda(), p.b.t().contiguous().cuda().t()
    assert ops.matmul_layout(a, b)[0] == "nt"
    c = ops.matmul(a, b, split_k=cases.FRONT_DOOR_SPLITS)
    torch.cuda.synchronize()
    _check(c, p.ref, "matmul nt split_k")
    with pytest.raises(ValueError):     # matmul_nt's own bound: it was asked
        ops.matmul(a, b, split_k=10 ** 6)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_matmul_auto_with_plan_one_is_the_unsplit_path(ops, layout):
    m, n, k = cases.PLAN_ONE
    assert ops.gemm_splitk_plan(m, n, k) == 1
    a, b = _views(payload(m, n, k), layout)
    auto = ops.matmul(a, b, split_k="auto")
    plain = ops.matmul(a, b, split_k=None)
    torch.cuda.synchronize()
    assert torch.equal(auto, plain)
    _check(auto, payload(m, n, k).ref, f"matmul {layout} plan 1")


@functools.lru_cache(maxsize=None)
def _linear_payload():
    tokens, n_out, n_in = cases.LINEAR
    g = _gen("linear", tokens, n_out, n_in)
    x = torch.randint(-1, 2, (tokens, n_in), generator=g).float()
    w = torch.randint(-1, 2, (n_out, n_in), generator=g).float()
    dy = torch.randint(-1, 2, (tokens, n_out), generator=g).float()
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    y64 = x64 @ w64.t()
    y64.backward(dy.double())
    # integers below 2^24: exact in the kernels' fp32 in any order, so the
    # bf16 result is the cast of the exact value (dw reaches past 2^8,
    # where bf16 rounds: compare after the cast)
    refs = []
    for t in (y64.detach(), x64.grad, w64.grad):
        assert torch.equal(t, t.round()) and float(t.abs().max()) < 2 ** 24
        refs.append(t.float().to(torch.bfloat16).float())
    return x, w, dy, refs


def _linear(ops, **kw):
    x, w, dy, _ = _linear_payload()
    xd = x.to(torch.bfloat16).cuda().requires_grad_()
    wd = w.to(torch.bfloat16).cuda().requires_grad_()
    y = ops.linear_bf16(xd, wd, **kw)
    y.backward(dy.to(torch.bfloat16).cuda())
    torch.cuda.synchronize()
    assert y.dtype == xd.grad.dtype == wd.grad.dtype == torch.bfloat16
    return y.detach(), xd.grad, wd.grad


def test_linear_bf16_auto_against_float64_autograd(ops):
    tokens, n_out, n_in = cases.LINEAR
    print(f"dW plan = {ops.gemm_splitk_plan(n_out, n_in, tokens)}")
    assert ops.gemm_splitk_plan(n_out, n_in, tokens) > 1   # dW does split
    refs = _linear_payload()[3]
    for got, ref, what in zip(_linear(ops, split_k="auto"), refs,
                              ("forward", "dx", "dw")):
        _check(got.float(), ref, f"linear auto {what}")


def test_linear_bf16_default_is_the_unsplit_composition(ops):
    x, w, dy, refs = _linear_payload()
    xd, wd = x.to(torch.bfloat16).cuda(), w.to(torch.bfloat16).cuda()
    dyd = dy.to(torch.bfloat16).cuda()
    before = (ops.matmul_nt(xd, wd).to(torch.bfloat16),
              ops.matmul(dyd, wd).to(torch.bfloat16),
              ops.matmul(dyd.t(), xd).to(torch.bfloat16))
    torch.cuda.synchronize()
    default, explicit = _linear(ops), _linear(ops, split_k=None)
    for d, e, b, ref in zip(default, explicit, before, refs):
        assert torch.equal(d, e) and torch.equal(d, b)
        _check(d.float(), ref, "linear default")


# ---------------------------------------------------------------------------
# error paths
# ---------------------------------------------------------------------------

def test_error_paths_raise_before_any_launch(ops):
    m, n, k = 128, 384, 256
    a = torch.ones(k, m, device="cuda").to(torch.bfloat16)      # tn: [K,M]
    b = torch.ones(k, n, device="cuda").to(torch.bfloat16)      # tn: [K,N]
    c = _poison((m, n))

    def ws(numel, dtype=torch.float32):
        return torch.zeros(numel, dtype=dtype, device="cuda")

    with pytest.raises(ValueError):
        ops.gemm_bf16_layout_splitk(c, a, b, "tn", 0)
    with pytest.raises(ValueError):
        ops.gemm_bf16_layout_splitk(c, a, b, "tn", k // 64 + 1)
    with pytest.raises(ValueError):  # too small
        ops.gemm_bf16_layout_splitk(c, a, b, "tn", 2,
                                    workspace=ws(2 * m * n - 1))
    with pytest.raises(ValueError):  # a view offset by one element
        ops.gemm_bf16_layout_splitk(c, a, b, "tn", 2,
                                    workspace=ws(2 * m * n + 4)[1:])
    with pytest.raises(TypeError):   # wrong dtype
        ops.gemm_bf16_layout_splitk(c, a, b, "tn", 2,
                                    workspace=ws(2 * m * n, torch.int32))
    with pytest.raises(ValueError):  # unknown layout
        ops.gemm_bf16_layout_splitk(c, a, b, "nx", 2)
    with pytest.raises(ValueError):  # shapes read in the wrong layout
        ops.gemm_bf16_layout_splitk(c, a, b, "tt", 2)
    with pytest.raises(ValueError):  # non-tile M
        ops.gemm_bf16_layout_splitk(_poison((64, n)), a[:, :64].contiguous(),
                                    b, "tn", 2)
    a8 = torch.zeros(k, m, device="cuda").to(torch.float8_e4m3fn)
    ai = torch.zeros(k, m, dtype=torch.int8, device="cuda")
    with pytest.raises(TypeError, match="transposed"):
        ops.gemm_bf16_layout_splitk(c, a8, a8, "tn", 2)
    with pytest.raises(TypeError, match="transposed"):
        ops.gemm_bf16_layout_splitk(c, ai, ai, "tn", 2)
    with pytest.raises(TypeError, match="transposed"):
        ops.matmul(ai.t(), ai, split_k=2)
    for bad in (True, 2.0, "Auto"):  # split_k with a bad type
        with pytest.raises(ValueError, match="split_k"):
            ops.matmul(a.t(), b, split_k=bad)
        with pytest.raises(ValueError, match="split_k"):
            ops.linear_bf16(a, a, split_k=bad)
    with pytest.raises(ValueError, match="split_k"):
        ops.linear_bf16(a, a, split_k=2)
    with pytest.raises(ValueError, match="K_padded"):
        ops.matmul(a.t(), b, split_k=k // 64 + 1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(c).all())


def test_native_launcher_guards_itself(ops):
    from hpc_patterns_amd._native import native

    hpk = native()
    m, n, k = 128, 128, 256
    a = torch.ones(k, m, device="cuda").to(torch.bfloat16)
    c = _poison((m, n))
    w = torch.zeros(4 * m * n + 4, device="cuda")
    args = (c.data_ptr(), a.data_ptr(), a.data_ptr())
    for mm, nn, kk, splits, wptr in [
            (64, n, k, 1, 0), (m, 64, k, 1, 0), (m, n, 32, 1, 0),
            (m, n, k, 0, w.data_ptr()), (m, n, k, k // 64 + 1, w.data_ptr()),
            (m, n, k, 2, 0), (m, n, k, 2, w.data_ptr() + 4)]:
        with pytest.raises(RuntimeError):
            hpk.gemm_bf16_layout_splitk(*args, mm, nn, kk, "tn", splits, wptr)
    with pytest.raises(RuntimeError):    # an operand off a 16-byte boundary
        hpk.gemm_bf16_layout_splitk(c.data_ptr(), a.data_ptr() + 2,
                                    a.data_ptr(), m, n, k, "tn", 1, 0)
    for lay in ("nt", "NN", ""):
        with pytest.raises(ValueError):
            hpk.gemm_bf16_layout_splitk(*args, m, n, k, lay, 2, w.data_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(c).all())

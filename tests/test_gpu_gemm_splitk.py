"""Split-K GEMM (native/gemm_splitk.hip) on the GPU: bitwise against a
float64 / int64 CPU reference for every split count, then the workspace
contract, stream handling, random operands, matmul_nt(split_k=...) and the
error paths.

Payloads are built on the CPU: integers -4..4 for bf16 and fp8, full-range
int8. _assert_exact checks, per payload, the condition under which "bitwise
equal for every S and any summation order" is the right expectation."""

import functools
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = ["bf16", "fp8", "i8"]
_IN_DTYPE = {"bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn,
             "i8": torch.int8}
_I32_POISON = 0x7FFFFFFF

Payload = namedtuple("Payload", "kind a b ref ref_wide")


def _gen(*key):
    # Python's hash() of a str is salted per process; spell the seed out
    s = 0
    for part in key:
        for ch in str(part):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator(device="cpu").manual_seed(s)


def _operand(kind, rows, k, g):
    if kind == "i8":
        return torch.randint(-128, 128, (rows, k), generator=g,
                             dtype=torch.int8)
    f = torch.randint(-4, 5, (rows, k), generator=g).float()
    return f.to(_IN_DTYPE[kind])


def _reference(kind, a, b):
    if kind == "i8":
        wide = torch.matmul(a.long(), b.long().t())
        return wide.to(torch.int32), wide
    wide = torch.matmul(a.double(), b.double().t())
    return wide.float(), wide


@functools.lru_cache(maxsize=None)
def payload(kind, m, n, k, tag=""):
    g = _gen("splitk", kind, m, n, k, tag)
    a, b = _operand(kind, m, k, g), _operand(kind, n, k, g)
    return Payload(kind, a, b, *_reference(kind, a, b))


def _assert_exact(p):
    """Every partial sum, over any subset of k and in any order, is exact
    in the accumulator, and the wide reference survives the cast to C's
    dtype — so every split count must give the same bits."""
    k = p.a.shape[1]
    if p.kind == "i8":
        assert 128 * 128 * k < 2 ** 31
        assert torch.equal(p.ref.long(), p.ref_wide)
        return
    av, bv = p.a.double(), p.b.double()
    assert torch.equal(av, av.round()) and torch.equal(bv, bv.round())
    assert k * float(av.abs().max()) * float(bv.abs().max()) < 2 ** 24
    assert torch.equal(p.ref.double(), p.ref_wide)


def _poison(shape, kind):
    if kind == "i8":
        return torch.full(shape, _I32_POISON, dtype=torch.int32,
                          device="cuda")
    return torch.full(shape, float("nan"), device="cuda")


def _is_poison(t, kind):
    if kind == "i8":
        return bool((t == _I32_POISON).all())
    return bool(torch.isnan(t).all())


def _check(got, p, what):
    got = got.cpu()
    if torch.equal(got, p.ref):
        return
    idx = (got != p.ref).nonzero()  # NaN poison compares unequal too
    head = [(int(i), int(j), got[i, j].item(), p.ref[i, j].item())
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
def _no_group_env(monkeypatch):
    monkeypatch.delenv("HPK_GEMM_GROUP", raising=False)


def _run(ops, p, splits, ws_extra=0, xcd_swizzle=False, a=None):
    """gemm_splitk into a poisoned C with a poisoned caller workspace of
    splits*M*N + ws_extra elements; returns (c, workspace)."""
    m, n = p.ref.shape
    c = _poison((m, n), p.kind)
    ws = _poison((splits * m * n + ws_extra,), p.kind)
    ops.gemm_splitk(c, p.a.cuda() if a is None else a, p.b.cuda(), splits,
                    workspace=ws, xcd_swizzle=xcd_swizzle)
    torch.cuda.synchronize()
    return c, ws


# (M, N, K, S): single trip into C; uneven partition and one-tile splits;
# multi-tile splits, where the pipeline reaches its steady state
_BITWISE = [(128, 128, 64, 1), (128, 128, 320, 2), (128, 128, 320, 3),
            (128, 128, 320, 5), (128, 128, 1024, 4)]


@pytest.mark.parametrize("shape", _BITWISE,
                         ids=["x".join(map(str, s[:3])) + f"-S{s[3]}"
                              for s in _BITWISE])
@pytest.mark.parametrize("kind", KINDS)
def test_bitwise(ops, kind, shape):
    m, n, k, splits = shape
    p = payload(kind, m, n, k)
    _assert_exact(p)
    c, ws = _run(ops, p, splits)
    _check(c, p, f"{kind} {shape}")
    if splits == 1:  # C is written directly: the workspace is not touched
        assert _is_poison(ws, kind)
    else:            # every partial is written
        assert not bool((ws == _I32_POISON).any() if kind == "i8"
                        else torch.isnan(ws).any())


@pytest.mark.parametrize("group", [None, "2"], ids=["rowmajor", "group2"])
@pytest.mark.parametrize("xcd_swizzle", [False, True],
                         ids=["linear", "swizzle"])
@pytest.mark.parametrize("kind", KINDS)
def test_ragged_grid(ops, monkeypatch, kind, xcd_swizzle, group):
    """15 tiles x 3 splits: the uneven arm of the XCD remap (q=1, r=7)."""
    if group is not None:
        monkeypatch.setenv("HPK_GEMM_GROUP", group)
    p = payload(kind, 384, 640, 192)
    _assert_exact(p)
    c, _ = _run(ops, p, 3, xcd_swizzle=xcd_swizzle)
    _check(c, p, f"{kind} ragged swizzle={xcd_swizzle} group={group}")


@pytest.mark.parametrize("kind", KINDS)
def test_reduce_walks_grid_stride(ops, kind):
    """M*N/4 vectors need more workgroups than the fold kernel launches."""
    from hpc_patterns_amd._native import native

    m, n, k = 1152, 1024, 128
    assert m * n // 4 // 256 > native().SPLITK_REDUCE_MAX_GRID
    p = payload(kind, m, n, k)
    _assert_exact(p)
    c, _ = _run(ops, p, 2)
    _check(c, p, f"{kind} grid-stride reduce")


@pytest.mark.parametrize("kind", KINDS)
def test_oversized_workspace_keeps_its_tail(ops, kind):
    p = payload(kind, 128, 128, 320)
    _assert_exact(p)
    splits, extra = 3, 4096 + 4
    c, ws = _run(ops, p, splits, ws_extra=extra)
    _check(c, p, f"{kind} oversized workspace")
    assert _is_poison(ws[splits * 128 * 128:], kind)
    assert ws[splits * 128 * 128:].numel() == extra


@pytest.mark.parametrize("kind", KINDS)
def test_partials_are_fresh_on_reuse(ops, kind):
    """Two products with different A through the same workspace."""
    p1 = payload(kind, 128, 128, 320)
    p2 = payload(kind, 128, 128, 320, "second")
    _assert_exact(p1)
    _assert_exact(p2)
    assert not torch.equal(p1.ref, p2.ref)
    ws = _poison((5 * 128 * 128,), kind)
    for p in (p1, p2):
        c = _poison((128, 128), kind)
        ops.gemm_splitk(c, p.a.cuda(), p.b.cuda(), 5, workspace=ws)
        torch.cuda.synchronize()
        _check(c, p, f"{kind} workspace reuse")


@pytest.mark.parametrize("kind", KINDS)
def test_side_stream(ops, kind):
    """Tile kernel and fold both run on the stream given: synchronizing
    that stream alone must be enough."""
    p = payload(kind, 128, 128, 1024)
    _assert_exact(p)
    a, b = p.a.cuda(), p.b.cuda()
    c = _poison((128, 128), kind)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())  # the poison fill
    ops.gemm_splitk(c, a, b, 4, stream=side)
    side.synchronize()
    _check(c, p, f"{kind} side stream")


@pytest.mark.parametrize("splits", [1, 4, 32])
def test_random_operands(ops, splits):
    m, n, k = 128, 256, 2048
    g = _gen("randn", m, n, k)
    a = torch.randn(m, k, generator=g).to(torch.bfloat16)
    b = torch.randn(n, k, generator=g).to(torch.bfloat16)
    ref = torch.matmul(a.double(), b.double().t())
    # running-sum bound of an fp32 accumulation of K terms; a fold of S
    # partials of K/S terms stays inside it
    bound = k * 2.0 ** -23 * torch.matmul(a.double().abs(),
                                          b.double().abs().t())
    ad, bd = a.cuda(), b.cuda()
    runs = []
    for _ in range(2):
        c = torch.full((m, n), float("nan"), device="cuda")
        ops.gemm_splitk(c, ad, bd, splits)
        torch.cuda.synchronize()
        runs.append(c)
    err = (runs[0].cpu().double() - ref).abs()
    print(f"split-K randn {m}x{n}x{k} S={splits}: worst |err|/bound = "
          f"{float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())
    assert torch.equal(runs[0], runs[1])  # deterministic


def test_matmul_nt_split_count(ops):
    p = payload("bf16", 100, 200, 1000)
    _assert_exact(p)
    c = ops.matmul_nt(p.a.cuda(), p.b.cuda(), split_k=4)
    torch.cuda.synchronize()
    assert c.shape == (100, 200) and c.dtype == torch.float32
    _check(c, p, "matmul_nt split_k=4")


def test_matmul_nt_auto_splits_a_skinny_product(ops):
    p = payload("bf16", 128, 128, 8192)
    _assert_exact(p)
    print(f"plan(128, 128, 8192) = {ops.gemm_splitk_plan(128, 128, 8192)}")
    c = ops.matmul_nt(p.a.cuda(), p.b.cuda(), split_k="auto")
    torch.cuda.synchronize()
    _check(c, p, "matmul_nt split_k=auto")


def test_matmul_nt_auto_leaves_a_full_grid_alone(ops):
    g = _gen("auto-large")
    a = _operand("bf16", 4096, 128, g).cuda()
    b = _operand("bf16", 4096, 128, g).cuda()
    assert ops.gemm_splitk_plan(4096, 4096, 128) == 1
    auto = ops.matmul_nt(a, b, split_k="auto")
    plain = ops.matmul_nt(a, b)
    torch.cuda.synchronize()
    assert torch.equal(auto, plain)


def test_matmul_nt_split_k_refuses_mx(ops):
    a = torch.zeros(128, 128, device="cuda").to(torch.float8_e4m3fn)
    s = torch.full((128, 4), 127, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ops.matmul_nt(a, a, s, s, split_k=2)
    packed = torch.zeros(128, 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ops.matmul_nt(packed, packed, s, s, split_k="auto")


def test_error_paths_raise_before_any_launch(ops):
    m, n, k = 128, 128, 256
    a = torch.ones(m, k, device="cuda").to(torch.bfloat16)
    b = torch.ones(n, k, device="cuda").to(torch.bfloat16)
    c = _poison((m, n), "bf16")

    def ws(numel, dtype=torch.float32):
        return torch.zeros(numel, dtype=dtype, device="cuda")

    with pytest.raises(ValueError):
        ops.gemm_splitk(c, a, b, 0)
    with pytest.raises(ValueError):
        ops.gemm_splitk(c, a, b, k // 64 + 1)
    with pytest.raises(ValueError):  # too small
        ops.gemm_splitk(c, a, b, 2, workspace=ws(2 * m * n - 1))
    with pytest.raises(TypeError):   # wrong dtype
        ops.gemm_splitk(c, a, b, 2, workspace=ws(2 * m * n, torch.int32))
    with pytest.raises(ValueError):  # a view offset by one element
        ops.gemm_splitk(c, a, b, 2, workspace=ws(2 * m * n + 4)[1:])
    with pytest.raises(ValueError):  # M = 64
        ops.gemm_splitk(_poison((64, n), "bf16"), a[:64], b, 2)
    with pytest.raises(TypeError):   # C of the wrong dtype
        ops.gemm_splitk(c.to(torch.int32), a, b, 2)
    torch.cuda.synchronize()
    assert _is_poison(c, "bf16")


def test_native_launchers_guard_themselves(ops):
    from hpc_patterns_amd._native import native

    hpk = native()
    m, n, k = 128, 128, 256
    a = torch.ones(m, k, device="cuda").to(torch.bfloat16)
    c = _poison((m, n), "bf16")
    w = torch.zeros(4 * m * n, device="cuda")
    args = (c.data_ptr(), a.data_ptr(), a.data_ptr())
    for mm, nn, kk, splits, wptr in [
            (64, n, k, 1, 0), (m, 64, k, 1, 0), (m, n, 32, 1, 0),
            (m, n, k, 0, w.data_ptr()), (m, n, k, k // 64 + 1, w.data_ptr()),
            (m, n, k, 2, 0), (m, n, k, 2, w.data_ptr() + 4)]:
        with pytest.raises(RuntimeError):
            hpk.gemm_splitk_bf16_nt(*args, mm, nn, kk, splits, wptr)
    torch.cuda.synchronize()
    assert _is_poison(c, "bf16")

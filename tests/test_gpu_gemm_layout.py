"""bf16 GEMM for nn/tn/tt operand layouts (native/gemm_layout.hip) on the
GPU: bitwise against a float64 CPU reference on exact payloads, against
the NT kernel on random operands, then determinism, streams, ops.matmul,
the error paths and linear_bf16.

Payloads are built on the CPU, in LOGICAL form a [M,K], b [K,N] (integers
-4..4), and laid out per layout by _stored; _assert_exact checks the
condition under which "bitwise equal" is the right expectation."""

import functools
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

LAYOUTS = ["nn", "tn", "tt"]
SINGLE_K = (128, 128, 64)        # the prologue is the epilogue
ONE_SWAP = (128, 128, 128)       # one buffer swap
RAGGED_GRID = (384, 640, 192)    # 15 workgroups, odd trips, M != N != K

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
    g = _gen("layout", m, n, k, tag)
    a = torch.randint(-4, 5, (m, k), generator=g).float()
    b = torch.randint(-4, 5, (k, n), generator=g).float()
    return _make(a, b)


def _assert_exact(p):
    """Integer operands, every partial sum exact in fp32 in any order, and
    the wide reference survives the cast to fp32."""
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


def _run(ops, p, layout, **kw):
    a, b = _stored(p, layout)
    c = _poison(tuple(p.ref.shape))
    ops.gemm_bf16_layout(c, a, b, layout, **kw)
    torch.cuda.synchronize()
    return c


@pytest.mark.parametrize("shape", [SINGLE_K, ONE_SWAP],
                         ids=["single_k", "one_swap"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_bitwise(ops, layout, shape):
    p = payload(*shape)
    _assert_exact(p)
    _check(_run(ops, p, layout), p.ref, f"{layout} {shape}")


@pytest.mark.parametrize("group", [None, "2"], ids=["rowmajor", "group2"])
@pytest.mark.parametrize("xcd_swizzle", [False, True],
                         ids=["linear", "swizzle"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ragged_grid(ops, monkeypatch, layout, xcd_swizzle, group):
    if group is not None:
        monkeypatch.setenv("HPK_GEMM_GROUP", group)
    p = payload(*RAGGED_GRID)
    _assert_exact(p)
    c = _run(ops, p, layout, xcd_swizzle=xcd_swizzle)
    _check(c, p.ref, f"{layout} ragged swizzle={xcd_swizzle} group={group}")


@functools.lru_cache(maxsize=None)
def _identity_payload(which):
    """A = I against an asymmetric B [128,256], or B = I against an
    asymmetric A [256,128]: the output IS the other operand, so a
    transposed or permuted read shows as a transposed or permuted C."""
    m, n, k = 128, 256, 128
    g = _gen("identity", which)
    if which == "a":
        a = torch.eye(m, k)
        b = torch.randint(-4, 5, (k, n), generator=g).float()
        b += torch.arange(n).float()[None, :] % 3   # rows differ from columns
    else:
        m, n = 256, 128
        a = torch.randint(-4, 5, (m, k), generator=g).float()
        a += torch.arange(k).float()[None, :] % 3
        b = torch.eye(k, n)
    return _make(a, b)


@pytest.mark.parametrize("which", ["a", "b"], ids=["A=I", "B=I"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_identity_operand(ops, layout, which):
    p = _identity_payload(which)
    _assert_exact(p)
    other = p.b if which == "a" else p.a
    assert torch.equal(p.ref, other.float())
    assert not torch.equal(other[:128, :128], other[:128, :128].t())
    _check(_run(ops, p, layout), p.ref, f"{layout} {which}=I")


@functools.lru_cache(maxsize=None)
def _gather_payload():
    """Each output is ONE product: A[m, k] is non-zero only at k = kof(m),
    where its value 1 + (m % 16) + 16 * (k % 8) names the row within its
    MFMA block and the k slot; B[k, n] = 1 + (k % 8) + 8 * (n % 16) names
    the k slot and the column. All values are integers <= 128, exact in
    bf16. kof walks K with a stride coprime to it, so every k of every
    tile is some row's."""
    m, n, k = 256, 128, 192
    mm = torch.arange(m)
    kof = (mm * 37 + 11) % k
    a = torch.zeros(m, k)
    a[mm, kof] = (1 + (mm % 16) + 16 * (kof % 8)).float()
    kk, nn = torch.arange(k)[:, None], torch.arange(n)[None, :]
    b = (1 + (kk % 8) + 8 * (nn % 16)).float()
    return _make(a, b), kof


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_hot_k_gather(ops, layout):
    p, kof = _gather_payload()
    _assert_exact(p)
    assert sorted(set(kof.tolist())) == list(range(192))
    # the reference is that single product
    m = torch.arange(256)
    assert torch.equal(p.ref, p.a.float()[m, kof][:, None] * p.b.float()[kof])
    _check(_run(ops, p, layout), p.ref, f"{layout} k gather")


@functools.lru_cache(maxsize=None)
def _randn_payload():
    m, n, k = 256, 384, 512
    g = _gen("randn", m, n, k)
    a = torch.randn(m, k, generator=g).to(torch.bfloat16)
    b = torch.randn(k, n, generator=g).to(torch.bfloat16)
    ref = torch.matmul(a.double(), b.double())
    # the family's bound: running fp32 sum of K terms
    bound = k * 2.0 ** -23 * torch.matmul(a.double().abs(), b.double().abs())
    return Payload(a, b, ref, ref), bound


@pytest.mark.parametrize("layout", LAYOUTS)
def test_random_operands_within_the_family_bound(ops, layout):
    p, bound = _randn_payload()
    c = _run(ops, p, layout)
    err = (c.cpu().double() - p.ref).abs()
    print(f"layout {layout} randn 256x384x512: worst |err|/bound = "
          f"{float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_random_operands_bit_identical_to_nt_db(ops, monkeypatch, layout):
    """Same k in the same fragment slot as the NT kernels: the MFMAs see
    the same operands in the same order, so the bits are bf16_db8's."""
    from hpc_patterns_amd._native import native

    p, _ = _randn_payload()
    m, k = p.a.shape
    n = p.b.shape[1]
    c = _run(ops, p, layout)
    monkeypatch.setenv("HPK_GEMM_VARIANT", "db")
    assert native().gemm_variant("bf16", m, n, k) == "bf16_db8"
    c_nt = _poison((m, n))
    ops.gemm_bf16(c_nt, p.a.cuda().contiguous(),
                  p.b.cuda().t().contiguous())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(c_nt).any())
    assert torch.equal(c, c_nt)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_deterministic(ops, layout):
    """20 runs, one result: the race screen for the counted vmcnt and the
    raw barriers."""
    p = payload(*RAGGED_GRID)
    a, b = _stored(p, layout)
    first = None
    for i in range(20):
        c = _poison(tuple(p.ref.shape))
        ops.gemm_bf16_layout(c, a, b, layout)
        if first is None:
            first = c
        else:
            assert torch.equal(c, first), f"{layout}: run {i} differs"
    _check(first, p.ref, f"{layout} repeated")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_side_stream(ops, layout):
    p = payload(*ONE_SWAP)
    a, b = _stored(p, layout)
    c = _poison(tuple(p.ref.shape))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())  # the poison fill, copies
    ops.gemm_bf16_layout(c, a, b, layout, stream=side)
    side.synchronize()
    _check(c, p.ref, f"{layout} side stream")


def test_nt_forwards_to_gemm_bf16(ops):
    p = payload(*ONE_SWAP)
    c = _poison((128, 128))
    ops.gemm_bf16_layout(c, p.a.cuda(), p.b.t().contiguous().cuda(), "nt")
    torch.cuda.synchronize()
    _check(c, p.ref, "nt")


@pytest.mark.parametrize("layout", ["nn", "nt", "tn", "tt"])
def test_matmul_ragged_from_views(ops, layout):
    p = payload(100, 130, 70)
    _assert_exact(p)
    a_st, b_st = _stored(p, layout)
    a = a_st.t() if layout[0] == "t" else a_st
    b = b_st.t() if layout[1] == "t" else b_st
    assert a.shape == (100, 70) and b.shape == (70, 130)
    assert ops.matmul_layout(a, b)[0] == layout
    c = ops.matmul(a, b)
    torch.cuda.synchronize()
    assert c.shape == (100, 130) and c.dtype == torch.float32
    _check(c, p.ref, f"matmul {layout}")


def test_error_paths_raise_before_any_launch(ops):
    from hpc_patterns_amd._native import native

    m, n, k = 128, 256, 64
    a = torch.ones(m, k, device="cuda").to(torch.bfloat16)      # nn: [M,K]
    b = torch.ones(k, n, device="cuda").to(torch.bfloat16)      # nn: [K,N]
    c = _poison((m, n))

    with pytest.raises(ValueError):      # bad layout string
        ops.gemm_bf16_layout(c, a, b, "nx")
    with pytest.raises(ValueError):
        ops.gemm_bf16_layout(c, a, b, "NN")
    with pytest.raises(ValueError):      # shapes read in the wrong layout
        ops.gemm_bf16_layout(c, a, b, "tt")
    with pytest.raises(ValueError):      # non-tile M
        ops.gemm_bf16_layout(_poison((64, n)), a[:64], b, "nn")
    with pytest.raises(ValueError):      # non-tile K
        ops.gemm_bf16_layout(c, a[:, :32].contiguous(), b[:32], "nn")
    with pytest.raises(TypeError):       # a non-contiguous, non-transposed view
        ops.gemm_bf16_layout(c, a, torch.ones(k, 2 * n, device="cuda")
                             .to(torch.bfloat16)[:, ::2], "nn")
    with pytest.raises(TypeError):
        ops.matmul(a, torch.ones(k, 2 * n, device="cuda")
                   .to(torch.bfloat16)[:, ::2])
    # a base pointer 2 bytes off a 16-byte boundary
    flat = torch.ones(k * n + 8, device="cuda").to(torch.bfloat16)
    off = flat[1:1 + k * n].view(k, n)
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    with pytest.raises(ValueError):
        ops.gemm_bf16_layout(c, a, off, "nn")
    with pytest.raises(RuntimeError):    # the launcher guards itself
        native().gemm_bf16_layout(c.data_ptr(), a.data_ptr(), off.data_ptr(),
                                  m, n, k, "nn")
    with pytest.raises(RuntimeError):
        native().gemm_bf16_layout(c.data_ptr(), a.data_ptr(), b.data_ptr(),
                                  m, 64, k, "nn")
    with pytest.raises(ValueError):      # nt is not this launcher's
        native().gemm_bf16_layout(c.data_ptr(), a.data_ptr(), b.data_ptr(),
                                  m, n, k, "nt")
    # fp8 / int8 in a non-NT layout
    a8 = torch.zeros(m, k, device="cuda").to(torch.float8_e4m3fn)
    b8 = torch.zeros(k, n, device="cuda").to(torch.float8_e4m3fn)
    with pytest.raises(TypeError, match="transposed"):
        ops.matmul(a8, b8)
    ai = torch.zeros(m, k, dtype=torch.int8, device="cuda")
    bi = torch.zeros(k, n, dtype=torch.int8, device="cuda")
    with pytest.raises(TypeError, match="transposed"):
        ops.matmul(ai.t().contiguous().t(), bi)
    with pytest.raises(TypeError, match="transposed"):
        ops.gemm_bf16_layout(c, ai, bi, "nn")
    torch.cuda.synchronize()
    assert bool(torch.isnan(c).all())


def test_matmul_accepts_a_misaligned_view(ops):
    """the front door clones what the strict call refuses"""
    p = payload(*ONE_SWAP)
    flat = torch.zeros(128 * 128 + 8, dtype=torch.bfloat16, device="cuda")
    off = flat[1:1 + 128 * 128].view(128, 128)
    off.copy_(p.b.cuda())
    assert off.data_ptr() % 16 != 0
    c = ops.matmul(p.a.cuda(), off)
    torch.cuda.synchronize()
    _check(c, p.ref, "matmul misaligned nn")


@pytest.mark.parametrize("shape", [SINGLE_K, (100, 130, 70)],
                         ids=["single_k", "ragged"])
def test_linear_bf16_against_float64_autograd(ops, shape):
    m, n, k = shape
    g = _gen("linear", m, n, k)
    x = torch.randint(-1, 2, (m, k), generator=g).float()
    w = torch.randint(-1, 2, (n, k), generator=g).float()
    dy = torch.randint(-1, 2, (m, n), generator=g).float()

    x64 = x.double().requires_grad_()
    w64 = w.double().requires_grad_()
    y64 = x64 @ w64.t()
    y64.backward(dy.double())
    # every result an integer of magnitude <= 256: exact in bf16
    for t in (y64.detach(), x64.grad, w64.grad):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 256
        assert torch.equal(t.to(torch.bfloat16).double(), t)

    xd = x.to(torch.bfloat16).cuda().requires_grad_()
    wd = w.to(torch.bfloat16).cuda().requires_grad_()
    y = ops.linear_bf16(xd, wd)
    y.backward(dy.to(torch.bfloat16).cuda())
    torch.cuda.synchronize()
    assert y.dtype == xd.grad.dtype == wd.grad.dtype == torch.bfloat16
    _check(y.detach().float(), y64.detach().float(), "linear forward")
    _check(xd.grad.float(), x64.grad.float(), "linear dx")
    _check(wd.grad.float(), w64.grad.float(), "linear dw")

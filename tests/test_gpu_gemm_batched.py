"""Batched, strided bf16 GEMM (native/gemm_batched.hip) on the GPU: bit
identity with the existing kernels, exact payloads against float64, batch
offsets, strides inside NaN-poisoned allocations, the head-interleaved
form, broadcast operands, alpha, specials, determinism, the front door
ops.bmm, autograd (ops.bmm_bf16) and the error paths.

Payloads are built on the CPU in LOGICAL form a [B,M,K], b [B,K,N]
(integers -4..4) and laid out per layout by _stored; _assert_exact checks
the condition under which "bitwise equal" is the right expectation. A bf16
output is compared with the one round-to-nearest-even conversion of the
exact fp32 value (torch's .to(bfloat16) on the CPU)."""

import functools
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

LAYOUTS = ["nt", "nn", "tn", "tt"]
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]
SINGLE_K = (128, 128, 64)        # the prologue is the epilogue
ONE_SWAP = (128, 128, 128)       # one buffer swap
THREE_TRIPS = (128, 128, 192)    # both buffer swaps
RAGGED_GRID = (384, 640, 192)    # 15 workgroups, odd trips, M != N != K
BF = torch.bfloat16

Payload = namedtuple("Payload", "a b ref")


def _gen(*key):
    s = 0
    for part in key:
        for ch in str(part):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator(device="cpu").manual_seed(s)


@functools.lru_cache(maxsize=None)
def payload(batch, m, n, k, tag=""):
    """distinct integer operands per batch; ref is float64"""
    g = _gen("batched", batch, m, n, k, tag)
    a = torch.randint(-4, 5, (batch, m, k), generator=g).float()
    b = torch.randint(-4, 5, (batch, k, n), generator=g).float()
    return Payload(a.to(BF), b.to(BF), torch.bmm(a.double(), b.double()))


@functools.lru_cache(maxsize=None)
def randn_payload(batch, m, n, k):
    g = _gen("batched-randn", batch, m, n, k)
    a = torch.randn(batch, m, k, generator=g).to(BF)
    b = torch.randn(batch, k, n, generator=g).to(BF)
    return Payload(a, b, torch.bmm(a.double(), b.double()))


def _assert_exact(p, alpha=1.0):
    """Integer operands, every partial sum exact in fp32 in any order, the
    wide reference (times alpha, a power of two) survives the cast to fp32."""
    k = p.a.shape[2]
    av, bv = p.a.double(), p.b.double()
    assert torch.equal(av, av.round()) and torch.equal(bv, bv.round())
    assert k * float(av.abs().max()) * float(bv.abs().max()) < 2 ** 24
    assert torch.equal((p.ref * alpha).float().double(), p.ref * alpha)


def _expect(ref64, dtype):
    """float64 -> what the kernel must write: exact in fp32, then at most
    the one rounding of the output type"""
    return ref64.float().to(dtype)


def _stored(p, layout):
    """the operands as layout stores them, on the GPU, contiguous"""
    a = p.a.transpose(1, 2).contiguous() if layout[0] == "t" else p.a
    b = p.b.transpose(1, 2).contiguous() if layout[1] == "t" else p.b
    return a.cuda(), b.cuda()


def _poison(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _check(got, ref, what):
    got = got.cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    if torch.equal(got, ref):
        return
    idx = (got != ref).nonzero()  # NaN poison compares unequal too
    head = [(tuple(int(v) for v in i), got[tuple(i)].item(),
             ref[tuple(i)].item()) for i in idx[:8]]
    pytest.fail(f"{what}: {len(idx)} of {got.numel()} outputs differ; "
                f"first (index, got, ref): {head}")


def _embed(vals, ld_pad, bs_pad, base, fill=float("nan")):
    """vals [B,R,C] as a view with ld = C + ld_pad, bs = R*ld + bs_pad,
    starting `base` elements into a flat allocation filled with `fill`"""
    bsz, rows, cols = vals.shape
    ld = cols + ld_pad
    bs = rows * ld + bs_pad
    flat = torch.full((base + bsz * bs + 8,), fill, dtype=vals.dtype,
                      device="cuda")
    view = flat.as_strided((bsz, rows, cols), (bs, ld, 1), base)
    view.copy_(vals)
    return flat, view


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


def _run(ops, p, layout, dtype, **kw):
    a, b = _stored(p, layout)
    c = _poison(tuple(p.ref.shape), dtype)
    ops.gemm_bf16_batched(c, a, b, layout, **kw)
    torch.cuda.synchronize()
    return c


def _parent_c32(ops, monkeypatch, p, layout):
    """fp32 C of the existing kernels, per batch, on contiguous per-batch
    copies: gemm_bf16_layout, and for nt gemm_bf16's double-buffered 128^2
    kernel"""
    from hpc_patterns_amd._native import native

    bsz, m, k = p.a.shape
    n = p.b.shape[2]
    monkeypatch.setenv("HPK_GEMM_VARIANT", "db")
    assert native().gemm_variant("bf16", m, n, k) == "bf16_db8"
    a, b = _stored(p, layout)
    out = _poison((bsz, m, n))
    for i in range(bsz):
        ops.gemm_bf16_layout(out[i], a[i].contiguous(), b[i].contiguous(),
                             layout)
    torch.cuda.synchronize()
    monkeypatch.delenv("HPK_GEMM_VARIANT")
    assert not bool(torch.isnan(out).any())
    return out


# ---------------------------------------------------------------------------
# 1. bit identity with the existing kernels
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [SINGLE_K, ONE_SWAP, RAGGED_GRID],
                         ids=["single_k", "one_swap", "ragged"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_batch_one_is_the_existing_kernel(ops, monkeypatch, layout, shape):
    p = randn_payload(1, *shape)
    c32 = _parent_c32(ops, monkeypatch, p, layout)
    got = _run(ops, p, layout, torch.float32)
    assert torch.equal(got, c32)
    got16 = _run(ops, p, layout, BF)
    assert torch.equal(got16, c32.to(BF))


# ---------------------------------------------------------------------------
# 2. exact payloads, distinct operands per batch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [SINGLE_K, THREE_TRIPS],
                         ids=["single_k", "three_trips"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_bitwise_batch_three(ops, layout, shape, dtype):
    p = payload(3, *shape)
    _assert_exact(p)
    _check(_run(ops, p, layout, dtype), _expect(p.ref, dtype),
           f"{layout} {shape}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("group", [None, "2"], ids=["rowmajor", "group2"])
@pytest.mark.parametrize("xcd_swizzle", [False, True],
                         ids=["linear", "swizzle"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ragged_grid(ops, monkeypatch, layout, xcd_swizzle, group, dtype):
    if group is not None:
        monkeypatch.setenv("HPK_GEMM_GROUP", group)
    p = payload(2, *RAGGED_GRID)
    _assert_exact(p)
    c = _run(ops, p, layout, dtype, xcd_swizzle=xcd_swizzle)
    _check(c, _expect(p.ref, dtype),
           f"{layout} ragged swizzle={xcd_swizzle} group={group}")


# ---------------------------------------------------------------------------
# 3. an operand that names its batch
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _named_batch_payload(which):
    """A_b = (b+1) * A0 with B fixed (or the other way round): C_b is
    (b+1) * C0, so a wrong batch offset on an operand or on C gives a wrong
    multiple"""
    bsz, m, n, k = 3, 128, 256, 128
    g = _gen("named", which)
    a0 = torch.randint(-4, 5, (m, k), generator=g).float()
    b0 = torch.randint(-4, 5, (k, n), generator=g).float()
    a0 += torch.arange(k).float()[None, :] % 3      # asymmetric
    b0 += torch.arange(n).float()[None, :] % 3
    scale = torch.arange(1, bsz + 1).float()[:, None, None]
    a = a0.expand(bsz, m, k) * (scale if which == "a" else 1.0)
    b = b0.expand(bsz, k, n) * (scale if which == "b" else 1.0)
    c0 = a0.double() @ b0.double()
    assert bool(c0.abs().sum() > 0)
    ref = c0[None] * scale.double()
    return Payload(a.contiguous().to(BF), b.contiguous().to(BF), ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_operand_names_its_batch(ops, layout, which, dtype):
    p = _named_batch_payload(which)
    _assert_exact(p)
    assert torch.equal(p.ref, torch.bmm(p.a.double(), p.b.double()))
    assert not torch.equal(p.ref[0], p.ref[1])
    _check(_run(ops, p, layout, dtype), _expect(p.ref, dtype),
           f"{layout} batch named by {which}")


# ---------------------------------------------------------------------------
# 4. strides with poison
# ---------------------------------------------------------------------------

def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("fill", [float("nan"), -777.0],
                         ids=["nan", "sentinel"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ld_pad", [8, 136])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_strided_slices_of_poisoned_allocations(ops, layout, ld_pad, dtype,
                                                fill):
    p = payload(3, 128, 256, 128, "strided")
    _assert_exact(p)
    a_st, b_st = _stored(p, layout)
    _, a = _embed(a_st, ld_pad, 24, 8)
    _, b = _embed(b_st, ld_pad, 8 * 7, 8)
    assert a.stride(1) == a_st.shape[2] + ld_pad
    assert a.stride(0) > a.shape[1] * a.stride(1)
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    want = _expect(p.ref, dtype)
    c_flat, c = _embed(torch.full(tuple(want.shape), fill, dtype=dtype),
                       ld_pad, 40, 8, fill=fill)
    before = c_flat.clone()
    ops.gemm_bf16_batched(c, a, b, layout)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(c).any())
    _check(c, want, f"{layout} ld+{ld_pad}")
    # every element outside the slices keeps its bits
    c.fill_(0)
    before.as_strided(c.shape, c.stride(), 8).fill_(0)
    assert torch.equal(_bits(c_flat), _bits(before))


# ---------------------------------------------------------------------------
# 5. head-interleaved form
# ---------------------------------------------------------------------------

T, H, D = 256, 3, 128


@functools.lru_cache(maxsize=None)
def _heads():
    g = _gen("heads")
    x = torch.randint(-4, 5, (T, H * D), generator=g).float()
    y = torch.randint(-4, 5, (T, H * D), generator=g).float()
    pm = torch.randint(-4, 5, (H, T, T), generator=g).float()
    return x.to(BF), y.to(BF), pm.to(BF)


@pytest.mark.parametrize("c_form", ["batch_major", "interleaved"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_q_kt_reads_heads_in_place(ops, dtype, c_form):
    x, y, _ = _heads()
    xd, yd = x.cuda(), y.cuda()
    q = xd.view(T, H, D).permute(1, 0, 2)           # [H, T, D]
    kt = yd.view(T, H, D).permute(1, 2, 0)          # [H, D, T]
    layout, q_st, k_st = ops.bmm_layout(q, kt)
    assert layout == "nt"
    assert q_st.stride() == k_st.stride() == (D, H * D, 1)
    ref = torch.bmm(x.view(T, H, D).permute(1, 0, 2).double(),
                    y.view(T, H, D).permute(1, 2, 0).double())
    assert D * 16 < 2 ** 24 and torch.equal(ref.float().double(), ref)
    want = _expect(ref, dtype)
    if c_form == "batch_major":
        c = _poison((H, T, T), dtype)
    else:                                           # storage [T, H, T]
        c = _poison((T, H, T), dtype).permute(1, 0, 2)
        assert c.stride() == (T, H * T, 1)
    ops.gemm_bf16_batched(c, q_st, k_st, "nt")
    torch.cuda.synchronize()
    _check(c, want, f"Q K^T {c_form}")


@pytest.mark.parametrize("c_form", ["batch_major", "interleaved"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_p_v_reads_heads_in_place(ops, dtype, c_form):
    _, y, pm = _heads()
    yd, pd = y.cuda(), pm.cuda()
    v = yd.view(T, H, D).permute(1, 0, 2)           # [H, K=T, N=D]
    layout, p_st, v_st = ops.bmm_layout(pd, v)
    assert layout == "nn" and v_st.stride() == (D, H * D, 1)
    ref = torch.bmm(pm.double(),
                    y.view(T, H, D).permute(1, 0, 2).double())
    assert T * 16 < 2 ** 24 and torch.equal(ref.float().double(), ref)
    want = _expect(ref, dtype)
    if c_form == "batch_major":
        c = _poison((H, T, D), dtype)
    else:                                           # storage [T, H, D]
        store = _poison((T, H, D), dtype)
        c = store.permute(1, 0, 2)
        assert c.stride() == (D, H * D, 1)          # ldc = H*D, bsC = D
    ops.gemm_bf16_batched(c, p_st, v_st, "nn")
    torch.cuda.synchronize()
    _check(c, want, f"P V {c_form}")


def test_bmm_copies_nothing_for_heads(ops, monkeypatch):
    x, y, pm = _heads()
    xd, yd = x.cuda(), y.cuda()
    q = xd.view(T, H, D).permute(1, 0, 2)
    kt = yd.view(T, H, D).permute(1, 2, 0)
    seen = []
    real = ops.gemm_bf16_batched

    def spy(c, a, b, layout, **kw):
        seen.append((layout, a.data_ptr(), a.stride(), b.data_ptr(),
                     b.stride()))
        return real(c, a, b, layout, **kw)

    monkeypatch.setattr(ops, "gemm_bf16_batched", spy)
    _, q_st, k_st = ops.bmm_layout(q, kt)
    assert ops.bmm_direct(q_st, 128, 64) and ops.bmm_direct(k_st, 128, 64)
    s = ops.bmm(q, kt, alpha=0.125)
    torch.cuda.synchronize()
    assert seen == [("nt", xd.data_ptr(), (D, H * D, 1), yd.data_ptr(),
                     (D, H * D, 1))]
    ref = torch.bmm(x.view(T, H, D).permute(1, 0, 2).double(),
                    y.view(T, H, D).permute(1, 2, 0).double()) * 0.125
    assert s.is_contiguous() and s.shape == (H, T, T)
    _check(s, ref.float(), "bmm Q K^T")


# ---------------------------------------------------------------------------
# 6. broadcast
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("which", ["a", "b", "both"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_broadcast_operand(ops, layout, which, dtype):
    p = payload(3, 128, 128, 128, "broadcast")
    a_st, b_st = _stored(p, layout)
    pa, pb = p.a, p.b
    if which in ("a", "both"):
        a_st = a_st[1].expand_as(a_st)
        pa = p.a[1].expand_as(p.a)
    if which in ("b", "both"):
        b_st = b_st[2].expand_as(b_st)
        pb = p.b[2].expand_as(p.b)
    assert (a_st.stride(0) == 0) == (which != "b")
    assert (b_st.stride(0) == 0) == (which != "a")
    c = _poison((3, 128, 128), dtype)
    ops.gemm_bf16_batched(c, a_st, b_st, layout)
    c2 = _poison((3, 128, 128), dtype)
    ops.gemm_bf16_batched(c2, a_st.contiguous(), b_st.contiguous(), layout)
    torch.cuda.synchronize()
    assert torch.equal(c, c2)
    _check(c, _expect(torch.bmm(pa.double(), pb.double()), dtype),
           f"{layout} broadcast {which}")


# ---------------------------------------------------------------------------
# 7. alpha
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("alpha", [0.125, -2.0])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_alpha_power_of_two_is_exact(ops, layout, alpha, dtype):
    p = payload(3, *THREE_TRIPS)
    _assert_exact(p, alpha)
    c = _run(ops, p, layout, dtype, alpha=alpha)
    _check(c, _expect(p.ref * alpha, dtype), f"{layout} alpha={alpha}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_alpha_one_third_is_one_fp32_multiply(ops, monkeypatch, layout):
    """against the fp32 C of the EXISTING kernels: one fp32 multiply, and
    for bf16 one rounding after it"""
    alpha = 1.0 / 3.0
    p = randn_payload(2, 128, 256, 192)
    c32 = _parent_c32(ops, monkeypatch, p, layout).cpu()
    want = c32 * alpha
    assert want.dtype == torch.float32
    assert torch.equal(want, c32 * torch.tensor(alpha, dtype=torch.float32))
    _check(_run(ops, p, layout, torch.float32, alpha=alpha), want,
           f"{layout} alpha=1/3 fp32")
    _check(_run(ops, p, layout, BF, alpha=alpha), want.to(BF),
           f"{layout} alpha=1/3 bf16")


@functools.lru_cache(maxsize=None)
def _tie_payload():
    """acc[m, n] = hi[n] + lo[n] from two products (a has two ones per
    row): 257 and 259 are bf16 ties (8 significant bits: 256, 258, 260),
    to be rounded down and up to even; their negatives; 0 and values that
    need no rounding. Column n carries case n % 6 scaled by 2^(n // 6 - 10)."""
    m, n, k = 128, 128, 64
    cases = [(256.0, 1.0, 256.0), (256.0, 3.0, 260.0),
             (-256.0, -1.0, -256.0), (-256.0, -3.0, -260.0),
             (0.0, 0.0, 0.0), (3.0, 0.75, 3.75)]
    a = torch.zeros(1, m, k)
    rows = torch.arange(m)
    a[0, rows, rows % 32] = 1.0
    a[0, rows, 32 + rows % 32] = 1.0
    b = torch.zeros(1, k, n)
    want = torch.zeros(n, dtype=torch.float64)
    for j in range(n):
        hi, lo, w = cases[j % 6]
        s = 2.0 ** (j // 6 - 10)
        b[0, :32, j], b[0, 32:, j], want[j] = hi * s, lo * s, w * s
    p = Payload(a.to(BF), b.to(BF), torch.bmm(a.double(), b.double()))
    assert torch.equal(p.b.float(), b)          # operands are bf16 values
    return p, want.expand(1, m, n)


@pytest.mark.parametrize("alpha", [1.0, 0.5, -1.0])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_bf16_ties_and_signed_zero(ops, layout, alpha):
    p, want = _tie_payload()
    assert torch.equal(p.ref.float().double(), p.ref)
    # the oracle agrees with the hand-written table, and the table
    # discriminates: truncation gives other numbers
    oracle = (p.ref.float() * alpha).to(BF)
    assert torch.equal(oracle.double(), want * alpha)
    trunc = ((p.ref.float() * alpha).view(torch.int32) & ~0xFFFF) \
        .view(torch.float32)
    assert not torch.equal(trunc.double(), want * alpha)
    c = _run(ops, p, layout, BF, alpha=alpha).cpu()
    _check(c, oracle, f"{layout} ties alpha={alpha}")
    c32 = _run(ops, p, layout, torch.float32, alpha=alpha).cpu()
    _check(c32, p.ref.float() * alpha, f"{layout} ties fp32")
    # a zero accumulator times alpha is an IEEE product: -0.0 for a negative
    # alpha, +0.0 otherwise; nothing short-circuits it
    zero_cols = torch.arange(128) % 6 == 4
    for out in (c, c32):
        z = out[0][:, zero_cols]
        assert bool((z == 0).all())
        assert bool((torch.signbit(z) == (alpha < 0)).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("alpha", [float("inf"), float("nan")],
                         ids=["inf", "nan"])
def test_alpha_not_finite_follows_ieee(ops, alpha, dtype):
    p = payload(2, *SINGLE_K)
    want = (p.ref.float() * alpha).to(dtype)
    if alpha == float("inf"):
        assert bool(torch.isnan(want).any()) and bool(torch.isinf(want).any())
    c = _run(ops, p, "nn", dtype, alpha=alpha).cpu()
    assert torch.equal(torch.isnan(c), torch.isnan(want))
    ok = ~torch.isnan(want)
    assert torch.equal(c[ok], want[ok])


# ---------------------------------------------------------------------------
# 8. randn
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_random_operands(ops, monkeypatch, layout):
    p = randn_payload(2, 128, 256, 512)
    k = 512
    bound = k * 2.0 ** -23 * torch.bmm(p.a.double().abs(), p.b.double().abs())
    c = _run(ops, p, layout, torch.float32)
    err = (c.cpu().double() - p.ref).abs()
    print(f"layout {layout} randn 2x128x256x512: worst |err|/bound = "
          f"{float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())
    assert torch.equal(c, _parent_c32(ops, monkeypatch, p, layout))


# ---------------------------------------------------------------------------
# 9. specials
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_inf_reaches_its_row_of_its_batch_only(ops, layout, dtype):
    clean = payload(3, 128, 128, 128, "specials")
    i0, k0 = 37, 81
    a, b = clean.a.float().clone(), clean.b.float().clone()
    b[1, k0] = torch.where(b[1, k0] == 0, torch.ones(()), b[1, k0])
    a[1, i0, k0] = 0
    expect = torch.bmm(a.double(), b.double()).float()
    expect[1, i0] = torch.sign(b[1, k0]) * float("inf")
    a[1, i0, k0] = float("inf")
    assert int(torch.isinf(expect).sum()) == 128
    p = Payload(a.to(BF), b.to(BF), expect.double())
    _check(_run(ops, p, layout, dtype), expect.to(dtype), f"{layout} Inf")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_bf16_subnormal_operand_is_not_flushed(ops, layout, dtype):
    """2^-133 (a bf16 subnormal) times 2^100 is the normal 2^-33"""
    i0, k0 = 37, 50
    a = torch.zeros(2, 128, 64)
    a[1, i0, k0] = 2.0 ** -133
    b = torch.randint(-4, 5, (2, 64, 128), generator=_gen("sub")).float()
    b[1, k0] = 2.0 ** 100
    a16, b16 = a.to(BF), b.to(BF)
    assert 0 < float(a16[1, i0, k0].double()) == 2.0 ** -133 < 2.0 ** -126
    expect = torch.zeros(2, 128, 128)
    expect[1, i0] = 2.0 ** -33
    assert torch.equal(torch.bmm(a16.double(), b16.double()).float(), expect)
    p = Payload(a16, b16, expect.double())
    _check(_run(ops, p, layout, dtype), expect.to(dtype),
           f"{layout} subnormal")


# ---------------------------------------------------------------------------
# 10. determinism and streams
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_deterministic(ops, layout, dtype):
    p = payload(2, *RAGGED_GRID)
    a, b = _stored(p, layout)
    first = None
    for i in range(10):
        c = _poison(tuple(p.ref.shape), dtype)
        ops.gemm_bf16_batched(c, a, b, layout)
        if first is None:
            first = c
        else:
            assert torch.equal(c, first), f"{layout}: run {i} differs"
    _check(first, _expect(p.ref, dtype), f"{layout} repeated")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_side_stream(ops, layout):
    p = payload(3, *THREE_TRIPS)
    a, b = _stored(p, layout)
    c = _poison(tuple(p.ref.shape))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())  # the poison fill, copies
    ops.gemm_bf16_batched(c, a, b, layout, stream=side)
    side.synchronize()
    _check(c, p.ref.float(), f"{layout} side stream")


# ---------------------------------------------------------------------------
# 11. front door
# ---------------------------------------------------------------------------

def _views(p, layout):
    """logical a [B,M,K], b [B,K,N] as views of what layout stores"""
    a_st, b_st = _stored(p, layout)
    return (a_st.transpose(1, 2) if layout[0] == "t" else a_st,
            b_st.transpose(1, 2) if layout[1] == "t" else b_st)


@pytest.mark.parametrize("out_dtype", [None, BF], ids=DT_IDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_bmm_ragged_from_views(ops, layout, out_dtype):
    p = payload(3, 100, 72, 40)
    _assert_exact(p)
    a, b = _views(p, layout)
    assert a.shape == (3, 100, 40) and b.shape == (3, 40, 72)
    assert ops.bmm_layout(a, b)[0] == layout
    c = ops.bmm(a, b, out_dtype=out_dtype, alpha=0.5)
    torch.cuda.synchronize()
    dtype = torch.float32 if out_dtype is None else BF
    assert c.shape == (3, 100, 72) and c.is_contiguous()
    _check(c, _expect(p.ref * 0.5, dtype), f"bmm {layout}")


@pytest.mark.parametrize("which", ["a", "b"])
def test_bmm_expanded_ragged_operand_is_padded_once(ops, monkeypatch, which):
    p = payload(3, 100, 72, 40)
    a, b = p.a.cuda(), p.b.cuda()
    pa, pb = p.a, p.b
    if which == "a":
        a, pa = a[0].expand(3, 100, 40), p.a[0].expand(3, 100, 40)
    else:
        b, pb = b[0].expand(3, 40, 72), p.b[0].expand(3, 40, 72)
    seen = []
    real = ops.gemm_bf16_batched

    def spy(c, a_, b_, layout, **kw):
        seen.append((a_.stride(0), b_.stride(0)))
        return real(c, a_, b_, layout, **kw)

    monkeypatch.setattr(ops, "gemm_bf16_batched", spy)
    c = ops.bmm(a, b)
    torch.cuda.synchronize()
    assert len(seen) == 1 and (seen[0][0] == 0) == (which == "a") \
        and (seen[0][1] == 0) == (which == "b")
    _check(c, torch.bmm(pa.double(), pb.double()).float(), "bmm expanded")


def test_bmm_runs_more_batches_than_one_grid_in_chunks(ops, monkeypatch):
    p = payload(3, *SINGLE_K)
    monkeypatch.setattr(ops, "GEMM_BATCHED_MAX_BATCH", 2)
    c = ops.bmm(p.a.cuda(), p.b.cuda())
    torch.cuda.synchronize()
    _check(c, p.ref.float(), "bmm in chunks")


def test_bmm_refuses_a_tensor_without_a_unit_stride(ops):
    a = torch.zeros(2, 128, 64, dtype=BF, device="cuda")
    b = torch.zeros(2, 64, 256, dtype=BF, device="cuda")[:, :, ::2]
    with pytest.raises(TypeError, match="no hidden copies"):
        ops.bmm(a, b)


# ---------------------------------------------------------------------------
# 12. autograd
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape,alpha", [((2, 128, 128, 64), 1.0),
                                         ((3, 100, 72, 40), 0.5)],
                         ids=["tiles", "ragged"])
def test_bmm_bf16_against_float64_autograd(ops, shape, alpha):
    """bound = 2^-8 |ref| + K_sum 2^-23 (|.| @ |.|). The first term is the
    one rounding to bf16 of each result (half an ulp of 8 significant bits
    is at most 2^-8 of the value) — dy enters as the bf16 tensor the
    reference gets too, so no second rounding has to fit into it. The
    second term is the family's summation bound, K_sum the summed dimension
    of that product (times |alpha| <= 1: the scaling is exact)."""
    bsz, m, n, k = shape
    g = _gen("autograd", *shape)
    a = torch.randn(bsz, m, k, generator=g).to(BF)
    b = torch.randn(bsz, k, n, generator=g).to(BF)
    dy = torch.randn(bsz, m, n, generator=g).to(BF)
    a64 = a.double().requires_grad_()
    b64 = b.double().requires_grad_()
    y64 = alpha * torch.bmm(a64, b64)
    y64.backward(dy.double())
    aa, ab, ady = a.double().abs(), b.double().abs(), dy.double().abs()
    eps = 2.0 ** -23 * abs(alpha)
    bounds = {
        "y": 2.0 ** -8 * y64.detach().abs() + k * eps * torch.bmm(aa, ab),
        "da": 2.0 ** -8 * a64.grad.abs()
        + n * eps * torch.bmm(ady, ab.transpose(1, 2)),
        "db": 2.0 ** -8 * b64.grad.abs()
        + m * eps * torch.bmm(aa.transpose(1, 2), ady),
    }
    ad = a.cuda().requires_grad_()
    bd = b.cuda().requires_grad_()
    y = ops.bmm_bf16(ad, bd, alpha=alpha)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    assert y.dtype == ad.grad.dtype == bd.grad.dtype == BF
    for name, got, ref in (("y", y.detach(), y64.detach()),
                           ("da", ad.grad, a64.grad),
                           ("db", bd.grad, b64.grad)):
        assert got.shape == ref.shape
        err = (got.cpu().double() - ref).abs()
        print(f"bmm_bf16 {shape} {name}: worst |err|/bound = "
              f"{float((err / bounds[name]).max()):.3e}")
        assert bool((err <= bounds[name]).all()), name


# ---------------------------------------------------------------------------
# 13. error paths
# ---------------------------------------------------------------------------

def test_error_paths_raise_before_any_launch(ops):
    from hpc_patterns_amd._native import native

    bsz, m, n, k = 2, 128, 256, 64
    a = torch.ones(bsz, m, k, device="cuda").to(BF)         # nn: [B,M,K]
    b = torch.ones(bsz, k, n, device="cuda").to(BF)         # nn: [B,K,N]
    c = _poison((bsz, m, n))
    c16 = _poison((bsz, m, n), BF)
    call = ops.gemm_bf16_batched

    with pytest.raises(ValueError):      # bad layout string
        call(c, a, b, "nx")
    with pytest.raises(ValueError):
        call(c, a, b, "NN")
    with pytest.raises(ValueError):      # shapes read in the wrong layout
        call(c, a, b, "tt")
    with pytest.raises(ValueError):      # batch mismatch
        call(c, a[:1], b, "nn")
    with pytest.raises(ValueError):      # non-tile M
        call(_poison((bsz, 64, n)), a[:, :64], b, "nn")
    with pytest.raises(ValueError):      # non-tile N
        call(_poison((bsz, m, 64)), a, b[:, :, :64], "nn")
    with pytest.raises(ValueError):      # non-tile K
        call(c, a[:, :, :32], b[:, :32], "nn")
    with pytest.raises(TypeError):       # rank
        call(c[0], a[0], b[0], "nn")
    with pytest.raises(TypeError):       # last stride not 1
        call(c, a, torch.ones(bsz, k, 2 * n, device="cuda").to(BF)[:, :, ::2],
             "nn")
    with pytest.raises(TypeError):       # dtypes
        call(c, a.float(), b.float(), "nn")
    with pytest.raises(TypeError):
        call(c.double(), a, b, "nn")
    with pytest.raises(TypeError):       # device
        call(c, a.cpu(), b, "nn")
    with pytest.raises(TypeError):       # alpha is a number
        call(c, a, b, "nn", alpha=torch.tensor(1.0))
    # fp8 / int8 operands
    a8 = torch.zeros(bsz, m, k, device="cuda").to(torch.float8_e4m3fn)
    b8 = torch.zeros(bsz, k, n, device="cuda").to(torch.float8_e4m3fn)
    with pytest.raises(TypeError, match="transposed"):
        call(c, a8, b8, "nn")
    with pytest.raises(TypeError, match="transposed"):
        ops.bmm(a8, b8)
    with pytest.raises(TypeError, match="transposed"):
        call(c, a.to(torch.int8), b.to(torch.int8), "nn")

    # a base pointer 2 bytes off a 16-byte boundary
    flat = torch.ones(bsz * k * n + 8, device="cuda").to(BF)
    off = flat[1:1 + bsz * k * n].view(bsz, k, n)
    assert off.data_ptr() % 16 != 0
    with pytest.raises(ValueError, match="16-byte"):
        call(c, a, off, "nn")
    # row stride / batch stride off a multiple of 8, row stride below a row
    wide = torch.ones(bsz, m, k + 4, device="cuda").to(BF)[:, :, :k]
    with pytest.raises(ValueError, match="multiples of 8"):
        call(c, wide, b, "nn")
    flat_a = torch.ones(bsz * (m * k + 4), device="cuda").to(BF)
    with pytest.raises(ValueError, match="multiples of 8"):
        call(c, flat_a.as_strided((bsz, m, k), (m * k + 4, k, 1)), b, "nn")
    with pytest.raises(ValueError, match="below its row"):
        call(c, flat_a.as_strided((bsz, m, k), (m * k, k - 8, 1)), b, "nn")
    # C: rows that overlap, batches that overlap, an expanded C
    flat_c = _poison((bsz * m * n,))
    with pytest.raises(ValueError, match="overlap"):
        call(flat_c.as_strided((bsz, m, n), (m * n, n - 8, 1)), a, b, "nn")
    with pytest.raises(ValueError, match="overlap"):
        call(flat_c.as_strided((bsz, m, n), (m * n - 8, n, 1)), a, b, "nn")
    with pytest.raises(ValueError, match="overlap"):
        call(c[0].expand(bsz, m, n), a, b, "nn")
    with pytest.raises(ValueError, match="overlap"):    # heads 8 too close
        call(flat_c.as_strided((bsz, m, n), (n - 8, 2 * n, 1)), a, b, "nn")
    # bf16 C: base, ldc, bsC on multiples of 8 elements
    flat16 = _poison((bsz * m * (n + 8) + 16,), BF)
    with pytest.raises(ValueError, match="bf16 c"):
        call(flat16.as_strided((bsz, m, n), (m * n, n, 1), 4), a, b, "nn")
    with pytest.raises(ValueError, match="bf16 c"):
        call(flat16.as_strided((bsz, m, n), (m * (n + 4), n + 4, 1)), a, b,
             "nn")
    with pytest.raises(ValueError, match="bf16 c"):
        call(flat16.as_strided((bsz, m, n), (m * n + 4, n, 1)), a, b, "nn")
    # the same fp32 strides are fine for an fp32 C: not judged there
    assert ops.gemm_batched_c_disjoint(bsz, m, n, n + 4, m * (n + 4))

    # batch = 65536: expanded, so no memory is needed
    big = 65536
    with pytest.raises(ValueError, match="batch"):
        call(c[:1].expand(big, m, n), a[:1].expand(big, m, k),
             b[:1].expand(big, k, n), "nn")

    # the launcher guards itself
    lib = native()
    args = dict(m=m, n=n, k=k, batch=bsz, lda=k, bsa=m * k, ldb=n, bsb=k * n,
                ldc=n, bsc=m * n, layout="nn")

    def raw(cc=c, c_is_bf16=0, **kw):
        lib.gemm_bf16_batched(cc.data_ptr(), c_is_bf16, a.data_ptr(),
                              b.data_ptr(), **{**args, **kw})

    with pytest.raises(ValueError):
        raw(layout="nx")
    for kw in (dict(m=64), dict(k=32), dict(batch=0), dict(batch=big),
               dict(lda=k + 4), dict(bsb=k * n + 4), dict(lda=k - 8),
               dict(ldc=n - 8), dict(bsc=0), dict(bsc=m * n - 8),
               dict(bsa=-8)):
        with pytest.raises(RuntimeError):
            raw(**kw)
    with pytest.raises(RuntimeError):
        lib.gemm_bf16_batched(c.data_ptr(), 0, a.data_ptr(),
                              off.data_ptr(), **args)
    with pytest.raises(RuntimeError):
        raw(cc=c16, c_is_bf16=1, ldc=n + 4, bsc=m * (n + 4))
    with pytest.raises(RuntimeError):
        lib.gemm_bf16_batched(c16.data_ptr() + 8, 1, a.data_ptr(),
                              b.data_ptr(), **args)

    torch.cuda.synchronize()
    for t in (c, c16, flat_c, flat16):
        assert bool(torch.isnan(t).all())

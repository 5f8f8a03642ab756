"""CPU guards of the activation epilogues (native/gemm_act.hip): the
reference functions are torch's, the special values are the documented ones,
the acceptance rule of tests/test_gpu_gemm_act.py discriminates and stays
narrow on every payload, the aux tile's way through the staged image is a
bijection without bank conflicts, and the front doors judge the new keywords
before they look at a tensor. No GPU."""

import math

import pytest
import torch
import torch.nn.functional as F

import gemm_act_cases as act
import gemm_epilogue_cases as cases

INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    from hpc_patterns_amd._native import native

    return native()


@pytest.fixture
def ops():
    from hpc_patterns_amd import ops as _ops

    return _ops


# ---------------------------------------------------------------------------
# the reference functions
# ---------------------------------------------------------------------------

def test_references_are_torchs(ops):
    z = torch.linspace(-12.0, 12.0, 4801, dtype=torch.float64)
    for name, fn in (("gelu", lambda t: F.gelu(t, approximate="tanh")),
                     ("relu", F.relu)):
        zz = z.clone().requires_grad_()
        y = fn(zz)
        y.sum().backward()
        got = ops.activation_reference(z, name)
        grad = ops.activation_grad_reference(z, name)
        assert got.dtype == torch.float64 and grad.dtype == torch.float64
        # the tanh and the sigmoid form differ by roundings of float64 only
        assert float((got - y.detach()).abs().max()) < 1e-14
        assert float((grad - zz.grad).abs().max()) < 1e-14
        first, second = ops.activation_grad_terms(z, name)
        assert torch.equal(first + second, grad)
    # a float32 input is widened, not computed in float32
    z32 = torch.randn(1000, generator=cases._gen("act-ref"))
    assert torch.equal(ops.activation_reference(z32, "gelu"),
                       ops.activation_reference(z32.double(), "gelu"))
    with pytest.raises(ValueError, match="erf form is not built"):
        ops.activation_reference(z, "gelu_erf")
    with pytest.raises(ValueError):
        ops.activation_grad_reference(z, "tanh")


def test_gelu_grad_T_is_bounded(ops):
    z = torch.linspace(-8.0, 8.0, 160001, dtype=torch.float64)
    first, second = ops.activation_grad_terms(z, "gelu")
    assert float((first.abs() + second.abs()).max()) <= 1.13


def test_special_values(ops):
    z = torch.tensor([INF, -INF, NAN, 0.0, -0.0, -20.0, -40.0],
                     dtype=torch.float64)
    g = ops.activation_reference(z, "gelu")
    assert g[0] == INF and math.isnan(g[1]) and math.isnan(g[2])
    assert g[3] == 0 and not torch.signbit(g[3])
    assert g[4] == 0 and torch.signbit(g[4])
    assert -1e-100 < float(g[5]) <= 0 and -1e-100 < float(g[6]) <= 0
    r = ops.activation_reference(z, "relu")
    assert r[0] == INF and r[1] == 0 and math.isnan(r[2])
    assert not bool(r[3:].any())
    # torch on the CPU agrees, NaN at -Inf included
    t = F.gelu(z, approximate="tanh")
    assert t[0] == INF and math.isnan(t[1]) and math.isnan(t[2])
    assert t[3] == 0 and t[4] == 0 and abs(float(t[5])) < 1e-100
    # z >= 16: s is 1 in fp32 long before, gelu returns z exactly
    big = torch.tensor([16.0, 100.0, 3e38], dtype=torch.float64)
    assert torch.equal(ops.activation_reference(big, "gelu"), big)


# ---------------------------------------------------------------------------
# the acceptance rule
# ---------------------------------------------------------------------------

def test_rne_bf16_is_one_rounding():
    x = torch.tensor([1.0, 1.00390625, 1.01171875, -1.00390625, 0.0,
                      1.00390625 + 2.0 ** -40, 3e-21, INF, -INF],
                     dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.015625, -1.0, 0.0, 1.0078125,
                         float(torch.tensor(3e-21).to(torch.bfloat16)),
                         INF, -INF], dtype=torch.float64)
    assert torch.equal(act.rne_bf16(x), want)
    # where float32 is exact the two-step cast agrees
    r = torch.randn(100000, generator=cases._gen("rne")).double()
    assert torch.equal(act.rne_bf16(r), r.float().to(torch.bfloat16).double())
    assert math.isnan(float(act.rne_bf16(torch.tensor([NAN]))[0]))


def _bf16_step(x, n):
    """the bf16 value n steps from the bf16 value x (same sign, away from
    0 for n > 0)"""
    bits = x.to(torch.bfloat16).view(torch.int16).int() + n
    return bits.to(torch.int16).view(torch.bfloat16)


def test_rule_accepts_and_rejects(ops):
    p = act.gelu_payload(*act.GELU_SHAPES[1])
    z32 = act.cpu_z32(p)
    ref, delta = act.forward_ref(ops, z32)
    best = act.rne_bf16(ref)
    assert bool(act.accepted(best, ref, delta).all())
    # two bf16 steps away, either side: rejected everywhere
    for n in (2, -2):
        off = _bf16_step(best, n)
        assert not bool(act.accepted(off, ref, delta).any())
    # one step away is rejected where the interval is one value
    lo, hi = act.interval(ref, delta)
    one = act.accepted(_bf16_step(best, 1), ref, delta)
    assert not bool(one[lo == hi].any())
    # ReLU offered as GELU
    relu = ops.activation_reference(z32, "relu").to(torch.bfloat16)
    share = float(act.accepted(relu, ref, delta).double().mean())
    assert share < 0.25, share
    # the erf GELU offered as the tanh one
    erf = F.gelu(z32.double()).to(torch.bfloat16)
    assert not bool(act.accepted(erf, ref, delta).all())
    # gradient mode: the same three
    acc32 = act.cpu_acc32(p)
    gref, gdelta = act.grad_ref(ops, acc32, p.aux)
    gbest = act.rne_bf16(gref)
    assert bool(act.accepted(gbest, gref, gdelta).all())
    # near the zero of gelu' (z = -0.75) the two terms cancel and delta,
    # which follows T, is wide against ref: two steps are judged where it
    # is not
    tight = gdelta <= gref.abs() * 2.0 ** -9
    assert float(tight.double().mean()) > 0.95
    for n in (2, -2):
        assert not bool(act.accepted(_bf16_step(gbest, n), gref,
                                     gdelta)[tight].any())
    mask = (acc32.double() * (p.aux.double() > 0)).to(torch.bfloat16)
    assert float(act.accepted(mask, gref, gdelta).double().mean()) < 0.25
    # a multiply AFTER the rounding of acc is caught
    late = (acc32.to(torch.bfloat16).double()
            * ops.activation_grad_reference(p.aux, "gelu")).to(torch.bfloat16)
    assert not bool(act.accepted(late, gref, gdelta).all())


def test_epsilon_covers_the_derived_bound():
    """docs/gemm.md: first-order bounds in units of 2^-24 for |z| <= 8"""
    u2 = 2 * 0.7978845608028654 * (8 + 0.044715 * 512)
    assert 49.2 < u2 < 49.4
    z = torch.linspace(-8.0, 8.0, 16001, dtype=torch.float64)
    for a_units in (act.EPS_A_FORWARD, act.EPS_A_GRAD):
        e = act.eps(z, a_units)
        assert float(e.max()) == float(e[0]) <= act.EPS_MAX
        assert float(e.min()) < (a_units + 0.01) * 2.0 ** -24  # at z = 0
    assert (act.EPS_A_FORWARD, act.EPS_A_GRAD) == (7.0, 19.0)
    assert act.EPS_MAX == 2.0 ** -16


@pytest.mark.parametrize("shape", act.gelu_payload_shapes(),
                         ids=lambda s: "x".join(map(str, s)))
def test_payloads_stay_in_range_and_intervals_narrow(ops, shape):
    p = act.gelu_payload(*shape)
    z32 = act.cpu_z32(p)
    zmax = float(z32.abs().max())
    assert zmax <= act.Z_MAX, zmax
    assert float(p.aux.float().abs().max()) <= act.Z_MAX
    fwd = act.ambiguous_share(*act.forward_ref(ops, z32))
    grad = act.ambiguous_share(*act.grad_ref(ops, act.cpu_acc32(p), p.aux))
    print(f"{shape}: max |z| {zmax:.2f}, ambiguous forward {fwd:.4%}, "
          f"gradient {grad:.4%}")
    assert fwd <= act.AMBIGUOUS_CAP and grad <= act.AMBIGUOUS_CAP
    # and the payload exercises both signs and the tails
    assert float(z32.min()) < -2.5 and float(z32.max()) > 2.5


@pytest.mark.parametrize("tokens", [act.MLP[0], cases.LINEAR[0]])
def test_mlp_payload_stays_in_range_and_intervals_narrow(ops, tokens):
    x, w1, b1, w2, b2, dy = act.mlp_payload(tokens, *act.MLP[1:])
    z32 = x.float() @ w1.float().t() + b1
    assert float(z32.abs().max()) <= act.Z_MAX
    fwd = act.ambiguous_share(*act.forward_ref(ops, z32))
    acc32 = dy.float() @ w2.float()
    grad = act.ambiguous_share(
        *act.grad_ref(ops, acc32, z32.to(torch.bfloat16)))
    assert fwd <= act.AMBIGUOUS_CAP and grad <= act.AMBIGUOUS_CAP


def test_hash_sign_aux_is_asymmetric():
    aux = act.hash_sign_aux(*cases.RAGGED_GRID[:2]).float()
    pos = aux > 0
    assert 0.3 < float(pos.double().mean()) < 0.7
    assert not torch.equal(pos[:384, :384], pos[:384, :384].t())
    # no two 128x128 tiles share a mask, nor does a tile equal its transpose
    tiles = [pos[i:i + 128, j:j + 128] for i in range(0, 384, 128)
             for j in range(0, 640, 128)]
    for i, t in enumerate(tiles):
        assert not torch.equal(t, t.t())
        for u in tiles[i + 1:]:
            assert not torch.equal(t, u)


# ---------------------------------------------------------------------------
# the aux tile through the staged image. The gradient epilogue adds no offset
# function: it runs gemm_out_read / gemm_out_lds_offset backwards.
# ---------------------------------------------------------------------------

def _lane_rc(wid, lane, m, n, r):
    wr, wc = divmod(wid, 4)
    return (wr * 64 + m * 16 + 4 * (lane >> 4) + r,
            wc * 32 + n * 16 + (lane & 15))


def test_aux_image_fill_is_a_bijection(lib):
    """the 16-byte LDS writes of the fill: every thread's 2 chunks per pass
    hold rows (row, row + 1) x 4 columns, and together they cover the 32 KiB
    image once"""
    chunks = set()
    for p in range(2):
        for t in range(512):
            for i in range(2):
                row, col = lib.gemm_out_read(t, p, i)
                off = lib.gemm_out_lds_offset(row, col)
                assert off % 16 == 0 and 0 <= off < 32768
                assert off not in chunks
                chunks.add(off)
                # the global rows the thread loaded: its 8 columns
                assert col // 8 == t % 16 and row == 2 * (32 * p + t // 16)
    assert len(chunks) == 2048


def test_aux_reads_are_conflict_free_and_find_their_element(lib):
    """ds_read_b32 in the C/D mapping: lane groups {0-31}, {32-63}, bank =
    (addr / 4) % 32; the dword holds rows (row, row + 1) of the lane's
    column, low half first"""
    for wid in range(8):
        for m in range(4):
            for n in range(2):
                for r in (0, 2):
                    offs = [lib.gemm_out_lds_offset(
                        *_lane_rc(wid, lane, m, n, r)) for lane in range(64)]
                    for half in (0, 32):
                        banks = [o // 4 % 32 for o in offs[half:half + 32]]
                        assert len(set(banks)) == 32
                    for lane in (0, 17, 63):
                        row, col = _lane_rc(wid, lane, m, n, r)
                        assert offs[lane] % 4 == 0
                        assert lib.gemm_out_lds_offset(row + 1, col) \
                            == offs[lane] + 2


# ---------------------------------------------------------------------------
# front doors
# ---------------------------------------------------------------------------

class _Untouchable:
    """stands in for a tensor; any look at it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"tensor looked at (.{name}) before the "
                             f"keywords were judged")


BF16 = torch.bfloat16


def test_matmul_judges_activation_keywords_first(ops):
    t = _Untouchable()
    aux = torch.zeros(2, 2, dtype=BF16)
    with pytest.raises(ValueError, match="activation must be one of"):
        ops.matmul(t, t, out_dtype=BF16, activation="silu")
    with pytest.raises(ValueError, match="erf form is not built"):
        ops.matmul(t, t, out_dtype=BF16, activation="gelu_erf")
    with pytest.raises(ValueError, match="need out_dtype"):
        ops.matmul(t, t, activation="relu")
    with pytest.raises(ValueError, match="need out_dtype"):
        ops.matmul(t, t, activation_grad=("relu", aux))
    with pytest.raises(ValueError, match="exclude each other"):
        ops.matmul(t, t, out_dtype=BF16, activation="gelu",
                   activation_grad=("gelu", aux))
    with pytest.raises(ValueError, match="takes no bias"):
        ops.matmul(t, t, out_dtype=BF16, bias=torch.zeros(2),
                   activation_grad=("gelu", aux))
    with pytest.raises(ValueError, match="name"):
        ops.matmul(t, t, out_dtype=BF16, activation_grad=("tanh", aux))
    with pytest.raises(ValueError, match="tuple"):
        ops.matmul(t, t, out_dtype=BF16, activation_grad="gelu")
    with pytest.raises(TypeError, match="aux must be a tensor"):
        ops.matmul(t, t, out_dtype=BF16, activation_grad=("gelu", None))
    with pytest.raises(ValueError, match="return_aux"):
        ops.matmul(t, t, out_dtype=BF16, activation="gelu", return_aux=1)
    with pytest.raises(ValueError, match="return_aux needs"):
        ops.matmul(t, t, out_dtype=BF16, return_aux=True)
    with pytest.raises(ValueError, match="split_k"):
        ops.matmul(t, t, out_dtype=BF16, activation="gelu", split_k="many")


def test_mlp_judges_keywords_first(ops):
    t = _Untouchable()
    with pytest.raises(ValueError, match="activation must be one of"):
        ops.mlp_bf16(t, t, None, t, None, activation="silu")
    with pytest.raises(ValueError, match="split_k"):
        ops.mlp_bf16(t, t, None, t, None, split_k=2)
    with pytest.raises(TypeError, match="b1 must be None or a tensor"):
        ops.mlp_bf16(t, t, 1.0, t, None)


def test_mlp_shape_and_dtype_rules(ops):
    x = torch.zeros(8, 16, dtype=BF16)
    w1 = torch.zeros(32, 16, dtype=BF16)
    w2 = torch.zeros(4, 32, dtype=BF16)
    with pytest.raises(ValueError, match="need x"):
        ops.mlp_bf16(x, w1, None, torch.zeros(4, 16, dtype=BF16), None)
    with pytest.raises(TypeError, match="must be bf16"):
        ops.mlp_bf16(x.float(), w1, None, w2, None)
    with pytest.raises(TypeError, match="contiguous"):
        ops.mlp_bf16(x, torch.zeros(16, 32, dtype=BF16).t(), None, w2, None)
    with pytest.raises(ValueError, match="b1 must have shape"):
        ops.mlp_bf16(x, w1, torch.zeros(4), w2, None)
    with pytest.raises(TypeError, match="b2 must be bfloat16 or float32"):
        ops.mlp_bf16(x, w1, None, w2, torch.zeros(4, dtype=torch.float16))


def test_matmul_aux_rules(ops):
    a = torch.zeros(100, 70, dtype=BF16)
    b = torch.zeros(70, 130, dtype=BF16)
    with pytest.raises(ValueError, match="aux must have shape"):
        ops.matmul(a, b, out_dtype=BF16,
                   activation_grad=("relu", torch.zeros(130, 100, dtype=BF16)))
    with pytest.raises(TypeError, match="contiguous 2-D bfloat16"):
        ops.matmul(a, b, out_dtype=BF16,
                   activation_grad=("relu", torch.zeros(100, 130)))


def test_old_paths_do_not_reach_the_new_entry_point(ops, monkeypatch):
    """matmul without the new keywords and linear_bf16 run what they ran:
    neither gemm_bf16_act nor its native twin"""
    def boom(*a, **k):
        raise AssertionError("new entry point reached")

    reached = []

    class Lib:
        def __getattr__(self, name):
            if name == "gemm_bf16_act" or name.startswith("ACT_"):
                return boom
            if name in ("gemm_bf16_epilogue", "colsum_bf16"):
                return lambda *a, **k: reached.append(name)
            raise RuntimeError(f"native {name}")    # another old path, no GPU

    monkeypatch.setattr(ops, "native", lambda: Lib())
    monkeypatch.setattr(ops, "gemm_bf16_act", boom)
    real_epilogue = ops.gemm_bf16_epilogue
    monkeypatch.setattr(ops, "gemm_bf16_epilogue",
                        lambda c, *a, **k: reached.append("epilogue"))
    monkeypatch.setattr(ops, "colsum_bf16",
                        lambda x, **k: torch.zeros(x.shape[1]))
    a = torch.zeros(128, 64, dtype=BF16)
    b = torch.zeros(64, 128, dtype=BF16)
    for kw in ({}, {"bias": torch.zeros(128)}, {"split_k": 1}):
        out = ops.matmul(a, b, out_dtype=BF16, **kw)
        assert out.dtype == BF16 and out.shape == (128, 128)
    assert reached == ["epilogue"] * 3
    x = torch.zeros(128, 64, dtype=BF16, requires_grad=True)
    w = torch.zeros(128, 64, dtype=BF16, requires_grad=True)
    bias = torch.zeros(128, requires_grad=True)
    ops.linear_bf16(x, w, bias=bias).sum().backward()
    assert x.grad is not None and w.grad is not None and bias.grad is not None
    assert reached == ["epilogue"] * 6
    monkeypatch.setattr(ops, "matmul_nt", lambda x, w, split_k=None:
                        torch.zeros(x.shape[0], w.shape[0]))
    assert ops.linear_bf16(x.detach(), w.detach()).shape == (128, 128)
    # and the new keywords do reach it
    for kw in ({"activation": "relu"},
               {"activation": "gelu", "return_aux": True},
               {"activation_grad": ("gelu", torch.zeros(128, 128,
                                                        dtype=BF16))}):
        with pytest.raises(AssertionError, match="new entry point"):
            ops.matmul(a, b, out_dtype=BF16, **kw)
    with pytest.raises(AssertionError, match="new entry point"):
        ops.mlp_bf16(x.detach(), w.detach(), None,
                     torch.zeros(128, 128, dtype=BF16), None)
    assert real_epilogue is not ops.gemm_bf16_epilogue

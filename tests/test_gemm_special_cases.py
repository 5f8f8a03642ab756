"""CPU guards for tests/gemm_special_cases.py: the reference is what it says,
every payload holds what it claims, and the conditions behind "bit-equal",
"entirely NaN" and the two-outcome class are checked, not assumed."""

import math

import pytest
import torch

import gemm_special_cases as sc

_PAYLOADS = sc.all_payloads()
_IDS = [p.name for p in _PAYLOADS]
_TINY = 2.0 ** -126


def _named(prefix):
    return [p for p in _PAYLOADS if p.name.startswith(prefix)]


def _bits(x):
    return x.view(torch.int16).int() & 0xFFFF


def test_payload_list_is_what_the_gpu_tests_run():
    assert len(sc.NONFINITE_ROWS) == 10 and len(sc.BF16_ROWS) == 5 \
        and len(sc.MX_ROWS) == 7
    assert len(_IDS) == len(set(_IDS))
    for prefix in ("nonfinite[bf16", "nonfinite[fp8", "nonfinite[mxfp8",
                   "overflow_and_underflow", "subnormal_inputs",
                   "extreme_scales[mxfp8", "extreme_scales[mxfp4",
                   "nan_scale[mxfp8", "nan_scale[mxfp4"):
        assert len(_named(prefix)) >= 2, prefix     # both sides at least


@pytest.mark.parametrize("p", _PAYLOADS, ids=_IDS)
def test_reference_matches_a_python_triple_loop(p):
    """8x8x8 corner, plain Python floats (IEEE doubles), classes included."""
    a, b = p.a_deq[:8, :8], p.b_deq[:8, :8]
    got = sc.reference(a, b).to(torch.float32)
    al, bl = a.tolist(), b.tolist()
    for i in range(8):
        for j in range(8):
            acc = 0.0
            for k in range(8):
                acc += al[i][k] * bl[j][k]
            want = torch.tensor(acc, dtype=torch.float64).float().item()
            have = got[i, j].item()
            if math.isnan(want):
                assert math.isnan(have), (i, j)
            else:
                assert have == want, (i, j, have, want)


@pytest.mark.parametrize("p", _PAYLOADS, ids=_IDS)
def test_two_outcome_class_is_capped_and_the_rest_is_normal(p):
    assert float(p.two.double().mean()) <= 0.25
    fin = torch.isfinite(p.wide) & (p.wide != 0) & ~p.two
    mag = p.wide[fin].abs()
    if mag.numel():
        assert float(mag.min()) >= _TINY
    # what is not Inf by design survives the cast to fp32 unchanged
    in_range = torch.isfinite(p.wide) & (p.wide.abs() < 2.0 ** 128)
    assert torch.equal(p.ref.double()[in_range], p.wide[in_range])
    over = torch.isfinite(p.wide) & ~in_range
    assert bool(torch.isinf(p.ref[over]).all())
    if not p.name.startswith("overflow"):
        assert not bool(over.any())


@pytest.mark.parametrize("p", _PAYLOADS, ids=_IDS)
def test_containment_lines(p):
    """Outside the planted rows / columns the reference is the clean one
    bit for bit; inside them it is what the design says."""
    if p.clean_ref is None:
        return
    m, n = p.ref.shape
    clean = torch.ones(m, n, dtype=torch.bool)
    clean[list(p.rows), :] = False
    clean[:, list(p.cols)] = False
    assert torch.equal(p.ref[clean], p.clean_ref[clean])
    assert bool(torch.isfinite(p.clean_ref).all())
    assert not bool(torch.isfinite(p.ref[~clean]).any())
    if not p.name.startswith("nonfinite[bf16"):
        assert bool(torch.isnan(p.ref[~clean]).all())   # entirely NaN


@pytest.mark.parametrize("p", _named("nonfinite"),
                         ids=[p.name for p in _named("nonfinite")])
def test_nonfinite_holds_the_planted_codes(p):
    x = p.a if p.rows else p.b
    other = p.b_deq if p.rows else p.a_deq
    lines = p.rows or p.cols
    if p.kind == "bf16":
        bits = _bits(x)
        for ln, want in zip(lines, ({0x7F80}, {0x7F80, 0xFF80}, None)):
            special = bits[ln][(bits[ln] & 0x7F80) == 0x7F80].tolist()
            if want is None:
                assert len(special) == 1 and special[0] & 0x7F     # a NaN
            else:
                assert set(special) == want and len(special) == len(want)
        out = p.ref[lines[0], :] if p.rows else p.ref[:, lines[0]]
        k_inf = int((bits[lines[0]] == 0x7F80).nonzero()[0])
        zero = other[:, k_inf] == 0
        assert bool(zero.any()) and bool((~zero).any())
        assert bool(torch.isnan(out[zero]).all())
        assert bool(torch.isinf(out[~zero]).all())
        assert bool((out == float("inf")).any()) \
            and bool((out == -float("inf")).any())
        both = p.ref[lines[1], :] if p.rows else p.ref[:, lines[1]]
        assert bool(torch.isnan(both).any())
        last = p.ref[lines[2], :] if p.rows else p.ref[:, lines[2]]
        assert bool(torch.isnan(last).all())
    else:
        raw = x.view(torch.uint8)
        got = [sorted(set(raw[ln].tolist()) & {0x7F, 0xFF}) for ln in lines]
        assert got == [[0x7F], [0xFF], [0x7F]]
    rest = torch.ones(x.shape[0], dtype=torch.bool)
    rest[list(lines)] = False
    assert bool(torch.isfinite(p.a_deq[rest] if p.rows
                               else p.b_deq[rest]).all())


@pytest.mark.parametrize("p", _named("overflow"),
                         ids=[p.name for p in _named("overflow")])
def test_overflow_payload_reaches_both_ends(p):
    side_a = "[a," in p.name
    fields = (_bits(p.a if side_a else p.b) >> 7) & 0xFF
    assert int(fields.min()) == 1 and int(fields.max()) == 254
    assert bool((p.ref == float("inf")).any())
    assert bool((p.ref == -float("inf")).any())
    assert not bool(torch.isnan(p.ref).any())
    sub = (p.wide != 0) & (p.wide.abs() < _TINY)
    assert int(sub.sum()) >= 16 and torch.equal(sub, p.two)
    terms = (p.a_deq != 0).double() @ (p.b_deq != 0).double().t()
    assert float(terms.max()) <= 1


@pytest.mark.parametrize("p", _named("subnormal"),
                         ids=[p.name for p in _named("subnormal")])
def test_subnormal_payload_holds_subnormals_of_both_signs(p):
    side_a = "[a," in p.name
    bits = _bits(p.a if side_a else p.b)
    sub = ((bits >> 7) & 0xFF) == 0
    assert bool(((bits & 0x7F)[sub] >= 1).all())        # none is a zero
    assert int((sub & (bits < 0x8000)).sum()) >= 100
    assert int((sub & (bits >= 0x8000)).sum()) >= 100
    assert float(sub.double().mean()) == 0.25
    assert float(p.two.double().mean()) == 0.25
    assert bool(torch.isfinite(p.wide).all())
    # every product, the subnormals' too, is a normal fp32
    assert float(p.wide.abs().min()) >= _TINY
    terms = (p.a_deq != 0).double() @ (p.b_deq != 0).double().t()
    assert float(terms.max()) == 1 and float(terms.min()) == 1
    # the subnormals meet all four weights
    hot = p.b_deq if side_a else p.a_deq
    two = p.two if side_a else p.two.t()        # [full row, hot row]
    weights = hot[hot != 0].unique().tolist()
    assert len(weights) == 4
    assert all(2.0 ** 20 <= abs(w) <= 2.0 ** 24 for w in weights)
    for w in weights:
        assert bool(two[:, (hot == w).any(1)].any()), w


@pytest.mark.parametrize("p", _named("extreme"),
                         ids=[p.name for p in _named("extreme")])
def test_extreme_scales_payload(p):
    side_a = p.rows != ()
    s_full, s_hot = (p.sa, p.sb) if side_a else (p.sb, p.sa)
    assert set(s_full.flatten().tolist()) == {0, 1, 2, 252, 253, 254}
    assert set(s_hot.flatten().tolist()) == {0, 1, 2, 252, 253, 254}
    assert set(s_full[:, 0::2].flatten().tolist()) == {0, 1, 2}
    assert set(s_full[:, 1::2].flatten().tolist()) == {252, 253, 254}
    # sa + sb - 254 within [-3, 3] wherever two blocks meet
    total = s_full.int()[:, None, :] + s_hot.int()[None, :, :] - 254
    assert int(total.min()) >= -3 and int(total.max()) <= 3
    assert bool(torch.isfinite(p.wide).all()) and not bool(p.two.any())
    terms = (p.a_deq != 0).double() @ (p.b_deq != 0).double().t()
    assert float(terms.max()) <= 1
    # the all-zero blocks, opposite non-zero data, under scales 0 and 254
    full, hot = (p.a_deq, p.b_deq) if side_a else (p.b_deq, p.a_deq)
    for ln, blk, s in ((3, 0, 0), (9, 1, 254)):
        assert int(s_full[ln, blk]) == s
        assert bool((full[ln, 32 * blk:32 * blk + 32] == 0).all())
        facing = (hot[:, 32 * blk:32 * blk + 32] != 0).any(1)
        assert int(facing.sum()) >= 32
        out = p.ref[ln, :] if side_a else p.ref[:, ln]
        assert bool((out[facing] == 0).all())
    # ... and the operand itself leaves fp32: 2^127 * 448 or * 6
    assert float(full.abs().max()) >= 2.0 ** 129


@pytest.mark.parametrize("p", _named("nan_scale"),
                         ids=[p.name for p in _named("nan_scale")])
def test_nan_scale_payload(p):
    s = p.sa if p.rows else p.sb
    lines = p.rows or p.cols
    assert int((s == 255).sum()) == 2
    assert int(s[lines[0], 0]) == 255 and int(s[lines[1], -1]) == 255
    other = p.sb if p.rows else p.sa
    assert int(other.max()) < 255


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("side", sc.SIDES)
def test_splitk_specials_sit_in_split_2_only(kind, side):
    p = sc.splitk_payload(kind, side)
    x = p.a_deq if side == "a" else p.b_deq
    k_bad = (~torch.isfinite(x)).any(0).nonzero().flatten().tolist()
    assert k_bad == list(sc.SPLITK_KS)
    assert all(128 <= k < 192 for k in k_bad)
    other = p.b_deq if side == "a" else p.a_deq
    assert bool(torch.isfinite(other).all())

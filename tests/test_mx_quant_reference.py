"""ops.quantize_mx_reference / ops.dequantize_mx: the pure-torch oracle of
the MX quantize kernel, pinned against the written contract (docs/gemm.md,
"MX quantize") on the CPU. tests/test_gpu_mx_quant.py then holds the
kernel to this oracle bit for bit."""

import pytest
import torch

import mx_quant_cases as cases
from hpc_patterns_amd import ops

FMTS = ("mxfp8", "mxfp4")


def _edge(fmt, name, dtype=torch.float32):
    names, blocks = cases.edge_blocks()
    x = blocks[names.index(name)].view(1, 32).to(dtype)
    q, s = ops.quantize_mx_reference(x, fmt)
    return cases.codes(q, fmt)[0].tolist(), int(s[0, 0])


def test_e2m1_tie_table():
    """Ties go to the code with the even index; 5.0 pins the scale at 127."""
    x = torch.zeros(1, 32)
    x[0, : len(cases.E2M1_TIES)] = torch.tensor([v for v, _ in cases.E2M1_TIES])
    q, s = ops.quantize_mx_reference(x, "mxfp4")
    assert s.tolist() == [[127]]
    nib = cases.unpack_nibbles(q)[0].tolist()
    assert nib[: len(cases.E2M1_TIES)] == [n for _, n in cases.E2M1_TIES]
    assert nib[len(cases.E2M1_TIES):] == [0] * (32 - len(cases.E2M1_TIES))


def test_e4m3_ties_round_to_even_mantissa():
    """Midpoints between adjacent e4m3 values at scale 127 (448 pins it):
    17 is halfway 16|18 -> 16 (0x58); 19 -> 20 (0x5A); the subnormal
    midpoints 2^-10 (0|2^-9) -> 0 and 3*2^-10 (2^-9|2^-8) -> 2^-8."""
    x = torch.zeros(1, 32)
    x[0, :5] = torch.tensor([448.0, 17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10])
    q, s = ops.quantize_mx_reference(x, "mxfp8")
    assert s.tolist() == [[127]]
    assert q.view(torch.uint8)[0, :5].tolist() == [0x7E, 0x58, 0x5A, 0x00, 0x02]


@pytest.mark.parametrize("fmt,scale_range", [("mxfp8", (118, 124)),
                                             ("mxfp4", (123, 129))])
def test_lossless_roundtrip(fmt, scale_range):
    v = cases.lossless(fmt, 128, 128)
    q, s = ops.quantize_mx_reference(v, fmt)
    assert q.shape == ((128, 128) if fmt == "mxfp8" else (128, 64))
    assert s.shape == (128, 4) and s.dtype == torch.uint8
    assert torch.equal(ops.dequantize_mx(q, s, fmt), v.double())
    live = s[v.view(128, 4, 32).abs().amax(-1) > 0]
    assert scale_range[0] <= int(live.min()) and int(live.max()) <= scale_range[1]


@pytest.mark.parametrize("fmt", FMTS)
def test_zero_blocks(fmt):
    assert _edge(fmt, "all_zero") == ([0] * 32, 0)
    neg = 0x80 if fmt == "mxfp8" else 8
    code, s = _edge(fmt, "neg_zero")
    assert (code[:3], set(code[3:]), s) == ([neg, 0, neg], {0}, 0)


@pytest.mark.parametrize("fmt", FMTS)
def test_subnormal_inputs_become_signed_zero(fmt):
    neg = 0x80 if fmt == "mxfp8" else 8
    code, s = _edge(fmt, "subnormal_only")
    assert (code[:4], set(code[4:]), s) == ([0, neg, 0, neg], {0}, 0)
    code, s = _edge(fmt, "subnormal_beside_normal")
    # 1.0 has exponent field 127: scale 119 / 125, 1.0 -> 2^8 / 2^2
    assert s == (119 if fmt == "mxfp8" else 125)
    assert code[:3] == ([0x78, 0, 0x80] if fmt == "mxfp8" else [6, 0, 8])


def test_saturates_instead_of_nan():
    """amax 1.9: scale 119, 1.9 * 2^8 = 486.4 > 448 saturates to 0x7E
    (0x7F would be NaN); in e2m1 1.9 * 4 = 7.6 saturates to 6."""
    code, s = _edge("mxfp8", "saturate_1p9")
    assert (code[:3], s) == ([0x7E, 0xFE, 0x78], 119)
    code, s = _edge("mxfp4", "saturate_1p9")
    assert (code[:3], s) == ([7, 15, 6], 125)


@pytest.mark.parametrize("fmt,emax,top", [("mxfp8", 8, 0x7E), ("mxfp4", 2, 7)])
def test_flt_max(fmt, emax, top):
    code, s = _edge(fmt, "flt_max")
    assert s == 254 - emax
    assert code[:2] == [top, top | (0x80 if fmt == "mxfp8" else 8)]
    assert code[2] == 0                       # 1.0 * 2^(127 - s) underflows
    # 2^120 * 2^(127 - s) = 2^(emax - 7)
    assert code[3] == (0x40 if fmt == "mxfp8" else 0)


@pytest.mark.parametrize("fmt", FMTS)
def test_small_amax_clamps_scale_to_zero(fmt):
    """Exponent field 2 <= emax: scale 0, elements times 2^127 = 4, -2, 3."""
    code, s = _edge(fmt, "scale_clamps_to_0")
    assert s == 0
    assert code[:3] == ([0x48, 0xC0, 0x44] if fmt == "mxfp8" else [6, 12, 5])


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["one_inf", "one_neg_inf", "one_nan"])
def test_non_finite_block_scale_is_nan(fmt, name):
    assert _edge(fmt, name)[1] == 255


@pytest.mark.parametrize("fmt", FMTS)
def test_bf16_input_equals_same_values_in_fp32(fmt):
    x = torch.cat([cases.wide_randn(8, 256), cases.edge_blocks()[1].view(1, -1)
                   .expand(8, -1)[:, :256]], dim=1).bfloat16()
    q16, s16 = ops.quantize_mx_reference(x, fmt)
    q32, s32 = ops.quantize_mx_reference(x.float(), fmt)
    assert torch.equal(s16, s32)
    assert torch.equal(q16.view(torch.uint8), q32.view(torch.uint8))


def test_dequantize_nan_scale_and_shapes():
    q = torch.zeros(2, 32, dtype=torch.uint8).view(torch.float8_e4m3fn)
    s = torch.tensor([[127], [255]], dtype=torch.uint8)
    d = ops.dequantize_mx(q, s, "mxfp8")
    assert d.dtype == torch.float64 and d.shape == (2, 32)
    assert bool((d[0] == 0).all()) and bool(d[1].isnan().all())
    with pytest.raises(ValueError):
        ops.dequantize_mx(q, s[:, :0], "mxfp8")


def test_reference_rejects_bad_arguments():
    with pytest.raises(ValueError):
        ops.quantize_mx_reference(torch.zeros(2, 48), "mxfp8")
    with pytest.raises(ValueError):
        ops.quantize_mx_reference(torch.zeros(2, 32), "mxfp6")
    with pytest.raises(TypeError):
        ops.quantize_mx_reference(torch.zeros(2, 32, dtype=torch.float16),
                                  "mxfp8")

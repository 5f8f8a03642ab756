"""Payloads and reference for the GEMM family on special values: NaN, Inf,
bf16 subnormals, fp32 overflow/underflow of the product, e8m0 scales
0/1/2/252/253/254 and the e8m0 NaN 255. Shared by
tests/test_gemm_special_cases.py (CPU guards) and
tests/test_gpu_gemm_specials.py (GPU). Everything here is CPU-only.

Reference: a float64 sum of ELEMENTWISE products of the dequantised
operands, cast to fp32. Not a BLAS matmul: a BLAS may skip zeros and so
lose 0 * Inf = NaN. Every payload has at most one class of non-finite term
per output, or only small finite terms, so the class of each output (exact
finite value, +Inf, -Inf, NaN) does not depend on the summation order.

Two-outcome class: hardware may flush subnormals. An output is in the class
when (a) its exact fp32 value is subnormal or (b) its only non-zero term has
a bf16-subnormal input. There, and only there, a zero of the exact value's
sign is accepted beside the exact value. That is a condition computed from
the payload, never from a result; every builder asserts that the class holds
at most 1/4 of its outputs.

int8 has no special values; its extremes are in tests/test_gpu_gemm_matrix.py.
"""

import functools
from collections import namedtuple

import torch

from test_gpu_gemm_matrix import (ROWS, _MX, _SCALES_SINGLE, _dequant,
                                  _full_range_operand, _gen,
                                  _one_hot_operand, sum_payload)

Special = namedtuple(
    "Special", "name kind a b sa sb a_deq b_deq wide ref two clean_ref "
               "rows cols")
# rows / cols: the output rows / columns that carry a planted special;
# clean_ref: the fp32 reference of the payload before planting (or None).

NONFINITE_ROWS = [r for r in ROWS if r.kind in ("bf16", "fp8", "mxfp8")]
BF16_ROWS = [r for r in ROWS if r.kind == "bf16"]
MX_ROWS = [r for r in ROWS if r.kind in _MX]
SIDES = ("a", "b")

SENTINEL = 12345.0          # C prefill: finite, NaN is a legitimate answer
_TINY = 2.0 ** -126         # smallest normal fp32 (and bf16)
_INF, _NAN = float("inf"), float("nan")
_SCALES_LOW, _SCALES_HIGH = (0, 1, 2), (252, 253, 254)


# ---------------------------------------------------------------------------
# reference and comparison
# ---------------------------------------------------------------------------

def dequant(kind, x, scale):
    """float64 value of an operand; a block under scale byte 255 is NaN."""
    v = _dequant(kind, x, scale)
    if scale is not None:
        nan_block = (scale == 255).repeat_interleave(32, dim=1)
        v = torch.where(nan_block, torch.full_like(v, _NAN), v)
    return v


def reference(a_deq, b_deq, chunk=16):
    """float64 [M,N]: sum over k of a[i,k] * b[j,k], elementwise products."""
    m, n = a_deq.shape[0], b_deq.shape[0]
    out = torch.empty(m, n, dtype=torch.float64)
    for i in range(0, m, chunk):
        out[i:i + chunk] = (a_deq[i:i + chunk, None, :]
                            * b_deq[None, :, :]).sum(-1)
    return out


def _bf16_subnormal(deq):
    return (deq != 0) & (deq.abs() < _TINY)


def two_outcome_mask(kind, a_deq, b_deq, wide):
    mask = (wide != 0) & (wide.abs() < _TINY)               # (a)
    if kind == "bf16":                                      # (b)
        anz, bnz = (a_deq != 0).double(), (b_deq != 0).double()
        terms = anz @ bnz.t()           # 0/1 masks: any matmul is exact
        asub = _bf16_subnormal(a_deq).double()
        bsub = _bf16_subnormal(b_deq).double()
        sub_terms = asub @ bnz.t() + anz @ bsub.t()
        mask = mask | ((terms == 1) & (sub_terms >= 1))
    return mask


def _finish(name, kind, a, b, sa, sb, clean_ref=None, rows=(), cols=()):
    a_deq, b_deq = dequant(kind, a, sa), dequant(kind, b, sb)
    wide = reference(a_deq, b_deq)
    two = two_outcome_mask(kind, a_deq, b_deq, wide)
    assert float(two.double().mean()) <= 0.25, name
    return Special(name, kind, a, b, sa, sb, a_deq, b_deq, wide,
                   wide.to(torch.float32), two, clean_ref,
                   tuple(rows), tuple(cols))


def mismatch_mask(got, p):
    """True where got is not an accepted result for p."""
    ref = p.ref
    got_nan, ref_nan = torch.isnan(got), torch.isnan(ref)
    exact = got == ref                  # +-Inf compare equal to themselves
    flushed = p.two & (got == 0) \
        & (torch.signbit(got) == torch.signbit(ref))
    return (got_nan != ref_nan) | (~ref_nan & ~exact & ~flushed)


def outcome_counts(got, p):
    """(exact, flushed) counts within the two-outcome class."""
    exact = int(((got == p.ref) & p.two).sum())
    flushed = int(((got == 0) & (p.ref != 0) & p.two).sum())
    return exact, flushed


def describe_mismatches(got, p, limit=8):
    bad = mismatch_mask(got, p).nonzero()
    head = []
    for i, j in bad[:limit]:
        t = torch.nan_to_num((p.a_deq[i] * p.b_deq[j]).abs(),
                             nan=_INF, posinf=_INF)
        kk = int(t.argmax())
        head.append((int(i), int(j), got[i, j].item(), p.ref[i, j].item(),
                     f"a[{kk}]={p.a_deq[i, kk].item()!r}",
                     f"b[{kk}]={p.b_deq[j, kk].item()!r}"))
    return len(bad), head


# ---------------------------------------------------------------------------
# payloads
# ---------------------------------------------------------------------------

def _bf16_bits(sign, exp, man):
    bits = (sign << 15) | (exp << 7) | man
    bits = torch.where(bits >= 32768, bits - 65536, bits)
    return bits.to(torch.int16).view(torch.bfloat16)


def _plant(kind, x, r, k, what):
    """what: a float for bf16, an e4m3 byte for fp8 / mxfp8."""
    if kind == "bf16":
        x[r, k] = what
    else:
        x.view(torch.uint8)[r, k] = what


@functools.lru_cache(maxsize=None)
def nonfinite(kind, side, m, n, k, ks=None):
    """sum_payload integers with specials in one operand: at rows
    {0, 37, m-1} of A, or at columns {5, 37, n-2} of the result through B
    (three lines, so that each of the three bf16 specials has its own), at
    k in ks = (0, 31, k-1) unless given. bf16: +Inf / -Inf and +Inf at
    different k / NaN; fp8, mxfp8: byte 0x7F / 0xFF / 0x7F."""
    clean = sum_payload(kind, m, n, k, _SCALES_SINGLE)
    k0, k1, k2 = ks or (0, 31, k - 1)
    a, b = clean.a.clone(), clean.b.clone()
    x, lines = (a, (0, 37, m - 1)) if side == "a" else (b, (5, 37, n - 2))
    if kind == "bf16":
        _plant(kind, x, lines[0], k0, _INF)
        _plant(kind, x, lines[1], k1, -_INF)
        _plant(kind, x, lines[1], k2, _INF)
        _plant(kind, x, lines[2], k2, _NAN)
    else:
        _plant(kind, x, lines[0], k0, 0x7F)
        _plant(kind, x, lines[1], k1, 0xFF)
        _plant(kind, x, lines[2], k2, 0x7F)
    rows, cols = (lines, ()) if side == "a" else ((), lines)
    return _finish(f"nonfinite[{kind},{side},{m}x{n}x{k}]", kind, a, b,
                   clean.sa, clean.sb, clean.ref, rows, cols)


def _gather_operands(kind, side, m, n, k, full, hot):
    return (full, hot) if side == "a" else (hot, full)


@functools.lru_cache(maxsize=None)
def overflow_and_underflow(kind, side, m, n, k):
    """k_gather with the full-side exponent field widened to 1..254: field
    254 times weight 2 is +-Inf, field 1 times weight 0.5 an fp32-subnormal
    product. Both meetings are planted (every fourth row each), not left to
    the seed."""
    assert kind == "bf16"
    g = _gen("overflow", kind, m, n, k, side)
    rows_full, rows_hot = (m, n) if side == "a" else (n, m)
    hot = _one_hot_operand(kind, rows_hot, k)
    k_two = (hot.float() == 2).any(0).nonzero().flatten()
    k_half = (hot.float() == 0.5).any(0).nonzero().flatten()
    cnt = rows_full * k
    sign = torch.randint(0, 2, (cnt,), generator=g).view(rows_full, k)
    exp = torch.randint(1, 255, (cnt,), generator=g).view(rows_full, k)
    man = torch.randint(0, 128, (cnt,), generator=g).view(rows_full, k)
    for r in range(0, rows_full, 4):
        exp[r, k_two[(r // 4) % len(k_two)]] = 254
        exp[r + 1, k_half[(r // 4) % len(k_half)]] = 1
    full = _bf16_bits(sign, exp, man)
    a, b = _gather_operands(kind, side, m, n, k, full, hot)
    return _finish(f"overflow_and_underflow[{side},{m}x{n}x{k}]", kind,
                   a, b, None, None)


def _one_hot_pow2(rows, k):
    """_one_hot_operand's positions with weights 2^20, -2^21, 2^23, 2^24."""
    w = torch.tensor([2.0 ** 20, -(2.0 ** 21), 2.0 ** 23, 2.0 ** 24])
    h = torch.zeros(rows, k)
    i = torch.arange(rows)
    h[i, (5 * i + 3) % k] = w[i % 4]
    return h.to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def subnormal_inputs(kind, side, m, n, k):
    """k_gather whose full-side operand holds a bf16 subnormal (field 0,
    mantissa 1..127, both signs) wherever (row + k) % 4 == 0, so that the
    subnormals meet all four weights. The weights are 2^20..2^24: the exact
    product of a subnormal (>= 2^-133) is a NORMAL fp32. The other three
    quarters are normal patterns of field 2..229 (253 - 24: the largest
    weight must not overflow them)."""
    assert kind == "bf16"
    g = _gen("subnormal", kind, m, n, k, side)
    rows_full, rows_hot = (m, n) if side == "a" else (n, m)
    cnt = rows_full * k
    sign = torch.randint(0, 2, (cnt,), generator=g).view(rows_full, k)
    exp = torch.randint(2, 230, (cnt,), generator=g).view(rows_full, k)
    man = torch.randint(0, 128, (cnt,), generator=g).view(rows_full, k)
    sub_man = torch.randint(1, 128, (cnt,), generator=g).view(rows_full, k)
    r = torch.arange(rows_full)[:, None]
    c = torch.arange(k)[None, :]
    is_sub = (r + c) % 4 == 0
    exp = torch.where(is_sub, torch.zeros_like(exp), exp)
    man = torch.where(is_sub, sub_man, man)
    full = _bf16_bits(sign, exp, man)
    hot = _one_hot_pow2(rows_hot, k)
    a, b = _gather_operands(kind, side, m, n, k, full, hot)
    return _finish(f"subnormal_inputs[{side},{m}x{n}x{k}]", kind,
                   a, b, None, None)


def _pick(values, shape, g):
    t = torch.tensor(values, dtype=torch.uint8)
    return t[torch.randint(0, len(values), shape, generator=g)]


@functools.lru_cache(maxsize=None)
def extreme_scales(kind, side, m, n, k):
    """k_gather with the full-format element operand. Its scales come from
    {0,1,2} on even K-blocks and {252,253,254} on odd ones; the one-hot
    operand's come from the opposite set, so sa + sb - 254 lies in [-2, 2]
    and every product is a normal fp32 (2^-127 is a float64 normal: the
    reference is exact). Row 3 of the full operand has an all-zero block 0
    under scale 0, row 9 an all-zero block 1 under scale 254, each opposite
    non-zero data: exact zeros, not NaN."""
    assert kind in _MX
    g = _gen("extreme", kind, m, n, k, side)
    rows_full, rows_hot = (m, n) if side == "a" else (n, m)
    full = _full_range_operand(kind, rows_full, k, g).clone()
    hot = _one_hot_operand(kind, rows_hot, k)
    nb = k // 32
    even = (torch.arange(nb) % 2 == 0)[None, :]
    s_full = torch.where(even, _pick(_SCALES_LOW, (rows_full, nb), g),
                         _pick(_SCALES_HIGH, (rows_full, nb), g))
    s_hot = torch.where(even, _pick(_SCALES_HIGH, (rows_hot, nb), g),
                        _pick(_SCALES_LOW, (rows_hot, nb), g))
    per_block = 32 if kind == "mxfp8" else 16       # bytes of one block
    raw = full.view(torch.uint8)
    raw[3, 0:per_block] = 0
    s_full[3, 0] = 0
    raw[9, per_block:2 * per_block] = 0
    s_full[9, 1] = 254
    a, b = _gather_operands(kind, side, m, n, k, full, hot)
    sa, sb = (s_full, s_hot) if side == "a" else (s_hot, s_full)
    lines = (3, 9)
    rows, cols = (lines, ()) if side == "a" else ((), lines)
    return _finish(f"extreme_scales[{kind},{side},{m}x{n}x{k}]", kind,
                   a, b, sa, sb, None, rows, cols)


@functools.lru_cache(maxsize=None)
def nan_scale(kind, side, m, n, k):
    """sum_payload data; scale byte 255 (e8m0 NaN) on block 0 of one row
    and on the last block of another (columns through B). Per OCP MX v1.0
    the block is all NaN, so those rows / columns are entirely NaN."""
    assert kind in _MX
    clean = sum_payload(kind, m, n, k, _SCALES_SINGLE)
    sa, sb = clean.sa.clone(), clean.sb.clone()
    s, lines = (sa, (37, m - 1)) if side == "a" else (sb, (5, n - 2))
    s[lines[0], 0] = 255
    s[lines[1], k // 32 - 1] = 255
    rows, cols = (lines, ()) if side == "a" else ((), lines)
    return _finish(f"nan_scale[{kind},{side},{m}x{n}x{k}]", kind,
                   clean.a, clean.b, sa, sb, clean.ref, rows, cols)


LAYOUT_SHAPE = (128, 128, 64)
SPLITK_SHAPE = (128, 128, 256)      # 4 K-tiles of 64: one per split
SPLITK_KS = (128, 159, 191)         # all inside split 2 of 4


def splitk_payload(kind, side):
    return nonfinite(kind, side, *SPLITK_SHAPE, ks=SPLITK_KS)


def row_payloads(row):
    """Every payload the raw-kernel tests feed this row."""
    shape = (row.tm, row.tn, row.kq)
    for side in SIDES:
        if row.kind in ("bf16", "fp8", "mxfp8"):
            yield nonfinite(row.kind, side, *shape)
        if row.kind == "bf16":
            yield overflow_and_underflow(row.kind, side, *shape)
            yield subnormal_inputs(row.kind, side, *shape)
        if row.kind in _MX:
            yield extreme_scales(row.kind, side, *shape)
            yield nan_scale(row.kind, side, *shape)


def all_payloads():
    seen = {}
    for row in ROWS:
        for p in row_payloads(row):
            seen.setdefault(p.name, p)
    for side in SIDES:
        for p in (nonfinite("bf16", side, *LAYOUT_SHAPE),
                  subnormal_inputs("bf16", side, *LAYOUT_SHAPE),
                  splitk_payload("bf16", side), splitk_payload("fp8", side)):
            seen.setdefault(p.name, p)
    return list(seen.values())

"""The table behind tests/test_gpu_stream_contract.py (docs/gemm.md,
"Streams"), shared with tests/test_stream_contract_logic.py, which guards on
the CPU that every ops function with a stream= keyword is placed, that the
padded shapes and temporary sizes below are what the front doors compute, and
that every payload makes "bitwise equal" the right expectation. torch on the
CPU only.

One Case per (function, path). `shape` is the logical (M, N, K) — for
colsum_bf16 (M, N, 0), for bmm with `batch` in kw — and `padded` what the
kernel runs on. `temps` are the byte sizes of the tensors the call allocates
and drops before it returns (padded operands, a padded C that is cropped,
scales, split-K workspace); probe C allocates four tensors of each on the
other stream. `probes` names the probes a case takes. `amax` / `bmax` bound the
integer operands: 4 / 4 everywhere, smaller where a bf16 output has to hold
the exact sum (K * amax * bmax + |bias| <= 256, every integer up to 256 being
a bf16 value).
"""

import functools
from collections import namedtuple

import torch

Case = namedtuple("Case", "name fn path shape padded kw temps probes amax bmax")

ALIGNED = "aligned, whole tiles"
BIAS_MAX = 8
I32_POISON = 0x7FFFFFFF

RAGGED = (130, 136, 72)
RAGGED_MX = (130, 136, 96)
P = (256, 256, 128)             # RAGGED padded: 256^2 kernels and 128/128/64
P_I8 = (256, 256, 256)
BF16_OUT = dict(out_dtype="bf16")


def _case(name, fn, path, shape, padded, kw, temps, probes="ABC", amax=4,
          bmax=4):
    return Case(name, fn, path, shape, padded, kw, tuple(temps), probes, amax,
                bmax)


def _nt(es, p=P, split=0, c=4):
    """ap, bp, C (cropped), split-K workspace"""
    mp, np_, kp = p
    return [mp * kp * es, np_ * kp * es, mp * np_ * c] \
        + ([split * mp * np_ * 4] if split > 1 else [])


_MX_PAD = [256 * 4, 256 * 4]    # a_scale, b_scale padded to [256, 128 // 32]

FRONT_DOOR_CASES = [
    # matmul_nt: the 256^2 kernels, then gemm_splitk, then MX with scales
    _case("nt-bf16", "matmul_nt", "bf16", RAGGED, P, {}, _nt(2)),
    _case("nt-fp8", "matmul_nt", "fp8", RAGGED, P, {}, _nt(1)),
    _case("nt-i8", "matmul_nt", "i8", RAGGED, P_I8, {}, _nt(1, P_I8)),
    _case("nt-bf16-S2", "matmul_nt", "bf16", RAGGED, P, dict(split_k=2),
          _nt(2, split=2)),
    _case("nt-fp8-S2", "matmul_nt", "fp8", RAGGED, P, dict(split_k=2),
          _nt(1, split=2)),
    _case("nt-i8-S2", "matmul_nt", "i8", RAGGED, P, dict(split_k=2),
          _nt(1, split=2)),
    _case("nt-mxfp8", "matmul_nt", "mxfp8", RAGGED_MX, P, {},
          _nt(1) + _MX_PAD),
    _case("nt-mxfp4", "matmul_nt", "mxfp4", RAGGED_MX, P, {},
          [256 * 64, 256 * 64, 256 * 256 * 4] + _MX_PAD),
    # matmul: the four layouts, fp32 out
    *[_case(f"mm-{lay}", "matmul", lay, RAGGED, P, {}, _nt(2))
      for lay in ("nt", "nn", "tn", "tt")],
    *[_case(f"mm-{lay}-S2", "matmul", lay, RAGGED, P, dict(split_k=2),
            _nt(2, split=2)) for lay in ("nt", "nn", "tn", "tt")],
    # matmul: bf16 out; the padded bias is a temporary too
    *[_case(f"mm-{lay}-bf16-bias", "matmul", lay, RAGGED, P,
            dict(BF16_OUT, bias=True), _nt(2, c=2) + [256 * 4], amax=3, bmax=1)
      for lay in ("nt", "tn")],
    _case("mm-nn-relu-aux", "matmul", "nn", RAGGED, P,
          dict(BF16_OUT, bias=True, activation="relu", return_aux=True),
          _nt(2, c=2) + [256 * 256 * 2, 256 * 4], amax=3, bmax=1),
    _case("mm-nn-relu-grad", "matmul", "nn", RAGGED, P,
          dict(BF16_OUT, activation_grad="relu"),
          _nt(2, c=2) + [256 * 256 * 2], amax=3, bmax=1),
    # a stored [128, 64] one element into its allocation: no pad, no crop,
    # only the .clone() of the misaligned operand
    _case("mm-nn-offset", "matmul", ALIGNED + ", a 2 bytes off -> clone",
          (128, 128, 64), (128, 128, 64), dict(layout="nn", offset_a=1),
          [128 * 64 * 2]),
    # matmul_mx: K 72 -> 96, quantize, then matmul_nt's MX path
    _case("mx-mxfp8", "matmul_mx", "mxfp8", RAGGED, P, {},
          [130 * 96 * 2, 136 * 96 * 2, 130 * 96, 136 * 96, 130 * 3, 136 * 3]
          + _nt(1) + _MX_PAD),
    _case("mx-mxfp4", "matmul_mx", "mxfp4", RAGGED, P, {},
          [130 * 96 * 2, 136 * 96 * 2, 130 * 48, 136 * 48, 130 * 3, 136 * 3,
           256 * 64, 256 * 64, 256 * 256 * 4] + _MX_PAD),
    # bmm
    _case("bmm-f32", "bmm", "nn", RAGGED, P, dict(batch=3),
          [3 * x for x in _nt(2)]),
    _case("bmm-bf16", "bmm", "nn", RAGGED, P, dict(BF16_OUT, batch=3),
          [3 * x for x in _nt(2, c=2)], amax=3, bmax=1),
    _case("bmm-broadcast", "bmm", "nn", RAGGED, P,
          dict(batch=3, broadcast_a=True),
          [256 * 128 * 2, 3 * 256 * 128 * 2, 3 * 256 * 256 * 4]),
    # heads of [T, H*D], T = D = 128, H = 3: read in place, nothing cropped
    _case("bmm-heads", "bmm", ALIGNED + ", heads read in place",
          (128, 128, 128), (128, 128, 128), dict(batch=3), [], probes="BC"),
    # colsum_bf16: (M, N); `padded` is (M, N up to 8, chunks)
    _case("colsum-pad", "colsum_bf16", "out=None", (5, 13, 0), (5, 16, 1), {},
          [5 * 16 * 2]),
    _case("colsum-pad-out", "colsum_bf16", "out, N padded -> copy_",
          (5, 13, 0), (5, 16, 1), dict(out="aligned"), [5 * 16 * 2, 16 * 4]),
    _case("colsum-chunks", "colsum_bf16", "out=None, two chunks", (64, 13, 0),
          (64, 16, 2), {}, [64 * 16 * 2]),
    _case("colsum-direct", "colsum_bf16", ALIGNED + ", out written directly",
          (5, 16, 0), (5, 16, 1), dict(out="aligned"), []),
    _case("colsum-out-offset", "colsum_bf16",
          ALIGNED + ", out 4 bytes off -> copy_", (5, 16, 0), (5, 16, 1),
          dict(out="offset"), [16 * 4]),
]

T = (128, 128, 128)             # whole tiles, two K-tiles: splits=2
_WS = [2 * 128 * 128 * 4]

# strict calls: whole tiles, workspace=None; each runs with the stream as a
# torch object and as its raw handle
STRICT_CASES = [
    _case("splitk-bf16", "gemm_splitk", "bf16", T, T, dict(splits=2), _WS,
          "BC"),
    _case("splitk-fp8", "gemm_splitk", "fp8", T, T, dict(splits=2), _WS, "BC"),
    _case("splitk-i8", "gemm_splitk", "i8", T, T, dict(splits=2), _WS, "BC"),
    _case("layout-splitk-tn", "gemm_bf16_layout_splitk", "tn", T, T,
          dict(splits=2), _WS, "BC"),
    _case("epilogue-S2", "gemm_bf16_epilogue", "nt", T, T,
          dict(splits=2, bias=True), _WS, "BC", amax=1, bmax=1),
    _case("act-S2", "gemm_bf16_act", "nt", T, T,
          dict(splits=2, bias=True, activation="relu", aux_out=True), _WS,
          "BC", amax=1, bmax=1),
    _case("quantize-mxfp8", "quantize_mx", "mxfp8", (130, 0, 96), (130, 0, 96),
          {}, [], "B"),
    _case("quantize-mxfp4", "quantize_mx", "mxfp4", (130, 0, 96), (130, 0, 96),
          {}, [], "B"),
    # one launch, no allocation: (numel, 0, 0)
    _case("fill", "fill", "", (1000, 0, 0), (1000, 0, 0), {}, [], "B"),
    _case("iota", "iota", "", (1000, 0, 0), (1000, 0, 0), {}, [], "B"),
    _case("accumulate", "accumulate", "", (1000, 0, 0), (1000, 0, 0), {}, [],
          "B"),
    _case("copy_kernel", "copy_kernel", "", (1000, 0, 0), (1000, 0, 0), {}, [],
          "B"),
]

FRONT_DOORS = {"matmul_nt", "matmul", "matmul_mx", "bmm", "colsum_bf16"}

# function -> None (it has STRICT_CASES of its own) or the front-door case
# that hands the same stream= to this single-launch call
STRICT = {
    "gemm_splitk": None, "gemm_bf16_layout_splitk": None,
    "gemm_bf16_epilogue": None, "gemm_bf16_act": None, "quantize_mx": None,
    "fill": None, "iota": None, "accumulate": None, "copy_kernel": None,
    "gemm_bf16": "nt-bf16", "gemm_fp8": "nt-fp8", "gemm_i8": "nt-i8",
    "gemm_mxfp8": "nt-mxfp8", "gemm_mxfp4": "nt-mxfp4",
    "gemm_bf16_layout": "mm-nn", "gemm_bf16_batched": "bmm-f32",
}

EXEMPT = {
    "reduce_sum": "returns a Python float: it synchronizes by design",
    "busy_wait": "the blocker of the probes itself",
    "busy_wait_mfma": "the blocker's matrix-core sibling, same single launch",
}

AUTOGRAD = ["linear", "linear-bias", "mlp-relu", "bmm"]


def gen(*key):
    # Python's hash() of a str is salted per process; spell the seed out
    s = 0
    for part in key:
        for ch in str(part):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator(device="cpu").manual_seed(s)


def ints(g, shape, vmax):
    return torch.randint(-vmax, vmax + 1, shape, generator=g).double()


Payload = namedtuple("Payload", "a b bias aux refs wide")
_OPERAND_DTYPE = {"bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn,
                  "i8": torch.int8, "mxfp8": torch.float8_e4m3fn,
                  "mxfp4": torch.float32}


def relu64(z):
    return torch.where(z > 0, z, torch.zeros_like(z))


@functools.lru_cache(maxsize=None)
def payload(name, probe):
    """Operands in LOGICAL form, float64 integers: a [M,K] (bmm: [B,M,K], a
    broadcast one [1,M,K]), b [K,N] — for matmul_nt / matmul_mx and the strict
    nt calls the caller stores b transposed — bias [N] and aux [M,N] where the
    case takes them. wide is the tuple of float64 results, refs the same in
    the output dtypes. colsum: a is x; quantize_mx: a is x, no refs here
    (quantize_mx_reference is the oracle); the one-launch calls: a, b flat."""
    case = by_name(name)
    g = gen("stream-contract", name, probe)
    m, n, k = case.shape
    kw = case.kw
    if case.fn == "colsum_bf16":
        x = ints(g, (m, n), case.amax)
        wide = (x.sum(0),)
        return Payload(x, None, None, None, (wide[0].float(),), wide)
    if case.fn == "quantize_mx":
        return Payload(ints(g, (m, k), case.amax), None, None, None, (), ())
    if case.fn in ("fill", "iota", "accumulate", "copy_kernel"):
        a, b = ints(g, (m,), case.amax), ints(g, (m,), case.bmax)
        wide = {"fill": torch.full((m,), float(int(b[0]) + 5.0)).double(),
                "iota": torch.arange(m).double(), "accumulate": a + b,
                "copy_kernel": b}[case.fn]
        return Payload(a, b, None, None, (wide.float(),), (wide,))
    batch = kw.get("batch")
    lead = () if batch is None else (batch,)
    a = ints(g, ((1,) if kw.get("broadcast_a") else lead) + (m, k), case.amax)
    b = ints(g, lead + (k, n), case.bmax)
    bias = ints(g, (n,), BIAS_MAX) if kw.get("bias") else None
    acc = torch.matmul(a, b)
    z = acc if bias is None else acc + bias
    aux = None
    out = torch.bfloat16 if kw.get("out_dtype") == "bf16" \
        or case.fn in ("gemm_bf16_epilogue", "gemm_bf16_act") \
        else torch.int32 if case.path == "i8" else torch.float32
    if kw.get("activation_grad"):
        aux = ints(g, (m, n), 4)
        wide = (acc * (aux > 0).double(),)
    elif kw.get("activation"):
        wide = (relu64(z), z) if kw.get("return_aux") or kw.get("aux_out") \
            else (relu64(z),)
    else:
        wide = (z,)
    refs = tuple(w.to(torch.int32) if out is torch.int32
                 else w.float().to(out) for w in wide)
    return Payload(a, b, bias, aux, refs, wide)


def assert_exact(case, p):
    """The _assert_exact condition: integer operands, K max|a| max|b| < 2^24
    so every partial sum is exact in any order, and the wide reference
    survives the cast to the output dtype — for a bf16 output, every wide
    value is a bf16 value. Every comparison is then bitwise."""
    for t in (p.a, p.b, p.bias, p.aux):
        if t is not None:
            assert torch.equal(t, t.round())
    if p.b is not None and case.shape[2]:
        k = case.shape[2]
        assert float(p.a.abs().max()) <= case.amax
        assert float(p.b.abs().max()) <= case.bmax
        assert k * case.amax * case.bmax < 2 ** 24
    elif case.fn == "colsum_bf16":
        assert case.shape[0] * case.amax < 2 ** 24
    assert len(p.refs) == len(p.wide)
    for ref, wide in zip(p.refs, p.wide):
        assert torch.equal(ref.double(), wide)
        if ref.dtype == torch.bfloat16:
            assert float(wide.abs().max()) <= 256
            assert torch.equal(wide.float().bfloat16().double(), wide)


def all_cases():
    return FRONT_DOOR_CASES + STRICT_CASES


def by_name(name):
    found = [c for c in all_cases() if c.name == name]
    assert len(found) == 1, name
    return found[0]


def case_probes(cases):
    return [(c.name, p) for c in cases for p in c.probes]

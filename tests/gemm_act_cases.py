"""The acceptance rule, the committed epsilon and the GELU payloads of
tests/test_gpu_gemm_act.py, shared with tests/test_gemm_act_logic.py, which
guards on the CPU that the rule discriminates and that its intervals stay
narrow on every payload. torch on the CPU only.

The rule (docs/gemm.md, "Activations"): the GPU's exp and reciprocal are not
bit-reproducible on the CPU, so a GELU output `got` is accepted iff

    RNE_bf16(ref - delta) <= got <= RNE_bf16(ref + delta)

    forward    ref = gelu64(z32)            delta = eps(z32) |ref|
    gradient   ref = acc32 gelu'64(aux)     delta = eps(aux) |acc32| T(aux)

with T = |s| + |second term| of gelu'. z32 and acc32 are fp32 results of
kernels that existed before the activation epilogues. eps is the bound
derived from the instruction sequence: (A + 4 |2u(z)|) 2^-24, the second
term being the error of exp's argument amplified by exp; its largest value
for |z| <= 8 is below EPS_MAX = 2^-16.
"""

import functools
import math
from collections import namedtuple

import torch

import gemm_epilogue_cases as cases

# docs/gemm.md, "Activations": relative error <= (A + 4 |2u|) 2^-24 with
# A = 6 (forward) and 18 (gradient) to first order, one unit added to each
# for the products of errors the first order leaves out. |2u| <= 49.3 for
# |z| <= 8, so eps <= 204.2 and 216.2 units: below EPS_MAX.
EPS_A_FORWARD = 7.0
EPS_A_GRAD = 19.0
EPS_MAX = 2.0 ** -16
Z_MAX = 8.0
AMBIGUOUS_CAP = 0.02

GELU_SHAPES = [(128, 128, 64), (256, 384, 512)]
MLP = (256, 128, 256, 128)          # tokens, in, hidden, out

GeluPayload = namedtuple("GeluPayload", "a b bias aux")


def rne_bf16(x):
    """float64 -> the nearest bf16 value (ties to even), as float64, in ONE
    rounding (x.float().to(bfloat16) would round twice). For |x| in the
    normal range of bf16 or 0; NaN and Inf pass through."""
    x = x.double().contiguous()
    bits = x.view(torch.int64)
    drop = 52 - 7
    lsb = (bits >> drop) & 1
    rounded = (bits + ((1 << (drop - 1)) - 1) + lsb) & ~((1 << drop) - 1)
    out = rounded.view(torch.float64)
    return torch.where(torch.isfinite(x), out, x)


def interval(ref, delta):
    return rne_bf16(ref - delta), rne_bf16(ref + delta)


def accepted(got, ref, delta):
    """elementwise: got (bf16 or anything exact in float64) inside the
    interval"""
    lo, hi = interval(ref, delta)
    got = got.double()
    return (lo <= got) & (got <= hi)


def ambiguous_share(ref, delta):
    lo, hi = interval(ref, delta)
    return float((lo != hi).double().mean())


def eps(z, a_units):
    z = z.double()
    u2 = 2.0 * 0.7978845608028654 * (z + 0.044715 * z * z * z)
    return (a_units + 4.0 * u2.abs()) * 2.0 ** -24


def forward_ref(ops, z32):
    """(ref, delta) of the forward rule from the fp32 pre-activation"""
    ref = ops.activation_reference(z32.double(), "gelu")
    return ref, eps(z32, EPS_A_FORWARD) * ref.abs()


def grad_ref(ops, acc32, aux):
    """(ref, delta) of the gradient rule from the fp32 accumulators and the
    bf16 aux"""
    first, second = ops.activation_grad_terms(aux.double(), "gelu")
    acc = acc32.double()
    return acc * (first + second), eps(aux, EPS_A_GRAD) * acc.abs() \
        * (first.abs() + second.abs())


def gelu_scale(k, count):
    """power of two for one operand of a randn product over k terms with
    `count` outputs: the largest that keeps the expected extreme of the
    outputs, sigma (sqrt(2 ln count) + 0.7), below 7.5"""
    sigma = 7.5 / (math.sqrt(2.0 * math.log(count)) + 0.7)
    return 2.0 ** math.floor(math.log2(sigma / math.sqrt(k)))


@functools.lru_cache(maxsize=None)
def gelu_payload(m, n, k):
    """randn bf16 operands, a scaled by a power of two, and a small bias
    ramp, so that max |a @ b + bias| <= 8 (asserted on the CPU); aux is a
    separate bf16 [m, n] tensor ~ 2.5 randn clipped to +-8 for the gradient
    mode."""
    g = cases._gen("act-gelu", m, n, k)
    a = (torch.randn(m, k, generator=g) * gelu_scale(k, m * n)).to(torch.bfloat16)
    b = torch.randn(k, n, generator=g).to(torch.bfloat16)
    bias = ((torch.arange(n) % 17) - 8).float() / 32.0
    aux = (2.5 * torch.randn(m, n, generator=g)).clamp(-Z_MAX, Z_MAX) \
        .to(torch.bfloat16)
    return GeluPayload(a, b, bias, aux)


def gelu_payload_shapes():
    """every (M, N, K) the GPU file judges by the rule"""
    assert cases.RANDN in GELU_SHAPES
    return GELU_SHAPES + [cases.SPLITK, cases.GRID_STRIDE[:3]]


def cpu_z32(p):
    return p.a.float() @ p.b.float() + p.bias


def cpu_acc32(p):
    return p.a.float() @ p.b.float()


def hash_sign_aux(m, n):
    """bf16 [m, n], value +-(1 + (row % 7)) with the sign a non-symmetric
    hash of (global row, global column): a tile-local, transposed or
    lane-indexed read of it gives another mask"""
    r = torch.arange(m).view(-1, 1)
    c = torch.arange(n).view(1, -1)
    h = (r * 2654435761 + c * 40503 + (r * c) % 8191 + (r >> 3) * 7) % 11
    sign = torch.where(h < 5, -1.0, 1.0)
    return (sign * (1 + (r % 7)).float()).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def mlp_payload(tokens, n_in, hidden, n_out):
    """x, w1, b1, w2, b2, dy: randn, scaled so the pre-activation stays
    within +-8"""
    g = cases._gen("act-mlp", tokens, n_in, hidden, n_out)
    x = torch.randn(tokens, n_in, generator=g).to(torch.bfloat16)
    w1 = (torch.randn(hidden, n_in, generator=g)
          * gelu_scale(n_in, tokens * hidden)).to(torch.bfloat16)
    b1 = ((torch.arange(hidden) % 17) - 8).float() / 32.0
    w2 = (torch.randn(n_out, hidden, generator=g)
          * gelu_scale(hidden, tokens * n_out)).to(torch.bfloat16)
    b2 = ((torch.arange(n_out) % 13) - 6).float() / 16.0
    dy = torch.randn(tokens, n_out, generator=g).to(torch.bfloat16)
    return x, w1, b1, w2, b2, dy

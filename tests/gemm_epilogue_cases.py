"""Payloads, shapes and the CPU oracle of tests/test_gpu_gemm_epilogue.py,
shared with tests/test_gemm_epilogue_logic.py, which guards on the CPU that
the oracle alone meets every exact expectation. torch on the CPU only.

Exact payloads are built in LOGICAL form a [M,K], b [K,N]:

    a   three non-zeros per row, values -2..2, at k spread over the K-tiles
    b   integers -4..4, column n scaled by 2^(n // 101)
    bias[n] = ((n % 101) - 50.5) * 2^(n // 101)

so |acc| <= 24 and |acc + bias| <= 74.5 times a power of two: 149 half
units, 8 significant bits, a bf16 value. The bias is an odd number of half
units times a power of two that changes every 101 columns, so it is
distinct in every column (and never zero), and it is asymmetric: a bias
indexed by row, by tile-local column or by lane gives other numbers.
"""

import functools
from collections import namedtuple

import torch

LAYOUTS = ["nt", "nn", "tn", "tt"]

# (M, N, K): one trip (the vmcnt(0) arm at once); three trips (both buffer
# swaps); a ragged grid of 15 workgroups
EXACT = [(128, 128, 64), (128, 128, 192)]
RAGGED_GRID = (384, 640, 192)
IDENTITY = (128, 256, 128)          # a = I: C is b, a transposed store shows
ROUNDING = (128, 128, 64)
RANDN = (256, 384, 512)
REPEATS = 10
SPLITK = (128, 128, 320)            # T = 5
SPLITK_SPLITS = (1, 2, 3, 5)
RAGGED_SPLITS = (2, 3)
# the bf16 fold walks grid-stride once M*N/8 > 1024 * 256: 129 tiles
GRID_STRIDE = (384, 5504, 128, 2)
COLSUM_M = (1, 7, 513, 4099)
COLSUM_N = (8, 136, 1000)
COLSUM_RANDN = (4099, 1000)
FRONT_DOOR = (100, 130, 70)         # logical; pads to (128, 256, 128)
LINEAR = (2048, 128, 128)           # tokens, out features, in features
N_CU = 256

Payload = namedtuple("Payload", "a b bias wide")

BF16_MAX = 3.3895313892515355e38    # 0x7F7F


def _gen(*key):
    s = 0
    for part in key:
        for ch in str(part):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator(device="cpu").manual_seed(s)


def col_scale(n):
    return torch.tensor([2.0 ** (j // 101) for j in range(n)],
                        dtype=torch.float64)


def exact_bias(n):
    base = torch.tensor([(j % 101) - 50.5 for j in range(n)],
                        dtype=torch.float64)
    return (base * col_scale(n)).float()


@functools.lru_cache(maxsize=None)
def exact_payload(m, n, k):
    g = _gen("epilogue", m, n, k)
    a = torch.zeros(m, k)
    rows = torch.arange(m)
    for j in range(3):
        a[rows, (5 * rows + j * (k // 3) + j) % k] = ((rows + j) % 5 - 2).float()
    b = torch.randint(-4, 5, (k, n), generator=g).double() * col_scale(n)
    bias = exact_bias(n)
    wide = a.double() @ b + bias.double()
    return Payload(a.to(torch.bfloat16), b.to(torch.bfloat16), bias, wide)


@functools.lru_cache(maxsize=None)
def identity_payload():
    m, n, k = IDENTITY
    a = torch.eye(m, k)
    kk, nn = torch.meshgrid(torch.arange(k), torch.arange(n), indexing="ij")
    b = ((3 * kk + 5 * nn) % 19 - 9).double() * col_scale(n)
    bias = exact_bias(n)
    wide = a.double() @ b + bias.double()
    return Payload(a.to(torch.bfloat16), b.to(torch.bfloat16), bias, wide)


# (acc, bias, expected bf16): ties both ways and their negatives, a sum
# just above a tie that is exact in fp32, sums that need no rounding
ROUNDING_CASES = [
    (256.0, 1.0, 256.0), (258.0, 1.0, 260.0),
    (-256.0, -1.0, -256.0), (-258.0, -1.0, -260.0),
    (256.0, 1.0 + 2.0 ** -15, 258.0), (-256.0, -1.0 - 2.0 ** -15, -258.0),
    (3.0, 0.75, 3.75),
]
OVERFLOW_COLS = 16  # the last columns: +-(bf16 max) + +-2^119 -> +-Inf


@functools.lru_cache(maxsize=None)
def rounding_payload():
    """One-hot k-gather: a[m, m % K] = 1, so acc[m, n] = b[m % K, n], a
    chosen bf16 value. Column n < N - 16 is case n % 7 scaled by 2^-n (a
    power of two moves a tie with it, and makes the bias distinct per
    column); the last 16 columns overflow to +-Inf."""
    m, n, k = ROUNDING
    a = torch.zeros(m, k)
    a[torch.arange(m), torch.arange(m) % k] = 1.0
    acc = torch.zeros(n, dtype=torch.float64)
    bias = torch.zeros(n, dtype=torch.float64)
    want = torch.zeros(n, dtype=torch.float64)
    nc = len(ROUNDING_CASES)
    for j in range(n - OVERFLOW_COLS):
        s = 2.0 ** -j
        c = ROUNDING_CASES[j % nc]
        acc[j], bias[j], want[j] = c[0] * s, c[1] * s, c[2] * s
    for j in range(n - OVERFLOW_COLS, n):
        sign = 1.0 if j % 2 == 0 else -1.0
        acc[j], bias[j] = sign * BF16_MAX, sign * 2.0 ** 119
        want[j] = sign * float("inf")
    b = acc.expand(k, n).contiguous()
    wide = a.double() @ b + bias          # float64: exact
    return Payload(a.to(torch.bfloat16), b.to(torch.bfloat16), bias.float(),
                   wide), want.expand(m, n)


@functools.lru_cache(maxsize=None)
def randn_payload(m, n, k):
    g = _gen("epilogue-randn", m, n, k)
    a = torch.randn(m, k, generator=g).to(torch.bfloat16)
    b = torch.randn(k, n, generator=g).to(torch.bfloat16)
    bias = (torch.arange(n).float() * 0.37 - 3.0) * 0.125
    return Payload(a, b, bias, None)


def stored(p, layout):
    """the operands as `layout` stores them, contiguous, on the CPU"""
    a = p.a.t().contiguous() if layout[0] == "t" else p.a
    b = p.b.t().contiguous() if layout[1] == "t" else p.b
    return a, b


def oracle(c32, bias=None):
    """THE reference of every test: fp32 C of an existing kernel (or an
    exact fp32 C), on the CPU, one fp32 add, one conversion"""
    c32 = c32.detach().cpu().float()
    if bias is not None:
        c32 = c32 + bias.detach().cpu().float()
    return c32.to(torch.bfloat16)


def bf16_exact_or_tie(wide):
    """True where a float64 value is a bf16 value, or lies exactly between
    two neighbouring ones (so round-to-nearest-even is defined by the tie
    rule alone, with no dependence on how the sum was formed)"""
    down = wide.float().view(torch.int32) & ~0xFFFF       # truncate
    lo = down.view(torch.float32).double()
    hi = (down + 0x10000).view(torch.float32).double()
    finite = torch.isfinite(wide) & torch.isfinite(hi)
    exact = wide == lo
    tie = (wide - lo) == (hi - wide)
    return ~finite | exact | tie


def colsum_payload(m, n):
    """integers -3..3, distinct pattern per column: every partial sum of a
    column is an integer below 2^24, exact in fp32 in any order"""
    g = _gen("colsum", m, n)
    x = torch.randint(-3, 4, (m, n), generator=g).float()
    x[:, ::3] += 1.0
    return x.to(torch.bfloat16)


def colsum_mr_pairs(plan):
    """every (M, R) the GPU file runs; plan(m, n) is colsum_plan at N_CU"""
    pairs = {(m, plan(m, -(-n // 8) * 8)) for m in COLSUM_M for n in COLSUM_N}
    pairs.add((COLSUM_RANDN[0], plan(*COLSUM_RANDN)))
    pairs.add((LINEAR[0], plan(LINEAR[0], LINEAR[1])))
    return sorted(pairs)

"""Payloads shared by tests/test_mx_quant_reference.py (CPU) and
tests/test_gpu_mx_quant.py (GPU). Everything is a float32 CPU tensor built
from a fixed seed; a block is 32 consecutive elements of a row."""

import torch

FLT_MAX = 3.4028234663852886e38
E2M1_MAGNITUDES = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
# the tie table of docs/gemm.md: value -> e2m1 nibble at scale 1.0
E2M1_TIES = [(4.0, 6), (0.25, 0), (0.75, 2), (1.25, 2), (1.75, 4),
             (2.5, 4), (3.5, 6), (5.0, 6), (-0.25, 8)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def lossless(fmt, rows, k, seed=0, scales=(124, 130)):
    """Values MX represents exactly: integers -4..4 (mxfp8) or the e2m1
    codes up to +-2 (mxfp4), times 2^(s-127) with s drawn per block."""
    g = _gen(seed)
    ints = torch.randint(-4, 5, (rows, k // 32, 32), generator=g)
    base = ints.float() if fmt == "mxfp8" else ints.float() * 0.5
    s = torch.randint(scales[0], scales[1] + 1, (rows, k // 32, 1), generator=g)
    return (base * torch.exp2((s - 127).float())).view(rows, k)


def wide_randn(rows, k, seed=1):
    """randn times a per-block 2^U(-20, 20)."""
    g = _gen(seed)
    x = torch.randn(rows, k // 32, 32, generator=g)
    u = torch.rand(rows, k // 32, 1, generator=g) * 40 - 20
    return (x * torch.exp2(u)).view(rows, k)


def edge_blocks():
    """[n, 32]: one edge block per row; names in EDGE_NAMES order."""
    def block(*head):
        b = torch.zeros(32)
        b[: len(head)] = torch.tensor(head, dtype=torch.float32)
        return b

    sub = 1e-40                              # fp32 (and bf16) subnormal
    rows = {
        "all_zero": block(),
        "neg_zero": block(-0.0, 0.0, -0.0),
        "subnormal_only": block(sub, -sub, 5e-39, -1.4e-45),
        "subnormal_beside_normal": block(1.0, sub, -sub, -0.375),
        "saturate_1p9": block(1.9, -1.9, 1.0, 0.1),
        "flt_max": block(FLT_MAX, -FLT_MAX, 1.0, 2.0 ** 120),
        "scale_clamps_to_0": block(2.0 ** -125, -(2.0 ** -126), 2.0 ** -126 * 1.5),
        "one_inf": block(1.0, float("inf"), -2.0),
        "one_neg_inf": block(1.0, -float("inf"), -2.0),
        "one_nan": block(3.0, 0.5, float("nan")),
    }
    return list(rows), torch.stack(list(rows.values()))


EDGE_NAMES, _ = edge_blocks()


def _pinned_blocks(values, pin):
    """Spread `values` over blocks of 31, each completed by one `pin`
    element (at a varying position) that fixes the block's scale."""
    vals = torch.tensor(values, dtype=torch.float32)
    n = -(-len(vals) // 31)
    out = torch.zeros(n, 32)
    for b in range(n):
        chunk = vals[b * 31:(b + 1) * 31]
        row = torch.cat([chunk, torch.zeros(31 - len(chunk))])
        p = (7 * b) % 32
        out[b] = torch.cat([row[:p], torch.tensor([pin]), row[p:]])
    return out


def e4m3_sweep():
    """Every finite e4m3 value and every midpoint between adjacent ones
    (exact in fp32 and in bf16), both signs, in blocks pinned at scale 127
    by one 448.0. Covers every rounding boundary of the format."""
    codes = torch.arange(0, 0x7F, dtype=torch.uint8)        # 0x7F is NaN
    mags = codes.view(torch.float8_e4m3fn).float()
    mids = (mags[:-1] + mags[1:]) / 2
    vals = torch.cat([mags, -mags, mids, -mids]).tolist()
    return _pinned_blocks(vals, 448.0)


def e2m1_sweep():
    """The same for e2m1: 8 magnitudes and 7 midpoints, both signs, pinned
    at scale 127 by one 6.0."""
    m = torch.tensor(E2M1_MAGNITUDES)
    mids = (m[:-1] + m[1:]) / 2
    vals = torch.cat([m, -m, mids, -mids]).tolist()
    return _pinned_blocks(vals, 6.0)


def sweep(fmt):
    return e4m3_sweep() if fmt == "mxfp8" else e2m1_sweep()


def unpack_nibbles(q):
    """uint8 [rows, K//2] -> uint8 nibbles [rows, K]."""
    return torch.stack([q & 0xF, q >> 4], dim=-1).view(q.shape[0], -1)


def codes(q, fmt):
    """One integer code per element: e4m3 byte or e2m1 nibble."""
    return q.view(torch.uint8) if fmt == "mxfp8" else unpack_nibbles(q)

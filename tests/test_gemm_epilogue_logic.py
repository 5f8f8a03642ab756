"""CPU guards of the bf16-output GEMM epilogue (native/gemm_epilogue.hip):
the oracle of tests/test_gpu_gemm_epilogue.py meets every exact expectation
by itself, the staged tile image is a bijection without bank conflicts, the
column-sum partition covers [0, M), and the front doors judge their new
keywords before they look at a tensor. No GPU."""

import pytest
import torch

import gemm_epilogue_cases as cases


@pytest.fixture(scope="module")
def lib():
    from hpc_patterns_amd._native import native

    return native()


@pytest.fixture
def ops():
    from hpc_patterns_amd import ops as _ops

    return _ops


# ---------------------------------------------------------------------------
# oracle guard
# ---------------------------------------------------------------------------

def _exact_payloads():
    out = [cases.exact_payload(*s) for s in cases.EXACT]
    out.append(cases.exact_payload(*cases.RAGGED_GRID))
    out.append(cases.exact_payload(*cases.SPLITK))
    out.append(cases.exact_payload(*cases.GRID_STRIDE[:3]))
    out.append(cases.identity_payload())
    return out


def test_exact_payloads_need_no_rounding():
    for p in _exact_payloads():
        wide = p.wide
        assert bool(cases.bf16_exact_or_tie(wide).all())
        # representable, not just a tie: the cast back and forth is exact
        assert torch.equal(wide.float().to(torch.bfloat16).double(), wide)
        # the oracle, from the exact fp32 product, gives the wide value
        c32 = (p.a.double() @ p.b.double()).float()
        assert torch.equal(c32.double(), p.a.double() @ p.b.double())
        assert torch.equal(cases.oracle(c32, p.bias).double(), wide)


def test_exact_bias_is_distinct_and_asymmetric():
    n = cases.RAGGED_GRID[1]
    bias = cases.exact_bias(n)
    assert len(set(bias.tolist())) == n
    assert not torch.equal(bias, bias.flip(0))
    assert torch.equal(bias.to(torch.bfloat16).float(), bias)


def test_rounding_payload_oracle():
    p, want = cases.rounding_payload()
    # every sum is exact in fp32, so the one rounding is the conversion's;
    # and but for the two "just above a tie" cases it is a bf16 value or a
    # tie
    finite = torch.isfinite(p.wide.float())
    assert torch.equal(p.wide.float().double()[finite], p.wide[finite])
    cols = torch.arange(p.wide.shape[1])
    above = (cols % len(cases.ROUNDING_CASES) >= 4) \
        & (cols % len(cases.ROUNDING_CASES) <= 5) \
        & (cols < p.wide.shape[1] - cases.OVERFLOW_COLS)
    assert bool(cases.bf16_exact_or_tie(p.wide)[:, ~above].all())
    assert not bool(cases.bf16_exact_or_tie(p.wide)[:, above].any())
    c32 = (p.a.double() @ p.b.double()).float()
    assert torch.equal(c32.double(), p.a.double() @ p.b.double())
    got = cases.oracle(c32, p.bias)
    assert torch.equal(got.double(), want)
    # the cases do discriminate: a bias rounded to bf16 first, or a
    # truncating conversion, gives other numbers
    early = (c32 + p.bias.to(torch.bfloat16).float()).to(torch.bfloat16)
    assert not torch.equal(early, got)
    trunc = ((c32 + p.bias).view(torch.int32) & ~0xFFFF).view(torch.float32)
    assert not torch.equal(trunc.double(), want)
    assert len(set(p.bias[:-cases.OVERFLOW_COLS].tolist())) \
        == p.bias.numel() - cases.OVERFLOW_COLS


def test_null_bias_is_no_add():
    c32 = torch.tensor([[-0.0, 1.0]])
    assert torch.signbit(cases.oracle(c32)[0, 0])
    assert not torch.signbit(cases.oracle(c32, torch.zeros(2))[0, 0])


# ---------------------------------------------------------------------------
# the staged tile: gemm_out_lds_offset / gemm_out_read, the functions the
# kernels call
# ---------------------------------------------------------------------------

def _lane_rc(wid, lane, m, n, r):
    """C/D mapping of the 8-wave 2x4 kernels: (row, col) of acc[m][n][r]"""
    wr, wc = divmod(wid, 4)
    return (wr * 64 + m * 16 + 4 * (lane >> 4) + r,
            wc * 32 + n * 16 + (lane & 15))


def test_image_is_a_bijection(lib):
    seen = set()
    for row in range(128):
        for col in range(128):
            off = lib.gemm_out_lds_offset(row, col)
            assert 0 <= off < 32768 and off % 2 == 0
            seen.add(off)
    assert len(seen) == 128 * 128
    # rows 2p and 2p+1 of a column share a dword, low half first
    for row in range(0, 128, 2):
        for col in range(128):
            off = lib.gemm_out_lds_offset(row, col)
            assert off % 4 == 0
            assert lib.gemm_out_lds_offset(row + 1, col) == off + 2


def test_writes_are_conflict_free(lib):
    """ds_write_b32: lane groups {0-31}, {32-63}, bank = (addr / 4) % 32"""
    for wid in range(8):
        for m in range(4):
            for n in range(2):
                for r in (0, 2):
                    for half in (0, 32):
                        banks = [lib.gemm_out_lds_offset(
                            *_lane_rc(wid, lane, m, n, r)) // 4 % 32
                            for lane in range(half, half + 32)]
                        assert len(set(banks)) == 32


# ds_read_b128: four groups of 16 lanes, bank = (addr / 4) % 64
_B128_GROUPS = [
    list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
    list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
    list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64)),
]


def test_reads_cover_the_tile_without_conflicts(lib):
    covered = set()
    for p in range(2):
        for wave in range(8):
            for i in range(2):
                addr = {}
                for lane in range(64):
                    t = wave * 64 + lane
                    row, col = lib.gemm_out_read(t, p, i)
                    assert row % 2 == 0 and col % 4 == 0
                    # the thread's 8 columns of rows row, row + 1
                    assert col // 8 == t % 16
                    assert row == 2 * (32 * p + t // 16)
                    addr[lane] = lib.gemm_out_lds_offset(row, col)
                    assert addr[lane] % 16 == 0
                    for dr in range(2):
                        for dc in range(4):
                            covered.add((row + dr, col + dc))
                            # the 16 bytes are 4 columns x 2 rows, in order
                            assert lib.gemm_out_lds_offset(row + dr, col + dc) \
                                == addr[lane] + 4 * dc + 2 * dr
                for group in _B128_GROUPS:
                    windows = [addr[lane] // 16 % 16 for lane in group]
                    assert len(set(windows)) == 16
            # reads 0 and 1 of a thread are its two chunks
            for lane in range(64):
                t = wave * 64 + lane
                c0 = lib.gemm_out_read(t, p, 0)[1]
                c1 = lib.gemm_out_read(t, p, 1)[1]
                odd_first = (t >> 3) & 1
                assert (c0, c1) == ((8 * (t % 16) + 4, 8 * (t % 16))
                                    if odd_first else
                                    (8 * (t % 16), 8 * (t % 16) + 4))
    assert len(covered) == 128 * 128


# ---------------------------------------------------------------------------
# column-sum partition and plan
# ---------------------------------------------------------------------------

def test_colsum_partition_covers_rows(lib):
    pairs = cases.colsum_mr_pairs(
        lambda m, n: lib.colsum_plan(m, n, cases.N_CU))
    assert any(r == 1 for _, r in pairs) and any(r > 1 for _, r in pairs)
    for m, r_total in pairs:
        assert 1 <= r_total <= min(m, lib.COLSUM_MAX_CHUNKS)
        nxt = 0
        for r in range(r_total):
            first, count = lib.colsum_rows(m, r_total, r)
            assert first == nxt and count >= 1
            nxt = first + count
        assert nxt == m
        if r_total > 1:
            assert m // r_total >= lib.COLSUM_MIN_ROWS


def test_colsum_pitch(lib):
    assert [lib.colsum_pitch(n) for n in (8, 1000, 1024, 1032)] \
        == [1024, 1024, 1024, 2048]


def test_fold_grid_stride_shape(lib):
    m, n, _, _ = cases.GRID_STRIDE
    assert m * n // 8 // 256 == lib.SPLITK_REDUCE_MAX_GRID + 8
    assert (m // 128) * (n // 128) == 129     # one tile past the capacity


# ---------------------------------------------------------------------------
# front doors: keywords before tensors, error types, padding
# ---------------------------------------------------------------------------

class _Untouchable:
    """stands in for a tensor; any look at it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"tensor looked at (.{name}) before the "
                             f"keywords were judged")


def test_matmul_judges_keywords_first(ops):
    t = _Untouchable()
    with pytest.raises(ValueError, match="out_dtype"):
        ops.matmul(t, t, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="out_dtype"):
        ops.matmul(t, t, out_dtype="bf16")
    with pytest.raises(TypeError, match="bias"):
        ops.matmul(t, t, out_dtype=torch.bfloat16, bias=[1.0])
    with pytest.raises(ValueError, match="bias needs out_dtype"):
        ops.matmul(t, t, bias=torch.zeros(4))
    with pytest.raises(ValueError, match="split_k"):
        ops.matmul(t, t, split_k="many", out_dtype=torch.bfloat16)


def test_linear_judges_keywords_first(ops):
    t = _Untouchable()
    with pytest.raises(ValueError, match="fused"):
        ops.linear_bf16(t, t, fused=1)
    with pytest.raises(ValueError, match="fused"):
        ops.linear_bf16(t, t, fused="yes")
    with pytest.raises(TypeError, match="bias"):
        ops.linear_bf16(t, t, bias=3.0)
    with pytest.raises(ValueError, match="split_k"):
        ops.linear_bf16(t, t, split_k=2, bias=torch.zeros(4))


def test_matmul_bf16_shape_and_dtype_rules(ops):
    a = torch.zeros(100, 70, dtype=torch.bfloat16)
    b = torch.zeros(70, 130, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="bias must have shape"):
        ops.matmul(a, b, out_dtype=torch.bfloat16, bias=torch.zeros(100))
    with pytest.raises(TypeError, match="bias must be bfloat16 or float32"):
        ops.matmul(a, b, out_dtype=torch.bfloat16,
                   bias=torch.zeros(130, dtype=torch.float64))
    with pytest.raises(ValueError, match="split_k"):
        ops.matmul(a, b, out_dtype=torch.bfloat16, split_k=3)  # 128/64 = 2
    with pytest.raises(TypeError, match="bf16 operands"):
        ops.matmul(a.float(), b.float(), out_dtype=torch.bfloat16)


def test_padded_bias(ops):
    bias = torch.arange(130, dtype=torch.bfloat16)
    out = ops.__dict__["_bias_f32"](bias, 130, 256, bias.device)
    assert out.dtype == torch.float32 and out.shape == (256,)
    assert torch.equal(out[:130], bias.float())     # widening is exact
    assert not bool(out[130:].any())
    same = torch.arange(128, dtype=torch.float32)
    assert ops.__dict__["_bias_f32"](same, 128, 128, same.device) is same
    assert ops.gemm_layout_pad_shapes(*cases.FRONT_DOOR) == (128, 256, 128)


def test_linear_shape_rules(ops):
    x = torch.zeros(8, 16, dtype=torch.bfloat16)
    w = torch.zeros(4, 16, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="bias must have shape"):
        ops.linear_bf16(x, w, bias=torch.zeros(8))
    with pytest.raises(TypeError, match="bias must be bfloat16 or float32"):
        ops.linear_bf16(x, w, bias=torch.zeros(4, dtype=torch.float16))


def test_linear_default_does_not_reach_new_entry_points(ops, monkeypatch):
    """without bias and fused, linear_bf16 runs what it ran before: none of
    the new functions, python or native"""
    def boom(*a, **k):
        raise AssertionError("new entry point reached")

    class Lib:
        def __getattr__(self, name):
            if name in ("gemm_bf16_epilogue", "colsum_bf16"):
                return boom
            raise RuntimeError(f"native {name}")    # the old path, no GPU

    monkeypatch.setattr(ops, "native", lambda: Lib())
    monkeypatch.setattr(ops, "gemm_bf16_epilogue", boom)
    monkeypatch.setattr(ops, "colsum_bf16", boom)
    seen = []
    monkeypatch.setattr(ops, "matmul_nt", lambda x, w, split_k=None:
                        seen.append(split_k) or torch.zeros(8, 4))
    x = torch.zeros(8, 16, dtype=torch.bfloat16)
    w = torch.zeros(4, 16, dtype=torch.bfloat16)
    for kw in ({}, {"split_k": "auto"}, {"fused": None}, {"fused": False},
               {"bias": None}):
        y = ops.linear_bf16(x, w, **kw)
        assert y.dtype == torch.bfloat16 and y.shape == (8, 4)
    assert seen == [None, "auto", None, None, None]
    # and the new keywords do reach them
    with pytest.raises(AssertionError, match="new entry point"):
        ops.linear_bf16(x, w, fused=True)

"""CPU guards of the batched, strided bf16 GEMM (native/gemm_batched.hip):
bmm_layout reads the layout from the strides, the C-overlap rule accepts
only disjoint images (enumerated), bmm's copy / no-copy decision and padded
shapes, keywords before tensors, and the existing front doors do not reach
the new native entry point. No GPU."""

import itertools

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from hpc_patterns_amd._native import native

    return native()


@pytest.fixture
def ops():
    from hpc_patterns_amd import ops as _ops

    return _ops


BF = torch.bfloat16


# ---------------------------------------------------------------------------
# bmm_layout
# ---------------------------------------------------------------------------

def test_layout_all_four_from_views(ops):
    bsz, m, n, k = 2, 3, 5, 7
    a_n = torch.zeros(bsz, m, k, dtype=BF)
    a_t = torch.zeros(bsz, k, m, dtype=BF).transpose(1, 2)
    b_n = torch.zeros(bsz, k, n, dtype=BF)
    b_t = torch.zeros(bsz, n, k, dtype=BF).transpose(1, 2)
    for (a, fa), (b, fb) in itertools.product(((a_n, "n"), (a_t, "t")),
                                              ((b_n, "n"), (b_t, "t"))):
        assert a.shape == (bsz, m, k) and b.shape == (bsz, k, n)
        layout, a_st, b_st = ops.bmm_layout(a, b)
        assert layout == fa + fb
        assert a_st.shape == ((bsz, k, m) if fa == "t" else (bsz, m, k))
        assert b_st.shape == ((bsz, k, n) if fb == "n" else (bsz, n, k))
        for st, src in ((a_st, a), (b_st, b)):
            assert st.stride(2) == 1 and st.is_contiguous()
            assert st.data_ptr() == src.data_ptr()      # a view, no copy


def test_layout_size_one_reads_as_row_major(ops):
    # [B, M, 1] contiguous: strides (M, 1, 1) fit both readings
    a = torch.zeros(2, 4, 1, dtype=BF)
    b = torch.zeros(2, 1, 1, dtype=BF)
    assert a.stride(2) == 1 and a.stride(1) == 1
    layout, a_st, b_st = ops.bmm_layout(a, b)
    assert layout == "nn" and a_st is a and b_st is b
    # the transposed view of a size-1 dimension is row-major as well
    at = torch.zeros(2, 1, 4, dtype=BF).transpose(1, 2)
    assert at.shape == (2, 4, 1) and at.stride() == (4, 1, 4)
    assert ops.bmm_layout(at, b)[0] == "tn"     # stride(2) == 4: not "n"
    at1 = torch.zeros(2, 1, 1, dtype=BF).transpose(1, 2)
    assert ops.bmm_layout(at1, b)[0] == "nn"


def test_layout_expanded_operand(ops):
    w = torch.zeros(7, 5, dtype=BF)                 # one [K,N] for all
    a = torch.zeros(3, 4, 7, dtype=BF)
    b = w.expand(3, 7, 5)
    layout, a_st, b_st = ops.bmm_layout(a, b)
    assert layout == "nn" and b_st.stride() == (0, 5, 1)
    assert b_st.data_ptr() == w.data_ptr()
    bt = torch.zeros(5, 7, dtype=BF).t().expand(3, 7, 5)   # stored [N,K]
    layout, _, b_st = ops.bmm_layout(a, bt)
    assert layout == "nt" and b_st.stride() == (0, 7, 1)
    assert b_st.shape == (3, 5, 7)


def test_layout_head_interleaved_permute(ops):
    t, h, d = 256, 3, 128
    x = torch.zeros(t, h * d, dtype=BF)
    y = torch.zeros(t, h * d, dtype=BF)
    q = x.view(t, h, d).permute(1, 0, 2)            # [H, T, D]
    k = y.view(t, h, d).permute(1, 2, 0)            # [H, D, T]
    layout, q_st, k_st = ops.bmm_layout(q, k)
    assert layout == "nt"
    assert q_st.shape == k_st.shape == (h, t, d)
    for st in (q_st, k_st):
        assert st.stride() == (d, h * d, 1)         # bs = D, ld = H*D
    assert q_st.data_ptr() == x.data_ptr() and k_st.data_ptr() == y.data_ptr()
    # P V: V [K=T, N=D] per head at ld = H*D
    p = torch.zeros(h, t, t, dtype=BF)
    v = y.view(t, h, d).permute(1, 0, 2)
    layout, _, v_st = ops.bmm_layout(p, v)
    assert layout == "nn" and v_st.stride() == (d, h * d, 1)


def test_layout_refuses_what_needs_a_copy(ops):
    a = torch.zeros(2, 4, 6, dtype=BF)
    b = torch.zeros(2, 6, 10, dtype=BF)[:, :, ::2]      # strides (60, 10, 2)
    assert b.shape == (2, 6, 5)
    with pytest.raises(TypeError, match="no hidden copies"):
        ops.bmm_layout(a, b)
    with pytest.raises(TypeError, match="3-D"):
        ops.bmm_layout(a[0], b)
    with pytest.raises(TypeError, match="3-D"):
        ops.bmm_layout(a, [1.0])
    with pytest.raises(ValueError, match="need a"):
        ops.bmm_layout(a, torch.zeros(2, 5, 3, dtype=BF))
    with pytest.raises(ValueError, match="need a"):      # no implicit batch
        ops.bmm_layout(a, torch.zeros(1, 6, 3, dtype=BF))


# ---------------------------------------------------------------------------
# the C-overlap rule against the enumerated address sets
# ---------------------------------------------------------------------------

def _images(batch, m, n, ldc, bsc):
    return [{b * bsc + i * ldc + j for i in range(m) for j in range(n)}
            for b in range(batch)]


def _disjoint(batch, m, n, ldc, bsc):
    imgs = _images(batch, m, n, ldc, bsc)
    if any(len(img) != m * n for img in imgs):      # rows of one image
        return False
    return len(set().union(*imgs)) == batch * m * n


def test_c_rule_accepts_only_disjoint_images(ops, lib):
    accepted = rejected_overlap = rejected_disjoint = 0
    for batch, m, n in itertools.product((1, 2, 3), (1, 2, 3), (1, 2, 4)):
        for ldc in range(0, 4 * n + 3):
            for bsc in range(0, 3 * m * n + 4):
                rule = ops.gemm_batched_c_disjoint(batch, m, n, ldc, bsc)
                assert rule == lib.gemm_batched_c_disjoint(batch, m, n, ldc,
                                                           bsc)
                truth = _disjoint(batch, m, n, ldc, bsc)
                if rule:
                    accepted += 1
                    assert truth, (batch, m, n, ldc, bsc)
                elif truth:
                    rejected_disjoint += 1      # the rule may be stricter
                else:
                    rejected_overlap += 1
    assert accepted > 100 and rejected_overlap > 100
    # what it turns away although disjoint: rows shorter than N of a
    # one-row image and the like, never one of the two forms
    assert rejected_disjoint < accepted


def test_c_rule_named_cases(ops):
    ok = ops.gemm_batched_c_disjoint
    # batch-major, contiguous and padded
    assert ok(3, 128, 128, 128, 128 * 128)
    assert ok(3, 128, 128, 136, 127 * 136 + 128)
    assert not ok(3, 128, 128, 136, 127 * 136 + 127)    # last row overlaps
    # heads interleaved inside a row: [T, H, D]
    assert ok(3, 256, 128, 3 * 128, 128)
    assert not ok(4, 256, 128, 3 * 128, 128)    # 4th head is the next row
    assert not ok(3, 256, 128, 3 * 128, 120)    # heads overlap by 8 columns
    assert not _disjoint(2, 2, 4, 8, 3)         # that kind, enumerated
    assert not ok(2, 2, 4, 8, 3)
    # an expanded C: every batch the same image
    assert not ok(2, 128, 128, 128, 0)
    # one batch: bsC means nothing
    assert ok(1, 128, 128, 128, 0) and ok(1, 128, 128, 128, 5)
    assert not ok(1, 128, 128, 127, 0)          # ldc < N
    assert not ok(0, 128, 128, 128, 0)


# ---------------------------------------------------------------------------
# copy / no copy, padded shapes
# ---------------------------------------------------------------------------

def test_direct_decision(ops):
    t, h, d = 256, 3, 128
    x = torch.zeros(t, h * d, dtype=BF)
    q = x.view(t, h, d).permute(1, 0, 2)
    assert ops.bmm_direct(q, 128, 64)                   # [H, T, D] K-contig
    assert ops.bmm_direct(q, 64, 128)                   # as a [K, X] operand
    full = torch.zeros(2, 128, 64, dtype=BF)
    assert ops.bmm_direct(full, 128, 64)
    assert not ops.bmm_direct(full, 64, 128)            # 64 columns of X
    assert not ops.bmm_direct(torch.zeros(2, 100, 64, dtype=BF), 128, 64)
    assert not ops.bmm_direct(torch.zeros(2, 128, 40, dtype=BF), 128, 64)
    # row stride off a multiple of 8
    wide = torch.zeros(2, 128, 68, dtype=BF)[:, :, :64]
    assert wide.stride(1) == 68 and not ops.bmm_direct(wide, 128, 64)
    assert ops.bmm_direct(torch.zeros(2, 128, 72, dtype=BF)[:, :, :64],
                          128, 64)
    # batch stride off a multiple of 8; with one batch it means nothing
    flat = torch.zeros(2 * (128 * 64 + 4), dtype=BF)
    odd = flat.as_strided((2, 128, 64), (128 * 64 + 4, 64, 1))
    assert not ops.bmm_direct(odd, 128, 64)
    assert ops.bmm_direct(odd[:1], 128, 64)
    # base 2 bytes / 16 bytes off
    base = torch.zeros(128 * 64 + 16, dtype=BF)
    assert base.data_ptr() % 16 == 0
    assert not ops.bmm_direct(base[1:1 + 128 * 64].view(1, 128, 64), 128, 64)
    assert ops.bmm_direct(base[8:8 + 128 * 64].view(1, 128, 64), 128, 64)
    # broadcast
    assert ops.bmm_direct(torch.zeros(128, 64, dtype=BF).expand(5, 128, 64),
                          128, 64)
    # a transposed view is not what the kernel reads
    assert not ops.bmm_direct(torch.zeros(2, 64, 128, dtype=BF)
                              .transpose(1, 2), 128, 64)


def test_padded_operand(ops):
    pad = ops.__dict__["_bmm_operand"]
    assert ops.gemm_layout_pad_shapes(100, 72, 40) == (128, 128, 64)
    t = torch.arange(3 * 100 * 40).reshape(3, 100, 40).to(BF)
    out = pad(t, 128, 64, 128, 64)
    assert out.shape == (3, 128, 64) and out.is_contiguous()
    assert torch.equal(out[:, :100, :40], t)
    assert not bool(out[:, 100:].any()) and not bool(out[:, :, 40:].any())
    # what qualifies is handed on as it is
    full = torch.zeros(3, 128, 64, dtype=BF)
    assert pad(full, 128, 64, 128, 64) is full
    # a broadcast operand is padded once
    w = torch.arange(100 * 40).reshape(100, 40).to(BF)
    out = pad(w.expand(3, 100, 40), 128, 64, 128, 64)
    assert out.shape == (3, 128, 64) and out.stride() == (0, 64, 1)
    assert torch.equal(out[2, :100, :40], w)
    assert ops.bmm_direct(out, 128, 64)


# ---------------------------------------------------------------------------
# keywords before tensors
# ---------------------------------------------------------------------------

class _Untouchable:
    """stands in for a tensor; any look at it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"tensor looked at (.{name}) before the "
                             f"keywords were judged")


def test_bmm_judges_keywords_first(ops):
    t = _Untouchable()
    with pytest.raises(ValueError, match="out_dtype"):
        ops.bmm(t, t, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="out_dtype"):
        ops.bmm(t, t, out_dtype="bf16")
    with pytest.raises(TypeError, match="alpha"):
        ops.bmm(t, t, alpha=torch.tensor(2.0))
    with pytest.raises(TypeError, match="alpha"):
        ops.bmm(t, t, out_dtype=torch.bfloat16, alpha="2")
    with pytest.raises(TypeError, match="alpha"):
        ops.bmm(t, t, alpha=None)
    with pytest.raises(TypeError, match="alpha"):
        ops.bmm_bf16(t, t, alpha=torch.tensor(2.0))
    # a non-finite alpha is a real number: it gets as far as the tensors
    for alpha in (float("inf"), float("nan"), 3):
        with pytest.raises(TypeError, match="a must be a 3-D tensor"):
            ops.bmm(t, t, alpha=alpha)


def test_bmm_dtype_rules_and_empty_products(ops):
    a = torch.zeros(2, 4, 6)
    b = torch.zeros(2, 6, 3)
    with pytest.raises(TypeError, match="bf16 operands"):
        ops.bmm(a, b)
    a8 = torch.zeros(2, 4, 6, dtype=torch.int8)
    with pytest.raises(TypeError, match="transposed"):
        ops.bmm(a8, a8.transpose(1, 2))
    # nothing to multiply: no kernel, so no GPU either
    z = ops.bmm(torch.zeros(2, 4, 0, dtype=BF), torch.zeros(2, 0, 3, dtype=BF))
    assert z.shape == (2, 4, 3) and z.dtype == torch.float32
    assert not bool(z.any())
    z = ops.bmm(torch.zeros(0, 4, 6, dtype=BF), torch.zeros(0, 6, 3, dtype=BF),
                out_dtype=torch.bfloat16)
    assert z.shape == (0, 4, 3) and z.dtype == BF
    # a CPU tensor is refused, not computed some other way
    with pytest.raises(TypeError, match="CUDA"):
        ops.bmm(a.to(BF), b.to(BF))


def test_strict_call_checks_without_a_gpu(ops):
    """everything up to the device test needs no GPU"""
    a = torch.zeros(2, 128, 64, dtype=BF)
    c = torch.zeros(2, 128, 128)
    with pytest.raises(ValueError, match="layout"):
        ops.gemm_bf16_batched(c, a, a, "xx")
    with pytest.raises(TypeError, match="bf16"):
        ops.gemm_bf16_batched(c, a.float(), a, "nt")
    with pytest.raises(TypeError, match="not built"):
        ops.gemm_bf16_batched(c, a.to(torch.int8), a.to(torch.int8), "nt")
    with pytest.raises(TypeError, match="fp32 or bf16"):
        ops.gemm_bf16_batched(c.double(), a, a, "nt")
    with pytest.raises(TypeError, match="alpha"):
        ops.gemm_bf16_batched(c, a, a, "nt", alpha=torch.tensor(1.0))
    with pytest.raises(TypeError, match="CUDA"):
        ops.gemm_bf16_batched(c, a, a, "nt")


# ---------------------------------------------------------------------------
# the existing paths do not reach the new native entry point
# ---------------------------------------------------------------------------

def test_existing_front_doors_do_not_reach_the_batched_entry(ops, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("new entry point reached")

    calls = []

    class Lib:
        def __getattr__(self, name):
            if name == "gemm_bf16_batched":
                return boom
            calls.append(name)
            raise RuntimeError(f"native {name}")    # the old path, no GPU

    monkeypatch.setattr(ops, "native", lambda: Lib())
    for name in ("gemm_bf16_batched", "bmm", "bmm_bf16"):
        monkeypatch.setattr(ops, name, boom)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))

    x = torch.zeros(128, 64, dtype=BF)
    w = torch.zeros(128, 64, dtype=BF)
    w2 = torch.zeros(128, 128, dtype=BF)
    runs = [
        lambda: ops.matmul(x, w.t()),
        lambda: ops.matmul(x.t(), torch.zeros(128, 128, dtype=BF)),
        lambda: ops.matmul(x, w.t(), out_dtype=torch.bfloat16),
        lambda: ops.matmul(x, w.t(), out_dtype=torch.bfloat16,
                           activation="relu"),
        lambda: ops.linear_bf16(x, w),
        lambda: ops.linear_bf16(x, w, fused=True),
        lambda: ops.mlp_bf16(x, w, None, w2, None),
    ]
    for run in runs:
        before = len(calls)
        with pytest.raises(RuntimeError, match="native "):
            run()
        assert len(calls) == before + 1     # it got to an existing kernel
    assert "gemm_bf16_batched" not in calls
    assert {"gemm_bf16_layout", "gemm_bf16_epilogue", "gemm_bf16_act"} \
        <= set(calls)

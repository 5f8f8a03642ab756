"""Host-only side of split-K for the nn/tn/tt layouts: ops.matmul and
ops.linear_bf16 judge split_k before they look at a tensor, matmul bounds
an int by the PADDED K, and the partition covers [0, T) for every (T, S)
tests/test_gpu_gemm_layout_splitk.py runs (a guard on that file's payload
choice; tests/test_gemm_splitk_logic.py tests the function). No GPU."""

import pytest
import torch

import gemm_layout_splitk_cases as cases
from hpc_patterns_amd import ops
from hpc_patterns_amd._native import native

BAD_SPLIT_K = [True, False, 2.0, "Auto", "8", "", [2], (1,), 1j]


def _views(layout, m, n, k):
    """logical a [M,K], b [K,N] on the CPU, stored as `layout` says"""
    a = torch.zeros(k, m, dtype=torch.bfloat16).t() if layout[0] == "t" \
        else torch.zeros(m, k, dtype=torch.bfloat16)
    b = torch.zeros(n, k, dtype=torch.bfloat16).t() if layout[1] == "t" \
        else torch.zeros(k, n, dtype=torch.bfloat16)
    assert ops.matmul_layout(a, b)[0] == layout
    return a, b


@pytest.mark.parametrize("bad", BAD_SPLIT_K, ids=repr)
def test_matmul_rejects_bad_split_k_first(bad):
    a, b = _views("tn", 128, 128, 64)
    with pytest.raises(ValueError, match="split_k"):
        ops.matmul(a, b, split_k=bad)
    # before the operands are looked at: these would be a TypeError
    with pytest.raises(ValueError, match="split_k"):
        ops.matmul(torch.zeros(2, 2, 2), None, split_k=bad)


@pytest.mark.parametrize("bad", BAD_SPLIT_K + [1, 3, 0, -1], ids=repr)
def test_linear_bf16_rejects_bad_split_k_first(bad):
    x = torch.zeros(128, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="split_k"):
        ops.linear_bf16(x, x, split_k=bad)
    with pytest.raises(ValueError, match="split_k"):   # else: a TypeError
        ops.linear_bf16(x.float(), None, split_k=bad)


def test_linear_bf16_still_judges_its_operands():
    x = torch.zeros(128, 64, dtype=torch.bfloat16)
    for sk in (None, "auto"):
        with pytest.raises(TypeError):
            ops.linear_bf16(x.float(), x.float(), split_k=sk)
        with pytest.raises(ValueError):
            ops.linear_bf16(x, x[:, :32], split_k=sk)


@pytest.mark.parametrize("layout", ["nn", "tn", "tt"])
def test_matmul_bounds_an_int_by_the_padded_k(layout):
    m, n, k = cases.FRONT_DOOR
    mp, np_, kp = ops.gemm_layout_pad_shapes(m, n, k)
    assert (mp, np_, kp) == (256, 256, 1024) and k // 64 < kp // 64
    a, b = _views(layout, m, n, k)
    for bad in (0, -1, kp // 64 + 1):
        with pytest.raises(ValueError, match="K_padded"):
            ops.matmul(a, b, split_k=bad)
    # K_padded / 64 itself (more than K // 64) passes the bound: the strict
    # call is reached and refuses the CPU tensors
    with pytest.raises(TypeError, match="CUDA"):
        ops.matmul(a, b, split_k=kp // 64)


def test_matmul_still_refuses_narrow_operands_with_split_k():
    a = torch.zeros(128, 64, dtype=torch.int8)
    b = torch.zeros(64, 128, dtype=torch.int8)
    with pytest.raises(TypeError, match="transposed"):
        ops.matmul(a, b, split_k=2)


def test_ktiles_cover_the_k_range_for_the_gpu_cases():
    hpk = native()
    pairs = cases.ts_pairs(
        lambda m, n, k: hpk.gemm_splitk_plan(m, n, k, cases.N_CU))
    assert (1, 1) in pairs and (5, 5) in pairs and (16, 4) in pairs
    for t, s in pairs:
        assert 1 <= s <= t, (t, s)
        nxt = 0
        for i in range(s):
            first, count = hpk.gemm_splitk_ktiles(t, s, i)
            assert first == nxt and count >= 1, (t, s, i)
            nxt = first + count
        assert nxt == t, (t, s)


def test_plans_the_gpu_cases_rely_on():
    hpk = native()
    plan = lambda m, n, k: hpk.gemm_splitk_plan(m, n, k, cases.N_CU)
    assert plan(*cases.PLAN_ONE) == 1
    assert plan(*cases.FRONT_DOOR) > 1
    tokens, n_out, n_in = cases.LINEAR
    assert plan(n_out, n_in, tokens) > 1        # dW splits

"""Host-only side of the split-K GEMM: gemm_splitk_ktiles (which K-tiles a
split walks; the function the kernel itself calls) and gemm_splitk_plan
(the automatic split count). No GPU. The plan tests assert properties of
the rule, not its two constants, which a new sweep may move."""

import pytest

from hpc_patterns_amd._native import native

T_VALUES = [1, 2, 5, 7, 64, 1023]

N_CU = [1, 2, 8, 104, 256, 304]
# (M, N): 1, 2, 4, 6, 15, 64, 256 and 1024 tiles of 128^2
MN = [(128, 128), (128, 256), (256, 256), (384, 256), (384, 640),
      (1024, 1024), (2048, 2048), (4096, 4096)]
K_VALUES = [64, 128, 192, 256, 512, 1024, 4096, 8192, 65536, 1 << 20]


def _split_counts(t):
    return sorted({s for s in (1, 2, 3, 5, t) if s <= t})


@pytest.mark.parametrize("t", T_VALUES)
def test_ktiles_tile_the_k_range_in_order(t):
    hpk = native()
    for splits in _split_counts(t):
        ranges = [hpk.gemm_splitk_ktiles(t, splits, s) for s in range(splits)]
        owner = [0] * t
        nxt = 0
        for first, count in ranges:
            assert first == nxt, (t, splits, ranges)  # in order, no gap
            assert count >= 1, (t, splits, ranges)    # none is empty
            for tile in range(first, first + count):
                owner[tile] += 1
            nxt = first + count
        assert nxt == t and owner == [1] * t, (t, splits, ranges)
        counts = [c for _, c in ranges]
        assert max(counts) - min(counts) <= 1, (t, splits, counts)
        assert counts == sorted(counts, reverse=True), (t, splits, counts)
        # the rule as the contract words it
        for s, (first, count) in enumerate(ranges):
            assert count == t // splits + (s < t % splits)
            assert first == s * (t // splits) + min(s, t % splits)


def test_ktiles_rejects_what_the_launchers_reject():
    hpk = native()
    for t, splits, s in [(4, 0, 0), (4, 5, 0), (4, 2, 2), (4, 2, -1),
                         (0, 1, 0)]:
        with pytest.raises(ValueError):
            hpk.gemm_splitk_ktiles(t, splits, s)


def _tiles(m, n):
    return -(-m // 128) * -(-n // 128)


def test_plan_constants_are_sane():
    hpk = native()
    assert hpk.SPLITK_MIN_TILES >= 1
    assert hpk.SPLITK_MAX_SPLITS >= 1


@pytest.mark.parametrize("n_cu", N_CU)
def test_plan_bounds(n_cu):
    hpk = native()
    for m, n in MN:
        for k in K_VALUES:
            plan = hpk.gemm_splitk_plan(m, n, k, n_cu)
            where = (m, n, k, n_cu, plan)
            assert 1 <= plan <= k // 64, where
            assert plan <= hpk.SPLITK_MAX_SPLITS, where
            if _tiles(m, n) >= n_cu:
                assert plan == 1, where
            if plan > 1:
                assert plan * _tiles(m, n) <= n_cu, where
                # every split keeps the minimum of K-tiles
                assert (k // 64) // plan >= hpk.SPLITK_MIN_TILES, where


def test_plan_one_compute_unit_never_splits():
    hpk = native()
    for m, n in MN:
        for k in K_VALUES:
            assert hpk.gemm_splitk_plan(m, n, k, 1) == 1


@pytest.mark.parametrize("n_cu", N_CU)
def test_plan_is_monotonic(n_cu):
    hpk = native()
    for m, n in MN:  # non-decreasing in K at fixed M, N
        plans = [hpk.gemm_splitk_plan(m, n, k, n_cu) for k in K_VALUES]
        assert plans == sorted(plans), (m, n, n_cu, plans)
    by_tiles = sorted(MN, key=lambda mn: _tiles(*mn))
    for k in K_VALUES:  # non-increasing in tiles at fixed K
        plans = [hpk.gemm_splitk_plan(m, n, k, n_cu) for m, n in by_tiles]
        assert plans == sorted(plans, reverse=True), (k, n_cu, plans)


def test_plan_splits_a_skinny_problem_on_a_big_device():
    """One tile and a long K on 256 compute units: the rule must answer
    more than 1 whatever its constants are, short of forbidding splits."""
    hpk = native()
    if hpk.SPLITK_MAX_SPLITS > 1:
        k = 64 * 2 * hpk.SPLITK_MIN_TILES
        assert hpk.gemm_splitk_plan(128, 128, k, 256) == 2
        assert hpk.gemm_splitk_plan(128, 128, 1 << 24, 256) == \
            min(256, hpk.SPLITK_MAX_SPLITS)


@pytest.mark.parametrize("n_cu", [8, 256])
def test_plan_rounds_unaligned_shapes_up(n_cu):
    hpk = native()
    up = lambda x, q: -(-x // q) * q
    for m, n, k in [(100, 200, 1000), (1, 1, 1), (129, 128, 65), (128, 127, 64),
                    (300, 300, 70000), (257, 1, 8191), (128, 128, 4096)]:
        assert hpk.gemm_splitk_plan(m, n, k, n_cu) == \
            hpk.gemm_splitk_plan(up(m, 128), up(n, 128), up(k, 64), n_cu), \
            (m, n, k)


def test_ops_plan_wrapper_passes_n_cu_through():
    from hpc_patterns_amd import ops

    hpk = native()
    for m, n, k in [(128, 128, 65536), (100, 200, 1000), (4096, 4096, 128)]:
        assert ops.gemm_splitk_plan(m, n, k, n_cu=256) == \
            hpk.gemm_splitk_plan(m, n, k, 256)

"""Shapes and split counts of tests/test_gpu_gemm_layout_splitk.py, shared
with tests/test_gemm_layout_splitk_logic.py, which guards on the CPU that
the partition covers [0, T) for every (T, S) the GPU file runs. No torch,
no GPU."""

# (M, N, K, S): a single trip straight into C; T = 5 with uneven partitions
# and one-tile splits; four tiles per split (buffer swap, steady state)
BITWISE = [(128, 128, 64, 1), (128, 128, 320, 2), (128, 128, 320, 3),
           (128, 128, 320, 5), (128, 128, 1024, 4)]
RAGGED_GRID = (384, 640, 192)       # 15 tiles, T = 3
RAGGED_SPLITS = (2, 3)
ROW_START = (128, 256, 320, 3)      # M != N != K; splits of 2, 2, 1 tiles
GRID_STRIDE = (1152, 1024, 128, 2)  # M*N/4 vectors > 1024 * 256 threads
PARENTS = (256, 256, 1024)          # randn against gemm_splitk / _layout
PARENT_SPLITS = (1, 3, 4)
WORKSPACE = (128, 128, 320)         # S = 3 oversized, S = 5 reused
SIDE_STREAM = (128, 128, 1024, 4)
REPEATS = 10
SPECIALS = (128, 128, 320, 3)
FRONT_DOOR = (200, 136, 1000)       # logical; pads to (256, 256, 1024)
FRONT_DOOR_SPLITS = 3
PLAN_ONE = (200, 136, 300)          # T = 5 < kSplitKMinTiles: plan 1
LINEAR = (2048, 128, 128)           # tokens, out features, in features
N_CU = 256                          # MI355X; what "auto" plans for there


def ts_pairs(plan):
    """Every (T, S) above; plan(m, n, k) answers for the "auto" cases."""
    pairs = {(k // 64, s) for _, _, k, s in BITWISE}
    pairs |= {(RAGGED_GRID[2] // 64, s) for s in RAGGED_SPLITS}
    pairs |= {(k // 64, s) for _, _, k, s in (ROW_START, GRID_STRIDE,
                                              SIDE_STREAM, SPECIALS)}
    pairs |= {(PARENTS[2] // 64, s) for s in PARENT_SPLITS}
    pairs |= {(WORKSPACE[2] // 64, 3), (WORKSPACE[2] // 64, 5)}
    kp = -(-FRONT_DOOR[2] // 64) * 64
    pairs |= {(kp // 64, FRONT_DOOR_SPLITS), (kp // 64, plan(*FRONT_DOOR))}
    tokens, n_out, n_in = LINEAR
    pairs.add((tokens // 64, plan(n_out, n_in, tokens)))    # dW: tn
    return sorted(pairs)

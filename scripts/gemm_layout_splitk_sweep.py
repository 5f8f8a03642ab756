#!/usr/bin/env python3
"""gemm_layout_splitk_sweep.py — what split-K buys the nn/tn/tt layout
kernels on the dW product of a linear layer, dW[N,K] = dy[M,N]^T @ x[M,K]
(layout tn on the tensors as stored, output N x K, sum over M tokens), and
whether gemm_splitk_plan's constants (kSplitKMinTiles, kSplitKMaxSplits in
native/include/hpk.h, from the NT sweep) suit them.

Method of scripts/gemm_splitk_sweep.py (docs/benchmarking.md): every row of
a shape is measured in INTERLEAVED rounds with the best kept per row, and
the sweep is bracketed by a fixed hipBLASLt control whose start/end delta is
the drift nothing tighter can be told apart from.

Per shape:
  (p)  ops.matmul(dy.t(), x)                      the path without a split
  (q)  dy.t().contiguous(), x.t().contiguous(), then
       ops.matmul_nt(..., split_k="auto")         both copies counted
  (r)  ops.matmul(dy.t(), x, split_k="auto")
  S=n  ops.gemm_bf16_layout_splitk with a caller workspace
One nn row (a dx-like product with a small output) rides along. Before
timing, (r) is asserted torch.equal to (q) where the plan splits (same
partition, same orders) and to (p) where it does not.

Usage (GPU box):  python scripts/gemm_layout_splitk_sweep.py [--rounds 3]
                      [--out profiles/gemm_layout_splitk_table.md]
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

# (layout, out rows, out cols, sum length): tn rows are dW[N,K] over M tokens
SHAPES = [("tn", 256, 256, 16384), ("tn", 256, 256, 65536),
          ("tn", 512, 512, 16384), ("tn", 512, 512, 65536),
          ("tn", 1024, 1024, 16384), ("tn", 4096, 4096, 4096),
          ("nn", 256, 256, 32768)]
SPLITS = [1, 2, 4, 8, 16, 32, 64, 128]
MAX_WORKSPACE_BYTES = 1 << 31


def time_gpu(fn, inner, reps=4, warm=1):
    """Best time of one call, in us: batches of `inner` calls between two
    device events."""
    import torch

    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(inner):
            fn()
        t1.record()
        t1.synchronize()
        best = min(best, t0.elapsed_time(t1) * 1e3 / inner)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()

    import torch

    from hpc_patterns_amd import ops
    from hpc_patterns_amd._native import native

    if not torch.cuda.is_available():
        sys.exit("gemm_layout_splitk_sweep.py needs a GPU")
    dev = torch.device("cuda", 0)
    hpk = native()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lines = []

    def emit(text=""):
        print(text, flush=True)
        lines.append(text)

    def rand(rows, cols):
        return (torch.rand(rows, cols, device=dev) * 2 - 1).to(torch.bfloat16)

    ca, cb = rand(4096, 4096), rand(4096, 4096)

    def control():
        return time_gpu(lambda: torch.matmul(ca, cb.t()), inner=10, reps=6,
                        warm=3)

    emit(f"device: {torch.cuda.get_device_name(0)}, {n_cu} CUs; "
         f"kSplitKMinTiles = {hpk.SPLITK_MIN_TILES}, "
         f"kSplitKMaxSplits = {hpk.SPLITK_MAX_SPLITS}; rounds = "
         f"{args.rounds}, inner = {args.inner}")
    c_start = control()
    emit(f"hipBLASLt bf16 4096^3 control (start): {c_start:8.1f} us")
    emit()

    results = {}
    for shape in SHAPES:
        layout, m, n, k = shape
        # logical a [m,k] @ b [k,n]; tn stores a as [k,m] (dy), nn as [m,k]
        a_st = rand(k, m) if layout[0] == "t" else rand(m, k)
        b_st = rand(k, n)
        a = a_st.t() if layout[0] == "t" else a_st
        b = b_st
        assert ops.matmul_layout(a, b)[0] == layout

        def path_q():
            a_nt = a_st.t().contiguous() if layout[0] == "t" else a_st
            return ops.matmul_nt(a_nt, b_st.t().contiguous(), split_k="auto")

        # a plan above 1 puts (q) on gemm_splitk: the same bits. A plan of
        # 1 puts it on a 256^2 kernel with another order; there (r) is (p)
        got_r = ops.matmul(a, b, split_k="auto")
        same = path_q() if ops.gemm_splitk_plan(m, n, k) > 1 \
            else ops.matmul(a, b)
        torch.cuda.synchronize()
        assert torch.equal(got_r, same), f"{shape}: (r) differs"
        del got_r, same

        c = torch.empty(m, n, device=dev)
        legal = [s for s in SPLITS
                 if s <= k // 64 and s * m * n * 4 <= MAX_WORKSPACE_BYTES]
        ws = torch.empty(max(legal) * m * n, device=dev)
        rows = {"(p)": lambda: ops.matmul(a, b),
                "(q)": path_q,
                "(r)": lambda: ops.matmul(a, b, split_k="auto")}
        for s in legal:
            rows[f"S={s}"] = lambda s=s: ops.gemm_bf16_layout_splitk(
                c, a_st, b_st, layout, s, workspace=ws)
        best = {name: float("inf") for name in rows}
        for _ in range(args.rounds):
            for name, fn in rows.items():
                best[name] = min(best[name], time_gpu(fn, args.inner))
        best["plan"] = ops.gemm_splitk_plan(m, n, k)
        results[shape] = best
        print(f"# {shape} done", flush=True)
        del a, b, a_st, b_st, c, ws
        torch.cuda.empty_cache()

    c_end = control()
    delta = abs(c_end - c_start) / c_start
    cols = ["(p)", "(q)", "(r)"] + [f"S={s}" for s in SPLITS]
    emit(f"### us per call, best of {args.rounds} interleaved rounds")
    emit()
    emit("| layout, out x sum | " + " | ".join(cols) +
         " | plan | (r)/(p) | (r)/(q) |")
    emit("|---|" + "---:|" * (len(cols) + 3))
    for shape in SHAPES:
        layout, m, n, k = shape
        r = results[shape]
        cells = [f"{r[c]:.1f}" if c in r else "-" for c in cols]
        emit(f"| {layout} {m} x {n} x {k} | " + " | ".join(cells) +
             f" | {r['plan']} | {r['(r)'] / r['(p)']:.3f} | "
             f"{r['(r)'] / r['(q)']:.3f} |")
    emit()
    emit(f"hipBLASLt bf16 4096^3 control (end)  : {c_end:8.1f} us")
    emit(f"control delta (|end - start| / start): {delta:.3f}")
    emit()

    bad = [f"{shape}: (r) is {r['(r)'] / r['(p)']:.3f}x (p)"
           for shape, r in results.items()
           if r["(r)"] > r["(p)"] * (1 + delta)]
    emit("acceptance ((r) <= (p) + delta at every shape): " +
         ("PASS" if not bad else "FAIL — " + "; ".join(bad)))
    emit()

    # what the plan's split count leaves on the table: the best S column
    emit("### the plan's S against the best timed S")
    emit()
    emit("| layout, out x sum | plan | S=plan | best S | best | plan/best |")
    emit("|---|---:|---:|---:|---:|---:|")
    for shape in SHAPES:
        layout, m, n, k = shape
        r = results[shape]
        timed = {s: r[f"S={s}"] for s in SPLITS if f"S={s}" in r}
        s_best = min(timed, key=timed.get)
        at_plan = timed.get(r["plan"])
        emit(f"| {layout} {m} x {n} x {k} | {r['plan']} | " +
             (f"{at_plan:.1f}" if at_plan is not None else "-") +
             f" | {s_best} | {timed[s_best]:.1f} | " +
             (f"{at_plan / timed[s_best]:.3f}" if at_plan is not None
              else "-") + " |")

    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

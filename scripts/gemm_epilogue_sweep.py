#!/usr/bin/env python3
"""gemm_epilogue_sweep.py — what the bf16-output epilogue with bias
(native/gemm_epilogue.hip) buys over the composition it replaces, per
layout, and what colsum_bf16 costs next to a torch column sum.

Method of scripts/gemm_layout_splitk_sweep.py (docs/benchmarking.md): every
row of a shape is measured in INTERLEAVED rounds with the best kept per row,
and the sweep is bracketed by a fixed hipBLASLt control whose start/end
delta is the drift nothing tighter can be told apart from.

Per layout and shape, y = bf16(a @ b + bias):
  (f)   ops.matmul(a, b, out_dtype=bf16, bias=bias, split_k="auto")
        the fused call
  (u)   the same 128^2 kernel into fp32 (gemm_bf16 under HPK_GEMM_VARIANT=db
        for nt, gemm_bf16_layout else; the split-K kernels where the plan
        splits), then torch add and cast: the composition the fusion replaces
  (u8)  nt only: default ops.matmul_nt (the 256^2 8-phase kernel where the
        shape allows) plus add and cast
Before timing, (f) is asserted torch.equal to (u).

colsum_bf16(dy) is timed against dy.float().sum(0) and against the K2 copy
kernel moving the bytes it reads.

Usage (GPU box):  python scripts/gemm_epilogue_sweep.py [--rounds 3]
                      [--out profiles/gemm_epilogue_table.md]
"""

from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

LAYOUTS = ["nt", "nn", "tn", "tt"]
# (M, N, K) logical: the cubes, then the dW shapes of the split-K table
# (tn: out rows, out cols, tokens)
CUBES = [(1024, 1024, 1024), (4096, 4096, 4096), (8192, 8192, 8192)]
DW = [(256, 256, 16384), (256, 256, 65536), (512, 512, 16384),
      (512, 512, 65536), (1024, 1024, 16384), (4096, 4096, 4096)]
COLSUM = [(4096, 1024), (16384, 4096), (65536, 256), (8192, 8192)]


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
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()

    import torch

    from hpc_patterns_amd import ops

    if not torch.cuda.is_available():
        sys.exit("gemm_epilogue_sweep.py needs a GPU")
    dev = torch.device("cuda", 0)
    bf16 = torch.bfloat16
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lines = []

    def emit(text=""):
        print(text, flush=True)
        lines.append(text)

    def rand(rows, cols):
        return (torch.rand(rows, cols, device=dev) * 2 - 1).to(bf16)

    ca, cb = rand(4096, 4096), rand(4096, 4096)

    def control():
        return time_gpu(lambda: torch.matmul(ca, cb.t()), inner=10, reps=6,
                        warm=3)

    emit(f"device: {torch.cuda.get_device_name(0)}, {n_cu} CUs; rounds = "
         f"{args.rounds}, inner = {args.inner}")
    c_start = control()
    emit(f"hipBLASLt bf16 4096^3 control (start): {c_start:8.1f} us")
    emit()

    def db_gemm(c, a_st, b_st):
        os.environ["HPK_GEMM_VARIANT"] = "db"
        try:
            ops.gemm_bf16(c, a_st, b_st)
        finally:
            del os.environ["HPK_GEMM_VARIANT"]

    results = {}
    jobs = [(lay, s) for s in CUBES for lay in LAYOUTS] + \
           [("tn", s) for s in DW]
    for layout, (m, n, k) in jobs:
        a_st = rand(k, m) if layout[0] == "t" else rand(m, k)
        b_st = rand(k, n) if layout[1] == "n" else rand(n, k)
        a = a_st.t() if layout[0] == "t" else a_st
        b = b_st if layout[1] == "n" else b_st.t()
        assert ops.matmul_layout(a, b)[0] == layout
        bias = torch.arange(n, device=dev, dtype=torch.float32) * 0.01 - 1.0
        plan = ops.gemm_splitk_plan(m, n, k)
        c32 = torch.empty(m, n, device=dev)
        ws = torch.empty(plan * m * n, device=dev) if plan > 1 else None

        def path_f():
            return ops.matmul(a, b, out_dtype=bf16, bias=bias, split_k="auto")

        def path_u():
            if plan > 1:
                ops.gemm_bf16_layout_splitk(c32, a_st, b_st, layout, plan,
                                            workspace=ws)
            elif layout == "nt":
                db_gemm(c32, a_st, b_st)
            else:
                ops.gemm_bf16_layout(c32, a_st, b_st, layout)
            return (c32 + bias).to(bf16)

        def path_u8():
            return (ops.matmul_nt(a_st, b_st) + bias).to(bf16)

        got, want = path_f(), path_u()
        torch.cuda.synchronize()
        assert torch.equal(got, want), f"{layout} {(m, n, k)}: (f) != (u)"
        del got, want
        rows = {"(f)": path_f, "(u)": path_u}
        if layout == "nt":
            rows["(u8)"] = path_u8
        inner = args.inner if m * n * k < 2 ** 36 else max(2, args.inner // 3)
        best = {name: float("inf") for name in rows}
        for _ in range(args.rounds):
            for name, fn in rows.items():
                best[name] = min(best[name], time_gpu(fn, inner))
        best["plan"] = plan
        results[(layout, m, n, k)] = best
        print(f"# {layout} {(m, n, k)} done", flush=True)
        del a, b, a_st, b_st, c32, ws
        torch.cuda.empty_cache()

    colsum = {}
    for m, n in COLSUM:
        dy = rand(m, n)
        dst = torch.empty_like(dy)
        got = ops.colsum_bf16(dy)
        ref = dy.double().sum(0)
        bound = (m - 1) * 2.0 ** -24 * dy.double().abs().sum(0)
        assert bool(((got.double() - ref).abs() <= bound).all()), (m, n)
        rows = {"colsum_bf16": lambda: ops.colsum_bf16(dy),
                "torch": lambda: dy.float().sum(0),
                "K2 copy": lambda: ops.copy_kernel(dst, dy)}
        best = {name: float("inf") for name in rows}
        for _ in range(args.rounds):
            for name, fn in rows.items():
                best[name] = min(best[name], time_gpu(fn, args.inner))
        best["R"] = ops.colsum_plan(m, n)
        colsum[(m, n)] = best
        del dy, dst
        torch.cuda.empty_cache()

    c_end = control()
    delta = abs(c_end - c_start) / c_start
    emit(f"### bf16(a @ b + bias), us per call, best of {args.rounds} "
         f"interleaved rounds")
    emit()
    emit("| layout | M x N x K | plan | (f) | (u) | (u8) | (f)/(u) | "
         "(f)/(u8) |")
    emit("|---|---|---:|---:|---:|---:|---:|---:|")
    for (layout, m, n, k), r in results.items():
        u8 = r.get("(u8)")
        emit(f"| {layout} | {m} x {n} x {k} | {r['plan']} | {r['(f)']:.1f} | "
             f"{r['(u)']:.1f} | " + (f"{u8:.1f}" if u8 else "-") +
             f" | {r['(f)'] / r['(u)']:.3f} | " +
             (f"{r['(f)'] / u8:.3f}" if u8 else "-") + " |")
    emit()
    emit("### colsum_bf16(dy), us per call")
    emit()
    emit("| M x N | R | colsum_bf16 | dy.float().sum(0) | K2 copy of the "
         "same bytes | read rate, TB/s |")
    emit("|---|---:|---:|---:|---:|---:|")
    for (m, n), r in colsum.items():
        emit(f"| {m} x {n} | {r['R']} | {r['colsum_bf16']:.1f} | "
             f"{r['torch']:.1f} | {r['K2 copy']:.1f} | "
             f"{m * n * 2 / r['colsum_bf16'] / 1e6:.2f} |")
    emit()
    emit(f"hipBLASLt bf16 4096^3 control (end)  : {c_end:8.1f} us")
    emit(f"control delta (|end - start| / start): {delta:.3f}")
    emit()
    bad = [f"{key}: (f) is {r['(f)'] / r['(u)']:.3f}x (u)"
           for key, r in results.items()
           if r["(f)"] >= r["(u)"] * (1 - delta)]
    emit("expectation ((f) ahead of (u) by more than the control delta at "
         "every row): " + ("MET" if not bad else "NOT MET — " + "; ".join(bad)))

    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

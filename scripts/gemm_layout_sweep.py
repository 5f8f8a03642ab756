#!/usr/bin/env python3
"""gemm_layout_sweep.py — the nn/tn/tt bf16 kernels (native/gemm_layout.hip)
against what the NT family offers for the same stored tensors.

Method of scripts/gemm_splitk_sweep.py (docs/benchmarking.md): the rows of
a (layout, shape) are measured in INTERLEAVED rounds with the best kept per
row, and the whole sweep is bracketed by a fixed hipBLASLt control whose
start/end delta is the drift nothing tighter can be told apart from.

Rows, per layout at 1024^3, 4096^3 and 8192^3:
  lay   ops.gemm_bf16_layout on the tensors as stored
  (a)   t().contiguous() of every operand that is not K-contiguous, then
        ops.gemm_bf16 under HPK_GEMM_VARIANT=db (the 128^2 double-buffered
        kernel, the same structure); copies included
  (b)   the same with the default kernel (256^2 8-phase); copies included
  (c)   ops.gemm_bf16 db on operands transposed beforehand: kernel only
  (c8)  ops.gemm_bf16 default on the same: kernel only, for information
lay/(c) judges the design (same DMAs, same MFMAs); lay/(a) and lay/(b) are
what a user compares.

Usage (GPU box):  python scripts/gemm_layout_sweep.py [--rounds 3]
                      [--out profiles/gemm_layout_table.md]
"""

from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SIZES = [1024, 4096, 8192]
LAYOUTS = ["nn", "tn", "tt"]
ROWS = ["lay", "(a)", "(b)", "(c)", "(c8)"]


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


def set_variant(value):
    # the launcher reads the variable at every call
    if value is None:
        os.environ.pop("HPK_GEMM_VARIANT", None)
    else:
        os.environ["HPK_GEMM_VARIANT"] = value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=0,
                    help="calls per sample; 0 = 50 / 20 / 10 by size")
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--out", default=None, help="also write the tables here")
    args = ap.parse_args()

    import torch

    from hpc_patterns_amd import ops
    from hpc_patterns_amd._native import native

    if not torch.cuda.is_available():
        sys.exit("gemm_layout_sweep.py needs a GPU")
    dev = torch.device("cuda", 0)
    hpk = native()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    sizes = [int(s) for s in args.sizes.split(",")]
    lines = []

    def emit(text=""):
        print(text, flush=True)
        lines.append(text)

    ca = (torch.rand(4096, 4096, device=dev) * 2 - 1).to(torch.bfloat16)
    cb = (torch.rand(4096, 4096, device=dev) * 2 - 1).to(torch.bfloat16)

    def control():
        return time_gpu(lambda: torch.matmul(ca, cb.t()), inner=10, reps=6,
                        warm=3)

    emit(f"device: {torch.cuda.get_device_name(0)}, {n_cu} CUs; rounds = "
         f"{args.rounds}")
    c_start = control()
    emit(f"hipBLASLt bf16 4096^3 control (start): {c_start:8.1f} us")
    emit()

    results = {}  # (layout, size) -> {row: us}
    for s in sizes:
        inner = args.inner or (50 if s <= 1024 else 20 if s <= 4096 else 10)
        m = n = k = s
        set_variant("db")
        assert hpk.gemm_variant("bf16", m, n, k) == "bf16_db8"
        set_variant(None)
        for layout in LAYOUTS:
            a_t, b_n = layout[0] == "t", layout[1] == "n"
            # as stored
            a = (torch.rand((k, m) if a_t else (m, k), device=dev) * 2 - 1) \
                .to(torch.bfloat16)
            b = (torch.rand((k, n) if b_n else (n, k), device=dev) * 2 - 1) \
                .to(torch.bfloat16)
            # transposed beforehand, for (c)
            a_nt = a.t().contiguous() if a_t else a
            b_nt = b.t().contiguous() if b_n else b
            c = torch.empty(m, n, device=dev)

            def copy_then_nt():
                ops.gemm_bf16(c, a.t().contiguous() if a_t else a,
                              b.t().contiguous() if b_n else b)

            rows = {
                "lay": (None, lambda: ops.gemm_bf16_layout(c, a, b, layout)),
                "(a)": ("db", copy_then_nt),
                "(b)": (None, copy_then_nt),
                "(c)": ("db", lambda: ops.gemm_bf16(c, a_nt, b_nt)),
                "(c8)": (None, lambda: ops.gemm_bf16(c, a_nt, b_nt)),
            }
            # the sweep measures what the tests prove equal
            set_variant("db")
            ops.gemm_bf16(c, a_nt, b_nt)
            set_variant(None)
            c_lay = torch.empty_like(c)
            ops.gemm_bf16_layout(c_lay, a, b, layout)
            torch.cuda.synchronize()
            assert torch.equal(c, c_lay), f"{layout} {s}: not bf16_db8's bits"
            del c_lay

            best = {name: float("inf") for name in rows}
            for _ in range(args.rounds):
                for name, (variant, fn) in rows.items():
                    set_variant(variant)
                    best[name] = min(best[name], time_gpu(fn, inner))
                    set_variant(None)
            results[(layout, s)] = best
            print(f"# {layout} {s}^3 done", flush=True)
            del a, b, a_nt, b_nt, c
            torch.cuda.empty_cache()

    c_end = control()
    delta = abs(c_end - c_start) / c_start

    emit(f"### us per call (TFLOP/s), best of {args.rounds} interleaved "
         f"rounds")
    emit()
    emit("| layout | M=N=K | " + " | ".join(ROWS) +
         " | lay/(a) | lay/(b) | lay/(c) |")
    emit("|---|---:|" + "---:|" * (len(ROWS) + 3))
    for s in sizes:
        flop = 2.0 * s * s * s
        for layout in LAYOUTS:
            r = results[(layout, s)]
            cells = [f"{r[x]:.1f} ({flop / r[x] * 1e-6:.0f})" for x in ROWS]
            emit(f"| {layout} | {s} | " + " | ".join(cells) +
                 f" | {r['lay'] / r['(a)']:.3f} | {r['lay'] / r['(b)']:.3f}"
                 f" | {r['lay'] / r['(c)']:.3f} |")
    emit()
    emit(f"hipBLASLt bf16 4096^3 control (end)  : {c_end:8.1f} us")
    emit(f"control delta (|end - start| / start): {delta:.3f}")

    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

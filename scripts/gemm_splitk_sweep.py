#!/usr/bin/env python3
"""gemm_splitk_sweep.py — where split-K pays, and the sweep behind the two
constants of gemm_splitk_plan (kSplitKMinTiles, kSplitKMaxSplits in
native/include/hpk.h).

Method of scripts/gemm_libcmp.py (findings.md #21): every variant of a
(shape, kind) is measured in INTERLEAVED rounds with the best kept per
variant, and the whole sweep is bracketed by a fixed hipBLASLt control whose
start/end delta is the drift nothing tighter can be told apart from.

Three short-K shapes ride along for kSplitKMinTiles; the acceptance rule
looks at the six long ones. Per shape and kind: ops.gemm_<kind> (the non-split path), gemm_splitk at
S in {1, 2, 4, ..., 128} where legal, matmul_nt(split_k="auto"), and the
vendor library for information. One timed sample is a batch of --inner
calls between two device events; the figure is the best batch / inner.

Usage (GPU box):  python scripts/gemm_splitk_sweep.py [--rounds 3]
                      [--out profiles/gemm_splitk_table.md]
"""

from __future__ import annotations

import argparse
import math
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SHAPES = [(128, 128, 65536), (256, 256, 65536), (512, 512, 32768),
          (1024, 1024, 16384), (2048, 2048, 8192), (4096, 4096, 4096)]
SKINNY = SHAPES[:3]  # where auto has to win by more than the drift
# short-K problems, for kSplitKMinTiles only: here T / S reaches 1, which it
# never does above. Timed and tabulated like the rest, outside the acceptance.
SHORT_K = [(128, 128, 4096), (128, 128, 8192), (256, 256, 8192)]
KINDS = ["bf16", "fp8", "i8"]
SPLITS = [1, 2, 4, 8, 16, 32, 64, 128]


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


def operands(kind, m, n, k, dev):
    import torch

    if kind == "i8":
        return (torch.randint(-128, 128, (m, k), dtype=torch.int8, device=dev),
                torch.randint(-128, 128, (n, k), dtype=torch.int8, device=dev),
                torch.int32)
    a = (torch.rand(m, k, device=dev) * 2 - 1).to(torch.bfloat16)
    b = (torch.rand(n, k, device=dev) * 2 - 1).to(torch.bfloat16)
    if kind == "fp8":
        a, b = a.to(torch.float8_e4m3fn), b.to(torch.float8_e4m3fn)
    return a, b, torch.float32


def library_call(kind, a, b):
    """The vendor library on the same operands, or None."""
    import torch

    if kind == "bf16":
        return lambda: torch.matmul(a, b.t())
    try:
        if kind == "fp8":
            one = torch.ones((), device=a.device)
            fn = lambda: torch._scaled_mm(a, b.t(), scale_a=one, scale_b=one,
                                          out_dtype=torch.bfloat16)
        else:
            fn = lambda: torch._int_mm(a, b.t())
        fn()
        torch.cuda.synchronize()
        return fn
    except Exception as exc:  # not every build has every entry point
        print(f"# no library {kind} path: {type(exc).__name__}", flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--out", default=None, help="also write the tables here")
    args = ap.parse_args()

    import torch

    from hpc_patterns_amd import ops
    from hpc_patterns_amd._native import native

    if not torch.cuda.is_available():
        sys.exit("gemm_splitk_sweep.py needs a GPU")
    dev = torch.device("cuda", 0)
    hpk = native()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lines = []

    def emit(text=""):
        print(text, flush=True)
        lines.append(text)

    ca = (torch.rand(4096, 4096, device=dev) * 2 - 1).to(torch.bfloat16)
    cb = (torch.rand(4096, 4096, device=dev) * 2 - 1).to(torch.bfloat16)

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

    gemm = {"bf16": ops.gemm_bf16, "fp8": ops.gemm_fp8, "i8": ops.gemm_i8}
    results = {}  # (kind, shape) -> {variant: us}
    for kind in args.kinds.split(","):
        for m, n, k in SHAPES + SHORT_K:
            a, b, out_dtype = operands(kind, m, n, k, dev)
            c = torch.empty(m, n, dtype=out_dtype, device=dev)
            legal = [s for s in SPLITS if s <= k // 64]
            ws = torch.empty(max(legal) * m * n, dtype=out_dtype, device=dev)
            variants = {"nosplit": lambda: gemm[kind](c, a, b)}
            for s in legal:
                variants[f"S={s}"] = \
                    lambda s=s: ops.gemm_splitk(c, a, b, s, workspace=ws)
            variants["auto"] = lambda: ops.matmul_nt(a, b, split_k="auto")
            lib = library_call(kind, a, b)
            if lib is not None:
                variants["library"] = lib
            best = {name: float("inf") for name in variants}
            for _ in range(args.rounds):
                for name, fn in variants.items():
                    best[name] = min(best[name], time_gpu(fn, args.inner))
            best["plan"] = ops.gemm_splitk_plan(m, n, k)
            results[(kind, (m, n, k))] = best
            print(f"# {kind} {m}x{n}x{k} done", flush=True)
            del a, b, c, ws
            torch.cuda.empty_cache()

    c_end = control()
    delta = abs(c_end - c_start) / c_start
    cols = ["nosplit"] + [f"S={s}" for s in SPLITS] + ["auto", "library"]
    for kind in args.kinds.split(","):
        emit(f"### {kind} — us per call, best of {args.rounds} interleaved "
             f"rounds")
        emit()
        emit("| M x N x K | " + " | ".join(cols) + " | plan | auto/nosplit |")
        emit("|---|" + "---:|" * (len(cols) + 2))
        for shape in SHAPES + SHORT_K:
            r = results[(kind, shape)]
            cells = [f"{r[c]:.1f}" if c in r else "-" for c in cols]
            emit(f"| {shape[0]} x {shape[1]} x {shape[2]} | " +
                 " | ".join(cells) +
                 f" | {r['plan']} | {r['auto'] / r['nosplit']:.3f} |")
        emit()
    emit(f"hipBLASLt bf16 4096^3 control (end)  : {c_end:8.1f} us")
    emit(f"control delta (|end - start| / start): {delta:.3f}")
    emit()

    # the acceptance rule of the constants, on this table
    bad = []
    for (kind, shape), r in results.items():
        if shape in SHORT_K:
            continue
        ratio = r["auto"] / r["nosplit"]
        if ratio > 1 + delta:
            bad.append(f"{kind} {shape}: auto is {ratio:.3f}x the non-split "
                       f"path")
        if shape in SKINNY and ratio >= 1 - delta:
            bad.append(f"{kind} {shape}: auto gains only "
                       f"{(1 - ratio) * 100:.1f}%, within the drift")
    emit("acceptance (auto <= nosplit + delta everywhere, beats it by more "
         "than delta at the three skinniest shapes): " +
         ("PASS" if not bad else "FAIL — " + "; ".join(bad)))
    emit()

    # what other constants would have chosen, read off the same table
    emit("### what the plan rule picks under other constants (worst and "
         "geometric-mean auto/nosplit over all shapes and kinds, from the "
         "S columns)")
    emit()
    emit("| kSplitKMinTiles | kSplitKMaxSplits | worst | geomean |")
    emit("|---:|---:|---:|---:|")
    for min_tiles in (1, 2, 4, 8, 16, 32):
        for max_splits in (8, 16, 32, 64, 128):
            worst, logsum, cnt = 0.0, 0.0, 0
            for (kind, (m, n, k)), r in results.items():
                tiles, t = (m // 128) * (n // 128), k // 64
                s = 1
                if tiles < n_cu:
                    s = max(1, min(n_cu // tiles, t // min_tiles, max_splits))
                key = "nosplit" if s == 1 else f"S={s}"
                if key not in r:  # a count the sweep did not time
                    continue
                ratio = r[key] / r["nosplit"]
                worst = max(worst, ratio)
                logsum += math.log(ratio)
                cnt += 1
            emit(f"| {min_tiles} | {max_splits} | {worst:.3f} | "
                 f"{math.exp(logsum / max(cnt, 1)):.3f} |")

    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

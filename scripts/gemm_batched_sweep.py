#!/usr/bin/env python3
"""gemm_batched_sweep.py — the batched, strided bf16 GEMM
(native/gemm_batched.hip) against what the tree could do without it: a
Python loop over the heads.

Method of scripts/gemm_act_sweep.py (docs/benchmarking.md): the rows of a
shape are measured in INTERLEAVED rounds with the best kept per row. The
batched call is timed TWICE (rows (b) and (b'), the same function): their
spread, and the delta of a fixed hipBLASLt control that brackets the sweep,
are what nothing tighter can be told apart from.

Shapes: H = 32 heads of D = 128 inside x, y [T, H*D] (row stride H*D, batch
stride D), T = 1024 and 4096:
  Q K^T   nt   S_h [T,T] = Q_h [T,D] K_h [T,D]^T        heads read in place
  P V     nn   O_h [T,D] = P_h [T,T] V_h [T,D]          V read in place
  dV      tn   dV_h [T,D] = P_h [T,T]^T dO_h [T,D]      dO read in place
Rows, fp32 output everywhere but (t):
  (b), (b')  ops.gemm_bf16_batched on the views, one launch
  (l)        a loop of ops.gemm_bf16_layout per head on contiguous per-head
             copies made beforehand (nt: gemm_bf16, whose default kernel at
             these shapes is printed)
  (l+c)      the same loop making the per-head contiguous() copies of the
             interleaved operands inside the timed region
  (t)        torch.bmm on the same views (bf16 output; orientation only)
(b) is checked torch.equal against (l) whenever both run the 128^2
double-buffered body, else close to it.

Usage (GPU box):  python scripts/gemm_batched_sweep.py [--rounds 3]
                      [--out profiles/gemm_batched_table.md]
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

HEADS, DIM = 32, 128
TOKENS = [1024, 4096]


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
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()

    import torch

    from hpc_patterns_amd import ops
    from hpc_patterns_amd._native import native

    if not torch.cuda.is_available():
        sys.exit("gemm_batched_sweep.py needs a GPU")
    dev = torch.device("cuda", 0)
    bf16 = torch.bfloat16
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lines = []

    def emit(text=""):
        print(text, flush=True)
        lines.append(text)

    def rand(*shape):
        return (torch.rand(*shape, device=dev) * 2 - 1).to(bf16)

    ca, cb = rand(4096, 4096), rand(4096, 4096)

    def control():
        return time_gpu(lambda: torch.matmul(ca, cb.t()), inner=10, reps=6,
                        warm=3)

    emit(f"device: {torch.cuda.get_device_name(0)}, {n_cu} CUs; rounds = "
         f"{args.rounds}, inner = {args.inner}")
    c_start = control()
    emit(f"hipBLASLt bf16 4096^3 control (start): {c_start:8.1f} us")
    emit()

    def measure(rows):
        best = {name: float("inf") for name in rows}
        for _ in range(args.rounds):
            for name, fn in rows.items():
                best[name] = min(best[name], time_gpu(fn, args.inner))
        return best

    h, d = HEADS, DIM
    results = []
    for t in TOKENS:
        x, y = rand(t, h * d), rand(t, h * d)
        pm = rand(h, t, t)
        heads_x = x.view(t, h, d).permute(1, 0, 2)      # [H, T, D] in place
        heads_y = y.view(t, h, d).permute(1, 0, 2)
        # (name, layout, a_stored, b_stored, interleaved operands, m, n, k)
        products = [
            ("Q K^T", "nt", heads_x, heads_y, (True, True), t, t, d),
            ("P V", "nn", pm, heads_y, (False, True), t, d, t),
            ("dV = P^T dO", "tn", pm, heads_y, (False, True), t, d, t),
        ]
        for name, layout, a_st, b_st, inter, m, n, k in products:
            c = torch.empty(h, m, n, device=dev)
            c_loop = torch.empty(h, m, n, device=dev)
            a_c = a_st.contiguous()
            b_c = b_st.contiguous()
            variant = native().gemm_variant("bf16", m, n, k) \
                if layout == "nt" else "bf16_lay"

            def batched():
                ops.gemm_bf16_batched(c, a_st, b_st, layout)

            def loop():
                for i in range(h):
                    ops.gemm_bf16_layout(c_loop[i], a_c[i], b_c[i], layout)

            def loop_copies():
                for i in range(h):
                    ai = a_st[i].contiguous() if inter[0] else a_st[i]
                    bi = b_st[i].contiguous() if inter[1] else b_st[i]
                    ops.gemm_bf16_layout(c_loop[i], ai, bi, layout)

            la = a_st.transpose(1, 2) if layout[0] == "t" else a_st
            lb = b_st.transpose(1, 2) if layout[1] == "t" else b_st

            def torch_bmm():
                return torch.bmm(la, lb)

            batched()
            loop()
            torch.cuda.synchronize()
            if variant in ("bf16_lay", "bf16_db8"):
                assert torch.equal(c, c_loop), (name, t)
            else:       # another summation order
                err = (c - c_loop).abs().max().item()
                assert err <= 1e-3 * c_loop.abs().max().item(), (name, t, err)
            best = measure({"(b)": batched, "(l)": loop,
                            "(l+c)": loop_copies, "(b')": batched,
                            "(t)": torch_bmm})
            results.append((name, layout, t, (m, n, k), variant, best))
            print(f"# {name} T={t} done", flush=True)
            del c, c_loop, a_c, b_c
        del x, y, pm
        torch.cuda.empty_cache()

    c_end = control()
    delta = abs(c_end - c_start) / c_start
    emit(f"### us per call over {h} heads, best of {args.rounds} interleaved "
         f"rounds")
    emit()
    emit("| product | layout | T | M x N x K per head | loop kernel | (b) | "
         "(b') | (l) | (l+c) | (t) | (b)/(l) | (b)/(l+c) | spread | "
         "vs (l) | vs (l+c) |")
    emit("|---|---|---:|---|---|---:|---:|---:|---:|---:|---:|---:|---:|---|"
         "---|")
    for name, layout, t, shape, variant, r in results:
        b = min(r["(b)"], r["(b')"])
        spread = max(abs(r["(b)"] - r["(b')"]) / r["(b)"], delta)

        def verdict(ratio):
            return "ahead" if ratio < 1 - spread else \
                ("behind" if ratio > 1 + spread else "level")

        rl, rc = b / r["(l)"], b / r["(l+c)"]
        again = r["(b')"]
        emit(f"| {name} | {layout} | {t} | {' x '.join(map(str, shape))} | "
             f"{variant} | {r['(b)']:.1f} | {again:.1f} | "
             f"{r['(l)']:.1f} | {r['(l+c)']:.1f} | {r['(t)']:.1f} | "
             f"{rl:.3f} | {rc:.3f} | {spread:.3f} | {verdict(rl)} | "
             f"{verdict(rc)} |")
    emit()
    emit(f"hipBLASLt bf16 4096^3 control (end)  : {c_end:8.1f} us")
    emit(f"control delta (|end - start| / start): {delta:.3f}")

    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

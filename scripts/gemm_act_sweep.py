#!/usr/bin/env python3
"""gemm_act_sweep.py — what the activation epilogues (native/gemm_act.hip)
buy over the compositions they replace.

Method of scripts/gemm_epilogue_sweep.py (docs/benchmarking.md): the rows of
a shape are measured in INTERLEAVED rounds with the best kept per row. Every
pair times its baseline TWICE (rows (u) and (u'), the same function): their
spread is what nothing tighter can be told apart from, and a fused row counts
as ahead only if it is ahead of (u) by more than that spread. A fixed
hipBLASLt control brackets the sweep.

Per shape tokens x hidden x in and per activation (relu, gelu = tanh form):
  (a) forward   (f) ops.matmul(x, w1.t(), out_dtype=bf16, bias=b1,
                    activation=act, return_aux=gelu)
                (u) ops.matmul(x, w1.t(), out_dtype=bf16, bias=b1), then
                    torch gelu(approximate="tanh") / relu on the bf16 result
  (b) gradient  (f) ops.matmul(dy, w2, out_dtype=bf16,
                    activation_grad=(act, aux))      dy [tokens, in]
                (u) ops.matmul(dy, w2, out_dtype=bf16), then torch's
                    gelu_backward / threshold_backward
  (c) MLP step  (f) ops.mlp_bf16 forward + backward, all five gradients
                (u) linear_bf16(fused=True), torch activation,
                    linear_bf16(fused=True) under autograd
split_k="auto" everywhere. The skinny rows are the split-K shapes of the
epilogue sweep read as M x N x K; they run (a) and (b) only.

Usage (GPU box):  python scripts/gemm_act_sweep.py [--rounds 3]
                      [--out profiles/gemm_act_table.md]
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

# tokens x hidden x in (out = in)
MLP_SHAPES = [(4096, 4096, 1024), (8192, 8192, 2048), (8192, 4096, 4096)]
SKINNY = [(256, 256, 16384), (256, 256, 65536), (512, 512, 16384),
          (512, 512, 65536), (1024, 1024, 16384)]
ACTS = ["relu", "gelu"]


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
    import torch.nn.functional as F

    from hpc_patterns_amd import ops

    if not torch.cuda.is_available():
        sys.exit("gemm_act_sweep.py needs a GPU")
    dev = torch.device("cuda", 0)
    bf16 = torch.bfloat16
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lines = []

    def emit(text=""):
        print(text, flush=True)
        lines.append(text)

    def rand(rows, cols, scale=1.0):
        return ((torch.rand(rows, cols, device=dev) * 2 - 1) * scale).to(bf16)

    ca, cb = rand(4096, 4096), rand(4096, 4096)

    def control():
        return time_gpu(lambda: torch.matmul(ca, cb.t()), inner=10, reps=6,
                        warm=3)

    emit(f"device: {torch.cuda.get_device_name(0)}, {n_cu} CUs; rounds = "
         f"{args.rounds}, inner = {args.inner}")
    c_start = control()
    emit(f"hipBLASLt bf16 4096^3 control (start): {c_start:8.1f} us")
    emit()

    def torch_act(z, act):
        return F.gelu(z, approximate="tanh") if act == "gelu" \
            else torch.relu(z)

    def torch_act_grad(dh, aux, act):
        if act == "gelu":
            return torch.ops.aten.gelu_backward(dh, aux, approximate="tanh")
        return torch.ops.aten.threshold_backward(dh, aux, 0)

    def measure(rows, inner):
        best = {name: float("inf") for name in rows}
        for _ in range(args.rounds):
            for name, fn in rows.items():
                best[name] = min(best[name], time_gpu(fn, inner))
        return best

    results = []
    for (tokens, hidden, n_in), with_mlp in \
            [(s, True) for s in MLP_SHAPES] + [(s, False) for s in SKINNY]:
        # |z| stays within a few units: uniform operands, 1/sqrt(K) scale
        x = rand(tokens, n_in)
        w1 = rand(hidden, n_in, 3.0 / n_in ** 0.5)
        b1 = torch.arange(hidden, device=dev, dtype=torch.float32) % 17 / 32
        w2 = rand(n_in, hidden, 3.0 / hidden ** 0.5)
        b2 = torch.arange(n_in, device=dev, dtype=torch.float32) % 13 / 16
        dy = rand(tokens, n_in)
        inner = args.inner if tokens * hidden * n_in < 2 ** 36 \
            else max(2, args.inner // 3)
        kw = dict(out_dtype=bf16, split_k="auto")
        for act in ACTS:
            gelu = act == "gelu"

            def fwd_f():
                return ops.matmul(x, w1.t(), bias=b1, activation=act,
                                  return_aux=gelu, **kw)

            def fwd_u():
                return torch_act(ops.matmul(x, w1.t(), bias=b1, **kw), act)

            res = fwd_f()
            h, z = res if gelu else (res, None)
            want = fwd_u()
            torch.cuda.synchronize()
            if gelu:    # torch rounds its fp32 gelu of bf16(z): not the bits
                err = (h.float() - want.float()).abs().max().item()
                assert err <= want.float().abs().max().item() / 64, err
            else:
                assert torch.equal(h, want), (tokens, hidden, n_in)
            aux = z if gelu else h

            def grad_f():
                return ops.matmul(dy, w2, activation_grad=(act, aux), **kw)

            def grad_u():
                return torch_act_grad(ops.matmul(dy, w2, **kw), aux, act)

            got, want = grad_f(), grad_u()
            torch.cuda.synchronize()
            if gelu:
                err = (got.float() - want.float()).abs().max().item()
                assert err <= want.float().abs().max().item() / 64, err
            else:
                assert torch.equal(got, want), (tokens, hidden, n_in)
            del res, h, want, got
            pairs = {"(a) forward": (fwd_f, fwd_u),
                     "(b) gradient": (grad_f, grad_u)}
            if with_mlp:
                leaves = [t.clone().requires_grad_()
                          for t in (x, w1, b1, w2, b2)]

                def step(fn):
                    for t in leaves:
                        t.grad = None
                    fn(*leaves).backward(dy)

                def mlp_f():
                    step(lambda *t: ops.mlp_bf16(*t, activation=act,
                                                 split_k="auto"))

                def mlp_u():
                    step(lambda xx, ww1, bb1, ww2, bb2: ops.linear_bf16(
                        torch_act(ops.linear_bf16(xx, ww1, bias=bb1,
                                                  fused=True,
                                                  split_k="auto"), act),
                        ww2, bias=bb2, fused=True, split_k="auto"))

                pairs["(c) MLP step"] = (mlp_f, mlp_u)
            for name, (f, u) in pairs.items():
                best = measure({"(f)": f, "(u)": u, "(u')": u}, inner)
                results.append(((tokens, hidden, n_in), act, name, best))
            print(f"# {(tokens, hidden, n_in)} {act} done", flush=True)
            del aux, z
        del x, w1, w2, dy
        torch.cuda.empty_cache()

    c_end = control()
    delta = abs(c_end - c_start) / c_start
    emit(f"### us per call, best of {args.rounds} interleaved rounds")
    emit()
    emit("| tokens x hidden x in | act | pair | (f) | (u) | (u') | (f)/(u) | "
         "spread | ahead |")
    emit("|---|---|---|---:|---:|---:|---:|---:|---|")
    for shape, act, name, r in results:
        again = r["(u')"]
        spread = abs(r["(u)"] - again) / r["(u)"]
        ratio = r["(f)"] / min(r["(u)"], again)
        ahead = "yes" if ratio < 1 - spread else \
            ("behind" if ratio > 1 + spread else "no")
        emit(f"| {' x '.join(map(str, shape))} | {act} | {name} | "
             f"{r['(f)']:.1f} | {r['(u)']:.1f} | {again:.1f} | "
             f"{ratio:.3f} | {spread:.3f} | {ahead} |")
    emit()
    emit(f"hipBLASLt bf16 4096^3 control (end)  : {c_end:8.1f} us")
    emit(f"control delta (|end - start| / start): {delta:.3f}")

    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

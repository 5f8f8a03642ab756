#!/usr/bin/env python
"""Host-push probe for StepPlan (native/step.hip): the numbers behind
profiles/flagship_host_push.md.

    python scripts/step_push_probe.py [--mib 256] [--reps 5] [--steps 30]

Part 1 is StepPlan.push_probe() on buffers of the flagship's shape: (a) can
the CPU store into the H2D destination, (b) push rate by thread count, (c)
D2H engine time alone, next to the engine H2D, next to a push of all of H2D
and next to each g-split. Part 2 runs whole steps (kernels included) through
plans with fixed push fractions and prints per-copy device times, the
workers' wake-up and finish times, and ms/step. Prints markdown tables.
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--fractions", default="0,0.1,0.2,0.3,0.4,0.5,auto")
    args = ap.parse_args()

    from hpc_patterns_amd.models.flagship import (DEFAULT_CONFIG,
                                                  FlagshipPatternStep)

    cfg = dict(DEFAULT_CONFIG)
    cfg["h2d_bytes"] = cfg["d2h_bytes"] = args.mib << 20
    dev = torch.device("cuda", 0)
    os.environ["HPK_STEP_COPY_TIMES"] = "1"

    def make(fraction):
        if fraction == "auto":
            os.environ.pop("HPK_STEP_PUSH", None)
        else:
            os.environ["HPK_STEP_PUSH"] = fraction
        return FlagshipPatternStep(device=dev, rank=0, world_size=1,
                                   config=dict(cfg))

    step = make("0")
    cfg["tripcount"] = step.config["tripcount"]  # calibrate once
    print(f"## probe, {args.mib} MiB per direction, median of {args.reps}\n")
    print("| quantity | value |\n|---|---|")
    for name, value in step.plan.push_probe(args.reps):
        print(f"| {name} | {value:.3f} |")
    step.close()

    print(f"\n## whole steps, {args.steps} after 5 warm-up, median (min-max)\n")
    print("| HPK_STEP_PUSH | g | threads | ms/step | H2D engine us | "
          "D2H engine us | pair us | workers first store us | "
          "workers done us |\n|---|---|---|---|---|---|---|---|---|")

    def fmt(v):
        return (f"{statistics.median(v):.1f} ({min(v):.1f}-{max(v):.1f})"
                if v else "-")

    for fraction in args.fractions.split(","):
        step = make(fraction)
        plan = step.plan
        for _ in range(5):
            step.step()
        plan.clear_copy_times()
        wall, wake, done = [], [], []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            step.step()
            wall.append((time.perf_counter() - t0) * 1e3)
            w, d = plan.push_times()
            if plan.push_threads:
                wake.append(w / 1e3)
                done.append(d / 1e3)
        ct = plan.copy_times()
        h2d = [(e - s) / 1e3 for s, e in ct[0::2] if e]
        d2h = [(e - s) / 1e3 for s, e in ct[1::2]]
        pair = [(max(a[1], b[1]) - min(a[0] or b[0], b[0])) / 1e3
                for a, b in zip(ct[0::2], ct[1::2])]
        print(f"| {fraction} | {plan.push_fraction:.3f} | {plan.push_threads} "
              f"| {fmt(wall)} | {fmt(h2d)} | {fmt(d2h)} | {fmt(pair)} "
              f"| {fmt(wake)} | {fmt(done)} |")
        step.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

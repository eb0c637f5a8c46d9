#!/usr/bin/env python
"""Evaluation-mode timing on the MI355X (LAB.md section "evaluation"): objgan_moments_accumulate for 128 x 2048 rows
against torch's fp64 GEMM `outer.addmm_(x64.T, x64)` on the same device, hipEvents over --calls calls after warm-up,
the two interleaved in one process.

    python tools/eval_time.py [--calls 50]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "obj-gan_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def time_moments(dev, calls):
    from objgan_hip import ops
    g = torch.Generator().manual_seed(0)
    x = torch.clamp(0.3 + 0.4 * torch.randn(128, 2048, generator=g), min=0).to(dev)
    x64 = x.double()
    acc = ops.MomentAccumulator(2048, dev)
    outer = torch.zeros(2048, 2048, dtype=torch.float64, device=dev)

    def kernel():
        acc.add(x)

    def gemm():
        outer.addmm_(x64.t(), x64)
    ms = {"kernel": [], "addmm": []}
    for fn in (kernel, gemm):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    for _ in range(calls):
        for name, fn in (("kernel", kernel), ("addmm", gemm)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {k: {"median_us": 1e3 * float(np.median(v)), "min_us": 1e3 * float(np.min(v))} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print(json.dumps({"moments_128x2048": time_moments(dev, args.calls)}), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Snapshot-grid timing on the MI355X (LAB.md section "snapshot grids"): the grids of one snapshot of a three-stage
tree at B = 16 -- word and bottom-up attention over the 128^2 and 256^2 outputs (maps of 64^2 and 128^2) and the DAMSM
word attention over the 256^2 output (17^2 regions, 272-pixel panels) -- composed on the device
(objgan_hip.ops.snapshot_grid, the uint8 grid copied back, wall clock around a synchronize) next to the same grids
built by the host restatement of tests/snapshot_helpers.py (numpy / scipy / PIL, the reference's route), in one process.

    python tools/snapshot_time.py [--repeats 3] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "obj-gan_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def grids(B=16, T=12, R=10, seed=0):
    """(name, image, lr image, maps, att_sze) of the five grids; softmax-like maps, tanh-like images"""
    g = torch.Generator().manual_seed(seed)
    img = {s: torch.tanh(torch.randn(B, 3, s, s, generator=g)) for s in (64, 128, 256)}

    def maps(n, a):
        return torch.softmax(torch.randn(B, n, a * a, generator=g), 2).reshape(B, n, a, a)
    return [("G_0", img[128], img[64], maps(T, 64), 64), ("bt_G_0", img[128], img[64], maps(R, 64), 64),
            ("G_1", img[256], img[128], maps(T, 128), 128), ("bt_G_1", img[256], img[128], maps(R, 128), 128),
            ("D", img[256], None, maps(T, 17), 17)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    from objgan_hip import ops
    import snapshot_helpers as SH
    dev = torch.device("cuda:0")
    cases = grids()
    strips = [SH.plain_strip(8, SH.vis_size_of(a, int(im.shape[2])), 12, 50) for _, im, _, _, a in cases]
    on_dev = [(im.to(dev), None if lr is None else lr.to(dev), m.to(dev), a, torch.from_numpy(s).to(dev))
              for (_, im, lr, m, a), s in zip(cases, strips)]

    def device_snapshot():
        return [ops.snapshot_grid(im, m, a, s, lr_imgs=lr).cpu().numpy() for im, lr, m, a, s in on_dev]

    device_snapshot()                                   # (expansion matrices built and uploaded, allocator warm)
    torch.cuda.synchronize()
    dev_ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        out = device_snapshot()
        torch.cuda.synchronize()
        dev_ms.append((time.perf_counter() - t0) * 1e3)
    # device time alone: events around the launches, no copy back
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    keep = [ops.snapshot_grid(im, m, a, s, lr_imgs=lr) for im, lr, m, a, s in on_dev]
    e1.record()
    torch.cuda.synchronize()
    res = {"grids": [c[0] for c in cases], "grid_bytes": int(sum(o.size for o in out)), "B": 16,
           "device_ms_with_copy_back": [round(v, 2) for v in dev_ms], "device_kernels_ms": round(e0.elapsed_time(e1), 2)}
    del keep
    if not args.no_host:
        t0 = time.perf_counter()
        host = [SH.grid(im, m, a, s, lr_imgs=lr) for (_, im, lr, m, a), s in zip(cases, strips)]
        res["host_restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["attention_bytes_differing"] = int(sum(
            (o[SH.regions(8, SH.vis_size_of(a, int(im.shape[2])), 12, 50, m.shape[1] + 1)["attention"]]
             != h[SH.regions(8, SH.vis_size_of(a, int(im.shape[2])), 12, 50, m.shape[1] + 1)["attention"]]).sum()
            for o, h, (_, im, _, m, a) in zip(out, host, cases)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()

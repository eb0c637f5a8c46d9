"""save_singleimages before and after the device JPEG encoder (csrc/jpeg_enc.hip), same process, same images:
B = 16 generator-like 256 x 256 fp32 images on the device -> 16 .jpg files in a temporary directory.
Wall clock per batch (median and spread over the runs) of the host loop (device_jpeg=False: the loop as it was) and of the
device path, device-event time of the two encoder stages, and the bytes that cross PCIe.  Prints one JSON line last.

    python tools/jpeg_encode_time.py [--runs 20] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "obj-gan_amd"))
from objgan_hip import ops  # noqa: E402
from evaluator import condGANEvaluator  # noqa: E402


def generator_like(n, size, dev):
    """smooth structure plus fine texture in [-1, 1], the statistics of a tanh output (a photograph-like JPEG load)"""
    g = torch.Generator().manual_seed(3)
    low = torch.nn.functional.interpolate(torch.randn(n, 3, size // 16, size // 16, generator=g), size=(size, size),
                                          mode="bicubic", align_corners=False)
    return torch.tanh(low * 1.2 + torch.randn(n, 3, size, size, generator=g) * 0.08).to(dev)


def spread(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median_ms": statistics.median(ts), "iqr_ms": q[2] - q[0], "min_ms": min(ts), "max_ms": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    x = generator_like(a.batch, a.size, dev)
    keys, ids = ["img%02d" % i for i in range(a.batch)], [0] * a.batch
    out = {"batch": a.batch, "size": a.size, "runs": a.runs}
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {}
        for name, kwargs in (("host_loop", {"device_jpeg": False}), ("device", {})):
            dirs[name] = os.path.join(tmp, name)
            os.makedirs(dirs[name])
            me = types.SimpleNamespace(image_dir=dirs[name])
            ts = []
            for r in range(a.warmup + a.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                condGANEvaluator.save_singleimages(me, x, keys, ids, **kwargs)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            out[name] = spread(ts[a.warmup:])
        files = {n: [open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))] for n, d in dirs.items()}
        out["identical_files"] = files["host_loop"] == files["device"] and len(files["device"]) == a.batch
        out["pcie_bytes_host_loop"] = a.batch * a.size * a.size * 3
        out["pcie_bytes_device"] = sum(len(f) for f in files["device"]) + 4 * a.batch
    # device-event time of the two stages, apart
    _, _, state = ops.jpeg_encode_device(x)
    stage_ms = {}
    for name, stages in (("transform", 1), ("entropy", 2)):
        ts = []
        for r in range(a.warmup + a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.jpeg_encode_device(x, stages=stages, state=state)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        stage_ms[name] = spread(ts[a.warmup:])
    out["stages_device_ms"] = stage_ms
    gain = out["host_loop"]["median_ms"] - out["device"]["median_ms"]
    out["device_path_wins"] = gain > out["host_loop"]["iqr_ms"] + out["device"]["iqr_ms"]
    for k in ("host_loop", "device"):
        print("%-10s median %.3f ms  iqr %.3f  min %.3f  max %.3f" % ((k,) + tuple(out[k][f] for f in ("median_ms", "iqr_ms", "min_ms", "max_ms"))))
    for k, v in stage_ms.items():
        print("%-10s device median %.3f ms  iqr %.3f" % (k, v["median_ms"], v["iqr_ms"]))
    print("PCIe bytes per batch: %d -> %d" % (out["pcie_bytes_host_loop"], out["pcie_bytes_device"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

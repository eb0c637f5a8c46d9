"""The annotation preprocessing (miscc/coco_prep.py) on the host and on the device, same process, same data: a synthetic
COCO-shaped set of --images 640 x 480 images with 7 star-shaped polygons of about 30 vertices each (seeded; no COCO
content) -> `build_gt_insanns` through the numpy + scipy route and through csrc/coco_masks.hip.  Wall clock of each route
(the device route once cold and --runs times warm), the device-event time of the kernels inside the device route and
their share of it, and whether the two dictionaries are identical.  Prints one JSON line last.

    python tools/prep_time.py [--images 1000] [--runs 3] [--BATCH 64]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "obj-gan_amd"))
from miscc import coco_prep  # noqa: E402
from objgan_hip import _lib, ops  # noqa: E402

H, W, PER_IMAGE, VERTS = 480, 640, 7, 30


def synthetic(n_images, seed=7):
    rng = np.random.RandomState(seed)
    images, anns = [], []
    for i in range(n_images):
        images.append({"id": i + 1, "height": H, "width": W, "file_name": "COCO_train2014_%012d.jpg" % (i + 1)})
        for k in range(PER_IMAGE):
            cx, cy = rng.uniform(60, W - 60), rng.uniform(60, H - 60)
            radius = rng.uniform(25, 160) * rng.uniform(0.6, 1.0, VERTS)
            angle = np.sort(rng.uniform(0, 2 * np.pi, VERTS))
            x = np.round(np.clip(cx + radius * np.cos(angle), 0, W - 1), 2)
            y = np.round(np.clip(cy + radius * np.sin(angle), 0, H - 1), 2)
            anns.append({"id": len(anns) + 1, "image_id": i + 1, "category_id": int(rng.randint(1, 81)), "iscrowd": 0,
                         "segmentation": [np.stack([x, y], 1).reshape(-1).tolist()],
                         "bbox": [float(x.min()), float(y.min()), float(x.max() - x.min()), float(y.max() - y.min())]})
    return {"images": images, "annotations": anns}, [im["file_name"].split(".")[0] for im in images]


def same(a, b):
    if sorted(a) != sorted(b):
        return False
    for key in a:
        for field, v in a[key].items():
            w = b[key][field]
            if field == "num_rois":
                ok = v == w
            elif v is None or w is None:
                ok = v is None and w is None
            elif field in ("rois", "masks"):
                ok = len(v) == len(w) and all(np.array_equal(p, q) for p, q in zip(v, w))
            else:
                ok = np.array_equal(v, w)
            if not ok:
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--BATCH", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("prep_time.py: needs the GPU (it times the device route)")
    dev = torch.device("cuda:0")
    dataset, names = synthetic(a.images)
    cats = {c: c - 1 for c in range(1, 81)}
    events = []
    real_call = _lib.call

    def timed_call(name, *args):
        if name != "objgan_poly_masks":
            return real_call(name, *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real_call(name, *args)
        e1.record()
        events.append((e0, e1))
    ops._lib.call = timed_call
    out = {"images": a.images, "instances": len(dataset["annotations"]), "height": H, "width": W, "batch": a.BATCH}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "insanns"))
        with open(os.path.join(tmp, "insanns", "instances_train2014.json"), "w") as f:
            json.dump(dataset, f)

        def run(device):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d = coco_prep.build_gt_insanns(tmp, names, "train", [64, 128, 256], 16, cats, device=device, batch=a.BATCH)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, d
        out["device_cold_s"], on_device = run(dev)
        warm, kernel = [], []
        for _ in range(a.runs):
            del events[:]
            t, on_device = run(dev)
            warm.append(t)
            kernel.append(sum(e0.elapsed_time(e1) for e0, e1 in events) / 1e3)
        out["device_s"] = {"median": statistics.median(warm), "min": min(warm), "max": max(warm)}
        out["device_kernels_s"] = {"median": statistics.median(kernel), "min": min(kernel), "max": max(kernel)}
        out["device_kernels_share"] = statistics.median(kernel) / statistics.median(warm)
        out["host_s"], on_host = run(None)
        out["identical"] = same(on_device, on_host)
    out["kept_instances"] = int(sum(d["num_rois"] for d in on_host.values()))
    print("host route   %.2f s" % out["host_s"])
    print("device route %.2f s (cold %.2f s), kernels %.3f s = %.1f %% of it" % (
        out["device_s"]["median"], out["device_cold_s"], out["device_kernels_s"]["median"], 100 * out["device_kernels_share"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

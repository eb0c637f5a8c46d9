"""Seeded synthetic TEST split for the shape generator's sampling command and grids (no COCO content):

    python tests/golden/shape_tiny_test/make_shape_tiny_test.py

Writes, beside itself, what shapeDataset.TextDataset(<here>, 'test') reads: test/filenames.pickle, captions.pickle,
categories.txt (the 16 categories of tests/golden/shape_tiny), test_shape_insanns.pickle in the reference's layout
(shape_generation/datasets.py:241-391) and test_imgs.bigfile (reference load.py: native int32 length + JPEG bytes per
image).  Five images with 1, 0, 10, 2 and 3 boxes, in this order: at batch size 2 without shuffling the whole batches
are (1 box, no box) and (10 boxes, 2 boxes).  Masks and box maps are 0 / 1 in uint8 (the loader casts to float32) and
the JPEGs are small smooth colour fields of different, non-square sizes, to keep the files small."""
import io
import os
import pickle
import struct

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
NB, S, FM, NCAT = 10, 64, 16, 16
COUNTS = (1, 0, 10, 2, 3)
SIZES = ((96, 80), (72, 100), (128, 96), (64, 64), (90, 70))          # (width, height) of the JPEGs
NAMES = ["person", "bicycle", "car", "dog", "traffic light", "bench", "bird", "cat", "horse", "sheep", "cow", "kite",
         "cup", "fork", "knife", "bowl"]


def main():
    rng = np.random.RandomState(2025)
    filenames = ["tinytest_%02d" % i for i in range(len(COUNTS))]
    words = sorted({w for n in NAMES for w in n.split()})
    ixtoword = {0: "<end>"}
    ixtoword.update({i + 1: w for i, w in enumerate(words)})
    wordtoix = {w: i for i, w in ixtoword.items()}
    anns = {}
    for name, n in zip(filenames, COUNTS):
        rois = np.zeros((NB, 6))
        fm_rois = np.zeros((NB, 6))
        d = {"rois": rois, "fm_rois": fm_rois, "masks": None, "pooled masks": None, "bbox maps": None,
             "bbox fmaps": None, "num_rois": n}
        if n:
            masks = np.zeros((n, S, S), np.uint8)
            bmaps = np.zeros((n, S, S), np.uint8)
            fmaps = np.zeros((n, FM, FM), np.uint8)
            for r in range(n):
                x, y = rng.randint(0, 36, 2)
                w, h = rng.randint(8, 26, 2)
                rois[r] = [x, y, w, h, rng.randint(0, NCAT), 0]
                fm_rois[r] = [x / 4.0, y / 4.0, w / 4.0, h / 4.0, rois[r, 4], 0]
                bmaps[r, y:y + h, x:x + w] = 1
                fmaps[r, y // 4:(y + h) // 4, x // 4:(x + w) // 4] = 1
                yy, xx = np.mgrid[0:S, 0:S]
                inside = ((xx - x - w / 2.0) / (0.5 * w)) ** 2 + ((yy - y - h / 2.0) / (0.5 * h)) ** 2 <= 1.0
                masks[r] = inside & (bmaps[r] > 0)
            d.update({"masks": masks, "pooled masks": masks.max(0), "bbox maps": bmaps, "bbox fmaps": fmaps})
        anns[name] = d
    os.makedirs(os.path.join(HERE, "test"), exist_ok=True)
    with open(os.path.join(HERE, "test", "filenames.pickle"), "wb") as f:
        pickle.dump(filenames, f, protocol=2)
    with open(os.path.join(HERE, "captions.pickle"), "wb") as f:
        pickle.dump([[], [[1]] * len(filenames), ixtoword, wordtoix], f, protocol=2)
    with open(os.path.join(HERE, "categories.txt"), "w") as f:
        for i, n in enumerate(NAMES):
            f.write("%d,%s\n" % (i + 1, n))
    with open(os.path.join(HERE, "test_shape_insanns.pickle"), "wb") as f:
        pickle.dump([anns], f, protocol=2)
    with open(os.path.join(HERE, "test_imgs.bigfile"), "wb") as f:
        for k, (w, h) in enumerate(SIZES):
            yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
            ph = rng.uniform(0, 6.28, (3, 2))
            fr = rng.uniform(0.03, 0.12, (3, 2))
            img = np.stack([127.5 + 120 * np.sin(fr[c, 0] * xx + ph[c, 0]) * np.cos(fr[c, 1] * yy + ph[c, 1])
                            for c in range(3)], 2)
            buf = io.BytesIO()
            Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(buf, format="JPEG", quality=85)
            f.write(struct.pack("i", len(buf.getvalue())))
            f.write(buf.getvalue())
    for leaf in ("test_shape_insanns.pickle", "test_imgs.bigfile"):
        print("wrote", leaf, os.path.getsize(os.path.join(HERE, leaf)), "bytes")


if __name__ == "__main__":
    main()

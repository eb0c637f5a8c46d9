"""Seeded synthetic data directory for the shape generator's training (no COCO content):

    python tests/golden/shape_tiny/make_shape_tiny.py

Writes, beside itself, what shapeDataset.TextDataset reads: train/filenames.pickle, captions.pickle (only its word
index is read), categories.txt (16 categories) and train_shape_insanns.pickle in the reference's layout
(shape_generation/datasets.py:241-391: per image rois, fm_rois, masks, pooled masks, bbox maps, bbox fmaps, num_rois).
Six images with 0, 10, 2, 1, 2 and 3 boxes.  Arrays are float32 (the reference's are float64; the loader casts to
float32 either way) to keep the file small."""
import os
import pickle

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NB, S, FM, NCAT = 10, 64, 16, 16
COUNTS = (0, 10, 2, 1, 2, 3)
NAMES = ["person", "bicycle", "car", "dog", "traffic light", "bench", "bird", "cat", "horse", "sheep", "cow", "kite",
         "cup", "fork", "knife", "bowl"]


def main():
    rng = np.random.RandomState(2024)
    filenames = ["tiny_%02d" % i for i in range(len(COUNTS))]
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
            masks = np.zeros((n, S, S), np.float32)
            bmaps = np.zeros((n, S, S), np.float32)
            fmaps = np.zeros((n, FM, FM), np.float32)
            for r in range(n):
                x, y = rng.randint(0, 36, 2)
                w, h = rng.randint(8, 26, 2)
                rois[r] = [x, y, w, h, rng.randint(0, NCAT), 0]
                fm_rois[r] = [x / 4.0, y / 4.0, w / 4.0, h / 4.0, rois[r, 4], 0]
                bmaps[r, y:y + h, x:x + w] = 1
                fmaps[r, y // 4:(y + h) // 4, x // 4:(x + w) // 4] = 1
                yy, xx = np.mgrid[0:S, 0:S]
                blob = np.exp(-(((xx - x - w / 2.0) / (0.4 * w)) ** 2 + ((yy - y - h / 2.0) / (0.4 * h)) ** 2))
                masks[r] = (blob * bmaps[r]).astype(np.float32)
            d.update({"masks": masks, "pooled masks": masks.max(0), "bbox maps": bmaps, "bbox fmaps": fmaps})
        anns[name] = d
    os.makedirs(os.path.join(HERE, "train"), exist_ok=True)
    with open(os.path.join(HERE, "train", "filenames.pickle"), "wb") as f:
        pickle.dump(filenames, f, protocol=2)
    with open(os.path.join(HERE, "captions.pickle"), "wb") as f:
        pickle.dump([[[1]] * len(filenames), [], ixtoword, wordtoix], f, protocol=2)
    with open(os.path.join(HERE, "categories.txt"), "w") as f:
        for i, n in enumerate(NAMES):
            f.write("%d,%s\n" % (i + 1, n))
    with open(os.path.join(HERE, "train_shape_insanns.pickle"), "wb") as f:
        pickle.dump([anns], f, protocol=2)
    print("wrote", os.path.getsize(os.path.join(HERE, "train_shape_insanns.pickle")), "bytes")


if __name__ == "__main__":
    main()

"""Writes the hand-made COCO-shaped fixture of tests/test_coco_prep_*.py: instances_val2014.json, keys.txt and
categories.txt in this directory.  Every coordinate below is written out by hand (our own data, no COCO content); nothing
lies beyond its image after the loaders' clip to [0, max(H, W) - 1], so the reference's own code runs on it.

    python tests/golden/coco_prep/make_fixture.py

The recorded results (gt_insanns.npz, shape_insanns.npz) are written by tests/coco_prep_ref.py from the reference.
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

CATEGORIES = [(1, "person"), (2, "bicycle"), (3, "car"), (18, "dog"), (44, "bottle")]

# (image id, height, width)
IMAGES = [(1, 40, 48),        # both axes grow to 64: no filter
          (2, 80, 40),        # portrait: axis 0 shrinks (radius 1), axis 1 grows
          (3, 130, 100),      # non-integer factors, radius 2 and 1
          (4, 480, 640),      # landscape, radius 13 and 18
          (5, 640, 480),      # portrait, radius 18 and 13
          (6, 200, 300),      # 13 instances, one of them under ROI_MIN_SIZE, two of equal area
          (7, 480, 640),      # boxes around the two ROI_MIN_SIZE thresholds
          (8, 64, 64),        # only a crowd annotation
          (9, 50, 70),        # no annotation at all
          (10, 480, 640),     # one instance, under ROI_MIN_SIZE for both loaders
          (11, 64, 64)]       # already 64 x 64: the resize is the identity


def rect(x, y, w, h):
    return [x, y, x + w, y, x + w, y + h, x, y + h]


def bbox_of(rings):
    xs = [v for r in rings for v in r[0::2]]
    ys = [v for r in rings for v in r[1::2]]
    return [min(xs), min(ys), max(xs) - min(xs), max(ys) - min(ys)]


# (image id, category id, rings[, bbox])
ANNOTATIONS = [
    # image 1: integer vertices (the half-open square 2..32), a triangle on a horizontal edge, a negative coordinate
    (1, 1, [[2, 2, 32, 2, 32, 32, 2, 32]]),
    (1, 3, [[5.5, 30.0, 40.25, 30.0, 22.75, 8.5]]),
    (1, 18, [[-3.5, 10.0, 12.0, -2.0, 20.5, 20.0, 4.0, 36.5]], [0, 0, 20.5, 36.5]),
    # image 2 (80 x 40): a vertex at y = H, clipped to 79; a self-intersecting ring; a ring that covers no pixel centre
    (2, 2, [[4.0, 20.5, 35.5, 22.0, 30.0, 80.0, 8.5, 71.25]]),
    (2, 44, [[5.0, 5.0, 35.0, 45.0, 35.0, 5.0, 5.0, 45.0]]),
    (2, 1, [[10.2, 10.2, 10.8, 10.2, 10.5, 10.8]], [2.0, 2.0, 30.0, 30.0]),
    # image 3 (130 x 100): an instance of two rings, one of them inside the other's box; a concave ring
    (3, 1, [[10.5, 12.25, 60.0, 15.5, 55.75, 70.0, 12.0, 64.5], [70.0, 80.0, 95.5, 82.5, 90.0, 120.0, 72.5, 118.0]]),
    (3, 3, [[20.0, 90.0, 50.0, 90.0, 50.0, 125.0, 35.0, 100.0, 20.0, 125.0]]),
    # image 4 (480 x 640, landscape): a vertex at x = W, clipped to 639; a many-sided ring; a thin diagonal sliver
    (4, 3, [[400.0, 100.5, 640.0, 120.0, 610.25, 300.75, 420.5, 280.0]]),
    (4, 1, [[100.5, 50.0, 180.0, 40.25, 260.75, 90.0, 300.0, 200.5, 250.25, 330.0, 160.0, 400.75, 90.5, 350.0,
             40.0, 250.25, 60.75, 120.0]]),
    (4, 18, [[10.0, 470.0, 300.0, 410.0, 302.0, 413.0]]),
    # image 5 (640 x 480, portrait): a vertex at y = H; two overlapping rings; a ring with a repeated vertex
    (5, 2, [[50.5, 400.0, 430.0, 380.25, 470.75, 640.0, 30.0, 600.5]]),
    (5, 1, [[100.0, 100.0, 300.0, 100.0, 300.0, 300.0, 100.0, 300.0], [200.5, 200.5, 400.5, 200.5, 400.5, 350.5, 200.5, 350.5]]),
    (5, 44, [[20.0, 20.0, 80.5, 25.0, 80.5, 25.0, 60.0, 90.5, 20.0, 20.0]]),
    # image 7 (480 x 640): 24 x 18 is under 10 at 256 and over 2 at 64; 12 x 10 is under both; one ordinary box
    (7, 1, [rect(100.0, 100.0, 24.0, 18.0)]),
    (7, 2, [rect(200.0, 200.0, 12.0, 10.0)]),
    (7, 3, [[300.5, 50.0, 500.0, 80.5, 450.25, 300.0, 320.0, 260.75]]),
    # image 10: a single box under both thresholds
    (10, 18, [rect(10.0, 10.0, 3.0, 3.0)]),
    # image 11 (64 x 64)
    (11, 1, [[8.0, 8.0, 50.5, 12.0, 40.0, 55.5, 10.25, 44.0]]),
]

# image 6 (200 x 300): thirteen instances; the second is under ROI_MIN_SIZE for both loaders, which shifts the reference's
# kept indices after its BOXES_NUM selection; the 40 x 30 and 30 x 40 boxes have equal area
for n, (x, y, w, h) in enumerate([(5.0, 5.0, 90.0, 60.0), (100.0, 5.0, 4.0, 3.0), (110.0, 8.0, 40.0, 30.0),
                                  (160.0, 10.0, 30.0, 40.0), (200.0, 5.0, 95.5, 80.25), (10.0, 70.0, 50.0, 45.0),
                                  (70.0, 75.5, 25.0, 20.0), (100.0, 60.0, 70.5, 65.0), (180.0, 90.0, 60.0, 55.5),
                                  (245.0, 95.0, 35.0, 33.0), (10.0, 130.0, 120.0, 62.5), (140.0, 150.0, 28.0, 22.0),
                                  (180.0, 150.0, 110.0, 45.0)]):
    ring = [x, y, x + w * 0.75, y + h * 0.125, x + w, y + h * 0.5, x + w * 0.5, y + h, x, y + h * 0.75]
    ANNOTATIONS.append((6, CATEGORIES[n % len(CATEGORIES)][0], [ring], [x, y, w, h]))


def main():
    images = [{"id": i, "height": h, "width": w, "file_name": "COCO_val2014_%012d.jpg" % i} for i, h, w in IMAGES]
    anns = []
    for k, item in enumerate(ANNOTATIONS):
        image_id, cat, rings = item[:3]
        bbox = item[3] if len(item) > 3 else bbox_of(rings)
        anns.append({"id": 1000 + k, "image_id": image_id, "category_id": cat, "iscrowd": 0, "segmentation": rings,
                     "bbox": bbox, "area": bbox[2] * bbox[3]})
    anns.append({"id": 2000, "image_id": 8, "category_id": 1, "iscrowd": 1, "bbox": [4, 4, 40, 40], "area": 1600,
                 "segmentation": {"counts": [260, 40, 24, 40, 3732], "size": [64, 64]}})
    # a crowd annotation next to polygons: it is skipped, not rasterised
    anns.insert(2, {"id": 2001, "image_id": 1, "category_id": 1, "iscrowd": 1, "bbox": [0, 0, 10, 10], "area": 100,
                    "segmentation": {"counts": [0, 100, 1820], "size": [40, 48]}})
    with open(os.path.join(HERE, "instances_val2014.json"), "w") as f:
        json.dump({"images": images, "annotations": anns,
                   "categories": [{"id": i, "name": n, "supercategory": "thing"} for i, n in CATEGORIES]}, f, indent=0)
    with open(os.path.join(HERE, "keys.txt"), "w") as f:
        f.write("".join("COCO_val2014_%012d\n" % i for i, _, _ in IMAGES))
    with open(os.path.join(HERE, "categories.txt"), "w") as f:
        f.write("".join("%d,%s\n" % c for c in CATEGORIES))


if __name__ == "__main__":
    main()

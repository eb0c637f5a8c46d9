"""The annotation pickles from COCO JSON, host route (obj-gan_amd/miscc/coco_prep.py, prepare_data.py): against the
results recorded from the unmodified reference loaders (tests/golden/coco_prep/*.npz, written by tests/coco_prep_ref.py)
and, where the reference tree is present, against those loaders themselves under the stubs the helper names."""
import os
import pickle
import sys

import numpy as np
import pytest

import coco_prep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pixels(mask):
    return sorted((int(r), int(c)) for r, c in zip(*np.nonzero(mask)))


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from miscc import coco_prep
    data_dir = R.make_data_dir(tmp_path_factory.mktemp("coco_prep"))
    names, cid = R.keys(), R.cats_index_dict()
    return {"data_dir": data_dir,
            "gt": coco_prep.build_gt_insanns(data_dir, names, "test", list(R.IMSIZE), R.FMSIZE, cid),
            "shape": coco_prep.build_shape_insanns(data_dir, names, "test", R.IMSIZE[0], R.FMSIZE, cid)}


@pytest.mark.parametrize("kind", ["gt", "shape"])
def test_host_route_equals_the_reference(built, kind):
    """every key of every image, np.array_equal and the same dtype: against the recorded files, and against the
    reference's own loader where its tree is present"""
    got = R.flatten(built[kind], R.keys())
    R.assert_same(got, dict(np.load(R.RECORDED[kind])), "recorded " + kind)
    if R.reference_available():
        ref = (R.reference_gt if kind == "gt" else R.reference_shape)(built["data_dir"], R.keys())
        R.assert_same(got, R.flatten(ref, R.keys()), "reference " + kind)


def test_the_fixture_reaches_every_branch(built):
    gt, shape, names = built["gt"], built["shape"], R.keys()
    assert [gt[k]["num_rois"] for k in names] == [3, 3, 2, 3, 3, 10, 1, 0, 0, 0, 1]
    assert [shape[k]["num_rois"] for k in names] == [3, 3, 2, 3, 3, 10, 2, 0, 0, 0, 1]     # ROI_MIN_SIZE 2 at 64 pixels
    assert isinstance(gt[names[0]]["rois"], list) and len(gt[names[0]]["rois"]) == 3
    assert isinstance(gt[names[0]]["masks"], list) and isinstance(shape[names[0]]["masks"], np.ndarray)
    assert gt[names[7]]["masks"] is None and gt[names[8]]["pooled masks"] is None and gt[names[9]]["bbox maps"] is None
    assert not gt[names[1]]["masks"][2].any()                   # the ring without a pixel centre: an all-zero mask
    assert np.array_equal(gt[names[10]]["masks"][0], (gt[names[10]]["masks"][0] > 0.5).astype(float))   # 64 -> 64
    for k in names[:5]:
        for m in gt[k]["masks"][:2]:
            assert m.shape == (64, 64) and m.dtype == np.float64 and 0.0 <= m.min() and m.max() <= 1.0 and m.max() > 0.5


def test_polygon_mask_by_hand():
    from miscc.coco_prep import polygon_mask
    # the half-open square: corners (2,2)-(32,32) give 30 x 30 pixels, (2,2) in, row and column 32 out
    m = polygon_mask([[2, 2, 32, 2, 32, 32, 2, 32]], 40, 48)
    assert m.sum() == 900 and m[2, 2] and m[31, 31] and not m[32].any() and not m[:, 32].any() and not m[1].any()
    # triangle (1,1) (5,1) (1,5): row y holds x in [1, 6 - y); the horizontal edge toggles nothing
    assert _pixels(polygon_mask([[1, 1, 5, 1, 1, 5]], 8, 8)) == [(y, x) for y in range(1, 5) for x in range(1, 6 - y)]
    # vertices between pixel centres: x in (0.5, 2.5) and y in [0.5, 2.5) hold the centres 1..2 x 1..2
    assert _pixels(polygon_mask([[0.5, 0.5, 2.5, 0.5, 2.5, 2.5, 0.5, 2.5]], 4, 4)) == [(1, 1), (1, 2), (2, 1), (2, 2)]
    # a bow tie (self-intersecting): two triangles that meet at (3, 3)
    bow = polygon_mask([[0, 0, 6, 6, 6, 0, 0, 6]], 7, 7)
    assert _pixels(bow) == [(y, x) for y in range(6) for x in range(7) if (x < y and x < 6 - y) or (x >= y and x >= 6 - y and x < 6)]
    # two rings are OR-ed, also where they overlap (even-odd holds per ring only)
    two = polygon_mask([[0, 0, 4, 0, 4, 4, 0, 4], [2, 2, 6, 2, 6, 6, 2, 6]], 8, 8)
    assert two.sum() == 16 + 16 - 4 and two[3, 3]
    # nothing between the pixel centres, pixels beyond the image ignored, no ring at all
    assert not polygon_mask([[10.2, 10.2, 10.8, 10.2, 10.5, 10.8]], 20, 20).any()
    assert polygon_mask([[-5, -5, 50, -5, 50, 50, -5, 50]], 6, 9).all()
    assert polygon_mask([], 5, 5).shape == (5, 5) and not polygon_mask([[]], 5, 5).any()
    with pytest.raises(ValueError):
        polygon_mask([[1, 2, 3]], 5, 5)


def test_polygon_mask_against_the_pixelwise_rule():
    """the prefix-toggle form against one comparison per pixel and edge (the helper's restatement), on every ring of the
    fixture and on random rings with vertices on and off the integer grid"""
    from miscc.coco_prep import polygon_mask
    rng = np.random.RandomState(5)
    cases = [(rings, H, W) for rings, H, W in R.fixture_instances() if H * W <= 130 * 100]
    for n in range(40):
        H, W = int(rng.randint(3, 40)), int(rng.randint(3, 40))
        pts = rng.uniform(0, max(H, W) - 1, size=(int(rng.randint(3, 9)), 2))
        if n % 2:
            pts = np.round(pts)
        pts[:, 0] = np.minimum(pts[:, 0], W - 1)
        pts[:, 1] = np.minimum(pts[:, 1], H - 1)
        cases.append(([pts.reshape(-1)], H, W))
    for rings, H, W in cases:
        want = np.zeros((H, W), dtype=bool)
        for ring in rings:
            rr, cc = R._polygon(ring[1::2], ring[0::2])
            want[rr, cc] = True
        assert np.array_equal(polygon_mask(rings, H, W), want)


def test_rle_segmentation_is_refused(tmp_path):
    import json
    from miscc import coco_prep
    data_dir = R.make_data_dir(tmp_path)
    path = os.path.join(data_dir, "insanns", "instances_val2014.json")
    with open(path) as f:
        ds = json.load(f)
    crowd = [a for a in ds["annotations"] if a["image_id"] == 8][0]
    crowd["iscrowd"] = 0                                        # an RLE that is not marked as crowd
    with open(path, "w") as f:
        json.dump(ds, f)
    with pytest.raises(ValueError, match="COCO_val2014_000000000008"):
        coco_prep.build_gt_insanns(data_dir, R.keys(), "test", list(R.IMSIZE), R.FMSIZE, R.cats_index_dict())
    with pytest.raises(KeyError):
        coco_prep.build_shape_insanns(data_dir, ["COCO_val2014_000000009999"], "test", 64, R.FMSIZE, R.cats_index_dict())


def test_read_instances(tmp_path):
    from miscc import coco_prep
    images, anns = coco_prep.read_instances(os.path.join(R.FIXTURE, "instances_val2014.json"))
    assert sorted(images) == sorted(R.keys()) and images[R.keys()[3]]["height"] == 480 and images[R.keys()[3]]["width"] == 640
    assert [a["id"] for a in anns[1]] == [1000, 1001, 2001, 1002] and 9 not in anns and len(anns[6]) == 13


def test_readers_build_the_missing_pickle(tmp_path, built, monkeypatch):
    """both readers build and write the pickle from the JSON (host route: no device here), and the written file goes
    through the same readers again"""
    from miscc import coco_prep, load
    import shapeDataset
    monkeypatch.setattr(coco_prep, "default_device", lambda: None)
    names, cid = R.keys(), R.cats_index_dict()
    data_dir = R.make_data_dir(tmp_path / "d", split="train")
    args = (data_dir, "train", "_gt_insanns.pickle", "gt", names, list(R.IMSIZE), R.FMSIZE, cid)
    first = load.load_anns_data(*args)
    with open(os.path.join(data_dir, "train_gt_insanns.pickle"), "rb") as f:
        assert f.read(2) == b"\x80\x02"                         # protocol 2, like the reference writes it
    os.remove(os.path.join(data_dir, "insanns", "instances_train2014.json"))
    again = load.load_anns_data(*args)                           # now read, not built
    for d in (first, again):
        R.assert_same(R.flatten(d, names), R.flatten(built["gt"], names), "gt reader")
    with pytest.raises(IOError):
        shapeDataset.TextDataset.load_anns_data(data_dir, "train", names, 64, R.FMSIZE, cid)
    R.make_data_dir(data_dir, split="train")
    first = shapeDataset.TextDataset.load_anns_data(data_dir, "train", names, 64, R.FMSIZE, cid)
    again = shapeDataset.TextDataset.load_anns_data(data_dir, "train")
    for d in (first, again):
        R.assert_same(R.flatten(d, names), R.flatten(built["shape"], names), "shape reader")
    with open(os.path.join(data_dir, "train_shape_insanns.pickle"), "rb") as f:
        assert isinstance(pickle.load(f), list)


def test_prepare_data_command(tmp_path, built, capsys):
    import prepare_data
    names = R.keys()
    empty = str(tmp_path / "empty")
    os.makedirs(empty)
    assert prepare_data.main(["--data_dir", empty, "--split", "test", "--cpu"]) == 2
    err = capsys.readouterr().err.strip().split("\n")
    assert len(err) == 1 and err[0].startswith("prepare_data.py: annotation file not found")
    data_dir = R.make_data_dir(tmp_path / "d")
    os.remove(os.path.join(data_dir, "categories.txt"))
    assert prepare_data.main(["--data_dir", data_dir, "--split", "test", "--cpu"]) == 2
    assert "category list not found" in capsys.readouterr().err
    R.make_data_dir(data_dir)
    assert prepare_data.main(["--data_dir", data_dir, "--split", "test", "--what", "both", "--cpu", "--BATCH", "3"]) == 0
    for leaf, kind in (("test_gt_insanns.pickle", "gt"), ("test_shape_insanns.pickle", "shape")):
        with open(os.path.join(data_dir, leaf), "rb") as f:
            R.assert_same(R.flatten(pickle.load(f)[0], names), R.flatten(built[kind], names), leaf)
    os.remove(os.path.join(data_dir, "test_shape_insanns.pickle"))
    assert prepare_data.main(["--data_dir", data_dir, "--split", "test", "--what", "gt", "--cpu"]) == 0
    assert not os.path.exists(os.path.join(data_dir, "test_shape_insanns.pickle"))


def test_prepare_data_exit_status_as_a_process(tmp_path):
    import subprocess
    p = subprocess.run([sys.executable, os.path.join(ROOT, "obj-gan_amd", "prepare_data.py"), "--data_dir", str(tmp_path),
                        "--split", "train", "--cpu"], capture_output=True, text=True)
    assert p.returncode == 2 and p.stderr.strip().count("\n") == 0 and "instances_train2014.json" in p.stderr


def test_abi_symbols_are_in_the_header_table():
    from objgan_hip import _lib
    assert len(_lib.SIGNATURES["objgan_poly_masks"]) == 18
    assert _lib.SIGNATURES["objgan_poly_masks"][1] is _lib._c_long
    assert len(_lib.SIGNATURES["objgan_poly_masks_covers"]) == 5
    assert _lib.LONG_RETURN["objgan_poly_masks_plan"] == [_lib._c_int] * 3


def test_no_forbidden_imports():
    """the product route needs neither pycocotools nor skimage"""
    for leaf in ("miscc/coco_prep.py", "prepare_data.py"):
        with open(os.path.join(ROOT, "obj-gan_amd", leaf)) as f:
            code = [ln for ln in f.read().split("\n") if ln.lstrip().startswith(("import ", "from "))]
        assert not [ln for ln in code if "pycocotools" in ln or "skimage" in ln]

"""TEST INFRASTRUCTURE for tests/test_coco_prep_*.py: the fixture under tests/golden/coco_prep/, the flat form in which
the two annotation dictionaries are recorded and compared, and -- where the reference tree is present -- the UNMODIFIED
reference loaders (image_generation/miscc/load.py `load_gt_insanns`, shape_generation/datasets.py
`TextDataset.load_insanns`, both through the reference's own pycocotools/coco.py `COCO`) run under these stubs:

  skimage.draw.polygon      `_polygon` below: skimage's bounding box and its point_in_polygon, pixel by pixel in numpy
                            (THIRD-PARTY ARITHMETIC restated; written independently of miscc/coco_prep.polygon_mask, which
                            never compares a pixel with an abscissa)
  skimage.transform.resize  `_resize` below: skimage >= 0.19's defaults as the two scipy.ndimage calls it makes
  skimage.io.imread         zeros of the size the JSON gives for the image (the loaders read only the shape)
  pycocotools._mask         a permissive stub (RLE code, never reached by the loaders)
  np.int / np.float         aliases (np.bool exists in numpy 2 and is left alone)
  nltk, torchtext, spacy, torchvision, easydict, models.roi_align   imported by the modules, unused by the loaders

    python tests/coco_prep_ref.py        # writes tests/golden/coco_prep/{gt,shape}_insanns.npz from the reference
"""
import contextlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "coco_prep")
REFERENCE = os.environ.get("OBJGAN_REFERENCE_ROOT", "/root/reference")
IMSIZE, FMSIZE = [64, 128, 256], 16
RECORDED = {"gt": os.path.join(FIXTURE, "gt_insanns.npz"), "shape": os.path.join(FIXTURE, "shape_insanns.npz")}


def keys():
    with open(os.path.join(FIXTURE, "keys.txt")) as f:
        return f.read().split()


def cats_index_dict():
    with open(os.path.join(FIXTURE, "categories.txt")) as f:
        return {int(ln.split(",")[0]): i for i, ln in enumerate(f.read().split("\n")) if ln}


def make_data_dir(root, split="test", names=None):
    """a data directory holding what the builders read: insanns/instances_val2014.json (also as train2014 when split is
    'train'), <split>/filenames.pickle, categories.txt"""
    import pickle
    import shutil
    root = str(root)
    os.makedirs(os.path.join(root, "insanns"), exist_ok=True)
    os.makedirs(os.path.join(root, split), exist_ok=True)
    shutil.copy(os.path.join(FIXTURE, "instances_val2014.json"),
                os.path.join(root, "insanns", "instances_%s2014.json" % ("train" if split == "train" else "val")))
    shutil.copy(os.path.join(FIXTURE, "categories.txt"), os.path.join(root, "categories.txt"))
    with open(os.path.join(root, split, "filenames.pickle"), "wb") as f:
        pickle.dump(list(names if names is not None else keys()), f, protocol=2)
    return root


def flatten(insanns, names):
    """{'<image index>/<field>': array}: every key of every annotation dictionary; a list becomes '<field>/<n>' entries
    plus '<field>:len', None becomes '<field>:none'"""
    flat = {}
    assert sorted(insanns) == sorted(names)
    for i, key in enumerate(names):
        for field, v in insanns[key].items():
            name = "%d/%s" % (i, field)
            if v is None:
                flat[name + ":none"] = np.array(1)
            elif isinstance(v, list):
                flat[name + ":len"] = np.array(len(v))
                for n, a in enumerate(v):
                    flat["%s/%d" % (name, n)] = np.asarray(a)
            else:
                flat[name] = np.asarray(v)
    return flat


def assert_same(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(set(got) ^ set(want)))
    for name in sorted(want):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, float(np.abs(g.astype(np.float64) - w.astype(np.float64)).max()))


def fixture_instances():
    """[(clipped rings, H, W)] of every non-crowd annotation of the fixture, in file order"""
    with open(os.path.join(FIXTURE, "instances_val2014.json")) as f:
        ds = json.load(f)
    sizes = {im["id"]: (im["height"], im["width"]) for im in ds["images"]}
    out = []
    for a in ds["annotations"]:
        if a["iscrowd"] == 0:
            H, W = sizes[a["image_id"]]
            out.append(([np.clip(np.array(r, dtype=np.float64), 0, max(H, W) - 1) for r in a["segmentation"]], H, W))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the reference under stubs
# ---------------------------------------------------------------------------------------------------------------------
def reference_available():
    return os.path.isdir(os.path.join(REFERENCE, "image_generation")) and os.path.isdir(os.path.join(REFERENCE, "shape_generation"))


def _polygon(r, c, shape=None):
    """skimage.draw.polygon(r, c): the pixels of the vertices' bounding box (from 0) that skimage's point_in_polygon
    accepts, tested one comparison per pixel and edge"""
    r, c = np.asarray(r, dtype=np.float64), np.asarray(c, dtype=np.float64)
    minr, maxr = int(max(0, r.min())), int(np.ceil(r.max()))
    minc, maxc = int(max(0, c.min())), int(np.ceil(c.max()))
    if shape is not None:
        maxr, maxc = min(shape[0] - 1, maxr), min(shape[1] - 1, maxc)
    rr, cc = np.mgrid[minr:maxr + 1, minc:maxc + 1]
    y, x = rr.astype(np.float64), cc.astype(np.float64)
    inside = np.zeros(rr.shape, dtype=bool)
    j = len(r) - 1
    for i in range(len(r)):
        if r[i] != r[j]:
            hit = ((r[i] <= y) & (y < r[j])) | ((r[j] <= y) & (y < r[i]))
            hit &= x < (c[j] - c[i]) * (y - r[i]) / (r[j] - r[i]) + c[i]
            inside ^= hit
        j = i
    return rr[inside], cc[inside]


def _resize(image, output_shape, **kwargs):
    """skimage.transform.resize(image, output_shape) of a 2-D float image with the defaults of skimage >= 0.19"""
    from scipy import ndimage as ndi
    assert not kwargs
    image = np.asarray(image, dtype=np.float64)
    output_shape = tuple(int(s) for s in output_shape)
    if image.shape == output_shape:
        return image.copy()
    factors = np.divide(image.shape, output_shape)
    filtered = image
    if any(o < i for o, i in zip(output_shape, image.shape)):
        filtered = ndi.gaussian_filter(image, np.maximum(0, (factors - 1) / 2), cval=0, mode="mirror")
    out = ndi.zoom(filtered, [1 / f for f in factors], order=1, mode="mirror", cval=0, grid_mode=True)
    return np.clip(out, image.min(), image.max())


class _Permissive(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: (_ for _ in ()).throw(RuntimeError("%s.%s is stubbed" % (self.__name__, name)))


class _AttrDict(dict):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        for key, v in list(self.items()):
            if isinstance(v, dict):
                self[key] = _AttrDict(v)
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _stubs(json_path):
    with open(json_path) as f:
        sizes = {im["file_name"].split(".")[0]: (im["height"], im["width"]) for im in json.load(f)["images"]}

    def imread(path):
        h, w = sizes[os.path.basename(path).split(".")[0]]
        return np.zeros((h, w, 3), dtype=np.uint8)

    mods = {}

    def mod(name, cls=types.ModuleType, **attrs):
        m = cls(name)
        m.__dict__.update(attrs)
        mods[name] = m
        parent, _, leaf = name.rpartition(".")
        if parent:
            setattr(mods[parent], leaf, m)
        return m
    mod("skimage")
    mod("skimage.draw", polygon=_polygon)
    mod("skimage.transform", resize=_resize)
    mod("skimage.io", imread=imread)
    mod("nltk")
    mod("nltk.tokenize", RegexpTokenizer=object)
    mod("torchtext", _Permissive)
    mod("spacy", load=lambda name: None)
    mod("torchvision", _Permissive)
    mod("torchvision.transforms", _Permissive)
    mod("easydict", EasyDict=_AttrDict)
    mod("models")
    mod("models.roi_align")
    mod("models.roi_align.modules")
    mod("models.roi_align.modules.roi_align", RoIAlignAvg=object)
    return mods


_OWN = ("miscc", "pycocotools", "datasets", "models")


@contextlib.contextmanager
def _reference_imports(root, json_path):
    """sys.modules and sys.path as the reference's stage under `root` needs them; both restored afterwards (the product
    package uses the same top-level names)"""
    os.environ.setdefault("MPLBACKEND", "Agg")
    np.int, np.float = int, float
    stubs = _stubs(json_path)
    stubs["pycocotools._mask"] = _Permissive("pycocotools._mask")

    def ours(n):
        return n.split(".")[0] in _OWN
    saved = {n: sys.modules.pop(n) for n in list(sys.modules) if ours(n) or n in stubs}
    saved_path = list(sys.path)
    pkg = os.path.join(os.path.dirname(HERE), "obj-gan_amd")
    try:
        sys.modules.update(stubs)
        sys.path = [root] + [p for p in sys.path if os.path.abspath(p or ".") != pkg]
        yield
    finally:
        sys.path = saved_path
        for n in list(sys.modules):
            if ours(n) or n in stubs:
                del sys.modules[n]
        sys.modules.update(saved)


def reference_gt(data_dir, names, split="test"):
    json_path = os.path.join(data_dir, "insanns", "instances_%s2014.json" % ("train" if split == "train" else "val"))
    with _reference_imports(os.path.join(REFERENCE, "image_generation"), json_path):
        import miscc.load as ref_load
        return ref_load.load_gt_insanns(data_dir, list(names), split, list(IMSIZE), FMSIZE, cats_index_dict())


def reference_shape(data_dir, names, split="test"):
    json_path = os.path.join(data_dir, "insanns", "instances_%s2014.json" % ("train" if split == "train" else "val"))
    with _reference_imports(os.path.join(REFERENCE, "shape_generation"), json_path):
        import datasets as ref_datasets
        fake = types.SimpleNamespace(imsize=IMSIZE[0], fmsize=FMSIZE, cats_index_dict=cats_index_dict())
        return ref_datasets.TextDataset.load_insanns(fake, data_dir, list(names), split)


def record():
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        data_dir = make_data_dir(tmp)
        for kind, fn in (("gt", reference_gt), ("shape", reference_shape)):
            flat = flatten(fn(data_dir, keys()), keys())
            np.savez_compressed(RECORDED[kind], **flat)
            print("wrote %s: %d arrays, %d bytes" % (RECORDED[kind], len(flat), os.path.getsize(RECORDED[kind])))


if __name__ == "__main__":
    record()

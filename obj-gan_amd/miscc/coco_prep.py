"""The instance-annotation pickles from COCO's own JSON (reference image_generation/miscc/load.py:502-651
`load_gt_insanns` -> `<split>_gt_insanns.pickle`, shape_generation/datasets.py:241-391 `load_insanns` ->
`<split>_shape_insanns.pickle`), without pycocotools, skimage or an image file:

  <data_dir>/insanns/instances_<train|val>2014.json      the COCO instance annotations ('test' reads val2014)

Per image, in the reference's order: the non-crowd annotations, the ROI_MIN_SIZE filter on the scaled box, the
BOXES_NUM largest boxes (np.argsort(...)[::-1], as miscc.utils.calc_sort_size), rois and fm_rois, per kept instance
the polygon clipped to [0, max(H, W) - 1], rasterised at image size and resized to S x S, the pooled mask, and the
two stacks of box maps.  The two loaders differ in three places, all kept: `rois` (three per-branch arrays | one
array), `fm_rois` (rois[0] / 2 | its own feature-map scales) and the feature-map bounds (halved again | not); `masks`
is a list in the first and an array in the second; and each runs under its own configuration: ROI_MIN_SIZE is 10 at the
256-pixel scale for the image generator and 2 at the 64-pixel scale for the shape generator.

Two things the reference does by accident are kept too, since its output is what these files have to hold:
  * after the BOXES_NUM selection its `kept_indices` are positions in the FILTERED box list, yet they index the
    unfiltered annotation list: when the filter dropped a box of an image with more than BOXES_NUM boxes, the masks
    belong to other annotations than the boxes;
  * the clip bound is max(H, W) - 1 on both axes.
What differs: height and width come from the JSON's image record (the reference opens the JPEG for them), an
annotation whose segmentation is run-length encoded is refused with a ValueError (the reference crashes in
segToMask), and polygon pixels beyond the image are ignored (the reference raises IndexError there).

THIRD-PARTY ARITHMETIC, restated: `COCO.segToMask` is `skimage.draw.polygon(y, x)` per ring, OR-ed; skimage's
`point_in_polygon` is the crossing-number test in float64 at integer pixel coordinates -- pixel (x, y) toggles for
every edge (i, j = i - 1) with

    ((yp[i] <= y && y < yp[j]) || (yp[j] <= y && y < yp[i]))  &&
    x < (xp[j] - xp[i]) * (y - yp[i]) / (yp[j] - yp[i]) + xp[i]

and is inside when it toggled an odd number of times.  `skimage.transform.resize` is `load.resize_mask` (scipy.ndimage).

Masks are made on the host (numpy + scipy, `device=None`) or in batches on the GPU (`objgan_hip.ops.poly_masks`,
csrc/coco_masks.hip: bit for bit the host route).  Selection, rois and box maps are the reference's own numpy calls on
the host in both routes.
"""
import json
import os

import numpy as np

from miscc.config import cfg
from miscc.load import resize_mask

BATCH = 64          # images per device call
# the shape generator's own configuration (reference shape_generation/miscc/config.py:61); cfg.ROI.ROI_MIN_SIZE is the
# image generator's 10
SHAPE_ROI_MIN_SIZE = 2


def annotation_file(data_dir, split):
    return os.path.join(data_dir, 'insanns', 'instances_%s2014.json' % ('train' if split == 'train' else 'val'))


def read_instances(json_path):
    """-> (images: name -> image record, anns: image id -> annotations in file order); the name is the file name up
    to its first dot, as pycocotools' index has it"""
    with open(json_path, 'r') as f:
        dataset = json.load(f)
    images = {im['file_name'].split('.')[0]: im for im in dataset.get('images', [])}
    anns = {}
    for ann in dataset.get('annotations', []):
        anns.setdefault(ann['image_id'], []).append(ann)
    return images, anns


def polygon_mask(rings, H, W):
    """bool [H, W]: `COCO.segToMask(rings, H, W)`, rings as flat [x0, y0, x1, y1, ...] lists.  The abscissa of an edge's
    crossing with row y does not depend on x, and for integer x `x < a` is `x < ceil(a)`: an edge toggles the prefix
    [0, ceil(a)) of the row, so the parity of a row is a running XOR over its toggle points."""
    out = np.zeros((H, W), dtype=bool)
    y = np.arange(H, dtype=np.float64)[:, None]
    for ring in rings:
        s = np.asarray(ring, dtype=np.float64)
        if s.ndim != 1 or s.size % 2:
            raise ValueError("polygon_mask: a ring is a flat list of x, y pairs")
        if s.size == 0:
            continue
        xi, yi = s[0::2][None, :], s[1::2][None, :]
        xj, yj = np.roll(xi, 1, axis=1), np.roll(yi, 1, axis=1)
        straddles = ((yi <= y) & (y < yj)) | ((yj <= y) & (y < yi))
        with np.errstate(divide='ignore', invalid='ignore'):
            cross = (xj - xi) * (y - yi) / (yj - yi) + xi
        rows, edges = np.nonzero(straddles)
        k = np.clip(np.ceil(cross[rows, edges]), 0, W).astype(np.int64)
        toggles = np.zeros((H, W + 1), dtype=np.int64)
        np.add.at(toggles, (rows, k), 1)                   # pixels [0, k) toggle: parity(x) = #(k > x) mod 2
        above = toggles.sum(axis=1, keepdims=True) - np.cumsum(toggles, axis=1)
        out |= (above[:, :W] & 1).astype(bool)
    return out


def _rings_of(ann, key):
    seg = ann['segmentation']
    if not isinstance(seg, list):
        raise ValueError("%s: annotation %s has a run-length encoded segmentation, which only crowd annotations "
                         "carry in COCO; it cannot be rasterised as a polygon" % (key, ann.get('id')))
    return seg


def _select(key, images, anns, last_scale_size, R, cats_index_dict, min_size):
    """steps 2-7 of the reference loop -> None (no box) or (H, W, raw_rois [n, 6], annotations of the kept boxes)"""
    if key not in images:
        raise KeyError("%s is not an image of the annotation file" % key)
    im = images[key]
    noncrowd = [a for a in anns.get(im['id'], []) if a['iscrowd'] == 0]
    if len(noncrowd) == 0:
        return None
    H, W = int(im['height']), int(im['width'])
    scale_h, scale_w = np.float64(last_scale_size / float(H)), np.float64(last_scale_size / float(W))
    raw_rois = np.zeros((len(noncrowd), 6))
    kept = []
    for i, ann in enumerate(noncrowd):
        bbox_width, bbox_height = ann['bbox'][2:4]
        if scale_w * bbox_width < min_size and scale_h * bbox_height < min_size:
            continue
        raw_rois[len(kept), :4] = ann['bbox']
        raw_rois[len(kept), 4] = cats_index_dict[ann['category_id']]
        kept.append(i)
    raw_rois = raw_rois[:len(kept)]
    if len(kept) == 0:
        return None
    if len(kept) > R:                                          # utils.calc_sort_size
        order = np.argsort(np.multiply(raw_rois[:, 2], raw_rois[:, 3]))[::-1].tolist()
        raw_rois = raw_rois[order, :][:R, :]
        kept = order[:R]                                       # (positions in the filtered list: see the module docstring)
    return H, W, raw_rois, [noncrowd[i] for i in kept]


def _clipped_rings(ann, key, H, W):
    top = max(H, W) - 1
    rings = []
    for ring in _rings_of(ann, key):
        if len(ring) % 2:
            raise ValueError("%s: annotation %s has a ring with an odd number of coordinates" % (key, ann.get('id')))
        rings.append(np.clip(np.array(ring, dtype=np.float64), 0, top))
    return rings


def instance_masks(instances, S, device=None):
    """instances: [(rings, H, W)] with clipped rings -> float64 [n, S, S] numpy: rasterised at H x W and resized to S x S.
    With a device, what csrc/coco_masks.hip covers goes through one `ops.poly_masks` call; what it refuses (a side or a
    filter radius beyond its caps) takes the host route here, like everything when device is None."""
    out = np.zeros((len(instances), S, S))
    on_dev = []
    if device is not None:
        from objgan_hip import ops
        on_dev = [i for i, (_, H, W) in enumerate(instances) if ops.poly_masks_covers(H, W, S)]
    taken = set(on_dev)
    for i, (rings, H, W) in enumerate(instances):
        if i not in taken:
            out[i] = resize_mask(polygon_mask(rings, H, W).astype(float), S)
    if on_dev:
        verts, ring_off, inst_ring = [], [0], [0]
        for i in on_dev:
            for ring in instances[i][0]:
                if ring.size:
                    verts.append(ring.reshape(-1, 2))
                    ring_off.append(ring_off[-1] + ring.size // 2)
            inst_ring.append(len(ring_off) - 1)
        verts = np.concatenate(verts) if verts else np.zeros((0, 2))
        got = ops.poly_masks(verts, ring_off, inst_ring, [instances[i][1] for i in on_dev],
                             [instances[i][2] for i in on_dev], S, device)
        out[on_dev] = got.cpu().numpy()
    return out


def _empty(rois, fm_rois):
    return {'rois': rois, 'fm_rois': fm_rois, 'masks': None, 'pooled masks': None, 'bbox maps': None,
            'bbox fmaps': None, 'num_rois': 0}


def _box_maps(boxes, size):
    """[n, size, size]: rows y .. y + h, columns x .. x + w of each (x, y, w, h), rounded and cut to size - 1"""
    maps = np.zeros((boxes.shape[0], size, size))
    for r in range(boxes.shape[0]):
        x_start = min(int(round(boxes[r, 0])), size - 1)
        y_start = min(int(round(boxes[r, 1])), size - 1)
        x_end = min(int(round(boxes[r, 0] + boxes[r, 2])), size - 1)
        y_end = min(int(round(boxes[r, 1] + boxes[r, 3])), size - 1)
        maps[r, y_start:y_end, x_start:x_end] = 1
    return maps


def _build(data_dir, filenames, split, S, select_size, min_size, cats_index_dict, device, assemble, batch=None):
    images, anns = read_instances(annotation_file(data_dir, split))
    R = cfg.ROI.BOXES_NUM
    batch = int(batch or BATCH)
    insanns_dict = {}
    for start in range(0, len(filenames), batch):
        if start % 512 == 0:
            print('%07d / %07d' % (start, len(filenames)))
        chosen, instances = [], []
        for key in filenames[start:start + batch]:
            sel = _select(key, images, anns, select_size, R, cats_index_dict, min_size)
            chosen.append((key, sel))
            if sel is not None:
                H, W, _, kept_anns = sel
                instances.extend((_clipped_rings(a, key, H, W), H, W) for a in kept_anns)
        masks = instance_masks(instances, S, device)
        at = 0
        for key, sel in chosen:
            if sel is None:
                insanns_dict[key] = assemble(None, None, None, None)
                continue
            H, W, raw_rois, _ = sel
            n = raw_rois.shape[0]
            insanns_dict[key] = assemble(H, W, raw_rois, masks[at:at + n])
            at += n
    return insanns_dict


def build_gt_insanns(data_dir, filenames, split, imsize, fmsize, cats_index_dict, device=None, batch=None):
    """The dictionary of the reference's `load_gt_insanns` (image generator), key for key and dtype for dtype."""
    print('creating %s gt_insanns' % split)
    nb, R, D = cfg.TREE.BRANCH_NUM, cfg.ROI.BOXES_NUM, cfg.ROI.BOXES_DIM

    def assemble(H, W, raw_rois, masks):
        rois = [np.zeros(shape=(R, D)) for _ in range(nb)]
        fm_rois = np.zeros(shape=(R, D))
        if raw_rois is None:
            return _empty(rois, fm_rois)
        num_rois = raw_rois.shape[0]
        for b in range(nb):
            scale_h, scale_w = np.float64(imsize[b] / float(H)), np.float64(imsize[b] / float(W))
            rois[b][:num_rois, :] = raw_rois
            rois[b][:, [0, 2]] = rois[b][:, [0, 2]] * scale_w
            rois[b][:, [1, 3]] = rois[b][:, [1, 3]] * scale_h
        fm_rois[:num_rois, :] = rois[0][:num_rois, :].copy()
        fm_rois[:, :4] = fm_rois[:, :4] / 2.0
        raw_masks = [masks[r].copy() for r in range(num_rois)]
        return {'rois': rois, 'fm_rois': fm_rois, 'masks': raw_masks, 'pooled masks': np.amax(raw_masks, axis=0),
                'bbox maps': _box_maps(rois[0][:num_rois, :4], imsize[0]),
                'bbox fmaps': _box_maps(fm_rois[:num_rois, :4] / 2.0, fmsize),        # 32 -> 16, halved again
                'num_rois': num_rois}

    return _build(data_dir, filenames, split, imsize[0], imsize[nb - 1], cfg.ROI.ROI_MIN_SIZE,
                  cats_index_dict, device, assemble, batch)


def build_shape_insanns(data_dir, filenames, split, imsize, fmsize, cats_index_dict, device=None, batch=None):
    """The dictionary of the reference's `load_insanns` (shape generator): `imsize` is one number there."""
    print('creating %s insanns' % split)
    R, D = cfg.ROI.BOXES_NUM, cfg.ROI.BOXES_DIM

    def assemble(H, W, raw_rois, masks):
        rois = np.zeros(shape=(R, D))
        fm_rois = np.zeros(shape=(R, D))
        if raw_rois is None:
            return _empty(rois, fm_rois)
        num_rois = raw_rois.shape[0]
        scales = np.array([imsize / float(H), imsize / float(W)])
        fm_scales = np.array([fmsize / float(H), fmsize / float(W)])
        rois[:num_rois, :] = raw_rois
        rois[:, [0, 2]] = rois[:, [0, 2]] * scales[1]
        rois[:, [1, 3]] = rois[:, [1, 3]] * scales[0]
        fm_rois[:num_rois, :] = raw_rois
        fm_rois[:, [0, 2]] = fm_rois[:, [0, 2]] * fm_scales[1]
        fm_rois[:, [1, 3]] = fm_rois[:, [1, 3]] * fm_scales[0]
        raw_masks = np.zeros((num_rois, imsize, imsize))
        raw_masks[:] = masks
        return {'rois': rois, 'fm_rois': fm_rois, 'masks': raw_masks, 'pooled masks': np.amax(raw_masks, axis=0),
                'bbox maps': _box_maps(rois[:num_rois, :4], imsize), 'bbox fmaps': _box_maps(fm_rois[:num_rois, :4], fmsize),
                'num_rois': num_rois}

    return _build(data_dir, filenames, split, imsize, imsize, SHAPE_ROI_MIN_SIZE,
                  cats_index_dict, device, assemble, batch)


def default_device():
    """cuda:0 when a GPU is present, else None (the host route)"""
    import torch
    return torch.device('cuda:0') if torch.cuda.is_available() else None

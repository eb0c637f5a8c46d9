"""Data set of the shape generator's training (reference shape_generation/datasets.py:31-72, 90-114, 393-413, 453-545).

Reads what the reference's preparation left in the data directory -- `<split>_shape_insanns.pickle` (per image: rois,
fm_rois, instance masks, pooled mask, box maps at 64x64 and 16x16, num_rois), `<split>/filenames.pickle`,
`captions.pickle` (for the word index of the category names) and `categories.txt`.  The annotation pickle is built
from `<data_dir>/insanns/instances_<train|val>2014.json` when it is missing (miscc/coco_prep.py: the reference's
`load_insanns` without pycocotools and skimage, masks on the GPU when there is one); the others are only read.

An item is the reference's minus the image (only its display path reads it: `images_for` fetches the images of a
batch's keys from `<split>_imgs.bigfile` when a grid is drawn), and with the box maps in their compact
form: the raw per-box maps [BOXES_NUM, S, S] and the category of each slot.  `prepare_data` uploads those kilobytes and
writes the one-hot `bbox_maps_fwd` / `bbox_maps_bwd` [B, R, nbf, S, S] on the device (`ops.boxmaps_onehot`);
`get_hmaps_rois` is the reference's host form of the same tensors.  The reference's quirk is kept: the backward
sequence is the forward one reversed over ALL BOXES_NUM slots and only then cut to the batch's largest box count, so an
image with fewer than BOXES_NUM boxes sees leading zero maps there.
"""
import csv
import os
import pickle
import re

import numpy as np
import torch
import torch.utils.data as data

from miscc.config import cfg
from objgan_hip import ops


def get_hmaps_rois(anno_dict, hmap_size, fmap_size, cats_index_dict):
    """the reference's host tensors of one image (datasets.py:90-114), float64 like there"""
    rois, fm_rois, num_rois = anno_dict['rois'], anno_dict['fm_rois'], int(anno_dict['num_rois'])
    nb, nc = cfg.ROI.BOXES_NUM, len(cats_index_dict)
    hmaps = np.zeros((nb, hmap_size, hmap_size))
    bbox_maps_fwd = np.zeros((nb, nc, hmap_size, hmap_size))
    bbox_maps_bwd = np.zeros((nb, nc, hmap_size, hmap_size))
    bbox_fmaps = np.zeros((nb, fmap_size, fmap_size))
    pooled_hmaps = np.zeros((hmap_size, hmap_size))
    if num_rois > 0:
        hmaps[:num_rois] = anno_dict['masks']
        pooled_hmaps = anno_dict['pooled masks'].copy()
        for r in range(num_rois):
            bbox_maps_fwd[r, int(rois[r, 4])] = anno_dict['bbox maps'][r]
        bbox_maps_bwd = bbox_maps_fwd[::-1].copy()
        bbox_fmaps[:num_rois] = anno_dict['bbox fmaps']
    return pooled_hmaps, hmaps, bbox_maps_fwd, bbox_maps_bwd, bbox_fmaps, rois, fm_rois, num_rois


def compact_item(anno_dict, hmap_size, fmap_size):
    """-> pooled_hmaps [S, S], hmaps [NB, S, S], raw box maps [NB, S, S], categories [NB] (int32; 0 in unused slots),
    bbox_fmaps [NB, fm, fm], rois, fm_rois, num_rois: fp32, what `prepare_data` uploads"""
    rois, num_rois = anno_dict['rois'], int(anno_dict['num_rois'])
    nb = cfg.ROI.BOXES_NUM
    hmaps = np.zeros((nb, hmap_size, hmap_size), np.float32)
    raw = np.zeros((nb, hmap_size, hmap_size), np.float32)
    fmaps = np.zeros((nb, fmap_size, fmap_size), np.float32)
    pooled = np.zeros((hmap_size, hmap_size), np.float32)
    cats = np.zeros((nb,), np.int32)
    if num_rois > 0:
        hmaps[:num_rois] = anno_dict['masks']
        pooled[:] = anno_dict['pooled masks']
        raw[:num_rois] = anno_dict['bbox maps']
        fmaps[:num_rois] = anno_dict['bbox fmaps']
        cats[:num_rois] = np.asarray(rois)[:num_rois, 4].astype(np.int32)
    return pooled, hmaps, raw, cats, fmaps, np.asarray(rois), np.asarray(anno_dict['fm_rois']), num_rois


def prepare_data(batch, device, num_classes):
    """A collated batch -> the tensors of one training step on `device` (reference prepare_data, datasets.py:31-72):
    everything cut to the batch's largest box count, which is read from the HOST copy of num_rois."""
    pooled, hmaps, raw, cats, fmaps, rois, fm_rois, num_rois, class_ids, keys = batch
    R = int(num_rois.max())
    if R < 1:
        raise ValueError("shapeDataset.prepare_data: no image of the batch has a box (the reference's step fails there too)")
    num_dev = num_rois.to(torch.int32).to(device)
    fwd, bwd = ops.boxmaps_onehot(raw.float().to(device), cats.to(torch.int32).to(device), num_dev, R, num_classes)
    return {"pooled_hmaps": pooled.float().unsqueeze(1).to(device),
            "hmaps": hmaps[:, :R].float().unsqueeze(2).contiguous().to(device),
            "bbox_maps_fwd": fwd, "bbox_maps_bwd": bwd,
            "bbox_fmaps": fmaps[:, :R].float().contiguous().to(device),
            "rois": rois.numpy(), "fm_rois": fm_rois, "num_rois": num_rois, "max_num_roi": R,
            "class_ids": np.asarray(class_ids), "keys": list(keys)}


class TextDataset(data.Dataset):
    def __init__(self, data_dir, split='train', base_size=64):
        self.imsize = base_size
        self.fmsize = cfg.ROI.FM_SIZE
        self.data_dir = data_dir
        self.split = split
        self.filenames = self.load_filenames(data_dir, split)
        self.ixtoword, self.wordtoix = self.load_dictionary(data_dir)
        self.n_words = len(self.ixtoword)
        self.class_id = self.load_class_id(os.path.join(data_dir, split), len(self.filenames))
        self.cats_dict, self.cats_index_dict = self.load_cats()
        self.insanns_dict = self.load_anns_data(data_dir, split, self.filenames, self.imsize, self.fmsize,
                                                self.cats_index_dict)
        self._img_bytes = self._img_index = None

    @staticmethod
    def load_filenames(data_dir, split):
        path = os.path.join(data_dir, split, 'filenames.pickle')
        if not os.path.isfile(path):
            raise IOError("%s not found" % path)
        with open(path, 'rb') as f:
            return pickle.load(f)

    @staticmethod
    def load_dictionary(data_dir):
        path = os.path.join(data_dir, 'captions.pickle')
        if not os.path.isfile(path):
            raise IOError("%s not found: the caption dictionary is built by the reference's preparation" % path)
        with open(path, 'rb') as f:
            x = pickle.load(f)
        return x[2], x[3]

    @staticmethod
    def load_class_id(split_dir, total_num):
        path = os.path.join(split_dir, 'class_info.pickle')
        if os.path.isfile(path):
            with open(path, 'rb') as f:
                return pickle.load(f)
        return np.arange(total_num)

    def load_cats(self):
        """categories.txt: `<category id>,<name>` per line -> (index -> word ids of the name, category id -> index)"""
        cats_dict, cats_index_dict = {}, {}
        with open(os.path.join(self.data_dir, 'categories.txt'), newline='') as f:
            rows = [r for r in csv.reader(f) if r]
        for i, row in enumerate(rows):
            tokens = [t.encode('ascii', 'ignore').decode('ascii') for t in re.findall(r'\w+', row[1].lower())]
            cats_dict[i] = [self.wordtoix[t] for t in tokens if len(t) > 0]
            cats_index_dict[int(row[0])] = i
        return cats_dict, cats_index_dict

    @staticmethod
    def load_anns_data(data_dir, split, filenames=None, imsize=None, fmsize=None, cats_index_dict=None):
        path = os.path.join(data_dir, '%s_shape_insanns.pickle' % split)
        if not os.path.isfile(path):
            from miscc import coco_prep
            if filenames is None or not os.path.isfile(coco_prep.annotation_file(data_dir, split)):
                raise IOError("%s not found, and no %s to build it from (prepare_data.py)"
                              % (path, coco_prep.annotation_file(data_dir, split)))
            insanns_dict = coco_prep.build_shape_insanns(data_dir, filenames, split, imsize, fmsize, cats_index_dict,
                                                         device=coco_prep.default_device())
            with open(path, 'wb') as f:
                pickle.dump([insanns_dict], f, protocol=2)
            print('Save to: ', path)
            return insanns_dict
        with open(path, 'rb') as f:
            return pickle.load(f)[0]

    # ---- the images: read by the display path only, so never part of an item ----
    def imgs_path(self):
        return os.path.join(self.data_dir, '%s_imgs.bigfile' % self.split)

    def __getstate__(self):
        # (a loader worker gets the data set without the open bigfile: a memory map does not pickle)
        return dict(self.__dict__, _img_bytes=None, _img_index=None)

    def has_images(self):
        """whether <split>_imgs.bigfile exists (it is never written from here)"""
        return os.path.isfile(self.imgs_path())

    def images_for(self, keys):
        """-> [n, 3, imsize, imsize] in [-1, 1]: the images of `keys` as the reference's item holds them (datasets.py:74-88:
        Pillow's bilinear resize, ToTensor, Normalize 0.5), read from <split>_imgs.bigfile, which is opened at the first
        call"""
        from miscc import load
        if self._img_bytes is None:
            if not self.has_images():
                raise IOError("%s not found" % self.imgs_path())
            self._img_bytes = load.load_imgs_data(self.data_dir, self.split, self.filenames)
            self._img_index = {k: i for i, k in enumerate(self.filenames)}
        return torch.stack([load.get_imgs(self._img_bytes[self._img_index[k]], [self.imsize], branch_num=1)[0]
                            for k in keys])

    def __getitem__(self, index):
        key = self.filenames[index]
        return compact_item(self.insanns_dict[key], self.imsize, self.fmsize) + (self.class_id[index], key)

    def __len__(self):
        return len(self.filenames)

"""Evaluation dataset over a prepared Obj-GAN data directory and the batch hand-over to the evaluator
(reference image_generation/testDataset.py): same class, same item tuples and the same `prepare_*` return
lists, element for element.

  cfg.TEST.USE_GT_BOX_SEG 0 / 1   ground-truth boxes (<split>_gt_insanns.pickle): the 17-tuple, `prepare_data`
  cfg.TEST.USE_GT_BOX_SEG 2       generated boxes, one layout per caption (<split>_gen_insanns.pickle): the
                                  14-tuple, `prepare_gen_data`
  no <split>_acts_tf0.pickle yet  (imgs, key), `prepare_acts_data`: the pass of evaluator.dump_fid_acts

The caption of an item is drawn with numpy.random exactly where the reference draws it, so a seeded run picks
the same captions.  Tensors move to `device` as in trainDataset.prepare_data (None keeps them on the host).
"""
import os

import numpy.random as random
import torch
import torch.utils.data as data

from miscc.config import cfg
from miscc.utils import attach_host
from miscc.load import (load_filenames, load_text_data, load_sample_filenames, load_glove_emb, load_cat_label,
                        load_class_id, load_cats, load_imgs_data, load_acts_data, load_anns_data, get_imgs,
                        get_caption, get_hmaps_rois, get_gen_rois)


# cfg.TEST.USE_GT_BOX_SEG -> (annotation file suffix, annotation kind, attribute the reference class keeps it under)
_LAYOUT_SOURCES = {0: ('_gt_insanns.pickle', 'gt', 'insanns_gt_dict'),
                   1: ('_gt_insanns.pickle', 'gt', 'insanns_gt_dict'),
                   2: ('_gen_insanns.pickle', 'gen', 'insanns_gen_dict')}


class TestDataset(data.Dataset):
    """Attributes follow the reference class (the evaluator reads them): filenames, captions, ixtoword / wordtoix /
    n_words, glove_*, cat_labels / cat_label_lens / sorted_cat_label_indices, class_id, cats_dict / cats_index_dict,
    img_bytes, acts_dict (None until the activation file exists) and insanns_gt_dict or insanns_gen_dict."""
    __test__ = False        # a data set, not a test class

    def __init__(self, data_dir, split='test', base_size=64):
        mode = cfg.TEST.USE_GT_BOX_SEG
        if mode not in _LAYOUT_SOURCES:     # the reference prints a line and fails later, on the first item
            raise ValueError("cfg.TEST.USE_GT_BOX_SEG must be 0, 1 (ground-truth layout) or 2 (generated layout), "
                             "got %r" % (mode,))
        self.gt_layout = mode != 2
        self.data_dir = data_dir
        self.embeddings_num = cfg.TEXT.CAPTIONS_PER_IMAGE
        self.imsize = [base_size * (2 ** b) for b in range(cfg.TREE.BRANCH_NUM)]
        self.fmsize = cfg.ROI.FM_SIZE
        names = {s: load_filenames(data_dir, s) for s in ('train', 'test')}
        text = load_text_data(data_dir, split, names['train'], names['test'])
        self.filenames, self.captions, self.ixtoword, self.wordtoix, self.n_words = text
        # a fixed (image, sentence) list replaces the split's file list and the random caption draw
        self.sentids = None
        if cfg.TEST.SAMPLE_VAL:
            self.filenames, self.sentids = load_sample_filenames(data_dir)
        glove = load_glove_emb(data_dir, split, names['train'], names['test'])
        self.glove_captions, self.glove_ixtoword, self.glove_wordtoix, self.glove_embed = glove
        self.cat_labels, self.cat_label_lens, self.sorted_cat_label_indices = \
            load_cat_label(data_dir, self.glove_wordtoix)
        self.number_example = len(self.filenames)
        self.class_id = load_class_id(os.path.join(data_dir, split), self.number_example)
        self.cats_dict, self.cats_index_dict = load_cats(data_dir, self.wordtoix)
        self.num_classes = len(self.cats_index_dict)
        self.img_bytes = load_imgs_data(data_dir, split, self.filenames)
        self.acts_dict = load_acts_data(data_dir, split)
        suffix, kind, attr = _LAYOUT_SOURCES[mode]
        self._layouts = load_anns_data(data_dir, split, suffix, kind, self.filenames, self.imsize, self.fmsize,
                                       self.cats_index_dict)
        setattr(self, attr, self._layouts)

    def __len__(self):
        return self.number_example

    def _sentence(self, index):
        """-> (caption slot within the image, row of the caption tables).  One numpy.random draw per item unless
        the sample list fixes the sentence: the same consumption as the reference."""
        if self.sentids is not None:
            row = self.sentids[index]
            return row % self.embeddings_num, row
        slot = random.randint(0, self.embeddings_num)
        return slot, index * self.embeddings_num + slot

    def __getitem__(self, index):
        """-> (imgs[3], key) while there is no activation file; else the reference item tuple: imgs[3], real FID
        activation, caption ids, GloVe ids, length, [hmaps[3] with ground-truth layout,] the three box-map stacks,
        rois[3], fm_rois, num_rois, [bt_masks[3], fm_bt_masks with ground-truth layout,] class id, key, caption row
        -- 17 entries with ground-truth layout, 14 with generated layout."""
        key = self.filenames[index]
        imgs = get_imgs(self.img_bytes[index], self.imsize)
        if self.acts_dict is None:
            return imgs, key
        slot, row = self._sentence(index)
        head = (imgs, self.acts_dict[key]) + tuple(get_caption(self.captions, self.glove_captions, row))
        tail = (self.class_id[index], key, row)
        sizes = (self.imsize, self.fmsize, self.cats_index_dict)
        if self.gt_layout:
            maps = get_hmaps_rois(self._layouts[key], *sizes)       # hmaps, 3 box maps, rois, fm_rois, n, 2 masks
            return head + tuple(maps) + tail
        return head + tuple(get_gen_rois(self._layouts[key], *sizes, slot)) + tail


class _Mover(object):
    """The moves of one collated batch: every per-sample tensor reordered by caption length (descending,
    `torch.sort` like the reference so ties fall the same way) and sent to `device`."""

    def __init__(self, cap_lens, device):
        self.device = device
        self.lens_sorted, self.order = torch.sort(cap_lens, 0, True)
        self.order_list = self.order.tolist()

    def put(self, t):
        return t if self.device is None else t.to(self.device, non_blocking=True)

    def take(self, t):
        return self.put(t[self.order])

    def take_small(self, t):    # box tables / counts: the host copy stays attached (miscc.utils._host)
        h = t[self.order]
        return h if self.device is None else attach_host(h.to(self.device, non_blocking=True), h)

    def pick(self, seq):
        return [seq[i] for i in self.order_list]

    def lens(self):
        return self.lens_sorted if self.device is None else attach_host(self.put(self.lens_sorted), self.lens_sorted)

    def box_maps(self, num_rois, fwd, bwd, fmaps):
        """the shape generator's inputs, cut to the batch's largest box count, as float32"""
        n = int(torch.max(num_rois))
        return [self.put(t[self.order, :n].float()) for t in (fwd, bwd, fmaps)]


def prepare_data(data, device=None):
    """Collated 17-tuple -> the reference's 17-item list (reference testDataset.py:109-180)."""
    (imgs, acts, captions, glove_captions, cap_lens, hmaps, bbox_maps_fwd, bbox_maps_bwd, bbox_fmaps, rois, fm_rois,
     num_rois, bt_masks, fm_bt_masks, class_ids, keys, sent_ids) = data
    m = _Mover(cap_lens, device)
    num_rois = num_rois[m.order]
    fwd, bwd, fmaps = m.box_maps(num_rois, bbox_maps_fwd, bbox_maps_bwd, bbox_fmaps)
    branches = range(len(imgs))
    return [[m.take(imgs[b]) for b in branches], acts[m.order].numpy(), m.take(captions).squeeze(),
            m.take(glove_captions).squeeze(), m.lens(), [m.take(hmaps[b].float()) for b in branches],
            fwd, bwd, fmaps, [m.take_small(rois[b]) for b in branches], m.take_small(fm_rois),
            num_rois if device is None else attach_host(m.put(num_rois), num_rois),
            [m.take(bt_masks[b].float()) for b in branches], m.take(fm_bt_masks.float()),
            class_ids[m.order].numpy(), m.pick(keys), m.pick(sent_ids)]


def prepare_gen_data(data, device=None):
    """Collated 14-tuple -> the reference's 14-item list (reference testDataset.py:183-244)."""
    (imgs, acts, captions, glove_captions, cap_lens, bbox_maps_fwd, bbox_maps_bwd, bbox_fmaps, rois, fm_rois,
     num_rois, class_ids, keys, sent_ids) = data
    m = _Mover(cap_lens, device)
    num_rois = num_rois[m.order]
    fwd, bwd, fmaps = m.box_maps(num_rois, bbox_maps_fwd, bbox_maps_bwd, bbox_fmaps)
    branches = range(len(imgs))
    return [[m.take(imgs[b]) for b in branches], acts[m.order].numpy(), m.take(captions).squeeze(),
            m.take(glove_captions).squeeze(), m.lens(), fwd, bwd, fmaps,
            [m.take_small(rois[b]) for b in branches], m.take_small(fm_rois),
            num_rois if device is None else attach_host(m.put(num_rois), num_rois),
            class_ids[m.order].numpy(), m.pick(keys), m.pick(sent_ids)]


def prepare_acts_data(data, device=None):
    """(imgs, keys) of the activation pass -> [images per branch on `device`, keys]."""
    imgs, keys = data
    return [[im if device is None else im.to(device, non_blocking=True) for im in imgs], keys]

"""Host-side readers of the reference's on-disk training data (reference image_generation/
miscc/load.py): the pickles and the image bigfile a prepared Obj-GAN data directory holds, and
the per-sample assembly of images, captions, layout maps and box slots.

Same function names, arguments and return values as the reference, restricted to what the
training path reads:

  <data_dir>/train/filenames.pickle, test/filenames.pickle   list of image keys
  <data_dir>/captions.pickle          [train_captions, test_captions, ixtoword, wordtoix]
  <data_dir>/captions_glove.pickle    [train_captions, test_captions, train_vocab, test_vocab]
                                      (the vocabs are torchtext Vocab objects: itos, stoi, vectors)
  <data_dir>/categories.txt           "<coco id>,<name>" per line
  <data_dir>/<split>_imgs.bigfile     for every key: int32 byte count + the JPEG file
  <data_dir>/<split>_gt_insanns.pickle [ {key: {'rois', 'fm_rois', 'masks', 'bbox maps',
                                               'bbox fmaps', 'num_rois', ...}} ]
  <data_dir>/<split>/class_info.pickle optional class ids
  <data_dir>/gen_masks/<key>/<i>/boxes.txt  layouts of the box generator (sample.py), "x,y,w,h,label,0" per line;
                                      <split>_gen_insanns.pickle is built from them when it is missing

  <data_dir>/insanns/instances_<train|val>2014.json  COCO's instance annotations: <split>_gt_insanns.pickle is built
                                      from them when it is missing (miscc/coco_prep.py, prepare_data.py)

Building the caption files from raw COCO (nltk / spacy / torchtext) is preprocessing, not the
training path: where one of them is missing the readers below raise instead of trying.
Third-party arithmetic the reference delegates to
packages that are absent here is restated and named where it happens (PIL bilinear resize for
torchvision.transforms.Resize, scipy.ndimage for skimage.transform.resize): parity of those two
is against the restatement, not against the packages (LAB.md section 6, "data path").
"""
import io
import mmap
import os
import pickle
import re
import struct
import types

import numpy as np
import torch
import torch.nn as nn

from miscc.config import cfg

_WORD = re.compile(r'\w+', re.UNICODE | re.MULTILINE | re.DOTALL)   # nltk RegexpTokenizer(r'\w+')


# ---------------------------------------------------------------------------------------------
# image bigfile (reference load.py:73-95)
# ---------------------------------------------------------------------------------------------
def write_imgs(data_dir, filenames, filepath):
    """Concatenate <data_dir>/images/<key>.jpg into the bigfile: native int32 length + bytes."""
    with open(filepath, 'wb') as wfid:
        for name in filenames:
            with open('%s/images/%s.jpg' % (data_dir, name), 'rb') as fid:
                img_bytes = fid.read()
            wfid.write(struct.pack('i', len(img_bytes)))
            wfid.write(img_bytes)


class BigFile(object):
    """The bigfile as an indexable sequence of byte strings, memory-mapped: the reference reads
    the whole file into a python list (13 GB for COCO train); here only the offset table lives in
    memory and every worker process shares the page cache."""

    def __init__(self, filepath, count):
        self._f = open(filepath, 'rb')
        size = os.fstat(self._f.fileno()).st_size
        self._mm = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ) if size else b''
        offs = np.zeros((count, 2), np.int64)
        pos = 0
        for i in range(count):
            if pos + 4 > size:
                raise ValueError("%s: truncated after %d of %d images" % (filepath, i, count))
            n = struct.unpack_from('i', self._mm, pos)[0]
            if n < 0 or pos + 4 + n > size:
                raise ValueError("%s: bad length %d for image %d" % (filepath, n, i))
            offs[i] = (pos + 4, n)
            pos += 4 + n
        self._offs = offs

    def __len__(self):
        return len(self._offs)

    def __getitem__(self, i):
        start, n = self._offs[i]
        return bytes(self._mm[start:start + n])


def read_imgs(data_dir, filenames, filepath):
    return BigFile(filepath, len(filenames))


def load_imgs_data(data_dir, split, filenames):
    filepath = os.path.join(data_dir, '%s_imgs.bigfile' % split)
    if not os.path.isfile(filepath):
        write_imgs(data_dir, filenames, filepath)
    return read_imgs(data_dir, filenames, filepath)


# ---------------------------------------------------------------------------------------------
# pickles
# ---------------------------------------------------------------------------------------------
class Vocab(object):
    """Stand-in for torchtext.vocab.Vocab when captions_glove.pickle is read without torchtext:
    the three attributes the training path uses are itos, stoi and vectors."""

    def __setstate__(self, state):
        self.__dict__.update(state)

    def __len__(self):
        return len(self.itos)


def _default_unk_index():
    return 0


class _DataUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module.startswith('torchtext'):
            if name == 'Vocab':
                return Vocab
            if name == '_default_unk_index':
                return _default_unk_index
        return super().find_class(module, name)


def _load_pickle(filepath, encoding='ASCII'):
    with open(filepath, 'rb') as f:
        return _DataUnpickler(f, encoding=encoding).load()


def load_filenames(data_dir, split):
    filepath = '%s/%s/filenames.pickle' % (data_dir, split)
    if os.path.isfile(filepath):
        return _load_pickle(filepath)
    return []


def load_text_data(data_dir, split, train_names, test_names):
    filepath = os.path.join(data_dir, 'captions.pickle')
    if not os.path.isfile(filepath):
        raise FileNotFoundError("%s: build it with the reference's preprocessing" % filepath)
    x = _load_pickle(filepath)
    train_captions, test_captions, ixtoword, wordtoix = x[0], x[1], x[2], x[3]
    n_words = len(ixtoword)
    if split == 'train':
        return train_names, train_captions, ixtoword, wordtoix, n_words
    return test_names, test_captions, ixtoword, wordtoix, n_words


def load_glove_emb(data_dir, split, train_names, test_names):
    filepath = os.path.join(data_dir, 'captions_glove.pickle')
    if not os.path.isfile(filepath):
        raise FileNotFoundError("%s: build it with the reference's preprocessing" % filepath)
    x = _load_pickle(filepath)
    captions, vocab = (x[0], x[2]) if split == 'train' else (x[1], x[3])
    glove_embed = nn.Embedding(len(vocab.itos), cfg.TEXT.GLOVE_EMBEDDING_DIM)
    glove_embed.weight.data.copy_(torch.as_tensor(vocab.vectors))
    return captions, vocab.itos, vocab.stoi, glove_embed


def _tokens(text):
    out = []
    for t in _WORD.findall(text.lower()):
        t = t.encode('ascii', 'ignore').decode('ascii')
        if len(t) > 0:
            out.append(t)
    return out


def _category_lines(data_dir):
    with open('%s/categories.txt' % data_dir, "r") as f:
        return [ln for ln in f.read().split('\n') if len(ln) > 0]


def load_cats(data_dir, wordtoix):
    """-> (cats_dict: row -> caption-vocabulary ids of the name, cats_index_dict: coco id -> row)"""
    cats_dict, cats_index_dict = {}, {}
    for i, line in enumerate(_category_lines(data_dir)):
        cid, name = line.split(',', 1)
        cats_dict[i] = [wordtoix[t] for t in _tokens(name)]
        cats_index_dict[int(cid)] = i
    return cats_dict, cats_index_dict


def load_cat_label(data_dir, glove_wordtoix, device=None):
    """GloVe ids of the category names, sorted by name length (descending), plus the permutation
    back to file order (reference load.py:307-354)."""
    cat_labels = []
    for line in _category_lines(data_dir):
        raw = _WORD.findall(line.replace("\ufffd\ufffd", " ").lower())[1:]    # drop the leading id
        tokens = [t for t in (w.encode('ascii', 'ignore').decode('ascii') for w in raw) if len(t) > 0]
        if len(tokens) == 0:
            continue
        cat_labels.append([glove_wordtoix[t] for t in tokens])
    lens = [len(c) for c in cat_labels]
    arr = np.zeros((len(cat_labels), max(lens)), dtype=np.int64)
    for i, c in enumerate(cat_labels):
        arr[i, :len(c)] = c
    cat_labels = torch.from_numpy(arr)
    cat_label_lens = torch.LongTensor(lens)
    sorted_lens, sorted_idx = torch.sort(cat_label_lens, 0, True)
    sorted_labels = cat_labels[sorted_idx]
    _, resorted_idx = torch.sort(sorted_idx, 0, False)
    if device is not None:
        sorted_labels, sorted_lens, resorted_idx = (t.to(device) for t in (sorted_labels, sorted_lens, resorted_idx))
    return sorted_labels, sorted_lens, resorted_idx


def load_class_id(data_dir, total_num):
    path = data_dir + '/class_info.pickle'
    if os.path.isfile(path):
        return _load_pickle(path)
    return np.arange(total_num)


def load_anns_data(data_dir, split, postfix, ann_type, filenames, imsize, fmsize, cats_index_dict):
    filepath = os.path.join(data_dir, '%s%s' % (split, postfix))
    if not os.path.isfile(filepath):
        if ann_type == 'gen' and os.path.isdir(os.path.join(data_dir, 'gen_masks')):
            # layouts written by sample.py (or by the reference's box generator): build the pickle as the reference does
            insanns_dict = load_gen_insanns(data_dir, filenames, split, imsize, fmsize, cats_index_dict)
            with open(filepath, 'wb') as f:
                pickle.dump([insanns_dict], f, protocol=2)
            print('Save to: ', filepath)
            return insanns_dict
        if ann_type == 'gt':
            from miscc import coco_prep
            if os.path.isfile(coco_prep.annotation_file(data_dir, split)):
                # COCO's own instance JSON: build the pickle as the reference does (masks on the GPU when there is one)
                insanns_dict = coco_prep.build_gt_insanns(data_dir, filenames, split, imsize, fmsize, cats_index_dict,
                                                          device=coco_prep.default_device())
                with open(filepath, 'wb') as f:
                    pickle.dump([insanns_dict], f, protocol=2)
                print('Save to: ', filepath)
                return insanns_dict
        raise FileNotFoundError("%s: %s" % (filepath, (
            "run sample.py to write <data_dir>/gen_masks/" if ann_type == 'gen' else
            "put COCO's instances_<train|val>2014.json under <data_dir>/insanns/ (prepare_data.py builds the pickle from it)")))
    return _load_pickle(filepath, encoding='latin1')[0]


def _read_boxes(path):
    """`boxes.txt` rows `x,y,w,h,label,crowd` as integers, fractions dropped toward zero (the reference reads them with
    pandas.read_csv(header=None).astype(int)); None for a missing or empty file."""
    if not (os.path.isfile(path) and os.path.getsize(path) > 0):
        return None
    with open(path) as f:
        rows = [[int(float(v)) for v in ln.split(',')] for ln in f.read().splitlines() if ln.strip()]
    return np.array(rows, dtype=np.int64) if rows else None


def load_gen_insanns(data_dir, filenames, split, imsize, fmsize, cats_index_dict):
    """{key: {caption index: annotation dictionary}} from `<data_dir>/gen_masks/<key>/<i>/boxes.txt` (reference
    load.py:653-776): boxes with both sides under ROI_MIN_SIZE dropped, the BOXES_NUM largest kept, rois per branch
    scale, feature-map rois and the two stacks of box maps; a caption without a usable box has num_rois 0 and no maps."""
    print('creating %s gen_insanns' % split)
    gen_dir = os.path.join(data_dir, 'gen_masks')
    nb, R, D = cfg.TREE.BRANCH_NUM, cfg.ROI.BOXES_NUM, cfg.ROI.BOXES_DIM
    scales = [imsize[b] / float(imsize[-1]) for b in range(nb)]
    insanns_dict = {}
    for key in filenames:
        key_dir = os.path.join(gen_dir, key)
        indices = sorted(int(name) for name in os.listdir(key_dir)) if os.path.isdir(key_dir) else []
        anno_dicts = {}
        for index in indices:
            boxes = _read_boxes(os.path.join(key_dir, str(index), 'boxes.txt'))
            rois = [np.zeros((R, D)) for _ in range(nb)]
            fm_rois = np.zeros((R, D))
            anno = {'rois': rois, 'fm_rois': fm_rois, 'bbox maps': None, 'bbox fmaps': None, 'num_rois': 0}
            anno_dicts[index] = anno
            if boxes is None:
                continue
            keep = [r for r in boxes if not (r[2] < cfg.ROI.ROI_MIN_SIZE and r[3] < cfg.ROI.ROI_MIN_SIZE)]
            if not keep:
                continue
            raw_rois = np.zeros((len(keep), 6))
            for n, r in enumerate(keep):
                raw_rois[n, :4] = r[:4]
                raw_rois[n, 4] = cats_index_dict[int(r[4])]
            if len(keep) > R:                                  # the largest boxes first, as utils.calc_sort_size
                order = np.argsort(np.multiply(raw_rois[:, 2], raw_rois[:, 3]))[::-1].tolist()
                raw_rois = raw_rois[order, :][:R, :]
            num_rois = raw_rois.shape[0]
            for b in range(nb):
                rois[b][:num_rois, :] = raw_rois
                rois[b][:, [0, 2]] = rois[b][:, [0, 2]] * scales[b]
                rois[b][:, [1, 3]] = rois[b][:, [1, 3]] * scales[b]
            fm_rois[:num_rois, :] = rois[0][:num_rois, :].copy()
            fm_rois[:, :4] = fm_rois[:, :4] / 2.0
            maps = np.zeros((num_rois, imsize[0], imsize[0]))
            fmaps = np.zeros((num_rois, fmsize, fmsize))
            for r in range(num_rois):
                x, y, w, h = rois[0][r, :4]
                x0, y0 = min(int(round(x)), imsize[0] - 1), min(int(round(y)), imsize[0] - 1)
                x1, y1 = min(int(round(x + w)), imsize[0] - 1), min(int(round(y + h)), imsize[0] - 1)
                maps[r, y0:y1, x0:x1] = 1
                x, y, w, h = fm_rois[r, :4]
                x0, y0 = min(int(round(x / 2.0)), fmsize - 1), min(int(round(y / 2.0)), fmsize - 1)
                x1 = min(int(round(x / 2.0 + w / 2.0)), fmsize - 1)
                y1 = min(int(round(y / 2.0 + h / 2.0)), fmsize - 1)
                fmaps[r, y0:y1, x0:x1] = 1
            anno.update({'bbox maps': maps, 'bbox fmaps': fmaps, 'num_rois': num_rois})
        insanns_dict[key] = anno_dicts
    return insanns_dict


# ---------------------------------------------------------------------------------------------
# per-sample assembly
# ---------------------------------------------------------------------------------------------
def get_caption(captions, glove_captions, sent_ix):
    """Caption ids and their GloVe ids, truncated to the shorter of the two, zero-padded to
    WORDS_NUM; longer captions keep WORDS_NUM randomly chosen words in order (np.random, like
    the reference load.py:114-140)."""
    sent_caption = np.asarray(captions[sent_ix]).astype('int64')
    sent_glove_caption = np.asarray(glove_captions[sent_ix]).astype('int64')
    n = min(len(sent_caption), len(sent_glove_caption))
    sent_caption, sent_glove_caption = sent_caption[:n], sent_glove_caption[:n]
    W = cfg.TEXT.WORDS_NUM
    x = np.zeros((W, 1), dtype='int64')
    glove_x = np.zeros((W, 1), dtype='int64')
    x_len = n
    if n <= W:
        x[:n, 0] = sent_caption
        glove_x[:n, 0] = sent_glove_caption
    else:
        ix = list(np.arange(n))
        np.random.shuffle(ix)
        ix = np.sort(ix[:W])
        x[:, 0] = sent_caption[ix]
        glove_x[:, 0] = sent_glove_caption[ix]
        x_len = W
    return x, glove_x, x_len


def _normalize_to_tensor(img):
    """transforms.ToTensor() + Normalize((.5,.5,.5), (.5,.5,.5)) of an RGB PIL image."""
    a = np.asarray(img, dtype=np.uint8)
    t = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(torch.float32).div_(255)
    return t.sub_(0.5).div_(0.5)


def decode_rgb(img_bytes):
    """The decoded image as a uint8 [H, W, 3] tensor: the `device_imgs` hand-over of trainDataset (the
    branch sizes are produced on the device, objgan_hip.ops.resize_pil_bilinear)."""
    from PIL import Image
    img = Image.open(io.BytesIO(img_bytes)).convert('RGB')
    return torch.from_numpy(np.array(img, dtype=np.uint8))


def get_imgs(img_bytes, imsize, normalize=None, branch_num=None):
    """Decode and resize to every branch size (torchvision Resize((s, s)) on a PIL image is PIL's
    bilinear resize with its built-in antialiasing).  branch_num: how many of the sizes in `imsize`
    (default cfg.TREE.BRANCH_NUM; the shape stage reads one)."""
    from PIL import Image
    img = Image.open(io.BytesIO(img_bytes)).convert('RGB')
    norm = normalize if normalize is not None else _normalize_to_tensor
    ret = []
    for i in range(cfg.TREE.BRANCH_NUM if branch_num is None else branch_num):
        ret.append(norm(img.resize((imsize[i], imsize[i]), Image.BILINEAR)))
    return ret


def resize_mask(mask, size):
    """skimage.transform.resize(mask, [size, size]) for a 2-D float image with the package's
    defaults (order 1, mode 'reflect', anti-aliasing Gaussian of sigma (s-1)/2 when shrinking by
    s, clip to the input range), restated on scipy.ndimage -- skimage itself is built on the same
    two calls."""
    from scipy import ndimage as ndi
    mask = np.asarray(mask, dtype=np.float64)
    if mask.shape == (size, size):
        return mask.copy()
    factors = (mask.shape[0] / float(size), mask.shape[1] / float(size))
    img = mask
    if max(factors) > 1:
        sigma = tuple(max(0.0, (f - 1) / 2.0) for f in factors)
        img = ndi.gaussian_filter(img, sigma, cval=0, mode='mirror')
    out = ndi.zoom(img, (size / float(mask.shape[0]), size / float(mask.shape[1])), order=1,
                   mode='mirror', cval=0, grid_mode=True)
    return np.clip(out, mask.min(), mask.max())


def get_hmaps_rois(anno_dict, hmap_size, fmap_size, cats_index_dict, with_hmaps=True, with_resized_masks=True):
    """Layout maps (per-category sums of the instance masks), per-slot box masks at every branch
    size and at the 32x32 feature scale, and the box-map tensors of the shape generator
    (reference load.py:152-191).
    with_resized_masks=False (the `device_masks` hand-over of TrainDataset): no host resize at all -- bt_masks[0] carries
    the raw instance masks (the 64-px branch mask IS the raw mask: resizing 64 -> 64 is the identity), the other mask
    arrays are empty ([0, S, S]) and `prepare_data` produces them on the device (objgan_hip.ops.resize_masks)."""
    rois = anno_dict['rois']
    fm_rois = anno_dict['fm_rois']
    raw_masks = anno_dict['masks']
    num_rois = anno_dict['num_rois']
    nb, ncat, R = cfg.TREE.BRANCH_NUM, len(cats_index_dict), cfg.ROI.BOXES_NUM
    hmaps = [np.zeros((ncat, hmap_size[b], hmap_size[b]) if with_hmaps else (0,)) for b in range(nb)]
    if not with_resized_masks:
        if with_hmaps:
            raise ValueError("get_hmaps_rois: the device mask hand-over rebuilds the layout maps on the device too")
        bt_masks = [np.zeros((R, hmap_size[0], hmap_size[0]))] + [np.zeros((0, hmap_size[b], hmap_size[b])) for b in range(1, nb)]
        fm_bt_masks = np.zeros((0, hmap_size[0] // 2, hmap_size[0] // 2))
        for r in range(num_rois):
            m = np.asarray(raw_masks[r], dtype=np.float64)
            if m.shape != (hmap_size[0], hmap_size[0]):
                raise ValueError("get_hmaps_rois: raw instance masks must be %d x %d for the device hand-over, got %s"
                                 % (hmap_size[0], hmap_size[0], m.shape))
            bt_masks[0][r] = m
    else:
        bt_masks = [np.zeros((R, hmap_size[b], hmap_size[b])) for b in range(nb)]
        fm_bt_masks = np.zeros((R, hmap_size[0] // 2, hmap_size[0] // 2))
        for r in range(num_rois):
            mask = raw_masks[r]
            cat = int(rois[0][r, 4])
            fm_bt_masks[r] = resize_mask(mask, hmap_size[0] // 2)
            for b in range(nb):
                re_mask = resize_mask(mask, hmap_size[b])
                bt_masks[b][r] = re_mask
                if with_hmaps:
                    hmaps[b][cat] += re_mask
    bbox_maps_fwd = np.zeros((R, ncat, hmap_size[0], hmap_size[0]))
    bbox_maps_bwd = np.zeros((R, ncat, hmap_size[0], hmap_size[0]))
    bbox_fmaps = np.zeros((R, fmap_size, fmap_size))
    if num_rois > 0:
        for r in range(num_rois):
            bbox_maps_fwd[r, int(rois[0][r, 4])] = anno_dict['bbox maps'][r]
        bbox_maps_bwd = bbox_maps_fwd[::-1].copy()
        bbox_fmaps[:num_rois] = anno_dict['bbox fmaps']
    return hmaps, bbox_maps_fwd, bbox_maps_bwd, bbox_fmaps, rois, fm_rois, num_rois, bt_masks, fm_bt_masks


def get_gen_rois(anno_dicts, hmap_size, fmap_size, cats_index_dict, sent_ix):
    """Box slots and box maps of the GENERATED layout of caption `sent_ix` of an image (reference load.py:194-214;
    `<split>_gen_insanns.pickle` holds one annotation dictionary per caption)."""
    anno = anno_dicts[sent_ix]
    rois, fm_rois, num_rois = anno['rois'], anno['fm_rois'], anno['num_rois']
    R, ncat = cfg.ROI.BOXES_NUM, len(cats_index_dict)
    bbox_maps_fwd = np.zeros((R, ncat, hmap_size[0], hmap_size[0]))
    bbox_maps_bwd = np.zeros((R, ncat, hmap_size[0], hmap_size[0]))
    bbox_fmaps = np.zeros((R, fmap_size, fmap_size))
    if num_rois > 0 and anno['bbox maps'] is not None:
        for r in range(num_rois):
            bbox_maps_fwd[r, int(rois[0][r, 4])] = anno['bbox maps'][r]
        bbox_maps_bwd = bbox_maps_fwd[::-1].copy()
        bbox_fmaps[:num_rois] = anno['bbox fmaps']
    return bbox_maps_fwd, bbox_maps_bwd, bbox_fmaps, rois, fm_rois, num_rois


# ---------------------------------------------------------------------------------------------
# evaluation split
# ---------------------------------------------------------------------------------------------
def acts_filename(split):
    """`<split>_acts_tf<USE_TF>.pickle` with the USE_TF value in effect: there is no TensorFlow route here, so the
    PyTorch file (`_tf0`) is the only one this package writes or reads."""
    return '%s_acts_tf%d.pickle' % (split, 0)


def load_acts_data(data_dir, split):
    """{key: float64 (2048,)} FID activations of the real images of a split, or None when the file is missing
    (reference load.py:465-477; evaluator.dump_fid_acts writes it)."""
    filepath = os.path.join(data_dir, acts_filename(split))
    if not os.path.isfile(filepath):
        print('Error: no such a file %s' % filepath)
        return None
    acts_dict = _load_pickle(filepath, encoding='latin1')[0]
    print('Load from: ', filepath)
    return acts_dict


def load_sample_filenames(data_dir):
    """`<data_dir>/sample/filenames.txt`, one `name,sentid` per line -> (names, sentence ids), for
    cfg.TEST.SAMPLE_VAL.  NOT pinned to the reference: its version (load.py:447-463) opens the file in binary mode
    and calls str.replace on the lines, which raises under Python 3, so there is nothing to compare against; this
    reads the same lines in text mode."""
    filepath = '%s/sample/filenames.txt' % data_dir
    filenames, sentids = [], []
    if os.path.isfile(filepath):
        with open(filepath, 'r') as f:
            lines = [ln.strip() for ln in f.read().splitlines()]
        print('Load filenames from: %s (%d)' % (filepath, len(lines)))
        for pair in lines:
            if not pair:
                continue
            name, sentid = pair.split(',')
            filenames.append(name)
            sentids.append(int(sentid))
    return filenames, sentids


def install_torchtext_stub():
    """Make `torchtext.vocab.Vocab` resolvable for plain pickle.load callers (tools, tests)."""
    import sys
    if 'torchtext' not in sys.modules:
        tt = types.ModuleType('torchtext')
        ttv = types.ModuleType('torchtext.vocab')
        ttv.Vocab = Vocab
        ttv._default_unk_index = _default_unk_index
        tt.vocab = ttv
        sys.modules['torchtext'] = tt
        sys.modules['torchtext.vocab'] = ttv

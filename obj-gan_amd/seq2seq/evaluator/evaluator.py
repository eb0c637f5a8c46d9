from __future__ import print_function, division

import collections
import os

import numpy as np
import torch

from seq2seq.dataset.prepare_dataset import indexes_from_sentence
from seq2seq.models.DecoderRNN import draw_noise


class Evaluator(object):
    """Samples a layout per caption and writes it where the image generator's data path reads it (reference
    box_generation/seq2seq/evaluator/evaluator.py).  Same constructor arguments; `batch_size` is the number of captions
    per device batch (the reference decodes one caption at a time whatever it is given).

    The post-processing restates evaluator.py:74-139: de-normalise, h = w * ratio, keep boxes whose four values are
    positive, drop the last entry (<eos>), label index -> category id, cap the count per category by a threshold drawn
    with np.random.normal from `gaussian_dict` (same place, same order: a seeded run draws the same thresholds),
    centre -> corner, clip to the 256 canvas."""

    def __init__(self, batch_size, early_stop_len, expt_dir, dev_cap_lang, dev_label_lang, x_mean_std, y_mean_std,
                 w_mean_std, r_mean_std, gaussian_dict, box_saving_folder, output_opt):
        self.batch_size = max(1, int(batch_size))
        self.early_stop_len = early_stop_len
        self.expt_dir = expt_dir
        self.dev_cap_lang = dev_cap_lang
        self.dev_label_lang = dev_label_lang
        self.x_mean_std = x_mean_std
        self.y_mean_std = y_mean_std
        self.w_mean_std = w_mean_std
        self.r_mean_std = r_mean_std
        self.gaussian_dict = gaussian_dict
        self.display_step = 200
        self.box_saving_folder = box_saving_folder
        self.std_img_size = 256.0
        self.output_opt = output_opt

    # ---- one caption: raw samples -> boxes ----------------------------------------------------------------------
    def postprocess(self, sequence, xy, wh):
        """sequence: label indices of one caption (the <eos> step included); xy, wh: its drawn pairs.
        -> (xs, ys, ws, hs, category ids as strings): corner boxes on the 256 canvas; five empty lists when at most
        one entry survives the positivity filter."""
        xs, ys = self.coord_converter(xy, self.x_mean_std[0], self.x_mean_std[1], self.y_mean_std[0], self.y_mean_std[1])
        ws, hs = self.coord_converter(wh, self.w_mean_std[0], self.w_mean_std[1], self.r_mean_std[0], self.r_mean_std[1])
        hs = np.multiply(ws, hs)
        ls = np.array([int(l) for l in sequence])
        xs, ys, ws, hs, ls = self.validity_indices(xs, ys, ws, hs, ls)
        if len(ls) <= 1:
            return [], [], [], [], []
        xs, ys, ws, hs = xs[:-1], ys[:-1], ws[:-1], hs[:-1]
        ls = np.array([int(self.dev_label_lang.index2word[int(l)]) for l in ls[:-1]])
        kept = []
        for label in collections.Counter(ls.tolist()):           # categories in order of first appearance
            mu, sigma = self.gaussian_dict[label]
            threshold = max(int(np.random.normal(mu, sigma, 1)[0]), 2)
            kept += np.where(ls == label)[0].tolist()[:threshold]
        kept.sort()
        xs, ys, ws, hs, ls = xs[kept], ys[kept], ws[kept], hs[kept], ls[kept]
        xs = np.clip(xs - ws / 2.0, 1, self.std_img_size - 1)
        ys = np.clip(ys - hs / 2.0, 1, self.std_img_size - 1)
        ws = np.minimum(ws, self.std_img_size - xs)
        hs = np.minimum(hs, self.std_img_size - ys)
        return xs, ys, ws, hs, [str(l) for l in ls]

    def coord_converter(self, coord_seq, mean_x, std_x, mean_y, std_y):
        xs = [x * std_x + mean_x for x, _ in coord_seq]
        ys = [y * std_y + mean_y for _, y in coord_seq]
        return np.array(xs, dtype=np.float64), np.array(ys, dtype=np.float64)

    def validity_indices(self, x_seq, y_seq, w_seq, h_seq, l_seq):
        valid = (x_seq > 0) & (y_seq > 0) & (w_seq > 0) & (h_seq > 0)
        return x_seq[valid], y_seq[valid], w_seq[valid], h_seq[valid], l_seq[valid]

    # ---- writing ------------------------------------------------------------------------------------------------
    def write_layouts(self, decoded, keys, captions=None):
        """decoded: per caption (sequence, xy, wh), in the order of `keys`.  Writes `<box_saving_folder><key>/<i>/
        boxes.txt` (i counts the captions of a key; the file is empty when no box is left) for output_opt 0, or
        one line per caption into `<expt_dir>/dev_bbox_test.txt` for output_opt 1.  Returns the layouts: per caption
        a list of (x, y, w, h, category id)."""
        seen = {}
        layouts = []
        fout_all = open('%s/dev_bbox_test.txt' % self.expt_dir, 'w') if self.output_opt == 1 else None
        for index, (sequence, xy, wh) in enumerate(decoded):
            xs, ys, ws, hs, ls = self.postprocess(sequence, xy, wh)
            layouts.append([(xs[i], ys[i], ws[i], hs[i], ls[i]) for i in range(len(ls))])
            if self.output_opt == 0:
                key = keys[index]
                sub_dir = '%s%s/%d/' % (self.box_saving_folder, key, seen.get(key, 0))
                seen[key] = seen.get(key, 0) + 1
                os.makedirs(sub_dir, exist_ok=True)
                with open('%s/boxes.txt' % sub_dir, 'w') as f:
                    for i in range(len(ls)):
                        f.write('%.2f,%.2f,%.2f,%.2f,%s,0\n' % (xs[i], ys[i], ws[i], hs[i], ls[i]))
            elif fout_all is not None and len(ls) > 0:
                words = [self.dev_cap_lang.index2word[w] for w in captions[index]] if captions is not None else []
                fout_all.write('%s - %s - ' % (keys[index], words))
                for i in range(len(ls)):
                    fout_all.write('%.2f,%.2f,%.2f,%.2f,%s - ' % (xs[i], ys[i], ws[i], hs[i], ls[i]))
                fout_all.write('\n')
        if fout_all is not None:
            fout_all.close()
        return layouts

    # ---- the tables of the device layout stage (objgan_hip.ops.layout_from_decode) ---------------------------------
    UNCAPPED = 1 << 30          # count cap of a label that names no category (<pad>, <sos>, <eos>, <unk>): never reached

    def label_categories(self):
        """[L] int64: decoder label index -> category id, int(index2word[l]); -1 where the word is not a number"""
        L = len(self.dev_label_lang.index2word)
        out = np.full((L,), -1, np.int64)
        for l in range(L):
            word = str(self.dev_label_lang.index2word[l])
            if word.isdigit():
                out[l] = int(word)
        return out

    def layout_tables(self, cats_index_dict, device=None):
        """-> (mean_std [8] float64: mean and std of x, y, w, r; label_to_cat [L] int32; cat_to_rel [maxcat + 1] int32:
        `cats_index_dict` as a table, -1 for an id it does not hold), on `device`: the constant inputs of
        ops.layout_from_decode, which restates `postprocess` and the readers of the files `write_layouts` writes."""
        mean_std = torch.tensor([float(v) for pair in (self.x_mean_std, self.y_mean_std, self.w_mean_std,
                                                       self.r_mean_std) for v in pair[:2]], dtype=torch.float64)
        label_to_cat = torch.from_numpy(self.label_categories().astype(np.int32))
        cat_to_rel = np.full((max(int(c) for c in cats_index_dict) + 1,), -1, np.int32)
        for cat, rel in cats_index_dict.items():
            cat_to_rel[int(cat)] = int(rel)
        tables = (mean_std, label_to_cat, torch.from_numpy(cat_to_rel))
        return tables if device is None else tuple(t.to(device) for t in tables)

    def draw_thresholds(self, rng, B):
        """[B, L] int32 count caps, max(int(normal(mu_l, sigma_l)), 2) for every (caption, label) in ONE draw; labels
        that name no category (or one `gaussian_dict` does not hold) get UNCAPPED.  The law of `postprocess`'s
        per-category draws, from another stream: `postprocess` draws only for the categories a caption shows, in order
        of appearance, so a seeded run reproduces the distribution of the file route's layouts, not its samples."""
        rng = np.random if rng is None else rng
        cats = self.label_categories()
        known = np.array([c >= 0 and int(c) in self.gaussian_dict for c in cats], bool)
        mu = np.array([self.gaussian_dict[int(c)][0] if k else 0.0 for c, k in zip(cats, known)], np.float64)
        sigma = np.array([self.gaussian_dict[int(c)][1] if k else 0.0 for c, k in zip(cats, known)], np.float64)
        draw = np.trunc(rng.normal(mu, sigma, size=(int(B), len(cats))))           # int(): toward zero
        caps = np.maximum(np.clip(draw, -self.UNCAPPED, self.UNCAPPED).astype(np.int64), 2)
        caps[:, ~known] = self.UNCAPPED
        return caps.astype(np.int32)

    # ---- the device part ----------------------------------------------------------------------------------------
    def decode(self, encoder, decoder, data, rng=None, noise=None):
        """-> per caption (sequence, xy, wh) and the caption ids; `batch_size` captions per launch.  noise: [N, T, 6]
        for all captions, or drawn caption by caption from `rng` (a numpy RandomState; default: np.random)."""
        device = next(decoder.parameters()).device
        seqs = [indexes_from_sentence(self.dev_cap_lang, item[0]) for item in data]
        decoded = []
        for start in range(0, len(seqs), self.batch_size):
            if (start // self.batch_size + 1) % self.display_step == 0:
                print('%07d / %07d' % (start, len(seqs)))
            batch = seqs[start:start + self.batch_size]
            lens = [len(s) for s in batch]
            caps = torch.zeros((len(batch), max(1, max(lens))), dtype=torch.int64)
            for b, s in enumerate(batch):
                caps[b, :len(s)] = torch.tensor(s, dtype=torch.int64)
            nz = noise[start:start + len(batch)] if noise is not None else \
                draw_noise(rng, len(batch), self.early_stop_len)
            _, hidden = encoder(caps.to(device), lens)
            other = decoder(hidden, None, is_training=0, early_stop_len=self.early_stop_len, noise=nz)[4]
            for b in range(len(batch)):
                decoded.append((other['sequence'][b], other['xy'][b], other['wh'][b]))
        return decoded, seqs

    def evaluate(self, encoder, decoder, data, keys, rng=None, noise=None):
        """Sample a layout for every caption of `data` and write it; returns the layouts (see write_layouts)."""
        decoded, seqs = self.decode(encoder, decoder, data, rng=rng, noise=noise)
        return self.write_layouts(decoded, keys, captions=seqs)

"""Caption text -> layout -> instance masks -> images in one process, with nothing written between the stages.

    box generator   PreEncoderRNN -> ops.box_decode                 labels, lengths, samples        (device)
    layout stage    ops.layout_from_decode -> ops.boxmaps_onehot    boxes, box tables, box maps     (device)
    shape + image   condGANEvaluator.sampling                       SHP_G_NET -> form_hmaps -> G_NET

The layout stage restates the file route between `sample.py --is_training 0` and `main.py --USE_GT_BOX_SEG 2`
(Evaluator.postprocess, write_layouts, load_gen_insanns, get_gen_rois, the collate of prepare_gen_data) and is pinned
to it bit for bit (tests/test_layout_gpu.py).  `TextToImage` needs no test split, no image bigfile, no activation file
and no Inception network.  Per batch ONE device-to-host copy precedes the image generator: the box counts and the
64-pixel box table, which `form_hmaps` and `form_clabels_feat` index on the host (miscc.utils.attach_host);
`sampling` itself reads the batch's largest count once more, as it does in evaluation mode."""
import os
import re
import sys
import types

import numpy as np
import torch

from miscc.config import cfg
from miscc.utils import attach_host, h2d

_WORD = re.compile(r'\w+')


def tokenize(text):
    """the words of a caption: re.findall(r'\\w+', text.lower())"""
    return _WORD.findall(text.lower())


def encode_caption(text, line, vocabularies, words_num, notices=None):
    """One caption against several vocabularies (dicts word -> id).  -> one id list per vocabulary, words outside a
    vocabulary dropped, the first `words_num` kept (None: all).  `notices` (a set) collects the dropped words.  A caption
    none of whose words is known to some vocabulary is refused with a ValueError naming `line`."""
    tokens = tokenize(text)
    out = []
    for vocab in vocabularies:
        ids = [vocab[w] for w in tokens if w in vocab]
        if notices is not None:
            notices.update(w for w in tokens if w not in vocab)
        if not ids:
            raise ValueError("caption %d (%r): no word of it is in the vocabulary" % (line, text.strip()))
        out.append(ids if words_num is None else ids[:words_num])
    return out


def boxes_txt(rows):
    """the text of a `boxes.txt` for (x, y, w, h, category id) rows, as Evaluator.write_layouts prints it"""
    return ''.join('%.2f,%.2f,%.2f,%.2f,%s,0\n' % (r[0], r[1], r[2], r[3], str(int(r[4]))) for r in rows)


def required_files(data_dir, net_g, box_ckpt, net_e=None, net_shp_g=None, box_encoder=None, mean_std=None,
                   gaussian_dict=None):
    """-> {role: path} of every file `TextToImage.from_files` reads (defaults: the reference's places under data_dir)"""
    from seq2seq.util.checkpoint import Checkpoint
    under = lambda p: p if p.startswith(data_dir) else data_dir + p          # (from_files leaves the full paths in cfg)
    net_e = net_e or under(cfg.TRAIN.NET_E)
    files = {"NET_G": net_g, "text encoder": net_e, "box generator's text encoder": box_encoder or net_e,
             "NET_SHP_G": net_shp_g or under(cfg.TEST.NET_SHP_G),
             "captions.pickle": os.path.join(data_dir, "captions.pickle"),
             "captions_glove.pickle": os.path.join(data_dir, "captions_glove.pickle"),
             "categories.txt": os.path.join(data_dir, "categories.txt"),
             "mean/std file": mean_std or os.path.join(data_dir, "box_label", "mean_std_train2014.txt"),
             "gaussian_dict.npy": gaussian_dict or os.path.join(data_dir, "box_label", "gaussian_dict.npy")}
    for name in (Checkpoint.MODEL_NAME, Checkpoint.CAP_WORD2INDEX, Checkpoint.CAP_INDEX2WORD,
                 Checkpoint.LABEL_WORD2INDEX, Checkpoint.LABEL_INDEX2WORD):
        files["box checkpoint %s" % name] = os.path.join(box_ckpt, name)
    return files


class TextToImage(object):
    """box_encoder / decoder: the box generator (seq2seq.models); layout: a seq2seq.evaluator.Evaluator holding the
    label vocabulary, the means and stds, `gaussian_dict` and early_stop_len; box_vocab: its caption vocabulary
    (word -> id); imager: a condGANEvaluator whose netG, netShpG, text_encoder and glove_emb are on `device`;
    wordtoix / glove_wordtoix: the image generator's two caption vocabularies."""

    def __init__(self, box_encoder, decoder, layout, box_vocab, imager, wordtoix, glove_wordtoix, device,
                 batch_size=16):
        self.box_encoder, self.decoder, self.layout, self.box_vocab = box_encoder, decoder, layout, box_vocab
        self.imager, self.wordtoix, self.glove_wordtoix = imager, wordtoix, glove_wordtoix
        self.device = device
        self.batch_size = max(1, int(batch_size))
        self.imsize = [cfg.TREE.BASE_SIZE * (2 ** b) for b in range(cfg.TREE.BRANCH_NUM)]
        self.mean_std, self.label_to_cat, self.cat_to_rel = layout.layout_tables(imager.cats_index_dict, device)
        self.clabels_emb = imager.prepare_cat_emb()
        self.last_decode = self.last_layout = None          # the device tensors of the last batch's first two stages
        self.events = None               # a list: receives (stage name, device event) marks (tools/generate_time.py)

    def _mark(self, name):
        if self.events is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.events.append((name, e))

    @classmethod
    def from_files(cls, data_dir, net_g, box_ckpt, device, net_e=None, net_shp_g=None, box_encoder=None, mean_std=None,
                   gaussian_dict=None, early_stop_len=10, batch_size=16, output_dir=''):
        """Loads with the loaders the two command lines use: Checkpoint.load and PreEncoderRNN (sample.py),
        load_text_data / load_glove_emb / load_cat_label / load_cats and condGANEvaluator.build_models (main.py)."""
        from evaluator import condGANEvaluator
        from miscc import load
        from seq2seq.dataset.prepare_dataset import Lang, read_mean_std
        from seq2seq.evaluator import Evaluator
        from seq2seq.models import PreEncoderRNN
        from seq2seq.util.checkpoint import Checkpoint
        files = required_files(data_dir, net_g, box_ckpt, net_e, net_shp_g, box_encoder, mean_std, gaussian_dict)
        checkpoint = Checkpoint.load(box_ckpt)
        decoder = checkpoint.model.eval().to(device)
        encoder = PreEncoderRNN(len(checkpoint.cap_word2index), nhidden=decoder.hidden_size)
        encoder.load_state_dict(torch.load(files["box generator's text encoder"], map_location='cpu'))
        encoder.eval().to(device)
        label_lang = Lang('label')
        label_lang.set_word2index(checkpoint.label_word2index)
        label_lang.set_index2word(checkpoint.label_index2word)
        stats = read_mean_std(files["mean/std file"])
        gauss = np.load(files["gaussian_dict.npy"], allow_pickle=True).item()
        layout = Evaluator(batch_size, early_stop_len, '', None, label_lang, stats[0], stats[1], stats[2], stats[3],
                           gauss, '', 0)
        ds = types.SimpleNamespace()
        _, _, ds.ixtoword, ds.wordtoix, ds.n_words = load.load_text_data(data_dir, 'test', [], [])
        _, _, ds.glove_wordtoix, ds.glove_embed = load.load_glove_emb(data_dir, 'test', [], [])
        ds.cat_labels, ds.cat_label_lens, ds.sorted_cat_label_indices = load.load_cat_label(data_dir, ds.glove_wordtoix)
        ds.cats_dict, ds.cats_index_dict = load.load_cats(data_dir, ds.wordtoix)
        cfg.TRAIN.NET_G, cfg.TRAIN.NET_E, cfg.TEST.NET_SHP_G = files["NET_G"], files["text encoder"], files["NET_SHP_G"]
        cfg.TEST.USE_GT_BOX_SEG = 2
        imager = condGANEvaluator(output_dir, None, ds, device=device)
        imager.build_models()
        return cls(encoder, decoder, layout, checkpoint.cap_word2index, imager, ds.wordtoix, ds.glove_wordtoix, device,
                   batch_size)

    # ---- text -------------------------------------------------------------------------------------------------
    def encode(self, captions, lines=None, notice=True):
        """-> per caption (box-generator ids, caption ids, GloVe ids); one notice on stderr names the dropped words.
        lines: the captions' line numbers for the refusal message (default: 1, 2, ...)"""
        from seq2seq.dataset.prepare_dataset import indexes_from_sentence
        dropped, out = set(), []
        box_lang = types.SimpleNamespace(word2index=self.box_vocab)
        for line, text in zip(lines if lines is not None else range(1, len(captions) + 1), captions):
            _, cap, glove = encode_caption(text, line, (self.box_vocab, self.wordtoix, self.glove_wordtoix), None,
                                           dropped)
            n = min(len(cap), len(glove), cfg.TEXT.WORDS_NUM)        # get_caption: the shorter of the two, the first words
            # the box generator reads the whole caption, framed by <sos> / <eos> where its vocabulary has them
            out.append((indexes_from_sentence(box_lang, tokenize(text)), cap[:n], glove[:n]))
        if dropped and notice:
            print("generate: words outside a vocabulary were dropped: %s" % ", ".join(sorted(dropped)), file=sys.stderr)
        return out

    # ---- one batch --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _batch(self, encoded, rng, noise):
        """encoded: the batch in INPUT order; noise: dict of per-caption rows in input order (box [B, T, 6], thresholds
        [B, L], img [B, Z_DIM], shp [B, BOXES_NUM, 4 classes]; each optional).  -> (images, boxes, nbox, raw masks,
        num_rois), all in input order."""
        from objgan_hip import ops
        from seq2seq.models.DecoderRNN import draw_noise
        dev, B, W = self.device, len(encoded), cfg.TEXT.WORDS_NUM
        T, R, C = int(self.layout.early_stop_len), cfg.ROI.BOXES_NUM, self.imager.num_classes
        lens = torch.tensor([len(e[1]) for e in encoded], dtype=torch.int64)
        lens_sorted, order = torch.sort(lens, 0, True)                  # as prepare_gen_data orders a batch
        order_list = order.tolist()
        rows = [encoded[i] for i in order_list]

        def take(key, draw):
            t = noise.get(key) if noise else None
            t = draw() if t is None else torch.as_tensor(t)[order]
            return t

        # box generator
        self._mark("start")
        box_lens = [len(r[0]) for r in rows]
        caps = torch.zeros((B, max(box_lens)), dtype=torch.int64)
        for b, r in enumerate(rows):
            caps[b, :box_lens[b]] = torch.tensor(r[0], dtype=torch.int64)
        nz = take("box", lambda: torch.from_numpy(draw_noise(rng, B, T)))
        th = take("thresholds", lambda: torch.from_numpy(self.layout.draw_thresholds(rng, B)))
        _, hidden = self.box_encoder(h2d(caps, dev), box_lens)
        h0, c0 = (s[0].contiguous() for s in self.decoder._init_state(hidden))
        d = self.decoder
        labels, lengths, samples = ops.box_decode(h0, c0, h2d(nz.to(torch.float64), dev), d._weights(),
                                                  (d.x_mean, d.y_mean, d.w_mean, d.r_mean), d.l_sos_id, d.l_eos_id)
        self.last_decode = (labels, lengths, samples)
        self._mark("encoder + decode")
        # layout stage
        lay = ops.layout_from_decode(labels, lengths, samples, self.mean_std, self.label_to_cat, self.cat_to_rel,
                                     h2d(th.to(torch.int32), dev), self.imsize, cfg.ROI.FM_SIZE, R,
                                     min_size=cfg.ROI.ROI_MIN_SIZE)
        self.last_layout = lay
        # the one read: box counts and the 64-pixel box table
        host = torch.cat((lay["rois"][0].reshape(B, -1), lay["num_rois"].to(torch.float64).unsqueeze(1)), 1).cpu()
        num_host = host[:, -1].to(torch.int64)
        rois0_host = host[:, :-1].reshape(B, R, 6).contiguous()
        n = max(int(num_host.max()), 1)
        fwd, bwd = ops.boxmaps_onehot(lay["raw_maps"], lay["cats"], lay["num_rois"], n, C)
        rois = [attach_host(lay["rois"][0], rois0_host)] + list(lay["rois"][1:])
        num_rois = attach_host(lay["num_rois"].to(torch.int64), num_host)
        self._mark("layout stage")
        # text embeddings of the image generator
        captions = torch.zeros((B, W), dtype=torch.int64)
        glove = torch.zeros((B, W), dtype=torch.int64)
        for b, r in enumerate(rows):
            captions[b, :len(r[1])] = torch.tensor(r[1], dtype=torch.int64)
            glove[b, :len(r[2])] = torch.tensor(r[2], dtype=torch.int64)
        captions, glove = h2d(captions, dev), h2d(glove, dev)
        cap_lens = attach_host(h2d(lens_sorted, dev), lens_sorted)
        im = self.imager
        words_embs, sent_emb = im.text_encoder(captions, cap_lens, int(lens_sorted.max()))
        num_words = words_embs.size(2)
        gw = torch.nn.functional.embedding(glove.reshape(-1), im.glove_emb.weight)
        data = {"rois": rois, "fm_rois": lay["fm_rois"], "num_rois": num_rois, "bbox_maps_fwd": fwd, "bbox_maps_bwd": bwd,
                "bbox_fmaps": lay["raw_fmaps"][:, :n].contiguous(), "words_embs": words_embs, "sent_emb": sent_emb,
                "glove_words_embs": gw.view(B, W, -1)[:, :num_words].transpose(1, 2),
                "mask": (captions == 0)[:, :num_words]}
        noise_img = take("img", lambda: None)
        noise_shp = take("shp", lambda: None)
        saved = cfg.TEST.USE_GT_BOX_SEG
        cfg.TEST.USE_GT_BOX_SEG = 2
        try:
            out = im.sampling(data, self.clabels_emb, self.imsize,
                              noise_img=None if noise_img is None else h2d(noise_img.float(), dev),
                              noise_shp=None if noise_shp is None else h2d(noise_shp.float(), dev))
        finally:
            cfg.TEST.USE_GT_BOX_SEG = saved
        self._mark("shape + image generator")
        back = torch.empty_like(order)
        back[order] = torch.arange(B)
        back_dev = h2d(back, dev)
        images = out["fake_imgs"][-1].index_select(0, back_dev)
        masks = out["raw_masks"].index_select(0, back_dev)
        boxes, nbox = lay["boxes"].index_select(0, back_dev), lay["nbox"].index_select(0, back_dev)
        return images, boxes, nbox, masks, num_host[back]

    def generate(self, captions, seed=None, noise=None, lines=None, notice=True):
        """captions: list of strings.  seed: fixes the three random streams (decoder noise and count caps: numpy; image
        and shape noise: torch on the device).  noise: recorded noise instead, see `_batch`.
        -> (images [N, 3, S, S] in [-1, 1]: fake_imgs[-1]; layouts: per caption an [n, 5] float64 array of
        (x, y, w, h, category id) on the 256 canvas; masks: per caption the [num_rois, 64, 64] instance masks)."""
        encoded = self.encode(captions, lines, notice)
        rng = None
        if seed is not None:
            rng = np.random.RandomState(seed)
            torch.manual_seed(seed)
            torch.cuda.manual_seed_all(seed)
        images, layouts, masks = [], [], []
        for start in range(0, len(encoded), self.batch_size):
            part = slice(start, start + self.batch_size)
            sub = None if noise is None else {k: torch.as_tensor(v)[part] for k, v in noise.items() if v is not None}
            img, boxes, nbox, msk, num = self._batch(encoded[part], rng, sub)
            images.append(img)
            boxes, nbox = boxes.cpu().numpy(), nbox.cpu().numpy()
            for b in range(len(nbox)):
                layouts.append(boxes[b, :int(nbox[b])].copy())
                masks.append(msk[b, :int(num[b])])
        return torch.cat(images, 0), layouts, masks

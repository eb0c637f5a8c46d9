"""Evaluation of the image generator (reference image_generation/evaluator.py): `evaluate` runs the test split through
generated boxes -> SHP_G_NET instance masks -> form_hmaps layout maps -> caption / GloVe embeddings -> G_NET
inference, and reports the three numbers of the Obj-GAN paper -- Inception score (with the negative log posterior),
R-precision of the DAMSM encoders over pools of cfg.TEST.RP_POOL_SIZE images, and FID -- in `<output>/Score/scores.txt`.

`sampling(...)` is one batch of steps (2)-(4); `dump_fid_acts` writes the FID activations of the real images once, in
the reference's file format.  What a batch computes stays on the device: the R-precision pool (region features, codes,
embeddings) is kept there and scored by the DAMSM losses on the kernels, and the 2048-d activations of fake and real
images go into two fp64 moment accumulators (objgan_hip.ops.MomentAccumulator) instead of a host array and np.cov.
Per batch the only device-to-host copy is the [B, 1000] Inception prediction; `sampling` also reads the batch's
largest box count (one scalar, one sync), and the real images' activations arrive from the loader on the host and are
uploaded ([B, 2048] fp64).  The Frechet distance itself (one 2048 x 2048 matrix square root per evaluation) is scipy's,
on the host.

cfg.TEST.SAVE_OPTIONS == 'SNAPSHOT' also writes the caption / attention grids of every displayed batch into
`<output>/Snapshot/` (composed on the device, miscc.utils.build_super_images; one uint8 array per grid comes back).

Not here: TensorFlow Inception (cfg.TEST.USE_TF is answered with a notice and the PyTorch route), building the
`*_insanns.pickle` files from COCO JSON, more than one GPU.
"""
import os
import pickle

import numpy as np
import torch

from miscc.config import cfg
from miscc.utils import mkdir_p, weights_init, form_clabels_feat, form_hmaps, _host
from miscc.utils import compute_inception_score, negative_log_posterior_probability
from miscc.utils import get_activations, calculate_frechet_distance
from miscc.losses import words_loss, sent_loss
from miscc.load import acts_filename
from model import G_NET, SHP_G_NET, RNN_ENCODER
from trainer import category_embeddings
from testDataset import prepare_data, prepare_gen_data, prepare_acts_data

SCORES_HEADER = 'mean, std, mean_conf, std_conf, accu_w, std_w, accu_s, std_s, fid_score \n'


class RPrecisionPool(object):
    """The R-precision bookkeeping of reference evaluator.py:376-419, quirks included: batches are collected until
    `rp_count >= pool_size`; the NEXT batch triggers the evaluation and is itself added to no pool; the collected
    rows are truncated to `pool_size`; word embeddings are zero-padded to the longest caption of the pool.  Tensors
    stay on the device they arrive on, and are cloned on arrival: an encoder replayed from a captured graph
    (objgan_hip.graphs.GraphedCallable) hands out storage that its next replay overwrites."""

    def __init__(self, pool_size, labels=None):
        self.pool_size = int(pool_size)
        self.labels = labels        # [pool_size] match labels (condGANEvaluator.prepare_labels); built on demand
        self.w_accuracy, self.s_accuracy = [], []
        self.last_inputs = None
        self._reset()

    def _reset(self):
        self.rp_count = 0
        self.regions, self.codes, self.words, self.sents, self.class_ids, self.cap_lens = [], [], [], [], [], []

    def step(self, region_features, cnn_code, words_embs, sent_emb, class_ids, cap_lens):
        """One batch.  -> (w_accu, s_accu) when this batch triggered an evaluation (and was discarded), else None."""
        if self.rp_count < self.pool_size:
            self.regions.append(region_features.detach().clone())
            self.codes.append(cnn_code.detach().clone())
            self.words.append(words_embs.detach().clone())
            self.sents.append(sent_emb.detach().clone())
            self.class_ids.append(np.asarray(class_ids))
            self.cap_lens.append(cap_lens.detach().clone())
            self.rp_count += int(sent_emb.size(0))
            return None
        P = self.pool_size
        regions = torch.cat(self.regions, 0)[:P]
        codes = torch.cat(self.codes, 0)[:P]
        sents = torch.cat(self.sents, 0)[:P]
        class_ids = np.concatenate(self.class_ids, 0)[:P]
        cap_lens = torch.cat(self.cap_lens, 0)[:P]
        max_len = int(torch.max(cap_lens))
        words = torch.zeros(self.rp_count, sents.size(1), max_len, dtype=sents.dtype, device=sents.device)
        accum = 0
        for w in self.words:
            words[accum:accum + w.size(0), :, :w.size(2)] = w
            accum += w.size(0)
        words = words[:P]
        labels = self.labels if self.labels is not None else torch.arange(P, device=sents.device)
        self.last_inputs = (regions, codes, words, sents, class_ids, cap_lens)
        with torch.no_grad():
            _, _, _, w_accu = words_loss(regions, words, labels, cap_lens, class_ids, P, is_training=False,
                                         need_att_maps=False)
            _, _, s_accu = sent_loss(codes, sents, labels, class_ids, P, is_training=False)
        self.w_accuracy.append(w_accu)
        self.s_accuracy.append(s_accu)
        self._reset()
        return w_accu, s_accu


class StagedMoments(object):
    """A MomentAccumulator behind a `rows`-row staging buffer: every accumulate call streams the 32 MB accumulator
    once, so batches of 16 are handed over eight at a time.  The statistics do not depend on where the calls are cut."""

    def __init__(self, D, device, rows=128):
        from objgan_hip import ops
        self.acc = ops.MomentAccumulator(D, device)
        self.stage = torch.empty(rows, D, dtype=torch.float32, device=device)
        self.fill = 0

    def add(self, x):
        x = x.detach().to(self.stage.device, torch.float32)
        while x.size(0):
            n = min(x.size(0), self.stage.size(0) - self.fill)
            self.stage[self.fill:self.fill + n].copy_(x[:n])
            self.fill += n
            x = x[n:]
            if self.fill == self.stage.size(0):
                self.flush()

    def flush(self):
        if self.fill:
            self.acc.add(self.stage[:self.fill])
            self.fill = 0

    def finalize(self):
        self.flush()
        mu, sigma = self.acc.finalize()
        return mu.cpu().numpy(), sigma.cpu().numpy()


class condGANEvaluator(object):
    def __init__(self, output_dir, data_loader, dataset, device=None):
        self.image_dir = os.path.join(output_dir, 'Image') if output_dir else ''
        self.score_dir = os.path.join(output_dir, 'Score') if output_dir else ''
        self.snapshot_dir = os.path.join(output_dir, 'Snapshot') if output_dir else ''      # made when first written to
        for d in (self.image_dir, self.score_dir):
            if d:
                mkdir_p(d)
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.batch_size = cfg.TRAIN.BATCH_SIZE
        self.data_loader = data_loader
        for name in ("n_words", "ixtoword", "cats_dict", "cats_index_dict", "cat_labels", "cat_label_lens",
                     "sorted_cat_label_indices"):
            setattr(self, name, getattr(dataset, name, None))
        self.num_classes = len(self.cats_index_dict) if self.cats_index_dict is not None else \
            getattr(dataset, "num_classes", 80)
        self.glove_emb = getattr(dataset, "glove_embed", None)
        self.text_encoder = getattr(dataset, "text_encoder", None)
        self.image_encoder = getattr(dataset, "image_encoder", None)
        self.inception_model = getattr(dataset, "inception_model", None)
        self.inception_model_fid = getattr(dataset, "inception_model_fid", None)
        self.display_interval = cfg.TRAIN.DISPLAY_INTERVAL
        self.num_batches = len(data_loader) if data_loader is not None else 0
        self.netG = self.netShpG = None

    def build_models(self):
        """-> [text_encoder, image_encoder, netG, netShpG] (reference evaluator.py:88-146).  Encoders the dataset handed
        over are used as they are; the others are read from the reference's files: the DAMSM pair from cfg.TRAIN.NET_E
        (`text_encoder` -> `image_encoder`), the two Inception monitors from the torchvision state dict next to them."""
        if self.text_encoder is None:
            enc = RNN_ENCODER(self.n_words, nhidden=cfg.TEXT.EMBEDDING_DIM)
            enc.load_state_dict(torch.load(cfg.TRAIN.NET_E, map_location="cpu"))
            print('Load text encoder from:', cfg.TRAIN.NET_E)
            self.text_encoder = enc
        for p in self.text_encoder.parameters():
            p.requires_grad_(False)
        self.text_encoder.to(self.device).eval()
        if self.image_encoder is None and cfg.TRAIN.NET_E:
            path = cfg.TRAIN.NET_E.replace('text_encoder', 'image_encoder')
            if os.path.isfile(path):
                from encoders import CNN_ENCODER
                enc = CNN_ENCODER(cfg.TEXT.EMBEDDING_DIM)
                enc.load_state_dict(torch.load(path, map_location="cpu"))
                print('Load image encoder from:', path)
                self.image_encoder = enc
        if self.image_encoder is not None:
            for p in self.image_encoder.parameters():
                p.requires_grad_(False)
            self.image_encoder.to(self.device).eval()
        netG = G_NET(self.num_classes)
        netG.apply(weights_init)
        netShpG = None
        if cfg.TEST.USE_GT_BOX_SEG > 0:
            netShpG = SHP_G_NET(self.num_classes)
            netShpG.apply(weights_init)
        if cfg.TRAIN.NET_G:
            netG.load_state_dict(torch.load(cfg.TRAIN.NET_G, map_location="cpu"))
            print('Load G from: ', cfg.TRAIN.NET_G)
        if netShpG is not None and cfg.TEST.NET_SHP_G and os.path.exists(cfg.TEST.NET_SHP_G):
            netShpG.load_state_dict(torch.load(cfg.TEST.NET_SHP_G, map_location="cpu"))
            print('Load Shape G from: ', cfg.TEST.NET_SHP_G)
        self.netG = netG.to(self.device).eval()
        self.netShpG = netShpG.to(self.device).eval() if netShpG is not None else None
        if self.glove_emb is not None:
            self.glove_emb.to(self.device).eval()
        if self.inception_model is not None:
            self.inception_model.to(self.device).eval()
        if self.inception_model_fid is not None:
            self.inception_model_fid.to(self.device).eval()
        return [self.text_encoder, self.image_encoder, self.netG, self.netShpG]

    def build_inception_monitors(self):
        """INCEPTION_V3 (Inception score) and INCEPTION_V3_FID on ONE trunk, from the torchvision ImageNet state dict
        the reference reads (model.py:294, 367); whichever the dataset handed over is kept."""
        import encoders
        if cfg.TEST.USE_TF:
            print('=' * 100 + '\ncfg.TEST.USE_TF is set but there is no TensorFlow Inception here: Inception score and FID come '
                  'from the PyTorch Inception-v3 (the `_tf0` activation file); they are not comparable with TF numbers\n'
                  + '=' * 100)
        if self.inception_model is None or self.inception_model_fid is None:
            if self.inception_model is not None:
                net = self.inception_model.model
            elif self.inception_model_fid is not None:
                net = self.inception_model_fid.trunk
            else:
                net = encoders.INCEPTION_V3_FID._load_pretrained()
            if self.inception_model is None:
                if not isinstance(net, encoders.Inception3):
                    raise RuntimeError("the Inception-score monitor needs a whole Inception3 (trunk + fc)")
                self.inception_model = encoders.INCEPTION_V3(net)
            if self.inception_model_fid is None:
                block_idx = encoders.INCEPTION_V3_FID.BLOCK_INDEX_BY_DIM[cfg.TEST.FID_DIMS]
                self.inception_model_fid = encoders.INCEPTION_V3_FID([block_idx], trunk=net)
        self.inception_model.to(self.device).eval()
        self.inception_model_fid.to(self.device).eval()

    def prepare_cat_emb(self):
        return category_embeddings(self.glove_emb.weight, self.cat_labels, self.cat_label_lens,
                                   self.sorted_cat_label_indices, len(self.cats_index_dict)).to(self.device)

    def prepare_labels(self):
        """match labels of one R-precision pool: image i belongs to caption i"""
        return torch.arange(cfg.TEST.RP_POOL_SIZE, device=self.device)

    @torch.no_grad()
    def sampling(self, data, clabels_emb, hmap_size, noise_img=None, noise_shp=None):
        """One batch of evaluator.py:290-340.  `data`: dict with rois[3] / fm_rois / num_rois, and either the
        ground-truth layout (hmaps, bt_masks, fm_bt_masks; cfg.TEST.USE_GT_BOX_SEG == 0) or the box maps of
        the shape generator (bbox_maps_fwd, bbox_maps_bwd, bbox_fmaps); captions / cap_lens /
        glove_captions, or precomputed words_embs / sent_emb / glove_words_embs / mask.
        -> dict(fake_imgs, attn_maps, bt_attn_maps, hmaps, raw_masks, is_pred)"""
        d = data
        rois, fm_rois, num_rois = d["rois"], d["fm_rois"], d["num_rois"]
        B = int(num_rois.shape[0])
        max_num_roi = int(torch.max(num_rois))
        if noise_img is None:
            noise_img = torch.randn(B, cfg.GAN.Z_DIM, device=self.device)
        raw_masks = None
        if cfg.TEST.USE_GT_BOX_SEG > 0:
            if noise_shp is None:
                noise_shp = torch.randn(B, cfg.ROI.BOXES_NUM, self.num_classes * 4, device=self.device)
            raw_masks = self.netShpG(noise_shp[:, :max_num_roi], d["bbox_maps_fwd"], d["bbox_maps_bwd"],
                                     d["bbox_fmaps"]).squeeze(2)
            hmaps, bt_masks, fm_bt_masks = form_hmaps(raw_masks, num_rois, rois[0], hmap_size, self.num_classes)
        else:
            hmaps, bt_masks, fm_bt_masks = d["hmaps"], d["bt_masks"], d["fm_bt_masks"]
        if "captions" in d and self.text_encoder is not None:
            captions, cap_lens = d["captions"], d["cap_lens"]
            max_len = int(torch.max(cap_lens))
            words_embs, sent_emb = self.text_encoder(captions, cap_lens, max_len)
            num_words = words_embs.size(2)
            mask = (captions == 0)[:, :num_words]
            gc = d["glove_captions"]
            gw = torch.nn.functional.embedding(gc.reshape(-1), self.glove_emb.weight)
            glove_words_embs = gw.view(gc.size(0), gc.size(1), -1)[:, :num_words].transpose(1, 2)
        else:
            words_embs, sent_emb = d["words_embs"], d["sent_emb"]
            glove_words_embs, mask = d["glove_words_embs"], d["mask"]
        clabels_feat = form_clabels_feat(clabels_emb, rois[0], num_rois)
        fake_imgs, _, attn_maps, bt_attn_maps, _, _ = self.netG(
            noise_img, sent_emb, words_embs, glove_words_embs, clabels_feat, mask, hmaps, rois, fm_rois,
            num_rois, bt_masks, fm_bt_masks, max_num_roi)
        out = {"fake_imgs": fake_imgs, "attn_maps": attn_maps, "bt_attn_maps": bt_attn_maps, "hmaps": hmaps,
               "raw_masks": raw_masks}
        if self.inception_model is not None:
            out["is_pred"] = self.inception_model(fake_imgs[-1])
        return out

    def save_img_results(self, fake_imgs, attn_maps, bt_attn_maps, captions, cap_lens, gen_iterations):
        """Snapshot/G_<n>_<i>.png and bt_G_<n>_<i>.png per attention stage (reference evaluator.py:170-205).  The
        reference's own call hands build_super_images keyword arguments it does not take (font_max, font_size) and
        raises; this is the trainer's form of the call (reference trainer.py:284-312).  -> the paths written."""
        from PIL import Image
        from miscc.utils import build_super_images
        mkdir_p(self.snapshot_dir)
        written = []
        for i in range(len(attn_maps)):
            img, lr_img = (fake_imgs[i + 1], fake_imgs[i]) if len(fake_imgs) > 1 else (fake_imgs[0], None)
            for prefix, maps in (("G", attn_maps[i]), ("bt_G", bt_attn_maps[i])):
                img_set, _ = build_super_images(img.detach(), captions, self.ixtoword, maps, int(maps.size(2)),
                                                lr_imgs=None if lr_img is None else lr_img.detach())
                path = '%s/%s_%d_%d.png' % (self.snapshot_dir, prefix, gen_iterations, i)
                Image.fromarray(img_set).save(path)
                written.append(path)
        return written

    def save_shape_results(self, imgs, hmaps, rois, num_rois, gen_iterations, model_type):
        """Snapshot/Shape<G|D>_<n>.png (reference evaluator.py:207-229): the real 64 x 64 images beside the per-box
        masks (G: generated) or the per-class layout maps (D: ground truth), every panel normalised on its own; the
        caption row of an image lists the first word of each box's category name."""
        from PIL import Image
        from miscc.utils import build_super_shape_images
        mkdir_p(self.snapshot_dir)
        B = int(hmaps.size(0))
        rois_np, nr = _host(rois), _host(num_rois).tolist()
        captions = torch.zeros(B, cfg.ROI.BOXES_NUM)
        for b in range(B):
            for r in range(int(nr[b])):
                captions[b, r] = self.cats_dict[int(rois_np[b, r, 4])][0]
        img_set, _ = build_super_shape_images(imgs.detach(), captions, self.ixtoword, hmaps.detach(), int(hmaps.size(2)),
                                              lr_imgs=None, font_max=20, font_size=12, max_word_num=cfg.ROI.BOXES_NUM,
                                              batch_size=B)
        path = '%s/Shape%s_%d.png' % (self.snapshot_dir, model_type, gen_iterations)
        Image.fromarray(img_set).save(path)
        return path

    def save_singleimages(self, images, keys, sent_ids, device_jpeg=True):
        """evaluator.py:225-233: [-1, 1] images -> <Image>/<key>_<sent id>.jpg.  A batch on the device whose sides are
        multiples of 16 is encoded there (ops.jpeg_encode: the same bytes Pillow writes, one launch pair and two copies per
        batch); everything else -- a CPU tensor, an odd size, device_jpeg=False -- takes the reference's host loop."""
        from PIL import Image
        images = images.detach()
        if device_jpeg and images.is_cuda:
            from objgan_hip import ops
            if ops.jpeg_encode_refusal(images) == 0:
                for i, data in enumerate(ops.jpeg_encode(images)):
                    with open('%s/%s_%d.jpg' % (self.image_dir, keys[i], sent_ids[i]), 'wb') as f:
                        f.write(data)
                return
        for i in range(images.size(0)):
            img = images[i].add(1).div(2).mul(255).clamp(0, 255).byte()
            ndarr = img.permute(1, 2, 0).cpu().numpy()
            Image.fromarray(ndarr).save('%s/%s_%d.jpg' % (self.image_dir, keys[i], sent_ids[i]))

    def write_scores(self, predictions):
        from miscc.utils import compute_inception_score, negative_log_posterior_probability
        preds = np.concatenate([p.detach().cpu().numpy() if torch.is_tensor(p) else np.asarray(p)
                                for p in predictions], 0)
        splits = min(10, self.batch_size)
        mean, std = compute_inception_score(preds, splits)
        mean_conf, std_conf = negative_log_posterior_probability(preds, splits)
        if self.score_dir:
            with open('%s/scores.txt' % self.score_dir, 'w') as fp:
                fp.write('mean, std, mean_conf, std_conf \n')
                fp.write('%f, %f, %f, %f' % (mean, std, mean_conf, std_conf))
        return mean, std, mean_conf, std_conf

    @torch.no_grad()
    def dump_fid_acts(self, data_dir, split):
        """FID activations of the REAL images of the loader -> <data_dir>/<split>_acts_tf0.pickle, the reference's format
        (evaluator.py:241-266): [ {key: float64 (2048,)} ], pickle protocol 2.  An existing file is left alone."""
        filepath = os.path.join(data_dir, acts_filename(split))
        if os.path.isfile(filepath):
            return
        self.build_inception_monitors()
        acts_dict = {}
        for count, data in enumerate(self.data_loader):
            if count % 10 == 0:
                print('%07d / %07d' % (count, self.num_batches))
            imgs, keys = prepare_acts_data(data, self.device)
            acts = get_activations(imgs[-1], self.inception_model_fid, len(keys)).double().cpu().numpy()
            for i, key in enumerate(keys):
                acts_dict[key] = np.array(acts[i], dtype=np.float64)
        with open(filepath, 'wb') as f:
            pickle.dump([acts_dict], f, protocol=2)
        print('Save to: ', filepath)

    def _default_noise(self, kind, shape):
        return torch.randn(*shape, device=self.device)

    @torch.no_grad()
    def evaluate(self, split_dir, hmap_size, noise_fn=None, trace=None):
        """The six steps of reference evaluator.py:268-466 over the loader -> the nine scores, also written to
        <Score>/scores.txt.  cfg.TEST.TEST_IMG_NUM counts BATCHES, like the reference.
        noise_fn(kind, shape) -> tensor on the device, kind 'img' ([B, Z_DIM]) or 'shp' ([B, BOXES_NUM, 4 classes]):
        lets a caller feed recorded noise; the default draws torch.randn there.
        trace: a list that receives one dict per batch (keys, fake images, FID activations, Inception predictions,
        on the host) -- for parity checks, not for full-size runs."""
        noise_fn = noise_fn if noise_fn is not None else self._default_noise
        self.build_inception_monitors()
        text_encoder, image_encoder, netG, netShpG = self.build_models()
        if image_encoder is None:
            raise RuntimeError("R-precision needs the DAMSM image encoder: %s is missing"
                               % cfg.TRAIN.NET_E.replace('text_encoder', 'image_encoder'))
        clabels_emb = self.prepare_cat_emb()
        snapshots = bool(self.snapshot_dir) and cfg.TEST.SAVE_OPTIONS == 'SNAPSHOT'
        save_images = bool(self.image_dir) and cfg.TEST.SAVE_OPTIONS in ('IMAGE', 'SNAPSHOT')
        pool = RPrecisionPool(cfg.TEST.RP_POOL_SIZE, self.prepare_labels())
        fake_stats = StagedMoments(cfg.TEST.FID_DIMS, self.device)
        real_stats = StagedMoments(cfg.TEST.FID_DIMS, self.device)
        predictions = []
        gen_iterations = 0
        for data in self.data_loader:
            # (1) general test data
            if cfg.TEST.USE_GT_BOX_SEG < 2:
                (imgs, acts, captions, glove_captions, cap_lens, gt_hmaps, bbox_maps_fwd, bbox_maps_bwd, bbox_fmaps, rois,
                 fm_rois, num_rois, gt_bt_masks, gt_fm_bt_masks, class_ids, keys, sent_ids) = prepare_data(data, self.device)
            else:
                (imgs, acts, captions, glove_captions, cap_lens, bbox_maps_fwd, bbox_maps_bwd, bbox_fmaps, rois, fm_rois,
                 num_rois, class_ids, keys, sent_ids) = prepare_gen_data(data, self.device)
                gt_hmaps = gt_bt_masks = gt_fm_bt_masks = None
            batch_size = len(keys)
            # (3) text embeddings (needed again by the R-precision pool, so computed here and handed to sampling)
            max_len = int(_host(cap_lens).max())
            words_embs, sent_emb = text_encoder(captions, cap_lens, max_len)
            words_embs, sent_emb = words_embs.detach().clone(), sent_emb.detach().clone()
            num_words = words_embs.size(2)
            gw = torch.nn.functional.embedding(glove_captions.reshape(-1), self.glove_emb.weight)
            batch = {"rois": rois, "fm_rois": fm_rois, "num_rois": num_rois, "hmaps": gt_hmaps, "bt_masks": gt_bt_masks,
                     "fm_bt_masks": gt_fm_bt_masks, "bbox_maps_fwd": bbox_maps_fwd, "bbox_maps_bwd": bbox_maps_bwd,
                     "bbox_fmaps": bbox_fmaps, "words_embs": words_embs, "sent_emb": sent_emb,
                     "glove_words_embs": gw.view(glove_captions.size(0), glove_captions.size(1), -1)[:, :num_words]
                     .transpose(1, 2), "mask": (captions == 0)[:, :num_words]}
            # (2), (4) layout and fake images
            noise_img = noise_fn('img', (batch_size, cfg.GAN.Z_DIM))
            noise_shp = noise_fn('shp', (batch_size, cfg.ROI.BOXES_NUM, self.num_classes * 4)) \
                if cfg.TEST.USE_GT_BOX_SEG > 0 else None
            out = self.sampling(batch, clabels_emb, hmap_size, noise_img=noise_img, noise_shp=noise_shp)
            images = out["fake_imgs"][-1].detach()
            if gen_iterations % self.display_interval == 0:
                if save_images:
                    self.save_singleimages(images, keys, sent_ids)
                if snapshots:
                    self.save_img_results(out["fake_imgs"], out["attn_maps"], out["bt_attn_maps"], captions, cap_lens,
                                          gen_iterations)
                    if cfg.TEST.USE_GT_BOX_SEG > 0:
                        self.save_shape_results(imgs[0], out["raw_masks"], rois[0], num_rois, gen_iterations, 'G')
                        if gt_hmaps is not None:
                            self.save_shape_results(imgs[0], gt_hmaps[0].squeeze(), rois[0], num_rois, gen_iterations, 'D')
                print('%d / %d' % (gen_iterations, self.num_batches))
            # (5) intermediate results
            region_features, cnn_code = image_encoder(images)
            pool.step(region_features, cnn_code, words_embs, sent_emb, class_ids, cap_lens)
            pred = out["is_pred"].cpu().numpy()                   # the one device-to-host copy of a batch
            predictions.append(pred)
            fake_acts = get_activations(images, self.inception_model_fid, batch_size)
            fake_stats.add(fake_acts)
            real_stats.add(torch.from_numpy(np.ascontiguousarray(acts)))
            if trace is not None:
                trace.append({"keys": list(keys), "sent_ids": [int(s) for s in sent_ids], "fake_img": images.cpu(),
                              "fake_acts": fake_acts.cpu(), "pred": pred})
            gen_iterations += 1
            if gen_iterations >= cfg.TEST.TEST_IMG_NUM:
                break
        # (6) evaluation
        predictions = np.concatenate(predictions, 0)
        splits = min(10, self.batch_size)
        mean, std = compute_inception_score(predictions, splits)
        mean_conf, std_conf = negative_log_posterior_probability(predictions, splits)
        accu_w, std_w = np.mean(pool.w_accuracy), np.std(pool.w_accuracy)
        accu_s, std_s = np.mean(pool.s_accuracy), np.std(pool.s_accuracy)
        real_mu, real_sigma = real_stats.finalize()
        fake_mu, fake_sigma = fake_stats.finalize()
        fid_score = calculate_frechet_distance(real_mu, real_sigma, fake_mu, fake_sigma)
        scores = (mean, std, mean_conf, std_conf, accu_w, std_w, accu_s, std_s, fid_score)
        if self.score_dir:
            with open('%s/scores.txt' % self.score_dir, 'w') as fp:
                fp.write(SCORES_HEADER)
                fp.write('%f, %f, %f, %f, %f, %f, %f, %f, %f' % scores)
        print('inception_score: mean, std, mean_conf, std_conf, accu_w, std_w, accu_s, std_s, fid_score')
        print('inception_score: %f, %f, %f, %f, %f, %f, %f, %f, %f' % scores)
        self.rp_pool = pool
        return scores

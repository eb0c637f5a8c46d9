#!/usr/bin/env python
"""Build tests/golden/data_tiny_eval/ (a prepared Obj-GAN data directory with 4 training and 6 test images, ground-truth
and generated test layouts) and record in tests/golden/eval_ref.pt what the UNMODIFIED reference returns for it:

  (a) data path   TestDataset items and prepare_data / prepare_gen_data / prepare_acts_data for USE_GT_BOX_SEG 0 and 2
  (b) FID         calculate_activation_statistics / calculate_frechet_distance on two seeded activation sets
  (c) R-precision words_loss / sent_loss (is_training=False) on a seeded pool of 100: similarity matrices, accuracies
  (d) end to end  one run of condGANEvaluator.dump_fid_acts + evaluate on the CPU with seeded networks: the noise
                  drawn, per image the fake image (fingerprint), FID activation and Inception prediction, the pool
                  similarities and the nine scores.  The activation pickle the reference wrote stays in the directory.

The reference's testDataset.py and evaluator.py are imported as they are through oracle/ref_data_harness.py; the
recording shims (noise, similarity matrices, activations) live here.  Needs /root/reference; the committed outputs are
what the tests read.

    python tests/golden/make_golden_eval.py
"""
import os
import pickle
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import ref_harness as RH, ref_data_harness as H, torch_encoders as TE     # noqa: E402
import make_golden_data as MGD                                                          # noqa: E402

DATA = os.path.join(HERE, "data_tiny_eval")
SEEDS = {"text": 21, "inception": 4, "emb": 5, "G": 17, "items": 11, "torch": 100, "pool": 9, "acts": (31, 32)}
POOL = {"P": 100, "nef": 256, "L": 12}


def seeded_emb_(enc, seed):
    """the two projections of a CNN_ENCODER, U(-0.1, 0.1) from a generator (the trunk is seeded on its own)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in (enc.emb_features.weight, enc.emb_cnn_code.weight, enc.emb_cnn_code.bias):
            p.copy_(torch.rand(p.shape, generator=g) * 0.2 - 0.1)
    return enc


def pool_inputs(seed=SEEDS["pool"], P=POOL["P"], nef=POOL["nef"], L=POOL["L"]):
    """the seeded R-precision pool the CPU test regenerates: captions are noisy copies of a direction that their image's
    regions contain, so that most rows have a clear best match"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(P, nef, generator=g)
    regions = 0.5 * torch.randn(P, nef, 17, 17, generator=g) + base.view(P, nef, 1, 1) * \
        (torch.rand(P, 1, 17, 17, generator=g) < 0.3).float()
    words = 0.7 * torch.randn(P, nef, L, generator=g) + base.view(P, nef, 1)
    cap_lens = torch.sort(torch.randint(3, L + 1, (P,), generator=g), descending=True)[0]
    cap_lens[0] = L
    codes = base + 0.8 * torch.randn(P, nef, generator=g)
    sents = base + 0.8 * torch.randn(P, nef, generator=g)
    class_ids = torch.randint(0, 60, (P,), generator=g).numpy()                  # repeated ids: masked mismatches
    return regions, codes, words, sents, class_ids, cap_lens


def fid_inputs():
    out = []
    for seed, shift in zip(SEEDS["acts"], (0.3, 0.35)):
        g = torch.Generator().manual_seed(seed)
        out.append(torch.clamp(shift + 0.4 * torch.randn(256, 64, generator=g), min=0).double().numpy())
    return out


def gap_ok(sims, bound_rel=1e-3):
    """rows of a similarity matrix whose best and second-best entries are further apart than twice the bound"""
    top = torch.topk(sims, 2, dim=1).values
    return (top[:, 0] - top[:, 1]) > 2 * bound_rel * top[:, 0].abs()


# ---- the tiny evaluation directory -----------------------------------------------------------------------------------
def build_directory(ns):
    rng = np.random.RandomState(19)
    shutil.rmtree(DATA, ignore_errors=True)
    for sub in ("train", "test", "images"):
        os.makedirs(os.path.join(DATA, sub))
    train = ["COCO_train2014_%012d" % i for i in (9, 25, 30, 34)]
    test = ["COCO_val2014_%012d" % i for i in (42, 73, 74, 133, 136, 139)]
    for split, names in (("train", train), ("test", test)):
        with open(os.path.join(DATA, split, "filenames.pickle"), "wb") as f:
            pickle.dump(names, f, protocol=2)
    with open(os.path.join(DATA, "categories.txt"), "w") as f:
        f.write("".join("%d,%s\n" % c for c in MGD.CATS))
    words = MGD.WORDS
    ixtoword = {0: "<end>"}
    ixtoword.update({i + 1: w for i, w in enumerate(words)})
    wordtoix = {w: i for i, w in ixtoword.items()}
    glove_itos = ["<unk>", "<pad>"] + sorted(words)
    glove_stoi = {w: i for i, w in enumerate(glove_itos)}

    def captions(n_imgs):
        caps, gcaps = [], []
        for _ in range(n_imgs * 5):
            n = int(rng.choice([3, 5, 6, 9, 12, 13, 17]))
            ws = [words[k] for k in rng.randint(0, len(words), n)]
            caps.append([wordtoix[w] for w in ws])
            g = [glove_stoi[w] for w in ws]
            gcaps.append(g[:-1] if rng.rand() < 0.25 and n > 3 else g)
        return caps, gcaps
    tr_c, tr_g = captions(len(train))
    te_c, te_g = captions(len(test))
    with open(os.path.join(DATA, "captions.pickle"), "wb") as f:
        pickle.dump([tr_c, te_c, ixtoword, wordtoix], f, protocol=2)
    Vocab = ns._stubs["torchtext.vocab"].Vocab
    vocabs = []
    for seed in (1, 2):
        v = Vocab()
        v.itos, v.stoi = list(glove_itos), dict(glove_stoi)
        v.vectors = torch.randn(len(glove_itos), 50, generator=torch.Generator().manual_seed(seed))
        vocabs.append(v)
    with open(os.path.join(DATA, "captions_glove.pickle"), "wb") as f:
        pickle.dump([tr_g, te_g, vocabs[0], vocabs[1]], f, protocol=2)
    shapes = [(48, 37), (64, 64), (30, 50), (71, 90), (40, 40), (33, 65), (56, 56), (44, 80), (90, 61), (64, 48)]
    for name, (h, w) in zip(train + test, shapes):
        with open(os.path.join(DATA, "images", name + ".jpg"), "wb") as f:
            f.write(MGD.smooth_image(rng, h, w))
    ns.load.write_imgs(DATA, train, os.path.join(DATA, "train_imgs.bigfile"))
    ns.load.write_imgs(DATA, test, os.path.join(DATA, "test_imgs.bigfile"))
    shutil.rmtree(os.path.join(DATA, "images"))

    def slim(ann, keep_masks):
        ann = dict(ann)
        ann["pooled masks"] = None                              # read by nothing downstream of the pickles
        if ann["bbox maps"] is not None:                        # 0 / 1 maps: bytes instead of float64
            ann["bbox maps"] = ann["bbox maps"].astype(np.uint8)
            ann["bbox fmaps"] = ann["bbox fmaps"].astype(np.uint8)
        if not keep_masks:
            ann["masks"] = None
        return ann
    gt = {name: slim(MGD.make_ann(rng, n), True) for name, n in zip(test, (2, 1, 0, 1, 1, 1))}
    with open(os.path.join(DATA, "test_gt_insanns.pickle"), "wb") as f:
        pickle.dump([gt], f, protocol=2)
    gen = {name: [slim(MGD.make_ann(rng, int(rng.choice([0, 1, 1, 2]))), False) for _ in range(5)] for name in test}
    with open(os.path.join(DATA, "test_gen_insanns.pickle"), "wb") as f:
        pickle.dump([gen], f, protocol=2)


# ---- the reference's testDataset.py and evaluator.py -----------------------------------------------------------------
def load_reference_eval(ns):
    base = RH.load_reference(branch_num=3)
    mods = {n: m for n, m in base._modules.items() if m is not None}
    mods.update({"miscc.load": ns.load, "trainDataset": ns.trainDataset, "trainer": ns.trainer})
    pkg = os.path.join(ROOT, "obj-gan_amd")
    names = list(mods) + ["testDataset", "evaluator"]
    saved = {n: sys.modules.pop(n) for n in names + list(ns._stubs) if n in sys.modules}
    saved_path = list(sys.path)
    try:
        sys.modules.update(ns._stubs)
        sys.modules.update(mods)
        sys.path = [RH.REF_ROOT] + [p for p in sys.path if os.path.abspath(p) != os.path.abspath(pkg)]
        import testDataset as ref_td
        import evaluator as ref_ev
    finally:
        sys.path = saved_path
        for n in names + list(ns._stubs):
            sys.modules.pop(n, None)
        sys.modules.update(saved)
    return base, ref_td, ref_ev


class _RecordingNN(object):
    """`nn` as the reference's losses module sees it: CrossEntropyLoss()(scores, labels) also records the scores"""

    def __init__(self, sink):
        self.sink = sink

    def __getattr__(self, k):
        return getattr(torch.nn, k)

    def CrossEntropyLoss(self):
        inner = torch.nn.CrossEntropyLoss()

        def call(scores, labels):
            self.sink.append(scores.detach().clone())
            return inner(scores, labels)
        return call


def fp(t, step=16):
    """make_golden_data.fingerprint with a coarser sample grid (the 256 x 256 maps of ten box slots add up)"""
    t = torch.as_tensor(t).double()
    return {"shape": tuple(t.shape), "sum": float(t.sum()), "sq": float((t * t).sum()), "step": step,
            "sample": t[..., ::step, ::step].float().clone()}


def record_item(it, mode):
    if mode == 0:
        (imgs, acts, caps, gcaps, cap_len, hmaps, fwd, bwd, fmaps, rois, fm_rois, num_rois, bt, fm_bt, cls_id, key,
         sent) = it
    else:
        imgs, acts, caps, gcaps, cap_len, fwd, bwd, fmaps, rois, fm_rois, num_rois, cls_id, key, sent = it
    rec = {"len": len(it), "img64": fp(imgs[0], 8), "img256": fp(imgs[2]), "acts_sum": float(np.sum(acts)),
           "caps": torch.as_tensor(caps), "glove_caps": torch.as_tensor(gcaps), "cap_len": int(cap_len),
           "fwd": fp(fwd), "bwd": fp(bwd), "fmaps": torch.as_tensor(fmaps).float(),
           "rois": [torch.as_tensor(r) for r in rois], "fm_rois": torch.as_tensor(fm_rois), "num_rois": int(num_rois),
           "cls_id": int(cls_id), "key": key, "sent": int(sent)}
    if mode == 0:
        rec.update({"hmap64": fp(hmaps[0]), "hmap256": fp(hmaps[2]), "bt_mask64": fp(bt[0]), "bt_mask256": fp(bt[2]),
                    "fm_bt_masks": fp(fm_bt)})
    return rec


def record_prepared(p, mode):
    if mode == 0:
        imgs, acts, caps, gcaps, lens, hmaps, fwd, bwd, fmaps, rois, fm_rois, num, bt, fm_bt, cls, keys, sents = p
    else:
        imgs, acts, caps, gcaps, lens, fwd, bwd, fmaps, rois, fm_rois, num, cls, keys, sents = p
    rec = {"len": len(p), "img64": fp(imgs[0], 8), "img256": fp(imgs[2]), "acts": fp(torch.as_tensor(acts).view(1, len(keys), -1), 1),
           "acts_dtype": str(acts.dtype), "captions": caps, "glove_captions": gcaps, "cap_lens": lens,
           "fwd": fp(fwd), "fwd_shape": tuple(fwd.shape), "bwd": fp(bwd), "fmaps": fmaps, "rois": rois, "fm_rois": fm_rois,
           "num_rois": num, "class_ids": np.asarray(cls), "keys": list(keys), "sent_ids": [int(s) for s in sents],
           "dtypes": {"fwd": str(fwd.dtype), "rois": str(rois[0].dtype), "captions": str(caps.dtype)}}
    if mode == 0:
        rec.update({"hmap64": fp(hmaps[0]), "hmap256": fp(hmaps[2]), "bt_mask64": fp(bt[0]), "fm_bt_masks": fp(fm_bt),
                    "dtypes": dict(rec["dtypes"], hmaps=str(hmaps[0].dtype), bt_masks=str(bt[0].dtype))})
    return rec


def write_checkpoints(base, ds, tmp):
    """seeded networks as the checkpoint files the reference evaluator reads"""
    os.makedirs(os.path.join(tmp, "pretrained"))
    net_e = os.path.join(tmp, "pretrained", "text_encoder100.pth")
    base.cfg.TRAIN.NET_E = net_e
    torch.save(TE.seeded_init_(TE.inception_v3(), SEEDS["inception"]).state_dict(),
               net_e.replace("text_encoder100.pth", "inception_v3_google-1a9a5a14.pth"))
    text = RH.seeded_state_(base.model.RNN_ENCODER(ds.n_words, nhidden=256), SEEDS["text"])
    torch.save(text.state_dict(), net_e)
    img = seeded_emb_(base.model.CNN_ENCODER(256), SEEDS["emb"])
    torch.save(img.state_dict(), net_e.replace("text_encoder", "image_encoder"))
    G = RH.seeded_state_(base.model.G_NET(len(ds.cats_index_dict)), SEEDS["G"])
    base.cfg.TRAIN.NET_G = os.path.join(tmp, "netG.pth")
    torch.save(G.state_dict(), base.cfg.TRAIN.NET_G)


def main():
    ns = H.load_reference_data(branch_num=3)
    with H.active(ns):
        base, ref_td, ref_ev = load_reference_eval(ns)
        cfg = base.cfg
        cfg.CUDA = False
        cfg.TEST.USE_TF = 0
        cfg.TEST.SAMPLE_VAL = False
        cfg.TEST.SAVE_OPTIONS = 'IMAGE'
        cfg.TRAIN.BATCH_SIZE = 2
        cfg.TRAIN.DISPLAY_INTERVAL = 1
        cfg.TEST.RP_POOL_SIZE = 4
        cfg.TREE.BRANCH_NUM = 3
        build_directory(ns)
        out = {"seeds": SEEDS}
        from torch.utils.data.dataloader import default_collate
        tmp = tempfile.mkdtemp()

        # (d) first half: the activation pass (the directory has no activation file yet)
        cfg.TEST.USE_GT_BOX_SEG = 0
        ds = ref_td.TestDataset(DATA, "test", base_size=64)
        assert ds.acts_dict is None
        first = ds[0]
        acts_batch = ref_td.prepare_acts_data(default_collate([ds[0], ds[1]]))
        out["acts_pass"] = {"item_len": len(first), "key": first[1], "img64": fp(first[0][0], 8),
                            "prepared_len": len(acts_batch), "keys": list(acts_batch[1]), "img256": fp(acts_batch[0][2])}
        write_checkpoints(base, ds, tmp)
        loader = torch.utils.data.DataLoader(ds, batch_size=2, drop_last=True, shuffle=False, num_workers=0)
        ev = ref_ev.condGANEvaluator(os.path.join(tmp, "out"), loader, ds)
        ev.dump_fid_acts(DATA, "test")
        ds.acts_dict = ns.load.load_acts_data(DATA, "test")

        # (a) data path
        out["data"] = {}
        for mode in (0, 2):
            cfg.TEST.USE_GT_BOX_SEG = mode
            dsm = ref_td.TestDataset(DATA, "test", base_size=64)
            np.random.seed(SEEDS["items"])
            items = [dsm[i] for i in range(len(dsm))]
            np.random.seed(SEEDS["items"])
            batch = default_collate([dsm[i] for i in range(len(dsm))])
            prepared = (ref_td.prepare_data if mode == 0 else ref_td.prepare_gen_data)(batch)
            out["data"][mode] = {"items": [record_item(it, mode) for it in items],
                                 "prepared": record_prepared(prepared, mode)}
        cfg.TEST.USE_GT_BOX_SEG = 0

        # (b) Frechet distance
        a, b = fid_inputs()
        mu1, s1 = base.utils.calculate_activation_statistics(a)
        mu2, s2 = base.utils.calculate_activation_statistics(b)
        out["fid"] = {"mu1": mu1, "sigma1": s1, "mu2": mu2, "sigma2": s2,
                      "fid": float(base.utils.calculate_frechet_distance(mu1, s1, mu2, s2))}

        # (c) R-precision on a seeded pool
        sink = []
        real_nn = base.losses.nn
        base.losses.nn = _RecordingNN(sink)
        try:
            regions, codes, words, sents, class_ids, cap_lens = pool_inputs()
            labels = torch.arange(POOL["P"])
            _, _, _, w_accu = base.losses.words_loss(regions, words, labels, cap_lens, class_ids, POOL["P"], is_training=False)
            _, _, s_accu = base.losses.sent_loss(codes, sents, labels, class_ids, POOL["P"], is_training=False)
            w_sims, s_sims = sink[0], sink[2]
            left_out = [float((~gap_ok(m)).float().mean()) for m in (w_sims, w_sims.t(), s_sims, s_sims.t())]
            print("pool: w_accu %.1f s_accu %.1f, rows without a clear gap: %s" % (w_accu, s_accu, left_out))
            assert max(left_out) <= 0.05, "reseed the pool: too many rows without a clear best match"
            out["pool"] = {"w_sims": w_sims, "s_sims": s_sims, "w_accu": w_accu, "s_accu": s_accu}

            # (d) second half: evaluate, with everything random recorded
            del sink[:]
            draws, act_calls, preds = [], [], []
            real_normal = torch.Tensor.normal_

            def recording_normal(self, *a, **k):
                r = real_normal(self, *a, **k)
                if tuple(r.shape) == (2, 100):           # the generator noise and the CA_NET eps of a batch, nothing else
                    draws.append(r.detach().clone())
                return r
            real_get = ref_ev.get_activations

            def recording_get(images, model, batch_size, verbose=False):
                r = real_get(images, model, batch_size, verbose)
                act_calls.append((images.detach().clone(), np.array(r)))
                return r
            hook = ev.inception_model.register_forward_hook(lambda m, i, o: preds.append(o.detach().clone()))
            torch.Tensor.normal_ = recording_normal
            ref_ev.get_activations = recording_get
            try:
                torch.manual_seed(SEEDS["torch"])
                np.random.seed(SEEDS["items"])
                ev.evaluate("test", ds.imsize)
            finally:
                torch.Tensor.normal_ = real_normal
                ref_ev.get_activations = real_get
                hook.remove()
        finally:
            base.losses.nn = real_nn
        with open(os.path.join(tmp, "out", "Score", "scores.txt")) as f:
            header, values = f.read().split("\n")
        nb = len(act_calls)
        assert len(draws) == 2 * nb and len(preds) == nb and len(sink) == 4, (len(draws), nb, len(preds), len(sink))
        out["e2e"] = {
            "header": header + "\n", "scores": [float(v) for v in values.split(",")],
            "noise_img": [draws[2 * i] for i in range(nb)], "ca_eps": [draws[2 * i + 1] for i in range(nb)],
            "fake_img": [fp(im) for im, _ in act_calls], "fake_acts": [torch.from_numpy(a).float() for _, a in act_calls],
            "pred": preds, "w_sims": sink[0], "s_sims": sink[2],
            "images_written": sorted(os.listdir(os.path.join(tmp, "out", "Image"))),
            "cfg": {"BATCH_SIZE": 2, "RP_POOL_SIZE": 4, "DISPLAY_INTERVAL": 1, "USE_GT_BOX_SEG": 0}}
        print("scores:", out["e2e"]["scores"])
        shutil.rmtree(tmp)
    torch.save(out, os.path.join(HERE, "eval_ref.pt"))
    sz = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(DATA) for f in fs)
    print("data_tiny_eval: %d KB, golden: %d KB" % (sz // 1024, os.path.getsize(os.path.join(HERE, "eval_ref.pt")) // 1024))


if __name__ == "__main__":
    main()

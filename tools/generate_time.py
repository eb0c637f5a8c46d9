#!/usr/bin/env python
"""Time of one batch of captions through pipeline.TextToImage at the reference's shapes (one MI355X): 80 categories, box
decoder H = 256 / 84 labels / K = 5 / T = 10, DAMSM encoder 256, G_NET and SHP_G_NET at their configured widths, all with
seeded random weights (no checkpoint is read; time does not depend on the values).

Per stage, device events after `--warmup` batches, median of `--steps`: encoder + decode | layout stage (with its one
device-to-host copy) | shape generator | form_hmaps | image generator.  Then the HOST file route between the same decoder
samples and the same device tensors -- write_layouts -> load_gen_insanns -> get_gen_rois -> collate -> prepare_gen_data
-- by the wall clock.  Prints one JSON line; `--out` also writes it.  Not a test: asserts nothing about time.

    python tools/generate_time.py [--B 16] [--steps 10] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "obj-gan_amd"))


def build(dev, B, seed=0):
    import evaluator as E
    import model as M
    import pipeline
    from miscc.config import cfg
    from seq2seq.evaluator import Evaluator
    from seq2seq.models import DecoderRNN, PreEncoderRNN
    torch.manual_seed(seed)
    C, V = 80, 2000
    words = ["w%d" % i for i in range(V)]
    wordtoix = {w: i + 1 for i, w in enumerate(words)}
    wordtoix["<end>"] = 0
    labels = ["<pad>", "<sos>", "<eos>", "<unk>"] + [str(c + 1) for c in range(C)]
    lang = types.SimpleNamespace(index2word=dict(enumerate(labels)), word2index={w: i for i, w in enumerate(labels)})
    decoder = DecoderRNN(lang.word2index, 0.0, 0.0, 0.0, 0.0, 1, 150, 256, 5, bidirectional=True)
    for p in decoder.parameters():
        p.data.uniform_(-0.08, 0.08)
    decoder.l_out.bias.data[:4] -= 4.0                       # full-length sequences: every step decodes a box
    encoder = PreEncoderRNN(V + 1, nhidden=256).eval()
    gauss = {c + 1: (3.0, 1.0) for c in range(C)}
    layout = Evaluator(B, 10, '', None, lang, (128.0, 60.0), (128.0, 60.0), (90.0, 40.0), (1.0, 0.35), gauss, '', 0)
    ds = types.SimpleNamespace(n_words=V + 1, ixtoword={i: w for w, i in wordtoix.items()}, cats_dict={},
                               cats_index_dict={c + 1: c for c in range(C)},
                               glove_embed=torch.nn.Embedding(V + 1, cfg.TEXT.GLOVE_EMBEDDING_DIM),
                               cat_labels=torch.randint(1, V, (C, 2)), cat_label_lens=torch.full((C,), 2),
                               sorted_cat_label_indices=torch.arange(C),
                               text_encoder=M.RNN_ENCODER(V + 1, nhidden=cfg.TEXT.EMBEDDING_DIM))
    cfg.TEST.USE_GT_BOX_SEG, cfg.TRAIN.BATCH_SIZE = 2, B
    imager = E.condGANEvaluator('', None, ds, device=dev)
    imager.text_encoder.to(dev).eval()
    imager.glove_emb.to(dev).eval()
    imager.netG = M.G_NET(C).to(dev).eval()
    imager.netShpG = M.SHP_G_NET(C).to(dev).eval()
    t2i = pipeline.TextToImage(encoder.to(dev), decoder.to(dev).eval(), layout, wordtoix, imager, wordtoix, wordtoix, dev,
                               batch_size=B)
    rs = np.random.RandomState(seed)
    captions = [" ".join(words[i] for i in rs.randint(0, V, size=rs.randint(5, 13))) for _ in range(B)]
    return t2i, captions


def instrument(t2i):
    """marks around the shape generator and form_hmaps inside condGANEvaluator.sampling"""
    import evaluator as E
    shp, form = t2i.imager.netShpG, E.form_hmaps

    class Marked(torch.nn.Module):
        def forward(self, *a):
            t2i._mark("text embeddings")
            out = shp(*a)
            t2i._mark("shape generator")
            return out
    t2i.imager.netShpG = Marked()

    def marked_form(*a, **k):
        out = form(*a, **k)
        t2i._mark("form_hmaps")
        return out
    E.form_hmaps = marked_form


def file_route(t2i, dev):
    """the host route for the last batch's decoder samples -> the tensors prepare_gen_data hands to the evaluator"""
    import testDataset
    from miscc import load
    from miscc.config import cfg
    labels, lengths, samples = (t.cpu().numpy() for t in t2i.last_decode)
    B = labels.shape[0]
    decoded = [(labels[b, :lengths[b]].astype(np.int64), [(s[0], s[1]) for s in samples[b, :lengths[b]]],
                [(s[2], s[3]) for s in samples[b, :lengths[b]]]) for b in range(B)]
    keys = ["k%d" % b for b in range(B)]
    cid, W = t2i.imager.cats_index_dict, cfg.TEXT.WORDS_NUM
    with tempfile.TemporaryDirectory() as d:
        t2i.layout.box_saving_folder = os.path.join(d, "gen_masks") + "/"
        t0 = time.perf_counter()
        t2i.layout.write_layouts(decoded, keys)
        anns = load.load_gen_insanns(d, keys, 'test', t2i.imsize, cfg.ROI.FM_SIZE, cid)
        items = [([torch.zeros(1)] * 3, np.zeros(1), np.zeros((W, 1), np.int64), np.zeros((W, 1), np.int64), W - b % 3)
                 + tuple(load.get_gen_rois(anns[k], t2i.imsize, cfg.ROI.FM_SIZE, cid, 0)) + (0, k, b)
                 for b, k in enumerate(keys)]
        out = testDataset.prepare_gen_data(torch.utils.data.default_collate(items), dev)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, int(out[10].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    t2i, captions = build(dev, args.B)
    instrument(t2i)
    stages = {}
    for step in range(args.warmup + args.steps):
        t2i.events = []
        t2i.generate(captions, seed=step, notice=False)
        torch.cuda.synchronize()
        if step >= args.warmup:
            ev = t2i.events
            for (_, a), (name, b) in zip(ev[:-1], ev[1:]):
                stages.setdefault(name, []).append(a.elapsed_time(b))
    t2i.events = None
    import sys as _sys
    _sys.stdout = _sys.stderr                    # the readers print progress lines
    host = [file_route(t2i, dev) for _ in range(5)]
    _sys.stdout = _sys.__stdout__
    med = {k: round(statistics.median(v), 3) for k, v in stages.items()}
    med["image generator"] = med.pop("shape + image generator")
    res = {"B": args.B, "steps": args.steps, "stage_ms_median": med, "total_ms": round(sum(med.values()), 3),
           "host_file_route_ms_median": round(statistics.median(h[0] for h in host), 3), "boxes_in_batch": host[0][1]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

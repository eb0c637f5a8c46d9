#!/usr/bin/env python
"""Milliseconds of one DAMSM pretraining step (damsm_trainer.DAMSMTrainer.train_step) at the recipe's shape -- B = 48
captions of up to L = 12 words, I = 300, H = 128, a COCO-sized vocabulary, 299 x 299 images -- and its split: the frozen
Inception trunk alone, the two losses forward + backward given features and embeddings, the text encoder forward +
backward (csrc/lstm_train.hip) alone; for orientation the same text encoder written with torch.nn.Embedding /
nn.Dropout / nn.LSTM on a packed sequence, forward + backward on the same device.  Seeded random images and trunk
weights: time does not depend on the values.  Host clock around work that ends in a device synchronise; every figure
is the median of --repeats windows of --steps calls after --warmup calls.  Prints one JSON line.

    python tools/damsm_time.py [--steps 100] [--warmup 5] [--repeats 5] [--out profiles/damsm_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "obj-gan_amd"))

B, L, I, H, NTOKEN, NEF = 48, 12, 300, 128, 27297, 256


def timed(fn, steps, warmup, repeats):
    """-> (median, min, max) milliseconds per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) * 1000.0 / steps)
    return [round(v, 3) for v in (statistics.median(windows), min(windows), max(windows))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("damsm_time.py: needs the GPU (a CPU run gives no time)")
    import damsm_trainer
    import encoders
    import model as M
    from miscc.losses import words_loss, sent_loss
    from miscc.utils import attach_host
    from objgan_hip import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    text = M.RNN_ENCODER(NTOKEN, nhidden=2 * H).to(dev).train()
    image = encoders.CNN_ENCODER(NEF, encoders.seeded_init_(encoders.inception_v3(), 1))
    for k, p in image.named_parameters():
        p.requires_grad_(k in damsm_trainer.PROJECTION_KEYS)
    image.train_projections = True
    image.to(dev).eval()
    tr = damsm_trainer.DAMSMTrainer('', None, None, dev, text, image)
    imgs = torch.tanh(torch.randn(B, 3, 299, 299, generator=g)).to(dev)
    caps = torch.randint(1, NTOKEN, (B, L), generator=g).to(dev)
    lens_h = torch.sort(torch.randint(5, L + 1, (B,), generator=g), descending=True)[0]
    lens_h[0] = L
    lens = attach_host(lens_h.to(dev), lens_h)
    class_ids = np.arange(B)
    labels = torch.arange(B, device=dev)
    t = lambda fn: timed(fn, args.steps, args.warmup, args.repeats)  # noqa: E731
    out = {"shape": {"B": B, "L": L, "I": I, "H": H, "ntoken": NTOKEN, "nef": NEF, "image": 299},
           "conv_math": ops.get_conv_math(), "steps": args.steps, "repeats": args.repeats,
           "ms": "median, min, max of the windows"}

    out["step_ms"] = t(lambda: tr.train_step(imgs, caps, lens, class_ids))

    def trunk():
        with torch.no_grad():
            return encoders.inception_trunk(image, ops.bilinear_resize(imgs, 299, 299), want_regions=True)
    out["trunk_ms"] = t(trunk)

    feats = torch.randn(B, NEF, 17, 17, generator=g).to(dev)
    code = torch.randn(B, NEF, generator=g).to(dev)
    words0, sent0 = (v.detach() for v in text(caps, lens, L))

    def loss():
        f, c, w, s = (v.clone().requires_grad_() for v in (feats, code, words0, sent0))
        w0, w1, _, _ = words_loss(f, w, labels, lens, class_ids, B, top1=False, need_att_maps=False)
        s0, s1, _ = sent_loss(c, s, labels, class_ids, B, top1=False)
        (w0 + w1 + s0 + s1).backward()
    out["loss_ms"] = t(loss)

    d_w, d_s = torch.randn_like(words0), torch.randn_like(sent0)

    def lstm():
        tr.arena.zero_grad()
        w, s = text(caps, lens, L)
        torch.autograd.backward((w, s), (d_w, d_s))
    out["lstm_fwd_bwd_ms"] = t(lstm)

    emb = torch.nn.Embedding(NTOKEN, I).to(dev)
    drop = torch.nn.Dropout(0.5)
    rnn = torch.nn.LSTM(I, H, 1, batch_first=True, bidirectional=True).to(dev)
    lens_list = lens_h.tolist()

    def stock():
        emb.zero_grad()
        rnn.zero_grad()
        packed = pack_padded_sequence(drop(emb(caps)), lens_list, batch_first=True)
        o, (h, _) = rnn(packed)
        w = pad_packed_sequence(o, batch_first=True)[0].transpose(1, 2)
        s = h.transpose(0, 1).reshape(B, 2 * H)
        torch.autograd.backward((w, s), (d_w[:, :, :w.shape[2]], d_s))
    out["torch_nn_lstm_fwd_bwd_ms"] = t(stock)

    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

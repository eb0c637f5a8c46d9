#!/usr/bin/env python
"""Captions per second of the box generator's fused training step (csrc/box_train.hip + fused Adam) at the real shape
(H = 256, 83 labels, K = 5, 10 steps per caption) for B = 1, 64, 1024, against the same step written with stock torch.nn
modules on the same device, batched over captions AND over time (one nn.LSTM call for all steps, nn.Linear heads and
both losses on the B * T rows at once, autograd, clip_grad_norm_, torch.optim.Adam) -- what a user would otherwise
run.  Prints one JSON line per batch size.

    python tools/boxgen_train_bench.py [--steps 20] [--warmup 5] [--out profiles/boxgen_train_bench.json]
"""
import argparse
import json
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "obj-gan_amd"))

H, L, K, T = 256, 83, 5, 10


def targets(B, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(4, L, (B, T + 1), generator=g)
    labels[:, 0], labels[:, T] = 1, 2
    boxes = torch.randn(B, T + 1, 4, generator=g)
    return labels.to(dev), boxes.to(dev), torch.randn(B, H, generator=g).to(dev) * 0.3, \
        torch.randn(B, H, generator=g).to(dev) * 0.3


def pdf(par, x, y):
    pi, ux, uy, sx, sy, rho = par
    x, y = x[:, None], y[:, None]
    z = ((x - ux) / sx) ** 2 + ((y - uy) / sy) ** 2 - 2 * rho * (x - ux) * (y - uy) / (sx * sy)
    a = -z / (2 * (1 - rho ** 2))
    a_max = a.max(dim=1, keepdim=True)[0]
    norm = torch.clamp(2 * math.pi * sx * sy * torch.sqrt(1 - rho ** 2), min=1e-5)
    return torch.log((pi * torch.exp(a - a_max) / norm).sum(dim=1) + 1e-5) + a_max[:, 0]


def mixture(raw):
    pi, ua, ub, sa, sb, rho = torch.split(raw, K, dim=1)
    return torch.softmax(pi, dim=1), ua, ub, torch.exp(sa), torch.exp(sb), torch.tanh(rho)


def stock_step(dec, opt, weight, labels, boxes, h0, c0):
    """the batched step with the decoder's own nn modules and autograd.  Teacher forcing makes every input known up
    front, so this is the formulation stock torch is best at: ONE nn.LSTM call over all T steps, the heads and both
    losses evaluated on the B * T rows at once."""
    B = labels.shape[0]
    first = torch.tensor([dec.x_mean, dec.y_mean, dec.w_mean, dec.r_mean], device=labels.device).expand(B, 1, 4)
    box = torch.cat((first, boxes[:, 1:T]), 1)                                     # the inputs of steps 0 .. T - 1
    inp = torch.cat((dec.xy_embedding(box[..., 0:2]), dec.wh_embedding(box[..., 2:4]), dec.l_embedding(labels[:, :T])), 2)
    out, _ = dec.rnn(inp, (h0[None], c0[None]))
    hh = out.reshape(B * T, H)
    nl = labels[:, 1:].reshape(B * T)
    nbox = boxes[:, 1:].reshape(B * T, 4)
    ps = torch.softmax(dec.l_out(hh), dim=1).clamp(1e-5, 1)
    xy_hidden = torch.cat((hh, F.one_hot(nl, L).float()), 1)
    xy = mixture(dec.xy_out(xy_hidden))
    nxy = dec.next_xy_embedding(torch.stack((nbox[:, 0], box[..., 1].reshape(B * T)), 1))
    wh = mixture(dec.wh_out(torch.cat((xy_hidden, nxy), 1)))
    lsum = F.nll_loss(ps, nl, weight=weight, reduction='sum')
    bsum = -pdf(xy, nbox[:, 0], nbox[:, 1]).sum() - pdf(wh, nbox[:, 2], nbox[:, 3]).sum()
    loss = (lsum + bsum) / (B * T)
    opt.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(dec.parameters(), 5)
    opt.step()


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--out", default=None)
    opt = ap.parse_args(argv)
    from seq2seq.models import DecoderRNN
    from seq2seq.trainer import FusedBoxStep
    dev = torch.device("cuda")
    w2i = {w: i for i, w in enumerate(["<pad>", "<sos>", "<eos>", "<unk>"] + [str(i) for i in range(1, L - 3)])}
    rows = []
    for B in opt.batches:
        torch.manual_seed(0)
        labels, boxes, h0, c0 = targets(B, dev)
        weight = torch.ones(L, device=dev)
        weight[0] = 0

        def fresh():
            d = DecoderRNN(w2i, 0.1, -0.2, 0.3, 0.05, B, 150, H, K, bidirectional=True)
            for p in d.parameters():
                p.data.uniform_(-0.08, 0.08)
            return d.to(dev)
        dec = fresh()
        fused = FusedBoxStep(dec, weight)
        lab, box, lens = DecoderRNN.pack_targets(labels, boxes[:, :, 0], boxes[:, :, 1], boxes[:, :, 2], boxes[:, :, 3])
        t_fused = timed(lambda: fused.step(h0, c0, lab, box, lens), opt.steps, opt.warmup)
        dec2 = fresh()
        adam = torch.optim.Adam(dec2.parameters())
        t_stock = timed(lambda: stock_step(dec2, adam, weight, labels, boxes, h0, c0), opt.steps, opt.warmup)
        row = {"B": B, "T": T, "fused_ms": round(t_fused * 1e3, 3), "stock_ms": round(t_stock * 1e3, 3),
               "fused_captions_per_s": round(B / t_fused, 1), "stock_captions_per_s": round(B / t_stock, 1),
               "ratio": round(t_stock / t_fused, 2)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if opt.out:
        with open(opt.out, "w") as f:
            json.dump({"shape": {"H": H, "L": L, "K": K, "T": T}, "steps": opt.steps, "warmup": opt.warmup,
                       "rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

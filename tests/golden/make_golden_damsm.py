#!/usr/bin/env python
"""Record what the UNMODIFIED reference computes for one DAMSM pretraining step of the text encoder, on the CPU:
RNN_ENCODER(ntoken=30, ninput=20, drop_prob=0, nhidden=16) in TRAINING mode, its words_loss and sent_loss, backward.

  tests/golden/damsm_ref.pt
    "config"   shapes, seed, the three gammas of the reference's cfg
    "params"   the encoder's state dict (seeded by tests/damsm_oracle.seeded_text_params)
    "captions" [4, 7] tokens, lengths 7, 5, 5, 1 (the reference packs: descending), tokens repeated inside a caption and
               across captions; "class_ids" with one equal pair; "feats" [4, 16, 3, 3], "codes" [4, 16]
    "words_emb", "sent_emb", "losses" (w_loss0, w_loss1, s_loss0, s_loss1),
    "grads"    d(sum of the four losses) / d(every encoder parameter), "d_feats", "d_codes"

    python tests/golden/make_golden_damsm.py          (needs the reference tree)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import damsm_oracle as DO                                                               # noqa: E402
from oracle import ref_harness as rh                                                    # noqa: E402

CONFIG = {"ntoken": 30, "ninput": 20, "nhidden": 16, "L": 7, "lens": (7, 5, 5, 1), "seed": 73, "class_ids": (11, 4, 11, 9)}
CAPTIONS = ((3, 7, 7, 12, 3, 29, 5), (7, 1, 12, 12, 28), (5, 5, 9, 3, 2), (7,))


def main():
    c = CONFIG
    ns = rh.load_reference()
    enc = ns.model.RNN_ENCODER(c["ntoken"], ninput=c["ninput"], drop_prob=0, nhidden=c["nhidden"])
    params = DO.seeded_text_params(c["ntoken"], c["ninput"], c["nhidden"] // 2, c["seed"])
    enc.load_state_dict(params, strict=True)
    enc.train()
    B = len(CAPTIONS)
    captions = torch.zeros(B, c["L"], dtype=torch.int64)
    for b, cap in enumerate(CAPTIONS):
        assert len(cap) == c["lens"][b]
        captions[b, :len(cap)] = torch.tensor(cap)
    lens = torch.tensor(c["lens"], dtype=torch.int64)
    g = torch.Generator().manual_seed(c["seed"] + 1)
    feats = torch.randn(B, c["nhidden"], 3, 3, generator=g).requires_grad_()
    codes = torch.randn(B, c["nhidden"], generator=g).requires_grad_()
    class_ids = np.asarray(c["class_ids"])
    labels = torch.arange(B)

    words_emb, sent_emb = enc(captions, lens, c["L"])
    w0, w1, _, _ = ns.losses.words_loss(feats, words_emb, labels, lens, class_ids, B)
    s0, s1, _ = ns.losses.sent_loss(codes, sent_emb, labels, class_ids, B)
    enc.zero_grad()
    (w0 + w1 + s0 + s1).backward()
    sm = ns.cfg.TRAIN.SMOOTH
    out = {"config": dict(c, gammas=(float(sm.GAMMA1), float(sm.GAMMA2), float(sm.GAMMA3))),
           "params": {k: v.detach().clone() for k, v in enc.state_dict().items()},
           "captions": captions, "feats": feats.detach().clone(), "codes": codes.detach().clone(),
           "words_emb": words_emb.detach().clone(), "sent_emb": sent_emb.detach().clone(),
           "losses": tuple(float(v.detach()) for v in (w0, w1, s0, s1)),
           "grads": {k: p.grad.detach().clone() for k, p in enc.named_parameters()},
           "d_feats": feats.grad.detach().clone(), "d_codes": codes.grad.detach().clone()}
    assert set(out["grads"]) == set(DO.TEXT_KEYS) and all(torch.isfinite(v).all() for v in out["grads"].values())
    assert out["config"]["gammas"] == DO.GAMMAS
    torch.save(out, DO.GOLDEN)
    print("wrote", DO.GOLDEN, os.path.getsize(DO.GOLDEN), "bytes; losses", out["losses"])


if __name__ == "__main__":
    main()

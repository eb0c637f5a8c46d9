#!/usr/bin/env python
"""Record what the UNMODIFIED reference box generator computes in TRAINING on the CPU, one caption at a time (its batch
size is 1): DecoderRNN.forward(is_training=1), Perplexity, BBLoss, Optimizer(Adam, max_grad_norm=5).step(),
prepare_data and random_batch.

  tests/golden/boxgen_train_ref.pt
    "small"  H = 32, L = 9, K = 2; captions of 1, 1, 2, 4, 4 and 7 steps (1 step = only <eos>): targets, initial
             state, trace, the two loss sums, all 17 gradients of the reference's loss, and for some captions the
             parameters after ONE reference optimizer step (clip active); one caption a second time with all label
             weights 1 ("unclipped": its gradient norm is below 5, verified here)
    "real"   H = 256, L = 83, K = 5 (weights of boxgen_oracle.real_modules); 4 captions of 1-10 steps: trace, loss
             sums, each tensor's gradient norm and its dot product with a seeded direction (direction())
    "data"   prepare_data / random_batch over tests/golden/boxgen_tiny/input_train.txt: vocabularies, counts, label
             weights, and the batches of a seeded random.choice stream
    "curve"  the loss per step of the fp64 restatement (tests/boxgen_train_oracle.py) trained under the schedule
             `sample.py --is_training 1 --seed S --batch_size 4` follows on the tiny input
  tests/golden/boxgen_tiny/input_train.txt   the tiny training input (written here, seeded)

Kept captions satisfy, in the reference's own run: every label probability a factor 2 away from the clamp edge 1e-5,
every mixture norm term a factor 2 above its 1e-5 clamp, all values finite.  Post-step parameters are recorded only for
captions whose first Adam update is the same to 1e-5 from the fp32 and the fp64 restatement of the gradient (see
make_small): elsewhere the reference's own rounding decides the comparison.

    python tests/golden/make_golden_boxgen_train.py          (needs the reference tree and dill)
"""
import importlib
import importlib.util
import math
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "obj-gan_amd"))

import boxgen_oracle as BO                                                              # noqa: E402
import boxgen_train_oracle as TO                                                        # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_boxgen", os.path.join(HERE, "make_golden_boxgen.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)

SMALL = {"H": 32, "L": 9, "K": 2, "lens": (1, 1, 2, 4, 4, 7), "seed": 31, "scale": 0.3, "means": (0.1, -0.2, 0.3, 0.05),
         "count_smooth": 1e5, "stepped": (3,), "unclipped": 3}
REAL = {"lens": (1, 3, 6, 10), "seed": 41, "count_smooth": 1e5, "direction_seed": 43}
DATA = {"seed": 17, "lines": 24, "batches": 3, "batch_size": 4, "count_smooth": 1e5}
CURVE = {"seed": 7, "batch_size": 4, "steps": 204, "num_epochs": 34}


def direction(key, shape, seed):
    """the seeded direction a tensor's gradient is projected on"""
    g = torch.Generator().manual_seed(seed + sum(ord(c) for c in key))
    return torch.randn(shape, generator=g, dtype=torch.float64)


def count_weights(L, seed, count_smooth):
    """label weights count_smooth / count^0.8 from seeded synthetic counts (the specials <sos> / <eos> counted too)"""
    rs = np.random.RandomState(seed)
    counts = rs.randint(50, 5000, size=L).astype(np.float64)
    w = torch.tensor(count_smooth / counts ** 0.8, dtype=torch.float32)
    w[0] = 1.0                                  # <pad>: never counted; Perplexity zeroes it
    return w


def reference_step(ns, decoder, h0, c0, labels, boxes, weight, K, stepped):
    """one caption through the reference: forward, both losses, backward, optionally one optimizer step"""
    loss_mod = importlib.import_module("seq2seq.loss.loss")
    optim_mod = importlib.import_module("seq2seq.optim.optim")
    n = labels.shape[0] - 1
    H = h0.shape[0]
    hidden = (h0.view(1, 2, H // 2).transpose(0, 1).contiguous(), c0.view(1, 2, H // 2).transpose(0, 1).contiguous())
    tl = torch.as_tensor(labels).long().view(1, -1)
    tb = [torch.as_tensor(boxes[:, i]).float().view(1, -1) for i in range(4)]
    lloss = loss_mod.Perplexity(weight.clone(), 0, 1.0)
    bloss = loss_mod.BBLoss(1, K, 1.0)
    outs, xy, wh, _, _ = decoder(hidden, None, tl, tb[0], tb[1], tb[2], tb[3], is_training=1)
    lloss.reset()
    bloss.reset()
    for step, out in enumerate(outs):
        lloss.eval_batch(out.contiguous().view(1, -1), tl[:, step + 1])
        bloss.eval_batch(xy[step], wh[step], tb[0][:, step + 1], tb[1][:, step + 1], tb[2][:, step + 1],
                         tb[3][:, step + 1], tl[:, step + 1])
    loss = lloss.get_loss() + bloss.get_loss()
    decoder.zero_grad()
    loss.backward()
    trace = torch.stack([torch.cat((outs[t],) + tuple(xy[t]) + tuple(wh[t]), dim=1)[0].detach() for t in range(n)])
    rec = {"labels": np.asarray(labels), "boxes": np.asarray(boxes, dtype=np.float32), "h0": h0, "c0": c0,
           "trace": trace.clone(), "label_sum": float(lloss.acc_loss), "box_sum": float(bloss.acc_loss),
           "n": int(lloss.norm_term), "loss": float(loss),
           "grads": {k: p.grad.detach().clone() for k, p in decoder.named_parameters()}}
    assert int(bloss.norm_term) == rec["n"] == n
    rec["grad_norm"] = float(torch.sqrt(sum((g.double() ** 2).sum() for g in rec["grads"].values())))
    if stepped:
        opt = optim_mod.Optimizer(torch.optim.Adam(decoder.parameters()), max_grad_norm=5)
        opt.step()
        rec["after"] = {k: v.detach().clone() for k, v in decoder.state_dict().items()}
    return rec


def margins(trace, L, K):
    """(label factor from the clamp edge, norm factor above its clamp) of a recorded trace"""
    p = trace[:, :L].double()
    label = float(torch.min(torch.maximum(p / 1e-5, 1e-5 / p)))
    worst = math.inf
    for o in (L, L + 6 * K):
        sa, sb, rho = (trace[:, o + i * K:o + (i + 1) * K].double() for i in (3, 4, 5))
        worst = min(worst, float((2 * math.pi * sa * sb * torch.sqrt(1 - rho ** 2)).min()) / 1e-5)
    return label, worst


def check(rec, L, K):
    label, norm = margins(rec["trace"], L, K)
    # (a probability AT the clamp value reads as factor 1: it is inside the forbidden band as well)
    assert label >= 2 and norm >= 2, (label, norm)
    assert torch.isfinite(rec["trace"]).all() and all(torch.isfinite(g).all() for g in rec["grads"].values())
    rec["label_margin"], rec["norm_margin"] = label, norm


def first_update(params, grads, max_norm=5):
    """clip_grad_norm_ + the first torch.optim.Adam step on fp32 copies -> the updates"""
    ps = [torch.nn.Parameter(p.clone().float()) for p in params.values()]
    for p, k in zip(ps, params):
        p.grad = grads[k].clone().float()
    torch.nn.utils.clip_grad_norm_(ps, max_norm)
    torch.optim.Adam(ps).step()
    return {k: p.detach() - params[k] for k, p in zip(params, ps)}


def small_decoder(ns_or_cls, w2i):
    c = SMALL
    dec = ns_or_cls(w2i, *c["means"], 1, 150, c["H"], c["K"], dropout_p=0.2, bidirectional=True)
    return BO.seeded_fill_(dec, c["seed"], scale=c["scale"])


def make_small(ns):
    c = SMALL
    w2i, _ = BO.label_vocabulary(range(1, c["L"] - 3))
    labels, boxes = TO.make_batch(c["seed"], list(c["lens"]), c["L"])
    g = torch.Generator().manual_seed(c["seed"])
    B = len(c["lens"])
    h0, c0 = torch.randn(B, c["H"], generator=g) * 0.5, torch.randn(B, c["H"], generator=g) * 0.5
    weight = count_weights(c["L"], c["seed"], c["count_smooth"])
    caps = []
    for b, n in enumerate(c["lens"]):
        dec = small_decoder(ns.dec.DecoderRNN, w2i)
        rec = reference_step(ns, dec, h0[b], c0[b], labels[b, :n + 1], boxes[b, :n + 1], weight, c["K"],
                             b in c["stepped"])
        check(rec, c["L"], c["K"])
        assert rec["grad_norm"] > 5.5, rec["grad_norm"]          # the clip is active
        caps.append(rec)
    b = c["unclipped"]
    n = c["lens"][b]
    dec = small_decoder(ns.dec.DecoderRNN, w2i)
    un = reference_step(ns, dec, h0[b], c0[b], labels[b, :n + 1], boxes[b, :n + 1], torch.ones(c["L"]), c["K"], True)
    check(un, c["L"], c["K"])
    assert un["grad_norm"] < 4.5, un["grad_norm"]                # the clip is not
    # Adam's first update is lr * g / (|g| + 1e-8): an element whose gradient is near 1e-8 turns the fp32 rounding of the
    # gradient into an O(1) change of its update.  The captions whose post-step parameters are recorded are those
    # where the reference's own arithmetic does not decide the comparison: the update from the fp32 and from the fp64
    # restatement of the gradient agree to 1e-5 (caption 5 with unit weights, 2e-4, is not such a caption).
    sd = small_decoder(ns.dec.DecoderRNN, w2i).state_dict()
    for rec, wgt in [(caps[i], weight) for i in c["stepped"]] + [(un, torch.ones(c["L"]))]:
        args = (sd, rec["h0"][None], rec["c0"][None], rec["labels"][None], rec["boxes"][None], [rec["n"]], c["means"],
                wgt, 1.0, 1.0, c["K"])
        u64 = first_update(sd, TO.step_ref(*args)["grads"])
        u32 = first_update(sd, TO.step_ref(*args, dtype=torch.float32)["grads"])
        rec["update_conditioning"] = max(TO.rel_l2(u32[k], u64[k]) for k in sd)
        assert rec["update_conditioning"] <= 1e-5, rec["update_conditioning"]
    print("small: clipped norms", [round(r["grad_norm"], 2) for r in caps], "unclipped", round(un["grad_norm"], 3))
    return {"config": dict(c), "weight": weight, "captions": caps, "unclipped": un}


def make_real(ns):
    c = REAL
    rc = BO.load_golden()["real"]["config"]
    L, K, H = rc["L"], rc["K"], rc["H"]
    w2i, _ = BO.label_vocabulary(range(1, L - 3))
    labels, boxes = TO.make_batch(c["seed"], list(c["lens"]), L)
    g = torch.Generator().manual_seed(c["seed"])
    B = len(c["lens"])
    h0, c0 = torch.randn(B, H, generator=g) * 0.3, torch.randn(B, H, generator=g) * 0.3
    weight = count_weights(L, c["seed"], c["count_smooth"])
    caps = []
    for b, n in enumerate(c["lens"]):
        dec = ns.dec.DecoderRNN(w2i, *rc["means"], 1, 150, H, K, dropout_p=0.2, bidirectional=True)
        BO.seeded_fill_(dec, rc["seed_dec"], bias_shift={w2i["<eos>"]: 1.3})
        rec = reference_step(ns, dec, h0[b], c0[b], labels[b, :n + 1], boxes[b, :n + 1], weight, K, False)
        check(rec, L, K)
        grads = rec.pop("grads")
        rec["grad_norms"] = {k: float(v.double().norm()) for k, v in grads.items()}
        rec["grad_dots"] = {k: float((v.double() * direction(k, v.shape, c["direction_seed"])).sum())
                            for k, v in grads.items()}
        caps.append(rec)
    print("real: norms", [round(r["grad_norm"], 1) for r in caps], "label margins",
          [round(r["label_margin"], 1) for r in caps])
    return {"config": dict(c), "weight": weight, "captions": caps}


def write_tiny_train(path, vocab_words, categories, seed, lines):
    rs = np.random.RandomState(seed)
    words = [w for w in vocab_words if w.isalpha()]
    out = []
    for _ in range(lines):
        cap = " ".join(words[i] for i in rs.randint(0, len(words), size=rs.randint(3, 8)))
        n = rs.randint(1, 6)
        labs = [categories[i] for i in rs.randint(0, len(categories), size=n)]
        xs, ys = rs.randint(20, 236, size=n), rs.randint(20, 236, size=n)
        ws = rs.randint(20, 180, size=n)
        rr = np.round(rs.uniform(0.5, 2.0, size=n), 2)
        out.append("\t".join([cap.capitalize() + "."] + [" ".join(str(v) for v in q) for q in (xs, ys, ws, rr, labs)]))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def make_data(ns):
    c = DATA
    t = BO.load_golden()["tiny"]
    w2i_cap, i2w_cap = t["vocabularies"][0], t["vocabularies"][1]
    write_tiny_train(TO.TINY_TRAIN, list(w2i_cap), t["config"]["categories"], c["seed"], c["lines"])
    mean_std = os.path.join(BO.TINY, "mean_std_test.txt")
    dev = os.path.join(BO.TINY, "input_test.txt")
    out = ns.ds.prepare_data(TO.TINY_TRAIN, dev, mean_std, 150, 1, dict(i2w_cap), dict(w2i_cap))
    tc, tl, tuples = out[0], out[1], out[2]
    weight = torch.ones(len(tl.word2index))
    for word in tl.word2index:
        if tl.word2count[word] == 0:
            continue
        weight[tl.word2index[word]] = weight[tl.word2index[word]] * c["count_smooth"] / float(
            math.pow(tl.word2count[word], 0.8))
    rec = {"config": dict(c), "label_word2index": dict(tl.word2index), "label_index2word": dict(tl.index2word),
           "label_word2count": dict(tl.word2count), "cap_word2count": dict(tc.word2count), "n_tuples": len(tuples),
           "dev_label_word2count": dict(out[4].word2count), "weight": weight, "batches": []}
    random.seed(c["seed"])
    for _ in range(c["batches"]):
        b = ns.ds.random_batch(c["batch_size"], tuples, tc, tl, out[6], out[7], out[8], out[9], is_training=1)
        rec["batches"].append([v.clone() if torch.is_tensor(v) else list(v) for v in b])
    return rec


def make_curve():
    """the fp64 restatement trained like `sample.py --is_training 1 --seed S --batch_size 4` on the tiny input"""
    import sample
    from seq2seq.dataset.prepare_dataset import prepare_data, random_batch
    c = CURVE
    t = BO.load_golden()["tiny"]
    w2i_cap, i2w_cap = t["vocabularies"][0], t["vocabularies"][1]
    out = prepare_data(TO.TINY_TRAIN, os.path.join(BO.TINY, "input_test.txt"), os.path.join(BO.TINY, "mean_std_test.txt"),
                       150, 1, dict(i2w_cap), dict(w2i_cap))
    tc, tl, tuples = out[0], out[1], out[2]
    means = tuple(ms[0] for ms in out[6:10])
    H, K = t["config"]["H"], t["config"]["K"]
    dec = sample.new_decoder(tl.word2index, means, c["batch_size"], 150, H, K, c["seed"])
    weight = sample.label_weights(tl, DATA["count_smooth"])
    enc = BO.tiny_encoder().double()
    params = {k: v.detach().double().clone() for k, v in dec.state_dict().items()}
    adam = torch.optim.Adam(list(params.values()))
    rng = random.Random(c["seed"] + 1)
    curve = []
    for _ in range(c["steps"]):
        caps, cap_lens, tlab, _, tx, ty, tw, tr = random_batch(c["batch_size"], tuples, tc, tl, out[6], out[7], out[8],
                                                               out[9], is_training=1, rng=rng, device="cpu")
        h0, c0 = [], []
        with torch.no_grad():
            for b, n in enumerate(cap_lens):
                _, (h, cc) = enc.rnn(enc.encoder(caps[b:b + 1, :n]))
                h0.append(torch.cat((h[0, 0], h[1, 0])))
                c0.append(torch.cat((cc[0, 0], cc[1, 0])))
        lens = [int((tlab[b, 1:] != 0).sum()) for b in range(tlab.shape[0])]
        boxes = torch.stack((tx, ty, tw, tr), dim=2)
        r = TO.step_ref(params, torch.stack(h0), torch.stack(c0), tlab, boxes, lens, means, weight, 1.0, 1.0, K)
        curve.append(r["loss"])
        for k, p in params.items():
            p.grad = r["grads"][k]
        torch.nn.utils.clip_grad_norm_(list(params.values()), 5)
        adam.step()
    first, last = float(np.mean(curve[:10])), float(np.mean(curve[-10:]))
    print("curve: first 10 %.4f last 10 %.4f" % (first, last))
    assert last < first
    return {"config": dict(c), "loss": curve, "first10": first, "last10": last}


def main():
    rec = MG.Recorder()
    ns = MG.load_reference_boxgen(rec)
    with MG.ref_active(ns):
        for name in ("seq2seq.loss.loss", "seq2seq.optim.optim"):
            ns._mods[name] = importlib.import_module(name)
        for name in ("seq2seq.loss", "seq2seq.optim"):
            if name in sys.modules:
                ns._mods[name] = sys.modules[name]
        out = {"small": make_small(ns), "real": make_real(ns), "data": make_data(ns)}
    out["curve"] = make_curve()
    torch.save(out, TO.GOLDEN)
    print("wrote", TO.GOLDEN, os.path.getsize(TO.GOLDEN), "bytes")


if __name__ == "__main__":
    main()

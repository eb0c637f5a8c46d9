"""Box-generator training, test helpers: a from-scratch fp64 torch restatement of the batched training step (teacher-forced
decode, the label and box losses with every quirk of the reference's loss classes, autograd), written from the formulas:

    input_t   = cat(xy_emb(x_t, y_t), wh_emb(w_t, r_t), l_emb[label_t])      (x_0.. = the means, label_0 = <sos>)
    h_t, c_t  = LSTM cell;   p_t = clamp(softmax(l_out h_t), 1e-5, 1)
    xy_t      = mixture(xy_out cat(h_t, onehot(label_{t+1})))
    wh_t      = mixture(wh_out cat(h_t, onehot(label_{t+1}), next_xy_emb(x_{t+1}, y_t)))     (the CURRENT y)
    label_b   = sum_t -w[label_{t+1}] p_t[label_{t+1}]                        (NLLLoss on probabilities, w[<pad>] = 0)
    box_b     = sum_t -[label_{t+1} != 0] (pdf(xy_t; x_{t+1}, y_{t+1}) + pdf(wh_t; w_{t+1}, r_{t+1}))
    pdf       = log(sum_k pi_k exp(a_k - a_max) / max(2 pi s s sqrt(1 - rho^2), 1e-5) + 1e-5) + a_max
    loss      = (lamda1 sum_b label_b + lamda2 sum_b box_b) / sum_b n_b

Needs neither the reference tree nor a GPU."""
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import boxgen_oracle as BO

BOUND = 1e-4                     # the project's operator bound
GOLDEN = os.path.join(BO.GOLDEN, "boxgen_train_ref.pt")
TINY_TRAIN = os.path.join(BO.TINY, "input_train.txt")


@functools.lru_cache(maxsize=None)
def load_golden():
    """tests/golden/boxgen_train_ref.pt (tests/golden/make_golden_boxgen_train.py wrote it); shared, do not modify"""
    return torch.load(GOLDEN, map_location="cpu", weights_only=False)


def mixture(raw, K):
    pi, ua, ub, sa, sb, rho = torch.split(raw, K, dim=-1)
    return torch.softmax(pi, dim=-1), ua, ub, torch.exp(sa), torch.exp(sb), torch.tanh(rho)


def pdf(par, x, y):
    """one mixture's value at (x, y); par: six [K] tensors"""
    pi, ux, uy, sx, sy, rho = par
    z = ((x - ux) / sx) ** 2 + ((y - uy) / sy) ** 2 - 2 * rho * (x - ux) * (y - uy) / (sx * sy)
    a = -z / (2 * (1 - rho ** 2))
    a_max = a.max()                      # the gradient runs through it, as in the reference
    norm = torch.clamp(2 * math.pi * sx * sy * torch.sqrt(1 - rho ** 2), min=1e-5)
    return torch.log((pi * torch.exp(a - a_max) / norm).sum() + 1e-5) + a_max


def step_ref(sd, h0, c0, labels, boxes, lens, first_input, weight, lamda1, lamda2, K, dtype=torch.float64, grad=True,
             dtrace=False, pad=0):
    """sd: decoder state dict; h0, c0 [B, H]; labels [B, T + 1] ints; boxes [B, T + 1, 4]; lens [B]; weight [L].
    -> dict: trace [B, T, L + 12K] (zero past each length), sums [B, 3] (label term, box term, n), loss, matches [B],
    grads {key: tensor} of the batch loss, margins (the smallest distance factors from the two clamps).
    pad: the label whose weight is zero and that n and matches leave out (the box mask stays label != 0).
    dtrace=True (with grad) adds "dtrace" [B, T, L + 12K]: per (b, t) the gradient of the batch loss with respect to the
    UNCLAMPED softmax (zero where the clamp is active) and to the activated mixture parameters; zero past a length."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(grad) for k, v in sd.items()}
    labels = torch.as_tensor(labels).long()
    boxes = torch.as_tensor(boxes).to(dtype)
    weight = torch.as_tensor(weight).to(dtype).clone()
    weight[pad] = 0
    B, T = labels.shape[0], labels.shape[1] - 1
    L = p["l_out.weight"].shape[0]
    rows, lsum, bsum, ns, matches, nodes = [], [], [], [], [], []
    label_margin, norm_margin = math.inf, math.inf
    for b in range(B):
        h, c = h0[b].to(dtype), c0[b].to(dtype)
        lt = bt = 0
        n = m = 0
        caption = []
        for t in range(int(lens[b])):
            x, y, w, r = (torch.tensor(float(v), dtype=dtype) for v in first_input) if t == 0 else boxes[b, t]
            nl = int(labels[b, t + 1])
            inp = torch.cat((F.linear(torch.stack((x, y)), p["xy_embedding.weight"], p["xy_embedding.bias"]),
                             F.linear(torch.stack((w, r)), p["wh_embedding.weight"], p["wh_embedding.bias"]),
                             p["l_embedding.weight"][int(labels[b, t])]))
            gates = F.linear(inp, p["rnn.weight_ih_l0"], p["rnn.bias_ih_l0"]) + \
                F.linear(h, p["rnn.weight_hh_l0"], p["rnn.bias_hh_l0"])
            gi, gf, gg, go = gates.chunk(4)
            c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
            h = torch.sigmoid(go) * torch.tanh(c)
            soft = torch.softmax(F.linear(h, p["l_out.weight"], p["l_out.bias"]), dim=0)
            ps = soft.clamp(1e-5, 1)
            onehot = torch.zeros(L, dtype=dtype)
            onehot[nl] = 1
            xy_hidden = torch.cat((h, onehot))
            xy = mixture(F.linear(xy_hidden, p["xy_out.weight"], p["xy_out.bias"]), K)
            nxy = F.linear(torch.stack((boxes[b, t + 1, 0], y)), p["next_xy_embedding.weight"],
                           p["next_xy_embedding.bias"])
            wh = mixture(F.linear(torch.cat((xy_hidden, nxy)), p["wh_out.weight"], p["wh_out.bias"]), K)
            caption.append(torch.cat((ps,) + xy + wh))
            nodes.append((b, t, (soft,) + xy + wh))
            lt = lt - weight[nl] * ps[nl]
            if nl != 0:
                bt = bt - pdf(xy, boxes[b, t + 1, 0], boxes[b, t + 1, 1]) - pdf(wh, boxes[b, t + 1, 2], boxes[b, t + 1, 3])
            if nl != pad:
                n += 1
                m += int(int(torch.argmax(ps)) == nl)
            with torch.no_grad():
                s = soft.detach()
                label_margin = min(label_margin, float(torch.min(torch.maximum(s / 1e-5, 1e-5 / s))))
                for q in (xy, wh):
                    nrm = 2 * math.pi * q[3] * q[4] * torch.sqrt(1 - q[5] ** 2)
                    norm_margin = min(norm_margin, float(nrm.min()) / 1e-5)
        rows.append(caption)
        lsum.append(lt)
        bsum.append(bt)
        ns.append(n)
        matches.append(m)
    N = sum(ns)
    loss = (lamda1 * sum(lsum) + lamda2 * sum(bsum)) / N
    grads = None
    TR = L + 12 * K
    dtr = None
    if grad:
        flat = [v for _, _, row in nodes for v in row] if dtrace else []
        got = torch.autograd.grad(loss, list(p.values()) + flat, allow_unused=True)
        grads = {k: (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(p.items(), got)}
        if dtrace:
            dtr = torch.zeros((B, T, TR), dtype=dtype)
            got = iter(got[len(p):])
            for b, t, row in nodes:
                dtr[b, t] = torch.cat([torch.zeros_like(v) if g is None else g for v, g in zip(row, got)])
    trace = torch.zeros((B, T, TR), dtype=dtype)
    for b, caption in enumerate(rows):
        for t, row in enumerate(caption):
            trace[b, t] = row.detach()
    val = lambda v: float(v.detach()) if torch.is_tensor(v) else float(v)
    sums = torch.tensor([[val(l), val(x), n] for l, x, n in zip(lsum, bsum, ns)], dtype=torch.float64)
    out = {"trace": trace, "sums": sums, "loss": val(loss), "matches": matches, "grads": grads,
           "label_margin": label_margin, "norm_margin": norm_margin}
    if dtr is not None:
        out["dtrace"] = dtr
    return out


# kernel layout <-> state dict: the order of the 17 tensors of objgan_box_decode and which of them are transposed
KERNEL_KEYS = ("l_embedding.weight", "xy_embedding.weight", "xy_embedding.bias", "wh_embedding.weight",
               "wh_embedding.bias", "next_xy_embedding.weight", "next_xy_embedding.bias", "rnn.weight_ih_l0",
               "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0", "l_out.weight", "l_out.bias", "xy_out.weight",
               "xy_out.bias", "wh_out.weight", "wh_out.bias")
TRANSPOSED = (7, 8, 11, 13, 15)


def to_state_layout(tensors):
    """17 tensors in the kernel's layout -> {state-dict key: tensor in nn layout}"""
    return {k: (t.t() if i in TRANSPOSED else t) for i, (k, t) in enumerate(zip(KERNEL_KEYS, tensors))}


def rel_l2(got, want):
    got, want = got.detach().double().cpu().reshape(-1), want.detach().double().cpu().reshape(-1)
    den = float(want.norm())
    return float((got - want).norm()) / (den if den > 0 else 1.0)


def make_batch(seed, lens, L, x_scale=1.0):
    """random targets for captions of the given step counts: labels [B, T + 1] (<sos>, categories >= 4, <eos> last,
    <pad> after), boxes [B, T + 1, 4] normal values (the <eos> step carries zeros like the reference's padding)"""
    rs = np.random.RandomState(seed)
    B, T = len(lens), max(lens)
    labels = np.zeros((B, T + 1), dtype=np.int64)
    boxes = np.zeros((B, T + 1, 4), dtype=np.float32)
    for b, n in enumerate(lens):
        labels[b, 0] = 1
        labels[b, 1:n] = rs.randint(4, L, size=n - 1)
        labels[b, n] = 2
        boxes[b, 1:n] = rs.standard_normal((n - 1, 4)).astype(np.float32) * x_scale
    return labels, boxes


def stack_captions(caps):
    """the golden's per-caption records as one batch: labels [B, T + 1] int64, boxes [B, T + 1, 4] (zero padded), lens,
    h0, c0 [B, H]"""
    lens = [int(c["n"]) for c in caps]
    B, T = len(caps), max(lens)
    labels = np.zeros((B, T + 1), dtype=np.int64)
    boxes = np.zeros((B, T + 1, 4), dtype=np.float32)
    for b, c in enumerate(caps):
        labels[b, :lens[b] + 1], boxes[b, :lens[b] + 1] = c["labels"], c["boxes"]
    return labels, boxes, lens, torch.stack([c["h0"] for c in caps]), torch.stack([c["c0"] for c in caps])


def small_decoder():
    """the product's decoder at the golden's small shape, weights regenerated by the seeded fill"""
    from seq2seq.models import DecoderRNN
    c = load_golden()["small"]["config"]
    w2i, _ = BO.label_vocabulary(range(1, c["L"] - 3))
    dec = DecoderRNN(w2i, *c["means"], 1, 150, c["H"], c["K"], dropout_p=0.2, bidirectional=True)
    return BO.seeded_fill_(dec, c["seed"], scale=c["scale"])


def direction(key, shape, seed):
    """the seeded direction the golden's gradient projections use (tests/golden/make_golden_boxgen_train.py)"""
    g = torch.Generator().manual_seed(seed + sum(ord(c) for c in key))
    return torch.randn(shape, generator=g, dtype=torch.float64)


def pad_batch(labels, boxes, T):
    """the same targets padded to T steps with values that must not matter"""
    B, T0 = labels.shape[0], labels.shape[1] - 1
    lab = np.zeros((B, T + 1), dtype=labels.dtype)
    box = np.full((B, T + 1, 4), 7.5, dtype=boxes.dtype)
    lab[:, :T0 + 1], box[:, :T0 + 1] = labels, boxes
    return lab, box

"""fp64 restatement of one DAMSM pretraining step, written from the formulas (AttnGAN, Xu et al. 2018, Eq. 7-13; the
packed bidirectional LSTM of torch.nn.LSTM; clip_grad_norm_; Adam).  Plain torch on the CPU: needs neither the reference
tree nor a GPU.  tests/golden/damsm_ref.pt (a run of the unmodified reference, tests/golden/make_golden_damsm.py) pins it.

    embed          embedding lookup (tokens clamped to the table) and dropout with a GIVEN keep-mask
    lstm_bidir     h, c recurrences of both directions over the first len words; zero past each length
    words_loss / sent_loss
    step_ref       losses and gradients of w_loss0 + w_loss1 + s_loss0 + s_loss1
    clip_coef / adam_ref
"""
import math
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "damsm_ref.pt")
GAMMAS = (4.0, 5.0, 10.0)           # cfg.TRAIN.SMOOTH.GAMMA1..3
F64 = torch.float64

LSTM_KEYS = ("rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0",
             "rnn.weight_ih_l0_reverse", "rnn.weight_hh_l0_reverse", "rnn.bias_ih_l0_reverse", "rnn.bias_hh_l0_reverse")
TEXT_KEYS = ("encoder.weight",) + LSTM_KEYS


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    d = float(b.norm())
    return float((a - b).norm()) / d if d > 0 else float((a - b).norm())


def load_golden():
    return torch.load(GOLDEN)


def seeded_text_params(ntoken, I, H, seed, scale=0.3):
    """{state-dict key: fp32 tensor} of an RNN_ENCODER with per-direction hidden size H"""
    g = torch.Generator().manual_seed(seed)
    shapes = {"encoder.weight": (ntoken, I)}
    for suffix in ("", "_reverse"):
        shapes["rnn.weight_ih_l0" + suffix] = (4 * H, I)
        shapes["rnn.weight_hh_l0" + suffix] = (4 * H, H)
        shapes["rnn.bias_ih_l0" + suffix] = (4 * H,)
        shapes["rnn.bias_hh_l0" + suffix] = (4 * H,)
    out = {}
    for k in TEXT_KEYS:
        s = shapes[k]
        fan = s[1] if len(s) > 1 and k != "encoder.weight" else 1
        out[k] = (torch.randn(s, generator=g) * (scale if fan == 1 else 1.0 / math.sqrt(fan))).float()
    return out


def embed(table, captions, keep_mask=None, p=0.0):
    """[B, L] tokens -> [B, L, I]: table rows of the tokens clamped to [0, ntoken - 1]; survivors of the keep-mask
    are scaled by fp32(1 / (1 - p)), the value the kernel is handed"""
    x = table[captions.clamp(0, table.shape[0] - 1)]
    if keep_mask is not None:
        scale = float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))
        x = x * keep_mask.to(x.dtype) * scale
    return x


def lstm_bidir(x, lens, params, max_len):
    """x [B, L, I] -> (words_emb [B, 2H, max_len], sent_emb [B, 2H]); gate order i, f, g, o; lengths clamped to [0, L]"""
    B, L, _ = x.shape
    H = params["rnn.weight_hh_l0"].shape[1]
    words = [[[None] * max_len for _ in range(2)] for _ in range(B)]
    sent = []
    zero = x.new_zeros(H)
    for b in range(B):
        n = max(0, min(int(lens[b]), L))
        last = []
        for d, suffix in enumerate(("", "_reverse")):
            w_ih, w_hh = params["rnn.weight_ih_l0" + suffix], params["rnn.weight_hh_l0" + suffix]
            bias = params["rnn.bias_ih_l0" + suffix] + params["rnn.bias_hh_l0" + suffix]
            h, c = zero, zero
            for s in range(n):
                t = s if d == 0 else n - 1 - s
                g = w_ih @ x[b, t] + w_hh @ h + bias
                i, f, gg, o = torch.sigmoid(g[:H]), torch.sigmoid(g[H:2 * H]), torch.tanh(g[2 * H:3 * H]), torch.sigmoid(g[3 * H:])
                c = f * c + i * gg
                h = o * torch.tanh(c)
                if t < max_len:
                    words[b][d][t] = h
            last.append(h)
        sent.append(torch.cat(last))
    rows = []
    for b in range(B):
        cols = [torch.cat([words[b][d][t] if words[b][d][t] is not None else zero for d in range(2)]) for t in range(max_len)]
        rows.append(torch.stack(cols, dim=1))
    return torch.stack(rows), torch.stack(sent)


def class_mask(class_ids, B):
    if class_ids is None:
        return None
    ids = torch.as_tensor(list(class_ids))[:B]
    m = ids.view(-1, 1) == ids.view(1, -1)
    m.fill_diagonal_(False)
    return m


def cross_entropy(scores, labels):
    return -(torch.log_softmax(scores, dim=1)[torch.arange(scores.shape[0]), labels]).mean()


def words_loss(feats, words, lens, class_ids, gammas=GAMMAS):
    """feats [B, nef, h, w], words [B, nef, L] -> (loss0, loss1, similarities [image, caption])"""
    g1, g2, g3 = gammas
    B, nef = feats.shape[:2]
    ctx = feats.reshape(B, nef, -1)                              # [B, nef, S]
    cols = []
    for i in range(B):
        n = min(int(lens[i]), words.shape[2])
        w = words[i, :, :n]                                      # [nef, n]
        attn = torch.einsum("bds,dl->bsl", ctx, w)               # Eq. 7
        attn = torch.softmax(attn, dim=2)                        # Eq. 8: over the words, per region
        attn = torch.softmax(attn.transpose(1, 2) * g1, dim=2)   # Eq. 9: over the regions, per word
        wc = torch.einsum("bds,bls->bdl", ctx, attn)             # [B, nef, n]
        cos = (wc * w.unsqueeze(0)).sum(1) / (wc.norm(dim=1) * w.norm(dim=0).unsqueeze(0)).clamp(min=1e-8)
        cols.append(torch.log(torch.exp(cos * g2).sum(1)))       # Eq. 10
    sim = torch.stack(cols, dim=1) * g3
    m = class_mask(class_ids, B)
    if m is not None:
        sim = sim.masked_fill(m, -float("inf"))
    labels = torch.arange(B)
    return cross_entropy(sim, labels), cross_entropy(sim.t(), labels), sim


def sent_loss(codes, sent, class_ids, gammas=GAMMAS, eps=1e-8):
    B = codes.shape[0]
    scores = codes @ sent.t() / (codes.norm(dim=1, keepdim=True) * sent.norm(dim=1, keepdim=True).t()).clamp(min=eps)
    scores = scores * gammas[2]
    m = class_mask(class_ids, B)
    if m is not None:
        scores = scores.masked_fill(m, -float("inf"))
    labels = torch.arange(B)
    return cross_entropy(scores, labels), cross_entropy(scores.t(), labels), scores


def encode(params, captions, lens, max_len, keep_mask=None, p=0.0):
    return lstm_bidir(embed(params["encoder.weight"], captions, keep_mask, p), lens, params, max_len)


def step_ref(text_params, captions, lens, max_len, feats, codes, class_ids, keep_mask=None, p=0.0, proj=None,
             gammas=GAMMAS, dtype=F64):
    """One forward + backward.  `feats` / `codes` are the image features [B, nef, h, w] and codes [B, nef] -- or, with
    proj = {"emb_features.weight", "emb_cnn_code.weight", "emb_cnn_code.bias"}, the trunk's regions [B, 768, h, w] and
    pooled code [B, 2048] that the two projections map to them.
    -> {"losses": (w0, w1, s0, s1), "grads": {key: gradient}, "d_feats", "d_codes", "words", "sent"}"""
    tp = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in text_params.items()}
    feats = feats.detach().to(dtype).clone().requires_grad_()
    codes = codes.detach().to(dtype).clone().requires_grad_()
    pp = {}
    f, c = feats, codes
    if proj is not None:
        pp = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in proj.items()}
        f = torch.einsum("oc,bchw->bohw", pp["emb_features.weight"].flatten(1), feats)
        c = codes @ pp["emb_cnn_code.weight"].t() + pp["emb_cnn_code.bias"]
    words, sent = encode(tp, captions, lens, max_len, keep_mask, p)
    w0, w1, _ = words_loss(f, words, lens, class_ids, gammas)
    s0, s1, _ = sent_loss(c, sent, class_ids, gammas)
    (w0 + w1 + s0 + s1).backward()
    grads = {k: v.grad for k, v in tp.items()}
    grads.update({k: v.grad for k, v in pp.items()})
    return {"losses": tuple(float(v.detach()) for v in (w0, w1, s0, s1)), "grads": grads, "d_feats": feats.grad,
            "d_codes": codes.grad, "words": words.detach(), "sent": sent.detach()}


def linear_probe_ref(text_params, captions, lens, max_len, r_words, r_sent, keep_mask=None, p=0.0, dtype=F64):
    """gradients of sum(words * r_words) + sum(sent * r_sent): the kernel's backward for a given (d_out, d_hn)"""
    tp = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in text_params.items()}
    words, sent = encode(tp, captions, lens, max_len, keep_mask, p)
    ((words * r_words.to(dtype)).sum() + (sent * r_sent.to(dtype)).sum()).backward()
    return {"grads": {k: v.grad for k, v in tp.items()}, "words": words.detach(), "sent": sent.detach()}


def clip_coef(grads, max_norm):
    """clip_grad_norm_: -> (the factor the gradients are multiplied by, their global L2 norm)"""
    norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    return min(1.0, max_norm / (norm + 1e-6)), norm


def adam_ref(p, g, m, v, lr, step, betas=(0.5, 0.999), eps=1e-8):
    """torch.optim.Adam's rule in fp64 -> (p, m, v) after step number `step` (1-based)"""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    m = m + (g - m) * (1 - betas[0])
    v = v * betas[1] + (1 - betas[1]) * g * g
    denom = v.sqrt() / math.sqrt(1 - betas[1] ** step) + eps
    return p - lr / (1 - betas[0] ** step) * (m / denom), m, v


def lr_schedule(lr0, epochs):
    """the learning rate in force during each epoch: after an epoch, lr *= 0.98 while lr > lr0 / 10"""
    out, lr = [], lr0
    for _ in range(epochs):
        out.append(lr)
        if lr > lr0 / 10.0:
            lr *= 0.98
    return out

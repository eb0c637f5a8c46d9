"""Box-generator test helpers: the seeded weight fill, and a plain torch / numpy restatement of the sampling path of the
reference's DecoderRNN (forward_step with is_training=0 and the loop around it), one caption at a time on the CPU.

The two draw formulas (`choose_component`, `cholesky_point`) are what tests/golden/make_golden_boxgen.py puts in place
of np.random.choice / np.random.multivariate_normal inside the reference's decoder module, and what csrc/box_decode.hip
computes; nothing else of the reference is replaced there.  Needs neither the reference tree nor a GPU."""
import numpy as np
import torch
import torch.nn.functional as F

LABEL_MARGIN = 1e-2         # log p(top-1) - log p(top-2) of the label softmax, at every step
EDGE_MARGIN = 1e-3          # distance of the uniform from every edge of the cumulative component weights
DECODER_KEYS = ("l_embedding.weight", "l_out.bias", "l_out.weight", "next_xy_embedding.bias",
                "next_xy_embedding.weight", "rnn.bias_hh_l0", "rnn.bias_ih_l0", "rnn.weight_hh_l0", "rnn.weight_ih_l0",
                "wh_embedding.bias", "wh_embedding.weight", "wh_out.bias", "wh_out.weight", "xy_embedding.bias",
                "xy_embedding.weight", "xy_out.bias", "xy_out.weight")


def label_vocabulary(categories):
    """word2index / index2word of the label language: the four specials, then the category ids as strings"""
    words = ["<pad>", "<sos>", "<eos>", "<unk>"] + [str(c) for c in categories]
    return {w: i for i, w in enumerate(words)}, {i: w for i, w in enumerate(words)}


def seeded_fill_(module, seed, scale=0.4, bias_shift=None, scales=None):
    """Per sorted state-dict key uniform(-scale, scale) from ONE torch.Generator (`scales` {key prefix: scale} overrides
    the scale of some modules); bias_shift {label index: value} is added to l_out.bias afterwards (<eos> raised so that
    sequences end at different steps)."""
    g = torch.Generator().manual_seed(seed)
    sd = module.state_dict()
    with torch.no_grad():
        for key in sorted(sd):
            s = next((v for k, v in (scales or {}).items() if key.startswith(k)), scale)
            sd[key].copy_((torch.rand(sd[key].shape, generator=g) * 2 - 1) * s)
        for index, value in (bias_shift or {}).items():
            sd["l_out.bias"][index] += value
    return module


def random_captions(seed, n, ntoken, lo=3, hi=12):
    """n captions of lo..hi random word ids in [1, ntoken)"""
    rs = np.random.RandomState(seed)
    return [rs.randint(1, ntoken, size=rs.randint(lo, hi + 1)).tolist() for _ in range(n)]


# ---- the two draws ---------------------------------------------------------------------------------------------------
def choose_component(p, u):
    """np.random.choice(len(p), p=p) for the uniform u: fp64 running sum divided by its last element, index = number
    of entries <= u (clamped).  -> (index, distance of u from the nearest edge)"""
    cdf = np.cumsum(np.asarray(p, dtype=np.float64))
    cdf /= cdf[-1]
    index = min(int(np.searchsorted(cdf, u, side='right')), len(cdf) - 1)
    return index, float(np.min(np.abs(cdf - u)))


def cholesky_point(mean, cov, z1, z2):
    """a draw from N(mean, cov) (2-d) as mean + chol(cov) @ (z1, z2), in fp64"""
    mean = np.array([float(v) for v in mean], dtype=np.float64)
    c = np.array([[float(v) for v in row] for row in cov], dtype=np.float64)
    l00 = np.sqrt(c[0, 0])
    l10 = c[0, 1] / l00
    l11 = np.sqrt(c[1, 1] - l10 * l10)
    return mean[0] + l00 * z1, mean[1] + (l10 * z1 + l11 * z2)


def _mixture(raw, K):
    pi, ua, ub, sa, sb, rho = torch.split(raw, K, dim=1)
    return torch.softmax(pi, dim=1), ua, ub, torch.exp(sa), torch.exp(sb), torch.tanh(rho)


def _draw(params, u, z1, z2, ft=np.float32):
    pi, ua, ub, sa, sb, rho = (p[0].numpy() for p in params)
    p = np.log(pi) / ft(0.4)
    p = np.exp(p - p.max())
    p = p / p.sum()
    k, edge = choose_component(p, u)
    t = ft(np.sqrt(0.4))
    s1, s2 = ft(sa[k] * t), ft(sb[k] * t)
    cov = [[s1 * s1, (rho[k] * s1) * s2], [(rho[k] * s1) * s2, s2 * s2]]
    a, b = cholesky_point([ua[k], ub[k]], cov, z1, z2)
    return a, b, edge


def decode_ref(sd, h0, c0, noise, first_input, sos, eos, K, dtype=torch.float32):
    """sd: decoder state dict (fp32, CPU); h0, c0 [B, H]; noise [B, T, 6] float64.
    -> labels [B, T] int32, lengths [B] int32, samples [B, T, 4] float64, trace [B, T, L + 12K] float32 (zero past
    each length), label margins [B] and edge margins [B] (the smallest over the caption's steps).
    dtype=torch.float64: the same formulas with no fp32 rounding anywhere (the trace is float64 then)."""
    ft = np.float32 if dtype == torch.float32 else np.float64
    sd = {k: v.detach().to(dtype).cpu() for k, v in sd.items()}
    noise = np.asarray(noise, dtype=np.float64)
    B, T = noise.shape[0], noise.shape[1]
    L = sd["l_out.weight"].shape[0]
    labels = np.zeros((B, T), dtype=np.int32)
    lengths = np.zeros((B,), dtype=np.int32)
    samples = np.zeros((B, T, 4), dtype=np.float64)
    trace = np.zeros((B, T, L + 12 * K), dtype=ft)
    lmargin = np.full((B,), np.inf)
    emargin = np.full((B,), np.inf)
    f32 = lambda *v: torch.tensor([[float(e) for e in v]], dtype=dtype)
    for b in range(B):
        h, c = h0[b:b + 1].to(dtype).cpu(), c0[b:b + 1].to(dtype).cpu()
        x, y, w, r = (np.float32(v) for v in first_input)
        label = sos
        for t in range(T):
            inp = torch.cat((F.linear(f32(x, y), sd["xy_embedding.weight"], sd["xy_embedding.bias"]),
                             F.linear(f32(w, r), sd["wh_embedding.weight"], sd["wh_embedding.bias"]),
                             sd["l_embedding.weight"][label:label + 1]), dim=1)
            gates = F.linear(inp, sd["rnn.weight_ih_l0"], sd["rnn.bias_ih_l0"]) + \
                F.linear(h, sd["rnn.weight_hh_l0"], sd["rnn.bias_hh_l0"])
            gi, gf, gg, go = gates.chunk(4, dim=1)
            c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
            h = torch.sigmoid(go) * torch.tanh(c)
            ps = torch.softmax(F.linear(h, sd["l_out.weight"], sd["l_out.bias"]), dim=1).clamp(1e-5, 1)
            top = torch.topk(ps[0], 2)
            label = int(top.indices[0])
            lmargin[b] = min(lmargin[b], float(torch.log(top.values[0].double()) - torch.log(top.values[1].double())))
            xy_hidden = torch.cat((h, ps), dim=1)
            xy_par = _mixture(F.linear(xy_hidden, sd["xy_out.weight"], sd["xy_out.bias"]), K)
            xs, ys, e1 = _draw(xy_par, *noise[b, t, 0:3], ft=ft)
            nxy = F.linear(f32(ft(xs), y), sd["next_xy_embedding.weight"], sd["next_xy_embedding.bias"])
            wh_par = _mixture(F.linear(torch.cat((xy_hidden, nxy), dim=1), sd["wh_out.weight"], sd["wh_out.bias"]), K)
            ws, hs, e2 = _draw(wh_par, *noise[b, t, 3:6], ft=ft)
            emargin[b] = min(emargin[b], e1, e2)
            labels[b, t] = label
            samples[b, t] = (xs, ys, ws, hs)
            trace[b, t] = torch.cat((ps,) + xy_par + wh_par, dim=1)[0].numpy()
            lengths[b] = t + 1
            x, y, w, r = ft(xs), ft(ys), ft(ws), ft(hs)
            if label == eos:
                break
    return labels, lengths, samples, trace, lmargin, emargin


def margins_ok(lmargin, emargin):
    return (np.asarray(lmargin) >= LABEL_MARGIN) & (np.asarray(emargin) >= EDGE_MARGIN)


def trajectory_error(got, want):
    """largest |got - want| / largest |want| over one caption's trajectory (a [T, n] block)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    den = np.max(np.abs(want))
    return float(np.max(np.abs(got - want)) / (den if den > 0 else 1.0))


def pack_layouts(insanns):
    """the dictionary of load_gen_insanns with its 0/1 map stacks bit-packed (they are most of its bytes)"""
    out = {}
    for key, annos in insanns.items():
        out[key] = {}
        for index, anno in annos.items():
            a = dict(anno)
            for name in ("bbox maps", "bbox fmaps"):
                if a[name] is not None:
                    m = np.asarray(a[name])
                    assert ((m == 0) | (m == 1)).all()
                    a[name] = (m.shape, str(m.dtype), np.packbits(m.astype(np.uint8)))
            out[key][index] = a
    return out


def unpack_maps(packed):
    if packed is None:
        return None
    shape, dtype, bits = packed
    return np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape).astype(dtype)


# ---- the committed golden -------------------------------------------------------------------------------------------
import functools
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = os.path.join(GOLDEN, "boxgen_tiny")


@functools.lru_cache(maxsize=None)
def load_golden():
    """tests/golden/boxgen_ref.pt (tests/golden/make_golden_boxgen.py wrote it); shared, do not modify"""
    return torch.load(os.path.join(GOLDEN, "boxgen_ref.pt"), map_location="cpu", weights_only=False)


def real_modules():
    """the product's encoder and decoder at the golden's real shape, weights regenerated by the seeded fill"""
    from seq2seq.models import PreEncoderRNN, DecoderRNN
    c = load_golden()["real"]["config"]
    w2i, _ = label_vocabulary(range(1, c["L"] - 3))
    encoder = seeded_fill_(PreEncoderRNN(c["ntoken"], nhidden=c["H"]), c["seed_enc"], scale=0.1).eval()
    decoder = DecoderRNN(w2i, *c["means"], 1, 150, c["H"], c["K"], dropout_p=0.2, bidirectional=True)
    seeded_fill_(decoder, c["seed_dec"], bias_shift={w2i["<eos>"]: 1.3}).eval()
    return encoder, decoder, w2i


TINY_ENCODER_SCALE = 0.3     # fill of the tiny input's caption encoder (no encoder weights are stored)


def tiny_encoder():
    """the caption encoder of tests/golden/boxgen_tiny/, regenerated by the seeded fill the golden's generator used"""
    from seq2seq.models import PreEncoderRNN
    t = load_golden()["tiny"]
    enc = PreEncoderRNN(len(t["vocabularies"][0]), nhidden=t["config"]["H"])
    return seeded_fill_(enc, t["config"]["seed_enc"], scale=TINY_ENCODER_SCALE).eval()


def stack_golden(captions, T):
    """the per-caption records as batch arrays: ids [B, Lmax] (zero padded), lens, noise, hn, cn, labels, lengths,
    samples, trace (zero past each length)"""
    B = len(captions)
    Lmax = max(len(c["ids"]) for c in captions)
    ids = torch.zeros((B, Lmax), dtype=torch.int64)
    labels = np.zeros((B, T), dtype=np.int32)
    samples = np.zeros((B, T, 4), dtype=np.float64)
    trace = np.zeros((B, T, captions[0]["trace"].shape[1]), dtype=np.float32)
    for b, c in enumerate(captions):
        n = c["length"]
        ids[b, :len(c["ids"])] = torch.tensor(c["ids"])
        labels[b, :n], samples[b, :n], trace[b, :n] = c["labels"], c["samples"], c["trace"].numpy()
    return {"ids": ids, "lens": [len(c["ids"]) for c in captions],
            "noise": np.stack([c["noise"] for c in captions]), "hn": torch.stack([c["hn"] for c in captions]),
            "cn": torch.stack([c["cn"] for c in captions]), "labels": labels,
            "lengths": np.array([c["length"] for c in captions], dtype=np.int32), "samples": samples, "trace": trace}

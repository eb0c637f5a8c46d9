"""TEST INFRASTRUCTURE: the shape generator's training step restated in plain torch, in the dtype of its inputs (the
tests hand it fp64).  Written from the behaviour: networks as functions of a state dict, the three losses, gradient
clipping, Adam, the EMA copy and the rule that the optimizers start afresh at every epoch.  Also the seeded inputs and
weights of the golden cases (tests/golden/make_golden_shapegen.py stores only what the reference computed from them)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

# (nbf, B, R): S = 64 and the 16x16 recurrent maps are fixed by the architecture
CASES = {"b2r3": (16, 2, 3), "r1": (16, 1, 1), "r10": (16, 1, 10), "wide": (80, 1, 2)}
SEEDS = {"inputs": 302, "G": 311, "INSD": 312, "GLBD": 313}
CLIP = 0.25
SAMPLE = 1024


# ---------------------------------------------------------------------------------------------
# seeded inputs / weights
# ---------------------------------------------------------------------------------------------
def make_inputs(case):
    """-> dict of fp32 CPU tensors: z [B, R, 4 nbf], fwd / bwd [B, R, nbf, 64, 64], fmaps [B, R, 16, 16], real masks
    [B, R, 1, 64, 64] in (0, 1) and their maximum over the boxes [B, 1, 64, 64], num_rois"""
    import synth_batch
    nbf, B, R = CASES[case]
    z, fwd, bwd, fmaps, rois, num = synth_batch.make_shape_inputs(seed=SEEDS["inputs"] + R, B_=B, R=R, nbf=nbf)
    if B == 1:
        num = torch.tensor([R])
    g = torch.Generator().manual_seed(SEEDS["inputs"] + 50 + R)
    real = torch.rand(B, R, 1, 64, 64, generator=g) * 0.98 + 0.01
    return {"z": z, "fwd": fwd, "bwd": bwd, "fmaps": fmaps, "real": real, "real_pooled": real.max(1)[0], "num_rois": num}


def seeded_state_(module, seed):
    """fill a module's parameters deterministically BY KEY (sorted): the reference's modules and the product's share keys
    and shapes.  Weights ~ N(0, 1.5 / fan_in), biases ~ N(0, 0.02)."""
    g = torch.Generator().manual_seed(seed)
    sd = module.state_dict()
    with torch.no_grad():
        for key in sorted(sd.keys()):
            t = sd[key]
            if t.dim() > 1:
                t.copy_(torch.randn(t.shape, generator=g) * (1.5 / t[0].numel()) ** 0.5)
            else:
                t.copy_(0.02 * torch.randn(t.shape, generator=g))
    return module


def sample(t, n=SAMPLE):
    """what the golden keeps of a large tensor: every k-th element of its flattening"""
    f = t.detach().reshape(-1)
    return f[::max(1, f.numel() // n)].clone()


# ---------------------------------------------------------------------------------------------
# networks
# ---------------------------------------------------------------------------------------------
def _inorm(x):
    m = x.mean((2, 3), keepdim=True)
    v = ((x - m) ** 2).mean((2, 3), keepdim=True)
    return (x - m) / torch.sqrt(v + 1e-5)


def _glu(x):
    c = x.shape[1] // 2
    return x[:, :c] * torch.sigmoid(x[:, c:])


def _down(sd, pre, x, k, pad):
    return F.leaky_relu(_inorm(F.conv2d(x, sd[pre + ".0.weight"], None, 2, pad)), 0.2)


def convlstm(x, w, b, reverse=False):
    """x [B, R, Cin, H, W] -> hidden states [B, R, Ch, H, W]; step t in slot t (R - 1 - t when reverse)"""
    B, R = x.shape[0], x.shape[1]
    Ch = w.shape[0] // 4
    h = x.new_zeros((B, Ch) + tuple(x.shape[3:]))
    c = h
    out = [None] * R
    for t in range(R):
        gates = F.conv2d(torch.cat((x[:, t], h), 1), w, b, 1, w.shape[2] // 2)
        i, f, o, g = gates.chunk(4, 1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        out[R - 1 - t if reverse else t] = h
    return torch.stack(out, 1)


def g_forward(sd, z, fwd, bwd, fmaps, r_num=1):
    B, R, nbf, S = fwd.shape[0], fwd.shape[1], fwd.shape[2], fwd.shape[3]
    fm = fmaps.shape[-1]

    def down(m):
        h = _down(sd, "downsample2", _down(sd, "downsample1", m.reshape(B * R, nbf, S, S), 3, 1), 3, 1)
        return h.view(B, R, -1, fm, fm)
    hf = convlstm(down(fwd), sd["fwd_convlstm.Gates.weight"], sd["fwd_convlstm.Gates.bias"])
    hb = convlstm(down(bwd), sd["bwd_convlstm.Gates.weight"], sd["bwd_convlstm.Gates.bias"], reverse=True)
    zz = z.unsqueeze(3).unsqueeze(4).expand(B, R, z.shape[2], fm, fm)
    h = torch.cat((hf, hb, zz), 2).reshape(B * R, -1, fm, fm)
    h = _glu(_inorm(F.conv2d(h, sd["jointConv.0.weight"], None, 1, 1)))
    h = h * fmaps.reshape(B * R, 1, fm, fm)
    for r in range(r_num):
        pre = "residual.%d.block." % r
        y = _glu(_inorm(F.conv2d(h, sd[pre + "0.weight"], None, 1, 1)))
        y = _glu(_inorm(F.conv2d(y, sd[pre + "3.weight"], None, 1, 1)))
        h = F.conv2d(y, sd[pre + "6.weight"], None, 1, 1) + h
    for name in ("upsample1", "upsample2"):
        h = F.interpolate(h, scale_factor=2, mode="nearest")
        h = _glu(_inorm(F.conv2d(h, sd[name + ".1.weight"], None, 1, 1)))
    return torch.sigmoid(F.conv2d(h, sd["img_net.img.0.weight"])).view(B, R, 1, S, S)


def d_probs(sd, x):
    for i in range(1, 5):
        x = _down(sd, "downsample%d" % i, x, 4, 1)
    y = F.conv2d(x, sd["get_logits.outlogits.0.weight"], sd["get_logits.outlogits.0.bias"], 4)
    return torch.sigmoid(y).reshape(-1)


def bce(p, target):
    """mean binary cross entropy against a constant label, the logarithm clamped at -100 like torch's"""
    if target:
        return -torch.clamp(torch.log(p), min=-100.0).mean()
    return -torch.clamp(torch.log(1 - p), min=-100.0).mean()


def first_max(x):
    """maximum over dim 1 whose gradient goes to the FIRST maximal entry"""
    m = x.max(1, keepdim=True)[0]
    is_max = (x == m)
    first = is_max & (is_max.cumsum(1) == 1)
    return (x * first.to(x.dtype)).sum(1)


def ins_d_loss(sdD, real, fake, maps):
    B, R, S = real.shape[0], real.shape[1], real.shape[3]
    ri = torch.cat((real, maps), 2).reshape(B * R, -1, S, S)
    fi = torch.cat((fake.detach(), maps), 2).reshape(B * R, -1, S, S)
    return bce(d_probs(sdD, ri), 1) + bce(d_probs(sdD, fi), 0)


def glb_d_loss(sdD, real_pooled, fake, maps):
    pm = maps.max(1)[0]
    fp = first_max(fake.detach())
    return bce(d_probs(sdD, torch.cat((real_pooled, pm), 1)), 1) + bce(d_probs(sdD, torch.cat((fp, pm), 1)), 0)


def g_loss(sdI, sdG_, fake, maps, ins_lambda=1.0, glb_lambda=1.0):
    B, R, S = fake.shape[0], fake.shape[1], fake.shape[3]
    ins = bce(d_probs(sdI, torch.cat((fake, maps), 2).reshape(B * R, -1, S, S)), 1) * ins_lambda
    glb = bce(d_probs(sdG_, torch.cat((first_max(fake), maps.max(1)[0]), 1)), 1) * glb_lambda
    return ins + glb, ins, glb


# ---------------------------------------------------------------------------------------------
# optimizer side
# ---------------------------------------------------------------------------------------------
def clip_divisor(grads, max_norm=CLIP):
    """-> (what clip_grad_norm_ divides by, the global L2 norm)"""
    norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    return max(1.0, (norm + 1e-6) / max_norm), norm


def adam(p, g, m, v, step, lr, b1=0.5, b2=0.999, eps=1e-8):
    """one torch.optim.Adam update; step counts from 1 -> (p, m, v)"""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1 - b2 ** step) + eps
    return p - (lr / (1 - b1 ** step)) * m / denom, m, v


def ema(avg, p, decay=0.999):
    return avg * decay + p * (1 - decay)


class OracleTrainer(object):
    """the whole step on state dicts, in fp64: `new_epoch` re-creates the three optimizers (zero moments, step 0)"""

    def __init__(self, sdG, sdI, sdL, lrG=2e-4, lrD=2e-4, r_num=1):
        dbl = lambda sd: {k: v.detach().double().clone() for k, v in sd.items()}     # noqa: E731
        self.sd = [dbl(sdG), dbl(sdI), dbl(sdL)]
        self.avg = {k: v.clone() for k, v in self.sd[0].items()}
        self.lr = [lrG, lrD, lrD]
        self.r_num = r_num
        self.new_epoch()

    def new_epoch(self, lr_rate=1.0):
        self.lr_rate = lr_rate
        self.m = [{k: torch.zeros_like(v) for k, v in sd.items()} for sd in self.sd]
        self.v = [{k: torch.zeros_like(v) for k, v in sd.items()} for sd in self.sd]
        self.steps = [0, 0, 0]

    def _leaf(self, i):
        return {k: v.clone().requires_grad_() for k, v in self.sd[i].items()}

    def _update(self, i, grads, divisor=1.0):
        self.steps[i] += 1
        for k in self.sd[i]:
            self.sd[i][k], self.m[i][k], self.v[i][k] = adam(self.sd[i][k], grads[k] / divisor, self.m[i][k], self.v[i][k],
                                                            self.steps[i], self.lr[i] * self.lr_rate)

    def step(self, z, fwd, bwd, fmaps, real, real_pooled):
        z, fwd, bwd, fmaps, real, real_pooled = (t.double() for t in (z, fwd, bwd, fmaps, real, real_pooled))
        out = {}
        G = self._leaf(0)
        fake = g_forward(G, z, fwd, bwd, fmaps, self.r_num)
        out["fake_hmaps"] = fake.detach()
        for i, name in ((1, "INSD"), (2, "GLBD")):
            D = self._leaf(i)
            err = ins_d_loss(D, real, fake, fwd) if i == 1 else glb_d_loss(D, real_pooled, fake, fwd)
            err.backward()
            out["err" + name] = err.detach()
            out["grad" + name] = {k: v.grad for k, v in D.items()}
            self._update(i, out["grad" + name])
        errG, ins, glb = g_loss(self.sd[1], self.sd[2], fake, fwd)
        errG.backward()
        out["errG"], out["insg_loss"], out["glbg_loss"] = errG.detach(), ins.detach(), glb.detach()
        grads = {k: v.grad for k, v in G.items()}
        div, norm = clip_divisor(list(grads.values()))
        out["gradG"], out["divisor"], out["normG"] = grads, div, norm
        self._update(0, grads, div)
        for k in self.avg:
            self.avg[k] = ema(self.avg[k], self.sd[0][k])
        return out


def top2_gap_stats(fake):
    """pooled-mask pixels: (exact ties between the two largest candidates, share of pixels whose two largest lie within
    1e-4, smallest gap) -- the condition under which a flipped argmax cannot carry a comparison"""
    if fake.shape[1] < 2:
        return 0, 0.0, float("inf")
    top = fake.detach().double().topk(2, dim=1)[0]
    gap = (top[:, 0] - top[:, 1]).reshape(-1)
    return int((gap == 0).sum()), float((gap < 1e-4).double().mean()), float(gap.min())


def np_boxmaps(raw, cats, num, R, C, NB=10):
    """numpy restatement of the one-hot box maps: forward, and the forward reversed over all NB slots then cut to R"""
    raw, cats = np.asarray(raw), np.asarray(cats)
    B, S = raw.shape[0], raw.shape[-1]
    full = np.zeros((B, NB, C, S, S), raw.dtype)
    for b in range(B):
        for r in range(int(num[b])):
            full[b, r, int(cats[b, r])] = raw[b, r]
    return full[:, :R].copy(), full[:, ::-1][:, :R].copy()

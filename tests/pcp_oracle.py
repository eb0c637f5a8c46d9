"""TEST INFRASTRUCTURE: the shape generator's perceptual term restated in plain torch, in the dtype of its inputs (the
tests hand it fp64), as a function of a torchvision-style VGG-bn state dict.  Written from the behaviour:
  1. fake_pooled = max over the boxes of the fake masks (gradient to the first maximal box), real_pooled likewise;
     each repeated to 3 channels and normalised (x - mean_c) / std_c;
  2. bilinear resize to 224 x 224 with align_corners=True, then 3x3 convolutions (pad 1), BatchNorm on its running
     statistics, ReLU, 2/2 max pools, x.view(N, -1), Linear-ReLU-Linear-ReLU-Linear (dropout is the identity in eval);
  3. taps: every ReLU output of the features, the two ReLU outputs of the classifier, the raw last Linear;
  4. gpcp = sum over the taps of mean |fake_i - real_i|; the loss term is PCP_LAMBDA * gpcp.
Also the seeded weights of the thin / full test networks and the generator step of tests/shapegen_oracle.py extended by
the term (tests/golden/make_golden_pcp.py stores only what the reference computed from the same seeds)."""
import torch
import torch.nn.functional as F

import shapegen_oracle as so

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
SIDE = 224
EPS = 1e-5
LAMBDA = 10.0
# chosen by tests/golden/make_golden_pcp.py's condition: with the masks of shapegen case b2r3 most seeds leave a ReLU / sign /
# argmax decision of the network within fp32 rounding of its threshold, and one flipped decision moves the mask gradient
# by 1e-3 .. 1e-2 between an fp32 and an fp64 run; this seed leaves none (floor 6e-6)
SEED_VGG = 374

_THIN = [4, 4, 'M', 8, 8, 'M', 8, 8, 8, 8, 'M', 16, 16, 16, 16, 'M', 16, 16, 16, 24, 'M']
# `wide`: 64 channels at 224 x 224 and 112 x 112, so that with two images the 64 -> 64 convolutions and their data gradients
# are above the 1e9 FLOP at which the default arithmetic (fp16x2) really takes a launch; thin behind that
WIDTHS = {"thin": (_THIN, (64, 48, 20)),
          "wide": ([64, 64, 'M', 64, 64, 'M'] + _THIN[6:], (64, 48, 20)),
          "thin512": (_THIN[:-2] + [512, 'M'], (4096, 4096, 1000)),
          "full": ([64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512, 512, 512, 512, 'M'],
                   (4096, 4096, 1000))}
# golden cases: name -> (widths, shapegen_oracle case)
GOLDEN_CASES = {"thin512": ("thin512", "b2r3")}


def empty_state(name):
    """zero tensors under torchvision's vgg19_bn keys for the widths `name`"""
    feats, cls = WIDTHS[name]
    sd, idx, cin = {}, 0, 3
    for v in feats:
        if v == 'M':
            idx += 1
            continue
        sd["features.%d.weight" % idx] = torch.zeros(v, cin, 3, 3)
        sd["features.%d.bias" % idx] = torch.zeros(v)
        for s in ("weight", "bias", "running_mean", "running_var"):
            sd["features.%d.%s" % (idx + 1, s)] = torch.zeros(v)
        sd["features.%d.num_batches_tracked" % (idx + 1)] = torch.zeros((), dtype=torch.long)
        idx, cin = idx + 3, v
    side = SIDE >> sum(1 for v in feats if v == 'M')
    width = cin * side * side
    for j, out in zip((0, 3, 6), cls):
        sd["classifier.%d.weight" % j] = torch.zeros(out, width)
        sd["classifier.%d.bias" % j] = torch.zeros(out)
        width = out
    return sd


def seeded_vgg_state_(sd, seed=SEED_VGG):
    """fill a VGG-bn state dict deterministically BY KEY (sorted): weights ~ N(0, 2 / fan_in), running variances
    0.5 + U(0, 1), running means 0.1 N(0, 1), BatchNorm scales 1 + 0.1 N(0, 1), every bias 0.02 N(0, 1);
    num_batches_tracked is left alone"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for key in sorted(sd.keys()):
            t = sd[key]
            if key.endswith("num_batches_tracked"):
                continue
            if t.dim() > 1:
                t.copy_(torch.randn(t.shape, generator=g) * (2.0 / t[0].numel()) ** 0.5)
            elif key.endswith("running_var"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
            elif key.endswith("running_mean"):
                t.copy_(0.1 * torch.randn(t.shape, generator=g))
            elif key.endswith("weight"):
                t.copy_(1.0 + 0.1 * torch.randn(t.shape, generator=g))
            else:
                t.copy_(0.02 * torch.randn(t.shape, generator=g))
    return sd


def seeded_vgg(name, seed=SEED_VGG):
    return seeded_vgg_state_(empty_state(name), seed)


# ---------------------------------------------------------------------------------------------
# the network and the term
# ---------------------------------------------------------------------------------------------
def normalise(pooled):
    """[B, 1, S, S] -> [B, 3, S, S]"""
    x = pooled.repeat(1, 3, 1, 1)
    mean = torch.tensor(MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=x.dtype).view(1, 3, 1, 1)
    return (x - mean) / std


def _layout(sd):
    convs = sorted(int(k.split(".")[1]) for k, v in sd.items() if k.startswith("features.") and k.endswith(".weight") and v.dim() == 4)
    fcs = sorted(int(k.split(".")[1]) for k, v in sd.items() if k.startswith("classifier.") and k.endswith(".weight"))
    return convs, fcs


def vgg_features(sd, x):
    """x: normalised [N, 3, h, w] -> the 19 taps (unfolded BatchNorm on running statistics)"""
    sd = {k: (v.to(x.dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    convs, fcs = _layout(sd)
    x = F.interpolate(x, size=(SIDE, SIDE), mode="bilinear", align_corners=True)
    taps = []
    for pos, i in enumerate(convs):
        x = F.conv2d(x, sd["features.%d.weight" % i], sd["features.%d.bias" % i], 1, 1)
        p = "features.%d." % (i + 1)
        x = (x - sd[p + "running_mean"].view(1, -1, 1, 1)) / torch.sqrt(sd[p + "running_var"].view(1, -1, 1, 1) + EPS)
        x = torch.relu(x * sd[p + "weight"].view(1, -1, 1, 1) + sd[p + "bias"].view(1, -1, 1, 1))
        taps.append(x)
        pools = (convs[pos + 1] - i - 3) if pos + 1 < len(convs) else None
        if pools is None:
            fc_in = sd["classifier.%d.weight" % fcs[0]].shape[1]
            while x.shape[1] * x.shape[2] * x.shape[3] != fc_in:
                x = F.max_pool2d(x, 2, 2)
        else:
            for _ in range(pools):
                x = F.max_pool2d(x, 2, 2)
    x = x.reshape(x.shape[0], -1)
    for pos, j in enumerate(fcs):
        x = F.linear(x, sd["classifier.%d.weight" % j], sd["classifier.%d.bias" % j])
        if pos + 1 < len(fcs):
            x = torch.relu(x)
        taps.append(x)
    return taps


def perceptual(sd, fake_pooled, real_pooled):
    """-> the per-tap means of |fake_i - real_i| as one tensor [19]"""
    ff = vgg_features(sd, normalise(fake_pooled))
    rf = vgg_features(sd, normalise(real_pooled))
    return torch.stack([(f - r).abs().mean() for f, r in zip(ff, rf)])


def g_loss_pcp(sdI, sdL, sdV, real, fake, maps, lam=LAMBDA):
    """-> (errG_total, insg, glbg, gpcp (weighted), per-tap means)"""
    base, ins, glb = so.g_loss(sdI, sdL, fake, maps)
    taps = perceptual(sdV, so.first_max(fake), real.max(1)[0])
    gpcp = taps.sum() * lam
    return base + gpcp, ins, glb, gpcp, taps


def oracle_step(sdG, sdI, sdL, sdV, x, lam=LAMBDA, dtype=torch.float64):
    """The generator step of the training iteration with the term, in `dtype`: both discriminators take their Adam step
    first (the generator's loss runs through the UPDATED discriminators), then errG, its gradient w.r.t. the fake masks
    and the generator's weights, and the clip."""
    tr = so.OracleTrainer(sdG, sdI, sdL)
    cast = lambda t: t.to(dtype)                                       # noqa: E731
    if dtype != torch.float64:
        tr.sd = [{k: cast(v) for k, v in sd.items()} for sd in tr.sd]
        tr.new_epoch()
    z, fwd, bwd, fmaps, real, real_pooled = (cast(x[k]) for k in ("z", "fwd", "bwd", "fmaps", "real", "real_pooled"))
    G = tr._leaf(0)
    fake = so.g_forward(G, z, fwd, bwd, fmaps, tr.r_num)
    fake.retain_grad()
    for i in (1, 2):
        D = tr._leaf(i)
        err = so.ins_d_loss(D, real, fake, fwd) if i == 1 else so.glb_d_loss(D, real_pooled, fake, fwd)
        err.backward()
        tr._update(i, {k: v.grad for k, v in D.items()})
    sdVc = {k: (cast(v) if v.is_floating_point() else v) for k, v in sdV.items()}
    errG, ins, glb, gpcp, taps = g_loss_pcp(tr.sd[1], tr.sd[2], sdVc, real, fake, fwd, lam)
    errG.backward()
    grads = {k: v.grad for k, v in G.items()}
    div, norm = so.clip_divisor(list(grads.values()))
    return {"errG": errG.detach(), "insg_loss": ins.detach(), "glbg_loss": glb.detach(), "gpcp_loss": gpcp.detach(),
            "pcp_score": taps.detach().sum(), "taps": taps.detach(), "dfake": fake.grad.detach(), "gradG": grads,
            "divisor": div, "normG": norm, "fake_hmaps": fake.detach()}

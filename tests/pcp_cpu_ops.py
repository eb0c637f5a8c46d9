"""TEST INFRASTRUCTURE: CPU definitions of the perceptual term's operators (`pcp_stem_forward`, `perceptual_taps`) on top
of tests/shapegen_cpu_ops.py, so that the host side of the feature -- model.VGG with its folded banks,
miscc/shape_losses.generator_loss, shape_trainer with the score file -- runs on CPU tensors.  The product never imports
this module."""
import torch
import torch.nn.functional as F

import shapegen_cpu_ops

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def pcp_stem_forward(x, oh=224, ow=None):
    y = F.interpolate(x, size=(oh, oh if ow is None else ow), mode="bilinear", align_corners=True).repeat(1, 3, 1, 1)
    return (y - torch.tensor(MEAN, dtype=x.dtype).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=x.dtype).view(1, 3, 1, 1)


def perceptual_taps(fake_pooled, real_pooled, layers):
    """definition: the folded layers on [fake; real], autograd does the rest (real is detached)"""
    B = fake_pooled.shape[0]
    x = pcp_stem_forward(torch.cat((fake_pooled, real_pooled.detach()), 0))
    means = []
    for layer in layers:
        if layer[0] == "pool":
            x = F.max_pool2d(x, 2, 2)
            continue
        if layer[0] == "conv":
            x = torch.relu(F.conv2d(x, layer[1], layer[2], 1, 1))
        else:
            x = F.conv2d(x.reshape(x.shape[0], -1, 1, 1), layer[1], layer[2])
            x = torch.relu(x) if layer[3] else x
        means.append((x[:B] - x[B:].detach()).abs().mean())
    return torch.stack(means)


def install(monkeypatch):
    shim = shapegen_cpu_ops.install(monkeypatch)
    for f in (pcp_stem_forward, perceptual_taps):
        setattr(shim, f.__name__, f)
    return shim

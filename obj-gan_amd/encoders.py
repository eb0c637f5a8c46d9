"""Frozen encoders around the hot path: Inception-v3 image encoder (DAMSM) and IS monitor.

SURVEY.md section 8f, rank 1 ("next" row): these networks are frozen (`requires_grad=False`, eval
mode) feature extractors that the reference takes from torchvision with ImageNet weights
(reference image_generation/model.py:182-315).  Neither torchvision nor the weights exist in this
environment, so the Inception-v3 trunk is restated here with the torchvision module names (a real
`inception_v3_google-*.pth` state dict, `AuxLogits.*` included, loads with strict=True).  Every
operator runs on the objgan_hip kernels: the convolutions (1x1, 3x3, 5x5, 1x7, 7x1, 1x3, 3x1; BatchNorm
folded, ReLU in the epilogue -- first measurements showed MIOpen falling back to `naive_conv_*`
kernels for this network, 43 % of all GPU time of a training step), the max / average pooling layers,
the 299x299 bilinear resize, the linear heads and the softmax; torch only concatenates.  There is no
CPU path here: the plain-PyTorch twin the parity tests compare against lives in
oracle/torch_encoders.py and exchanges weights with these modules through the state dict.  The bench
and the parity tests use seeded random weights (no checkpoint can be shipped or downloaded).
"""
import types

import torch
import torch.nn as nn

from objgan_hip import ops


class BasicConv2d(nn.Module):
    """conv (no bias) -> BatchNorm(eps 1e-3, eval) -> ReLU.

    The frozen eval-mode BatchNorm is folded into the filter bank once
    (w' = w * gamma / sqrt(var + eps), b' = beta - mean * gamma / sqrt(var + eps)) and the block is
    ONE launch of the MFMA implicit-GEMM kernel with a bias + ReLU epilogue."""

    def __init__(self, cin, cout, **kw):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, bias=False, **kw)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)
        self._folded = None

    def _fold(self):
        key = (self.conv.weight.device, self.conv.weight._version, self.bn.weight._version,
               self.bn.running_var._version, self.conv.weight.data_ptr())
        if self._folded is None or self._folded[2] != key:
            with torch.no_grad():
                scale = self.bn.weight / torch.sqrt(self.bn.running_var + self.bn.eps)
                w = (self.conv.weight * scale.view(-1, 1, 1, 1)).contiguous()
                b = (self.bn.bias - self.bn.running_mean * scale).contiguous()
            self._folded = (w, b, key)
        return self._folded[:2]

    def forward(self, x):
        if self.training or self.conv.weight.requires_grad:
            raise RuntimeError("the Inception encoder is a frozen eval-mode network")
        w, b = self._fold()
        return ops.conv2d_frozen(x, w, b, self.conv.stride[0], self.conv.padding, act="relu")


def _chain(cin, spec):
    """spec: list of (cout, kernel, stride, padding) -> nn.ModuleList of BasicConv2d."""
    mods = []
    for cout, k, s, p in spec:
        mods.append(BasicConv2d(cin, cout, kernel_size=k, stride=s, padding=p))
        cin = cout
    return mods


class InceptionA(nn.Module):
    def __init__(self, cin, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch5x5_1, self.branch5x5_2 = _chain(cin, [(48, 1, 1, 0), (64, 5, 1, 2)])
        self.branch3x3dbl_1, self.branch3x3dbl_2, self.branch3x3dbl_3 = _chain(
            cin, [(64, 1, 1, 0), (96, 3, 1, 1), (96, 3, 1, 1)])
        self.branch_pool = BasicConv2d(cin, pool_features, kernel_size=1)

    def forward(self, x):
        return torch.cat([
            self.branch1x1(x),
            self.branch5x5_2(self.branch5x5_1(x)),
            self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))),
            self.branch_pool(ops.avg_pool2d(x, 3, 1, 1)),
        ], 1)


class InceptionB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1, self.branch3x3dbl_2, self.branch3x3dbl_3 = _chain(
            cin, [(64, 1, 1, 0), (96, 3, 1, 1), (96, 3, 2, 0)])

    def forward(self, x):
        return torch.cat([
            self.branch3x3(x),
            self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))),
            ops.max_pool2d(x, 3, 2),
        ], 1)


class InceptionC(nn.Module):
    def __init__(self, cin, channels_7x7):
        super().__init__()
        c7 = channels_7x7
        self.branch1x1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7_1, self.branch7x7_2, self.branch7x7_3 = _chain(
            cin, [(c7, 1, 1, 0), (c7, (1, 7), 1, (0, 3)), (192, (7, 1), 1, (3, 0))])
        (self.branch7x7dbl_1, self.branch7x7dbl_2, self.branch7x7dbl_3, self.branch7x7dbl_4,
         self.branch7x7dbl_5) = _chain(cin, [(c7, 1, 1, 0), (c7, (7, 1), 1, (3, 0)),
                                             (c7, (1, 7), 1, (0, 3)), (c7, (7, 1), 1, (3, 0)),
                                             (192, (1, 7), 1, (0, 3))])
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        bd = x
        for m in (self.branch7x7dbl_1, self.branch7x7dbl_2, self.branch7x7dbl_3, self.branch7x7dbl_4,
                  self.branch7x7dbl_5):
            bd = m(bd)
        return torch.cat([self.branch1x1(x), b7, bd,
                          self.branch_pool(ops.avg_pool2d(x, 3, 1, 1))], 1)


class InceptionD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1, self.branch3x3_2 = _chain(cin, [(192, 1, 1, 0), (320, 3, 2, 0)])
        (self.branch7x7x3_1, self.branch7x7x3_2, self.branch7x7x3_3, self.branch7x7x3_4) = _chain(
            cin, [(192, 1, 1, 0), (192, (1, 7), 1, (0, 3)), (192, (7, 1), 1, (3, 0)), (192, 3, 2, 0)])

    def forward(self, x):
        b7 = x
        for m in (self.branch7x7x3_1, self.branch7x7x3_2, self.branch7x7x3_3, self.branch7x7x3_4):
            b7 = m(b7)
        return torch.cat([self.branch3x3_2(self.branch3x3_1(x)), b7,
                          ops.max_pool2d(x, 3, 2)], 1)


class InceptionE(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(cin, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        b3 = self.branch3x3_1(x)
        b3 = torch.cat([self.branch3x3_2a(b3), self.branch3x3_2b(b3)], 1)
        bd = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        bd = torch.cat([self.branch3x3dbl_3a(bd), self.branch3x3dbl_3b(bd)], 1)
        return torch.cat([self.branch1x1(x), b3, bd,
                          self.branch_pool(ops.avg_pool2d(x, 3, 1, 1))], 1)


class InceptionAux(nn.Module):
    """Parameter holder for torchvision's auxiliary head (`AuxLogits.*` keys of the ImageNet
    checkpoint): never executed -- the reference only runs the network in eval mode."""

    def __init__(self, cin, num_classes):
        super().__init__()
        self.conv0 = BasicConv2d(cin, 128, kernel_size=1)
        self.conv1 = BasicConv2d(128, 768, kernel_size=5)
        self.fc = nn.Linear(768, num_classes)


class Inception3(nn.Module):
    """Inception-v3 with torchvision's module names and state-dict keys."""

    def __init__(self, num_classes=1000):
        super().__init__()
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, 32)
        self.Mixed_5c = InceptionA(256, 64)
        self.Mixed_5d = InceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, 128)
        self.Mixed_6c = InceptionC(768, 160)
        self.Mixed_6d = InceptionC(768, 160)
        self.Mixed_6e = InceptionC(768, 192)
        self.AuxLogits = InceptionAux(768, num_classes)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280)
        self.Mixed_7c = InceptionE(2048)
        self.fc = nn.Linear(2048, num_classes)

    def trunk(self, x, want_regions=False):
        return inception_trunk(self, x, want_regions)

    def forward(self, x):
        return ops.linear(self.trunk(x), self.fc.weight.detach(), self.fc.bias.detach())


TRUNK_MODULES = ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "Conv2d_3b_1x1", "Conv2d_4a_3x3",
                 "Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d",
                 "Mixed_6e", "Mixed_7a", "Mixed_7b", "Mixed_7c")


def inception_trunk(m, x, want_regions=False):
    """299x299 image -> (17x17x768 region features, 2048-d pooled code); `m` is any module that
    owns the trunk blocks under their torchvision names."""
    x = m.Conv2d_2b_3x3(m.Conv2d_2a_3x3(m.Conv2d_1a_3x3(x)))
    x = ops.max_pool2d(x, 3, 2)
    x = m.Conv2d_4a_3x3(m.Conv2d_3b_1x1(x))
    x = ops.max_pool2d(x, 3, 2)
    x = m.Mixed_5d(m.Mixed_5c(m.Mixed_5b(x)))
    x = m.Mixed_6e(m.Mixed_6d(m.Mixed_6c(m.Mixed_6b(m.Mixed_6a(x)))))
    regions = x                                     # 768 x 17 x 17
    x = m.Mixed_7c(m.Mixed_7b(m.Mixed_7a(x)))
    x = ops.avg_pool2d(x, 8).flatten(1)             # 2048
    return (regions, x) if want_regions else x


def inception_v3(**kw):
    return Inception3(**kw)


def seeded_init_(module, seed):
    """Deterministic random weights (He-style scale so activations stay O(1)); identical on every
    machine, so the oracle and the product path share the same frozen encoder without shipping
    a checkpoint."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in sorted(module.named_parameters()):
            if name.startswith("AuxLogits.") or ".AuxLogits." in name:
                p.zero_()                   # never-executed holder: kept out of the random stream
                continue
            if p.dim() > 1:
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / fan_in) ** 0.5)
            elif name.endswith("weight"):
                p.fill_(1.0)
            else:
                p.zero_()
    return module


class CNN_ENCODER(nn.Module):
    """Image encoder of the DAMSM loss (reference model.py:182-287): frozen Inception-v3 trunk +
    two projections (`emb_features` 1x1 conv 768 -> nef, `emb_cnn_code` Linear 2048 -> nef)."""

    def __init__(self, nef, trunk=None):
        super().__init__()
        self.nef = nef
        net = trunk if trunk is not None else inception_v3()
        for p in net.parameters():
            p.requires_grad = False
        for name in TRUNK_MODULES:          # same attribute / state-dict names as the reference
            setattr(self, name, getattr(net, name))
        self.emb_features = nn.Conv2d(768, nef, kernel_size=1, stride=1, padding=0, bias=False)
        self.emb_cnn_code = nn.Linear(2048, nef)
        self.emb_features.weight.data.uniform_(-0.1, 0.1)
        self.emb_cnn_code.weight.data.uniform_(-0.1, 0.1)
        # Set by the DAMSM pretraining loop (damsm_trainer.py).  requires_grad alone cannot be the switch: a freshly
        # built encoder has it on, and the generator's DAMSM term differentiates such an encoder down to the image.
        self.train_projections = False

    def forward(self, x):
        x = ops.bilinear_resize(x, 299, 299)
        if self.train_projections and self.emb_features.weight.requires_grad:
            # DAMSM pretraining: the two projections learn; the trunk stays frozen and the image is data (no gradient)
            with torch.no_grad():
                regions, code = inception_trunk(self, x, want_regions=True)
            return (ops.conv2d(regions, self.emb_features.weight),
                    ops.linear(code, self.emb_cnn_code.weight, self.emb_cnn_code.bias))
        regions, code = inception_trunk(self, x, want_regions=True)
        return (ops.conv2d_frozen(regions, self.emb_features.weight.detach()),
                ops.linear(code, self.emb_cnn_code.weight.detach(), self.emb_cnn_code.bias.detach()))


class INCEPTION_V3(nn.Module):
    """Per-step Inception-score monitor (reference model.py:290-315)."""

    def __init__(self, net=None):
        super().__init__()
        self.model = net if net is not None else inception_v3()
        for p in self.model.parameters():
            p.requires_grad = False
        # not part of the reference's state dict: non-persistent
        self.register_buffer("mean", torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), persistent=False)
        self.register_buffer("std", torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1), persistent=False)

    def forward(self, input):
        x = (input * 0.5 + 0.5 - self.mean) / self.std
        x = ops.bilinear_resize(x, 299, 299)
        return ops.softmax_strided(self.model(x), 1)


# The four stages of the FID network: `blocks.{0..3}.{position}` in the reference's state dict (its pooling layers sit
# behind the convolutions of a stage and own no parameters, so the keys agree).
FID_BLOCKS = (TRUNK_MODULES[0:3], TRUNK_MODULES[3:5], TRUNK_MODULES[5:13], TRUNK_MODULES[13:16])


class INCEPTION_V3_FID(nn.Module):
    """FID feature network (reference model.py:318-451): the Inception-v3 trunk held as `blocks.{0..3}.*`, fed with
    the half-pixel bilinear 299 x 299 resize and the reference's re-normalisation, returning the pooled 2048-d
    activations as `[pool3]` of shape [B, 2048, 1, 1].  Resize and affine are one launch
    (`ops.bilinear_resize_halfpixel` with the two affines of the reference forward folded per channel).  Only output
    block 3 runs here; the shallower feature maps (64 / 192 / 768-d) are refused."""

    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}

    def __init__(self, output_blocks=(DEFAULT_BLOCK_INDEX,), resize_input=True, trunk=None):
        super().__init__()
        self.resize_input = resize_input
        self.output_blocks = sorted(output_blocks)
        self.last_needed_block = max(output_blocks)
        if self.output_blocks != [3]:
            dims = {v: k for k, v in self.BLOCK_INDEX_BY_DIM.items()}
            raise NotImplementedError(
                "INCEPTION_V3_FID: only output block 3 (2048-d pooled features, cfg.TEST.FID_DIMS = 2048) is "
                "implemented, got blocks %s (%s-d)" % (self.output_blocks, [dims.get(b, "?") for b in self.output_blocks]))
        net = trunk if trunk is not None else self._load_pretrained()
        for p in net.parameters():
            p.requires_grad = False
        self.blocks = nn.ModuleList()
        for names in FID_BLOCKS:
            self.blocks.append(nn.Sequential(*[getattr(net, n) for n in names]))
        # the same modules under their torchvision names, for `inception_trunk`; not a Module, so no second key set
        self.trunk = types.SimpleNamespace(**{n: getattr(net, n) for n in TRUNK_MODULES})
        # (x * 0.5 + 0.5) * a + b with a = std / 0.5, b = (mean - 0.5) / 0.5  ==  x * (0.5 a) + (0.5 a + b)
        a = torch.tensor([0.229, 0.224, 0.225]) / 0.5
        b = (torch.tensor([0.485, 0.456, 0.406]) - 0.5) / 0.5
        self.register_buffer("in_scale", 0.5 * a, persistent=False)
        self.register_buffer("in_shift", 0.5 * a + b, persistent=False)

    @staticmethod
    def _load_pretrained():
        """The torchvision ImageNet state dict next to the DAMSM encoders, like the reference (model.py:367-370)."""
        from miscc.config import cfg
        net = inception_v3()
        path = cfg.TRAIN.NET_E.replace('text_encoder100.pth', 'inception_v3_google-1a9a5a14.pth')
        net.load_state_dict(torch.load(path, map_location="cpu"))
        return net

    def forward(self, inp):
        x = inp
        if self.resize_input:
            x = ops.bilinear_resize_halfpixel(x, 299, 299, self.in_scale, self.in_shift)
        else:
            x = x * self.in_scale.view(1, 3, 1, 1) + self.in_shift.view(1, 3, 1, 1)
        pool3 = inception_trunk(self.trunk, x)
        return [pool3.view(pool3.size(0), -1, 1, 1)]

"""Host restatement (TEST INFRASTRUCTURE ONLY) of the shape generator's pictures: what reference
shape_generation/miscc/utils.py:59-300 (build_super_images / build_super_images2) computes below the caption strip, and
the mask dump of shape_generation/trainer.py:389-397, in numpy / PIL.  tests/golden/make_golden_shape_snapshot.py runs
the unmodified reference functions on the cases below; tests/test_shape_snapshot_cpu.py pins this file to those
results byte for byte.

Masks are drawn at their own size, so everything is float32 like the reference's numpy arrays.  Defined here because
the reference leaves it undefined: a panel or mask with max == min divides 0 by 0 and casts NaN to uint8 -- it is 0
(on the machine the golden was recorded on the reference gives 0 as well); raw values outside [0, 1] saturate."""
import numpy as np
import torch

import snapshot_helpers as SH

FONT_MAX, FONT_SIZE = 20, 12


def _u8(x):
    """np.uint8 of values in [0, 255] (truncation), saturating outside and 0 for NaN"""
    x = np.asarray(x, np.float32)
    return np.where(x >= 0, np.minimum(x, np.float32(255)), np.float32(0)).astype(np.uint8)


def panel_bytes(m, form):
    """one float32 [a, a] map -> uint8 [a, a]: 'norm' (v - min) / (max - min) * 255, 'raw' v * 255"""
    m = np.asarray(m, np.float32)
    if form == "raw":
        return _u8(m * np.float32(255))
    mn, mx = m.min(), m.max()
    if mx == mn:
        return np.zeros(m.shape, np.uint8)
    t = (m - mn) / (mx - mn)
    return _u8(t * np.float32(255))


def grid(imgs, maps, strip, form, max_word_num=10, font_max=FONT_MAX, nvis=None):
    """-> uint8 [nvis * (font_max + 2 s), (max_word_num + 2) * (s + 2), 3]; imgs [B, 3, s, s] in [-1, 1], maps [B, R, (1,) s, s]
    float32, strip uint8 [>= nvis * font_max, width, 3] copied into the caption rows; form 'norm' | 'raw'"""
    B, s = int(imgs.shape[0]), int(imgs.shape[2])
    nvis = min(8, B) if nvis is None else nvis
    hi = SH._image_panels(imgs[:nvis], s)
    pad = np.zeros([s, 2, 3], np.uint8)
    blank = np.zeros([s, s, 3], np.uint8)
    blocks = []
    for i in range(nvis):
        m = maps[i].detach().cpu().float().reshape(-1, s, s)
        m = torch.cat([m.max(dim=0, keepdim=True)[0], m], 0).numpy()
        img = np.uint8(hi[i])
        line, merged = [img, pad], [img, pad]
        for j in range(max_word_num + 1):
            if j < m.shape[0]:
                att = np.repeat(panel_bytes(m[j], form)[:, :, None], 3, 2)
                line += [att, pad]
                merged += [SH._merged(hi[i], att), pad]
            else:
                line += [blank, pad]
                merged += [blank, pad]
        blocks.append(np.concatenate([strip[i * font_max:(i + 1) * font_max], np.concatenate(line, 1),
                                      np.concatenate(merged, 1)], 0))
    return np.concatenate(blocks, 0).astype(np.uint8)


def below_strip(g, nvis, s, font_max=FONT_MAX):
    """the rows of a grid that no caption text reaches"""
    rows = np.ones(g.shape[0], bool)
    for n in range(nvis):
        y0 = n * (font_max + 2 * s)
        rows[y0:y0 + font_max] = False
    return g[rows]


def mask_rgb(planes):
    """float32 [N, h, w] -> uint8 [N, h, w, 3], plane by plane (v - min) / (max - min) * 255"""
    planes = np.asarray(planes, np.float32)
    return np.stack([np.repeat(panel_bytes(p, "norm")[:, :, None], 3, 2) for p in planes])


# ---- the fixed-seed cases, shared by the golden generator and the tests -----------------------------------------------
GRID_CASES = {"s8r3": (8, 8, 3), "s16r3": (8, 16, 3), "s8r10": (8, 8, 10), "s8r1": (8, 8, 1)}    # name -> (B, S, R)


def grid_case(name, B=None):
    """imgs [B, 3, S, S] in (-1, 1), maps [B, R, S, S] in [0, 1): from R = 3 on two all-zero slots (the last of images 1 and
    2) and one constant 0.25 panel; at R = 1 one all-zero image (panel 0, the maximum, is zero as well)"""
    B0, S, R = GRID_CASES[name]
    B = B0 if B is None else B
    g = torch.Generator().manual_seed(700 + 10 * S + R)
    imgs = torch.tanh(torch.randn(B0, 3, S, S, generator=g))
    maps = torch.rand(B0, R, S, S, generator=g)
    if R >= 3:
        maps[1, 2] = 0.0
        maps[2, 2] = 0.0
        maps[0, 1] = 0.25
    else:
        maps[1 % B0, 0] = 0.0
    return {"imgs": imgs[:B].clone(), "maps": maps[:B].clone(), "S": S, "R": R}

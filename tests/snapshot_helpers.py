"""Host restatement (TEST INFRASTRUCTURE ONLY) of the caption / attention snapshot grids: what reference
image_generation/miscc/utils.py:59-306 (build_super_images / build_super_shape_images) computes below the caption
strip, in numpy / scipy / PIL, with PIL's own `paste` for the merged panels.

THIRD-PARTY ARITHMETIC, PARITY UNPINNED: skimage is not installed here.  `pyramid_expand` is taken as skimage >= 0.19
evaluates it on scipy.ndimage -- per channel an order-1 `zoom` (grid_mode, mode 'mirror') to the upscaled size, then
`gaussian_filter(sigma, truncate=4, mode='mirror')`, in float64 -- the convention of oracle/mask_resize.py and
miscc/load.py.  tests/golden/make_golden_snapshot.py runs the unmodified reference functions with exactly this
statement in skimage's place; tests/test_snapshot_cpu.py pins this file to those grids byte for byte.

Dtypes follow the reference: expanded maps are float64 (scipy's result), maps drawn at their own size stay float32 and
are normalised in float32.  One case is defined here because the reference leaves it undefined: in the global form an
image whose maps give max == min divides 0 by 0 and casts NaN to uint8 -- such panels are 0 (csrc/snapshot.hip).
"""
import numpy as np
import torch
from PIL import Image
from scipy import ndimage

COLOR_DIC = {0: [128, 64, 128], 1: [244, 35, 232], 2: [70, 70, 70], 3: [102, 102, 156], 4: [190, 153, 153],
             5: [153, 153, 153], 6: [250, 170, 30], 7: [220, 220, 0], 8: [107, 142, 35], 9: [152, 251, 152],
             10: [70, 130, 180], 11: [220, 20, 60], 12: [255, 0, 0], 13: [0, 0, 142], 14: [119, 11, 32], 15: [0, 60, 100],
             16: [0, 80, 100], 17: [0, 0, 230], 18: [0, 0, 70], 19: [0, 0, 0]}


def pyramid_expand(image, upscale=2, sigma=None, **_ignored):
    """skimage.transform.pyramid_expand of an [h, w] or [h, w, c] image as scipy.ndimage evaluates it (see above)"""
    image = np.asarray(image, np.float64)
    if sigma is None:
        sigma = 2 * upscale / 6.0
    planes = image[:, :, None] if image.ndim == 2 else image
    out = []
    for c in range(planes.shape[2]):
        z = ndimage.zoom(planes[:, :, c], upscale, order=1, mode='mirror', grid_mode=True)
        out.append(ndimage.gaussian_filter(z, sigma=sigma, truncate=4.0, mode='mirror'))
    out = np.stack(out, 2)
    return out[:, :, 0] if image.ndim == 2 else out


def plain_strip(nvis, vis_size, max_word_num, font_max):
    """the caption canvas before any text is drawn: ones, then one colour per word column"""
    strip = np.ones([nvis * font_max, (max_word_num + 2) * (vis_size + 2), 3], np.uint8)
    for i in range(max_word_num):
        strip[:, (i + 2) * (vis_size + 2):(i + 3) * (vis_size + 2), :] = COLOR_DIC[i]
    return strip


def vis_size_of(att_sze, img_size):
    return att_sze * 16 if att_sze == 17 else img_size


def _image_panels(imgs, vis_size):
    """[n, 3, h, w] in [-1, 1] -> float32 [n, vis, vis, 3] in [0, 255] (nn.Upsample bilinear, three in-place fp32 steps)"""
    x = torch.nn.functional.interpolate(imgs.detach().cpu().float().clone(), size=(vis_size, vis_size), mode='bilinear',
                                        align_corners=False)
    x.add_(1).div_(2).mul_(255)
    return np.transpose(x.numpy(), (0, 2, 3, 1))


def _merged(img_f32, att):
    merged = Image.new('RGBA', att.shape[:2][::-1], (0, 0, 0, 0))
    mask = Image.new('L', att.shape[:2][::-1], 210)
    merged.paste(Image.fromarray(np.uint8(img_f32)), (0, 0))
    merged.paste(Image.fromarray(np.uint8(att)), (0, 0), mask)
    return np.array(merged)[:, :, :3]


def grid(imgs, attn_maps, att_sze, strip, lr_imgs=None, max_word_num=12, font_max=50, nvis=None, per_panel_norm=False):
    """-> uint8 [nvis * (font_max + 2 vis), (max_word_num + 2) * (vis + 2), 3].  attn_maps: [B, T, a, a] tensor or a list
    of per-image [1, T_i, a, a] tensors; strip: uint8 [>= nvis * font_max, width, 3], copied into the caption rows."""
    B = int(imgs.shape[0])
    nvis = min(8, B) if nvis is None else nvis
    vis = vis_size_of(att_sze, int(imgs.shape[2]))
    hi = _image_panels(imgs[:nvis], vis)
    lo = _image_panels(lr_imgs[:nvis], vis) if lr_imgs is not None else hi
    pad = np.zeros([vis, 2, 3])
    blank = np.zeros([vis, vis, 3])
    blocks = []
    for i in range(nvis):
        maps = attn_maps[i].detach().cpu().float().reshape(1, -1, att_sze, att_sze)
        maps = torch.cat([maps.max(dim=1, keepdim=True)[0], maps], 1).reshape(-1, 1, att_sze, att_sze)
        maps = np.transpose(maps.repeat(1, 3, 1, 1).numpy(), (0, 2, 3, 1))        # float32 [P, a, a, 3]
        if vis // att_sze > 1:
            panels = [pyramid_expand(m, sigma=20, upscale=vis // att_sze) for m in maps]
        else:
            panels = [m for m in maps]
        gmin, gmax = 1, 0
        for m in panels:
            gmin = m.min() if gmin > m.min() else gmin
            gmax = m.max() if gmax < m.max() else gmax
        line, line_merged = [lo[i], pad], [hi[i], pad]
        for j in range(max_word_num + 1):
            if j < len(panels):
                m = panels[j]
                if per_panel_norm:
                    if m.max() != m.min():
                        m = (m - m.min()) / (m.max() - m.min())
                    m = m * 255
                elif gmax == gmin:
                    m = np.zeros_like(m)                     # the reference's 0 / 0 (see the module docstring)
                else:
                    m = (m - gmin) / (gmax - gmin)
                    m = m * 255
                line += [m, pad]
                line_merged += [_merged(hi[i], m), pad]
            else:
                line += [blank, pad]
                line_merged += [blank, pad]
        blocks.append(np.concatenate([strip[i * font_max:(i + 1) * font_max], np.concatenate(line, 1),
                                      np.concatenate(line_merged, 1)], 0))
    return np.concatenate(blocks, 0).astype(np.uint8)


def regions(nvis, vis, max_word_num, font_max, num_attn):
    """boolean masks over the grid's pixels: 'strip', 'attention' (panels 0 .. num_attn - 1 of the first line),
    'image' (both image panels), 'merged' (merged panels 0 .. num_attn - 1)"""
    Hg, Wg = nvis * (font_max + 2 * vis), (max_word_num + 2) * (vis + 2)
    out = {k: np.zeros((Hg, Wg), bool) for k in ("strip", "attention", "image", "merged")}
    drawn = min(num_attn, max_word_num + 1)
    for n in range(nvis):
        y0 = n * (font_max + 2 * vis)
        out["strip"][y0:y0 + font_max] = True
        y1 = y0 + font_max
        out["image"][y1:y1 + 2 * vis, :vis] = True
        for j in range(drawn):
            x0 = (j + 1) * (vis + 2)
            out["attention"][y1:y1 + vis, x0:x0 + vis] = True
            out["merged"][y1 + vis:y1 + 2 * vis, x0:x0 + vis] = True
    return out


# ---- the fixed-seed cases of the issue, shared by the golden generator and the tests -------------------------------
def _imgs(g, B, s):
    return torch.tanh(torch.randn(B, 3, s, s, generator=g))


def case_a():
    """B = 8, T = 5, att_sze 8, image 16^2, lr 8^2: upscale 2, panels far smaller than the filter radius, zero panels"""
    g = torch.Generator().manual_seed(101)
    return {"imgs": _imgs(g, 8, 16), "lr": _imgs(g, 8, 8), "attn": torch.rand(8, 5, 8, 8, generator=g), "att_sze": 8}


def case_b():
    """att_sze 16, image 16^2, lr 8^2: maps drawn at their own size (float32 normalisation), lr upsample"""
    g = torch.Generator().manual_seed(102)
    return {"imgs": _imgs(g, 8, 16), "lr": _imgs(g, 8, 8), "attn": torch.rand(8, 5, 16, 16, generator=g), "att_sze": 16}


def case_c():
    """att_sze 17, image 32^2, no lr, two images: vis 272, upscale 16, image upsample 32 -> 272"""
    g = torch.Generator().manual_seed(103)
    return {"imgs": _imgs(g, 2, 32), "lr": None, "attn": torch.rand(2, 4, 17, 17, generator=g), "att_sze": 17}


def case_d(s):
    """shape variant: [8, 10, s, s] maps on image 16^2, font_max 20, max_word_num 10, constant maps for the max == min
    branch.  A constant map stays constant only where nothing is summed: at s = 16 (drawn as it is) the constants are
    0.5 and 0; at s = 8 the expansion of a non-zero constant carries rounding noise that normalisation would blow up
    to full range on either side, so the constant there is 0 (every product exact)."""
    g = torch.Generator().manual_seed(104 + s)
    attn = torch.rand(8, 10, s, s, generator=g)
    attn[1, 3] = 0.0
    attn[2, 0] = 0.5 if s == 16 else 0.0
    return {"imgs": _imgs(g, 8, 16), "lr": None, "attn": attn, "att_sze": s}

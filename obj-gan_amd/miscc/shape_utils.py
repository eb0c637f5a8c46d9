"""Snapshot grids of the shape generator (reference shape_generation/miscc/utils.py:59-300): per image a caption strip
with the category word of every box, one line [image | mask panels] and one line [image | panels pasted over the image].
The strip is drawn on the host with PIL, everything below it is composed on the device (objgan_hip.ops.snapshot_grid)
and only the finished uint8 grid is copied back.

    build_super_images    every panel normalised by its own minimum / maximum, (v - min) / (max - min) * 255
    build_super_images2   the raw masks, v * 255

Defined here where the reference is not:
  * a panel with max == min (every empty box slot: an all-zero mask) is the reference's 0 / 0 cast to uint8; it is 0;
  * nvis = min(8, B): the reference indexes past a batch of fewer than 8; from B = 8 on the grid is the reference's;
  * a raw mask value outside [0, 1] saturates to 0 / 255 (the reference's cast of it is undefined).
"""
import numpy as np

from miscc.config import cfg
from miscc.utils import COLOR_DIC, drawCaption, h2d
from objgan_hip import ops


def caption_strip(captions, ixtoword, nvis, vis_size, font_max, font_size, max_word_num, device):
    """the caption rows of a grid, drawn on the host and uploaded: (uint8 device tensor [nvis * font_max, width, 3],
    sentences); the four grids of one display call share one strip"""
    text_convas = np.ones([nvis * font_max, (max_word_num + 2) * (vis_size + 2), 3], dtype=np.uint8)
    for i in range(max_word_num):
        text_convas[:, (i + 2) * (vis_size + 2):(i + 3) * (vis_size + 2), :] = COLOR_DIC[i]
    text_map, sentences = drawCaption(text_convas, captions[:nvis], ixtoword, vis_size, 2, 2, font_max=font_max,
                                      font_size=font_size)
    return h2d(np.array(text_map, dtype=np.uint8), device), sentences


def _super_images(real_imgs, captions, ixtoword, attn_maps, att_sze, lr_imgs, font_max, font_size, max_word_num, norm,
                  strip):
    max_word_num = cfg.TEXT.WORDS_NUM if max_word_num is None else int(max_word_num)
    nvis = min(8, int(real_imgs.size(0)))
    vis_size = att_sze * 16 if att_sze == 17 else int(real_imgs.size(2))
    if strip is None:
        strip = caption_strip(captions, ixtoword, nvis, vis_size, font_max, font_size, max_word_num, real_imgs.device)
    strip, sentences = strip
    maps = attn_maps.reshape(int(attn_maps.shape[0]), -1, att_sze, att_sze)
    grid = ops.snapshot_grid(real_imgs, maps, att_sze, strip, lr_imgs=lr_imgs, max_word_num=max_word_num,
                             font_max=font_max, nvis=nvis, norm=norm)
    return grid.cpu().numpy(), sentences          # the one device-to-host copy: the finished grid


def build_super_images(real_imgs, captions, ixtoword, attn_maps, att_sze, lr_imgs=None, font_max=50, font_size=50,
                       batch_size=None, max_word_num=None, strip=None):
    """Reference shape_generation/miscc/utils.py:59-180 for DEVICE tensors.  real_imgs [B, 3, s, s] in [-1, 1]; attn_maps
    [B, R, (1,) a, a] masks with a == s; captions [B, n] word ids on the host (0 ends a caption).  -> (uint8 ndarray
    [nvis * (font_max + 2 s), (max_word_num + 2) * (s + 2), 3], sentences).  max_word_num defaults to cfg.TEXT.WORDS_NUM at
    call time; batch_size is accepted for the reference's signature and not used (the strip has nvis rows).  strip: what
    `caption_strip` returned for these captions and sizes (None: drawn here)."""
    return _super_images(real_imgs, captions, ixtoword, attn_maps, att_sze, lr_imgs, font_max, font_size, max_word_num,
                         "panel_unguarded", strip)


def build_super_images2(real_imgs, captions, ixtoword, attn_maps, att_sze, lr_imgs=None, font_max=50, font_size=50,
                        batch_size=None, max_word_num=None, strip=None):
    """Reference shape_generation/miscc/utils.py:182-300: the same grid with the masks drawn as they are, v * 255."""
    return _super_images(real_imgs, captions, ixtoword, attn_maps, att_sze, lr_imgs, font_max, font_size, max_word_num,
                         "raw", strip)

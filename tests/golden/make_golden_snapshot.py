#!/usr/bin/env python
"""Record in tests/golden/snapshot_ref.npz what the UNMODIFIED reference `miscc.utils.build_super_images` /
`build_super_shape_images` return for the fixed-seed cases (a), (b) and (d) of tests/snapshot_helpers.py, with their
inputs.  The reference is imported as it is through oracle/ref_harness.py; two of its third-party calls are routed:

  skimage.transform.pyramid_expand -> tests/snapshot_helpers.pyramid_expand (the scipy.ndimage statement; skimage is not
                                      installed here: THIRD-PARTY ARITHMETIC, PARITY UNPINNED)
  ImageFont.truetype               -> a TrueType font of this machine (the reference's FreeMono path does not exist); the
                                      caption rows therefore depend on the machine and no test compares them

Needs /root/reference; the committed .npz is what the tests read.

    python tests/golden/make_golden_snapshot.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import ref_harness as RH            # noqa: E402
import snapshot_helpers as SH                   # noqa: E402

OUT = os.path.join(HERE, "snapshot_ref.npz")
WORDS = ["<end>", "a", "zebra", "standing", "beside", "giraffes", "on", "grassland", "today"]


def captions_for(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    caps = torch.randint(1, len(WORDS), (B, T), generator=g)
    caps[3, T - 2:] = 0                          # a shorter caption
    return caps


def main():
    ref = RH.load_reference()
    U = ref.utils
    from PIL import ImageFont
    real_truetype = ImageFont.truetype
    local = None
    for name in ("DejaVuSansMono.ttf", "FreeMono.ttf", "DejaVuSans.ttf"):
        try:
            real_truetype(name, 50)
            local = name
            break
        except OSError:
            continue
    if local is None:
        raise RuntimeError("no TrueType font on this machine")
    U.skimage.transform.pyramid_expand = SH.pyramid_expand
    ImageFont.truetype = lambda font=None, size=10, *a, **k: real_truetype(local, size)
    ixtoword = dict(enumerate(WORDS))
    rec = {}
    try:
        for name, case in (("a", SH.case_a()), ("b", SH.case_b())):
            caps = captions_for(8, 5, 7)
            grid, sentences = U.build_super_images(case["imgs"].clone(), caps, ixtoword, case["attn"].clone(),
                                                   case["att_sze"], lr_imgs=case["lr"].clone(), batch_size=8,
                                                   max_word_num=12)
            assert grid is not None and grid.dtype == np.uint8 and len(sentences) == 8
            rec[name + "_grid"] = grid
            rec[name + "_captions"] = caps.numpy()
        for s in (8, 16):
            case = SH.case_d(s)
            caps = torch.zeros(8, 10)
            grid, _ = U.build_super_shape_images(case["imgs"].clone(), caps, ixtoword, case["attn"].clone(), s,
                                                 lr_imgs=None, font_max=20, font_size=12, batch_size=8, max_word_num=10)
            assert grid is not None and grid.dtype == np.uint8
            rec["d%d_grid" % s] = grid
    finally:
        ImageFont.truetype = real_truetype
    for name, case in (("a", SH.case_a()), ("b", SH.case_b()), ("d8", SH.case_d(8)), ("d16", SH.case_d(16))):
        rec[name + "_imgs"] = case["imgs"].numpy()
        rec[name + "_attn"] = case["attn"].numpy()
        if case["lr"] is not None:
            rec[name + "_lr"] = case["lr"].numpy()
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", {k: v.shape for k, v in rec.items() if k.endswith("_grid")})


if __name__ == "__main__":
    main()

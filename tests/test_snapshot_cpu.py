"""Snapshot grids, host side: the restatement the GPU tests compare against (tests/snapshot_helpers.py) is pinned to
what the unmodified reference returned (tests/golden/snapshot_ref.npz, tests/golden/make_golden_snapshot.py), the
merged-panel blend of the library to the installed Pillow, and the new entry points are declared, listed and exported."""
import os
import re

import numpy as np
import pytest
import torch

import snapshot_helpers as SH
from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", "snapshot_ref.npz")


@pytest.mark.parametrize("name", ["a", "b", "d8", "d16"])
def test_helper_equals_the_reference_grids_below_the_caption_strip(name):
    gold = np.load(GOLD)
    case = {"a": SH.case_a, "b": SH.case_b, "d8": lambda: SH.case_d(8), "d16": lambda: SH.case_d(16)}[name]()
    # the committed inputs are the ones the case functions regenerate
    assert np.array_equal(gold[name + "_imgs"], case["imgs"].numpy())
    assert np.array_equal(gold[name + "_attn"], case["attn"].numpy())
    if case["lr"] is not None:
        assert np.array_equal(gold[name + "_lr"], case["lr"].numpy())
    shape = name.startswith("d")
    mw, fm = (10, 20) if shape else (12, 50)
    got = SH.grid(case["imgs"], case["attn"], case["att_sze"], SH.plain_strip(8, 16, mw, fm), lr_imgs=case["lr"],
                  max_word_num=mw, font_max=fm, per_panel_norm=shape)
    want = gold[name + "_grid"]
    assert got.shape == want.shape == (8 * (fm + 32), (mw + 2) * 18, 3)
    below = ~SH.regions(8, 16, mw, fm, case["attn"].shape[1] + 1)["strip"]     # (the strip depends on the font)
    assert np.array_equal(got[below], want[below])
    if shape:       # the constant maps took the max == min branch: drawn unnormalised
        R = SH.regions(8, 16, mw, fm, 11)
        y0, x0 = 2 * (fm + 32) + fm, (0 + 2) * 18                              # image 2, map 0 = panel 1
        assert R["attention"][y0, x0]
        assert (want[y0:y0 + 16, x0:x0 + 16] == (127 if name == "d16" else 0)).all()


def test_blend_table_equals_pillow_on_all_pairs():
    from PIL import Image
    from objgan_hip import ops
    table = ops.paste_blend_table()
    im = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, 1)           # rows: image byte, columns: attention byte
    att = np.ascontiguousarray(im.T)
    merged = Image.new('RGBA', (256, 256), (0, 0, 0, 0))
    merged.paste(Image.fromarray(np.stack([im] * 3, -1)), (0, 0))
    merged.paste(Image.fromarray(np.stack([att] * 3, -1)), (0, 0), Image.new('L', (256, 256), 210))
    want = np.array(merged)
    assert table.shape == (256, 256) and table.dtype == np.uint8
    for c in range(3):
        assert np.array_equal(table, want[:, :, c])


def test_snapshot_entry_points_are_declared_listed_and_exported():
    from objgan_hip import _lib, build, ops
    header = open(os.path.join(ROOT, "include", "objgan_hip.h")).read()
    lib = _lib.load()
    for name in ("objgan_snapshot_grid", "objgan_snapshot_blend_table", "objgan_snapshot_ws_doubles"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES or name in _lib.LONG_RETURN, name
        assert getattr(lib, name) is not None
    assert "snapshot.hip" in build.sources()
    assert callable(ops.snapshot_grid)
    # the workspace query is host-only arithmetic: expanded maps + half product + tile and panel statistics
    assert lib.objgan_snapshot_ws_doubles(8, 5, 8, 16) == 48 * 256 + 48 * 128 + 2 * 48 + 2 * 8 * 7
    assert lib.objgan_snapshot_ws_doubles(8, 5, 16, 8) == 0
    with pytest.raises(_lib.ObjganHipError):        # no CPU path
        ops.snapshot_grid(torch.zeros(1, 3, 16, 16), torch.zeros(1, 2, 16, 16), 16, torch.zeros(50, 252, 3, dtype=torch.uint8),
                          nvis=1)


def test_expansion_matrix_is_the_scipy_statement():
    """M A M^T against zoom + gaussian_filter of scipy, at the sizes the grids use (and one panel narrower than the
    filter radius many times over)"""
    from objgan_hip import ops
    rng = np.random.RandomState(3)
    for a, vis in ((8, 16), (17, 272), (64, 128)):
        M = ops.expansion_matrix(a, vis)
        A = rng.rand(a, a)
        want = SH.pyramid_expand(A, upscale=vis // a, sigma=20)
        assert M.shape == (vis, a) and np.abs(M.dot(A).dot(M.T) - want).max() < 1e-14


def test_draw_caption_falls_back_without_the_reference_font(monkeypatch, capsys):
    from miscc import utils as U
    from miscc.config import cfg
    monkeypatch.setattr(cfg, "DATA_DIR", "/nonexistent/data/dir")
    monkeypatch.setattr(U, "_FONTS", {})
    canvas = SH.plain_strip(2, 16, 12, 50)
    caps = torch.tensor([[1, 2, 0], [2, 2, 1]])
    img, sentences = U.drawCaption(canvas, caps, {1: "zebra", 2: "grassland"}, 16)
    assert sentences == [["zebra", "grassland"], ["grassland", "grassland", "zebra"]]
    out = np.asarray(img)
    assert out.shape == canvas.shape and out.dtype == np.uint8
    assert (out != canvas).any()                                            # something was drawn
    U.drawCaption(canvas, caps, {1: "zebra", 2: "grassland"}, 16)
    assert capsys.readouterr().out.count("caption font") == 1              # one notice per process

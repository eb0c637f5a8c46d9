"""Snapshot grids on the device (csrc/snapshot.hip, objgan_hip.ops.snapshot_grid, miscc.utils.build_super_images,
condGANTrainer.save_img_results) against the host restatement of tests/snapshot_helpers.py, computed at test time.

Bounds (fixed seeds):
  attention panels   byte-exact.  Both sides work in fp64 (fp32 where the maps are drawn at their own size, with the same
                     three operations); a different summation order moves a value by ~1e-13 of a grey level.
  image / merged     at most 1 grey level anywhere, at most 1e-3 of those panels' bytes: fp32 bilinear + the three-step
                     affine carry ~2 ulp at 255 (3e-5 of a level), so ~1e-4 of the values straddle an integer; where
                     vis equals the image size the image panel is byte-exact.
  caption strip      equal to the uploaded strip; pads and panels past the last map are 0.
"""
import os
import random

import numpy as np
import pytest
import torch

import snapshot_helpers as SH
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _strip(nvis, vis, mw, fm, seed=5):
    """a caption strip with content in every byte (the compose kernel copies it; no font involved)"""
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, size=(nvis * fm, (mw + 2) * (vis + 2), 3)).astype(np.uint8)


def _run(dev, case, mw, fm, nvis, per_panel=False, strip=None):
    from objgan_hip import ops
    vis = SH.vis_size_of(case["att_sze"], int(case["imgs"].shape[2]))
    strip = _strip(nvis, vis, mw, fm) if strip is None else strip
    attn = case["attn"]
    attn_dev = [m.to(dev) for m in attn] if isinstance(attn, list) else attn.to(dev)
    got = ops.snapshot_grid(case["imgs"].to(dev), attn_dev, case["att_sze"], torch.from_numpy(strip).to(dev),
                            lr_imgs=None if case["lr"] is None else case["lr"].to(dev), max_word_num=mw, font_max=fm,
                            nvis=nvis, per_panel_norm=per_panel)
    want = SH.grid(case["imgs"], attn, case["att_sze"], strip, lr_imgs=case["lr"], max_word_num=mw, font_max=fm,
                   nvis=nvis, per_panel_norm=per_panel)
    return got.cpu().numpy(), want, strip, vis


def _check(got, want, strip, vis, mw, fm, nvis, num_attn, exact_image, tag):
    assert got.shape == want.shape == (nvis * (fm + 2 * vis), (mw + 2) * (vis + 2), 3) and got.dtype == np.uint8
    R = SH.regions(nvis, vis, mw, fm, num_attn)
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    att_bad = int((diff[R["attention"]] != 0).sum())
    soft = R["image"] | R["merged"]
    soft_max, soft_share = int(diff[soft].max()), float((diff[soft] != 0).mean())
    rest = ~(R["attention"] | soft | R["strip"])
    print("%s: attention bytes differing %d of %d; image+merged max %d, share %.3g; image exact: %s"
          % (tag, att_bad, 3 * int(R["attention"].sum()), soft_max, soft_share, int(diff[R["image"]].max()) == 0))
    assert np.array_equal(got[R["strip"]].reshape(nvis, fm, -1, 3), strip.reshape(nvis, fm, -1, 3))
    assert att_bad == 0
    assert soft_max <= 1 and soft_share <= 1e-3
    if exact_image:
        assert int(diff[R["image"]].max()) == 0
    assert np.array_equal(got[rest], want[rest]) and not got[rest].any()          # pads and empty panels


def test_case_a_upscale_2_far_below_the_filter_radius(dev):
    got, want, strip, vis = _run(dev, SH.case_a(), 12, 50, 8)
    _check(got, want, strip, vis, 12, 50, 8, 6, False, "a")
    # the caption strip aside, this is what the unmodified reference returned
    gold = np.load(os.path.join(ROOT, "tests", "golden", "snapshot_ref.npz"))["a_grid"]
    R = SH.regions(8, 16, 12, 50, 6)
    assert np.array_equal(got[R["attention"]], gold[R["attention"]])


def test_case_b_maps_at_their_own_size(dev):
    got, want, strip, vis = _run(dev, SH.case_b(), 12, 50, 8)
    _check(got, want, strip, vis, 12, 50, 8, 6, False, "b")
    R = SH.regions(8, 16, 12, 50, 6)
    lr_panel = R["image"].copy()
    lr_panel[:] = False
    for n in range(8):
        y1 = n * (50 + 32) + 50
        lr_panel[y1 + 16:y1 + 32, :16] = True           # second line: the image at its own size -> byte-exact
    assert np.array_equal(got[lr_panel], want[lr_panel])
    gold = np.load(os.path.join(ROOT, "tests", "golden", "snapshot_ref.npz"))["b_grid"]
    assert np.array_equal(got[R["attention"]], gold[R["attention"]])


def test_case_c_vis_272_upscale_16(dev):
    got, want, strip, vis = _run(dev, SH.case_c(), 12, 50, 2)
    assert vis == 272
    _check(got, want, strip, vis, 12, 50, 2, 5, False, "c")


@pytest.mark.parametrize("s", [8, 16])
def test_case_d_shape_variant_with_constant_maps(dev, s):
    got, want, strip, vis = _run(dev, SH.case_d(s), 10, 20, 8, per_panel=True)
    _check(got, want, strip, vis, 10, 20, 8, 11, True, "d%d" % s)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "snapshot_ref.npz"))["d%d_grid" % s]
    R = SH.regions(8, 16, 10, 20, 11)
    assert np.array_equal(got[R["attention"]], gold[R["attention"]])


def test_edge_cases_batch_sizes_zero_maps_and_ragged_lists(dev):
    from miscc import utils as U
    g = torch.Generator().manual_seed(7)
    words = {1: "zebra", 2: "grass"}
    for B, rows in ((10, 8), (4, 4)):
        imgs, lr = torch.tanh(torch.randn(B, 3, 16, 16, generator=g)), torch.tanh(torch.randn(B, 3, 8, 8, generator=g))
        attn = torch.rand(B, 3, 8, 8, generator=g)
        attn[1] = 0.0                                   # an image whose maps are all zero: panels of 0
        caps = torch.ones(B, 3, dtype=torch.long)
        grid, sentences = U.build_super_images(imgs.to(dev), caps, words, attn.to(dev), 8, lr_imgs=lr.to(dev), max_word_num=12)
        assert grid.dtype == np.uint8 and grid.shape == (rows * (50 + 32), 14 * 18, 3) and len(sentences) == B
        want = SH.grid(imgs, attn, 8, SH.plain_strip(rows, 16, 12, 50), lr_imgs=lr, max_word_num=12, font_max=50, nvis=rows)
        R = SH.regions(rows, 16, 12, 50, 4)
        assert np.array_equal(grid[R["attention"]], want[R["attention"]])
        y1 = 1 * 82 + 50
        assert not grid[y1:y1 + 16, 18:].any()          # zero maps: attention panels of image 1 are 0, nothing undefined
        diff = np.abs(grid.astype(np.int16) - want.astype(np.int16))[R["image"] | R["merged"]]
        assert diff.max() <= 1 and (diff != 0).mean() <= 1e-3
    # per-image lists of different lengths (the DAMSM word attention of captions of different lengths)
    case = SH.case_a()
    case["attn"] = [case["attn"][i:i + 1, :1 + i % 5].clone() for i in range(8)]
    got, want, strip, vis = _run(dev, case, 12, 50, 8)
    R = SH.regions(8, 16, 12, 50, 1)                    # (regions of the shortest list; every other byte is compared below)
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    soft = R["image"] | SH.regions(8, 16, 12, 50, 6)["merged"]
    assert diff[~soft].max() == 0 and diff[soft].max() <= 1 and (diff[soft] != 0).mean() <= 1e-3


def test_the_same_call_twice_gives_identical_bytes(dev):
    from objgan_hip import ops
    case = SH.case_c()
    strip = torch.from_numpy(_strip(2, 272, 12, 50)).to(dev)
    args = (case["imgs"].to(dev), case["attn"].to(dev), 17, strip)
    one = ops.snapshot_grid(*args, nvis=2)
    two = ops.snapshot_grid(*args, nvis=2)
    assert torch.equal(one, two)


def test_trainer_save_img_results_writes_the_grids_and_leaves_training_untouched(dev, tmp_path, monkeypatch):
    """tests/golden/data_tiny, one stage, B = 2: save_img_results writes the reference's file names with the expected
    sizes; the generator arena, EMA, optimiser moments, BatchNorm buffers and training flags are bit-identical
    afterwards, and the next train_step equals the train_step of a twin trainer that took no snapshot."""
    from PIL import Image
    from torch.utils.data.dataloader import default_collate
    import model as M
    import trainDataset
    import trainer as T
    from oracle import ref_harness as rh
    from miscc.config import cfg

    class _ConstEncoder(object):
        """constant image encoder: fixed region features for the DAMSM terms (as tests/test_trainer_cpu.py)"""

        def __init__(self, regions, code):
            self.regions, self.code = regions.detach(), code.detach()

        def __call__(self, x):
            return self.regions, self.code

        def parameters(self):
            return []

        def eval(self):
            return self

    monkeypatch.setattr(cfg.TREE, "BRANCH_NUM", 1)
    monkeypatch.setattr(cfg.TRAIN, "BATCH_SIZE", 2)
    monkeypatch.setattr(cfg.TRAIN, "NET_G", '')
    monkeypatch.setattr(cfg.TRAIN, "FLAG", True)
    ds = trainDataset.TrainDataset(os.path.join(ROOT, "tests", "golden", "data_tiny"), "train", base_size=64,
                                   device_hmaps=True)
    nc, B = ds.num_classes, 2
    g0 = torch.Generator().manual_seed(11)
    regions_c, code_c = torch.randn(B, 256, 17, 17, generator=g0).to(dev), torch.randn(B, 256, generator=g0).to(dev)
    np.random.seed(4)
    collated = default_collate([ds[0], ds[1]])
    noise = torch.randn(B, cfg.GAN.Z_DIM, generator=g0).to(dev)
    eps = torch.randn(B, cfg.GAN.CONDITION_DIM, generator=g0).to(dev)

    def make(out_dir):
        ds.image_encoder = _ConstEncoder(regions_c, code_c)
        ds.text_encoder = rh.seeded_state_(M.RNN_ENCODER(ds.n_words, nhidden=cfg.TEXT.EMBEDDING_DIM), 91).to(dev).eval()
        for p in ds.text_encoder.parameters():
            p.requires_grad_(False)
        tr = T.condGANTrainer(str(out_dir), None, ds, device=dev)
        tr.batch_size = B
        nets = [ds.text_encoder, ds.image_encoder, rh.seeded_state_(M.G_NET(nc), 92),
                [rh.seeded_state_(M.PAT_D_NET64(), 93)], [rh.seeded_state_(M.SHP_D_NET64(nc), 94)],
                rh.seeded_state_(M.OBJ_SS_D_NET(nc), 95), rh.seeded_state_(M.OBJ_LS_D_NET(nc), 96), 0]
        for m in [nets[2], nets[5], nets[6]] + nets[3] + nets[4]:
            m.to(dev).train()
        tr.build_models = lambda: nets
        tr.setup()
        tr.netG.ca_net.fixed_eps = eps
        batch = trainDataset.batch_dict(trainDataset.prepare_data(collated, dev, nc), tr.clabels_emb)
        return tr, batch

    def state(tr):
        a = tr.optimizerG.arena
        out = [a.flat, a.grad, a.exp_avg, a.exp_avg_sq, tr.avg_param_G] + [b_ for _, b_ in tr.netG.named_buffers()]
        return [t.detach().clone() for t in out], [m.training for m in tr.netG.modules()]

    tr, batch = make(tmp_path / "with")
    assert tr.fixed_noise.shape == (B, cfg.GAN.Z_DIM)
    before = state(tr)
    written = tr.save_img_results(batch, tr.fixed_noise, 3, name='average')
    after = state(tr)
    assert all(torch.equal(x, y) for x, y in zip(before[0], after[0])) and before[1] == after[1]
    # one stage has no attention stage: the DAMSM grid only (17 x 17 regions -> 272-pixel panels)
    assert sorted(os.listdir(tr.image_dir)) == ["D_average_3.png"] and [os.path.basename(p) for p in written] == ["D_average_3.png"]
    assert Image.open(written[0]).size == (14 * 274, B * (50 + 2 * 272))
    assert Image.open(written[0]).mode == "RGB"
    random.seed(5)
    torch.manual_seed(5)
    got = tr.train_step(batch, noise=noise)
    twin, batch2 = make(tmp_path / "without")
    random.seed(5)
    torch.manual_seed(5)
    want = twin.train_step(batch2, noise=noise)
    for k in ("errPatD0", "errShpD0", "errG", "kl"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["fake_imgs"][0], want["fake_imgs"][0])
    assert torch.equal(tr.optimizerG.arena.flat, twin.optimizerG.arena.flat)


def test_evaluator_snapshot_writers(dev, tmp_path):
    """evaluator.save_img_results / save_shape_results on a three-stage output of B = 2: the reference's file names in
    Snapshot/, the grids' sizes, and the shape grid's panels against the host restatement (64 x 64 maps drawn at their own
    size, every panel normalised on its own, more maps than panels in the ground-truth form)."""
    from PIL import Image
    import evaluator as E
    from miscc.config import cfg

    class DS(object):
        ixtoword = {1: "zebra", 2: "grass"}
        cats_dict = {0: [1], 1: [2]}
        cats_index_dict = {0: 0, 1: 1}
    ev = E.condGANEvaluator(str(tmp_path), None, DS(), device=dev)
    g = torch.Generator().manual_seed(9)
    B = 2
    fake = [torch.tanh(torch.randn(B, 3, s, s, generator=g)).to(dev) for s in (64, 128, 256)]
    attn = [torch.rand(B, 4, a, a, generator=g).to(dev) for a in (64, 128)]
    bt = [torch.rand(B, 3, a, a, generator=g).to(dev) for a in (64, 128)]
    caps = torch.tensor([[1, 2, 1, 0], [2, 1, 1, 2]])
    ev.save_img_results(fake, attn, bt, caps, None, 5)
    rois = torch.zeros(B, cfg.ROI.BOXES_NUM, 5)
    rois[:, :2, 4] = torch.tensor([0., 1.])
    num_rois = torch.tensor([2, 1])
    masks = torch.rand(B, 2, 64, 64, generator=g)
    layout = torch.rand(B, 14, 64, 64, generator=g)
    layout[0, 3] = 0.25                                  # a constant map: drawn as it is
    ev.save_shape_results(fake[0], masks.to(dev), rois, num_rois, 5, 'G')
    ev.save_shape_results(fake[0], layout.to(dev), rois, num_rois, 5, 'D')
    assert sorted(os.listdir(ev.snapshot_dir)) == ["G_5_0.png", "G_5_1.png", "ShapeD_5.png", "ShapeG_5.png", "bt_G_5_0.png",
                                                   "bt_G_5_1.png"]
    sizes = {n: Image.open(os.path.join(ev.snapshot_dir, n)).size for n in os.listdir(ev.snapshot_dir)}
    mw = cfg.TEXT.WORDS_NUM
    assert sizes["G_5_0.png"] == sizes["bt_G_5_0.png"] == ((mw + 2) * 130, B * (50 + 256))
    assert sizes["G_5_1.png"] == sizes["bt_G_5_1.png"] == ((mw + 2) * 258, B * (50 + 512))
    bn = cfg.ROI.BOXES_NUM
    assert sizes["ShapeG_5.png"] == sizes["ShapeD_5.png"] == ((bn + 2) * 66, B * (20 + 128))
    for name, maps in (("ShapeG_5.png", masks), ("ShapeD_5.png", layout)):
        got = np.array(Image.open(os.path.join(ev.snapshot_dir, name)))
        want = SH.grid(fake[0].cpu(), maps, 64, SH.plain_strip(B, 64, bn, 20), max_word_num=bn, font_max=20, nvis=B,
                       per_panel_norm=True)
        R = SH.regions(B, 64, bn, 20, maps.shape[1] + 1)
        assert np.array_equal(got[R["attention"]], want[R["attention"]]) and np.array_equal(got[R["image"]], want[R["image"]])
        assert np.array_equal(got[R["merged"]], want[R["merged"]])      # (image panels at their own size: exact)

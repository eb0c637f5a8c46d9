"""The shape generator's pictures on the MI355X: the mask dump kernel and the two shape-stage forms of the grid kernel
against the host restatement (tests/shape_snapshot_helpers.py) and against what the unmodified reference drew
(tests/golden/shape_snapshot_ref.npz), the trainer's display call, the sampling command's path on the fixture
tests/golden/shape_tiny_test.

Bounds: everything here is byte for byte.  The masks are drawn at their own size, the image panels at the images' own
size, and both sides round the same fp32 operations one by one; no sum is involved, so there is no order to differ in."""
import os

import numpy as np
import pytest
import torch

import shape_snapshot_helpers as SSH
import snapshot_helpers as SH
import shapegen_oracle as so
from conftest import ROOT

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "shape_snapshot_ref.npz")
TINY = os.path.join(ROOT, "tests", "golden", "shape_tiny")
FIXTURE = os.path.join(ROOT, "tests", "golden", "shape_tiny_test")
NBF = 16


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _ops():
    from objgan_hip import ops
    return ops


# ---------------------------------------------------------------------------------------------
# mask_to_rgb8
# ---------------------------------------------------------------------------------------------
def _planes(h, w, count, seed):
    """`count` planes: random, with negative values, constant non-zero, {0, 1e-40}, exact 0 and 1, then random again"""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(count, h, w, generator=g)
    p[1] = torch.randn(h, w, generator=g) * 3 - 1
    p[2] = 0.37
    p[3] = 0.0
    p[3].view(-1)[(h * w) // 2] = 1e-40                    # a denormal maximum: 0 and 255, as numpy gives
    p[4] = (torch.rand(h, w, generator=g) > 0.5).float()
    p[5] = -torch.rand(h, w, generator=g) * 1e-3
    return p


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (7, 9), (5, 13), (64, 64)])
def test_mask_to_rgb8_against_the_helper(dev, h, w):
    ops = _ops()
    planes = _planes(h, w, 40, 11 + h * w)
    assert float(planes[3].max()) > 0.0                     # (the denormal survived the host)
    pd = planes.to(dev)
    want_all = SSH.mask_rgb(planes.numpy())
    if h * w > 1:
        assert want_all[3].max() == 255 and want_all[3].astype(int).sum() == 3 * 255 and not want_all[2].any()
    # N = 1, every kind of plane on its own
    for k in range(6):
        got = ops.mask_to_rgb8(pd[k])
        assert got.shape == (1, h, w, 3) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy()[0], want_all[k]), (h, w, k)
    # all planes, in order
    assert np.array_equal(ops.mask_to_rgb8(pd).cpu().numpy(), want_all)
    # N = 30 through a non-contiguous, unordered selection with a repeated index
    sel = [39, 3, 17, 2, 2, 0, 5, 31, 4, 1, 38, 9, 22, 7, 36, 11, 29, 13, 27, 15, 25, 8, 23, 19, 21, 6, 33, 35, 3, 10]
    assert len(sel) == 30 and len(set(sel)) < 30
    got = ops.mask_to_rgb8(pd, sel)
    again = ops.mask_to_rgb8(pd, sel)
    torch.cuda.synchronize()
    assert torch.equal(got, again)
    assert np.array_equal(got.cpu().numpy(), want_all[sel])
    assert torch.equal(ops.mask_to_rgb8(pd, torch.tensor(sel, device=dev)), got)          # a device selection
    # a base that is not 16-byte aligned takes the scalar path and gives the same bytes
    shifted = torch.empty(planes.numel() + 1, device=dev)[1:].view_as(planes).copy_(pd)
    assert shifted.data_ptr() % 16 != 0
    assert torch.equal(ops.mask_to_rgb8(shifted, sel), got)


def test_mask_to_rgb8_refuses_a_selection_outside_the_planes(dev):
    ops = _ops()
    from objgan_hip._lib import ObjganHipError
    pd = torch.rand(4, 8, 8, device=dev)
    for sel in ([4], [-1], [], torch.tensor([0, 7], device=dev)):
        with pytest.raises(ObjganHipError):
            ops.mask_to_rgb8(pd, sel)
    with pytest.raises(ObjganHipError):
        ops.mask_to_rgb8(pd.cpu())


# ---------------------------------------------------------------------------------------------
# snapshot_grid, the shape stage's forms
# ---------------------------------------------------------------------------------------------
def _strip(nvis, S, seed=5):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, size=(nvis * SSH.FONT_MAX, 12 * (S + 2), 3)).astype(np.uint8)


def _grid(dev, case, norm, nvis, strip):
    got = _ops().snapshot_grid(case["imgs"].to(dev), case["maps"].to(dev), case["S"], torch.from_numpy(strip).to(dev),
                               max_word_num=10, font_max=SSH.FONT_MAX, nvis=nvis, norm=norm)
    return got.cpu().numpy()


@pytest.mark.parametrize("form,norm", [("norm", "panel_unguarded"), ("raw", "raw")])
@pytest.mark.parametrize("name", list(SSH.GRID_CASES))
def test_grid_forms_against_the_reference_golden(dev, gold, name, form, norm):
    B, S, R = SSH.GRID_CASES[name]
    case = SSH.grid_case(name)
    strip = _strip(8, S)
    got = _grid(dev, case, norm, 8, strip)
    ref = gold["%s_%s_grid" % (name, form)]
    assert got.shape == ref.shape
    assert np.array_equal(SSH.below_strip(got, 8, S), SSH.below_strip(ref, 8, S))
    assert np.array_equal(got, SSH.grid(case["imgs"], case["maps"], strip, form))           # the strip rows included
    assert np.array_equal(got, _grid(dev, case, norm, 8, strip))
    # three images: nvis = 3
    small = SSH.grid_case(name, B=3)
    strip3 = _strip(3, S, seed=6)
    assert np.array_equal(_grid(dev, small, norm, 3, strip3), SSH.grid(small["imgs"], small["maps"], strip3, form))


def test_raw_form_saturates_outside_the_unit_range(dev):
    case = SSH.grid_case("s8r3")
    case["maps"][3, 0] = case["maps"][3, 0] * 4 - 2                 # values in [-2, 2)
    strip = _strip(8, 8)
    got = _grid(dev, case, "raw", 8, strip)
    assert np.array_equal(got, SSH.grid(case["imgs"], case["maps"], strip, "raw"))
    y, x = 3 * (SSH.FONT_MAX + 16) + SSH.FONT_MAX, 2 * 10
    assert got[y:y + 8, x:x + 8].min() == 0 and got[y:y + 8, x:x + 8].max() == 255


def test_existing_forms_are_unchanged_and_expansion_refuses_the_new_ones(dev):
    ops = _ops()
    from objgan_hip._lib import ObjganHipError
    for case, mw, fm, per_panel, num_attn in ((SH.case_b(), 12, 50, False, 6), (SH.case_d(16), 10, 20, True, 11)):
        rng = np.random.RandomState(5)
        strip = rng.randint(0, 256, size=(8 * fm, (mw + 2) * 18, 3)).astype(np.uint8)
        args = (case["imgs"].to(dev), case["attn"].to(dev), 16, torch.from_numpy(strip).to(dev))
        kw = dict(lr_imgs=None if case["lr"] is None else case["lr"].to(dev), max_word_num=mw, font_max=fm, nvis=8)
        got = ops.snapshot_grid(*args, norm="panel" if per_panel else "global", **kw)
        assert torch.equal(got, ops.snapshot_grid(*args, per_panel_norm=per_panel, **kw))       # the older spelling
        want = SH.grid(case["imgs"], case["attn"], 16, strip, lr_imgs=case["lr"], max_word_num=mw, font_max=fm, nvis=8,
                       per_panel_norm=per_panel)
        R = SH.regions(8, 16, mw, fm, num_attn)
        got = got.cpu().numpy()
        assert np.array_equal(got[R["attention"]], want[R["attention"]])
        assert np.array_equal(got[R["strip"]], want[R["strip"]])
        assert int(np.abs(got.astype(np.int16) - want.astype(np.int16)).max()) <= 1
    a = SH.case_a()                                                     # 8 x 8 maps on 16 x 16 images: an expansion
    strip = torch.zeros(8 * 50, 14 * 18, 3, dtype=torch.uint8, device=dev)
    for norm in ("raw", "panel_unguarded"):
        with pytest.raises(ObjganHipError):
            ops.snapshot_grid(a["imgs"].to(dev), a["attn"].to(dev), 8, strip, norm=norm)
    with pytest.raises(ObjganHipError):
        ops.snapshot_grid(a["imgs"].to(dev), a["attn"].to(dev), 8, strip, norm="other")


# ---------------------------------------------------------------------------------------------
# the trainer's display call
# ---------------------------------------------------------------------------------------------
def _cfg(monkeypatch, B, flag=True, display=500):
    from miscc.config import cfg
    monkeypatch.setitem(cfg.GAN, "R_NUM", 1)
    monkeypatch.setitem(cfg.TRAIN, "BATCH_SIZE", B)
    monkeypatch.setitem(cfg.TRAIN, "FLAG", flag)
    monkeypatch.setitem(cfg.TRAIN, "NET_G", "")
    monkeypatch.setitem(cfg.TRAIN, "MAX_EPOCH", 1)
    monkeypatch.setitem(cfg.TRAIN, "PRINT_INTERVAL", 100)
    monkeypatch.setitem(cfg.TRAIN, "DISPLAY_INTERVAL", display)
    monkeypatch.setitem(cfg.TRAIN, "RNN_GRAD_CLIP", 0.25)
    monkeypatch.setitem(cfg.TRAIN.SMOOTH, "PCP_LAMBDA", 0.0)
    monkeypatch.setitem(cfg.TRAIN.SMOOTH, "INS_LAMBDA", 1.0)
    monkeypatch.setitem(cfg.TRAIN.SMOOTH, "GLB_LAMBDA", 1.0)
    return cfg


def _fixture():
    import shapeDataset
    return shapeDataset.TextDataset(FIXTURE, "test", base_size=64)


def _seeded_trainer(dev, out_dir, ds):
    import model
    import shape_trainer
    t = shape_trainer.condGANTrainer(str(out_dir), None, ds, device=dev)
    t.attach(so.seeded_state_(model.SHP_G_NET(NBF), so.SEEDS["G"]), so.seeded_state_(model.INS_D_NET(NBF), so.SEEDS["INSD"]),
             so.seeded_state_(model.GLB_D_NET(NBF), so.SEEDS["GLBD"]))
    t.define_optimizers(1.0)
    return t


def _state(t):
    """every tensor of the training state: the three arenas, their moments, the generator's step state, the EMA copy,
    the noise buffer and the device's random stream"""
    out = {"avg": t.avg_param_G, "noise": t.noise, "rng": torch.cuda.get_rng_state(t.device),
           "optG.state": t.optimizerG.state, "optG.clip": t.optimizerG.clip, "optG.coef": t.optimizerG.coef}
    for name, a in (("G", t.arenaG), ("INSD", t.arenaINSD), ("GLBD", t.arenaGLBD)):
        out.update({name + ".flat": a.flat, name + ".grad": a.grad, name + ".m": a.exp_avg, name + ".v": a.exp_avg_sq})
        if a.gate_state is not None:
            out[name + ".gate"] = a.gate_state
    return {k: v.detach().clone() for k, v in out.items()}


def _same_bits(a, b):
    """bit for bit, whatever the bits say: the noise buffer is uninitialised memory when the noise is handed in, and the
    suite fills free device memory with NaNs, which compare unequal to themselves by value"""
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _generator_masks(dev, flat, batch, noise):
    """the masks of a fresh SHP_G_NET holding the flat parameter vector `flat`, computed by the test itself"""
    import model
    net = model.SHP_G_NET(NBF).to(dev)
    off = 0
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        assert off == flat.numel()
        return net(noise, batch["bbox_maps_fwd"], batch["bbox_maps_bwd"], batch["bbox_fmaps"])


def test_display_call_writes_the_four_grids_and_leaves_the_training_state(dev, tmp_path, monkeypatch):
    import shapeDataset
    from PIL import Image
    _cfg(monkeypatch, 8)
    ds = _fixture()
    collate = torch.utils.data.default_collate
    idx = (0, 2, 3, 4, 1, 2, 3, 4)                                      # 1, 10, 2, 3, 0, 10, 2, 3 boxes
    g = torch.Generator().manual_seed(41)
    z1, z2, zf = (torch.randn(8, 10, 4 * NBF, generator=g).to(dev) for _ in range(3))
    losses = {}
    for run in ("with", "without"):
        t = _seeded_trainer(dev, tmp_path / run, ds)
        batch = shapeDataset.prepare_data(collate([ds[i] for i in idx]), dev, NBF)
        R = batch["max_num_roi"]
        assert R == 10
        t.train_step(batch, noise=z1[:, :R])
        if run == "with":
            before = _state(t)
            paths = t.save_img_results(batch, zf[:, :R], 7, name="average")
            torch.cuda.synchronize()
            after = _state(t)
            for k in before:
                assert _same_bits(before[k], after[k]), k
            assert not torch.equal(t.avg_param_G, t.arenaG.flat)        # (the swap had something to swap)
            image_dir = os.path.join(str(tmp_path / run), "Image")
            assert sorted(os.listdir(image_dir)) == sorted("%s_average_7.png" % s for s in ("G", "D", "G2", "D2"))
            assert sorted(paths) == sorted(os.path.join(image_dir, f) for f in os.listdir(image_dir))
            fake = _generator_masks(dev, t.avg_param_G, batch, zf[:, :R]).cpu()
            imgs = ds.images_for(batch["keys"][:8])
            for tag, maps, form in (("G", fake, "norm"), ("D", batch["hmaps"].cpu(), "norm"), ("G2", fake, "raw"),
                                    ("D2", batch["hmaps"].cpu(), "raw")):
                got = np.array(Image.open(os.path.join(image_dir, "%s_average_7.png" % tag)))
                assert got.shape == (8 * (20 + 128), 12 * 66, 3) and got.dtype == np.uint8
                want = SSH.grid(imgs, maps, got, form)                  # (the strip is the file's own: fonts differ by machine)
                bad = int((SSH.below_strip(got, 8, 64) != SSH.below_strip(want, 8, 64)).sum())
                print(tag, "bytes differing below the strip:", bad)
                assert bad == 0, tag
            # the image with one box: its real mask spans the full range, its nine empty slots (the reference's 0 / 0) are 0
            d_norm = np.array(Image.open(os.path.join(image_dir, "D_average_7.png")))
            assert d_norm[20:20 + 64, 2 * 66:3 * 66 - 2].max() == 255 and not d_norm[20:20 + 64, 3 * 66:].any()
        out = t.train_step(batch, noise=z2[:, :R])
        torch.cuda.synchronize()
        losses[run] = {k: out[k].clone() for k in ("errINSD", "errGLBD", "errG", "insg_loss", "glbg_loss")}
        losses[run]["flat"] = t.arenaG.flat.clone()
    for k in losses["with"]:
        assert _same_bits(losses["with"][k], losses["without"][k]), k


def test_training_draws_the_grids_at_the_interval_and_goes_without_an_image_file(dev, tmp_path, monkeypatch, capsys):
    import shapeDataset
    import shape_trainer
    _cfg(monkeypatch, 2, display=1)
    # a data directory that has its images: 2 whole batches of the fixture, a grid set after each
    ds = _fixture()
    loader = torch.utils.data.DataLoader(ds, batch_size=2, drop_last=True, shuffle=False)
    t = shape_trainer.condGANTrainer(str(tmp_path / "a"), loader, ds, device=dev)
    t.train()
    text = capsys.readouterr().out
    assert "Not built" in text and "grids" not in text.split("Not built", 1)[1].splitlines()[0]
    want = {"%s_average_%d.png" % (s, n) for s in ("G", "D", "G2", "D2") for n in (1, 2)}
    assert set(os.listdir(os.path.join(str(tmp_path / "a"), "Image"))) == want
    # one without: one notice, the same training, no picture
    ds = shapeDataset.TextDataset(TINY, "train", base_size=64)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, drop_last=True, shuffle=False)
    t = shape_trainer.condGANTrainer(str(tmp_path / "b"), loader, ds, device=dev)
    t.train()
    text = capsys.readouterr().out
    assert text.count("train_imgs.bigfile") == 1 and text.count("without the DISPLAY_INTERVAL grids") == 1
    assert os.listdir(os.path.join(str(tmp_path / "b"), "Image")) == []
    assert "netG_epoch_1.pth" in os.listdir(os.path.join(str(tmp_path / "b"), "Model"))


# ---------------------------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------------------------
def test_sampling_on_the_fixture(dev, gold, tmp_path, monkeypatch, capsys):
    import model
    import shapeDataset
    import shape_trainer
    from PIL import Image
    cfg = _cfg(monkeypatch, 2, flag=False)
    ckpt = os.path.join(str(tmp_path), "netG_epoch_0.pth")
    net = so.seeded_state_(model.SHP_G_NET(NBF), so.SEEDS["G"])
    torch.save(net.state_dict(), ckpt)
    monkeypatch.setitem(cfg.TRAIN, "NET_G", ckpt)
    ds = _fixture()
    loader = torch.utils.data.DataLoader(ds, batch_size=2, drop_last=True, shuffle=False)
    t = shape_trainer.condGANTrainer(str(tmp_path / "unused"), loader, ds, device=dev)
    assert not os.path.exists(str(tmp_path / "unused"))
    g = torch.Generator().manual_seed(43)
    noise = [torch.randn(2, 10, 4 * NBF, generator=g), torch.from_numpy(gold["sampling_noise"])]
    assert list(gold["sampling_keys"]) == ds.filenames[2:4]              # the golden's batch is this loader's second

    def word(i, r):
        return ds.ixtoword[ds.cats_dict[int(ds.insanns_dict[ds.filenames[i]]["rois"][r, 4])][0]]

    written, skipped = t.sampling("test", noise=noise)
    text = capsys.readouterr().out
    single = os.path.join(str(tmp_path), "netG_epoch_0", "valid", "single")
    names = ["tinytest_00_%s.png" % word(0, 0), "tinytest_02_%s.png" % word(2, 0), "tinytest_03_%s.png" % word(3, 0)]
    assert sorted(os.listdir(single)) == names and (written, skipped) == (3, 1)
    assert "1 images without a box skipped" in text
    assert names[1:] == list(gold["sampling_files"])
    got = np.stack([np.array(Image.open(os.path.join(single, n))) for n in names])
    assert got.shape == (3, 64, 64, 3) and got.dtype == np.uint8
    # the masks this test computes itself, batch by batch as the loader cuts them
    net = net.to(dev).eval()
    own = []
    for step, idx in enumerate(((0, 1), (2, 3))):
        batch = shapeDataset.prepare_data(torch.utils.data.default_collate([ds[i] for i in idx]), dev, NBF)
        with torch.no_grad():
            own.append(net(noise[step].to(dev)[:, :batch["max_num_roi"]], batch["bbox_maps_fwd"], batch["bbox_maps_bwd"],
                           batch["bbox_fmaps"]).cpu())
    assert np.array_equal(got[0], SSH.mask_rgb(own[0][0, 0].numpy())[0])
    assert np.array_equal(got[1:], SSH.mask_rgb(own[1][:, 0, 0].numpy()))
    # ... and what the unmodified reference wrote for the batch the golden covers
    diff = np.abs(got[1:].astype(np.int16) - gold["sampling_pixels"].astype(np.int16))
    print("sampling vs the reference's PNG pixels: %d of %d bytes differ, largest difference %d; masks rel-L2 %.3g"
          % (int((diff != 0).sum()), diff.size, int(diff.max()),
             float(np.linalg.norm(own[1][:, 0, 0].numpy() - gold["sampling_masks"]) / np.linalg.norm(gold["sampling_masks"]))))
    assert np.array_equal(got[1:], gold["sampling_pixels"])

    # every box: one file per box, the ten-box image gives ten
    written, skipped = t.sampling("test", noise=noise, all_boxes=True)
    capsys.readouterr()
    files = sorted(os.listdir(single))
    per_box = [f for f in files if f not in names]
    assert (written, skipped) == (13, 1) and len(per_box) == 13
    assert len([f for f in per_box if f.startswith("tinytest_02_")]) == 10
    assert "tinytest_02_9_%s.png" % word(2, 9) in per_box and "tinytest_03_1_%s.png" % word(3, 1) in per_box
    assert np.array_equal(np.array(Image.open(os.path.join(single, "tinytest_02_0_%s.png" % word(2, 0)))), got[1])
    want = SSH.mask_rgb(own[1][0, :, 0].numpy())
    for r in range(10):
        assert np.array_equal(np.array(Image.open(os.path.join(single, "tinytest_02_%d_%s.png" % (r, word(2, r))))), want[r]), r

"""The shape generator's pictures without a GPU: the host restatement (tests/shape_snapshot_helpers.py) against what the
unmodified reference drew (tests/golden/shape_snapshot_ref.npz), the command line's sampling branch and its refusals,
the C-ABI of the new entry, the fixture's images, the notice of a data directory without images."""
import io
import os

import numpy as np
import pytest
import torch

import shape_snapshot_helpers as SSH
import snapshot_helpers as SH
from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", "shape_snapshot_ref.npz")
TINY = os.path.join(ROOT, "tests", "golden", "shape_tiny")
FIXTURE = os.path.join(ROOT, "tests", "golden", "shape_tiny_test")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("form", ["norm", "raw"])
@pytest.mark.parametrize("name", list(SSH.GRID_CASES))
def test_helper_equals_the_reference_grids_below_the_strip(gold, name, form):
    B, S, R = SSH.GRID_CASES[name]
    case = SSH.grid_case(name)
    assert np.array_equal(case["imgs"].numpy(), gold[name + "_imgs"]) and np.array_equal(case["maps"].numpy(), gold[name + "_maps"])
    ref = gold["%s_%s_grid" % (name, form)]
    got = SSH.grid(case["imgs"], case["maps"], SH.plain_strip(8, S, 10, SSH.FONT_MAX), form)
    assert got.shape == ref.shape == (8 * (SSH.FONT_MAX + 2 * S), 12 * (S + 2), 3)
    assert np.array_equal(SSH.below_strip(got, 8, S), SSH.below_strip(ref, 8, S))
    assert np.array_equal(got, ref)            # (the captions of the recorded cases are empty: the strip is plain too)


def test_what_the_reference_drew_for_constant_panels(gold):
    """the recorded grids hold the cases the kernels define: zero slots and a constant panel are 0 in the normalised
    form, the constant 0.25 panel is trunc(0.25 * 255) = 63 in the raw form"""
    S, fm = 8, SSH.FONT_MAX

    def panel(grid, n, j):
        y, x = n * (fm + 2 * S) + fm, (j + 1) * (S + 2)
        return grid[y:y + S, x:x + S]
    norm, raw = gold["s8r3_norm_grid"], gold["s8r3_raw_grid"]
    for n, j in ((1, 3), (2, 3), (0, 2)):                      # panel j shows map j - 1
        assert not panel(norm, n, j).any(), (n, j)
    assert not panel(raw, 1, 3).any() and not panel(raw, 2, 3).any()
    assert (panel(raw, 0, 2) == 63).all()
    assert panel(norm, 0, 1).max() == 255 and panel(norm, 0, 1).min() == 0
    # R = 10 fills max_word_num + 1 panels, R = 1 leaves all but two empty
    assert panel(gold["s8r10_raw_grid"], 0, 10).any() and not panel(gold["s8r1_raw_grid"], 0, 3).any()
    assert not panel(gold["s8r1_norm_grid"], 1, 1).any() and not panel(gold["s8r1_norm_grid"], 1, 2).any()


def test_helper_mask_dump_equals_the_reference_png_pixels(gold):
    assert np.array_equal(SSH.mask_rgb(gold["sampling_masks"]), gold["sampling_pixels"])
    assert gold["sampling_pixels"].min() == 0 and gold["sampling_pixels"].max() == 255
    tiny = np.zeros((5, 7), np.float32)
    tiny[2, 3] = 1e-40                                          # a denormal: numpy keeps it
    out = SSH.mask_rgb(np.stack([np.full((5, 7), 0.3, np.float32), tiny]))
    assert not out[0].any() and out[1][2, 3].tolist() == [255] * 3 and int(out[1].astype(int).sum()) == 3 * 255


def test_command_line_sampling_refusals(capsys, tmp_path):
    import shape_main
    with pytest.raises(SystemExit) as e:
        shape_main.main(["--data_dir", FIXTURE])
    assert isinstance(e.value.code, str) and "\n" not in e.value.code
    assert "--FLAG" in e.value.code and "--NET_G" in e.value.code
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        shape_main.main(["--NET_G", str(tmp_path / "netG_epoch_9.pth"), "--data_dir", FIXTURE])
    assert e.value.code == 2
    out = capsys.readouterr()
    assert out.out == "" and len(out.err.strip().splitlines()) == 1 and "netG_epoch_9.pth" in out.err


def test_command_line_options():
    import shape_main
    a = shape_main.parse_args(["--FLAG"])
    assert a.DISPLAY_INTERVAL == 5 and a.ALL_BOXES is False
    a = shape_main.parse_args(["--NET_G", "x.pth", "--ALL_BOXES", "--DISPLAY_INTERVAL", "0"])
    assert a.DISPLAY_INTERVAL == 0 and a.ALL_BOXES is True and not a.FLAG
    from miscc.config import cfg
    assert cfg.TRAIN.DISPLAY_INTERVAL == 500                  # the config default is not the command line's


def test_c_abi_has_the_mask_dump():
    from objgan_hip import _lib
    header = open(os.path.join(ROOT, "include", "objgan_hip.h")).read()
    assert "int objgan_mask_to_rgb8(const float* masks, const int* sel, unsigned char* out, int N, int HW, void* stream);" in header
    assert len(_lib.SIGNATURES["objgan_mask_to_rgb8"]) == 6
    assert getattr(_lib.load(build_if_missing=False), "objgan_mask_to_rgb8") is not None


def test_snapshot_grid_names_its_norms():
    from objgan_hip import ops
    assert ops.SNAPSHOT_NORMS == {"global": 0, "panel": 1, "raw": 2, "panel_unguarded": 3}


def test_images_for_reads_the_bigfile_like_the_reference_loader():
    import shapeDataset
    from miscc import load
    from PIL import Image
    ds = shapeDataset.TextDataset(FIXTURE, "test", base_size=64)
    assert [int(ds.insanns_dict[k]["num_rois"]) for k in ds.filenames] == [1, 0, 10, 2, 3]
    assert ds.has_images() and ds._img_bytes is None                 # opened at the first call
    keys = [ds.filenames[i] for i in (3, 0, 4)]
    got = ds.images_for(keys)
    assert got.shape == (3, 3, 64, 64) and got.dtype == torch.float32
    assert float(got.min()) >= -1.0 and float(got.max()) <= 1.0 and float(got.std()) > 0.1
    big = load.load_imgs_data(FIXTURE, "test", ds.filenames)
    for k, t in zip(keys, got):
        raw = big[ds.filenames.index(k)]
        assert torch.equal(t, load.get_imgs(raw, [64, 64, 64])[0])
        # Pillow resize, ToTensor, Normalize(0.5, 0.5) written out
        img = Image.open(io.BytesIO(raw)).convert("RGB").resize((64, 64), Image.BILINEAR)
        want = (torch.from_numpy(np.asarray(img).transpose(2, 0, 1).copy()).float() / 255 - 0.5) / 0.5
        assert torch.equal(t, want)
    # an item is what it was: ten entries, no image
    assert len(ds[2]) == 10 and ds[2][7] == 10
    train = shapeDataset.TextDataset(TINY, "train", base_size=64)
    assert not train.has_images()
    with pytest.raises(IOError):
        train.images_for(train.filenames[:1])
    assert not os.path.exists(os.path.join(TINY, "train_imgs.bigfile"))           # never written from here


def test_training_without_an_image_file_says_so_once_and_draws_nothing(capsys, tmp_path, monkeypatch):
    import shapeDataset
    import shape_trainer
    from miscc.config import cfg
    monkeypatch.setitem(cfg.TRAIN, "FLAG", True)
    monkeypatch.setitem(cfg.TRAIN, "DISPLAY_INTERVAL", 1)
    t = shape_trainer.condGANTrainer(str(tmp_path), None, shapeDataset.TextDataset(TINY, "train", base_size=64), device="cpu")
    assert os.path.isdir(os.path.join(str(tmp_path), "Image"))
    capsys.readouterr()
    assert t.display_ready() is False
    text = capsys.readouterr().out
    assert len(text.strip().splitlines()) == 1 and "train_imgs.bigfile" in text and "without" in text
    monkeypatch.setitem(cfg.TRAIN, "DISPLAY_INTERVAL", 0)
    t = shape_trainer.condGANTrainer(str(tmp_path), None, shapeDataset.TextDataset(FIXTURE, "test", base_size=64), device="cpu")
    assert t.display_ready() is False and capsys.readouterr().out == ""           # switched off: nothing to say

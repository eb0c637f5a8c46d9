"""JPEG encode on the device (csrc/jpeg_enc.hip through ops.jpeg_encode) against Pillow itself, the encoder of the
reference's save_singleimages (evaluator.py:225-233): BYTE-EXACT files for the case list of tests/jpeg_encode_model.py
(whose coverage of the entropy stage's hazards tests/test_jpeg_encode_cpu.py asserts), in batches and alone, from uint8
and from the generator's fp32 output, decoded again by the device decoder, and through save_singleimages.  Tolerance: none."""
import os
import types

import numpy as np
import pytest
import torch

import jpeg_encode_model as M
from conftest import note

pytestmark = pytest.mark.gpu


def _parent_loop(image_dir, images, keys, sent_ids):
    """save_singleimages as it was before the device path (reference evaluator.py:225-233), on whatever device"""
    from PIL import Image
    for i in range(images.size(0)):
        img = images[i].add(1).div(2).mul(255).clamp(0, 255).byte()
        ndarr = img.permute(1, 2, 0).cpu().numpy()
        Image.fromarray(ndarr).save('%s/%s_%d.jpg' % (image_dir, keys[i], sent_ids[i]))


def _read_all(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_device_jpeg_encode_writes_pillows_bytes(dev):
    from objgan_hip import ops
    cases = M.cases(big=True)
    assert {rgb.shape[:2] for _, rgb, _ in cases} == {(16, 16), (16, 32), (48, 16), (64, 64), (256, 256)}
    groups = {}
    for name, rgb, q in cases:
        groups.setdefault((rgb.shape[:2], q), []).append((name, rgb))
    assert len(groups) == 25
    bad, count = [], 0
    for ((H, W), q), members in groups.items():
        batch = torch.from_numpy(np.stack([rgb for _, rgb in members])).to(dev)
        files = ops.jpeg_encode(batch, quality=q)
        assert len(files) == len(members) and all(isinstance(f, bytes) for f in files)
        for (name, rgb), data in zip(members, files):
            count += 1
            if data != M.pillow(rgb, q):
                bad.append(name)
    assert not bad, (len(bad), bad[:8])
    note("device JPEG encode vs Pillow: %d images (16x16 .. 256x256, qualities 75 1 30 95 100)" % count, "byte-exact")


def test_device_jpeg_encode_batches(dev):
    from objgan_hip import ops
    pool = [rgb for name, rgb, q in M.cases() if rgb.shape[:2] == (64, 64) and q == 75]
    rng = np.random.default_rng(7)
    pool = pool + [rng.integers(0, 256, (64, 64, 3), dtype=np.uint8) for _ in range(16 - len(pool))]
    alone = [ops.jpeg_encode(torch.from_numpy(rgb[None]).to(dev))[0] for rgb in pool]
    assert alone == [M.pillow(rgb) for rgb in pool]
    for n in (1, 3, 16):
        batch = torch.from_numpy(np.stack(pool[:n])).to(dev)
        first, second = ops.jpeg_encode(batch), ops.jpeg_encode(batch)
        assert first == alone[:n], n
        assert second == first, n
    # a batch of full-size images, the other orientation of the mix: strides between images at 1 536 blocks each
    big = [M._content(kind, 256, 256, np.random.default_rng(3)) for kind in ("smooth", "noise", "primaries")]
    files = ops.jpeg_encode(torch.from_numpy(np.stack(big)).to(dev), quality=95)
    assert files == [M.pillow(rgb, 95) for rgb in big]


def _fp32_batch(n, H, W, seed):
    """generator-like fp32 [n, 3, H, W] with -1, 1, values outside [-1, 1] and values whose (x + 1) / 2 * 255 lies within
    a few ulps of an integer on either side"""
    g = torch.Generator().manual_seed(seed)
    x = torch.tanh(torch.randn(n, 3, H, W, generator=g) * 1.5) * 1.2
    flat = x.view(-1)
    k = torch.arange(256, dtype=torch.float64)
    edge = (k * 2 / 255 - 1).to(torch.float32)
    near = [edge]
    for direction in (2.0, -2.0):
        e = edge
        for _ in range(3):
            e = torch.nextafter(e, torch.full_like(e, direction))
            near.append(e)
    near = torch.cat(near + [torch.tensor([-1.0, 1.0, -1.5, 1.5, -0.0, 0.0, 1.0000001, -1.0000001])])
    assert near.numel() <= flat.numel() // 2
    pos = torch.randperm(flat.numel(), generator=g)[:near.numel()]
    flat[pos] = near
    return x


def test_device_jpeg_encode_fp32_form_is_the_host_loops(dev, tmp_path):
    from objgan_hip import ops
    for n, H, W in ((2, 32, 48), (3, 64, 64), (1, 256, 256)):
        x = _fp32_batch(n, H, W, seed=H + W).to(dev)
        d = str(tmp_path / ("%dx%d" % (H, W)))
        os.makedirs(d)
        keys, ids = ["k%d" % i for i in range(n)], list(range(n))
        _parent_loop(d, x, keys, ids)
        want = [open("%s/%s_%d.jpg" % (d, k, i), "rb").read() for k, i in zip(keys, ids)]
        assert ops.jpeg_encode(x) == want, (n, H, W)
        # a non-contiguous view of the same values
        assert ops.jpeg_encode(x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)) == want, (n, H, W)
        # and the bytes the model makes of the host's conversion
        assert want == [M.encode(M.to_bytes_host(x[i].cpu().numpy()))[0] for i in range(n)]


def test_device_jpeg_encode_and_decode_meet(dev):
    import io
    from PIL import Image
    from objgan_hip import ops
    rgbs = [rgb for name, rgb, q in M.cases() if rgb.shape[:2] == (48, 16) and q == 95]
    files = ops.jpeg_encode(torch.from_numpy(np.stack(rgbs)).to(dev), quality=95)
    decoded = ops.jpeg_decode(files, dev)
    for f, got in zip(files, decoded):
        assert np.array_equal(got.cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)).convert("RGB")))


def test_save_singleimages_on_device_tensors(dev, tmp_path):
    from evaluator import condGANEvaluator
    x = _fp32_batch(4, 64, 64, seed=11).to(dev)
    keys, ids = ["COCO_a", "COCO_b", "c", "d"], [0, 2, 1, 0]
    dirs = {}
    for sub, kwargs in (("device", {}), ("host", {"device_jpeg": False})):
        dirs[sub] = str(tmp_path / sub)
        os.makedirs(dirs[sub])
        condGANEvaluator.save_singleimages(types.SimpleNamespace(image_dir=dirs[sub]), x, keys, ids, **kwargs)
    os.makedirs(str(tmp_path / "want"))
    _parent_loop(str(tmp_path / "want"), x, keys, ids)
    want = _read_all(str(tmp_path / "want"))
    assert sorted(want) == ["COCO_a_0.jpg", "COCO_b_2.jpg", "c_1.jpg", "d_0.jpg"]
    assert _read_all(dirs["device"]) == want and _read_all(dirs["host"]) == want
    # an odd size takes the host route and still writes Pillow's files
    odd = _fp32_batch(2, 24, 40, seed=12).to(dev)
    for sub in ("odd", "odd_want"):
        os.makedirs(str(tmp_path / sub))
    condGANEvaluator.save_singleimages(types.SimpleNamespace(image_dir=str(tmp_path / "odd")), odd, keys[:2], ids[:2])
    _parent_loop(str(tmp_path / "odd_want"), odd, keys[:2], ids[:2])
    assert _read_all(str(tmp_path / "odd")) == _read_all(str(tmp_path / "odd_want"))
    assert len(_read_all(str(tmp_path / "odd"))) == 2

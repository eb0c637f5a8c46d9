"""JPEG encode without a GPU: the numpy model of tests/jpeg_encode_model.py -- the specification the device encoder
(csrc/jpeg_enc.hip) is held to -- against the installed Pillow, byte for byte; that the case list the GPU test shares
contains every hazard of the entropy stage; the C-ABI declarations and the host-only entry points (header, plan,
refusals); and that save_singleimages on CPU tensors still writes what the reference's loop writes."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import jpeg_encode_model as M


@pytest.fixture(scope="module")
def encoded():
    """[(name, rgb, quality, model bytes, census)] of the small case list, computed once"""
    return [(name, rgb, q) + M.encode(rgb, q) for name, rgb, q in M.cases(big=False)]


def test_model_writes_pillows_bytes(encoded):
    assert len(encoded) == len(M.SIZES) * len(M.QUALITIES) * len(M.CONTENTS)
    bad = [name for name, rgb, q, data, _ in encoded if data != M.pillow(rgb, q)]
    assert not bad, bad[:8]
    # Pillow's save(path) without arguments is quality 75: the file save_singleimages writes
    name, rgb, q, data, _ = encoded[0]
    assert q == 75
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG")
    assert buf.getvalue() == data


def test_case_list_covers_every_hazard(encoded):
    assert all(max(rgb.shape[:2]) <= 64 for _, rgb, _, _, _ in encoded)
    census = [c for _, _, _, _, c in encoded]
    assert any(c["zrl"] > 0 for c in census), "no ZRL symbol (run > 15)"
    assert any(c["no_eob"] > 0 for c in census), "no block without EOB"
    assert any(c["eob_only"] > 0 for c in census), "no EOB-only block"
    dc = set().union(*(c["dc_cats"] for c in census))
    ac = set().union(*(c["ac_cats"] for c in census))
    assert 0 in dc and 11 in dc, sorted(dc)
    assert 10 in ac, sorted(ac)
    assert any(c["stuffed"] > 0 for c in census), "no stuffed FF"
    assert {c["pad_bits"] for c in census} == set(range(8)), sorted({c["pad_bits"] for c in census})
    assert any(c["last_byte_ff_padded"] for c in census), "no stream whose padded last byte is FF"


def test_entry_points_are_declared_and_bound():
    from objgan_hip import _lib, build, ops
    text = open(build.HEADER).read()
    for name in ("objgan_jpeg_enc_header", "objgan_jpeg_enc_plan", "objgan_jpeg_encode", "objgan_jpeg_enc_header_bytes"):
        assert name + "(" in text, name
    assert {"objgan_jpeg_enc_header", "objgan_jpeg_encode"} <= set(_lib.SIGNATURES)
    assert {"objgan_jpeg_enc_plan", "objgan_jpeg_enc_header_bytes"} <= set(_lib.LONG_RETURN)
    assert callable(ops.jpeg_encode)
    assert build.PER_FILE_FLAGS["jpeg_enc.hip"] == ["-ffp-contract=off"]
    assert "jpeg_enc.hip" in build.sources()


def test_host_header_is_the_models_and_the_plan_is_the_derived_bound():
    from objgan_hip import _lib
    lib = _lib.load()
    nb = int(lib.objgan_jpeg_enc_header_bytes())
    assert nb == M.HEADER_BYTES == 623
    for (H, W), q in [((16, 16), 75), ((16, 32), 1), ((48, 16), 30), ((64, 64), 95), ((256, 256), 100), ((4096, 272), 50)]:
        buf = (ctypes.c_ubyte * nb)()
        _lib.call("objgan_jpeg_enc_header", H, W, q, buf)
        assert bytes(buf) == M.header(H, W, q), (H, W, q)
    # slot: header + twice the raw bytes of blocks * 1660 bits (22 DC + 63 * 26 AC, all stuffed) + EOI, rounded to 16
    slot = ctypes.c_long(0)
    ws = lib.objgan_jpeg_enc_plan(16, 256, 256, 75, 1, ctypes.byref(slot))
    blocks = 256 * 6
    raw = (blocks * 1660 + 7) // 8
    assert slot.value == (623 + 2 * raw + 2 + 15) // 16 * 16
    assert ws >= 16 * (blocks * 128 + raw)
    # the longest code strings the tables allow, from the tables themselves
    sizes = {k: M._derive(*t)[1] for k, t in (("dl", M.DC_LUMA), ("dc", M.DC_CHROMA), ("al", M.AC_LUMA), ("ac", M.AC_CHROMA))}
    dc_max = max(int(sizes[k][c]) + c for k in ("dl", "dc") for c in range(12))
    ac_max = max(int(sizes[k][s]) + (s & 15) for k in ("al", "ac") for s in range(256) if sizes[k][s] and (s & 15) <= 10)
    assert dc_max + 63 * ac_max == 1660


def test_refusals_name_their_reason_and_launch_nothing(monkeypatch):
    from objgan_hip import _lib, ops

    def no_launch(name, *args):
        raise AssertionError("launched " + name)
    monkeypatch.setattr(_lib, "call", no_launch)
    u8 = lambda h, w: torch.zeros(2, h, w, 3, dtype=torch.uint8)                    # noqa: E731
    for images, quality, reason, word in [(u8(8, 16), 75, 2, "multiples of 16"), (u8(24, 16), 75, 2, "multiples of 16"),
                                          (torch.zeros(2, 3, 16, 24), 75, 2, "multiples of 16"),
                                          (u8(16, 16), 0, 4, "quality"), (u8(16, 16), 101, 4, "quality"),
                                          (torch.zeros(2, 16, 16, 3, dtype=torch.int16), 75, 5, "uint8"),
                                          (torch.zeros(2, 3, 16, 16, dtype=torch.float64), 75, 5, "uint8"),
                                          (torch.zeros(2, 1, 16, 16), 75, 5, "uint8"),
                                          (torch.zeros(0, 3, 16, 16), 75, 1, "empty")]:
        assert ops.jpeg_encode_refusal(images, quality) == reason
        with pytest.raises(ops.JpegEncodeRefused) as e:
            ops.jpeg_encode(images, quality)
        assert e.value.reason == reason and word in str(e.value), str(e.value)
        assert isinstance(e.value, _lib.ObjganHipError)
    # the C entry point itself refuses (0, nothing launched) what the plan refuses; the pointers are never touched
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    for H, W in ((8, 16), (24, 16)):
        assert lib.objgan_jpeg_encode(one, 0, 1, H, W, one, one, 1 << 20, one, one, 1 << 20, 3, None) == 0
    assert lib.objgan_jpeg_encode(one, 2, 1, 16, 16, one, one, 1 << 20, one, one, 1 << 20, 3, None) == 0
    assert lib.objgan_jpeg_encode(one, 0, 1, 16, 16, one, one, 16, one, one, 1 << 20, 3, None) == 0      # slot too small
    assert lib.objgan_jpeg_enc_plan(1, 16, 16, 0, 0, None) == -4 and lib.objgan_jpeg_enc_plan(1, 16, 16, 101, 0, None) == -4
    # a batch the device would take, on the CPU: no silent host fall-back inside the op
    monkeypatch.undo()
    with pytest.raises(_lib.ObjganHipError, match="needs a HIP device"):
        ops.jpeg_encode(u8(16, 16))


def _parent_loop(image_dir, images, keys, sent_ids):
    """save_singleimages as it was before the device path (reference evaluator.py:225-233)"""
    from PIL import Image
    for i in range(images.size(0)):
        img = images[i].add(1).div(2).mul(255).clamp(0, 255).byte()
        ndarr = img.permute(1, 2, 0).cpu().numpy()
        Image.fromarray(ndarr).save('%s/%s_%d.jpg' % (image_dir, keys[i], sent_ids[i]))


def test_save_singleimages_on_cpu_tensors_is_the_parents_loop(tmp_path):
    from evaluator import condGANEvaluator
    g = torch.Generator().manual_seed(5)
    images = (torch.rand(3, 3, 32, 48, generator=g) * 2.4 - 1.2)
    keys, sent_ids = ["a", "b", "c"], [0, 3, 1]
    for sub, kwargs in (("new", {}), ("off", {"device_jpeg": False})):
        os.makedirs(str(tmp_path / sub))
        condGANEvaluator.save_singleimages(types.SimpleNamespace(image_dir=str(tmp_path / sub)), images, keys, sent_ids, **kwargs)
    os.makedirs(str(tmp_path / "want"))
    _parent_loop(str(tmp_path / "want"), images, keys, sent_ids)
    names = sorted(os.listdir(str(tmp_path / "want")))
    assert names == ["a_0.jpg", "b_3.jpg", "c_1.jpg"]
    for sub in ("new", "off"):
        assert sorted(os.listdir(str(tmp_path / sub))) == names
        for n in names:
            assert (tmp_path / sub / n).read_bytes() == (tmp_path / "want" / n).read_bytes(), (sub, n)
    # the model's byte conversion is the loop's
    for i in range(3):
        assert (tmp_path / "want" / names[i]).read_bytes() == M.encode(M.to_bytes_host(images[i].numpy()))[0]

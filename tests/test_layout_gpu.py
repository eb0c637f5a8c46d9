"""The device layout stage (csrc/layout.hip, ops.layout_from_decode) and the caption-to-image pipeline built on it,
against the FILE ROUTE: Evaluator.postprocess -> write_layouts -> load_gen_insanns -> get_gen_rois -> the collate of
prepare_gen_data (tests/layout_cases.py runs it through a temporary directory).  Every comparison is bit for bit."""
import os
import types

import numpy as np
import pytest
import torch

import boxgen_oracle as BO
import layout_cases as LC
from eval_helpers import cfg_snapshot, cfg_restore

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in LC.cases()}


def _device_route(dev, case, th=None, l2c=None, c2r=None, T_pad=0, tie_rule=None):
    from objgan_hip import ops
    B = case["labels"].shape[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    labels, samples = case["labels"], case["samples"]
    if T_pad:
        labels = np.concatenate((labels, np.zeros((B, T_pad), labels.dtype)), 1)
        samples = np.concatenate((samples, np.zeros((B, T_pad, 4))), 1)
    return ops.layout_from_decode(t(labels), t(case["lengths"]), t(samples), t(case["mean_std"]),
                                  t(LC.label_to_cat() if l2c is None else l2c), t(LC.cat_to_rel() if c2r is None else c2r),
                                  t(LC.thresholds(B) if th is None else th), LC.IMSIZE, LC.FMSIZE, LC.R,
                                  min_size=LC.MIN_SIZE, tie_rule=tie_rule)


def _same_bits(got, want, what):
    got = got.cpu().numpy()
    want = np.asarray(want).astype(got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, np.argwhere(got != want)[:5].tolist())


def _compare(dev, got, want, what, C=len(LC.CATS_INDEX)):
    from objgan_hip import ops
    torch.cuda.synchronize()
    for k in ("boxes", "nbox", "fm_rois", "num_rois", "cats", "raw_maps", "raw_fmaps"):
        _same_bits(got[k], want[k], (what, k))
    assert len(got["rois"]) == len(LC.IMSIZE)
    for i in range(len(LC.IMSIZE)):
        _same_bits(got["rois"][i], want["rois"][i], (what, "rois", i))
    # the cut prepare_gen_data makes: the batch's largest count, float32
    n = int(want["num_rois"].max())
    if n > 0:
        fwd, bwd = ops.boxmaps_onehot(got["raw_maps"], got["cats"], got["num_rois"], n, C)
        _same_bits(fwd, want["bbox_maps_fwd"][:, :n].astype(np.float32), (what, "bbox_maps_fwd"))
        _same_bits(bwd, want["bbox_maps_bwd"][:, :n].astype(np.float32), (what, "bbox_maps_bwd"))
        _same_bits(got["raw_fmaps"][:, :n], want["bbox_fmaps"][:, :n].astype(np.float32), (what, "bbox_fmaps"))


@pytest.mark.parametrize("name", [n for n in CASES if n != "tied"])          # ("tied": the next test)
def test_layout_from_decode_matches_the_file_route(dev, tmp_path, name):
    case = CASES[name]
    want = LC.file_route(case, str(tmp_path))
    _compare(dev, _device_route(dev, case), want, name)


def test_tied_areas_match_the_file_route(dev, tmp_path):
    """More than R boxes with equal areas on both sides of the cut, against the file route as it runs on this host.
    Which boxes of a tie np.argsort(area)[::-1] keeps depends on numpy's sort: insertion (stable; the later box first
    after the reversal) in its generic code, its AVX-512 network for 64-bit keys where it dispatches that one (there this
    case keeps boxes [8, 10, 5, 15, 2, 1, 7, 11, 0, 9], the insertion rule [8, 10, 5, 15, 11, 7, 2, 1, 0, 14]).  The kernel
    has both orders; ops.argsort_tie_rule finds out which one the host's numpy follows."""
    from objgan_hip import ops
    assert ops.argsort_tie_rule() in (0, 1)
    case = CASES["tied"]
    want = LC.file_route(case, str(tmp_path))
    _compare(dev, _device_route(dev, case), want, "tied")


class _Numpy(object):
    """numpy with argsort replaced"""

    def __init__(self, argsort):
        self.argsort = argsort

    def __getattr__(self, k):
        return getattr(np, k)


def test_tied_areas_follow_the_insertion_rule(dev, tmp_path, monkeypatch):
    """tie_rule = 0 against the file route with load_gen_insanns's argsort made the stable one, whatever the host's is"""
    from miscc import load
    monkeypatch.setattr(load, "np", _Numpy(lambda a, *args, **kw: np.argsort(a, kind="stable")))
    for name in ("tied", "tied_random"):
        want = LC.file_route(CASES[name], str(tmp_path / name))
        if name == "tied":
            assert want["rois"][2][0, :, 2].tolist() == [50, 40, 30, 60, 12, 15, 24, 30, 20, 10]
        _compare(dev, _device_route(dev, CASES[name], tie_rule=0), want, name + ", stable argsort")


def test_unknown_tie_order_is_refused(dev, monkeypatch):
    """a host whose argsort follows neither rule: refused where a cut can happen, harmless where it cannot"""
    from objgan_hip import ObjganHipError, ops
    monkeypatch.setattr(ops, "_TIE_RULE", [None])
    with pytest.raises(ObjganHipError):
        _device_route(dev, CASES["tied"])
    _device_route(dev, CASES["filter"])                  # T = 8: at most 7 boxes, R = 10
    with pytest.raises(ObjganHipError):
        _device_route(dev, CASES["tied"], tie_rule=2)    # the entry point's own answer


def test_more_than_17_steps_are_refused(dev):
    from objgan_hip import ObjganHipError, _lib, ops
    case = CASES["many"]
    assert case["labels"].shape[1] == 17
    with pytest.raises(ObjganHipError):
        _device_route(dev, case, T_pad=1)
    # the entry point itself answers with its error code
    B, T, L, R = 1, 18, len(LC.WORDS), LC.R
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    i32, f64, f32 = torch.int32, torch.float64, torch.float32
    args = [z((B, T), i32), z((B,), i32), z((B, T, 4), f64), z((8,), f64), z((L,), i32), z((45,), i32), z((B, L), i32),
            z((B, T, 5), f64), z((B,), i32), z((3, B, R, 6), f64), z((B, R, 6), f64), z((B,), i32), z((B, R), i32),
            z((B, R, 64, 64), f32), z((B, R, 16, 16), f32), z((B, R, 8), i32)]
    rc = _lib.load().objgan_layout_from_decode(*[ops._p(a) for a in args], ops._iarr(LC.IMSIZE), 3, 16, R, 10, 0, B, T, L, 45,
                                               ops._stream())
    assert rc == 0


def test_decoder_fed_layouts_match_the_file_route(dev, tmp_path):
    """a small random decoder (H = 32, 7 labels, K = 2, B = 5, T = 10): real box_decode output through both routes"""
    from objgan_hip import ops
    from seq2seq.models import DecoderRNN
    H, K, B, T, seed = 32, 2, 5, 10, 9
    cats = (1, 2, 3)
    w2i, i2w = BO.label_vocabulary(cats)
    decoder = DecoderRNN(w2i, 0.3, -0.1, 0.2, 0.4, 1, 150, H, K, bidirectional=True)
    BO.seeded_fill_(decoder, seed, bias_shift={w2i["<eos>"]: 0.3, w2i["<pad>"]: -8.0, w2i["<sos>"]: -8.0, w2i["<unk>"]: -8.0})
    decoder.to(dev)
    g = torch.Generator().manual_seed(seed + 1)
    h0, c0 = torch.rand(B, H, generator=g) * 2 - 1, torch.rand(B, H, generator=g) * 2 - 1
    rs = np.random.RandomState(seed + 2)
    noise = np.concatenate((rs.random_sample((B, T, 1)), rs.standard_normal((B, T, 2)),
                            rs.random_sample((B, T, 1)), rs.standard_normal((B, T, 2))), 2)
    labels, lengths, samples = ops.box_decode(h0.to(dev), c0.to(dev), torch.from_numpy(noise).to(dev), decoder._weights(),
                                              (0.3, -0.1, 0.2, 0.4), decoder.l_sos_id, decoder.l_eos_id)
    mean_std = np.array((128.0, 60.0, 128.0, 60.0, 90.0, 40.0, 1.0, 0.35))
    case = {"name": "decoder", "labels": labels.cpu().numpy(), "lengths": lengths.cpu().numpy(),
            "samples": samples.cpu().numpy(), "mean_std": mean_std}
    lang = types.SimpleNamespace(index2word=i2w, word2index=w2i)
    gauss = {1: (2.0, 0.0), 2: (3.0, 0.0), 3: (1.0, 0.0)}
    cats_index = {1: 0, 2: 1, 3: 2}
    ev = LC.make_evaluator(mean_std, str(tmp_path), lang, gauss)
    want = LC.file_route(case, str(tmp_path), cats_index, ev)
    assert int(want["nbox"].sum()) > 0 and int(want["num_rois"].sum()) > 0
    ms, l2c, c2r = ev.layout_tables(cats_index, dev)
    th = torch.from_numpy(ev.draw_thresholds(np.random.RandomState(0), B)).to(dev)
    got = ops.layout_from_decode(labels, lengths, samples, ms, l2c, c2r, th, LC.IMSIZE, LC.FMSIZE, LC.R)
    _compare(dev, got, want, "decoder-fed", C=3)


# ---------------------------------------------------------------------------------------------
# TextToImage end to end
# ---------------------------------------------------------------------------------------------
CAPTIONS = ["A person rides a bicycle near the traffic light.", "Two people, and a dog!",
            "Big red car at night in the rain near a stop sign and a small person"]
GAUSS0 = {1: (3.0, 0.0), 2: (2.0, 0.0), 10: (2.4, 0.0), 13: (1.0, 0.0), 3: (3.0, 0.0)}


@pytest.fixture(scope="module")
def t2i(dev):
    import evaluator as E
    import model as M
    import pipeline
    from miscc import load
    from miscc.config import cfg
    from oracle import ref_harness as rh
    from seq2seq.dataset.prepare_dataset import read_mean_std
    from seq2seq.evaluator import Evaluator
    from seq2seq.util.checkpoint import Checkpoint
    saved = cfg_snapshot(cfg)
    cfg.TREE.BRANCH_NUM, cfg.TEST.USE_GT_BOX_SEG, cfg.TRAIN.BATCH_SIZE = 3, 2, 3
    data = os.path.join(BO.GOLDEN, "data_tiny_eval")
    ds = types.SimpleNamespace()
    _, _, ds.ixtoword, ds.wordtoix, ds.n_words = load.load_text_data(data, 'test', [], [])
    _, _, ds.glove_wordtoix, ds.glove_embed = load.load_glove_emb(data, 'test', [], [])
    ds.cat_labels, ds.cat_label_lens, ds.sorted_cat_label_indices = load.load_cat_label(data, ds.glove_wordtoix)
    ds.cats_dict, ds.cats_index_dict = load.load_cats(data, ds.wordtoix)
    ds.text_encoder = rh.seeded_state_(M.RNN_ENCODER(ds.n_words, nhidden=cfg.TEXT.EMBEDDING_DIM), 31)
    C = len(ds.cats_index_dict)
    imager = E.condGANEvaluator('', None, ds, device=dev)
    imager.text_encoder.to(dev).eval()
    imager.glove_emb.to(dev).eval()
    imager.netG = rh.seeded_state_(M.G_NET(C), 32).to(dev).eval()
    imager.netShpG = rh.seeded_state_(M.SHP_G_NET(C), 33).to(dev).eval()
    ckpt = Checkpoint.load(os.path.join(BO.TINY, "checkpoints", "tiny"))
    lang = types.SimpleNamespace(index2word=ckpt.label_index2word, word2index=ckpt.label_word2index)
    stats = read_mean_std(os.path.join(BO.TINY, "mean_std_test.txt"))
    layout = Evaluator(3, 10, '', None, lang, stats[0], stats[1], stats[2], stats[3], GAUSS0, '', 0)
    pipe = pipeline.TextToImage(BO.tiny_encoder().to(dev), ckpt.model.eval().to(dev), layout, ckpt.cap_word2index, imager,
                                ds.wordtoix, ds.glove_wordtoix, dev, batch_size=3)
    yield pipe
    cfg_restore(cfg, saved)


def _noise(t2i, seed):
    from miscc.config import cfg
    g = torch.Generator().manual_seed(seed)
    rs = np.random.RandomState(seed)
    B, T, C = len(CAPTIONS), 10, t2i.imager.num_classes
    box = np.concatenate((rs.random_sample((B, T, 1)), rs.standard_normal((B, T, 2)),
                          rs.random_sample((B, T, 1)), rs.standard_normal((B, T, 2))), 2)
    return {"box": torch.from_numpy(box), "img": torch.randn(B, cfg.GAN.Z_DIM, generator=g),
            "shp": torch.randn(B, cfg.ROI.BOXES_NUM, C * 4, generator=g)}, \
        torch.randn(B, cfg.GAN.CONDITION_DIM, generator=g)


def test_generate_matches_the_staged_route(dev, t2i, tmp_path):
    """TextToImage.generate on 3 captions with fixed noise (sigma = 0) against: boxes.txt written by Evaluator ->
    load_gen_insanns -> the collate and prepare_gen_data -> condGANEvaluator.sampling with the same noise"""
    import testDataset
    from miscc import load
    from miscc.config import cfg
    noise, eps = _noise(t2i, 5)
    im = t2i.imager
    im.netG.ca_net.fixed_eps = eps.to(dev)           # rows of the length-ordered batch, in both routes
    try:
        images, layouts, masks = t2i.generate(CAPTIONS, noise=noise)
        torch.cuda.synchronize()
        # ---- the staged route ----
        encoded = t2i.encode(CAPTIONS, notice=False)
        data_dir = str(tmp_path)
        keys = ["line%d" % i for i in range(len(CAPTIONS))]
        ev = t2i.layout
        ev.box_saving_folder, ev.expt_dir, ev.dev_cap_lang = os.path.join(data_dir, "gen_masks") + "/", data_dir, \
            types.SimpleNamespace(word2index=t2i.box_vocab)
        import pipeline
        with torch.no_grad():
            decoded, seqs = ev.decode(t2i.box_encoder, t2i.decoder, [[pipeline.tokenize(c)] for c in CAPTIONS],
                                      noise=noise["box"].numpy())
        assert seqs == [e[0] for e in encoded]
        staged_layouts = ev.write_layouts(decoded, keys)
        imsize, fmsize, cid = t2i.imsize, cfg.ROI.FM_SIZE, im.cats_index_dict
        anns = load.load_gen_insanns(data_dir, keys, 'test', imsize, fmsize, cid)
        W = cfg.TEXT.WORDS_NUM
        items = []
        for i, key in enumerate(keys):
            cap, glove = np.zeros((W, 1), np.int64), np.zeros((W, 1), np.int64)
            cap[:len(encoded[i][1]), 0], glove[:len(encoded[i][2]), 0] = encoded[i][1], encoded[i][2]
            imgs = [torch.zeros(3, s, s) for s in imsize]
            items.append((imgs, np.zeros(4), cap, glove, len(encoded[i][1]))
                         + tuple(load.get_gen_rois(anns[key], imsize, fmsize, cid, 0)) + (0, key, i))
        batch = testDataset.prepare_gen_data(torch.utils.data.default_collate(items), dev)
        (_, _, captions, glove_captions, cap_lens, fwd, bwd, fmaps, rois, fm_rois, num_rois, _, skeys, sent_ids) = batch
        order = [int(s) for s in sent_ids]
        from miscc.utils import _host
        with torch.no_grad():                           # evaluate() runs all of this without autograd
            words_embs, sent_emb = im.text_encoder(captions, cap_lens, int(_host(cap_lens).max()))
            gw = torch.nn.functional.embedding(glove_captions.reshape(-1), im.glove_emb.weight)
        num_words = words_embs.size(2)
        d = {"rois": rois, "fm_rois": fm_rois, "num_rois": num_rois, "bbox_maps_fwd": fwd, "bbox_maps_bwd": bwd,
             "bbox_fmaps": fmaps, "words_embs": words_embs, "sent_emb": sent_emb,
             "glove_words_embs": gw.view(glove_captions.size(0), glove_captions.size(1), -1)[:, :num_words].transpose(1, 2),
             "mask": (captions == 0)[:, :num_words]}
        out = im.sampling(d, t2i.clabels_emb, imsize, noise_img=noise["img"][order].to(dev),
                          noise_shp=noise["shp"][order].to(dev))
        torch.cuda.synchronize()
    finally:
        im.netG.ca_net.fixed_eps = None
    want = out["fake_imgs"][-1]
    nums = _host(num_rois).tolist()
    print("num_rois (length order):", nums, "order:", order)
    assert sum(nums) > 0, "no caption has a box: pick another noise seed"
    assert tuple(images.shape) == (3, 3, 256, 256) and bool(torch.isfinite(images).all())
    assert torch.equal(images[order], want)
    for pos, i in enumerate(order):
        rows = np.array([[x, y, w, h, int(l)] for x, y, w, h, l in staged_layouts[i]], np.float64).reshape(-1, 5)
        assert layouts[i].tobytes() == rows.tobytes()
        assert torch.equal(masks[i], out["raw_masks"][pos, :nums[pos]])
        with open(os.path.join(data_dir, "gen_masks", keys[i], "0", "boxes.txt")) as f:
            assert f.read() == pipeline.boxes_txt(layouts[i])


def test_generate_is_repeatable_with_a_seed(dev, t2i):
    a = t2i.generate(CAPTIONS, seed=11, notice=False)
    b = t2i.generate(CAPTIONS, seed=11, notice=False)
    c = t2i.generate(CAPTIONS, seed=12, notice=False)
    torch.cuda.synchronize()
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert not torch.equal(a[0], c[0])


def test_generate_refuses_a_caption_without_a_known_word(dev, t2i):
    with pytest.raises(ValueError, match="caption 2 "):
        t2i.generate(["a person", "xylophone zeppelin"])

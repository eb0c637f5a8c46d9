"""Box generator on the device: csrc/box_decode.hip and the c_n-returning encoder entry point against the reference's
recorded run (tests/golden/boxgen_ref.pt) and, at a small shape, against the restatement of tests/boxgen_oracle.py;
batch independence byte for byte; sample.py end to end into the image generator's data path."""
import os
import shutil

import numpy as np
import pytest
import torch

import boxgen_oracle as BO
from conftest import note, rel_l2
from eval_helpers import cfg_snapshot, cfg_restore

pytestmark = pytest.mark.gpu

OPERATOR_BOUND = 1e-4           # the project's operator bound


def _decode(decoder, h0, c0, noise, cpw=None):
    from objgan_hip import ops
    out = ops.box_decode(h0, c0, noise, decoder._weights(), (decoder.x_mean, decoder.y_mean, decoder.w_mean,
                                                             decoder.r_mean), decoder.l_sos_id, decoder.l_eos_id,
                         trace=True, cpw=cpw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _check_against(got, want, lengths, what):
    """labels / lengths exact, samples and trace within the operator bound per caption trajectory, zero past the end"""
    labels, lens, samples, trace = got
    assert np.array_equal(lens, lengths), what
    assert np.array_equal(labels, want["labels"]), what
    worst_s = worst_t = 0.0
    for b, n in enumerate(lengths):
        assert not labels[b, n:].any() and not samples[b, n:].any() and not trace[b, n:].any(), (what, b)
        worst_s = max(worst_s, BO.trajectory_error(samples[b], want["samples"][b]))
        worst_t = max(worst_t, BO.trajectory_error(trace[b], want["trace"][b]))
    assert np.isfinite(samples).all() and np.isfinite(trace).all()
    note("boxgen %s: samples, worst trajectory error" % what, "%.3g" % worst_s)
    note("boxgen %s: trace, worst trajectory error" % what, "%.3g" % worst_t)
    print("%s: samples %.3g trace %.3g" % (what, worst_s, worst_t))
    assert worst_s <= OPERATOR_BOUND and worst_t <= OPERATOR_BOUND, (what, worst_s, worst_t)


@pytest.fixture(scope="module")
def real(dev):
    g = BO.load_golden()["real"]
    encoder, decoder, w2i = BO.real_modules()
    return g["config"], BO.stack_golden(g["captions"], g["config"]["T"]), encoder.to(dev), decoder.to(dev)


def test_real_shape_matches_reference(dev, real):
    """H = 256, 83 labels, K = 5, T = 10, the golden's captions in one batch: encoder state, then the decode from it"""
    from objgan_hip import ops
    c, s, encoder, decoder = real
    ids = s["ids"].to(dev)
    out, (hn, cn) = encoder(ids, s["lens"])
    B = ids.shape[0]
    hn_cat, cn_cat = (t.transpose(0, 1).reshape(B, -1) for t in (hn, cn))
    for name, got, want in (("h_n", hn_cat, s["hn"]), ("c_n", cn_cat, s["cn"])):
        e = rel_l2(got, want)
        note("boxgen encoder %s rel-L2" % name, "%.3g" % e)
        assert e <= OPERATOR_BOUND, (name, e)
    # the existing entry point on the same inputs: same bits
    lens = torch.tensor(s["lens"], dtype=torch.int32)
    old_out, old_hn = ops.lstm_bidir_forward(encoder.encoder.weight.detach(), ids, lens, *encoder._weights(), ids.shape[1])
    assert torch.equal(old_out.transpose(1, 2), out) and torch.equal(old_hn, hn_cat)
    assert torch.equal(out[0, s["lens"][0]:], torch.zeros_like(out[0, s["lens"][0]:]))
    got = _decode(decoder, hn_cat.contiguous(), cn_cat.contiguous(), torch.from_numpy(s["noise"]).to(dev))
    _check_against(got, s, s["lengths"], "real shape")
    # the module's forward returns the same, per caption
    soft, xy_par, wh_par, _, other = decoder((hn, cn), None, is_training=0, early_stop_len=c["T"], noise=s["noise"],
                                             trace=True)
    assert other["length"] == s["lengths"].tolist()
    for b, n in enumerate(s["lengths"]):
        assert other["sequence"][b].tolist() == s["labels"][b, :n].tolist()
        assert np.array_equal(np.array(other["xy"][b]), got[2][b, :n, :2])
        assert np.array_equal(np.array(other["wh"][b]), got[2][b, :n, 2:])
    assert torch.equal(torch.cat((soft, xy_par, wh_par), 2).cpu(), torch.from_numpy(got[3]))


def test_batch_independence_is_bit_exact(dev, real):
    """a caption alone, in a full tile, in the tile after a full one and at several places of B = 13, and with other
    tile sizes: the same bytes in all four outputs"""
    from objgan_hip import ops
    c, s, _, decoder = real
    cpw = ops.box_decode_cpw()
    h, cc, nz = s["hn"].to(dev), s["cn"].to(dev), torch.from_numpy(s["noise"]).to(dev)
    n_all = h.shape[0]
    picks = [int(np.argmax(s["lengths"] == 1)), int(np.argmax((s["lengths"] > 1) & (s["lengths"] < c["T"]))),
             int(np.argmax(s["lengths"] == c["T"]))]
    for i in picks:
        alone = _decode(decoder, h[i:i + 1], cc[i:i + 1], nz[i:i + 1])
        assert alone[1][0] == s["lengths"][i]
        others = [k for k in range(n_all) if k != i]
        layouts = [(cpw, cpw - 1, None), (cpw, 0, None), (cpw + 1, cpw, None), (13, 0, None), (13, 6, None),
                   (13, 12, None), (13, 5, 1), (13, 5, 2), (1, 0, 1)]
        for B, pos, tile in layouts:
            rows = (others * 2)[:B - 1]
            rows.insert(pos, i)
            idx = torch.tensor(rows, device=dev)
            got = _decode(decoder, h[idx], cc[idx], nz[idx], cpw=tile)
            for a, g in zip(alone, got):
                assert a[0].tobytes() == g[pos].tobytes(), (i, B, pos, tile)


@pytest.mark.parametrize("T", [1, 3])
def test_small_shape_matches_restatement(dev, T):
    """H = 32, 7 labels, K = 2, B = 5 (two workgroups, the second one partly empty) against the CPU restatement;
    captions whose label or component choice the restatement finds within the margins are left out (at most 1 in 4)"""
    from seq2seq.models import DecoderRNN
    H, K, B, seed = 32, 2, 5, 9
    w2i, _ = BO.label_vocabulary((1, 2, 3))
    decoder = DecoderRNN(w2i, 0.3, -0.1, 0.2, 0.4, 1, 150, H, K, bidirectional=True)
    BO.seeded_fill_(decoder, seed, bias_shift={w2i["<eos>"]: 0.3})
    g = torch.Generator().manual_seed(seed + 1)
    h0, c0 = torch.rand(B, H, generator=g) * 2 - 1, torch.rand(B, H, generator=g) * 2 - 1
    rs = np.random.RandomState(seed + 2)
    noise = np.concatenate((rs.random_sample((B, T, 1)), rs.standard_normal((B, T, 2)),
                            rs.random_sample((B, T, 1)), rs.standard_normal((B, T, 2))), 2)
    labels, lengths, samples, trace, lm, em = BO.decode_ref(decoder.state_dict(), h0, c0, noise, (0.3, -0.1, 0.2, 0.4),
                                                            w2i["<sos>"], w2i["<eos>"], K)
    keep = np.nonzero(BO.margins_ok(lm, em))[0]
    assert len(keep) >= B - B // 4, "the restatement alone must leave at most 1 caption in 4 out: pick another seed"
    decoder.to(dev)
    got = _decode(decoder, h0.to(dev), c0.to(dev), torch.from_numpy(noise).to(dev))
    want = {"labels": labels[keep], "samples": samples[keep], "trace": trace[keep]}
    _check_against([a[keep] for a in got], want, lengths[keep], "small shape T=%d" % T)
    if T == 3:
        assert len(set(lengths[keep].tolist())) > 1          # some captions end early, some do not


def test_sample_py_end_to_end(dev, tmp_path):
    """sample.py over the tiny input with fixed seeds: the reference's boxes.txt files to the last printed digit; the
    layouts then load through load_anns_data into TestDataset (generated-layout mode)"""
    import sample
    import testDataset
    from miscc.config import cfg
    t = BO.load_golden()["tiny"]
    data = os.path.join(str(tmp_path), "data")
    shutil.copytree(os.path.join(BO.GOLDEN, "data_tiny_eval"), data)
    os.remove(os.path.join(data, "test_gen_insanns.pickle"))
    encoder_path = os.path.join(str(tmp_path), "text_encoder")
    torch.save(BO.tiny_encoder().state_dict(), encoder_path)
    rc = sample.main(["--is_training", "0", "--dev_path", os.path.join(BO.TINY, "input_test.txt"),
                      "--dev_filename_path", os.path.join(BO.TINY, "filenames_test.txt"),
                      "--mean_std_path", os.path.join(BO.TINY, "mean_std_test.txt"),
                      "--gaussian_dict_path", os.path.join(BO.TINY, "gaussian_dict.npy"),
                      "--expt_dir", BO.TINY, "--load_checkpoint", "tiny",
                      "--encoder_path", encoder_path,
                      "--box_saving_folder", os.path.join(data, "gen_masks"), "--embedding_dim", str(t["config"]["H"]),
                      "--batch_size", "7", "--seed", str(t["config"]["seed"]), "--log-level", "warning"])
    assert rc == 0
    out, ref = os.path.join(data, "gen_masks_tiny"), os.path.join(BO.TINY, "gen_masks_ref")
    worst, n_boxes = 0.0, 0
    for key in sorted(set(t["keys"])):
        assert sorted(os.listdir(os.path.join(out, key))) == sorted(os.listdir(os.path.join(ref, key)))
        for index in os.listdir(os.path.join(ref, key)):
            got = open(os.path.join(out, key, index, "boxes.txt")).read().splitlines()
            want = open(os.path.join(ref, key, index, "boxes.txt")).read().splitlines()
            assert len(got) == len(want), (key, index)
            for a, b in zip(got, want):
                a, b = a.split(","), b.split(",")
                assert a[4:] == b[4:]
                worst = max(worst, max(abs(float(x) - float(y)) for x, y in zip(a[:4], b[:4])))
                n_boxes += 1
    note("boxgen sample.py: largest difference of a printed coordinate (%d boxes)" % n_boxes, "%.3g" % worst)
    assert n_boxes >= len(t["keys"]) and worst <= 0.01 + 1e-9
    os.rename(out, os.path.join(data, "gen_masks"))
    saved = cfg_snapshot(cfg)
    try:
        cfg.TREE.BRANCH_NUM, cfg.TEST.SAMPLE_VAL, cfg.TEST.USE_GT_BOX_SEG = 3, False, 2
        ds = testDataset.TestDataset(data, "test", base_size=64)
        assert os.path.isfile(os.path.join(data, "test_gen_insanns.pickle"))
        assert sorted(ds.insanns_gen_dict) == sorted(set(t["keys"]))
        assert all(sorted(v) == list(range(5)) for v in ds.insanns_gen_dict.values())
        assert sum(a["num_rois"] for v in ds.insanns_gen_dict.values() for a in v.values()) > 0
        item = ds[0]
        assert len(item) == 14 and int(item[10]) == ds.insanns_gen_dict[item[12]][item[13] % 5]["num_rois"]
    finally:
        cfg_restore(cfg, saved)

"""Box generator, host side (no GPU): the restatement of the decode against the reference's recorded run, the
post-processing, the layout reader, the checkpoint reader and the refusals.  The golden comes from
tests/golden/make_golden_boxgen.py (the unmodified reference on the CPU)."""
import filecmp
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

import boxgen_oracle as BO

RESTATEMENT_BOUND = 1e-5        # restatement against golden


def test_restatement_matches_reference_decode():
    """tests/boxgen_oracle.decode_ref (what the GPU tests use where the reference is absent) against the reference's
    run at the real shape: labels and lengths exact, samples and trace within 1e-5 of each trajectory's largest value."""
    g = BO.load_golden()["real"]
    c = g["config"]
    _, decoder, w2i = BO.real_modules()
    s = BO.stack_golden(g["captions"], c["T"])
    labels, lengths, samples, trace, lm, em = BO.decode_ref(decoder.state_dict(), s["hn"], s["cn"], s["noise"],
                                                            c["means"], w2i["<sos>"], w2i["<eos>"], c["K"])
    assert np.array_equal(lengths, s["lengths"]) and np.array_equal(labels, s["labels"])
    assert len(lengths) >= 12 and {1, c["T"]} <= set(lengths.tolist()) and len(set(lengths.tolist()) - {1, c["T"]}) >= 2
    worst = 0.0
    for b in range(len(lengths)):
        worst = max(worst, BO.trajectory_error(samples[b], s["samples"][b]), BO.trajectory_error(trace[b], s["trace"][b]))
    print("restatement vs reference: worst trajectory error %.3g" % worst)
    assert worst <= RESTATEMENT_BOUND
    assert BO.margins_ok(lm, em).all()
    assert np.allclose(lm, [k["label_margin"] for k in g["captions"]], rtol=1e-3, atol=1e-5)


def _tiny_evaluator(folder, batch_size=4):
    from seq2seq.dataset.prepare_dataset import prepare_test_data
    from seq2seq.evaluator import Evaluator
    t = BO.load_golden()["tiny"]
    w2i_cap, i2w_cap, w2i, i2w = t["vocabularies"]
    cap_lang, label_lang, tuples, xm, ym, wm, rm, keys = prepare_test_data(
        os.path.join(BO.TINY, "input_test.txt"), os.path.join(BO.TINY, "mean_std_test.txt"), 150, 1, w2i_cap, i2w_cap,
        w2i, i2w, os.path.join(BO.TINY, "filenames_test.txt"))
    gaussian = np.load(os.path.join(BO.TINY, "gaussian_dict.npy"), allow_pickle=True).item()
    ev = Evaluator(batch_size, t["config"]["T"], folder, cap_lang, label_lang, xm, ym, wm, rm, gaussian,
                   os.path.join(folder, "gen_masks_out") + "/", 0)
    return ev, tuples, keys


def _same_tree(a, b):
    cmp = filecmp.dircmp(a, b)
    assert not cmp.left_only and not cmp.right_only, (cmp.left_only, cmp.right_only)
    for name in cmp.common_files:
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), (a, name)
    for name in cmp.common_dirs:
        _same_tree(os.path.join(a, name), os.path.join(b, name))


def test_postprocessing_writes_the_reference_files(tmp_path):
    """the reference's raw samples and a seeded np.random through the product's evaluator: every boxes.txt is byte for
    byte what the reference's Evaluator.evaluate wrote; the readers find the recorded caption ids"""
    from seq2seq.dataset.prepare_dataset import indexes_from_sentence
    t = BO.load_golden()["tiny"]
    ev, tuples, keys = _tiny_evaluator(str(tmp_path))
    assert keys == t["keys"] and len(tuples) == len(keys)
    assert [indexes_from_sentence(ev.dev_cap_lang, it[0]) for it in tuples] == [c["ids"] for c in t["captions"]]
    decoded = [(c["labels"], [(s[0], s[1]) for s in c["samples"]], [(s[2], s[3]) for s in c["samples"]])
               for c in t["captions"]]
    np.random.seed(t["config"]["seed"])
    layouts = ev.write_layouts(decoded, keys)
    _same_tree(os.path.join(str(tmp_path), "gen_masks_out"), os.path.join(BO.TINY, "gen_masks_ref"))
    assert len(layouts) == len(keys) and sum(len(l) for l in layouts) >= len(keys)
    first = open(os.path.join(BO.TINY, "gen_masks_ref", keys[0], "0", "boxes.txt")).read().splitlines()
    assert ['%.2f,%.2f,%.2f,%.2f,%s,0' % b for b in layouts[0]] == first


def test_load_gen_insanns_matches_reference(tmp_path):
    """the numpy port against the dictionary the reference's load_gen_insanns built from the same tree, and the
    pickle load_anns_data builds when only gen_masks/ exists"""
    from miscc import load
    from miscc.config import cfg
    t = BO.load_golden()["tiny"]
    a = t["insanns_args"]
    data_dir = os.path.join(BO.TINY, "gen_masks_cases")
    saved = cfg.TREE.BRANCH_NUM
    cfg.TREE.BRANCH_NUM = 3
    try:
        got = load.load_gen_insanns(data_dir, a["filenames"], "test", a["imsize"], a["fmsize"], a["cats_index_dict"])
        work = os.path.join(str(tmp_path), "data")
        shutil.copytree(data_dir, work)
        built = load.load_anns_data(work, "test", "_gen_insanns.pickle", "gen", a["filenames"], a["imsize"],
                                    a["fmsize"], a["cats_index_dict"])
        with pytest.raises(FileNotFoundError):
            load.load_anns_data(work, "test", "_gt_insanns.pickle", "gt", a["filenames"], a["imsize"], a["fmsize"],
                                a["cats_index_dict"])
        with pytest.raises(FileNotFoundError):
            load.load_anns_data(str(tmp_path), "test", "_gen_insanns.pickle", "gen", a["filenames"], a["imsize"],
                                a["fmsize"], a["cats_index_dict"])
    finally:
        cfg.TREE.BRANCH_NUM = saved
    with open(os.path.join(work, "test_gen_insanns.pickle"), "rb") as f:
        assert pickle.load(f, encoding="latin1")[0].keys() == built.keys()
    want = t["insanns"]
    nones = 0
    for result in (got, built):
        assert list(result.keys()) == list(want.keys())
        for key in want:
            assert sorted(result[key].keys()) == sorted(want[key].keys()), key
            for index, w in want[key].items():
                r = result[key][index]
                assert set(r.keys()) == set(w.keys())
                assert r["num_rois"] == w["num_rois"]
                assert len(r["rois"]) == 3 and all(np.array_equal(x, y) for x, y in zip(r["rois"], w["rois"]))
                assert np.array_equal(r["fm_rois"], w["fm_rois"])
                for name in ("bbox maps", "bbox fmaps"):
                    m = BO.unpack_maps(w[name])
                    if m is None:
                        nones += 1
                        assert r[name] is None and r["num_rois"] == 0
                    else:
                        assert r[name].dtype == m.dtype and np.array_equal(r[name], m)
    assert nones >= 2 * 2 * 2                   # the empty file and the all-small file, both stacks, both results
    assert max(w["num_rois"] for annos in want.values() for w in annos.values()) == 10     # the BOXES_NUM cut


def test_checkpoint_load_reads_the_reference_directory():
    """a directory written by the reference's Checkpoint.save: equal state dict, equal vocabularies, a fresh module"""
    from seq2seq.models import DecoderRNN
    from seq2seq.util.checkpoint import Checkpoint
    t = BO.load_golden()["tiny"]
    ck = Checkpoint.load(os.path.join(BO.TINY, Checkpoint.CHECKPOINT_DIR_NAME, "tiny"))
    assert type(ck.model) is DecoderRNN and ck.model._packed is None
    sd = ck.model.state_dict()
    assert tuple(sorted(sd)) == BO.DECODER_KEYS == tuple(sorted(t["decoder_state"]))
    for k, v in t["decoder_state"].items():
        assert torch.equal(sd[k], v), k
    assert (ck.cap_word2index, ck.cap_index2word, ck.label_word2index, ck.label_index2word) == t["vocabularies"]
    c = t["config"]
    assert ck.model.hidden_size == c["H"] and ck.model.gmm_comp_num == c["K"] and ck.model.bidirectional_encoder
    assert ck.model.x_mean == 128.0 and ck.model.r_mean == 1.0


def test_refusals(capsys):
    import sample
    from objgan_hip import ops, _lib
    from seq2seq.models import DecoderRNN
    assert sample.main(["--is_training", "1"]) != 0
    assert "training the box generator" in capsys.readouterr().err
    assert sample.build_parser().parse_args([]).is_training == 1            # the reference's default
    w2i, _ = BO.label_vocabulary((1, 2, 3))
    with pytest.raises(NotImplementedError, match="attention"):
        DecoderRNN(w2i, 0.0, 0.0, 0.0, 0.0, 1, 150, 32, 2, use_attention=True)
    dec = DecoderRNN(w2i, 0.0, 0.0, 0.0, 0.0, 1, 150, 32, 2, bidirectional=True)
    hidden = (torch.zeros(2, 1, 16), torch.zeros(2, 1, 16))
    with pytest.raises(NotImplementedError, match="out of scope"):
        dec(hidden, None, is_training=1, early_stop_len=3)
    with pytest.raises(_lib.ObjganHipError, match="no CPU path"):
        ops.box_decode(torch.zeros(1, 32), torch.zeros(1, 32), torch.zeros(1, 3, 6, dtype=torch.float64),
                       dec._weights(), (0.0, 0.0, 0.0, 0.0), 1, 2)
    with pytest.raises(_lib.ObjganHipError):
        dec(hidden, None, is_training=0, early_stop_len=3, noise=np.zeros((1, 3, 6)))


def test_noise_rows_do_not_depend_on_batching():
    from seq2seq.models.DecoderRNN import draw_noise
    whole = draw_noise(np.random.RandomState(3), 5, 4)
    rs = np.random.RandomState(3)
    parts = np.concatenate([draw_noise(rs, 2, 4), draw_noise(rs, 3, 4)])
    assert whole.shape == (5, 4, 6) and np.array_equal(whole, parts)
    assert (whole[:, :, [0, 3]] >= 0).all() and (whole[:, :, [0, 3]] < 1).all()


def test_box_decode_limits_are_bad_args_on_the_host():
    """4H <= 1024, labels <= 256, K <= 8, T <= 32, the tile's LDS: refused before any launch (no GPU needed)"""
    from objgan_hip import _lib
    lib = _lib.load()
    ok = dict(B=0, T=10, H=256, L=83, K=5, A=50, sos=1, eos=2, cpw=4)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.objgan_box_decode(*([None] * 20), 0.0, 0.0, 0.0, 0.0, None, None, None, None, a["B"], a["T"], a["H"],
                                     a["L"], a["K"], a["A"], a["sos"], a["eos"], a["cpw"], None)
    assert call() == 1                                              # B = 0: nothing to do
    for bad in (dict(H=257), dict(L=257, H=256), dict(K=9), dict(T=33), dict(T=0), dict(cpw=3), dict(eos=83), dict(A=65)):
        assert call(**bad) == 0, bad
    assert call(B=1, cpw=8) == 0                                    # eight captions of this shape exceed 64 KiB of LDS
    assert lib.objgan_box_decode_default_cpw() == 4

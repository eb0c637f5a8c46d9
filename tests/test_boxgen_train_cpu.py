"""Box-generator training, host side (no GPU): the fp64 restatement and the seq2seq.loss classes against the reference's
recorded steps, the dataset functions against its recorded vocabularies and batches, the checkpoint round trip, the
refusals and the declarations of the new entry points.  Golden: tests/golden/make_golden_boxgen_train.py."""
import os
import re

import numpy as np
import pytest
import torch

import boxgen_oracle as BO
import boxgen_train_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("objgan_box_train_ws_floats", "objgan_box_train_forward", "objgan_box_train_loss",
                "objgan_box_train_backward", "objgan_box_train_clip")


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


def _check_caption(c, ref, b=0):
    n = c["n"]
    worst = max(BO.trajectory_error(ref["trace"][b, :n].numpy(), c["trace"].numpy()),
                _rel(float(ref["sums"][b, 0]), c["label_sum"]), _rel(float(ref["sums"][b, 1]), c["box_sum"]))
    assert int(ref["sums"][b, 2]) == n
    return worst


def test_restatement_matches_reference_small():
    """golden (a): trace, loss sums and all 17 gradients of every caption, and of the unclipped variant"""
    g = TO.load_golden()["small"]
    c0 = g["config"]
    sd = TO.small_decoder().state_dict()
    worst = 0.0
    for c, weight in [(c, g["weight"]) for c in g["captions"]] + [(g["unclipped"], torch.ones(c0["L"]))]:
        labels, boxes, lens, h0, cc = TO.stack_captions([c])
        ref = TO.step_ref(sd, h0, cc, labels, boxes, lens, c0["means"], weight, 1.0, 1.0, c0["K"])
        worst = max(worst, _check_caption(c, ref), _rel(ref["loss"], c["loss"]))
        worst = max([worst] + [TO.rel_l2(ref["grads"][k], v) for k, v in c["grads"].items()])
        assert ref["label_margin"] >= 2 and ref["norm_margin"] >= 2
    print("restatement vs reference, small: worst %.3g" % worst)
    assert worst <= TO.BOUND
    assert sorted(c["n"] for c in g["captions"]) == [1, 1, 2, 4, 4, 7]
    assert all(c["grad_norm"] > 5 for c in g["captions"]) and g["unclipped"]["grad_norm"] < 5


def test_restatement_matches_reference_real():
    """golden (b), the 4 captions as one batch: trace and sums per caption, the batch gradient's norms and projections
    against sum n_b g_b / sum n_b of the recorded single-caption values"""
    g = TO.load_golden()["real"]
    c = BO.load_golden()["real"]["config"]
    _, dec, _ = BO.real_modules()
    labels, boxes, lens, h0, c0 = TO.stack_captions(g["captions"])
    ref = TO.step_ref(dec.state_dict(), h0, c0, labels, boxes, lens, c["means"], g["weight"], 1.0, 1.0, c["K"])
    worst = max(_check_caption(cap, ref, b) for b, cap in enumerate(g["captions"]))
    N = sum(lens)
    for k, v in ref["grads"].items():
        d = TO.direction(k, v.shape, g["config"]["direction_seed"])
        want = sum(cap["n"] * cap["grad_dots"][k] for cap in g["captions"]) / N
        scale = sum(cap["n"] * cap["grad_norms"][k] for cap in g["captions"]) / N * float(d.norm())
        worst = max(worst, abs(float((v * d).sum()) - want) / scale)
    print("restatement vs reference, real: worst %.3g" % worst)
    assert worst <= TO.BOUND
    assert all(cap["label_margin"] >= 2 and cap["norm_margin"] >= 2 for cap in g["captions"])


def test_loss_classes_match_reference():
    """seq2seq.loss.Perplexity / BBLoss fed the reference's recorded traces -- golden (a) with its unit-weight record,
    and golden (b) at the real shape: its sums and its loss"""
    from seq2seq.loss import Perplexity, BBLoss
    g, real = TO.load_golden()["small"], TO.load_golden()["real"]
    rc = BO.load_golden()["real"]["config"]
    cases = [(c, g["weight"], g["config"]["L"], g["config"]["K"]) for c in g["captions"]]
    cases.append((g["unclipped"], torch.ones(g["config"]["L"]), g["config"]["L"], g["config"]["K"]))
    cases += [(c, real["weight"], rc["L"], rc["K"]) for c in real["captions"]]
    worst = 0.0
    for c, weight, L, K in cases:
        lloss, bloss = Perplexity(weight.clone(), 0, 1.0), BBLoss(1, K, 1.0)
        lloss.reset()
        bloss.reset()
        tr = c["trace"]
        for t in range(c["n"]):
            tl = torch.tensor([int(c["labels"][t + 1])])
            box = [torch.tensor([float(v)]) for v in c["boxes"][t + 1]]
            xy = tuple(tr[t:t + 1, L + i * K:L + (i + 1) * K] for i in range(6))
            wh = tuple(tr[t:t + 1, L + 6 * K + i * K:L + 6 * K + (i + 1) * K] for i in range(6))
            lloss.eval_batch(tr[t:t + 1, :L], tl)
            bloss.eval_batch(xy, wh, box[0], box[1], box[2], box[3], tl)
        worst = max(worst, _rel(float(lloss.acc_loss), c["label_sum"]), _rel(float(bloss.acc_loss), c["box_sum"]),
                    _rel(float(lloss.get_loss() + bloss.get_loss()), c["loss"]))
        assert int(lloss.norm_term) == int(bloss.norm_term) == c["n"]
    assert worst <= TO.BOUND, worst


def _tiny_data():
    from seq2seq.dataset.prepare_dataset import prepare_data
    t = BO.load_golden()["tiny"]
    return prepare_data(TO.TINY_TRAIN, os.path.join(BO.TINY, "input_test.txt"), os.path.join(BO.TINY, "mean_std_test.txt"),
                        150, 1, dict(t["vocabularies"][1]), dict(t["vocabularies"][0]))


def test_dataset_matches_reference():
    """prepare_data / random_batch: the reference's vocabularies, counts, label weights and batches, exactly"""
    import random
    import sample
    from seq2seq.dataset.prepare_dataset import random_batch, filter_tuples, nums_from_sentence, pad_seq
    d = TO.load_golden()["data"]
    out = _tiny_data()
    tc, tl, tuples = out[0], out[1], out[2]
    assert len(tuples) == d["n_tuples"]
    assert (tl.word2index, tl.index2word, tl.word2count) == (d["label_word2index"], d["label_index2word"],
                                                             d["label_word2count"])
    assert tc.word2count == d["cap_word2count"] and out[4].word2count == d["dev_label_word2count"]
    assert torch.equal(sample.label_weights(tl, d["config"]["count_smooth"]), d["weight"])
    random.seed(d["config"]["seed"])
    for want in d["batches"]:
        got = random_batch(d["config"]["batch_size"], tuples, tc, tl, out[6], out[7], out[8], out[9], is_training=1,
                           device="cpu")
        assert len(got) == 8
        for a, b in zip(got, want):
            assert torch.equal(a, b) if torch.is_tensor(b) else list(a) == list(b)
        assert list(got[1]) == sorted(got[1], reverse=True)
    assert nums_from_sentence(1.0, 2.0, "3 5") == [0, 1.0, 2.0, 0] and pad_seq([1], 3, 0) == [1, 0, 0]
    assert len(filter_tuples(tuples, 150, 1)) == len(tuples) and filter_tuples(tuples, 2, 1) == []


def test_checkpoint_round_trip(tmp_path):
    """Checkpoint.save -> load: state dict bit-equal, vocabularies, epoch, step, Adam moments and step count restored"""
    from seq2seq.optim import Optimizer
    from seq2seq.util.checkpoint import Checkpoint
    dec = TO.small_decoder()
    dec._weights()                                       # the kernel-layout cache must not reach the file
    adam = torch.optim.Adam(dec.parameters())
    g = torch.Generator().manual_seed(1)
    for p in dec.parameters():
        adam.state[p] = {"step": torch.tensor(7.0), "exp_avg": torch.randn(p.shape, generator=g),
                         "exp_avg_sq": torch.rand(p.shape, generator=g)}
    w2i, i2w = BO.label_vocabulary(range(1, 6))
    path = Checkpoint(dec, Optimizer(adam, max_grad_norm=5), 3, 41, {"a": 1}, {1: "a"}, w2i, i2w).save(str(tmp_path))
    assert sorted(os.listdir(path)) == sorted(["model.pt", "trainer_states.pt", "cap_word2index.pt",
                                               "cap_index2word.pt", "label_word2index.pt", "label_index2word.pt"])
    assert Checkpoint.get_latest_checkpoint(str(tmp_path)) == path
    ck = Checkpoint.load(path)
    assert (ck.epoch, ck.step, ck.cap_word2index, ck.cap_index2word) == (3, 41, {"a": 1}, {1: "a"})
    assert (ck.label_word2index, ck.label_index2word) == (w2i, i2w)
    sd, want = ck.model.state_dict(), dec.state_dict()
    assert tuple(sorted(sd)) == BO.DECODER_KEYS
    assert all(torch.equal(sd[k], want[k]) for k in want)
    assert ck.optimizer.max_grad_norm == 5 and isinstance(ck.optimizer.optimizer, torch.optim.Adam)
    for p, q in zip(dec.parameters(), ck.model.parameters()):
        a, b = adam.state[p], ck.optimizer.optimizer.state[q]
        assert float(b["step"]) == 7.0 and torch.equal(a["exp_avg"], b["exp_avg"])
        assert torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])


def test_entry_points_declared_listed_and_exported():
    from objgan_hip import _lib
    header = open(os.path.join(ROOT, "include", "objgan_hip.h")).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES or name in _lib.LONG_RETURN, name
        assert hasattr(lib, name), name


def test_host_refusals_of_the_entry_points():
    """limits are bad arguments on the host, before any launch (no GPU needed); CPU tensors have no path"""
    from objgan_hip import _lib, ops
    lib = _lib.load()
    ok = dict(B=0, T=10, H=256, L=83, K=5, A=50, cpw=4)

    def ws(**kw):
        a = dict(ok, **kw)
        return lib.objgan_box_train_ws_floats(a["B"], a["T"], a["H"], a["L"], a["K"], a["A"])

    def fwd(ws_floats=1 << 40, **kw):
        a = dict(ok, **kw)
        return lib.objgan_box_train_forward(*([None] * 22), 0.0, 0.0, 0.0, 0.0, None, None, ws_floats, a["B"], a["T"],
                                            a["H"], a["L"], a["K"], a["A"], a["cpw"], None)

    def bwd(ws_floats=1 << 40, **kw):
        a = dict(ok, **kw)
        return lib.objgan_box_train_backward(*([None] * 12), ws_floats, a["B"], a["T"], a["H"], a["L"], a["K"], a["A"],
                                             a["cpw"], None)
    assert fwd() == 1 and bwd() == 1 and ws() == 0 and ws(B=2) > 0 and ws(B=2, T=150) > ws(B=2)
    for bad in (dict(H=257), dict(L=257), dict(K=9), dict(T=257), dict(T=0), dict(cpw=3), dict(A=65), dict(cpw=8)):
        assert fwd(**bad) == 0, bad
    for bad in (dict(H=257), dict(L=257), dict(K=9), dict(T=257), dict(T=0), dict(cpw=3), dict(A=65)):
        assert bwd(**bad) == 0, bad
        if "cpw" not in bad:
            assert ws(B=1, **bad) == 0, bad
    assert fwd(B=1) == 0 and bwd(B=1) == 0                          # null pointers
    assert fwd(B=1, ws_floats=10) == 0 and bwd(B=1, ws_floats=10) == 0
    assert lib.objgan_box_train_loss(*([None] * 5), 1.0, 1.0, None, None, 0, 10, 83, 5, 0, None) == 1
    for L, K, T, pad in ((257, 5, 10, 0), (83, 9, 10, 0), (83, 5, 257, 0), (83, 5, 10, 83)):
        assert lib.objgan_box_train_loss(*([None] * 5), 1.0, 1.0, None, None, 1, T, L, K, pad, None) == 0
    assert lib.objgan_box_train_loss(*([None] * 5), 1.0, 1.0, None, None, 1, 10, 83, 5, 0, None) == 0
    assert lib.objgan_box_train_clip(None, 10, 5.0, None, None, None) == 0
    dec = TO.small_decoder()
    W = dec._weights()
    lab, box, ln = torch.zeros(1, 3, dtype=torch.int32), torch.zeros(1, 3, 4), torch.ones(1, dtype=torch.int32)
    with pytest.raises(_lib.ObjganHipError, match="no CPU path"):
        ops.box_train_forward(torch.zeros(1, 32), torch.zeros(1, 32), lab, box, ln, W, (0, 0, 0, 0))
    with pytest.raises(_lib.ObjganHipError, match="no CPU path"):
        ops.box_train_loss(torch.zeros(1, 2, 33), lab, box, ln, torch.ones(9), 1.0, 1.0, 2)
    with pytest.raises(_lib.ObjganHipError, match="no CPU path"):
        ops.box_train_backward(torch.zeros(1, 2, 33), torch.zeros(1, 2, 33), torch.zeros(1, 32), lab, ln, W,
                               torch.zeros(8))
    with pytest.raises(_lib.ObjganHipError, match="no CPU path"):
        ops.box_train_clip(torch.zeros(8), 5.0)


def test_decoder_training_refusals():
    from seq2seq.models import DecoderRNN
    w2i, _ = BO.label_vocabulary((1, 2, 3))
    hidden = (torch.zeros(2, 1, 16), torch.zeros(2, 1, 16))
    tl, tx = torch.tensor([[1, 4, 2]]), torch.zeros(1, 3)
    dec = DecoderRNN(w2i, 0.0, 0.0, 0.0, 0.0, 1, 150, 32, 2, bidirectional=True, input_dropout_p=0.1)
    with pytest.raises(NotImplementedError, match="input_dropout_p"):
        dec(hidden, None, tl, tx, tx, tx, tx, is_training=1)
    dec = DecoderRNN(w2i, 0.0, 0.0, 0.0, 0.0, 1, 150, 32, 2, bidirectional=True, dropout_p=0.2)
    with pytest.raises(NotImplementedError, match="out of scope"):
        dec(hidden, None, is_training=1)
    labels, boxes, lens = DecoderRNN.pack_targets(torch.tensor([[1, 4, 5, 2], [1, 2, 0, 0]]), *([torch.zeros(2, 4)] * 4))
    assert lens.tolist() == [3, 1] and labels.dtype == torch.int32 and tuple(boxes.shape) == (2, 4, 4)


def test_sample_training_refuses_missing_inputs(tmp_path, capsys):
    import sample
    rc = sample.main(["--is_training", "1", "--train_path", str(tmp_path / "absent.txt")])
    err = capsys.readouterr().err
    assert rc != 0 and "training the box generator" in err and len(err.strip().splitlines()) == 1

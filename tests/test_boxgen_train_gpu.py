"""Box-generator training on the device: csrc/box_train.hip (forward, loss, backward, clip) and the fused Adam against
the reference's recorded single-caption steps (tests/golden/boxgen_train_ref.pt) and the fp64 restatement of
tests/boxgen_train_oracle.py; batch independence bit for bit; the autograd route; sample.py --is_training 1 end to
end.  Every bound is the project's operator bound."""
import os
import pickle

import numpy as np
import pytest
import torch

import boxgen_oracle as BO
import boxgen_train_oracle as TO
from conftest import note

pytestmark = pytest.mark.gpu

BOUND = TO.BOUND


def _dev_targets(labels, boxes, lens, dev):
    return (torch.as_tensor(labels).to(torch.int32).to(dev).contiguous(),
            torch.as_tensor(boxes).float().to(dev).contiguous(), torch.tensor(list(lens), dtype=torch.int32, device=dev))


def _step(decoder, h0, c0, labels, boxes, lens, weight, dev, cpw=None, W=None):
    """forward, loss, backward on the device -> trace, sums [B, 4] + N, dtrace, grads {state key: tensor}"""
    from objgan_hip import ops
    W = decoder._weights() if W is None else W
    lab, box, ln = _dev_targets(labels, boxes, lens, dev)
    first = (decoder.x_mean, decoder.y_mean, decoder.w_mean, decoder.r_mean)
    h0, c0 = h0.float().to(dev).contiguous(), c0.float().to(dev).contiguous()
    trace, ws = ops.box_train_forward(h0, c0, lab, box, ln, W, first, cpw=cpw)
    w = torch.as_tensor(weight).float().clone()
    w[0] = 0
    sums, dtrace = ops.box_train_loss(trace, lab, box, ln, w.to(dev), 1.0, 1.0, decoder.gmm_comp_num)
    grads = ops.box_train_backward(dtrace, trace, c0, lab, ln, W, ws, cpw=cpw)
    torch.cuda.synchronize()
    s = sums.cpu()
    return {"trace": trace.cpu(), "sums": s[:-1].view(-1, 4), "N": float(s[-1]), "dtrace": dtrace.cpu(),
            "grads": {k: v.detach().cpu().clone() for k, v in TO.to_state_layout(grads).items()}, "flat": grads}


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


@pytest.fixture(scope="module")
def small(dev):
    g = TO.load_golden()["small"]
    return g, TO.small_decoder().to(dev)


def test_small_shape_matches_reference_per_caption(dev, small):
    """golden (a): every caption alone, as the reference ran it: trace, loss sums, all 17 gradients"""
    g, dec = small
    worst = {"trace": 0.0, "sums": 0.0, "grads": 0.0}
    for c in g["captions"]:
        labels, boxes, lens, h0, c0 = TO.stack_captions([c])
        r = _step(dec, h0, c0, labels, boxes, lens, g["weight"], dev)
        worst["trace"] = max(worst["trace"], BO.trajectory_error(r["trace"][0].numpy(), c["trace"].numpy()))
        worst["sums"] = max(worst["sums"], _rel(float(r["sums"][0, 0]), c["label_sum"]),
                            _rel(float(r["sums"][0, 1]), c["box_sum"]))
        assert int(r["sums"][0, 2]) == c["n"] == int(r["N"])
        for k, want in c["grads"].items():
            worst["grads"] = max(worst["grads"], TO.rel_l2(r["grads"][k], want))
    for k, v in worst.items():
        note("boxgen train small vs reference: %s, worst" % k, "%.3g" % v)
        print("small vs reference", k, "%.3g" % v)
    assert max(worst.values()) <= BOUND, worst


@pytest.fixture(scope="module")
def real_ref():
    """the fp64 restatement of the real-shape batch, computed once"""
    g = TO.load_golden()["real"]
    _, dec, _ = BO.real_modules()
    labels, boxes, lens, h0, c0 = TO.stack_captions(g["captions"])
    c = BO.load_golden()["real"]["config"]
    ref = TO.step_ref(dec.state_dict(), h0, c0, labels, boxes, lens, c["means"], g["weight"], 1.0, 1.0, c["K"])
    ref3 = TO.step_ref(dec.state_dict(), h0[:3], c0[:3], labels[:3], boxes[:3], lens[:3], c["means"], g["weight"], 1.0,
                       1.0, c["K"])
    return g, dec, (labels, boxes, lens, h0, c0), ref, ref3


def test_real_shape_batch(dev, real_ref):
    """H = 256, 83 labels, K = 5: the golden's 4 captions as one batch; trace and sums against the reference, gradient
    norms and projections against sum n_b g_b / sum n_b of its recorded single-caption values, full gradients against
    the restatement.  cpw is 1, 2 or 4 at this shape (8 exceeds the LDS), all of which divide 4: the partly filled tile
    is the first three captions under cpw = 2, whose rows must be the same bits."""
    g, dec, (labels, boxes, lens, h0, c0), ref, ref3 = real_ref
    dec = dec.to(dev)
    r = _step(dec, h0, c0, labels, boxes, lens, g["weight"], dev, cpw=4)
    r3 = _step(dec, h0[:3], c0[:3], labels[:3], boxes[:3], lens[:3], g["weight"], dev, cpw=2)     # cpw does not divide B
    worst_t = worst_s = 0.0
    for b, c in enumerate(g["captions"]):
        n = c["n"]
        assert not r["trace"][b, n:].any()
        worst_t = max(worst_t, BO.trajectory_error(r["trace"][b, :n].numpy(), c["trace"].numpy()))
        worst_s = max(worst_s, _rel(float(r["sums"][b, 0]), c["label_sum"]), _rel(float(r["sums"][b, 1]), c["box_sum"]))
        if b < 3:
            assert torch.equal(r3["trace"][b, :n], r["trace"][b, :n])
    # the partly filled tile: its loss sums against the reference, its gradients against the restatement of those three
    worst_s3 = max(_rel(float(r3["sums"][b, i]), g["captions"][b][k]) for b in range(3)
                   for i, k in ((0, "label_sum"), (1, "box_sum")))
    assert [int(v) for v in r3["sums"][:, 2]] == lens[:3] and int(r3["N"]) == sum(lens[:3])
    # its dtrace rows are the full batch's up to the normaliser 1 / sum n_b (two fp32 roundings of it)
    assert TO.rel_l2(r3["dtrace"] * (sum(lens[:3]) / sum(lens)), r["dtrace"][:3]) <= 1e-6
    worst_g3 = max(TO.rel_l2(r3["grads"][k], v) for k, v in ref3["grads"].items())
    N = sum(c["n"] for c in g["captions"])
    seed = g["config"]["direction_seed"]
    worst_d = worst_g = 0.0
    for k, want in ref["grads"].items():
        worst_g = max(worst_g, TO.rel_l2(r["grads"][k], want))
        d = TO.direction(k, want.shape, seed)
        dot_ref = sum(c["n"] * c["grad_dots"][k] for c in g["captions"]) / N
        scale = sum(c["n"] * c["grad_norms"][k] for c in g["captions"]) / N * float(d.norm())
        worst_d = max(worst_d, abs(float((r["grads"][k].double() * d).sum()) - dot_ref) / scale)
    # a single caption's gradient norms, directly
    c = g["captions"][-1]
    one = _step(dec, h0[-1:], c0[-1:], labels[-1:], boxes[-1:], lens[-1:], g["weight"], dev)
    worst_n = max(_rel(float(one["grads"][k].double().norm()), v) for k, v in c["grad_norms"].items())
    for name, v in (("trace", worst_t), ("loss sums", worst_s), ("gradients vs fp64", worst_g),
                    ("projections vs reference", worst_d), ("gradient norms vs reference", worst_n),
                    ("partly filled tile, loss sums", worst_s3), ("partly filled tile, gradients vs fp64", worst_g3)):
        note("boxgen train real shape: %s, worst" % name, "%.3g" % v)
        print("real", name, "%.3g" % v)
    assert max(worst_t, worst_s, worst_g, worst_d, worst_n, worst_s3, worst_g3) <= BOUND


def _edge(dev, H, K, lens, seed, bias=None, L=9):
    from seq2seq.models import DecoderRNN
    w2i, _ = BO.label_vocabulary(range(1, L - 3))
    dec = BO.seeded_fill_(DecoderRNN(w2i, 0.1, -0.2, 0.3, 0.05, 1, 150, H, K, bidirectional=True), seed, scale=0.3)
    if bias is not None:
        with torch.no_grad():
            dec.l_out.bias.add_(torch.tensor(bias))
    labels, boxes = TO.make_batch(seed, lens, L)
    g = torch.Generator().manual_seed(seed)
    h0, c0 = torch.randn(len(lens), H, generator=g) * 0.5, torch.randn(len(lens), H, generator=g) * 0.5
    weight = torch.rand(L, generator=g) + 0.5
    ref = TO.step_ref(dec.state_dict(), h0, c0, labels, boxes, lens, (0.1, -0.2, 0.3, 0.05), weight, 1.0, 1.0, K)
    return dec.to(dev), (labels, boxes, lens, h0, c0), weight, ref


def _against_ref(r, ref, lens, what):
    worst_t = max(BO.trajectory_error(r["trace"][b].numpy(), ref["trace"][b].numpy()) for b in range(len(lens)))
    worst_s = max(_rel(float(r["sums"][b, i]), float(ref["sums"][b, i])) for b in range(len(lens)) for i in (0, 1))
    worst_g = max(TO.rel_l2(r["grads"][k], v) for k, v in ref["grads"].items())
    assert [int(v) for v in r["sums"][:, 2]] == [int(v) for v in ref["sums"][:, 2]]
    assert [int(v) for v in r["sums"][:, 3]] == ref["matches"]
    for name, v in (("trace", worst_t), ("loss sums", worst_s), ("gradients", worst_g)):
        note("boxgen train %s vs fp64: %s, worst" % (what, name), "%.3g" % v)
        print(what, name, "%.3g" % v)
    assert max(worst_t, worst_s, worst_g) <= BOUND, (what, worst_t, worst_s, worst_g)


def test_edge_shape_h20_k1(dev):
    """4H = 80 is not a multiple of the wave, one mixture component, B = 5 with lengths {1, 1, 2, 4, 7}"""
    lens = [1, 1, 2, 4, 7]
    dec, batch, weight, ref = _edge(dev, 20, 1, lens, 3)
    assert ref["label_margin"] >= 2 and ref["norm_margin"] >= 2
    r = _step(dec, batch[3], batch[4], batch[0], batch[1], lens, weight, dev)
    _against_ref(r, ref, lens, "H=20 K=1")
    # another pad label (<eos>, the last target of every caption): the normaliser and the per-caption counts agree
    from objgan_hip import ops
    lab, box, ln = _dev_targets(batch[0], batch[1], lens, dev)
    sums = ops.box_train_loss(r["trace"].to(dev), lab, box, ln, weight.to(dev), 1.0, 1.0, 1, pad=2)[0].cpu()
    assert float(sums[-1]) == float(sums[:-1].view(-1, 4)[:, 2].sum()) == sum(n - 1 for n in lens)


def test_label_clamp_active(dev):
    """l_out.bias pushes most label probabilities below 1e-5: their gradient is zero; none within a factor 2 of it"""
    lens = [7, 4, 2]
    dec, batch, weight, ref = _edge(dev, 32, 2, lens, 3, bias=[0, 0, 9.0, 0, 0, 0, 0, 0, -6.0])
    assert ref["label_margin"] >= 2
    r = _step(dec, batch[3], batch[4], batch[0], batch[1], lens, weight, dev, cpw=1)
    clamped = r["trace"][:, :, :9] == np.float32(1e-5)
    assert int(clamped.sum()) >= 3 and not r["dtrace"][:, :, :9][clamped].any()
    _against_ref(r, ref, lens, "clamp active")


def test_rows_do_not_depend_on_batching(dev, small):
    """a caption alone, in a batch, under another cpw and padded to a larger T: the same trace and dtrace rows, bit for
    bit once the batch normaliser is the same; gradients identical run to run and unchanged by padding; the batch
    gradient is sum n_b g_b / sum n_b of the single-caption gradients"""
    g, dec = small
    caps = g["captions"]
    labels, boxes, lens, h0, c0 = TO.stack_captions(caps)
    a = _step(dec, h0, c0, labels, boxes, lens, g["weight"], dev, cpw=4)
    b = _step(dec, h0, c0, labels, boxes, lens, g["weight"], dev, cpw=4)
    plab, pbox = TO.pad_batch(labels, boxes, 12)
    p = _step(dec, h0, c0, plab, pbox, lens, g["weight"], dev, cpw=4)
    o = _step(dec, h0, c0, labels, boxes, lens, g["weight"], dev, cpw=1)
    T = max(lens)
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k                   # run to run
        assert torch.equal(a["grads"][k], p["grads"][k]), k                   # extra padding
    assert torch.equal(a["trace"], o["trace"]) and torch.equal(a["dtrace"], o["dtrace"])
    assert torch.equal(a["trace"], p["trace"][:, :T]) and torch.equal(a["dtrace"], p["dtrace"][:, :T])
    assert not p["trace"][:, T:].any() and not p["dtrace"][:, T:].any()
    # reversed order, another place in the batch
    rev = list(range(len(lens)))[::-1]
    r = _step(dec, h0[rev], c0[rev], labels[rev], boxes[rev], [lens[i] for i in rev], g["weight"], dev, cpw=2)
    assert torch.equal(r["trace"][rev], a["trace"]) and torch.equal(r["dtrace"][rev], a["dtrace"])
    # alone: the trace rows are the same bits; dtrace differs by the normaliser n_b / N only
    N = sum(lens)
    mix = {k: torch.zeros_like(v, dtype=torch.float64) for k, v in a["grads"].items()}
    for i, n in enumerate(lens):
        one = _step(dec, h0[i:i + 1], c0[i:i + 1], labels[i:i + 1, :n + 1], boxes[i:i + 1, :n + 1], [n], g["weight"], dev)
        assert torch.equal(one["trace"][0], a["trace"][i, :n])
        for k in mix:
            mix[k] += one["grads"][k].double() * n / N
    worst = max(TO.rel_l2(a["grads"][k], mix[k]) for k in mix)
    note("boxgen train: batch gradient vs sum n_b g_b / N, worst", "%.3g" % worst)
    assert worst <= BOUND


def _host_update(params, grads, max_norm=5):
    """clip_grad_norm_ + torch.optim.Adam fed the given gradients, in fp32 on the CPU -> updates"""
    ps = [torch.nn.Parameter(p.clone()) for p in params.values()]
    for p, k in zip(ps, params):
        p.grad = grads[k].clone()
    torch.nn.utils.clip_grad_norm_(ps, max_norm)
    torch.optim.Adam(ps).step()
    return {k: p.detach() - params[k] for k, p in zip(params, ps)}


@pytest.mark.parametrize("case", ["clipped", "unclipped"])
def test_clip_and_adam_update(dev, case):
    """one fused step: the UPDATE p_after - p_before against clip_grad_norm_ + torch.optim.Adam on the device's own
    gradients, and against the reference's recorded post-step parameters"""
    from seq2seq.trainer import FusedBoxStep
    g = TO.load_golden()["small"]
    c = g["captions"][g["config"]["stepped"][0]] if case == "clipped" else g["unclipped"]
    weight = g["weight"] if case == "clipped" else torch.ones(g["config"]["L"])
    dec = TO.small_decoder().to(dev)
    before = {k: v.detach().cpu().clone() for k, v in dec.state_dict().items()}
    labels, boxes, lens, h0, c0 = TO.stack_captions([c])
    lab, box, ln = _dev_targets(labels, boxes, lens, dev)
    fused = FusedBoxStep(dec, weight)
    fused.gradients(h0.to(dev), c0.to(dev), lab, box, ln)
    grads = {k: v.detach().cpu().clone() for k, v in TO.to_state_layout(fused.g).items()}
    fused.update()
    fused.sync_to_module()
    torch.cuda.synchronize()
    norm = float(fused.clip[1])
    assert (norm > 5) == (case == "clipped") and abs(norm - c["grad_norm"]) <= 1e-4 * c["grad_norm"]
    assert float(fused.state[0]) == 1.0
    after = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    want = _host_update(before, grads)
    worst_h = max(TO.rel_l2(after[k] - before[k], want[k]) for k in before)
    worst_r = max(TO.rel_l2(after[k] - before[k], c["after"][k] - before[k]) for k in before)
    note("boxgen train %s: update vs clip_grad_norm_ + Adam, worst" % case, "%.3g" % worst_h)
    note("boxgen train %s: update vs the reference's step, worst" % case, "%.3g" % worst_r)
    print(case, "update vs host %.3g vs reference %.3g" % (worst_h, worst_r))
    assert worst_h <= BOUND and worst_r <= BOUND


def test_autograd_route_gives_the_fused_gradients(dev, small):
    """the reference-style loop (decoder(...), eval_batch per step, loss.backward()) on the returned lists"""
    from seq2seq.loss import Perplexity, BBLoss
    g, _ = small
    dec = TO.small_decoder().to(dev)
    caps = [g["captions"][3], g["captions"][4]]                       # equal lengths: no padded step reaches BBLoss
    labels, boxes, lens, h0, c0 = TO.stack_captions(caps)
    fused = _step(dec, h0, c0, labels, boxes, lens, g["weight"], dev)
    H = h0.shape[1] // 2
    hidden = tuple(s.view(-1, 2, H).transpose(0, 1).contiguous().to(dev) for s in (h0, c0))
    tl = torch.as_tensor(labels).to(dev)
    tb = [torch.as_tensor(boxes[:, :, i]).to(dev) for i in range(4)]
    lloss, bloss = Perplexity(g["weight"].clone().to(dev), 0, 1.0), BBLoss(2, dec.gmm_comp_num, 1.0)
    outs, xy, wh, _, other = dec(hidden, None, tl, tb[0], tb[1], tb[2], tb[3], is_training=1)
    assert len(outs) == lens[0] and len(other["sequence"]) == lens[0]
    for step, out in enumerate(outs):
        lloss.eval_batch(out.contiguous().view(2, -1), tl[:, step + 1])
        bloss.eval_batch(xy[step], wh[step], tb[0][:, step + 1], tb[1][:, step + 1], tb[2][:, step + 1],
                         tb[3][:, step + 1], tl[:, step + 1])
    loss = lloss.get_loss() + bloss.get_loss()
    dec.zero_grad()
    loss.backward()
    want = (fused["sums"][:, 0].sum() + fused["sums"][:, 1].sum()) / fused["N"]
    assert _rel(float(loss), float(want)) <= BOUND
    worst = max(TO.rel_l2(p.grad, fused["grads"][k]) for k, p in dec.named_parameters())
    note("boxgen train: autograd route vs fused gradients, worst", "%.3g" % worst)
    assert worst <= BOUND


def test_sample_trains_and_samples_end_to_end(dev, tmp_path, capsys):
    """sample.main(["--is_training", "1", ...]) on the tiny training file (H = 32, batch 4, seeded, 204 steps) writes a
    checkpoint `--is_training 0` samples from; the mean loss of the last 10 steps lies below that of the first 10 by
    at least half the drop the fp64 restatement's recorded curve shows under the same schedule"""
    import sample
    from seq2seq.trainer import SupervisedTrainer
    from seq2seq.util.checkpoint import Checkpoint
    t = BO.load_golden()["tiny"]
    curve = TO.load_golden()["curve"]
    cfg = curve["config"]
    vocab, enc_path, expt = str(tmp_path / "captions.pickle"), str(tmp_path / "enc.pth"), str(tmp_path / "expt")
    with open(vocab, "wb") as f:
        pickle.dump([None, None, dict(t["vocabularies"][1]), dict(t["vocabularies"][0])], f)
    torch.save(BO.tiny_encoder().state_dict(), enc_path)
    history = []
    orig = SupervisedTrainer._train_epoches

    def keeping(self, *a, **k):
        out = orig(self, *a, **k)
        history.extend(self.history)
        return out
    SupervisedTrainer._train_epoches = keeping
    common = ["--dev_path", os.path.join(BO.TINY, "input_test.txt"), "--mean_std_path",
              os.path.join(BO.TINY, "mean_std_test.txt"), "--encoder_path", enc_path, "--expt_dir", expt,
              "--embedding_dim", str(t["config"]["H"]), "--gmm_comp_num", str(t["config"]["K"]),
              "--batch_size", str(cfg["batch_size"]), "--seed", str(cfg["seed"]), "--train_path", TO.TINY_TRAIN]
    try:
        rc = sample.main(["--is_training", "1", "--vocab_path", vocab, "--num_epochs", str(cfg["num_epochs"]),
                          "--print_every", "1", "--checkpoint_every", "1000", "--log-level", "warning"] + common)
    finally:
        SupervisedTrainer._train_epoches = orig
    capsys.readouterr()
    assert rc == 0 and len(history) == cfg["steps"]
    loss = [l + b for _, l, b in history]
    first, last = float(np.mean(loss[:10])), float(np.mean(loss[-10:]))
    note("boxgen train end to end: mean loss first 10 / last 10 steps (fp64 curve %.1f / %.1f)"
         % (curve["first10"], curve["last10"]), "%.1f / %.1f" % (first, last))
    assert first - last >= 0.5 * (curve["first10"] - curve["last10"]), (first, last, curve["first10"], curve["last10"])
    name = os.path.basename(Checkpoint.get_latest_checkpoint(expt))
    ck = Checkpoint.load(os.path.join(expt, Checkpoint.CHECKPOINT_DIR_NAME, name))
    assert ck.step == cfg["steps"] and ck.optimizer is not None
    rc = sample.main(["--is_training", "0", "--load_checkpoint", name, "--dev_filename_path",
                      os.path.join(BO.TINY, "filenames_test.txt"), "--gaussian_dict_path",
                      os.path.join(BO.TINY, "gaussian_dict.npy"), "--box_saving_folder", str(tmp_path / "gen_masks"),
                      "--log-level", "warning"] + common)
    assert rc == 0
    out = str(tmp_path / "gen_masks") + "_%s" % name
    assert sum(f == "boxes.txt" for _, _, fs in os.walk(out) for f in fs) == len(t["keys"])
    # --resume continues from the written epoch, step and Adam state: two more epochs of 6 steps.  The run counts past
    # total_steps and no multiple of checkpoint_every falls into it: the checkpoint after the last epoch holds it
    rc = sample.main(["--is_training", "1", "--resume", "--vocab_path", vocab, "--num_epochs", str(cfg["num_epochs"] + 1),
                      "--print_every", "1000", "--checkpoint_every", "1000", "--log-level", "warning"] + common)
    capsys.readouterr()
    assert rc == 0
    ck2 = Checkpoint.load(Checkpoint.get_latest_checkpoint(expt))
    assert ck2.step == cfg["steps"] + 12 and ck2.epoch == cfg["num_epochs"] + 1
    steps = {float(s["step"]) for s in ck2.optimizer.optimizer.state.values()}
    assert steps == {float(cfg["steps"] + 12)}
    assert any(not torch.equal(a, b) for a, b in zip(ck.model.state_dict().values(), ck2.model.state_dict().values()))

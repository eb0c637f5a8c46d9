"""DAMSM pretraining on the device: csrc/lstm_train.hip (training forward, BPTT, weight / table gradients) against the
recorded run of the unmodified reference (tests/golden/damsm_ref.pt) and the fp64 restatement of tests/damsm_oracle.py;
bit identity with the frozen forward; batch independence and run-to-run determinism bit for bit; the whole step with
clip and Adam; the launch refusals; pretrain_DAMSM.py end to end.  Bound: the project's operator bound, 1e-4 rel-L2
against fp64."""
import glob
import os

import pytest
import torch

import damsm_oracle as DO
from conftest import ROOT, note, rel_l2

pytestmark = pytest.mark.gpu

BOUND = 1e-4
SUFFIXES = ("", "_reverse")


def _packed(params, dev):
    """the frozen launch's operands: transposed stacks [2][I][4H], [2][H][4H], biases [2][4H]"""
    st = lambda name, t: torch.stack([params["rnn.%s_l0%s" % (name, s)].t() if t else params["rnn.%s_l0%s" % (name, s)]  # noqa: E731
                                      for s in SUFFIXES]).contiguous().to(dev)
    return st("weight_ih", True), st("weight_hh", True), st("bias_ih", False), st("bias_hh", False)


def _leaves(params, dev):
    return {k: v.detach().clone().to(dev).requires_grad_() for k, v in params.items()}


def _train_call(leaves, captions, lens, max_len, keep=None, p=0.0):
    from objgan_hip import ops
    pair = lambda name: tuple(leaves["rnn.%s_l0%s" % (name, s)] for s in SUFFIXES)  # noqa: E731
    return ops.lstm_bidir_train(leaves["encoder.weight"], captions, lens, pair("weight_ih"), pair("weight_hh"),
                                pair("bias_ih"), pair("bias_hh"), max_len, keep, p)


def _probe(params, captions, lens, max_len, r_words, r_sent, dev, keep=None, p=0.0):
    """device gradients of sum(words * r_words) + sum(sent * r_sent), i.e. the backward for (d_out, d_hn) = (r_words, r_sent)"""
    leaves = _leaves(params, dev)
    words, sent = _train_call(leaves, captions.to(dev), torch.tensor(lens), max_len, None if keep is None else keep.to(dev), p)
    ((words * r_words.to(dev)).sum() + (sent * r_sent.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    return words.detach().cpu(), sent.detach().cpu(), {k: v.grad.detach().cpu() for k, v in leaves.items()}


def _check_probe(tag, params, captions, lens, max_len, dev, keep=None, p=0.0, seed=0):
    H2 = 2 * params["rnn.weight_hh_l0"].shape[1]
    g = torch.Generator().manual_seed(100 + seed)
    rw, rs = torch.randn(len(lens), H2, max_len, generator=g), torch.randn(len(lens), H2, generator=g)
    words, sent, grads = _probe(params, captions, lens, max_len, rw, rs, dev, keep, p)
    want = DO.linear_probe_ref(params, captions, lens, max_len, rw, rs, keep, p)
    errs = {"words": rel_l2(words, want["words"]), "sent": rel_l2(sent, want["sent"])}
    errs.update({k: rel_l2(grads[k], want["grads"][k]) for k in DO.TEXT_KEYS})
    worst = max(errs, key=errs.get)
    note("lstm_train %s vs fp64 restatement: worst rel-L2 (%s)" % (tag, worst), "%.3e" % errs[worst])
    assert all(torch.isfinite(v).all() for v in grads.values()), tag
    assert errs[worst] < BOUND, (tag, errs)
    return grads, want


# ---- bit identity of the training forward -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["golden", "recipe"])
def test_training_forward_is_the_frozen_forward_bit_for_bit(dev, shape):
    from objgan_hip import ops
    if shape == "golden":
        g = DO.load_golden()
        params, caps, lens, outs = g["params"], g["captions"], list(g["config"]["lens"]), (g["config"]["L"], 4)
    else:
        params = DO.seeded_text_params(40, 300, 128, 11)
        caps = torch.randint(1, 40, (5, 12), generator=torch.Generator().manual_seed(12))
        lens, outs = [12, 9, 5, 1, 0], (12, 7)
    wt_ih, wt_hh, b_ih, b_hh = _packed(params, dev)
    table, caps_d, lens_d = params["encoder.weight"].to(dev), caps.to(dev), torch.tensor(lens)
    for max_len in outs:
        w0, s0 = ops.lstm_bidir_forward(table, caps_d, lens_d, wt_ih, wt_hh, b_ih, b_hh, max_len)
        w1, s1, ws = ops.lstm_bidir_train_forward(table, caps_d, lens_d, wt_ih, wt_hh, b_ih, b_hh, max_len)
        assert torch.equal(w0, w1) and torch.equal(s0, s1), (shape, max_len)
        assert torch.isfinite(ws[:ops.lstm_train_ws_sections(len(lens), caps.shape[1], table.shape[1],
                                                              wt_hh.shape[1])[0]["dgate"][0]]).all()
        w2, s2 = _train_call({k: v.to(dev) for k, v in params.items()}, caps_d, lens_d, max_len)      # the autograd route
        assert torch.equal(w0, w2) and torch.equal(s0, s2)


# ---- kernel gradients ---------------------------------------------------------------------------------------------------
def test_golden_step_matches_the_reference(dev):
    """the recorded reference run (H = 8: 4H below a wave): losses, every encoder gradient, d feats, d codes"""
    import model as M
    from miscc.losses import words_loss, sent_loss
    g = DO.load_golden()
    c = g["config"]
    enc = M.RNN_ENCODER(c["ntoken"], ninput=c["ninput"], drop_prob=0, nhidden=c["nhidden"])
    enc.load_state_dict(g["params"], strict=True)
    enc.to(dev).train()
    feats, codes = g["feats"].to(dev).requires_grad_(), g["codes"].to(dev).requires_grad_()
    lens = torch.tensor(c["lens"])
    B = len(c["lens"])
    import numpy as np
    words, sent = enc(g["captions"].to(dev), lens, c["L"])
    labels = torch.arange(B, device=dev)
    ids = np.asarray(c["class_ids"])
    w0, w1, _, _ = words_loss(feats, words, labels, lens.to(dev), ids, B, top1=False, need_att_maps=False)
    s0, s1, _ = sent_loss(codes, sent, labels, ids, B, top1=False)
    (w0 + w1 + s0 + s1).backward()
    torch.cuda.synchronize()
    errs = {"words": rel_l2(words, g["words_emb"]), "sent": rel_l2(sent, g["sent_emb"]),
            "d_feats": rel_l2(feats.grad, g["d_feats"]), "d_codes": rel_l2(codes.grad, g["d_codes"])}
    for name, got, want in zip(("w0", "w1", "s0", "s1"), (w0, w1, s0, s1), g["losses"]):
        errs[name] = abs(float(got) - want) / abs(want)
    errs.update({k: rel_l2(p.grad, g["grads"][k]) for k, p in enc.named_parameters()})
    for k, v in sorted(errs.items()):
        note("damsm golden step vs reference: %s" % k, "%.3e" % v)
    assert set(errs) >= set(DO.TEXT_KEYS) and max(errs.values()) < BOUND, errs


EDGE_CAPS = torch.tensor([[3, 7, 7, 12, 3, 29, 5], [7, 1, 12, 12, 28, 0, 0], [7, 400, -3, 7, 29, 0, 0], [7, 0, 0, 0, 0, 0, 0],
                          [9, 9, 9, 0, 0, 0, 0]])
EDGE_LENS = [7, 5, 5, 1, 0]         # L, 1 and 0 in one batch; token 7 in every caption with words; 400 and -3 out of range


@pytest.mark.parametrize("I,H,max_len,drop", [(20, 8, 7, 0.0), (20, 20, 7, 0.0), (1, 8, 7, 0.0), (70, 20, 4, 0.0),
                                              (70, 8, 9, 0.5), (20, 20, 4, 0.5)])
def test_kernel_gradients_at_the_edges(dev, I, H, max_len, drop):
    """H = 8 (4H below a wave), H = 20 (4H no multiple of 64), I = 1 and 70, Lout < L and > L, lengths L / 1 / 0,
    out-of-range and negative tokens, a token in every caption, a keep-mask with p = 0.5"""
    params = DO.seeded_text_params(30, I, H, 7 + I + H)
    keep = None
    if drop > 0:
        keep = (torch.rand(5, 7, I, generator=torch.Generator().manual_seed(5)) >= drop).to(torch.uint8)
    grads, want = _check_probe("I=%d H=%d Lout=%d p=%g" % (I, H, max_len, drop), params, EDGE_CAPS, EDGE_LENS, max_len, dev,
                               keep, drop, seed=I + H)
    table = grads["encoder.weight"]
    used = {min(max(t, 0), 29) for b, n in enumerate(EDGE_LENS) for t in EDGE_CAPS[b, :n].tolist()}
    assert 9 not in used and 29 in used and 0 in used                            # 9 sits in the empty caption only
    for r in range(30):
        if r not in used:
            assert torch.equal(table[r], torch.zeros(I)), r                       # exactly zero, not NaN (poisoned allocator)
    for s in SUFFIXES:
        assert torch.equal(grads["rnn.bias_ih_l0" + s], grads["rnn.bias_hh_l0" + s])


# ---- batch independence and determinism ------------------------------------------------------------------------------
def _raw(params, caps, lens, max_len, rw, rs, dev, keep=None, scale=1.0):
    """the two launches without autograd -> (workspace sections, the five gradient stacks)"""
    from objgan_hip import ops
    wt_ih, wt_hh, b_ih, b_hh = _packed(params, dev)
    table, caps_d, lens_d = params["encoder.weight"].to(dev), caps.to(dev), torch.tensor(lens)
    keep = None if keep is None else keep.to(dev)
    _, _, ws = ops.lstm_bidir_train_forward(table, caps_d, lens_d, wt_ih, wt_hh, b_ih, b_hh, max_len, keep, scale)
    w_ih = torch.stack([params["rnn.weight_ih_l0" + s] for s in SUFFIXES]).to(dev)
    w_hh = torch.stack([params["rnn.weight_hh_l0" + s] for s in SUFFIXES]).to(dev)
    grads = ops.lstm_bidir_backward(rw.to(dev), rs.to(dev), caps_d, lens_d, w_ih, w_hh, ws, table.shape[0], max_len, keep,
                                    scale)
    torch.cuda.synchronize()
    B, L, I, H = caps.shape[0], caps.shape[1], table.shape[1], w_hh.shape[2]
    sec = {k: ops.lstm_train_ws_view(ws, k, B, L, I, H).cpu() for k in ops.lstm_train_ws_sections(B, L, I, H)[0]}
    return sec, [t.cpu() for t in grads]


def test_a_caption_does_not_depend_on_its_batch(dev):
    params = DO.seeded_text_params(30, 70, 20, 21)
    g = torch.Generator().manual_seed(22)
    rw, rs = torch.randn(5, 40, 7, generator=g), torch.randn(5, 40, generator=g)
    keep = (torch.rand(5, 7, 70, generator=g) >= 0.5).to(torch.uint8)
    full, _ = _raw(params, EDGE_CAPS, EDGE_LENS, 7, rw, rs, dev, keep, 2.0)
    for b in (0, 2, 3):
        one, _ = _raw(params, EDGE_CAPS[b:b + 1], EDGE_LENS[b:b + 1], 7, rw[b:b + 1], rs[b:b + 1], dev, keep[b:b + 1], 2.0)
        for k in ("gates", "cell", "hidden", "x", "dgate", "dx"):
            assert torch.equal(one[k][0], full[k][b]), (b, k)
    assert float(full["dgate"][4].abs().sum()) == 0 and float(full["dgate"][3, :, 1:].abs().sum()) == 0


def test_backward_is_deterministic(dev):
    """two runs: identical bits in the nine parameter gradients (table, 2 x weight_ih, 2 x weight_hh, 4 biases) and in
    the gate and input deltas"""
    params = DO.seeded_text_params(30, 300, 128, 31)
    g = torch.Generator().manual_seed(32)
    caps = torch.randint(1, 30, (5, 12), generator=g)
    lens = [12, 9, 5, 1, 0]
    rw, rs = torch.randn(5, 256, 12, generator=g), torch.randn(5, 256, generator=g)
    runs = []
    for _ in range(2):
        sec, grads = _raw(params, caps, lens, 12, rw, rs, dev)
        d_w_ih, d_w_hh, d_b_ih, d_b_hh, d_table = grads
        runs.append([d_table, d_w_ih[0], d_w_ih[1], d_w_hh[0], d_w_hh[1], d_b_ih[0], d_b_ih[1], d_b_hh[0], d_b_hh[1],
                     sec["dgate"], sec["dx"]])
    assert len(runs[0]) == 11
    for a, b in zip(*runs):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    used = {t for b, n in enumerate(lens) for t in caps[b, :n].tolist()}
    absent = [r for r in range(30) if r not in used]
    assert absent and float(runs[0][0][absent].abs().sum()) == 0 and not torch.isnan(runs[0][0]).any()


# ---- the whole step ------------------------------------------------------------------------------------------------------
class _Projections(torch.nn.Module):
    """the image encoder behind its frozen trunk: regions [B, 768, 17, 17] and pooled code [B, 2048] in, as CNN_ENCODER
    hands them to its two projections in pretraining"""

    def __init__(self, nef, seed):
        super().__init__()
        self.emb_features = torch.nn.Conv2d(768, nef, 1, bias=False)
        self.emb_cnn_code = torch.nn.Linear(2048, nef)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self.emb_features.weight.copy_(torch.randn(nef, 768, 1, 1, generator=g) / 768 ** 0.5)
            self.emb_cnn_code.weight.copy_(torch.randn(nef, 2048, generator=g) / 2048 ** 0.5)
            self.emb_cnn_code.bias.copy_(torch.randn(nef, generator=g) * 0.1)

    def forward(self, x):
        from objgan_hip import ops
        regions, code = x
        return (ops.conv2d(regions, self.emb_features.weight),
                ops.linear(code, self.emb_cnn_code.weight, self.emb_cnn_code.bias))


@pytest.fixture(scope="module")
def whole_step():
    """inputs and the fp64 restatement of the step at I = 300, H = 128, nef = 256, B = 4 (computed once)"""
    import numpy as np
    g = torch.Generator().manual_seed(41)
    params = DO.seeded_text_params(50, 300, 128, 42)
    caps = torch.randint(1, 50, (4, 12), generator=g)
    caps[1, 2] = caps[0, 2]
    lens = [12, 9, 6, 3]
    keep = (torch.rand(4, 12, 300, generator=g) >= 0.5).to(torch.uint8)
    regions = torch.relu(torch.randn(4, 768, 17, 17, generator=g))
    code = torch.relu(torch.randn(4, 2048, generator=g))
    proj = _Projections(256, 43)
    class_ids = np.asarray([5, 2, 5, 7])
    want = DO.step_ref(params, caps, lens, 12, regions, code, class_ids, keep, 0.5,
                       proj={k: v.detach() for k, v in proj.state_dict().items()})
    return {"params": params, "caps": caps, "lens": lens, "keep": keep, "regions": regions, "code": code,
            "proj": proj.state_dict(), "class_ids": class_ids, "want": want}


def _device_step(ws, dev, math):
    import damsm_trainer
    import model as M
    from miscc.utils import attach_host
    from objgan_hip import ops
    text = M.RNN_ENCODER(50, nhidden=256)
    text.load_state_dict(ws["params"], strict=True)
    text.fixed_keep_mask = ws["keep"].to(dev)
    proj = _Projections(256, 0)
    proj.load_state_dict(ws["proj"])
    tr = damsm_trainer.DAMSMTrainer('', None, None, dev, text.to(dev).train(), proj.to(dev))
    a = tr.arena
    before = a.flat.clone()
    lens = torch.tensor(ws["lens"])
    prev = ops.get_conv_math()
    ops.set_conv_math(math)
    try:
        four = tr.train_step((ws["regions"].to(dev), ws["code"].to(dev)), ws["caps"].to(dev),
                             attach_host(lens.to(dev), lens), ws["class_ids"])
        torch.cuda.synchronize()
    finally:
        ops.set_conv_math(prev)
    keys = ["text." + k for k, _ in text.named_parameters()] + list(damsm_trainer.PROJECTION_KEYS)
    grads = {k.replace("text.", ""): p.grad.detach().cpu() for k, p in zip(keys, a.params)}
    return {"losses": four.cpu().tolist(), "grads": grads, "before": before.cpu(), "after": a.flat.cpu(),
            "grad_flat": a.grad.cpu(), "m": a.exp_avg.cpu(), "v": a.exp_avg_sq.cpu(), "n_text": a.n_text,
            "clip_out": a.clip_out.cpu(), "lr": tr.lr, "clip": tr.clip, "state": [s.cpu() for s in a.state]}


def test_whole_step_against_the_restatement(dev, whole_step):
    want = whole_step["want"]
    errs = {}
    for math in ("fp32", "default"):
        from objgan_hip import ops
        r = _device_step(whole_step, dev, "fp32" if math == "fp32" else ops.get_conv_math())
        e = {"loss %d" % i: abs(g - w) / abs(w) for i, (g, w) in enumerate(zip(r["losses"], want["losses"]))}
        e.update({k: rel_l2(r["grads"][k], want["grads"][k]) for k in want["grads"]})
        assert set(want["grads"]) == set(DO.TEXT_KEYS) | {"emb_features.weight", "emb_cnn_code.weight", "emb_cnn_code.bias"}
        # clip and Adam: the fp64 rule applied to the device's own gradients
        nt, g = r["n_text"], r["grad_flat"].double()
        coef, norm = DO.clip_coef([g[:nt]], r["clip"])
        assert coef < 1.0, "the clip is meant to be active here"
        e["clip norm"] = abs(float(r["clip_out"][1]) - norm) / norm
        g = torch.cat((g[:nt] * coef, g[nt:]))
        zero = torch.zeros_like(g)
        p, m, v = DO.adam_ref(r["before"], g, zero, zero, r["lr"], 1)
        e["params"], e["m"], e["v"] = rel_l2(r["after"], p), rel_l2(r["m"], m), rel_l2(r["v"], v)
        # the update itself: p is rounded to fp32 after the subtraction, an error of ulp(p) / 2 per element against an
        # update of lr per element: (0.3 * 2^-24) / 0.002 ~ 1e-5 relative, well inside the bound
        e["update"] = rel_l2(r["after"].double() - r["before"].double(), p - r["before"].double())
        assert all(float(s[0]) == 1.0 for s in r["state"])
        for k, val in sorted(e.items()):
            note("damsm whole step (%s) vs fp64 restatement: %s" % (math, k), "%.3e" % val)
        errs[math] = e
    for k, v in errs["fp32"].items():
        assert v < BOUND, ("fp32", k, v)
    for k, v in errs["default"].items():
        # the default arithmetic meets the bound, or stays within 1.25 x of the fp32 run
        assert v < BOUND or v <= 1.25 * errs["fp32"][k], ("default", k, v, errs["fp32"][k])


# ---- launch refusals -------------------------------------------------------------------------------------------------
def test_launches_refuse_what_the_frozen_launch_refuses(dev):
    """4H > 1024 and an LDS overflow: OG_BAD_ARGS from the host check, before any launch (the operands are never read:
    one float each)"""
    from objgan_hip import _lib, ops
    one = torch.zeros(1, device=dev)
    caps = torch.zeros((1, 2), dtype=torch.int64, device=dev)
    lens = torch.ones(1, dtype=torch.int32, device=dev)
    p = ops._p
    lib = _lib.load()
    for I, H in ((4, 257), (16000, 128)):           # 4H = 1028; (16000 + 6 * 128) floats = 67072 bytes of LDS
        n = lib.objgan_lstm_bidir_train_ws_floats(1, 2, I, H)
        assert lib.objgan_lstm_bidir_forward(p(one), p(caps), p(lens), p(one), p(one), p(one), p(one), p(one), p(one),
                                             1, 2, 2, I, H, 5, ops._stream()) == 0
        assert lib.objgan_lstm_bidir_train_forward(p(one), p(caps), p(lens), None, 1.0, p(one), p(one), p(one), p(one),
                                                   p(one), p(one), p(one), n, 1, 2, 2, I, H, 5, ops._stream()) == 0
        assert lib.objgan_lstm_bidir_backward(p(one), p(one), p(caps), p(lens), None, 1.0, p(one), p(one), p(one), n,
                                              p(one), p(one), p(one), p(one), p(one), 1, 2, 2, I, H, 5, ops._stream()) == 0
    # a workspace that is too small is refused as well
    assert lib.objgan_lstm_bidir_train_forward(p(one), p(caps), p(lens), None, 1.0, p(one), p(one), p(one), p(one),
                                               p(one), p(one), p(one), 1, 1, 2, 2, 4, 8, 5, ops._stream()) == 0
    torch.cuda.synchronize()
    with pytest.raises(_lib.ObjganHipError):
        ops.lstm_bidir_train(torch.zeros(5, 4, device=dev), caps, lens, *[(torch.zeros(1028, 4, device=dev),) * 2,
                             (torch.zeros(1028, 257, device=dev),) * 2, (torch.zeros(1028, device=dev),) * 2,
                             (torch.zeros(1028, device=dev),) * 2], 2)


# ---- the command, end to end ---------------------------------------------------------------------------------------------
def test_pretrain_command_end_to_end(dev, tmp_path, monkeypatch, capsys):
    """pretrain_DAMSM.py on tests/golden/data_tiny with seeded trunk weights, 2 epochs at batch 4: the loss falls, the
    files load into condGANTrainer.build_models, and the loaded text encoder gives the training encoder's eval bits"""
    import encoders
    import pretrain_DAMSM
    import trainDataset
    import trainer as T
    from miscc.config import cfg
    for key in ("DATA_DIR", "WORKERS", "GPU_IDS", "CUDA"):
        monkeypatch.setitem(cfg, key, cfg[key])
    for key in ("BATCH_SIZE", "MAX_EPOCH", "SNAPSHOT_INTERVAL", "PRINT_INTERVAL", "NET_E", "NET_G", "FLAG"):
        monkeypatch.setitem(cfg.TRAIN, key, cfg.TRAIN[key])
    monkeypatch.setitem(cfg.TREE, "BRANCH_NUM", 1)
    # the command names its device through the environment (for the loader's workers); undone after the test
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", os.environ.get("CUDA_VISIBLE_DEVICES", "0"))
    rng = torch.random.get_rng_state()
    weights = tmp_path / "inception_v3.pth"
    torch.save(encoders.seeded_init_(encoders.inception_v3(), 3).state_dict(), weights)
    data = os.path.join(ROOT, "tests", "golden", "data_tiny")
    try:
        algo = pretrain_DAMSM.main(["--data_dir", data, "--output_dir", str(tmp_path), "--NET_INCEPTION", str(weights),
                                    "--BATCH_SIZE", "4", "--MAX_EPOCH", "2", "--manualSeed", "7", "--PRINT_INTERVAL", "1"])
    finally:
        torch.random.set_rng_state(rng)
    out = capsys.readouterr().out
    assert "validation skipped" in out and out.count("| end epoch") == 2
    first, second = (sum(four) for four in algo.epoch_losses)
    note("pretrain_DAMSM.py data_tiny: summed loss of epoch 1 and 2", "%.4f %.4f" % (first, second))
    assert second < first, (first, second)
    files = sorted(os.path.basename(f) for f in glob.glob(os.path.join(algo.model_dir, "*.pth")))
    assert files == ["image_encoder2.pth", "text_encoder2.pth"]

    cfg.TRAIN.NET_E = os.path.join(algo.model_dir, "text_encoder2.pth")
    cfg.TRAIN.NET_G = ''
    ds = trainDataset.TrainDataset(data, "train", base_size=64, device_hmaps=True)
    tr = T.condGANTrainer('', None, ds, device=dev)
    text, image = tr.build_models()[:2]
    assert not text.training and not any(p.requires_grad for p in list(text.parameters()) + list(image.parameters()))
    caps = torch.tensor([[1, 2, 3, 2, 0, 0, 0, 0, 0, 0, 0, 0], [3, 3, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]], device=dev)
    lens = torch.tensor([4, 3])
    trained = algo.text_encoder.eval()
    with torch.no_grad():
        a_w, a_s = text(caps, lens, 4)
        b_w, b_s = trained(caps, lens, 4)
    assert torch.equal(a_w, b_w) and torch.equal(a_s, b_s)
    for k in ("emb_features.weight", "emb_cnn_code.weight", "emb_cnn_code.bias"):
        assert torch.equal(image.state_dict()[k], algo.image_encoder.state_dict()[k])
    # and the encoders did move
    fresh = encoders.CNN_ENCODER(256)
    assert not torch.equal(image.state_dict()["emb_cnn_code.bias"].cpu(), fresh.state_dict()["emb_cnn_code.bias"])

"""DAMSM pretraining, the parts that need no GPU: the fp64 restatement (tests/damsm_oracle.py) against the recorded run
of the unmodified reference (tests/golden/damsm_ref.pt), the command's refusals, the learning-rate schedule, the
checkpoint key sets, and the untouched eval-mode RNN_ENCODER."""
import os

import pytest
import torch

import cpu_ops_shim
import damsm_oracle as DO
from conftest import ROOT, rel_l2

DATA = os.path.join(ROOT, "tests", "golden", "data_tiny")
BOUND = 1e-4            # the project's operator bound


@pytest.fixture(scope="module")
def golden():
    return DO.load_golden()


def test_restatement_meets_the_reference_golden(golden):
    c = golden["config"]
    r = DO.step_ref(golden["params"], golden["captions"], list(c["lens"]), c["L"], golden["feats"], golden["codes"],
                    c["class_ids"])
    assert rel_l2(r["words"], golden["words_emb"]) < BOUND and rel_l2(r["sent"], golden["sent_emb"]) < BOUND
    for got, want in zip(r["losses"], golden["losses"]):
        assert abs(got - want) <= BOUND * abs(want), (r["losses"], golden["losses"])
    assert set(golden["grads"]) == set(DO.TEXT_KEYS)
    for k in DO.TEXT_KEYS:
        assert rel_l2(r["grads"][k], golden["grads"][k]) < BOUND, k
    assert rel_l2(r["d_feats"], golden["d_feats"]) < BOUND and rel_l2(r["d_codes"], golden["d_codes"]) < BOUND
    # the golden is the case the issue describes: repeated tokens inside and across captions, one equal class pair
    caps, lens = golden["captions"], c["lens"]
    assert tuple(lens) == (7, 5, 5, 1) and len(set(c["class_ids"])) == len(c["class_ids"]) - 1
    words = [caps[b, :n].tolist() for b, n in enumerate(lens)]
    assert any(len(set(w)) < len(w) for w in words) and set(words[0]) & set(words[1]) & set(words[3])
    # bias_ih and bias_hh receive the same gradient, the sum of the gate deltas (the reference's two sums differ by rounding)
    for s in ("", "_reverse"):
        assert rel_l2(golden["grads"]["rnn.bias_ih_l0" + s], golden["grads"]["rnn.bias_hh_l0" + s]) < 1e-6


def test_restatement_edges_are_consistent():
    """length 0 contributes nothing, tokens are clamped, a keep-mask scales the survivors"""
    p = DO.seeded_text_params(9, 5, 3, 5)
    caps = torch.tensor([[1, 2, 3, 4], [100, -7, 0, 0], [5, 5, 5, 5]])
    g = torch.Generator().manual_seed(1)
    rw, rs = torch.randn(3, 6, 4, generator=g), torch.randn(3, 6, generator=g)
    a = DO.linear_probe_ref(p, caps, [4, 2, 0], 4, rw, rs)
    assert float(a["words"][2].abs().sum()) == 0 and float(a["sent"][2].abs().sum()) == 0
    assert float(a["grads"]["encoder.weight"][5].abs().sum()) == 0          # token 5 only in the empty caption
    b = DO.linear_probe_ref(p, torch.tensor([[1, 2, 3, 4], [8, 0, 0, 0], [5, 5, 5, 5]]), [4, 2, 0], 4, rw, rs)
    assert torch.equal(a["words"], b["words"])                                # 100 -> 8, -7 -> 0
    keep = torch.ones(3, 4, 5, dtype=torch.uint8)
    keep[0, 1] = 0
    k = DO.linear_probe_ref(p, caps, [4, 2, 0], 4, rw, rs, keep_mask=keep, p=0.5)
    x = DO.embed(p["encoder.weight"].double(), caps, keep, 0.5)
    assert float(x[0, 1].abs().sum()) == 0 and torch.equal(x[0, 0], p["encoder.weight"][1].double() * 2)
    assert not torch.equal(k["words"], a["words"])


def _refused(capsys, argv):
    import pretrain_DAMSM
    with pytest.raises(SystemExit) as e:
        pretrain_DAMSM.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err.strip()
    assert err.startswith("pretrain_DAMSM.py: ") and len(err.splitlines()) == 1, err
    return err


def test_command_refusals(tmp_path, capsys):
    weights = tmp_path / "inception.pth"
    weights.write_bytes(b"")
    assert "data directory" in _refused(capsys, ["--data_dir", str(tmp_path / "nowhere")])
    assert "Inception" in _refused(capsys, ["--data_dir", DATA])
    assert "Inception" in _refused(capsys, ["--data_dir", DATA, "--NET_INCEPTION", str(tmp_path / "missing.pth")])
    # the resume pair: both files must be there
    assert "pair" in _refused(capsys, ["--data_dir", DATA, "--NET_E", str(tmp_path / "text_encoder5.pth")])
    (tmp_path / "text_encoder5.pth").write_bytes(b"")
    err = _refused(capsys, ["--data_dir", DATA, "--NET_E", str(tmp_path / "text_encoder5.pth")])
    assert "image_encoder5.pth" in err
    assert "no device" in _refused(capsys, ["--data_dir", DATA, "--NET_INCEPTION", str(weights), "--gpu", "-1"])


def test_recipe_defaults_and_learning_rate_schedule():
    import damsm_trainer
    import pretrain_DAMSM
    a = pretrain_DAMSM.parse_args([])
    assert (a.BATCH_SIZE, a.ENCODER_LR, a.RNN_GRAD_CLIP, a.MAX_EPOCH, a.SNAPSHOT_INTERVAL, a.PRINT_INTERVAL) == (
        48, 0.002, 0.25, 600, 5, 200)
    assert damsm_trainer.BETAS == (0.5, 0.999)
    lr, got = a.ENCODER_LR, []
    for _ in range(a.MAX_EPOCH):
        got.append(lr)
        lr = damsm_trainer.next_lr(lr, a.ENCODER_LR)
    assert got == DO.lr_schedule(a.ENCODER_LR, a.MAX_EPOCH)
    assert got[0] == 0.002 and got[1] == 0.002 * 0.98
    # decays while above a tenth of the start, then stays: 0.98^114 is the first power at or below 0.1
    assert all(abs(v - 0.002 * 0.98 ** i) < 1e-15 for i, v in enumerate(got[:115]))
    assert got[113] > 0.0002 >= got[114] and set(got[114:]) == {got[114]}
    assert damsm_trainer.resume_epoch("/x/Model/text_encoder35.pth") == 35 and damsm_trainer.resume_epoch("enc.pth") == 0


def test_checkpoints_load_strictly_into_fresh_encoders(tmp_path):
    import damsm_trainer
    import encoders
    import model as M
    text = M.RNN_ENCODER(23, nhidden=256)
    image = encoders.CNN_ENCODER(256, encoders.seeded_init_(encoders.inception_v3(), 3)).eval()
    for k, p in image.named_parameters():
        p.requires_grad_(k in damsm_trainer.PROJECTION_KEYS)
    tr = damsm_trainer.DAMSMTrainer(str(tmp_path), None, None, torch.device("cpu"), text, image, max_epoch=2)
    a = tr.arena
    assert a.n_text == sum(p.numel() for p in text.parameters()) and a.n == a.n_text + 768 * 256 + 2048 * 256 + 256
    assert all(p.data_ptr() == a.flat[o:].data_ptr() for p, o in ((a.params[0], 0), (a.params[-3], a.n_text)))
    with torch.no_grad():
        a.flat.mul_(1.5)                                    # what the optimiser does: through the arena
    tr.save(2)
    sd_t = torch.load(tmp_path / "Model" / "text_encoder2.pth")
    sd_i = torch.load(tmp_path / "Model" / "image_encoder2.pth")
    assert set(sd_t) == set(DO.TEXT_KEYS)
    assert all(v.untyped_storage().nbytes() == v.numel() * v.element_size() for v in sd_t.values())   # no arena views
    fresh_t = M.RNN_ENCODER(23, nhidden=256)
    fresh_i = encoders.CNN_ENCODER(256)
    fresh_t.load_state_dict(sd_t, strict=True)
    fresh_i.load_state_dict(sd_i, strict=True)
    for k, v in text.state_dict().items():
        assert torch.equal(fresh_t.state_dict()[k], v), k
    for k in damsm_trainer.PROJECTION_KEYS:
        assert torch.equal(fresh_i.state_dict()[k], image.state_dict()[k]), k
    assert not fresh_i.train_projections and fresh_t.fixed_keep_mask is None


def test_eval_mode_rnn_encoder_is_unchanged(monkeypatch):
    """eval mode: the frozen launch (here its CPU shim), whatever drop_prob"""
    import model as M
    cpu_ops_shim.install(monkeypatch)
    p = DO.seeded_text_params(30, 300, 128, 3)
    enc = M.RNN_ENCODER(30, nhidden=256)
    enc.load_state_dict(p, strict=True)
    enc.eval()
    caps = torch.tensor([[3, 7, 7, 12, 3, 29, 5, 0, 0, 0, 0, 0], [7, 1, 12, 12, 28, 0, 0, 0, 0, 0, 0, 0]])
    lens = torch.tensor([7, 5])
    with torch.no_grad():
        words, sent = enc(caps, lens, 7)
    want_w, want_s = DO.encode({k: v.double() for k, v in p.items()}, caps, [7, 5], 7)
    assert words.shape == (2, 256, 7) and sent.shape == (2, 256) and not words.requires_grad
    assert rel_l2(words, want_w) < 1e-5 and rel_l2(sent, want_s) < 1e-5
    assert float(words[1, :, 5:].abs().sum()) == 0


def test_training_mode_has_no_cpu_path():
    """training mode no longer raises NotImplementedError: it goes to the trainable kernel, which refuses CPU tensors"""
    import model as M
    from objgan_hip import _lib
    enc = M.RNN_ENCODER(30, ninput=20, drop_prob=0, nhidden=16).train()
    with pytest.raises(_lib.ObjganHipError, match="no CPU path"):
        enc(torch.tensor([[3, 7, 0], [7, 0, 0]]), torch.tensor([2, 1]), 2)


def test_header_declares_the_training_entry_points():
    from objgan_hip import _lib
    assert len(_lib.SIGNATURES["objgan_lstm_bidir_train_forward"]) == 20
    assert len(_lib.SIGNATURES["objgan_lstm_bidir_backward"]) == 22
    assert len(_lib.LONG_RETURN["objgan_lstm_bidir_train_ws_floats"]) == 4

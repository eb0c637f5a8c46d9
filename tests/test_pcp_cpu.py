"""The shape generator's perceptual term without a GPU: the fp64 oracle (tests/pcp_oracle.py) against the reference
golden, the BatchNorm fold, state-dict handling, the refusals, the host side of the trainer (score file, print line) on
CPU definitions of the new operators, the C-ABI.

Observed, oracle (fp64) vs the reference's fp32 CPU run (tests/golden/pcp_ref.pt, case thin512): errG / pcp_score 1.3e-7,
per-tap means 3.4e-7, clipped generator gradient 2.9e-6; the mask gradient d errG / d fake_hmaps is stored with its own
floor (ReLU / sign / argmax decisions that differ between the fp32 and the fp64 run)."""
import os
import re
import shutil

import pytest
import torch

from conftest import ROOT, rel_l2, note
import shapegen_oracle as so
import pcp_oracle as po
import pcp_cpu_ops

GOLD = os.path.join(ROOT, "tests", "golden", "pcp_ref.pt")
TINY = os.path.join(ROOT, "tests", "golden", "shape_tiny")


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, map_location="cpu", weights_only=False)


def seeded_nets(nbf):
    import model
    from miscc.config import cfg
    cfg.GAN.R_NUM = 1
    return (so.seeded_state_(model.SHP_G_NET(nbf), so.SEEDS["G"]),
            so.seeded_state_(model.INS_D_NET(nbf), so.SEEDS["INSD"]),
            so.seeded_state_(model.GLB_D_NET(nbf), so.SEEDS["GLBD"]))


def test_oracle_matches_reference_golden(gold):
    c = gold["cases"]["thin512"]
    assert gold["seeds"]["VGG"] == po.SEED_VGG and gold["lambda"] == po.LAMBDA
    nbf = c["nbf"]
    G, I, L = seeded_nets(nbf)
    x = so.make_inputs(c["shapegen_case"])
    o = po.oracle_step(G.state_dict(), I.state_dict(), L.state_dict(), po.seeded_vgg(c["widths"]), x)
    e_loss = max(abs(float(o["errG"]) - c["errG"]) / abs(c["errG"]),
                 abs(float(o["gpcp_loss"]) - c["gpcp_loss"]) / abs(c["gpcp_loss"]),
                 abs(float(o["pcp_score"]) - c["item_pcp_score"]) / abs(c["item_pcp_score"]))
    e_taps = float(((o["taps"] - c["taps"].double()).abs() / c["taps"].double().abs()).max())
    e_dfake = rel_l2(c["dfake"], o["dfake"])
    keys = list(c["gradG_clipped"])
    worst = rel_l2(torch.cat([so.sample(o["gradG"][k] / o["divisor"]) for k in keys]),
                   torch.cat([c["gradG_clipped"][k]["sample"] for k in keys]))
    e_norm = abs(o["normG"] - c["normG"]) / c["normG"]
    note("pcp oracle vs reference thin512 loss / taps / dfake / G grads / G norm",
         "%.3g %.3g %.3g %.3g %.3g" % (e_loss, e_taps, e_dfake, worst, e_norm))
    print("loss", e_loss, "taps", e_taps, "dfake", e_dfake, "gradG", worst, "norm", e_norm, "floor", c["floor"])
    assert e_loss <= 1e-5 and e_taps <= 1e-5
    assert e_dfake <= 4 * c["floor"]["dfake"]
    assert e_norm <= 4 * c["floor"]["normG"]
    assert worst <= 4 * c["floor"]["gradG_samples"]


def test_golden_respects_its_conditions(gold):
    bound = {"thin512": 1e-4, "full": 1e-2}
    for case, c in gold["cases"].items():
        assert c["smallest_gap"] > 0, case
        assert max(c["floor"]["dfake"], c["floor"]["gradG"]) <= bound[case], (case, c["floor"])
        assert c["taps"].numel() == 19


def test_batchnorm_fold_in_fp64_against_the_unfolded_evaluation():
    import model
    sd = po.seeded_vgg("thin")
    layers = model.vgg_fold(sd)
    convs = [l for l in layers if l[0] == "conv"]
    idx = sorted(int(k.split(".")[1]) for k, v in sd.items() if k.startswith("features.") and v.dim() == 4)
    assert len(convs) == len(idx) == 16
    for (_, w, b), i in zip(convs, idx):                       # every element: ONE rounding of the fp64 formula
        p = "features.%d." % (i + 1)
        k = sd[p + "weight"].double() / torch.sqrt(sd[p + "running_var"].double() + 1e-5)
        w64 = sd["features.%d.weight" % i].double() * k.view(-1, 1, 1, 1)
        b64 = (sd["features.%d.bias" % i].double() - sd[p + "running_mean"].double()) * k + sd[p + "bias"].double()
        assert w.dtype == torch.float32 and torch.equal(w, w64.float()) and torch.equal(b, b64.float())
    # and the folded chain against the unfolded network, both evaluated in fp64
    g = torch.Generator().manual_seed(5)
    x = po.normalise(torch.rand(2, 1, 64, 64, generator=g, dtype=torch.float64))
    want = po.vgg_features(sd, x)
    y = torch.nn.functional.interpolate(x, size=(224, 224), mode="bilinear", align_corners=True)
    got = []
    for layer in layers:
        if layer[0] == "pool":
            y = torch.nn.functional.max_pool2d(y, 2, 2)
        elif layer[0] == "conv":
            y = torch.relu(torch.nn.functional.conv2d(y, layer[1].double(), layer[2].double(), 1, 1))
            got.append(y)
        else:
            y = torch.nn.functional.conv2d(y.reshape(y.shape[0], -1, 1, 1), layer[1].double(), layer[2].double())
            y = torch.relu(y) if layer[3] else y
            got.append(y.reshape(y.shape[0], -1))
    assert len(got) == len(want) == 19
    worst = max(rel_l2(a, b) for a, b in zip(got, want))
    print("folded vs unfolded, worst tap", worst)
    assert worst <= 2e-6                                       # 19 layers of fp32-rounded weights (6e-8 each)


def test_state_dict_keys_and_dimension_inference():
    import model
    from objgan_hip._lib import ObjganHipError
    for name in ("thin", "thin512"):
        feats, cls = po.WIDTHS[name]
        sd = po.empty_state(name)
        plan = model.vgg_plan(sd)
        kinds = [p[0] for p in plan]
        assert kinds == ["pool" if v == "M" else "conv" for v in feats] + ["fc"] * 3
        assert [p[1] for p in plan if p[0] == "conv"] == [0, 3, 7, 10, 14, 17, 20, 23, 27, 30, 33, 36, 40, 43, 46, 49]
        assert [p[1:] for p in plan if p[0] == "fc"] == [(0, True), (3, True), (6, False)]
        net = model.VGG(po.seeded_vgg(name) if name == "thin" else sd)
        assert net.num_taps == 19 and not net.training and not list(net.parameters())
        fcs = [l for l in net.layers() if l[0] == "fc"]
        c5 = [v for v in feats if v != "M"][-1]
        assert tuple(fcs[0][1].shape) == (cls[0], c5 * 7 * 7, 1, 1) and tuple(fcs[2][1].shape) == (cls[2], cls[1], 1, 1)
        assert net.train().training is False
    # torchvision's own layout: the same index pattern as the thin networks, 512 * 7 * 7 -> 4096
    full_feats = po.WIDTHS["full"][0]
    assert [v == "M" for v in full_feats] == [v == "M" for v in po.WIDTHS["thin"][0]]
    # a network with FOUR pools in its features and a 14 x 14 map into the classifier is read off the tensors too
    sd = po.empty_state("thin")
    sd["classifier.0.weight"] = torch.zeros(64, 24 * 14 * 14)
    assert [p[0] for p in model.vgg_plan(sd)].count("pool") == 4
    sd = po.empty_state("thin")
    del sd["features.1.running_var"]
    with pytest.raises(ObjganHipError, match="features.1.running_var"):
        model.vgg_plan(sd)
    sd = po.empty_state("thin")
    sd["classifier.0.weight"] = torch.zeros(64, 1000)
    with pytest.raises(ObjganHipError, match="classifier.0.weight"):
        model.vgg_plan(sd)
    sd = po.empty_state("thin")
    sd["classifier.3.weight"] = torch.zeros(48, 63)
    with pytest.raises(ObjganHipError, match="classifier.3.weight"):
        model.vgg_plan(sd)
    with pytest.raises(ObjganHipError):
        model.vgg_plan({})


def test_vgg_norm_is_the_references():
    from miscc.utils import vgg_norm
    x = torch.rand(2, 3, 5, 5)
    assert torch.equal(vgg_norm(x[:, :1].repeat(1, 3, 1, 1)), po.normalise(x[:, :1]))


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_refusal_missing_weights_file(tmp_path):
    from miscc.shape_losses import check_pcp_lambda
    from objgan_hip._lib import ObjganHipError
    path = str(tmp_path / "pretrained" / "vgg19_bn-c79401a0.pth")
    with pytest.raises(ObjganHipError) as e:
        check_pcp_lambda(10.0, path)
    assert path in str(e.value) and "not built without" in str(e.value) and "--PCP_LAMBDA 0" in str(e.value)
    with pytest.raises(ObjganHipError):
        check_pcp_lambda(10.0)
    check_pcp_lambda(0.0, path)                                # nothing to load: fine
    os.makedirs(os.path.dirname(path))
    open(path, "wb").close()
    check_pcp_lambda(10.0, path)


def _loss_args(monkeypatch, lam):
    pcp_cpu_ops.install(monkeypatch)
    from miscc.config import cfg
    monkeypatch.setitem(cfg.TRAIN.SMOOTH, "PCP_LAMBDA", lam)
    monkeypatch.setitem(cfg.TRAIN.SMOOTH, "INS_LAMBDA", 1.0)
    monkeypatch.setitem(cfg.TRAIN.SMOOTH, "GLB_LAMBDA", 1.0)
    x = so.make_inputs("r1")
    _, I, L = seeded_nets(16)
    return I, L, x


def test_refusal_model_with_zero_lambda(monkeypatch):
    import model
    from miscc.shape_losses import generator_loss
    from objgan_hip._lib import ObjganHipError
    I, L, x = _loss_args(monkeypatch, 0.0)
    with pytest.raises(ObjganHipError, match="PCP_LAMBDA is 0"):
        generator_loss(I, L, model.VGG(po.seeded_vgg("thin")), x["real"], x["real"], x["fwd"])
    out = generator_loss(I, L, None, x["real"], x["real"], x["fwd"])          # and the old form is unchanged
    assert len(out) == 2 and len(out[1]) == 2


def test_refusal_lambda_without_model(monkeypatch):
    from miscc.shape_losses import generator_loss
    from objgan_hip._lib import ObjganHipError
    I, L, x = _loss_args(monkeypatch, 10.0)
    with pytest.raises(ObjganHipError, match="vgg_model is None"):
        generator_loss(I, L, None, x["real"], x["real"], x["fwd"])


# ---------------------------------------------------------------------------------------------
# host side of the trainer
# ---------------------------------------------------------------------------------------------
def make_trainer(monkeypatch, tmp_path, nbf, B, vgg_sd):
    import model
    pcp_cpu_ops.install(monkeypatch)
    import shape_trainer
    from miscc.config import cfg
    monkeypatch.setitem(cfg.TRAIN, "BATCH_SIZE", B)
    monkeypatch.setitem(cfg.TRAIN, "FLAG", True)
    monkeypatch.setitem(cfg.TRAIN.SMOOTH, "PCP_LAMBDA", po.LAMBDA)
    monkeypatch.setitem(cfg.TRAIN.SMOOTH, "INS_LAMBDA", 1.0)
    monkeypatch.setitem(cfg.TRAIN.SMOOTH, "GLB_LAMBDA", 1.0)
    ds = type("DS", (), {"cats_dict": {}, "cats_index_dict": {i: i for i in range(nbf)}})()
    t = shape_trainer.condGANTrainer(str(tmp_path), None, ds, device="cpu")
    t.attach(*seeded_nets(nbf), vgg=model.VGG(vgg_sd))
    return t


def batch_of(x):
    return {"max_num_roi": x["z"].shape[1], "bbox_maps_fwd": x["fwd"], "bbox_maps_bwd": x["bwd"], "bbox_fmaps": x["fmaps"],
            "hmaps": x["real"], "pooled_hmaps": x["real_pooled"]}


def test_host_step_against_oracle_and_score_file(monkeypatch, tmp_path):
    case = "b2r3"
    nbf, B, R = so.CASES[case]
    x = so.make_inputs(case)
    sdV = po.seeded_vgg("thin")
    t = make_trainer(monkeypatch, tmp_path, nbf, B, sdV)
    want = po.oracle_step(t.netG.state_dict(), t.netINSD.state_dict(), t.netGLBD.state_dict(), sdV, x)
    t.define_optimizers(1.0)
    out = t.train_step(batch_of(x), noise=x["z"])
    for k in ("errG", "gpcp_loss", "pcp_score", "insg_loss", "glbg_loss"):
        assert abs(float(out[k]) - float(want[k])) <= 1e-5 * abs(float(want[k])), k
    assert abs(float(out["gpcp_loss"]) - po.LAMBDA * float(out["pcp_score"])) <= 1e-6 * float(out["gpcp_loss"])
    assert abs(float(out["clip"][1]) - want["normG"]) <= 2e-3 * want["normG"]
    first = t.write_score(0)
    assert first == pytest.approx(float(out["pcp_score"]), rel=1e-6)
    text = open(os.path.join(str(tmp_path), "Score", "scores_0.txt")).read()
    assert re.fullmatch(r"pcp_score -?\d+\.\d{6}", text) and float(text.split()[1]) == pytest.approx(first, abs=1e-6)
    # a new epoch re-creates the optimizers; the score goes on from where it was (the reference never resets it)
    t.define_optimizers(1.0)
    out2 = t.train_step(batch_of(x), noise=x["z"])
    second = t.write_score(1)
    assert second == pytest.approx(first + float(out2["pcp_score"]), rel=1e-6) and second > first
    assert os.path.exists(os.path.join(str(tmp_path), "Score", "scores_1.txt"))


def test_train_loop_prints_and_writes_like_the_reference(monkeypatch, tmp_path, capsys):
    import shapeDataset
    import shape_trainer
    from miscc.config import cfg
    pcp_cpu_ops.install(monkeypatch)
    data = str(tmp_path / "data")
    shutil.copytree(TINY, data)
    os.makedirs(os.path.join(data, "pretrained"))
    torch.save(po.seeded_vgg("thin"), os.path.join(data, "pretrained", "vgg19_bn-c79401a0.pth"))
    for key, val in (("BATCH_SIZE", 2), ("FLAG", True), ("MAX_EPOCH", 2), ("NET_G", ""), ("PRINT_INTERVAL", 2),
                     ("SNAPSHOT_INTERVAL", 5), ("RNN_GRAD_CLIP", 0.25)):
        monkeypatch.setitem(cfg.TRAIN, key, val)
    for key, val in (("PCP_LAMBDA", 10.0), ("INS_LAMBDA", 1.0), ("GLB_LAMBDA", 1.0)):
        monkeypatch.setitem(cfg.TRAIN.SMOOTH, key, val)
    monkeypatch.setitem(cfg, "DATA_DIR", data)
    monkeypatch.setitem(cfg.GAN, "R_NUM", 1)
    torch.manual_seed(3)
    ds = shapeDataset.TextDataset(data, "train", base_size=64)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, drop_last=True, shuffle=False)
    t = shape_trainer.condGANTrainer(str(tmp_path / "out"), loader, ds, device="cpu")
    t.train()
    text = capsys.readouterr().out
    assert "Not built" in text and "perceptual" not in text.split("Not built", 1)[1].splitlines()[0]
    logs = [l for l in text.splitlines() if l.startswith("insg_loss:")]
    assert logs and all(re.fullmatch(r"insg_loss: \S+ glbg_loss: \S+ gpcp_loss: -?\d+\.\d\d ", l) for l in logs), logs
    scores = [float(l.split()[1]) for l in text.splitlines() if l.startswith("pcp_score: ")]
    assert len(scores) == 2 and 0 < scores[0] < scores[1]
    for epoch in range(2):
        m = re.fullmatch(r"pcp_score (\d+\.\d{6})", open(os.path.join(str(tmp_path / "out"), "Score", "scores_%d.txt" % epoch)).read())
        assert m and float(m.group(1)) == pytest.approx(scores[epoch], abs=1e-5)
    assert {"netG_epoch_0.pth", "netG_epoch_2.pth"} <= set(os.listdir(t.model_dir))


def test_c_abi_exports_the_perceptual_symbols():
    from objgan_hip import _lib
    names = ("objgan_pcp_stem_forward", "objgan_pcp_stem_backward", "objgan_l1_tap_forward", "objgan_l1_tap_backward")
    header = open(os.path.join(ROOT, "include", "objgan_hip.h")).read()
    lib = _lib.load(build_if_missing=False)
    for name in names:
        assert "int %s(" % name in header, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert "long objgan_l1_tap_ws_doubles(" in header and "objgan_l1_tap_ws_doubles" in _lib.LONG_RETURN
    assert len(_lib.SIGNATURES["objgan_l1_tap_forward"]) == 7 and len(_lib.SIGNATURES["objgan_l1_tap_backward"]) == 9
    assert lib.objgan_l1_tap_ws_doubles(5) >= 1 and lib.objgan_l1_tap_ws_doubles(0) == 0

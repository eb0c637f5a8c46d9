"""Shape generator training without a GPU: the fp64 oracle against the reference golden, the host side of the step
(trainer, arenas, losses, data set) on CPU definitions against the oracle, the command line's refusals, the C-ABI.

Observed, oracle (fp64) vs the reference's fp32 CPU run (tests/golden/shapegen_train_ref.pt), worst of the four cases:
masks 4.3e-7, losses 1.1e-6, discriminator gradient tensors 5.1e-6, clipped generator gradient tensors 9.2e-5 (the
nbf = 80 case; 4.9e-6 at nbf = 16), generator gradient norm 8.9e-5 (bounds 1e-5 / 1e-5 / 2e-3 / 2e-3 / 2e-3)."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_l2, note
import shapegen_oracle as so
import shapegen_cpu_ops

GOLD = os.path.join(ROOT, "tests", "golden", "shapegen_train_ref.pt")
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


def oracle_step(case):
    nbf = so.CASES[case][0]
    G, I, L = seeded_nets(nbf)
    x = so.make_inputs(case)
    tr = so.OracleTrainer(G.state_dict(), I.state_dict(), L.state_dict())
    return tr, tr.step(x["z"], x["fwd"], x["bwd"], x["fmaps"], x["real"], x["real_pooled"]), x


def check_grads(got, want, bound, tag, scale=1.0):
    worst = 0.0
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k] / scale
        e = rel_l2(so.sample(g), w["sample"])
        en = abs(float(g.double().norm()) - w["norm"]) / max(w["norm"], 1e-30)
        worst = max(worst, e, en)
        assert e <= bound and en <= bound, (tag, k, e, en)
    return worst


@pytest.mark.parametrize("case", list(so.CASES))
def test_oracle_matches_reference_golden(gold, case):
    c = gold["cases"][case]
    _, out, _ = oracle_step(case)
    e_mask = rel_l2(out["fake_hmaps"][..., ::2, ::2], c["fake_hmaps_s2"])
    e_loss = max(abs(float(out[k]) - c[k]) / abs(c[k]) for k in ("errINSD", "errGLBD", "errG"))
    note("shapegen oracle vs reference %s masks / losses" % case, "%.3g %.3g" % (e_mask, e_loss))
    print(case, "masks", e_mask, "losses", e_loss)
    assert e_mask <= 1e-5 and e_loss <= 1e-5
    wd = max(check_grads(out["gradINSD"], c["gradINSD"], 2e-3, case + " INSD"),
             check_grads(out["gradGLBD"], c["gradGLBD"], 2e-3, case + " GLBD"))
    wg = check_grads(out["gradG"], c["gradG_clipped"], 2e-3, case + " G", scale=out["divisor"])
    e_norm = abs(out["normG"] - c["normG"]) / c["normG"]
    note("shapegen oracle vs reference %s D grads / G grads / G norm" % case, "%.3g %.3g %.3g" % (wd, wg, e_norm))
    print(case, "D grads", wd, "G grads", wg, "norm", e_norm)
    assert e_norm <= 2e-3


def test_golden_respects_the_max_condition(gold):
    for case, c in gold["cases"].items():
        assert c["near_tie_share"] <= 0.005 and c["smallest_gap"] > 0, case


def make_trainer(monkeypatch, tmp_path, nbf, B):
    shapegen_cpu_ops.install(monkeypatch)
    import shape_trainer
    from miscc.config import cfg
    monkeypatch.setitem(cfg.TRAIN, "BATCH_SIZE", B)
    monkeypatch.setitem(cfg.TRAIN, "FLAG", True)
    monkeypatch.setitem(cfg.TRAIN.SMOOTH, "PCP_LAMBDA", 0.0)
    monkeypatch.setitem(cfg.TRAIN.SMOOTH, "INS_LAMBDA", 1.0)
    monkeypatch.setitem(cfg.TRAIN.SMOOTH, "GLB_LAMBDA", 1.0)
    ds = type("DS", (), {"cats_dict": {}, "cats_index_dict": {i: i for i in range(nbf)}})()
    t = shape_trainer.condGANTrainer(str(tmp_path), None, ds, device="cpu")
    t.attach(*seeded_nets(nbf))
    return t


def batch_of(x):
    return {"max_num_roi": x["z"].shape[1], "bbox_maps_fwd": x["fwd"], "bbox_maps_bwd": x["bwd"], "bbox_fmaps": x["fmaps"],
            "hmaps": x["real"], "pooled_hmaps": x["real_pooled"]}


def test_host_step_two_epochs_against_oracle(monkeypatch, tmp_path):
    """two consecutive steps with an epoch boundary between them: the second starts from zero moments and step 1"""
    case = "b2r3"
    nbf, B, R = so.CASES[case]
    x = so.make_inputs(case)
    t = make_trainer(monkeypatch, tmp_path, nbf, B)
    orc = so.OracleTrainer(t.netG.state_dict(), t.netINSD.state_dict(), t.netGLBD.state_dict())
    keysG = [k for k, _ in t.netG.named_parameters()]

    def flat(d, keys):
        return torch.cat([d[k].reshape(-1) for k in keys])

    for epoch in range(2):
        t.define_optimizers(1.0)
        orc.new_epoch(1.0)
        before = t.arenaG.flat.double().clone()
        avg_before = t.avg_param_G.double().clone()
        out = t.train_step(batch_of(x), noise=x["z"])
        want = orc.step(x["z"], x["fwd"], x["bwd"], x["fmaps"], x["real"], x["real_pooled"])
        for k in ("errINSD", "errGLBD", "errG"):
            assert abs(float(out[k]) - float(want[k])) <= 1e-5 * abs(float(want[k])), (epoch, k)
        assert rel_l2(out["fake_hmaps"], want["fake_hmaps"]) <= 1e-5
        # gradients and the clip, against the oracle's
        g = t.arenaG.grad[:t.arenaG.n].double()
        assert rel_l2(g, flat(want["gradG"], keysG)) <= 2e-3
        assert abs(float(out["clip"][1]) - want["normG"]) <= 2e-3 * want["normG"]
        assert abs(float(out["clip"][0]) - want["divisor"]) <= 2e-3 * want["divisor"]
        # a fresh optimizer: step 1, moments (1 - beta) g and (1 - beta2) g^2 of THIS step's clipped gradient alone
        assert t.optimizerG.state.tolist() == [1.0, 0.5, 0.999], epoch
        assert t.optimizerINSD.steps_taken == 1 and t.optimizerGLBD.steps_taken == 1
        gc = g / float(out["clip"][0])
        assert rel_l2(t.arenaG.exp_avg, 0.5 * gc) <= 1e-5
        assert rel_l2(t.arenaG.exp_avg_sq, 0.001 * gc * gc) <= 1e-5
        # Adam and the EMA copy, against the fp64 rule applied to the trainer's own gradient
        p1, _, _ = so.adam(before, gc, torch.zeros_like(gc), torch.zeros_like(gc), 1, 2e-4)
        assert rel_l2(t.arenaG.flat.double() - before, p1 - before) <= 1e-4
        # (the EMA moves a weight by 1e-3 of an Adam step, below fp32's resolution of the weight: compare values, at a
        # few fp32 roundings, and make sure that bound tells a moved average from an unmoved one)
        want_avg = so.ema(avg_before, p1)
        assert rel_l2(t.avg_param_G, want_avg) <= 2e-7 < 1e-6 < rel_l2(avg_before, want_avg) * (1 + 9 * epoch)
        # and the discriminators' state against the oracle's after its own updates
        for net, i in ((t.netINSD, 1), (t.netGLBD, 2)):
            for k, p in net.named_parameters():
                assert float((p.detach().double() - orc.sd[i][k]).abs().max()) <= 2.5e-4 * 2, (epoch, k)   # |update| <= lr per element
            assert rel_l2(torch.cat([p.grad.reshape(-1) for p in net.parameters()]),
                          flat(want["gradINSD" if i == 1 else "gradGLBD"], [k for k, _ in net.named_parameters()])) <= 2e-3
        # the oracle goes on from the trainer's weights (fp32 Adam steps of +-lr do not follow an fp64 run element-wise)
        for sd, net in zip(orc.sd, (t.netG, t.netINSD, t.netGLBD)):
            for k, p in net.named_parameters():
                sd[k] = p.detach().double().clone()


def load_tiny():
    import shapeDataset
    return shapeDataset.TextDataset(TINY, "train", base_size=64)


def test_dataset_box_maps_reversed_over_ten_then_cut(monkeypatch):
    shapegen_cpu_ops.install(monkeypatch)
    import shapeDataset
    ds = load_tiny()
    assert len(ds) == 6 and len(ds.cats_index_dict) == 16
    nums = [int(ds.insanns_dict[k]["num_rois"]) for k in ds.filenames]
    assert nums[0] == 0 and nums[1] == 10 and 2 in nums
    collate = torch.utils.data.default_collate
    for idx in (0, 1, nums.index(2)):
        other = 1 if idx == 0 else idx          # a batch needs one box: pair the empty image with the full one
        items = [ds[idx], ds[other]]
        batch = collate(items)
        out = shapeDataset.prepare_data(batch, "cpu", 16)
        R = out["max_num_roi"]
        raw = np.stack([it[2] for it in items])
        cats = np.stack([it[3] for it in items])
        fwd, bwd = so.np_boxmaps(raw, cats, [it[7] for it in items], R, 16)
        assert np.array_equal(out["bbox_maps_fwd"].numpy(), fwd) and np.array_equal(out["bbox_maps_bwd"].numpy(), bwd)
        # the reference's host form of the same image
        host = shapeDataset.get_hmaps_rois(ds.insanns_dict[ds.filenames[idx]], 64, 16, ds.cats_index_dict)
        assert np.array_equal(host[2][:R].astype(np.float32), fwd[0]) and np.array_equal(host[3][:R].astype(np.float32), bwd[0])
        assert np.array_equal(out["hmaps"][0, :, 0].numpy(), host[1][:R].astype(np.float32))
        assert np.array_equal(out["pooled_hmaps"][0, 0].numpy(), host[0].astype(np.float32))
        if 0 < nums[idx] < 10 and R < 10:
            assert not bwd[0].any() or R > 10 - nums[idx]       # leading zero maps: the boxes sit at the far end of 10 slots
    with pytest.raises(ValueError):
        shapeDataset.prepare_data(collate([ds[0], ds[0]]), "cpu", 16)


def test_checkpoint_loads_into_shp_g_net(monkeypatch, tmp_path):
    import model
    case = "r1"
    nbf, B, R = so.CASES[case]
    x = so.make_inputs(case)
    t = make_trainer(monkeypatch, tmp_path, nbf, B)
    t.define_optimizers(1.0)
    t.train_step(batch_of(x), noise=x["z"])
    live = t.arenaG.flat.clone()
    t.save_model(3)
    assert torch.equal(t.arenaG.flat, live)                          # the live weights are back
    assert set(os.listdir(os.path.join(str(tmp_path), "Model"))) == {"netG_epoch_3.pth", "netGLBD.pth", "netINSD.pth"}
    sd = torch.load(os.path.join(str(tmp_path), "Model", "netG_epoch_3.pth"), map_location="cpu")
    net = model.SHP_G_NET(nbf)
    net.load_state_dict(sd, strict=True)
    assert torch.equal(torch.cat([p.reshape(-1) for p in net.parameters()]), t.avg_param_G)     # the EMA copy
    assert not torch.equal(t.avg_param_G, live)
    model.INS_D_NET(nbf).load_state_dict(torch.load(os.path.join(str(tmp_path), "Model", "netINSD.pth")), strict=True)
    model.GLB_D_NET(nbf).load_state_dict(torch.load(os.path.join(str(tmp_path), "Model", "netGLBD.pth")), strict=True)


def test_discriminator_keys_are_the_references():
    import model
    want = ["downsample%d.0.weight" % i for i in range(1, 5)] + ["get_logits.outlogits.0.weight", "get_logits.outlogits.0.bias"]
    for cls in (model.INS_D_NET, model.GLB_D_NET):
        sd = cls(80).state_dict()
        assert sorted(sd) == sorted(want)
        assert tuple(sd["downsample1.0.weight"].shape) == (40, 81, 4, 4)
        assert tuple(sd["downsample4.0.weight"].shape) == (5, 10, 4, 4)
        assert tuple(sd["get_logits.outlogits.0.weight"].shape) == (1, 5, 4, 4)


def test_command_line_refusals(capsys):
    import shape_main
    from objgan_hip._lib import ObjganHipError
    with pytest.raises(ObjganHipError) as e:
        shape_main.main(["--FLAG", "--PCP_LAMBDA", "10", "--data_dir", TINY])
    assert "--PCP_LAMBDA 0" in str(e.value) and "not built" in str(e.value)
    with pytest.raises(ObjganHipError):
        shape_main.main(["--FLAG", "--data_dir", TINY])               # the reference's default is 10
    with pytest.raises(SystemExit) as e:
        shape_main.main(["--PCP_LAMBDA", "0", "--data_dir", TINY])
    assert isinstance(e.value.code, str) and "\n" not in e.value.code and "--FLAG" in e.value.code


def test_c_abi_exports_the_new_symbols():
    import ctypes
    from objgan_hip import _lib
    names = ("objgan_convlstm_cell_forward", "objgan_convlstm_cell_backward", "objgan_box_max_forward",
             "objgan_box_max_backward", "objgan_boxmaps_onehot")
    header = open(os.path.join(ROOT, "include", "objgan_hip.h")).read()
    lib = _lib.load(build_if_missing=False)
    for name in names:
        assert "int %s(" % name in header, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert len(_lib.SIGNATURES["objgan_convlstm_cell_forward"]) == 13
    assert len(_lib.SIGNATURES["objgan_convlstm_cell_backward"]) == 14

"""The shape generator's perceptual term on the MI355X: the stem pair, the per-tap L1 kernels, the whole `perceptual`
Function on a thin network against the fp64 oracle (tests/pcp_oracle.py), the trainer step against the reference golden
(tests/golden/pcp_ref.pt), the command line at the reference's default PCP_LAMBDA.

Bounds: stem and l1_tap_forward 1e-6 against fp64, l1_tap_backward bit-equal to the fp32 expression of its formula, all
of them bit-identical across two runs; the Function: fp32 arithmetic within 4 x e_cpu, the default arithmetic within
max(1.25 x the fp32 run's + 2e-8, 4 x e_cpu), where e_cpu is the error of an fp32 CPU evaluation of the oracle against
fp64 on the same inputs (asserted <= 1e-4 for the gradients first; the `wide` case, whose launches really run fp16x2,
has the flip floor of GRAD_FLOOR instead); trainer step vs golden: losses and per-tap means max(1e-5, 4 x floor), clipped
generator gradient and its norm max(4e-3, 4 x floor).

Observed on an MI355X: stem forward / backward vs fp64 <= 1.34e-7 / <= 9.4e-8 over the five shapes; l1_tap_forward
<= 2.7e-8 (n = 1 ... 2^20 + 3); l1_tap_backward bit-equal in all 48 cases.  Function, thin, taps / sum / gradient vs fp64:
B1 R1 fp32 1.7e-6 / 1.1e-7 / 6.0e-7, fp16x2 2.9e-6 / 1.9e-7 / 7.5e-7 (e_cpu 6.0e-6 / 5.1e-7 / 3.4e-6); B2 R3 fp32 8.2e-7 /
1.1e-8 / 5.7e-7, fp16x2 = bf16x3 1.8e-6 / 2.3e-7 / 6.8e-7 (e_cpu 1.8e-6 / 1.3e-7 / 6.6e-6); bf16 2.0e-2 / 2.0e-3 / 0.44.
Function, wide B2 R2 (3 forward and 3 data-gradient launches on fp16x2, the maxima verified): fp32 7.4e-7 / 2.9e-7 /
3.4e-3, fp16x2 5.4e-7 / 7.8e-8 / 1.4e-3 (e_cpu 3.3e-6 / 9.3e-7 / 1.6e-3: decisions flip, see GRAD_FLOOR).  VGG.forward
thin, worst tap 4.0e-6.  Trainer step vs the reference golden thin512: losses 2.3e-7, per-tap means 7.0e-7, clipped
generator gradient 5.6e-6, its norm 1.3e-6 (floors 1.3e-7 / 1.1e-6 / 6.5e-6)."""
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, PKG, rel_l2, note
import shapegen_oracle as so
import pcp_oracle as po

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden", "pcp_ref.pt")
TINY = os.path.join(ROOT, "tests", "golden", "shape_tiny")


def _ops():
    from objgan_hip import ops
    return ops


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, map_location="cpu", weights_only=False)


# ---------------------------------------------------------------------------------------------
# stem
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,OH", [(1, 64, 224), (3, 5, 7), (2, 1, 4), (2, 7, 1), (1, 64, 64)])
def test_stem_forward_backward_against_fp64(dev, N, S, OH):
    ops = _ops()
    g = torch.Generator().manual_seed(900 + 31 * N + 7 * S + OH)
    x = torch.rand(N, 1, S, S, generator=g)
    dy = torch.randn(N, 3, OH, OH, generator=g)
    xt = x.double().requires_grad_()
    yt = po.normalise(F.interpolate(xt, size=(OH, OH), mode="bilinear", align_corners=True))
    yt.backward(dy.double())
    xd, dyd = x.to(dev), dy.to(dev)
    y1, y2 = ops.pcp_stem_forward(xd, OH), ops.pcp_stem_forward(xd, OH)
    d1, d2 = ops.pcp_stem_backward(dyd, S), ops.pcp_stem_backward(dyd, S)
    torch.cuda.synchronize()
    e_f, e_b = rel_l2(y1, yt), rel_l2(d1, xt.grad)
    note("pcp stem (N, S, OH) = (%d, %d, %d) forward / backward vs fp64" % (N, S, OH), "%.3g %.3g" % (e_f, e_b))
    print((N, S, OH), "forward", e_f, "backward", e_b)
    assert tuple(y1.shape) == (N, 3, OH, OH) and tuple(d1.shape) == (N, 1, S, S)
    assert torch.equal(y1, y2) and torch.equal(d1, d2)
    assert e_f <= 1e-6 and e_b <= 1e-6
    if S == OH:                                               # identity geometry: the stem only normalises
        assert rel_l2(y1, po.normalise(x.double())) <= 1e-6


# ---------------------------------------------------------------------------------------------
# per-tap L1
# ---------------------------------------------------------------------------------------------
TAP_SIZES = [1, 3, 63, 257, 4099, (1 << 20) + 3]
_TAPS = {}


def tap_problem(n):
    """ReLU'd halves (a large share of exact zeros in both), some planted f == r != 0, a gradient from below"""
    if n not in _TAPS:
        g = torch.Generator().manual_seed(700 + n % 1000)
        f = torch.relu(torch.randn(n + 1, generator=g))
        r = torch.relu(torch.randn(n + 1, generator=g))
        k = torch.arange(0, n + 1, 5)
        r[k] = f[k]                                            # equal pairs: zeros and non-zeros alike
        if n >= 3:
            f[1] = r[1] = 0.75
        gd = torch.randn(n + 1, generator=g)
        _TAPS[n] = (f, r, gd)
    return _TAPS[n]


@pytest.mark.parametrize("n", TAP_SIZES)
def test_l1_tap_forward_against_fp64(dev, n):
    ops = _ops()
    f, r, _ = tap_problem(n)
    f, r = f[:n], r[:n]
    want = float((f.double() - r.double()).abs().mean())
    fd, rd = f.to(dev), r.to(dev)
    out1 = torch.full((19,), float("nan"), device=dev)
    out2 = torch.full((19,), float("nan"), device=dev)
    ops.l1_tap_forward(fd, rd, out1, 7)
    ops.l1_tap_forward(fd, rd, out2, 7)
    torch.cuda.synchronize()
    got = float(out1[7])
    err = abs(got - want) / max(abs(want), 1e-30)
    note("l1_tap_forward n = %d vs fp64" % n, "%.3g" % err)
    print(n, got, want, err)
    assert torch.equal(out1[7], out2[7])
    assert torch.isnan(out1[:7]).all() and torch.isnan(out1[8:]).all()      # one slot, nothing else
    assert err <= 1e-6


@pytest.mark.parametrize("n", TAP_SIZES)
@pytest.mark.parametrize("down", [False, True])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("offset", [0, 1])
def test_l1_tap_backward_is_the_fp32_expression(dev, n, down, relu, offset):
    ops = _ops()
    f, r, gd = (t.to(dev)[offset:offset + n] for t in tap_problem(n))
    assert (f.data_ptr() % 16 == 0) == (offset == 0)
    coef = torch.tensor([0.3 / n], device=dev)
    s = torch.sign(f - r)
    want = (gd + coef * s) if down else coef * s
    if relu:
        want = want * (f > 0).float()
    g, am = ops.l1_tap_backward(f, r, gd if down else None, coef, relu, want_amax=True)
    torch.cuda.synchronize()
    assert torch.equal(g, want)
    assert float(am.max()) == float(want.abs().max()) and am.numel() == 1024 and bool((am >= 0).all())
    if n >= 3 and offset == 0:
        assert float(s[1]) == 0.0 and float(g[1]) == (float(gd[1]) if down else 0.0)       # the planted f == r != 0


# ---------------------------------------------------------------------------------------------
# the whole Function on the thin network
# ---------------------------------------------------------------------------------------------
_FN_REF = {}


# What the fp32 CPU evaluation's gradient may differ from fp64 by before the test refuses its own inputs.  thin: 1e-4 (no
# decision flipped).  wide: at 64 channels and 224 x 224 some decision ALWAYS flips -- 56 consecutive mask seeds gave
# 1.0e-4 ... 1.1e-2, median 2e-3, for fp32 against fp64 on the CPU -- so the precondition is the 1e-2 that the golden maker
# allows the full-width network, and the same 1e-2 is the least a gradient bound of this case can be: WHICH decisions flip
# differs between any two fp32 evaluations (summation order), so one CPU sample of that spread cannot bound another.
GRAD_FLOOR = {"thin": 1e-4, "wide": 1e-2}


def fn_problem(widths, B, R):
    """seeded masks and the oracle's results: fp64, and fp32 on the CPU (e_cpu, the floor of the bounds)"""
    key = (widths, B, R)
    if key not in _FN_REF:
        sd = po.seeded_vgg(widths)
        # One ReLU / sign / pool-argmax decision of the network within fp32 rounding of its threshold moves the gradient by
        # 1e-3 between an fp32 and an fp64 evaluation, and WHICH masks have such a decision depends on the host's fp32
        # summation order (seed 814, thin, B = R = 1: 1.0e-5 on one machine, 2.8e-3 on another).  So the masks are the
        # first of a short fixed list of seeds whose fp32 CPU evaluation is within 1e-4 of fp64 on the machine that runs
        # the test: chosen by the reference arithmetic's own error, never by what the kernels give.  The seed is noted.
        for seed in range(814, 822):
            g = torch.Generator().manual_seed(seed)
            fake = torch.rand(B, R, 1, 64, 64, generator=g)
            real = torch.rand(B, 1, 64, 64, generator=g)
            res = {}
            for dt in (torch.float64, torch.float32):
                fh = fake.to(dt).clone().requires_grad_()
                fp = so.first_max(fh)
                fp.retain_grad()
                taps = po.perceptual({k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}, fp, real.to(dt))
                (taps.sum() * po.LAMBDA).backward()
                res[dt] = (taps.detach(), fp.grad.detach(), fh.grad.detach())
            if rel_l2(res[torch.float32][2], res[torch.float64][2]) <= GRAD_FLOOR[widths]:
                break
        note("pcp Function %s B%d R%d: seed of the masks" % key, "%d" % seed)
        print("masks of seed", seed)
        _FN_REF[key] = (fake, real, sd, res)
    return _FN_REF[key]


def fn_errors(got, want):
    taps, dfp, dfh = got
    return (float(((taps.double().cpu() - want[0].double()).abs() / want[0].double().abs()).max()),
            abs(float(taps.double().sum()) - float(want[0].double().sum())) / float(want[0].double().sum()),
            rel_l2(dfp, want[1]), rel_l2(dfh, want[2]))


def run_fn(dev, net, fake, real):
    ops = _ops()
    fh = fake.detach().to(dev).requires_grad_()
    rp = real.detach().to(dev).requires_grad_()
    fp = ops.box_max(fh)
    fp.retain_grad()
    taps = net.perceptual(fp, rp)
    (taps.sum() * po.LAMBDA).backward()
    torch.cuda.synchronize()
    assert rp.grad is None
    return taps.detach(), fp.grad.detach(), fh.grad.detach()


class igemm_census(object):
    """counts the objgan_conv_igemm launches of a block by (direction, arithmetic the kernel ran): argument 14 of the
    entry point is `transpose` (1: data gradient), argument 31 the arithmetic (4 / 5: fp16x2, gathered / on records)"""

    def __enter__(self):
        from objgan_hip import _lib
        self.lib, self.orig, self.seen = _lib, _lib.call, {}

        def counting(name, *args):
            if name == "objgan_conv_igemm":
                k = (int(args[14]), int(args[31]))
                self.seen[k] = self.seen.get(k, 0) + 1
            return self.orig(name, *args)
        _lib.call = counting
        return self

    def __exit__(self, *exc):
        self.lib.call = self.orig

    def h2(self, transpose):
        return sum(n for (t, m), n in self.seen.items() if t == transpose and m in (4, 5))


# ("wide", 2, 2): four images forward, two backward, of 64 channels at 224 x 224 -- the 64 -> 64 convolutions (14.8 GFLOP forward, 7.4 GFLOP data
# gradient) and those at 112 x 112 are above the 1e9 FLOP below which fp16x2 hands a launch to bf16x3
@pytest.mark.parametrize("widths,B,R", [("thin", 1, 1), ("thin", 2, 3), ("wide", 2, 2)])
def test_perceptual_function_against_fp64_oracle(dev, widths, B, R):
    import model
    ops = _ops()
    fake, real, sd, res = fn_problem(widths, B, R)
    e_cpu = fn_errors(res[torch.float32], res[torch.float64])
    print("e_cpu (taps, sum, d fake_pooled, d fake_hmaps)", e_cpu)
    assert e_cpu[2] <= GRAD_FLOOR[widths] and e_cpu[3] <= GRAD_FLOOR[widths]       # a loose floor must not hide a failure
    net = model.VGG(sd).to(dev)
    saved = ops.get_conv_math()
    errs = {}
    try:
        for math in ("fp32", "fp16x2"):
            ops.set_conv_math(math)
            with igemm_census() as census:
                a = run_fn(dev, net, fake, real)
            b = run_fn(dev, net, fake, real)
            assert all(torch.equal(p, q) for p, q in zip(a, b)), math
            assert tuple(a[0].shape) == (19,) and tuple(a[1].shape) == (B, 1, 64, 64) and tuple(a[2].shape) == (B, R, 1, 64, 64)
            errs[math] = fn_errors(a, res[torch.float64])
            note("pcp Function %s B%d R%d %s: taps / sum / d fake_pooled / d fake_hmaps vs fp64 (e_cpu %s)"
                 % (widths, B, R, math, " ".join("%.3g" % e for e in e_cpu)), " ".join("%.3g" % e for e in errs[math]))
            print(math, errs[math], census.seen)
            if math == "fp32":
                assert census.h2(0) == census.h2(1) == 0
            elif widths == "wide":
                # the default arithmetic really ran: forward launches on fused-ReLU maxima, data gradients on the maxima
                # the tap-backward kernel left
                assert census.h2(0) >= 3 and census.h2(1) >= 3, census.seen
                ops._H2_VERIFY["on"], before = True, ops._H2_VERIFY["checked"]
                try:
                    c = run_fn(dev, net, fake, real)          # every maximum handed to a kernel is re-derived and compared
                finally:
                    ops._H2_VERIFY["on"] = False
                # (the three data gradients read the tap-backward kernel's maxima, the forward launches a fused-ReLU epilogue's)
                assert ops._H2_VERIFY["checked"] - before >= 4 and all(torch.equal(p, q) for p, q in zip(a, c))
    finally:
        ops.set_conv_math(saved)
    for i, (e32, edef, ec) in enumerate(zip(errs["fp32"], errs["fp16x2"], e_cpu)):
        flips = GRAD_FLOOR[widths] if (widths == "wide" and i >= 2) else 0.0      # gradients of the wide case, see GRAD_FLOOR
        assert e32 <= max(4 * ec, flips)
        assert edef <= max(1.25 * e32 + 2e-8, 4 * ec, flips)


@pytest.mark.parametrize("math,bound", [("bf16x3", None), ("bf16", 5e-2)])
def test_perceptual_function_under_the_other_arithmetics(dev, math, bound):
    """bf16x3 (exact three-way split: fp32 results, the default row's bound) and bf16 (operands rounded to 8 bits: 2^-8
    per operand over 19 layers, 5e-2 on the taps; its ReLU / sign decisions differ, so the gradient is only finite)"""
    import model
    ops = _ops()
    fake, real, sd, res = fn_problem("thin", 2, 3)
    e_cpu = fn_errors(res[torch.float32], res[torch.float64])
    net = model.VGG(sd).to(dev)
    saved = ops.get_conv_math()
    try:
        ops.set_conv_math(math)
        a = run_fn(dev, net, fake, real)
        b = run_fn(dev, net, fake, real)
    finally:
        ops.set_conv_math(saved)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert all(bool(torch.isfinite(t).all()) for t in a)
    e = fn_errors(a, res[torch.float64])
    note("pcp Function thin B2 R3 %s: taps / sum / d fake_pooled / d fake_hmaps vs fp64" % math, " ".join("%.3g" % v for v in e))
    print(math, e)
    if bound is None:
        assert all(v <= 4 * ec + 2e-8 for v, ec in zip(e, e_cpu))
    else:
        assert e[0] <= bound and e[1] <= bound and float(a[2].abs().sum()) > 0


def test_forward_returns_the_19_features(dev):
    """`forward(x)`, the reference's signature: the taps of a normalised 3-channel input"""
    import model
    g = torch.Generator().manual_seed(77)
    x = po.normalise(torch.rand(2, 1, 64, 64, generator=g))
    sd = po.seeded_vgg("thin")
    want = po.vgg_features(sd, x.double())
    got = model.VGG(sd).to(dev)(x.to(dev))
    torch.cuda.synchronize()
    assert len(got) == 19 and all(tuple(a.shape) == tuple(b.shape) for a, b in zip(got, want))
    worst = max(rel_l2(a, b) for a, b in zip(got, want))
    note("pcp VGG.forward thin, worst tap vs fp64", "%.3g" % worst)
    assert worst <= 1e-4


# ---------------------------------------------------------------------------------------------
# the trainer step against the reference golden
# ---------------------------------------------------------------------------------------------
def make_trainer(dev, tmp_path, nbf, B, vgg_sd):
    import model
    import shape_trainer
    from miscc.config import cfg
    cfg.GAN.R_NUM = 1
    cfg.TRAIN.BATCH_SIZE = B
    cfg.TRAIN.FLAG = True
    cfg.TRAIN.SMOOTH.PCP_LAMBDA = po.LAMBDA
    cfg.TRAIN.SMOOTH.INS_LAMBDA = 1.0
    cfg.TRAIN.SMOOTH.GLB_LAMBDA = 1.0
    ds = type("DS", (), {"cats_dict": {}, "cats_index_dict": {i: i for i in range(nbf)}})()
    t = shape_trainer.condGANTrainer(str(tmp_path), None, ds, device=dev)
    t.attach(so.seeded_state_(model.SHP_G_NET(nbf), so.SEEDS["G"]), so.seeded_state_(model.INS_D_NET(nbf), so.SEEDS["INSD"]),
             so.seeded_state_(model.GLB_D_NET(nbf), so.SEEDS["GLBD"]), vgg=model.VGG(vgg_sd))
    return t


# (`full` is in the golden only when the build machine could run it: make_golden_pcp.py --full)
@pytest.mark.parametrize("case", sorted(torch.load(GOLD, map_location="cpu", weights_only=False)["cases"], reverse=True))
def test_trainer_step_against_reference_golden(dev, gold, tmp_path, case):
    from miscc.config import cfg
    ops = _ops()
    c = gold["cases"][case]
    nbf, B, R = c["nbf"], c["B"], c["R"]
    x = so.make_inputs(c["shapegen_case"])
    try:
        t = make_trainer(dev, tmp_path, nbf, B, po.seeded_vgg(c["widths"]))
        t.define_optimizers(1.0)
        batch = {"max_num_roi": R, "bbox_maps_fwd": x["fwd"].to(dev), "bbox_maps_bwd": x["bwd"].to(dev),
                 "bbox_fmaps": x["fmaps"].to(dev), "hmaps": x["real"].to(dev), "pooled_hmaps": x["real_pooled"].to(dev)}
        out = t.train_step(batch, noise=x["z"].to(dev))
        with torch.no_grad():
            taps = t.vgg.perceptual(ops.box_max(out["fake_hmaps"]), ops.box_max(batch["hmaps"]))
        torch.cuda.synchronize()
    finally:
        cfg.TRAIN.SMOOTH.PCP_LAMBDA = 0.0
    fl = c["floor"]
    e_loss = max(abs(float(out["errG"]) - c["errG"]) / abs(c["errG"]),
                 abs(float(out["gpcp_loss"]) - c["gpcp_loss"]) / abs(c["gpcp_loss"]),
                 abs(float(out["pcp_score"]) - c["item_pcp_score"]) / abs(c["item_pcp_score"]))
    e_taps = float(((taps.double().cpu() - c["taps"].double()).abs() / c["taps"].double().abs()).max())
    div, norm = float(out["clip"][0]), float(out["clip"][1])
    got, ref = [], []
    for k, p in t.netG.named_parameters():
        got.append(so.sample(p.grad.detach().cpu() / div))
        ref.append(c["gradG_clipped"][k]["sample"])
    e_g = rel_l2(torch.cat(got), torch.cat(ref))
    e_n = abs(norm - c["normG"]) / c["normG"]
    note("pcp trainer step vs reference %s losses / taps / G grads / G norm (floors %.3g %.3g %.3g)"
         % (case, fl["loss"], fl["taps"], fl["gradG_samples"]), "%.3g %.3g %.3g %.3g" % (e_loss, e_taps, e_g, e_n))
    print(case, "losses", e_loss, "taps", e_taps, "G", e_g, "norm", e_n, "floor", fl)
    assert float(t.pcp_score) == float(out["pcp_score"])
    assert e_loss <= max(1e-5, 4 * fl["loss"]) and e_taps <= max(1e-5, 4 * fl["taps"])
    g_floor = max(fl["gradG"], fl["gradG_samples"], fl["dfake"])
    assert e_g <= max(4e-3, 4 * g_floor) and e_n <= max(4e-3, 4 * g_floor)


# ---------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------
def test_shape_main_trains_with_the_default_lambda(dev, tmp_path):
    data = str(tmp_path / "data")
    shutil.copytree(TINY, data)
    os.makedirs(os.path.join(data, "pretrained"))
    torch.save(po.seeded_vgg("thin"), os.path.join(data, "pretrained", "vgg19_bn-c79401a0.pth"))
    cmd = [sys.executable, os.path.join(PKG, "shape_main.py"), "--FLAG", "--BATCH_SIZE", "2", "--MAX_EPOCH", "2",
           "--data_dir", data, "--output_dir", str(tmp_path), "--manualSeed", "7"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    r = subprocess.run(cmd, cwd=PKG, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-3000:]
    vals = [float(m) for m in re.findall(r"gpcp_loss: (\S+)", text)]
    assert vals and all(v == v and abs(v) != float("inf") for v in vals), text[-2000:]
    model_dir = [line.split(":", 1)[1].strip() for line in text.splitlines() if line.startswith("Model directory:")][0]
    score_dir = os.path.join(os.path.dirname(model_dir), "Score")
    scores = []
    for epoch in range(2):
        m = re.fullmatch(r"pcp_score (-?\d+\.\d+)", open(os.path.join(score_dir, "scores_%d.txt" % epoch)).read())
        assert m, epoch
        scores.append(float(m.group(1)))
    assert 0 < scores[0] < scores[1]
    assert {"netG_epoch_0.pth", "netG_epoch_1.pth", "netG_epoch_2.pth", "netINSD.pth", "netGLBD.pth"} <= set(os.listdir(model_dir))

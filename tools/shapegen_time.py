#!/usr/bin/env python
"""Time of the shape generator's training at the reference's shape (B = 40, R = 10, nbf = 80; one MI355X):

  * generator forward + backward with the split ConvLSTM recurrence (ops.convlstm_sequence) against the per-step
    cat + conv cell loop of CLSTMCell.forward under autograd, alternating, in the same process on the same inputs,
    with the relative difference of their masks and of one gradient;
  * the whole training step (G, both Ds, clip, Adam, EMA);
  * library entry-point calls per pass (host-side count of objgan_* launches; torch's own kernels are not in it).
Device events around `--steps` passes after `--warmup` passes.  Prints one JSON line; `--out` also writes it to a file.
`--step-only`: just the step loop (the run to put under a kernel trace).  Not a test: asserts nothing about time.

`--pcp`: the cost of the perceptual term instead, at the reference batch of 40 and at 16 in ONE call.  The frozen
VGG-19-bn comes from `--vgg-weights FILE` (torchvision's vgg19_bn-c79401a0.pth) or, without a file, from seeded
full-width weights.  Per batch size, alternating runs on the same seeded batch:
  * the whole training step with PCP_LAMBDA = 10 against the same tree with PCP_LAMBDA = 0.  The difference is the COST
    OF THE TERM (about 3 B VGG-19 passes: 2 B forward, B data gradient), not a regression of anything;
  * the term alone (`VGG.perceptual` forward + backward);
  * the new memory-bound kernels (stem pair, l1_tap_forward, l1_tap_backward) replayed at every tap's shape: their
    time over the bytes they must move, as a share of the HBM peak (8 TB/s);
  * the convolutions inside the term: algorithmic FLOP (forward on 2 B images, data gradient on B, Linears included)
    over the term's time minus the replayed kernels' time (the five pool passes stay in that remainder).

`--display`: the cost of the pictures at the reference batch of 40.  One `save_img_results` call (wall clock around
the call with a device synchronisation on both sides, the four PNG files written to a temporary directory) per PNG
compression level; five training steps with and without one display call behind them, as `train` issues it (the files
left to the worker threads); the call split into its parts -- the generator forward with the EMA swap, the caption strip, the four grid
compositions with their device-to-host copies, the four PNG encodings -- beside the training step with PCP_LAMBDA 0 and
10 (seeded full-width VGG unless `--vgg-weights`), decoding eight 640 x 480 JPEGs the way `images_for` does, and the
rate of `sampling` over `--sample-batches` synthetic batches, files included.

    python tools/shapegen_time.py [--B 40] [--R 10] [--nbf 80] [--steps 10] [--warmup 3] [--out FILE] [--step-only]
    python tools/shapegen_time.py --display [--steps 5] [--warmup 2] [--sample-batches 10] [--out FILE]
    python tools/shapegen_time.py --pcp [--vgg-weights FILE] [--pcp-batches 40,16] [--steps 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "obj-gan_amd"))


def inputs(B, R, nbf, dev, seed=0):
    from objgan_hip import ops
    g = torch.Generator().manual_seed(seed)
    xy = torch.randint(0, 36, (B, 10, 2), generator=g)
    wh = torch.randint(8, 26, (B, 10, 2), generator=g)
    ar = torch.arange(64)
    inx = (ar.view(1, 1, 64) >= xy[..., 0:1]) & (ar.view(1, 1, 64) < (xy + wh)[..., 0:1])
    iny = (ar.view(1, 1, 64) >= xy[..., 1:2]) & (ar.view(1, 1, 64) < (xy + wh)[..., 1:2])
    raw = (iny.unsqueeze(3) & inx.unsqueeze(2)).float()
    num = torch.randint(1, R + 1, (B,), generator=g)
    num[0] = R
    raw = raw * (torch.arange(10).view(1, 10, 1, 1) < num.view(B, 1, 1, 1)).float()
    cats = torch.randint(0, nbf, (B, 10), generator=g).to(torch.int32)
    fwd, bwd = ops.boxmaps_onehot(raw.to(dev), cats.to(dev), num.to(torch.int32).to(dev), R, nbf)
    fmaps = torch.nn.functional.max_pool2d(raw[:, :R], 4).to(dev)
    real = (torch.rand(B, R, 1, 64, 64, generator=g) * raw[:, :R].unsqueeze(2)).to(dev)
    rois = torch.cat([xy, wh, cats.view(B, 10, 1).long(), torch.zeros(B, 10, 1, dtype=torch.long)], 2).double()
    return {"max_num_roi": R, "bbox_maps_fwd": fwd, "bbox_maps_bwd": bwd, "bbox_fmaps": fmaps.contiguous(),
            "hmaps": real, "pooled_hmaps": real.max(1)[0], "rois": rois.numpy(), "num_rois": num,
            "keys": ["img_%05d" % i for i in range(B)],
            # the collated item tuple of shapeDataset (what `sampling` takes from its loader)
            "item": (real.max(1)[0][:, 0].cpu(), torch.zeros(B, 10, 64, 64), raw, cats, torch.nn.functional.max_pool2d(raw, 4),
                     rois, rois / 4.0, num, torch.arange(B), ["img_%05d" % i for i in range(B)])}


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


HBM_PEAK = 8.0e12          # bytes / s, MI355X


def seeded_vgg_state(seed=331):
    """full-width weights in torchvision's layout: N(0, 2 / fan_in) banks, running variances 0.5 + U(0, 1)"""
    import model
    g = torch.Generator().manual_seed(seed)
    sd = model.vgg_init_state()
    for k in sorted(sd):
        t = sd[k]
        if t.dim() > 1:
            t.copy_(torch.randn(t.shape, generator=g) * (2.0 / t[0].numel()) ** 0.5)
        elif k.endswith("running_var"):
            t.copy_(0.5 + torch.rand(t.shape, generator=g))
        elif k.endswith("running_mean"):
            t.copy_(0.1 * torch.randn(t.shape, generator=g))
    return sd


def pcp_glue(vgg, B, dev, steps, warmup):
    """replay of the new kernels at the term's shapes -> (ms, bytes) per kernel family for ONE training step"""
    from objgan_hip import ops
    shapes, x = [], (2 * B, 3, 224, 224)
    for layer in vgg.layers():
        if layer[0] == "pool":
            x = (x[0], x[1], x[2] // 2, x[3] // 2)
            continue
        x = (x[0], layer[1].shape[0], x[2], x[3]) if layer[0] == "conv" else (x[0], layer[1].shape[0], 1, 1)
        shapes.append((layer[0] == "conv" or layer[3], B * x[1] * x[2] * x[3]))
    out = {}
    xs = torch.rand(2 * B, 1, 64, 64, device=dev)
    dy = torch.randn(B, 3, 224, 224, device=dev)
    out["stem_forward"] = (timed(lambda: ops.pcp_stem_forward(xs), steps, warmup), 4.0 * (xs.numel() + 2 * B * 3 * 224 * 224))
    out["stem_backward"] = (timed(lambda: ops.pcp_stem_backward(dy, 64), steps, warmup), 4.0 * (dy.numel() + B * 64 * 64))
    means = torch.empty(len(shapes), device=dev)
    coef = torch.full((1,), 1e-6, device=dev)
    fwd_ms = bwd_ms = fwd_b = bwd_b = 0.0
    for slot, (relu, n) in enumerate(shapes):
        f, r, gd = (torch.relu(torch.randn(n, device=dev)) for _ in range(3))
        last = slot == len(shapes) - 1
        fwd_ms += timed(lambda: ops.l1_tap_forward(f, r, means, slot), steps, warmup)
        bwd_ms += timed(lambda: ops.l1_tap_backward(f, r, None if last else gd, coef, relu), steps, warmup)
        fwd_b += 8.0 * n
        bwd_b += (12.0 if last else 16.0) * n
        del f, r, gd
    out["l1_tap_forward"] = (fwd_ms, fwd_b)
    out["l1_tap_backward"] = (bwd_ms, bwd_b)
    return out


def pcp_conv_flop(vgg, B):
    flop, x = 0.0, (3, 224, 224)
    for layer in vgg.layers():
        if layer[0] == "pool":
            x = (x[0], x[1] // 2, x[2] // 2)
            continue
        w = layer[1]
        px = x[1] * x[2] if layer[0] == "conv" else 1
        flop += 2.0 * w.numel() * px * 3 * B           # forward on 2 B images + data gradient on B
        x = (w.shape[0], x[1], x[2]) if layer[0] == "conv" else (w.shape[0], 1, 1)
    return flop


def pcp_main(a, dev):
    """--pcp: see the module docstring"""
    import tempfile
    import model
    import shape_trainer
    from miscc.config import cfg
    from objgan_hip import ops
    sd = torch.load(a.vgg_weights, map_location="cpu") if a.vgg_weights else seeded_vgg_state()
    res = {"mode": "pcp", "R": a.R, "nbf": a.nbf, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "conv_math": ops.get_conv_math(), "weights": a.vgg_weights or "seeded full-width", "hbm_peak_bytes_per_s": HBM_PEAK,
           "note": "term_cost_ms is the cost of the perceptual term (about 3 B VGG-19 passes), not a regression", "batches": {}}
    ds = type("DS", (), {"cats_dict": {}, "cats_index_dict": {i: i for i in range(a.nbf)}})()
    vgg = model.VGG(sd).to(dev)
    del sd
    for B in [int(v) for v in a.pcp_batches.split(",")]:
        cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.FLAG, cfg.GAN.R_NUM = B, True, 1
        cfg.TRAIN.SMOOTH.INS_LAMBDA, cfg.TRAIN.SMOOTH.GLB_LAMBDA = 1.0, 1.0
        batch = inputs(B, a.R, a.nbf, dev)
        trainers = {}
        for lam in (0.0, 10.0):
            torch.manual_seed(0)
            cfg.TRAIN.SMOOTH.PCP_LAMBDA = 0.0               # (build_models would look for the weights file)
            t = shape_trainer.condGANTrainer(tempfile.mkdtemp(prefix="shapegen_time_"), None, ds, device=dev)
            t.build_models()
            if lam:
                t.vgg = vgg
            t.define_optimizers(1.0)
            trainers[lam] = t

        def step(lam):
            cfg.TRAIN.SMOOTH.PCP_LAMBDA = lam
            return trainers[lam].train_step(batch)

        fp = batch["pooled_hmaps"].clone().requires_grad_()
        rp = torch.rand_like(fp)

        def term():
            fp.grad = None
            (vgg.perceptual(fp, rp).sum() * 10.0).backward()

        ms = {"lambda_0": [], "lambda_10": [], "term_alone": []}
        for _ in range(a.rounds):                            # alternate
            ms["lambda_0"].append(timed(lambda: step(0.0), a.steps, a.warmup))
            ms["lambda_10"].append(timed(lambda: step(10.0), a.steps, a.warmup))
            ms["term_alone"].append(timed(term, a.steps, a.warmup))
        glue = pcp_glue(vgg, B, dev, a.steps, a.warmup)
        glue_ms = sum(v[0] for v in glue.values())
        term_ms = min(ms["term_alone"])
        flop = pcp_conv_flop(vgg, B)
        res["batches"][str(B)] = {
            "step_ms": ms, "term_cost_ms": min(ms["lambda_10"]) - min(ms["lambda_0"]),
            "new_kernels": {k: {"ms": v[0], "bytes": v[1], "share_of_hbm_peak": v[1] / (v[0] * 1e-3) / HBM_PEAK}
                            for k, v in glue.items()},
            "new_kernels_total": {"ms": glue_ms, "bytes": sum(v[1] for v in glue.values()),
                                  "share_of_hbm_peak": sum(v[1] for v in glue.values()) / (glue_ms * 1e-3) / HBM_PEAK},
            "convolutions": {"algorithmic_tflop": flop / 1e12, "ms": term_ms - glue_ms,
                             "tflops": flop / ((term_ms - glue_ms) * 1e-3) / 1e12,
                             "what": "term alone minus the replayed new kernels; the five pool passes stay in the remainder"}}
        cfg.TRAIN.SMOOTH.PCP_LAMBDA = 0.0
        del trainers, batch
        torch.cuda.empty_cache()
    return res


def wall(fn, steps, warmup):
    """host wall clock per call in ms, the device drained on both sides"""
    import time
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def display_main(a, dev):
    """--display: see the module docstring"""
    import io
    import tempfile
    import numpy as np
    from PIL import Image
    import model
    import shape_trainer
    from miscc import load, shape_utils
    from miscc.config import cfg
    from objgan_hip import ops
    B, R, nbf = a.B, a.R, a.nbf
    cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.FLAG, cfg.GAN.R_NUM = B, True, 1
    cfg.TRAIN.SMOOTH.INS_LAMBDA, cfg.TRAIN.SMOOTH.GLB_LAMBDA, cfg.TRAIN.SMOOTH.PCP_LAMBDA = 1.0, 1.0, 0.0
    ds = type("DS", (), {"cats_dict": {i: [1 + i % 7] for i in range(nbf)}, "cats_index_dict": {i: i for i in range(nbf)},
                         "ixtoword": {i: "word%d" % i for i in range(8)}})()
    torch.manual_seed(0)
    out_dir = tempfile.mkdtemp(prefix="shapegen_time_")
    t = shape_trainer.condGANTrainer(out_dir, None, ds, device=dev)
    t.build_models()
    t.define_optimizers(1.0)
    batch = inputs(B, R, nbf, dev)
    imgs = torch.tanh(torch.randn(B, 3, 64, 64, device=dev))
    z = torch.randn(B, R, 4 * nbf, device=dev)
    res = {"mode": "display", "B": B, "R": R, "nbf": nbf, "steps": a.steps, "warmup": a.warmup, "conv_math": ops.get_conv_math()}
    res["step_ms_lambda_0"] = [timed(lambda: t.train_step(batch), a.steps, a.warmup) for _ in range(a.rounds)]
    sd = torch.load(a.vgg_weights, map_location="cpu") if a.vgg_weights else seeded_vgg_state()
    t.vgg = model.VGG(sd).to(dev)
    del sd
    cfg.TRAIN.SMOOTH.PCP_LAMBDA = 10.0
    res["step_ms_lambda_10"] = [timed(lambda: t.train_step(batch), a.steps, a.warmup) for _ in range(a.rounds)]
    cfg.TRAIN.SMOOTH.PCP_LAMBDA = 0.0
    t.vgg = None
    torch.cuda.empty_cache()
    res["save_img_results_ms"] = {}
    for level in (6, 1):
        shape_trainer.PNG_COMPRESS_LEVEL = level
        res["save_img_results_ms"]["png_level_%d" % level] = [
            wall(lambda: t.save_img_results(batch, z, 5, name="average", imgs=imgs), a.steps, a.warmup) for _ in range(a.rounds)]
        res.setdefault("png_bytes", {})["level_%d" % level] = {f: os.path.getsize(os.path.join(t.image_dir, f))
                                                               for f in sorted(os.listdir(t.image_dir))}
    # what the grids add to training at the reference's interval: 5 steps with and without one display call behind them
    # (wait=False, as train() calls it: the files of a call are awaited by the next one)
    shape_trainer.PNG_COMPRESS_LEVEL = 1

    def interval(display):
        for _ in range(5):
            t.train_step(batch)
        if display:
            t.save_img_results(batch, z, 5, name="average", imgs=imgs, wait=False)
    res["five_steps_ms"] = {"without_display": [], "with_display": []}
    for _ in range(a.rounds):                                # alternate
        res["five_steps_ms"]["without_display"].append(wall(lambda: interval(False), a.steps, a.warmup))
        res["five_steps_ms"]["with_display"].append(wall(lambda: interval(True), a.steps, a.warmup))
    t.finish_images()
    # the parts
    nvis = 8
    parts = {}
    with torch.no_grad():
        parts["generator_forward_nvis"] = wall(lambda: t.netG(z[:nvis], batch["bbox_maps_fwd"][:nvis], batch["bbox_maps_bwd"][:nvis],
                                                              batch["bbox_fmaps"][:nvis]), a.steps, a.warmup)
        parts["generator_forward_batch"] = wall(lambda: t.netG(z, batch["bbox_maps_fwd"], batch["bbox_maps_bwd"],
                                                               batch["bbox_fmaps"]), a.steps, a.warmup)
        fake = t.netG(z[:nvis], batch["bbox_maps_fwd"][:nvis], batch["bbox_maps_bwd"][:nvis], batch["bbox_fmaps"][:nvis])
    caps = np.ones((nvis, 10), np.int64)
    parts["caption_strip"] = wall(lambda: shape_utils.caption_strip(caps, ds.ixtoword, nvis, 64, 20, 12, 10, dev), a.steps, a.warmup)
    strip = shape_utils.caption_strip(caps, ds.ixtoword, nvis, 64, 20, 12, 10, dev)
    parts["one_grid_compose_and_copy"] = wall(lambda: shape_utils.build_super_images(
        imgs[:nvis], caps, ds.ixtoword, fake, 64, font_max=20, font_size=12, max_word_num=10, strip=strip), a.steps, a.warmup)
    grid = shape_utils.build_super_images(imgs[:nvis], caps, ds.ixtoword, fake, 64, font_max=20, font_size=12, max_word_num=10,
                                          strip=strip)[0]
    res["grid_shape"] = list(grid.shape)
    for level in (6, 1, 0):
        parts["one_png_encode_level_%d" % level] = wall(
            lambda: Image.fromarray(grid).save(io.BytesIO(), format="PNG", compress_level=level), a.steps, a.warmup)
    g = np.random.RandomState(0)
    buf = io.BytesIO()
    Image.fromarray(np.clip(np.cumsum(g.randn(480, 640, 3), 1) * 4 + 128, 0, 255).astype(np.uint8)).save(buf, format="JPEG", quality=90)
    parts["decode_8_jpegs_640x480"] = wall(lambda: [load.get_imgs(buf.getvalue(), [64], branch_num=1) for _ in range(8)],
                                           a.steps, a.warmup)
    res["parts_ms"] = parts
    # sampling: a synthetic split of whole batches, the trainer's own generator as the checkpoint
    import time
    ckpt = os.path.join(out_dir, "netG_epoch_0.pth")
    torch.save({k: v.detach().cpu() for k, v in t.netG.state_dict().items()}, ckpt)
    cfg.TRAIN.NET_G = ckpt
    items = []
    for k in range(a.sample_batches):
        item = list(inputs(B, R, nbf, dev, seed=k)["item"])
        item[9] = ["b%03d_%s" % (k, key) for key in item[9]]
        items.append(tuple(item))
    t.data_loader = items
    t.sampling("test")                                       # warm-up pass (filter banks, allocator, directory)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    written, skipped = t.sampling("test")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res["sampling"] = {"images": written, "skipped": skipped, "seconds": dt, "images_per_s": written / dt}
    cfg.TRAIN.NET_G = ""
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=40)
    ap.add_argument("--R", type=int, default=10)
    ap.add_argument("--nbf", type=int, default=80)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--pcp", action="store_true")
    ap.add_argument("--vgg-weights", type=str, default="")
    ap.add_argument("--pcp-batches", type=str, default="40,16")
    ap.add_argument("--display", action="store_true")
    ap.add_argument("--sample-batches", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    if a.pcp or a.display:
        line = json.dumps(display_main(a, dev) if a.display else pcp_main(a, dev))
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    from miscc.config import cfg
    from objgan_hip import ops, _lib
    import shape_trainer
    cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.FLAG, cfg.GAN.R_NUM = a.B, True, 1
    cfg.TRAIN.SMOOTH.PCP_LAMBDA, cfg.TRAIN.SMOOTH.INS_LAMBDA, cfg.TRAIN.SMOOTH.GLB_LAMBDA = 0.0, 1.0, 1.0
    torch.manual_seed(0)
    ds = type("DS", (), {"cats_dict": {}, "cats_index_dict": {i: i for i in range(a.nbf)}})()
    import tempfile
    t = shape_trainer.condGANTrainer(tempfile.mkdtemp(prefix="shapegen_time_"), None, ds, device=dev)
    t.build_models()
    t.define_optimizers(1.0)
    batch = inputs(a.B, a.R, a.nbf, dev)
    calls = [0]
    orig_call = _lib.call

    def counting(name, *args):
        calls[0] += 1
        return orig_call(name, *args)
    _lib.call = counting

    def count(fn):
        torch.cuda.synchronize()
        calls[0] = 0
        fn()
        return calls[0]

    res = {"B": a.B, "R": a.R, "nbf": a.nbf, "steps": a.steps, "warmup": a.warmup, "conv_math": ops.get_conv_math()}
    step = lambda: t.train_step(batch)                  # noqa: E731
    if not a.step_only:
        z = torch.randn(a.B, a.R, 4 * a.nbf, device=dev)
        gy = torch.randn(a.B, a.R, 1, 64, 64, device=dev)
        net = t.netG

        def g_pass(split):
            net.split_recurrence = split
            t.arenaG.zero_grad()
            with ops.direct_wgrad_scope():
                y = net(z, batch["bbox_maps_fwd"], batch["bbox_maps_bwd"], batch["bbox_fmaps"])
                y.backward(gy)
            return y
        ys = g_pass(True).detach().clone()
        gs = t.arenaG.grad.clone()
        yl = g_pass(False).detach().clone()
        gl = t.arenaG.grad.clone()
        rel = lambda p, q: float((p.double() - q.double()).norm() / q.double().norm())      # noqa: E731
        res["split_vs_loop_rel_l2"] = {"masks": rel(ys, yl), "gradient_arena": rel(gs, gl)}
        res["g_fwd_bwd_calls"] = {"split": count(lambda: g_pass(True)), "loop": count(lambda: g_pass(False))}
        ms = {"split": [], "loop": []}
        for _ in range(a.rounds):                            # alternate the two versions
            for name, split in (("split", True), ("loop", False)):
                ms[name].append(timed(lambda: g_pass(split), a.steps, a.warmup))
        res["g_fwd_bwd_ms"] = ms
        net.split_recurrence = True
    res["step_calls"] = count(step)
    res["step_ms"] = [timed(step, a.steps, a.warmup) for _ in range(1 if a.step_only else a.rounds)]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Time of the shape generator's training at the reference's shape (B = 40, R = 10, nbf = 80; one MI355X):

  * generator forward + backward with the split ConvLSTM recurrence (ops.convlstm_sequence) against the per-step
    cat + conv cell loop of CLSTMCell.forward under autograd, alternating, in the same process on the same inputs,
    with the relative difference of their masks and of one gradient;
  * the whole training step (G, both Ds, clip, Adam, EMA);
  * library entry-point calls per pass (host-side count of objgan_* launches; torch's own kernels are not in it).
Device events around `--steps` passes after `--warmup` passes.  Prints one JSON line; `--out` also writes it to a file.
`--step-only`: just the step loop (the run to put under a kernel trace).  Not a test: asserts nothing about time.

    python tools/shapegen_time.py [--B 40] [--R 10] [--nbf 80] [--steps 10] [--warmup 3] [--out FILE] [--step-only]
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
    return {"max_num_roi": R, "bbox_maps_fwd": fwd, "bbox_maps_bwd": bwd, "bbox_fmaps": fmaps.contiguous(),
            "hmaps": real, "pooled_hmaps": real.max(1)[0]}


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
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
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

#!/usr/bin/env python
"""Time the box decoder's launch (csrc/box_decode.hip) at the reference's shape: H = 256, 83 labels, K = 5, T = 10.

    python tools/box_decode_bench.py [--captions 1024] [--reps 20] [--out FILE]

hipEvents around one launch, warm, median of --reps, the tile sizes (captions per workgroup) alternating within every
repetition so that they see the same machine state.  The weights are uniform(-0.08, 0.08) as the reference initialises
them, with the <eos> logit pushed down: every caption runs all T steps, so the figure is the upper bound of a decode.
The outputs of all tile sizes are compared byte for byte before anything is timed.  Needs an MI355X (no fallback)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "obj-gan_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captions", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("box_decode_bench: no GPU")
    from objgan_hip import ops
    from seq2seq.models import DecoderRNN
    dev = torch.device("cuda:0")
    H, L, K, T, B = 256, 83, 5, 10, opt.captions
    words = ["<pad>", "<sos>", "<eos>", "<unk>"] + [str(i) for i in range(1, L - 3)]
    decoder = DecoderRNN({w: i for i, w in enumerate(words)}, 0.0, 0.0, 0.0, 0.0, 1, 150, H, K, bidirectional=True)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for p in decoder.parameters():
            p.copy_(torch.rand(p.shape, generator=g) * 0.16 - 0.08)
        decoder.l_out.bias[decoder.l_eos_id] -= 10.0
    decoder.to(dev)
    h0 = (torch.rand(B, H, generator=g) * 2 - 1).to(dev)
    c0 = (torch.rand(B, H, generator=g) * 2 - 1).to(dev)
    rs = np.random.RandomState(0)
    noise = torch.from_numpy(np.concatenate((rs.random_sample((B, T, 1)), rs.standard_normal((B, T, 2)),
                                             rs.random_sample((B, T, 1)), rs.standard_normal((B, T, 2))), 2)).to(dev)
    first = (decoder.x_mean, decoder.y_mean, decoder.w_mean, decoder.r_mean)
    weights = decoder._weights()

    def run(cpw):
        return ops.box_decode(h0, c0, noise, weights, first, decoder.l_sos_id, decoder.l_eos_id, cpw=cpw)

    tiles = [1, 2, 4]
    outs = {cpw: [t.cpu() for t in run(cpw)] for cpw in tiles}                 # warm-up of every variant
    torch.cuda.synchronize()
    for cpw in tiles[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[tiles[0]], outs[cpw])), "tile size changed the result"
    assert int(outs[1][1].min()) == T, "a caption ended early"
    times = {cpw: [] for cpw in tiles}
    for _ in range(opt.reps):
        for cpw in tiles:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            run(cpw)
            stop.record()
            stop.synchronize()
            times[cpw].append(start.elapsed_time(stop))
    res = {"captions": B, "steps": T, "reps": opt.reps, "default_cpw": ops.box_decode_cpw(),
           "ms": {str(c): {"median": statistics.median(v), "min": min(v), "max": max(v)} for c, v in times.items()},
           "us_per_caption": {str(c): 1e3 * statistics.median(v) / B for c, v in times.items()}}
    line = json.dumps(res)
    print(line)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Edge-shape cases of the box generator kernels (csrc/box_train.hip: forward, loss, BPTT, reduce, clip; and
csrc/box_decode.hip) with their fp64 references, shared by tests/test_boxgen_edges_cpu.py and
tests/test_boxgen_edges_gpu.py (no GPU import here).

One table per family; every entry carries an `id` that names the branch it is there for.  The references are the
restatements of tests/boxgen_train_oracle.py (`step_ref`, with its `dtrace` / `pad` extensions) and
tests/boxgen_oracle.py (`decode_ref`, with its `dtype` extension) in float64; the fp32 oracle is the same restatement in
float32.  The metric and the rule for M are those of tests/kernel_edge_cases.py: per compared block
e = max |a - ref64| / max |ref64| (denominator 1 for an all-zero reference), the kernel must satisfy
e_k <= M[family] * max(e_o, 2^-23) with e_o the same figure of the fp32 oracle, and rel_l2 <= TO.BOUND per tensor.

Blocks: the trace per caption; the two loss sums per caption; dtrace per (b, t) row and per segment of it (the L label
entries, the 6K of the xy mixture, the 6K of the wh mixture: their scales differ by orders of magnitude, one maximum
over the row would hide the smaller two); each of the 17 gradients.  dtrace and the sums are compared twice: those
of the chain with the restatement's (family box_loss), and those of the loss entry point alone, fed the restatement's
trace rounded to fp32, with the fp64 loss of that rounded trace (family box_loss_alone).  Counts (n, matches, N), zeros
past a length and bit-equalities are asserted as equalities.
"""
import functools
import math

import numpy as np
import torch

import boxgen_oracle as BO
import boxgen_train_oracle as TO

EPS32 = 2.0 ** -23
FIRST = (0.1, -0.2, 0.3, 0.05)          # (x, y, w, r) of the first step
SOS, EOS = 1, 2
LDS_BYTES = 64 * 1024
BT_MAX = {"T": 256, "L": 256, "K": 8, "A": 64}
BD_MAX = {"T": 32, "L": 256, "K": 8, "A": 64}

# One constant per family.  Rule (tests/kernel_edge_cases.py): the largest e_k / max(e_o, 2^-23) seen on the MI355X
# (the `boxgen-edge-max` lines of the parity log), times 4, rounded up to a power of two.  Beside each value: the
# family maximum of the run that set it, and the case and block it came from.
M = {
    "box_train": 16.0,       # 3.71   T70-second-lane-trip (d rnn.weight_ih_l0; every case but the one of M_CASE)
    "box_loss": 32.0,        # 7.7    T256-limit-lens-256-64-65-1 (dtrace[0,164].wh; every case but the one of M_CASE)
    "box_loss_alone": 16.0,  # 3.13   cpw8-B17-last-tile-all-zero (dtrace[11,0].xy)
    "box_clip": 2.0,         # 0.333  n65537 (the norm; the divisor is bit-equal to its definition in every case)
    "box_decode": 16.0,      # 2.98   tie-across-lanes-4-69 (trace[4])
}

# box_loss is above 16.  A row of the chain's dtrace is the loss gradient AT THE KERNELS' OWN TRACE, compared with the
# restatement's gradient at ITS trace.  The box term's d / d sigma goes with sigma^-3 and d / d u with 1 / (x - u), so
# the trace's own error (inside box_train's bound) comes back three-fold and more in dtrace: 1.0e-6 at step 164 of the
# 256-step caption, where the recurrence has carried the fp32 state that far (the oracle, whose LSTM sums in another
# order, has 1.3e-7 on that row).  That is the forward's figure, not the loss kernel's: the fifth
# family, box_loss_alone, runs the loss entry point on the restatement's trace rounded to fp32 against the fp64 loss of
# that rounded trace and stays at 3.13 (2.89 in the T = 256 case).
#
# One case is above these: box_train of norm-clamp-K1-tuned, 12.9 on box_sum[0] (7.37 on d xy_embedding.bias), every other
# block of it below 4.  The case sets the sigma entries of wh_out.bias to -7 to reach the normaliser clamp.  The kernels
# START each head's fmaf chain from the bias (acc = bias; acc = fmaf(w, x, acc) ...), so each of the 43 partial sums of
# a sigma logit is rounded at magnitude 7: 2^-24 * 8 per step, a random walk of 1e-6 rms (2.7e-6 worst of 200 trials in
# an fp32 emulation of that order on the CPU; 1.5e-7 rms with the bias added last, which is torch's order and the fp32
# oracle's).  sigma = exp(logit) turns that absolute error into a relative one, and the box term goes with
# z ~ sigma^-2 = 1e6 at the untuned steps: 2 d sigma / sigma = 2e-6 on box_sum, and on every gradient that the box
# term dominates.  The trace itself shows nothing (sigma is 1e-3 of the row's maximum).  With the biases of a trained
# or freshly initialised decoder (|b| < 1) the same chain keeps the oracle's level, which is what every other case
# measures.  dtrace of the chain sees the same sigma three-fold (d / d sigma ~ sigma^-3): 7.7e-6 on dtrace[1,2].wh, ratio
# 64.5.  The loss kernel is not involved: fed the reference's trace it stays at 1.22 in this case (box_loss_alone).
M_CASE = {("box_train", "norm-clamp-K1-tuned"): 64.0,     # 12.9   box_sum[0]
          ("box_loss", "norm-clamp-K1-tuned"): 256.0}     # 64.5   dtrace[1,2].wh


def m_bound(fam, case):
    return M_CASE.get((fam, case["id"]), M[fam])


# ---- weights -----------------------------------------------------------------------------------------------------------
def state_shapes(H, L, K, A):
    """nn-layout shapes of the decoder's 17 tensors, in the order of TO.KERNEL_KEYS"""
    return [(L, H), (A, 2), (A,), (A, 2), (A,), (A, 2), (A,), (4 * H, 2 * A + H), (4 * H, H), (4 * H,), (4 * H,),
            (L, H), (L,), (6 * K, H + L), (6 * K,), (6 * K, H + L + A), (6 * K,)]


def random_state(H, L, K, A, seed, scale=0.3):
    """a decoder state dict (keys of TO.KERNEL_KEYS, nn layout), uniform(-scale, scale) from one generator; built
    directly and not through DecoderRNN, whose next_xy / xy / wh embeddings are fixed at A = 50"""
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.rand(s, generator=g) * 2 - 1) * scale for k, s in zip(TO.KERNEL_KEYS, state_shapes(H, L, K, A))}


def to_kernel_layout(sd):
    """state dict -> the 17 contiguous tensors of the kernels' layout (the inverse of TO.to_state_layout)"""
    return [(sd[k].t() if i in TO.TRANSPOSED else sd[k]).contiguous() for i, k in enumerate(TO.KERNEL_KEYS)]


# ---- launch arithmetic, restated from bt_fwd_launch / bd_launch / objgan_box_train_backward ------------------------------
def train_lds_bytes(H, L, K, A, cpw):
    I, G, Q = 2 * A + H, 4 * H, 6 * K
    return 4 * cpw * (I + H + L + A + H + G + 2 * Q + 8 + 3)


def decode_lds_bytes(H, L, K, A, cpw):
    I, G, Q = 2 * A + H, 4 * H, 6 * K
    return 4 * cpw * (I + H + L + A + H + G + 2 * Q + 4 + 3)


def bptt_lds_bytes(H, cpw):
    return 4 * cpw * (2 * H + 4 * H)


def launch_facts(H, L, K, A, cpw, lens, T):
    """what a case reaches, from its shape alone"""
    clamped = [min(max(int(n), 0), T) for n in lens]
    B = len(lens)
    waves = (4 * H + 63) // 64
    tiles = [clamped[i:i + cpw] for i in range(0, B, cpw)]
    return {
        "threads": waves * 64, "waves": waves, "gate_rows_masked": 4 * H < waves * 64,
        "caption_trips": -(-cpw // waves),                      # trips of `for c = wid; c < CPW; c += nw`
        "loss_trips": -(-T // 64),                              # trips of `for t = lane; t < T; t += 64`
        "softmax_trips": -(-L // 64),
        "head_threads": 64 + 2 * K,
        "tiles": len(tiles), "tile_maxlen": [max(t) for t in tiles], "last_tile_captions": len(tiles[-1]) if tiles else 0,
        "clamped": clamped, "N": sum(clamped),
        "lds": train_lds_bytes(H, L, K, A, cpw), "lds_bptt": bptt_lds_bytes(H, cpw),
    }


# ---- training cases ------------------------------------------------------------------------------------------------------
def _tc(id, H, K, lens, L=9, A=10, cpw=4, T=None, seed=11, **kw):
    c = dict(id=id, H=H, K=K, L=L, A=A, lens=list(lens), cpw=cpw, seed=seed, pad=0, T=T, scale=0.3)
    c.update(kw)
    if c["T"] is None:
        c["T"] = max(max(c["lens"]), 1)
    return c


B17_LENS = [3, 1, 4, 1, 5, 2, 6, 5, 3, 5, 8, 2, 7, 1, 6, 4, 0]

TRAIN_CASES = [
    _tc("T70-second-lane-trip", 20, 2, [70, 1, 65, 3, 0]),
    _tc("T256-limit-lens-256-64-65-1", 20, 1, [256, 64, 65, 1]),
    _tc("cpw8-B11-partial-tile-zero-lens", 20, 1, [3, 1, 0, 7, 2, 5, 0, 4, 6, 1, 2], cpw=8),
    _tc("cpw8-B17-last-tile-all-zero", 16, 1, B17_LENS, cpw=8),
    _tc("lens-clamped", 16, 2, [9, -2, 6, 0, 3], T=6),
    _tc("all-lens-zero-N0", 16, 1, [0, 0, 0], T=3, no_reference=True),
    _tc("pad-inside-caption", 16, 2, [6, 4], pad_inside=[(0, 3)]),
    _tc("pad2", 16, 2, [6, 4], pad_inside=[(0, 3)], pad=2),
    _tc("norm-clamp-K1-tuned", 32, 1, [7, 4, 2], seed=31, sigma_bias=-7.0, tuned=True, norm_clamp=True),
    _tc("K8-limit", 12, 8, [4, 2, 6]),
    _tc("L65", 16, 2, [3, 5], L=65, set_labels=[(1, 2, 64)]),
    _tc("L256-limit", 16, 2, [3, 5], L=256, set_labels=[(0, 1, 64), (1, 1, 255), (1, 3, 128)]),
    _tc("A64-limit", 8, 2, [4, 2], A=64),
    _tc("A1", 8, 2, [4, 2], A=1),
    _tc("H2", 2, 2, [4, 2]),
    _tc("H16-one-full-wave", 16, 2, [4, 2]),
]
CPW_INVARIANT = "cpw8-B11-partial-tile-zero-lens"      # the batch whose bits are compared under cpw 1, 2, 4 and 8


def train_case(id):
    return next(c for c in TRAIN_CASES if c["id"] == id)


def build_train(case):
    """-> sd (nn layout, fp32), h0, c0 [B, H], labels [B, T + 1] int64, boxes [B, T + 1, 4] fp32, lens as the case
    passes them to the kernels, clamped lens (what the reference runs on), weight [L]"""
    H, L, K, A, T = case["H"], case["L"], case["K"], case["A"], case["T"]
    sd = random_state(H, L, K, A, case["seed"], case["scale"])
    if case.get("sigma_bias") is not None:
        sd["wh_out.bias"][3 * K:5 * K] = case["sigma_bias"]
    lens = case["lens"]
    clamped = [min(max(int(n), 0), T) for n in lens]
    B = len(lens)
    # a caption of zero steps still carries one step of targets, which nothing may read
    labels, boxes = TO.make_batch(case["seed"], [max(n, 1) for n in clamped], L)
    if labels.shape[1] - 1 < T:
        labels, boxes = TO.pad_batch(labels, boxes, T)
    for b, t, label in case.get("set_labels", ()):             # targets (and next inputs) in the later lane trips
        assert 0 < t < clamped[b]
        labels[b, t] = label
    for b, t in case.get("pad_inside", ()):
        assert 0 < t < clamped[b]
        labels[b, t] = 0                                      # a <pad> target before the end: mask = 0 at step t - 1
    g = torch.Generator().manual_seed(case["seed"] + 1)
    h0, c0 = torch.randn(B, H, generator=g) * 0.5, torch.randn(B, H, generator=g) * 0.5
    weight = torch.rand(L, generator=g) + 0.5
    if case.get("tuned"):
        # each caption's last (w, r) target placed inside its own wh component: z is O(1) at that step.  The target
        # feeds no later step, so the trace of one pass stays valid
        first = TO.step_ref(sd, h0, c0, labels, boxes, clamped, FIRST, weight, 1.0, 1.0, K, grad=False)
        o = L + 6 * K
        for b, n in enumerate(clamped):
            row = first["trace"][b, n - 1]
            boxes[b, n, 2] = np.float32(float(row[o + K]) + 0.5 * float(row[o + 3 * K]))
            boxes[b, n, 3] = np.float32(float(row[o + 2 * K]) - 0.25 * float(row[o + 4 * K]))
    return {"sd": sd, "h0": h0, "c0": c0, "labels": labels, "boxes": boxes, "lens": lens, "clamped": clamped,
            "weight": weight}


@functools.lru_cache(maxsize=None)
def train_reference(id, dtype=torch.float64):
    """the restatement of a case, computed once per precision and shared: do not modify"""
    case = train_case(id)
    b = build_train(case)
    return TO.step_ref(b["sd"], b["h0"], b["c0"], b["labels"], b["boxes"], b["clamped"], FIRST, b["weight"], 1.0, 1.0,
                       case["K"], dtype=dtype, dtrace=True, pad=case["pad"])


def max_err(a, ref):
    a, ref = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    if a.numel() == 0:
        return 0.0
    den = float(ref.abs().max())
    return float((a - ref).abs().max()) / (den if den > 0 else 1.0)


def train_blocks(case, r, clamped):
    """{family: {block name: tensor}} of a result in the form of step_ref (trace, sums, dtrace, grads).
    box_train: the chain end to end -- the trace and the two sums per caption, the 17 gradients.
    box_loss: the two sums per caption and every row of dtrace, in three segments (check_train_case hands in those of
    the loss entry point alone as well, as family box_loss_alone)."""
    L, Q = case["L"], 6 * case["K"]
    sums, dtrace = r["sums"], r["dtrace"]
    tr, ls = {}, {}
    for b, n in enumerate(clamped):
        if n == 0:
            continue
        tr["trace[%d]" % b] = r["trace"][b, :n]
        tr["label_sum[%d]" % b], tr["box_sum[%d]" % b] = r["sums"][b, 0], r["sums"][b, 1]
        ls["label_sum[%d]" % b], ls["box_sum[%d]" % b] = sums[b, 0], sums[b, 1]
        for t in range(n):
            row = dtrace[b, t]
            ls["dtrace[%d,%d].label" % (b, t)] = row[:L]
            ls["dtrace[%d,%d].xy" % (b, t)] = row[L:L + Q]
            ls["dtrace[%d,%d].wh" % (b, t)] = row[L + Q:]
    gr = {"d " + k: v for k, v in r["grads"].items()}
    return {"box_train": dict(tr, **gr), "box_loss": ls}


def compare(fam_blocks_k, fam_blocks_o, fam_blocks_r):
    """-> {family: (worst ratio e_k / max(e_o, 2^-23), its block, e_k, e_o)}"""
    out = {}
    for fam, ref in fam_blocks_r.items():
        worst = (0.0, None, 0.0, 0.0)
        for name, want in ref.items():
            e_k, e_o = max_err(fam_blocks_k[fam][name], want), max_err(fam_blocks_o[fam][name], want)
            ratio = e_k / max(e_o, EPS32)
            if ratio > worst[0] or worst[1] is None:
                worst = (ratio, name, e_k, e_o)
        out[fam] = worst
    return out


def rel_l2_tensors(r, ref):
    """rel_l2 of every whole tensor against the reference"""
    out = {"trace": TO.rel_l2(r["trace"], ref["trace"]), "dtrace": TO.rel_l2(r["dtrace"], ref["dtrace"]),
           "sums": TO.rel_l2(r["sums"][:, :2], ref["sums"][:, :2])}
    for k, v in ref["grads"].items():
        out["d " + k] = TO.rel_l2(r["grads"][k], v)
    return out


def _dev_batch(dev, batch):
    lab = torch.as_tensor(batch["labels"]).to(torch.int32).to(dev).contiguous()
    box = torch.as_tensor(batch["boxes"]).float().to(dev).contiguous()
    ln = torch.tensor(list(batch["lens"]), dtype=torch.int32, device=dev)
    return lab, box, ln


def _split_sums(sums):
    s = sums.cpu()
    per = s[:-1].view(-1, 4)
    return per[:, :3], [int(v) for v in per[:, 3]], float(s[-1])


def run_train(ops, dev, case, batch, cpw=None):
    """forward, loss, backward on the device, every output buffer NaN-filled beforehand where the wrapper lets the
    caller own it -> the form of step_ref: trace, sums [B, 3], matches, N, dtrace, grads {state key: tensor}"""
    W = [w.to(dev) for w in to_kernel_layout(batch["sd"])]
    lab, box, ln = _dev_batch(dev, batch)
    h0, c0 = batch["h0"].float().to(dev).contiguous(), batch["c0"].float().to(dev).contiguous()
    cpw = case["cpw"] if cpw is None else cpw
    trace, ws = ops.box_train_forward(h0, c0, lab, box, ln, W, FIRST, cpw=cpw)
    # the weights go in as they are: giving `pad` the weight zero is the kernel's part
    sums, dtrace = ops.box_train_loss(trace, lab, box, ln, batch["weight"].float().to(dev), 1.0, 1.0, case["K"],
                                      pad=case["pad"])
    grads = [torch.full(s, float("nan"), dtype=torch.float32, device=dev)
             for s in ops.box_weight_shapes(case["H"], case["L"], case["K"], case["A"])]
    ops.box_train_backward(dtrace, trace, c0, lab, ln, W, ws, grads=grads, cpw=cpw)
    torch.cuda.synchronize()
    per, matches, N = _split_sums(sums)
    return {"trace": trace.cpu(), "sums": per, "matches": matches, "N": N,
            "dtrace": dtrace.cpu(), "grads": {k: v.detach().cpu().clone() for k, v in TO.to_state_layout(grads).items()}}


def run_loss(ops, dev, case, batch, trace):
    """the loss entry point alone on a given trace -> sums [B, 3], matches, N, dtrace"""
    lab, box, ln = _dev_batch(dev, batch)
    sums, dtrace = ops.box_train_loss(trace.float().to(dev).contiguous(), lab, box, ln, batch["weight"].float().to(dev),
                                      1.0, 1.0, case["K"], pad=case["pad"])
    torch.cuda.synchronize()
    return _split_sums(sums) + (dtrace.cpu(),)


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_train_case(ops, dev, case, note=None):
    """one training case on the device against the fp64 restatement -> {family: worst ratio}"""
    batch = build_train(case)
    clamped = batch["clamped"]
    r = run_train(ops, dev, case, batch)
    again = run_train(ops, dev, case, batch)
    for k in r["grads"]:
        assert same_bits(r["grads"][k], again["grads"][k]), ("gradient bits differ run to run", k)
    for b, n in enumerate(clamped):                       # exact zeros (not NaN) past each clamped length
        assert not r["trace"][b, n:].any() and not r["dtrace"][b, n:].any(), ("not zero past the length", b, n)
        if n == 0:
            assert not r["sums"][b].any() and r["matches"][b] == 0, ("sums of an empty caption", b)
    for k in ("trace", "dtrace"):
        assert bool(torch.isfinite(r[k]).all()), k
    for k, v in r["grads"].items():
        assert bool(torch.isfinite(v).all()), ("unwritten or non-finite gradient element", k)
    if case.get("no_reference"):
        # N = 0: the reference divides by zero; the kernels' inv = 0 makes every output an exact zero
        assert r["N"] == 0.0 and not r["sums"].any() and not r["trace"].any() and not r["dtrace"].any()
        for k, v in r["grads"].items():
            assert not v.any(), k
        return {}
    ref, o32 = train_reference(case["id"]), train_reference(case["id"], torch.float32)
    assert [int(v) for v in r["sums"][:, 2]] == [int(v) for v in ref["sums"][:, 2]], "n per caption"
    assert r["matches"] == ref["matches"], "arg-max matches"
    assert r["N"] == float(ref["sums"][:, 2].sum()), "N"
    blocks_o, blocks_r = train_blocks(case, o32, clamped), train_blocks(case, ref, clamped)
    worst = compare(train_blocks(case, r, clamped), blocks_o, blocks_r)
    # box_loss_alone: the loss entry point fed the restatement's trace rounded to fp32, against the fp64 loss OF THAT
    # ROUNDED TRACE (box_loss, the chain's own dtrace, carries the forward's trace error besides, see M)
    t32 = ref["trace"].float()
    loss_sums, matches, N, loss_dtrace = run_loss(ops, dev, case, batch, t32)
    assert matches == ref["matches"] and N == r["N"]
    for b, n in enumerate(clamped):
        assert not loss_dtrace[b, n:].any(), ("not zero past the length", b, n)
    want, want32 = loss_reference(case, batch, t32), loss_reference(case, batch, t32, torch.float32)
    alone = [{"box_loss_alone": train_blocks(case, dict(r, sums=s_, dtrace=d_), clamped)["box_loss"]}
             for s_, d_ in ((loss_sums, loss_dtrace), want32, want)]
    worst.update(compare(*alone))
    l2 = rel_l2_tensors(r, ref)
    l2["dtrace of the reference trace"] = TO.rel_l2(loss_dtrace, want[1])
    for fam, (ratio, name, e_k, e_o) in worst.items():
        line = "%.3g  (%s: e_k %.3g, e_o %.3g)" % (ratio, name, e_k, e_o)
        print("boxgen-edge-max %s:%s %s" % (fam, case["id"], line))
        if note is not None:
            note("boxgen-edge-max %s:%s" % (fam, case["id"]), line)
    worst_l2 = max(l2, key=l2.get)
    print("boxgen-edge-rel_l2 %s worst %s %.3g" % (case["id"], worst_l2, l2[worst_l2]))
    if note is not None:
        note("boxgen-edge-rel_l2 %s (%s)" % (case["id"], worst_l2), "%.3g" % l2[worst_l2])
    for fam, (ratio, name, e_k, e_o) in worst.items():
        assert ratio <= m_bound(fam, case), (fam, case["id"], name, ratio, e_k, e_o)
    assert l2[worst_l2] <= TO.BOUND, (case["id"], worst_l2, l2[worst_l2])
    return {fam: w[0] for fam, w in worst.items()}


def check_cpw_invariance(ops, dev, case):
    """trace, dtrace and every gradient: the same bits under cpw 1, 2, 4 and 8"""
    batch = build_train(case)
    runs = {cpw: run_train(ops, dev, case, batch, cpw=cpw) for cpw in (1, 2, 4, 8)}
    for cpw in (2, 4, 8):
        assert same_bits(runs[1]["trace"], runs[cpw]["trace"]), ("trace", cpw)
        assert same_bits(runs[1]["dtrace"], runs[cpw]["dtrace"]), ("dtrace", cpw)
        assert torch.equal(runs[1]["sums"], runs[cpw]["sums"]), ("sums", cpw)
        for k in runs[1]["grads"]:
            assert same_bits(runs[1]["grads"][k], runs[cpw]["grads"][k]), ("gradient", k, cpw)


# ---- the loss alone, as a function of a given trace -----------------------------------------------------------------------
def row_terms(row, nl, box, weight, L, K, pad=0):
    """(label term, box term) of one (b, t) as a function of its trace row [L + 12K] (softmax, then the activated
    mixtures); nl: the step's target label, box: its four target values"""
    w = weight.to(row.dtype).clone()
    w[pad] = 0
    ps = row[:L].clamp(1e-5, 1)
    lt, bt = -w[nl] * ps[nl], torch.zeros((), dtype=row.dtype)
    if nl != 0:
        xy = tuple(row[L + i * K:L + (i + 1) * K] for i in range(6))
        wh = tuple(row[L + 6 * K + i * K:L + 6 * K + (i + 1) * K] for i in range(6))
        bt = -TO.pdf(xy, box[0], box[1]) - TO.pdf(wh, box[2], box[3])
    return lt, bt


def row_loss(row, nl, box, weight, N, L, K, pad=0):
    """the contribution of one (b, t) to the batch loss (lamda1 = lamda2 = 1)"""
    lt, bt = row_terms(row, nl, box, weight, L, K, pad)
    return (lt + bt) / N


def loss_reference(case, batch, trace, dtype=torch.float64):
    """Perplexity + BBLoss of a GIVEN trace (the loss entry point's own input) and the gradient with respect to it,
    row by row with autograd in `dtype` -> sums [B, 2], dtrace [B, T, L + 12K].  On the restatement's own fp64 trace
    it returns the restatement's sums and dtrace (tests/test_boxgen_edges_cpu.py)."""
    L, K, pad = case["L"], case["K"], case["pad"]
    clamped = batch["clamped"]
    labels = torch.as_tensor(batch["labels"])
    boxes = torch.as_tensor(batch["boxes"]).to(dtype)
    N = sum(int(labels[b, t + 1] != pad) for b, n in enumerate(clamped) for t in range(n))
    sums = torch.zeros((len(clamped), 2), dtype=torch.float64)
    dtrace = torch.zeros(tuple(trace.shape), dtype=dtype)
    for b, n in enumerate(clamped):
        for t in range(n):
            row = trace[b, t].detach().to(dtype).clone().requires_grad_(True)
            lt, bt = row_terms(row, int(labels[b, t + 1]), boxes[b, t + 1], batch["weight"], L, K, pad)
            dtrace[b, t] = torch.autograd.grad((lt + bt) / N, row)[0]
            sums[b, 0] += float(lt.detach())
            sums[b, 1] += float(bt.detach())
    return sums, dtrace


# ---- clip cases ------------------------------------------------------------------------------------------------------------
CLIP_NS = (1, 255, 256, 257, 65537)
CLIP_CASES = [dict(id="n%d" % n, n=n, seed=5 + n, kind="random") for n in CLIP_NS] + \
             [dict(id="n257-zero-gradient", n=257, seed=0, kind="zero")]


def clip_gradient(case):
    if case["kind"] == "zero":
        return torch.zeros(case["n"])
    return torch.randn(case["n"], generator=torch.Generator().manual_seed(case["seed"]))


def clip_facts(n):
    """bt_sumsq_kernel: 256 blocks of `chunk` elements; which blocks have work and where the `hi` clamp acts"""
    chunk = -(-n // 256)
    busy = -(-n // chunk)
    return {"chunk": chunk, "busy_blocks": busy, "empty_blocks": 256 - busy, "last_block_short": busy * chunk > n}


def clip_expected(g, max_norm):
    """-> fp64 norm, the fp32 divisor max(1, (fp32(norm) + 1e-6) / max_norm) evaluated in fp32"""
    norm = math.sqrt(float((g.double() ** 2).sum()))
    div = (np.float32(norm) + np.float32(1e-6)) / np.float32(max_norm)
    return norm, np.float32(max(np.float32(1.0), div))


def check_clip_case(ops, dev, case, note=None):
    g = clip_gradient(case)
    gd = g.to(dev)

    def run(max_norm):
        partials = torch.full((256,), float("nan"), dtype=torch.float64, device=dev)     # fresh, poisoned
        out = torch.full((2,), float("nan"), dtype=torch.float32, device=dev)
        ops.box_train_clip(gd, max_norm, partials=partials, out=out)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    out = run(5.0)
    norm, div = clip_expected(g, 5.0)
    if case["kind"] == "zero":
        assert out[1] == 0.0 and out[0] == 1.0, out
        return 0.0
    # the fp32 oracle of the norm is the fp64 value rounded once; the divisor's is its definition (e_o = 0)
    ratios = {"norm": (abs(float(out[1]) - norm) / norm, abs(float(np.float32(norm)) - norm) / norm),
              "divisor": (abs(float(out[0]) - float(div)) / float(div), 0.0)}
    ratio = max(e_k / max(e_o, EPS32) for e_k, e_o in ratios.values())
    line = "%.3g  (norm: e_k %.3g, e_o %.3g; divisor: e_k %.3g)" % ((ratio,) + ratios["norm"] + ratios["divisor"][:1])
    print("boxgen-edge-max box_clip:%s %s" % (case["id"], line))
    if note is not None:
        note("boxgen-edge-max box_clip:%s" % case["id"], line)
    assert ratio <= M["box_clip"], (case["id"], ratios)
    assert out[0] == max(np.float32(1.0), (out[1] + np.float32(1e-6)) / np.float32(5.0)), out     # of its own norm: exact
    # max_norm a factor 1 +- 2^-10 around the measured norm: the divisor is exactly 1 on one side, above 1 on the other
    measured = float(out[1])
    above, below = run(measured * (1 + 2.0 ** -10)), run(measured * (1 - 2.0 ** -10))
    assert above[0] == 1.0 and above[1] == out[1], above
    want = (out[1] + np.float32(1e-6)) / np.float32(measured * (1 - 2.0 ** -10))
    assert below[0] > 1.0 and abs(float(below[0]) - float(want)) <= M["box_clip"] * EPS32 * float(want), (below, want)
    assert below[1] == out[1], below
    return ratio


# ---- decode cases ----------------------------------------------------------------------------------------------------------
def _dc(id, H=16, K=2, L=9, A=10, T=6, B=8, cpw=4, seed=21, bias=None, **kw):
    c = dict(id=id, H=H, K=K, L=L, A=A, T=T, B=B, cpw=cpw, seed=seed, bias=dict(bias or {}), tie=None, scale=0.4)
    c.update(kw)
    return c


DECODE_CASES = [
    _dc("cpw8-B11-H20", H=20, B=11, cpw=8, seed=24, bias={EOS: 0.3}, same_bytes_as_cpw=1),
    _dc("T32-limit", K=1, T=32, B=4, bias={EOS: -9.0, 5: 1.0}),
    _dc("all-end-at-step-1", T=5, B=5, bias={EOS: 9.0}),
    _dc("K8-limit", K=8, T=3, B=4, bias={EOS: 0.3}),
    _dc("L130", L=130, T=3, B=4, bias={EOS: 1.0, 129: 2.0}),
    _dc("tie-same-lane-3-67", L=130, T=1, B=5, tie=(3, 67)),
    _dc("tie-across-lanes-5-70", L=130, T=1, B=5, tie=(5, 70)),
    # lane 0 meets an odd lane last: a butterfly that takes the other lane's entry on a tie ends on the larger index
    _dc("tie-across-lanes-4-69", L=130, T=1, B=5, tie=(4, 69)),
]


def decode_case(id):
    return next(c for c in DECODE_CASES if c["id"] == id)


def build_decode(case):
    H, L, K, A, T, B = (case[k] for k in "HLKATB")
    sd = random_state(H, L, K, A, case["seed"], case["scale"])
    for index, value in case["bias"].items():
        sd["l_out.bias"][index] += value
    if case["tie"]:
        lo, hi = case["tie"]
        sd["l_out.weight"][hi] = sd["l_out.weight"][lo]      # the same row and bias: the same bits in every arithmetic
        sd["l_out.bias"][lo] += 8.0
        sd["l_out.bias"][hi] = sd["l_out.bias"][lo]
    g = torch.Generator().manual_seed(case["seed"] + 1)
    h0, c0 = torch.rand(B, H, generator=g) * 2 - 1, torch.rand(B, H, generator=g) * 2 - 1
    rs = np.random.RandomState(case["seed"] + 2)
    noise = np.concatenate((rs.random_sample((B, T, 1)), rs.standard_normal((B, T, 2)),
                            rs.random_sample((B, T, 1)), rs.standard_normal((B, T, 2))), 2)
    return {"sd": sd, "h0": h0, "c0": c0, "noise": noise}


@functools.lru_cache(maxsize=None)
def decode_reference(id, dtype=torch.float64):
    """(labels, lengths, samples, trace, label margins, edge margins) of a case, computed once per precision: shared"""
    case = decode_case(id)
    b = build_decode(case)
    return BO.decode_ref(b["sd"], b["h0"], b["c0"], b["noise"], FIRST, SOS, EOS, case["K"], dtype=dtype)


def decode_keep(case):
    """captions the fp32 restatement decides with margin (the rule of test_small_shape_matches_restatement); a tie case
    has no label margin by construction, its label is stated instead"""
    _, _, _, _, lm, em = decode_reference(case["id"], torch.float32)
    ok = (np.asarray(em) >= BO.EDGE_MARGIN) if case["tie"] else BO.margins_ok(lm, em)
    return np.nonzero(ok)[0]


def run_decode(ops, dev, case, batch, cpw=None):
    W = [w.to(dev) for w in to_kernel_layout(batch["sd"])]
    out = ops.box_decode(batch["h0"].to(dev), batch["c0"].to(dev), torch.from_numpy(batch["noise"]).to(dev), W, FIRST,
                         SOS, EOS, trace=True, cpw=case["cpw"] if cpw is None else cpw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def check_decode_case(ops, dev, case, note=None):
    batch = build_decode(case)
    labels, lens, samples, trace = got = run_decode(ops, dev, case, batch)
    r64, r32 = decode_reference(case["id"]), decode_reference(case["id"], torch.float32)
    keep = decode_keep(case)
    assert len(keep) >= case["B"] - case["B"] // 4
    assert np.isfinite(samples).all() and np.isfinite(trace).all()
    for b in range(case["B"]):
        n = int(lens[b])
        assert 1 <= n <= case["T"]
        assert not labels[b, n:].any() and not samples[b, n:].any() and not trace[b, n:].any(), ("zero fill", b)
    if case["tie"]:
        assert (labels[:, 0] == case["tie"][0]).all(), ("the first maximum", labels[:, 0])
        assert (lens == 1).all()
    if case["id"] == "all-end-at-step-1":
        assert (lens == 1).all() and (labels[:, 0] == EOS).all()
    worst = (0.0, None, 0.0, 0.0)
    for b in keep:
        assert int(r32[1][b]) == int(r64[1][b]) and np.array_equal(r32[0][b], r64[0][b]), ("restatements disagree", b)
        assert int(lens[b]) == int(r64[1][b]), ("length", b)
        if not case["tie"]:
            assert np.array_equal(labels[b], r64[0][b]), ("labels", b)
        for name, i in (("samples", 2), ("trace", 3)):
            e_k, e_o = BO.trajectory_error(got[i][b], r64[i][b]), BO.trajectory_error(r32[i][b], r64[i][b])
            assert e_k <= TO.BOUND, (case["id"], name, b, e_k)
            ratio = e_k / max(e_o, EPS32)
            if ratio > worst[0] or worst[1] is None:
                worst = (ratio, "%s[%d]" % (name, b), e_k, e_o)
    line = "%.3g  (%s: e_k %.3g, e_o %.3g)" % worst
    print("boxgen-edge-max box_decode:%s %s" % (case["id"], line))
    if note is not None:
        note("boxgen-edge-max box_decode:%s" % case["id"], line)
    assert worst[0] <= M["box_decode"], (case["id"], worst)
    if case.get("same_bytes_as_cpw"):
        other = run_decode(ops, dev, case, batch, cpw=case["same_bytes_as_cpw"])
        for a, b in zip(got, other):
            assert a.tobytes() == b.tobytes(), "bytes differ between tile sizes"
    return worst[0]

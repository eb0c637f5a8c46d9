"""Edge-shape cases of the norm, attention, pooling, resize, optimiser, LSTM, ROIAlign and lift-stem kernels, with their
fp64 references, shared by tests/test_kernel_edges_cpu.py and tests/test_kernel_edges_gpu.py (no GPU import here).

One table per operator; every entry carries an `id` that names the branch of the host dispatch / the kernel it is there
for.  One `run_<operator>(ns, case, dtype, device)` per operator builds the seeded fp32 inputs of a case, casts them to
`dtype`, calls the operator of the namespace `ns` and returns {name: tensor} of EVERY output and gradient.  The same
runner serves three purposes:

    reference(op, case)   ns = REF (the plain definitions below) in float64 on the CPU
    oracle32(op, case)    ns = REF in float32 on the CPU (what the existing suite compares with; ROIAlign: the C oracle)
    the kernels           ns = objgan_hip.ops in float32 on the device (or tests/cpu_ops_shim.py on the CPU)

Metric per compared tensor (`max_err`): max |a - ref64| / max |ref64| (denominator 1 for an all-zero reference): a
maximum over elements, because a whole-tensor rel_l2 averages one wrong tail float4 away.  The kernel must satisfy
e_k <= M[family] * max(e_o, 2^-23) with e_o the same figure of the fp32 oracle, and the family's rel_l2 bound.
"""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_ref as tr

EPS32 = 2.0 ** -23

# One constant per operator family.  Rule: the largest e_k / max(e_o, 2^-23) seen on the MI355X (the parity log that
# conftest.note() writes, its `edge-max` lines), times 4 (the kernels add in slot / wave order, which is neither torch's
# order nor the same from shape to shape, and one seed is one sample), rounded up to a power of two.  Beside each value:
# the family maximum of the run that set it, and the case it came from.
#
# One tensor is above 16: running_var of the norm family in data variant c8 (31.2 on planes, 12.4 on the generic
# path).  It has a bound of its own (M_TENSOR below), so that y, dx, dgamma, dbeta, dres and running_mean of every norm
# case keep the family's.  The kernels take the variance from ONE pass of shifted sums,
# var = sum((x - K)^2) / n - (sum(x - K) / n)^2 with K = element 0 of the group.  With element 0 eight standard
# deviations from the mean the two terms are 65 var and 64 var: their fp32 rounding (2^-24 each, plus that of the
# partial sums) comes back 65-fold in the difference, 4e-6 relative, which is what the run shows (3.7e-6); torch's
# oracle centres on the mean in double and keeps 3e-8.  y, dx and the parameter gradients see the variance through
# rstd and stay at the oracle's level (ratios 0.5 .. 1.2 in the same case).
M = {
    "norm": 16.0,            # 2.28   bn-generic-2splits-boundary-inside-plane-data-b (dbeta; every tensor but running_var)
    "norm_eval": 8.0,        # 1.01   eval-plane-2x6x16x16-glu
    "attn_general": 8.0,     # 1.86   Q63-below-one-wave
    "attn_bu": 8.0,          # 1.25   B3-d50-idf48-R10-L12-normalized-no-mask
    "masked_max": 8.0,       # 1.03   R1-P257
    "softmax": 16.0,         # 2.28   rows-dim64-outer5-backward
    "bmm": 4.0,              # 1.00   Bt2-M64-N65-K16-A-broadcast-batch-stride0
    "bce": 4.0,              # 0.93   n1-target1-p-1e-30
    "pool": 4.0,             # 0.93   max-k3-s1-6x7-nine-windows-per-pixel
    "bilinear": 8.0,         # 1.19   IH1-1x6-to-4x12
    "fold": 4.0,             # 0.52   sum2x2-17x5
    "stream": 4.0,           # 1.00   adam-n600001-second-grid-stride-trip
    "lstm": 8.0,             # 1.21   max_len3-shorter-than-captions
    "roi": 8.0,              # 1.98   unstaged-many-taps (dfeat of the atomic scatter, 1.72 in another run; the ordered backward: 1.25, C64)
    "lift_taps": 8.0,        # 1.42   identity-5-to-5
    "lift_stem": 8.0,        # 1.07   1x3-to-4-h1
}

# Per-tensor exceptions to M: running_var of the norm family, for the reason above; the family's M then comes from
# every other norm tensor.
M_TENSOR = {("norm", "running_var"): 128.0}     # 31.2   bn-plane-hw8196-chunk-ends-in-one-float4-data-c8


def m_bound(fam, name):
    return M_TENSOR.get((fam, name), M[fam])


# rel_l2 bounds per family and tensor, kept here against the fp64 reference.  Each is the bound tests/test_kernels_gpu.py
# asserts for that tensor of that operator:
#   norm          y, dres, running statistics 1e-4 (TOL); dx, dgamma, dbeta 5e-4      test_norm_act_forward_backward
#   attn_general  1e-4 throughout; dsrc 5e-4 where the backward walks several chunks  test_attn_general(_large_query)
#   attn_bu       1e-4                                                                test_attn_bu
#   masked_max    out 1e-6, df 1e-4                                                   test_masked_max
#   softmax       y 1e-5, dx 1e-4                                                     test_softmax_strided
#   bmm           1e-5                                                                test_bmm_strided_matches_torch
#   bce           1e-5 (the loss there: |d| < 1e-5 max(1, |loss|); no looser here)    test_bce_const_matches_torch
#   pool          1e-6 (the average pools there; the maximum's dx: allclose 1e-6)     test_pooling_kernels_match_torch
#   bilinear      1e-5                                                                test_bilinear_resize
#   stream        p, m, v, avg 1e-6                                                   test_adam_and_ema, test_gated_adam_*
#   lstm          1e-5                                                                test_rnn_encoder_matches_oracle_*
#   roi           dfeat 1e-5 (y is bit-equal to the C oracle besides)                 test_roi_align_bit_exact
#   lift_stem     1e-4 (TOL), and the same for the four lift kernels alone            test_lift_stem_conv_matches_the_reference_formulation
# Tensors without an existing test:
#   norm_eval y   1e-4, the bound of the training-mode forward (the same apply arithmetic).
#   fold y        1e-6, as the average pools: a sum of four fp32 terms (sum2x2) or at most four (reflect_fold), each
#                 addition within 2^-24 of the partial sum.
#   stream update 1e-4: p - p0 is ~lr = 1e-2 while p (order 1) carries its fp32 rounding 2^-24 |p| = 6e-8, i.e. 6e-6 of
#                 the update per element before any arithmetic of the step itself; 1e-4 leaves a factor 16 over that.
RL2 = {
    "norm": {"y": 1e-4, "dres": 1e-4, "running_mean": 1e-4, "running_var": 1e-4, "dx": 5e-4, "dgamma": 5e-4, "dbeta": 5e-4},
    "norm_eval": {"y": 1e-4},
    "attn_general": {"wc": 1e-4, "attn": 1e-4, "dx": 1e-4, "dsrc": 1e-4},
    "attn_bu": {"wc": 1e-4, "attn": 1e-4, "dsrc": 1e-4},
    "masked_max": {"out": 1e-6, "df": 1e-4},
    "softmax": {"y": 1e-5, "dx": 1e-4},
    "bmm": {"C": 1e-5, "dA": 1e-5, "dB": 1e-5},
    "bce": {"loss": 1e-5, "dp": 1e-5},
    "pool": {"y": 1e-6, "dx": 1e-6},
    "bilinear": {"y": 1e-5, "dx": 1e-5},
    "fold": {"y": 1e-6},
    "stream": {"p": 1e-6, "m": 1e-6, "v": 1e-6, "avg": 1e-6, "update": 1e-4},
    "lstm": {"words": 1e-5, "sent": 1e-5},
    "roi": {"y": 1e-5, "dfeat": 1e-5},
    "lift_taps": {"y": 1e-4, "dz": 1e-4, "dbias": 1e-4},
    "lift_stem": {"y": 1e-4, "dseg": 1e-4, "dw": 1e-4, "db": 1e-4},
}
ATTN_DSRC_MULTI_CHUNK = 5e-4


def rl2_bound(fam, case, name):
    if fam == "attn_general" and name == "dsrc" and case["chunks"] > 1:
        return ATTN_DSRC_MULTI_CHUNK
    if fam == "bilinear":
        # The source coordinate scale * o is an fp32 product of an fp32 quotient (torch's definition, and the kernel's):
        # two roundings of 2^-24 of a coordinate of up to max(IH, IW), which become the error of the interpolation
        # weight and, times |x1 - x0| ~ sqrt(2) rms, of y and dx.  Against fp64 coordinates that is 2^-23 max(IH, IW)
        # for ANY fp32 implementation: below the 1e-5 of the existing test up to 83 pixels (its maps have at most 64),
        # 4.8e-5 on the 400-pixel map of the second-trip case (the fp32 oracle measures 3.1e-5 there).
        return max(RL2[fam][name], EPS32 * max(case["shape"][2], case["shape"][3]))
    if fam in ("lift_taps", "lift_stem"):
        # the same coordinate rule (the tables hold the fp32 source coordinates of bilinear_fwd_kernel): 8.7e-5 at the
        # 726 pixels of the second-trip case, so 1e-4 stays in force for every case here
        return max(RL2[fam][name], EPS32 * max(case["SH"], case["SW"]))
    return RL2[fam][name]


# launch geometry the cases rely on (tests/test_kernel_edges_cpu.py proves each against the built library / the sources)
NORM_CHUNK = 8192            # csrc/norm.hip OG_NORM_CHUNK
IN_FUSED_MAX = 65536         # csrc/norm.hip OG_IN_FUSED_MAX
SM_ROWS_MAX = 1024           # csrc/attention.hip 64 * OG_SM_PER
MM_RMAX = 16                 # csrc/attention.hip MM_RMAX
STREAM_ITEMS = 2048 * 256    # csrc/common.h og_stream_grid: work items of one trip of a grid-stride loop
ROI_MAX_SAMPLES = 256        # csrc/roi_align.hip: AH * AW a workgroup parks in LDS
ROI_TAB_MAX = 512            # rois per call the ordered backward takes
ROI_LDS_SMP = 1024           # samples of one image the gather kernel stages in LDS ...
ROI_LDS_G = 4096             # ... with nlist * nc * S top gradients of the slab
ROI_LDS_START = 4608         # anchor-range starts in LDS when HW + 1 <= this
ROI_SEQ = 24                 # a (pixel, channel) element with at most this many taps is summed by one lane
ROI_SUB = 16                 # lanes of the butterfly above it
LIFT_MAXE = 8                # csrc/lift_stem.hip: CSR entries of one source index an adjoint thread keeps in registers


def roi_cpb(channels):
    """channels per workgroup of roi_align_bwd_gather_kernel (objgan_roi_align_backward_ordered)"""
    return 8 if channels >= 64 else 1


def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case["id"].encode()) & 0x7FFFFFFF)


def _to(t, dtype, device, grad=False):
    if t is None:
        return None
    t = t.to(device=device, dtype=dtype if t.is_floating_point() else t.dtype)
    return t.requires_grad_() if grad else t


# =====================================================================================================================
# metric
# =====================================================================================================================
def _clean(a, ref):
    """(a, ref) as float64 CPU tensors with the positions where ref is NaN / infinite zeroed in both -- after checking
    that `a` holds exactly the same NaN / infinity there."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (tuple(a.shape), tuple(ref.shape))
    bad = ~torch.isfinite(ref)
    if bool(bad.any()):
        assert torch.equal(torch.isnan(a), torch.isnan(ref)), "NaN at different positions"
        inf = torch.isinf(ref)
        assert torch.equal(a[inf], ref[inf]), "infinities differ"
        a, ref = a.masked_fill(bad, 0.0), ref.masked_fill(bad, 0.0)
    return a, ref


def max_err(a, ref):
    a, ref = _clean(a, ref)
    if ref.numel() == 0:
        return 0.0
    den = float(ref.abs().max())
    return float((a - ref).abs().max()) / (den if den > 0 else 1.0)


def rel_l2(a, ref):
    a, ref = _clean(a, ref)
    den = float(torch.linalg.vector_norm(ref))
    return float(torch.linalg.vector_norm(a - ref)) / (den if den > 0 else 1.0)


# =====================================================================================================================
# REF: the plain definitions (dtype-agnostic; float64 = the reference, float32 = the oracle)
# =====================================================================================================================
class _MaskedMaxFirst(torch.autograd.Function):
    """out[b, c, p] = max_r f[b, c, r] * m[b, r, (c,) p] with an EXPLICIT first-occurrence arg-max in the backward
    (autograd's max spreads / picks ties by its own rule; the kernel documents "first max wins")."""

    @staticmethod
    def forward(ctx, f, m, ih, iw):
        B, num, R = f.shape[0], f.shape[1], f.shape[2]
        P = ih * iw
        f3 = f.reshape(B, num, R)
        if m.dim() == 4:
            m4 = m.reshape(B, 1, R, P).expand(B, num, R, P)
        else:
            m4 = m.reshape(B, R, num, P).permute(0, 2, 1, 3)
        prod = f3.unsqueeze(3) * m4                                   # [B, num, R, P]
        best = prod.max(dim=2).values
        slot = torch.arange(R).view(1, 1, R, 1)
        arg = torch.where(prod == best.unsqueeze(2), slot, torch.full_like(slot, R)).min(dim=2).values
        ctx.save_for_backward(m4, arg)
        ctx.fshape = tuple(f.shape)
        return best.reshape(B, num, ih, iw)

    @staticmethod
    def backward(ctx, dout):
        m4, arg = ctx.saved_tensors
        B, num, R, P = m4.shape
        hit = arg.unsqueeze(2) == torch.arange(R).view(1, 1, R, 1)
        df = (dout.reshape(B, num, 1, P) * m4 * hit).sum(dim=3)
        return df.reshape(ctx.fshape), None, None, None


def roi_geometry_np(rois, H, W, AH, AW, scale):
    """The sample geometry of ROIAlign in the arithmetic the header of csrc/roi_align.hip documents: roi quantities are
    float; `end - start + 1.`, `size / (aligned - 1.)` are evaluated in double and rounded to float; h = ph * bin + start
    is a float product, then a float sum; hstart = (int) fminf(floor(h), H - 2).  rois [n, 5] float32 with an integer
    image index -> per (roi, sample = ph * AW + pw): off = hstart * W + wstart, valid, h_ratio, w_ratio (float32), and
    image [n]."""
    f32, f64 = np.float32, np.float64
    r = np.asarray(rois, f32)
    sc = f32(scale)
    start_w, start_h, end_w, end_h = r[:, 1] * sc, r[:, 2] * sc, r[:, 3] * sc, r[:, 4] * sc
    roi_w = np.maximum(((end_w - start_w).astype(f64) + 1.0).astype(f32), f32(0))
    roi_h = np.maximum(((end_h - start_h).astype(f64) + 1.0).astype(f32), f32(0))
    bin_h = (roi_h.astype(f64) / (f64(AH) - 1.0)).astype(f32)
    bin_w = (roi_w.astype(f64) / (f64(AW) - 1.0)).astype(f32)
    ph = np.repeat(np.arange(AH), AW).astype(f32)[None, :]
    pw = np.tile(np.arange(AW), AH).astype(f32)[None, :]
    h = (ph * bin_h[:, None]).astype(f32) + start_h[:, None]
    w = (pw * bin_w[:, None]).astype(f32) + start_w[:, None]
    assert h.dtype == f32 and w.dtype == f32
    hstart = np.minimum(np.floor(h.astype(f64)).astype(f32), f32(H - 2)).astype(np.int64)
    wstart = np.minimum(np.floor(w.astype(f64)).astype(f32), f32(W - 2)).astype(np.int64)
    valid = ~((h < 0) | (h >= f32(H)) | (w < 0) | (w >= f32(W)))
    return dict(off=hstart * W + wstart, hstart=hstart, wstart=wstart, valid=valid, h_ratio=h - hstart.astype(f32),
                w_ratio=w - wstart.astype(f32), image=r[:, 0].astype(np.int64))


def _group_count(x, per_channel):
    return x[0, 0].numel() * (x.shape[0] if per_channel else 1)


class _Ref(object):
    @staticmethod
    def norm_act(x, gamma=None, beta=None, residual=None, running_mean=None, running_var=None, per_channel=False,
                 mode=None, eps=1e-5, momentum=0.1):
        """oracle.torch_ref.norm_act; a group of ONE value, which torch refuses in training mode and the kernels define
        (var = 0, no unbiasing), in closed form: xhat = 0, so z = beta (or 0), y = act(z) + residual, dx = 0,
        dgamma = 0, dbeta = sum dz, running_mean = (1 - momentum) rm + momentum x, running_var = (1 - momentum) rv."""
        if _group_count(x, per_channel) > 1:
            return tr.norm_act(x, gamma, beta, residual, running_mean, running_var, per_channel, mode, eps, momentum)
        z = x * 0.0
        if gamma is not None:
            z = z * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
        if per_channel and running_mean is not None:
            with torch.no_grad():
                running_mean.mul_(1.0 - momentum).add_(x.detach()[0, :, 0, 0], alpha=momentum)
                running_var.mul_(1.0 - momentum)
        y = tr.glu(z) if mode == "glu" else F.leaky_relu(z, 0.2) if mode == "lrelu" else z
        return y if residual is None else y + residual

    attn_general = staticmethod(tr.attn_general)
    attn_bu = staticmethod(tr.attn_bu)
    bilinear_resize = staticmethod(tr.bilinear_resize)
    avgpool2s1 = staticmethod(tr.avgpool2s1)
    bmm = staticmethod(torch.bmm)

    @staticmethod
    def norm_act_eval(x, gamma, beta, running_mean, running_var, mode=None, eps=1e-5):
        """the closed formula of eval-mode BatchNorm + activation"""
        v = lambda t: t.view(1, -1, 1, 1)
        y = (x - v(running_mean)) / torch.sqrt(v(running_var) + eps) * v(gamma) + v(beta)
        if mode == "glu":
            return tr.glu(y)
        return F.leaky_relu(y, 0.2) if mode == "lrelu" else y

    @staticmethod
    def masked_max(f, m, ih, iw):
        return _MaskedMaxFirst.apply(f, m, ih, iw)

    @staticmethod
    def softmax_strided(x, dim, scale=1.0, lens=None, rowvalid=None):
        """torch.softmax on the truncated span, zeros elsewhere"""
        d = dim % x.dim()
        outer = int(math.prod(x.shape[:d]))
        n = x.shape[d]
        xs = (x * scale).reshape(outer, n, -1)
        rows = []
        for o in range(outer):
            span = n if lens is None else max(0, min(n, int(lens[o % lens.numel()])))
            live = rowvalid is None or int(rowvalid[o]) != 0
            y = torch.zeros_like(xs[o])
            if span > 0 and live:
                y = torch.cat([torch.softmax(xs[o, :span], dim=0), y[span:]], dim=0)
            rows.append(y)
        return torch.stack(rows).reshape(x.shape)

    @staticmethod
    def bce_const(prob, target):
        return F.binary_cross_entropy(prob, torch.full_like(prob, float(target)))

    @staticmethod
    def max_pool2d(x, kernel_size, stride):
        return F.max_pool2d(x, kernel_size, stride)

    @staticmethod
    def avg_pool2d(x, kernel_size, stride=None, padding=0):
        return F.avg_pool2d(x, kernel_size, stride, padding)

    @staticmethod
    def sum2x2(dy, h, w):
        """adjoint of F.interpolate(scale_factor=2, mode='nearest'): dy [P, 2h, 2w] -> [P, h, w]"""
        x = torch.zeros(dy.shape[0], 1, h, w, dtype=dy.dtype, requires_grad=True)
        F.interpolate(x, scale_factor=2, mode="nearest").backward(dy.unsqueeze(1))
        return x.grad[:, 0]

    @staticmethod
    def reflect_fold(dxp, h, w):
        """adjoint of F.pad(mode='reflect') by one pixel: dxp [P, h + 2, w + 2] -> [P, h, w]"""
        x = torch.zeros(dxp.shape[0], 1, h, w, dtype=dxp.dtype, requires_grad=True)
        F.pad(x, (1, 1, 1, 1), mode="reflect").backward(dxp.unsqueeze(1))
        return x.grad[:, 0]

    @staticmethod
    def adam_step_(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0, n=None):
        pn, mn, vn = tr.adam_step(p, g * grad_scale, m, v, lr, beta1, beta2, eps, step)
        p.copy_(pn)
        m.copy_(mn)
        v.copy_(vn)

    @staticmethod
    def ema_update_(avg, p, decay):
        avg.mul_(decay).add_(p, alpha=1.0 - decay)

    @staticmethod
    def lstm_bidir_forward(table, captions, lens, wt_ih, wt_hh, b_ih, b_hh, max_len):
        """torch.nn.LSTM per caption on its first `len` tokens; ids clamped to [0, ntoken), len to [0, L] (the kernel's
        header); words [B, 2H, max_len] zero from t = len on, sent [B, 2H] = [forward h_n | reverse h_n], zero for len 0."""
        B, L = captions.shape
        I, H = wt_ih.shape[1], wt_ih.shape[2] // 4
        rnn = torch.nn.LSTM(I, H, batch_first=True, bidirectional=True).to(table.dtype)
        with torch.no_grad():
            for d, suffix in enumerate(("", "_reverse")):
                getattr(rnn, "weight_ih_l0" + suffix).copy_(wt_ih[d].t())
                getattr(rnn, "weight_hh_l0" + suffix).copy_(wt_hh[d].t())
                getattr(rnn, "bias_ih_l0" + suffix).copy_(b_ih[d])
                getattr(rnn, "bias_hh_l0" + suffix).copy_(b_hh[d])
            emb = table[captions.clamp(0, table.shape[0] - 1)]
            words = torch.zeros(B, 2 * H, int(max_len), dtype=table.dtype)
            sent = torch.zeros(B, 2 * H, dtype=table.dtype)
            for b in range(B):
                n = max(0, min(L, int(lens[b])))
                if n == 0:
                    continue
                out, (hn, _) = rnn(emb[b:b + 1, :n])
                t = min(n, int(max_len))
                words[b, :, :t] = out[0, :t].t()
                sent[b] = torch.cat([hn[0, 0], hn[1, 0]])
        return words, sent

    @staticmethod
    def roi_align(features, rois, aligned_height, aligned_width, spatial_scale):
        """ROIAlign as csrc/roi_align.hip states it.  Which four pixels a sample reads (hstart, wstart), whether it
        counts (valid) and its fractional offsets (h_ratio, w_ratio) are the operator's DEFINITION: an index decision,
        taken once by roi_geometry_np in the float / double mix of the C reference.  Everything after it runs in the
        dtype of `features`: the four weights, the forward sum, and (autograd of index_select) the index_add_ scatter
        of the backward.  An invalid sample reads pixel 0 with four zero weights."""
        B, C, H, W = features.shape
        geo = roi_geometry_np(rois.detach().cpu().numpy(), H, W, aligned_height, aligned_width, spatial_scale)
        n, S = geo["valid"].shape
        dt = features.dtype
        ok = torch.from_numpy(geo["valid"]).to(dt)
        hr, wr = torch.from_numpy(geo["h_ratio"]).to(dt), torch.from_numpy(geo["w_ratio"]).to(dt)
        base = torch.from_numpy(np.where(geo["valid"], geo["image"][:, None] * (H * W) + geo["off"], 0).astype(np.int64))
        planes = features.permute(0, 2, 3, 1).reshape(B * H * W, C)
        y = 0
        for step, wt in ((0, (1 - hr) * (1 - wr)), (1, (1 - hr) * wr), (W, hr * (1 - wr)), (W + 1, hr * wr)):
            y = y + (ok * wt).reshape(n * S, 1) * planes.index_select(0, (base + step).reshape(-1))
        return y.reshape(n, aligned_height, aligned_width, C).permute(0, 3, 1, 2)

    class _LiftTapsFn(object):
        """ops._LiftTapsFn as the operator reads: z [N, 9 Mo, h, w], channel (dh * 3 + dw) * Mo + co = tap (dh, dw) of
        output channel co; y = bias + sum over the taps of the (dh, dw) window of reflect_pad(lift(z_tap))."""

        @staticmethod
        def apply(z, bias, SH, SW):
            Mo = z.shape[1] // 9
            y = 0
            for dh in range(3):
                for dw in range(3):
                    t = dh * 3 + dw
                    up = F.interpolate(z[:, t * Mo:(t + 1) * Mo], size=(SH, SW), mode="bilinear", align_corners=True)
                    y = y + F.pad(up, (1, 1, 1, 1), mode="reflect")[:, :, dh:dh + SH, dw:dw + SW]
            return y if bias is None else y + bias.view(1, -1, 1, 1)

    @staticmethod
    def lift_stem_conv(seg, w, bias, size):
        """the formula of tests/cpu_ops_shim.lift_stem_conv (reference model.py:1217-1226)"""
        up = F.interpolate(seg, size=(size, size), mode="bilinear", align_corners=True)
        return F.conv2d(F.pad(up, (1, 1, 1, 1), mode="reflect"), w, bias)


REF = _Ref()


# =====================================================================================================================
# norm
# =====================================================================================================================
# Data variants:
#   a   randn * 2 + 3
#   b   channel 0 constant (2.5: var == 0), the last channel = 1 + k * 2^-23 with k in 0 .. 3 (values that differ in the
#       last ulps only; under GLU a gate, so that no output channel is all zero), the rest as (a)
#   c0  mean 1e3, standard deviation 1.0, element 0 of every plane near the mean
#   c8  the same with element 0 of every plane eight standard deviations away (the shifted sums use element 0 as shift)
# Variant (c) magnitudes: with standard deviation 1e-1 at mean 1e3 the fp32 ORACLE is already 2e-4 .. 4e-4 away from
# fp64 in rel_l2 (the fp32 rounding of the mean, 3e-5, is 3e-4 standard deviations) -- above the family's 1e-4 bound,
# which stays; 1e3 / 1.0 leaves the oracle at 3e-5.
C_MEAN, C_STD = 1.0e3, 1.0
BN, IN = True, False


def _norm(cid, N, C, H, W, pc, mode, affine=False, res=False, data="a", eps=1e-5, P=1, plane=False, fused=False):
    return dict(id=cid, shape=(N, C, H, W), pc=pc, mode=mode, affine=affine, res=res, data=data, eps=eps,
                P=P, plane=plane, fused=fused)


_NORM_BASE = [
    # generic statistics path (HW % 4 != 0 or HW < 256) with more than one split per group: norm_stats_kernel /
    # norm_bwd_stats_kernel with gridDim.y > 1, then norm_partials_sum_kernel
    _norm("bn-generic-2splits-boundary-inside-plane", 9, 6, 15, 15, BN, "glu", affine=True, P=2),
    _norm("bn-generic-3splits", 5, 3, 21, 21, BN, "lrelu", affine=True, P=3),
    _norm("in-generic-2splits", 1, 4, 33, 35, IN, "glu", P=2),
    # HW = 65540 > OG_IN_FUSED_MAX: the three-kernel plane path with per_channel = 0; ninth chunk = one float4
    _norm("in-plane-unfused-hw65540-last-chunk-one-float4", 1, 2, 4, 16385, IN, None, res=True, P=9, plane=True),
    _norm("in-fused-at-limit-hw65536", 1, 2, 256, 256, IN, "glu", P=8, plane=True, fused=True),
    _norm("bn-plane-hw8196-chunk-ends-in-one-float4", 2, 4, 2, 4098, BN, "glu", affine=True, P=4, plane=True),
    _norm("bn-plane-hw8192-mode-none-residual", 2, 3, 64, 128, BN, None, affine=True, res=True, P=2, plane=True),
    # a group of ONE value: var == 0 and the `cnt > 1` branch of the unbiased variance (closed-form reference, torch
    # refuses such a group in training mode) ...
    _norm("bn-count1-var0-mode-none", 1, 1, 1, 1, BN, None),
    _norm("in-count1-var0-lrelu", 2, 2, 1, 1, IN, "lrelu"),
    # ... and the smallest groups torch defines
    _norm("bn-count2-mode-none", 2, 1, 1, 1, BN, None),
    _norm("in-count2-lrelu", 2, 2, 1, 2, IN, "lrelu"),
    # neighbours: fused InstanceNorm below its limit with a residual, BatchNorm + LeakyReLU on planes
    _norm("in-fused-16x16-residual", 2, 4, 16, 16, IN, None, res=True, plane=True, fused=True),
    _norm("bn-plane-lrelu-16x20", 3, 5, 16, 20, BN, "lrelu", affine=True, P=3, plane=True),
    # second trip of norm_apply_kernel's / norm_bwd_apply_kernel's grid-stride loop: odd HW, 526338 elements
    _norm("bn-generic-apply-second-grid-stride-trip", 1, 2, 513, 513, BN, "lrelu", affine=True, P=258),
]
# data variants (b) and (c) over a plane subset and a generic subset, modes None and GLU.  LeakyReLU runs on variant (a)
# only (bn-generic-3splits, bn-plane-lrelu-16x20, in-count2-lrelu, the second-trip case): its derivative jumps from 0.2
# to 1 at z == 0, and which side an element falls on is not a defined comparison in (b), where the constant channel
# gives z == beta everywhere, nor in (c), where the fp32 rounding of x at mean 1e3 (6e-5 deviations) moves elements
# across z == 0: on bn-generic-3splits with data c0 the fp32 ORACLE's dx is 8.5e-2 from fp64 in the maximum metric.
_NORM_VARIANT_OF = ("bn-plane-hw8196-chunk-ends-in-one-float4", "in-fused-16x16-residual",
                    "bn-generic-2splits-boundary-inside-plane", "in-generic-2splits")


def _norm_cases():
    out = []
    for i, c in enumerate(_NORM_BASE):
        # half of the cases with a non-default eps; the groups of two values always (dx = rstd * (dy0 - dy1) / 2 *
        # eps / (var + eps) there: with eps = 1e-5 the fp32 oracle itself is 6e-4 away in rel_l2)
        out.append(dict(c, eps=1e-3 if (i % 2 or "count2" in c["id"]) else 1e-5))
    base = {c["id"]: c for c in out}
    for cid in _NORM_VARIANT_OF:
        for v in ("b", "c0", "c8"):
            out.append(dict(base[cid], id="%s-data-%s" % (cid, v), data=v))
    return out


NORM_CASES = _norm_cases()
NORM_MOMENTUM = 0.3


def _norm_data(case, g):
    N, C, H, W = case["shape"]
    v = case["data"]
    if v in ("a", "b"):
        x = torch.randn(N, C, H, W, generator=g) * 2 + 3.0
        if v == "b":
            x[:, 0] = 2.5
            x[:, C - 1] = 1.0 + torch.randint(0, 4, (N, H, W), generator=g).float() * 2.0 ** -23
        return x
    x = C_MEAN + C_STD * torch.randn(N, C, H, W, generator=g)
    x[:, :, 0, 0] = C_MEAN + (0.01 if v == "c0" else 8.0) * C_STD
    return x


def run_norm(ns, case, dtype, device):
    N, C, H, W = case["shape"]
    pc, mode, affine = case["pc"], case["mode"], case["affine"]
    g = _gen(case)
    Co = C // 2 if mode == "glu" else C
    x = _to(_norm_data(case, g), dtype, device, True)
    gamma = _to(torch.randn(C, generator=g) * 0.2 + 1, dtype, device, True) if affine else None
    beta = _to(torch.randn(C, generator=g) * 0.1, dtype, device, True) if affine else None
    res = _to(torch.randn(N, Co, H, W, generator=g), dtype, device, True) if case["res"] else None
    # BatchNorm starts from random running statistics with momentum 0.3: a wrong (1 - momentum) shows
    rm = _to(torch.randn(C, generator=g) * 0.5, dtype, device) if pc else None
    rv = _to(torch.rand(C, generator=g) + 0.5, dtype, device) if pc else None
    gy = _to(torch.randn(N, Co, H, W, generator=g), dtype, device)
    y = ns.norm_act(x, gamma, beta, res, rm, rv, pc, mode, case["eps"], NORM_MOMENTUM)
    y.backward(gy)
    out = {"y": y, "dx": x.grad}
    if affine:
        out.update(dgamma=gamma.grad, dbeta=beta.grad)
    if res is not None:
        out["dres"] = res.grad
    if pc:
        out.update(running_mean=rm, running_var=rv)
    return out


NORM_EVAL_CASES = [dict(id="eval-%s-%s" % (name, mode), shape=shape, mode=mode, plane=plane, eps=eps)
                   for name, shape, plane in (("plane-2x6x16x16", (2, 6, 16, 16), True), ("generic-3x6x5x7", (3, 6, 5, 7), False))
                   for mode, eps in ((None, 1e-5), ("lrelu", 1e-3), ("glu", 1e-5))]


def run_norm_eval(ns, case, dtype, device):
    N, C, H, W = case["shape"]
    g = _gen(case)
    x = _to(torch.randn(N, C, H, W, generator=g) * 2 + 3.0, dtype, device)
    gamma = _to(torch.randn(C, generator=g) * 0.2 + 1, dtype, device)
    beta = _to(torch.randn(C, generator=g) * 0.1, dtype, device)
    rm = _to(torch.randn(C, generator=g) * 0.5 + 3.0, dtype, device)
    rv = _to(torch.rand(C, generator=g) * 4 + 0.5, dtype, device)
    with torch.no_grad():
        return {"y": ns.norm_act_eval(x, gamma, beta, rm, rv, case["mode"], case["eps"])}


# =====================================================================================================================
# attention
# =====================================================================================================================
def _ag(cid, B, idf, ih, iw, L, mask=True, dattn=True, chunks=1):
    return dict(id=cid, B=B, idf=idf, ih=ih, iw=iw, L=L, mask=mask, dattn=dattn, chunks=chunks)


ATTN_GENERAL_CASES = (
    # attn_general<32> / <48> / <64>, each with L = 1, 7 and 16 (deadbits: no padded word at L = 16)
    [_ag("idf%d-L%d" % (idf, L), 2, idf, 5, 6, L) for idf in (32, 48, 64) for L in (1, 7, 16)] +
    [_ag("Q1", 3, 48, 1, 1, 7), _ag("Q63-below-one-wave", 3, 48, 7, 9, 7),
     _ag("Q257-one-pixel-in-second-workgroup", 3, 48, 1, 257, 7)] +
    # backward waves that walk 2 / 8 chunks of 64 pixels and end in a ragged chunk
    [_ag("Q8451-chunks2-ragged%s" % ("" if da else "-no-dattn"), 1, 48, 1, 8451, 12, dattn=da, chunks=2) for da in (True, False)] +
    [_ag("Q32833-chunks8-ragged%s" % ("" if da else "-no-dattn"), 1, 48, 1, 32833, 12, dattn=da, chunks=8) for da in (True, False)])
ATTN_GENERAL_REJECTED = [_ag("L17-rejected", 2, 48, 4, 4, 17, mask=False), _ag("idf40-rejected", 2, 40, 4, 4, 7, mask=False)]


def _ragged_mask(B, L, g):
    """mask[b, l] = True past a random length >= 1 (every row keeps a live word), row 0 unmasked"""
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    return torch.arange(L).unsqueeze(0) >= lens.unsqueeze(1)


def run_attn_general(ns, case, dtype, device):
    B, idf, ih, iw, L = case["B"], case["idf"], case["ih"], case["iw"], case["L"]
    g = _gen(case)
    x = _to(torch.randn(B, idf, ih, iw, generator=g), dtype, device, True)
    src = _to(torch.randn(B, idf, L, generator=g) * 0.3, dtype, device, True)
    mask = _to(_ragged_mask(B, L, g), dtype, device) if case["mask"] else None
    gw = _to(torch.randn(B, idf, ih, iw, generator=g), dtype, device)
    ga = _to(torch.randn(B, L, ih, iw, generator=g), dtype, device)
    wc, attn = ns.attn_general(x, src, mask)
    loss = (wc * gw).sum()
    if case["dattn"]:
        loss = loss + (attn * ga).sum()
    loss.backward()
    return {"wc": wc, "attn": attn, "dx": x.grad, "dsrc": src.grad}


def _bu(cid, B, d2, idf, R, L, normalize, mask, zero_tgt=False):
    return dict(id=cid, B=B, d2=d2, idf=idf, R=R, L=L, normalize=normalize, mask=mask, zero_tgt=zero_tgt)


ATTN_BU_CASES = (
    [_bu("B%d-d%d-idf%d-R%d-L%d-%s-%s" % (B, d2, idf, R, L, "normalized" if nz else "raw-scores", "ragged-mask" if mk else "no-mask"),
         B, d2, idf, R, L, nz, mk)
     for (B, d2, idf, R, L) in ((1, 50, 48, 1, 1), (3, 50, 48, 10, 12), (2, 7, 32, 16, 3))
     for nz in (True, False) for mk in (False, True)] +
    [_bu("zero-label-vector-eps-clamp", 3, 50, 48, 10, 12, True, True, zero_tgt=True)])


def run_attn_bu(ns, case, dtype, device):
    B, d2, idf, R, L = case["B"], case["d2"], case["idf"], case["R"], case["L"]
    g = _gen(case)
    tgt = torch.randn(B, d2, R, 1, generator=g)
    if case["zero_tgt"]:
        tgt[:, :, 0] = 0.0                  # |tgt| |ctx| = 0 -> the eps clamp
    ctx1 = torch.randn(B, d2, L, generator=g)
    if not case["normalize"]:
        ctx1 = ctx1 * 0.3                   # raw scores of a few units, as the normalised ones
    src = _to(torch.randn(B, idf, L, generator=g), dtype, device, True)
    mask = _to(_ragged_mask(B, L, g), dtype, device) if case["mask"] else None
    gw = _to(torch.randn(B, idf, R, 1, generator=g), dtype, device)
    wc, attn = ns.attn_bu(_to(tgt, dtype, device), _to(ctx1, dtype, device), src, mask, case["normalize"])
    (wc * gw).sum().backward()
    return {"wc": wc, "attn": attn, "dsrc": src.grad}


def _mm(cid, B, num, R, ih, iw, mask="shared", tie=False):
    return dict(id=cid, B=B, num=num, R=R, ih=ih, iw=iw, mask=mask, tie=tie)


MASKED_MAX_CASES = (
    [_mm("R%d-P%d" % (R, ih * iw), 2, 5, R, ih, iw) for R in (1, 16) for (ih, iw) in ((1, 1), (1, 257))] +
    # a CONTIGUOUS 5-D mask that differs per channel: m_stride_c != 0
    [_mm("mask5d-per-channel-R%d" % R, 2, 5, R, 7, 9, mask="per_channel") for R in (3, 16)] +
    [_mm("nonzero-ties-first-max-wins", 2, 6, 4, 9, 9, tie=True)])
MASKED_MAX_REJECTED = [_mm("R17-rejected", 1, 3, 17, 2, 2)]
TIE_RECT = (slice(2, 7), slice(3, 8))        # where the binary masks of slots 1 and 3 overlap (slot 3 lives only there)


def masked_max_inputs(case):
    B, num, R, ih, iw = case["B"], case["num"], case["R"], case["ih"], case["iw"]
    g = _gen(case)
    f = torch.randn(B, num, R, 1, generator=g)
    shape = (B, R, ih, iw) if case["mask"] == "shared" else (B, R, num, ih, iw)
    m = (torch.rand(shape, generator=g) > 0.4).float() * torch.rand(shape, generator=g)
    if case["tie"]:
        # two boxes of one class: identical f rows (both signs over the channels), binary masks that overlap on a
        # rectangle -> products tie exactly and are not 0; the other slots stay small so the tie is often the maximum
        f[:, :, 3] = f[:, :, 1]
        m = m * 0.3
        m[:, 1] = 0.0
        m[:, 1, 1:8, 2:9] = 1.0
        m[:, 3] = 0.0
        m[(slice(None), 3) + TIE_RECT] = 1.0
    go = torch.randn(B, num, ih, iw, generator=g)
    return f, m, go


def run_masked_max(ns, case, dtype, device):
    f, m, go = masked_max_inputs(case)
    f = _to(f, dtype, device, True)
    out = ns.masked_max(f, _to(m, dtype, device), case["ih"], case["iw"])
    (out * _to(go, dtype, device)).sum().backward()
    return {"out": out, "df": f.grad}


def _sm(cid, shape, dim, scale=1.0, lens=None, rowvalid=None, rows=True, backward=False):
    return dict(id=cid, shape=shape, dim=dim, scale=scale, lens=lens, rowvalid=rowvalid, rows=rows, backward=backward)


def _softmax_cases():
    out = []
    for dim in (1, 64, 65, 289, 1024, 1025):
        rows = dim <= SM_ROWS_MAX                       # 1025: the fallback to the strided kernel with inner == 1
        kind = "rows" if rows else "strided-fallback"
        for outer in (1, 5):                            # 5: not a multiple of the 4 rows of a workgroup
            out.append(_sm("%s-dim%d-outer%d-backward" % (kind, dim, outer), (outer, dim), 1, scale=4.0, rows=rows, backward=True))
        out.append(_sm("%s-dim%d-lens-0-1-dim-dim+3" % (kind, dim), (5, dim), 1, scale=4.0, lens=[0, 1, dim, dim + 3], rows=rows))
    out.append(_sm("rows-dim65-rowvalid", (5, 65), 1, scale=0.5, rowvalid=[1, 0, 1, 1, 0]))
    out.append(_sm("rows-dim289-lens-and-rowvalid", (6, 289), 1, scale=4.0, lens=[289, 17, 0, 300], rowvalid=[1, 1, 1, 0, 0, 1]))
    out.append(_sm("strided-inner11-rowvalid", (5, 7, 11), 1, scale=2.0, rowvalid=[1, 0, 1, 1, 0], rows=False))
    out.append(_sm("strided-inner11-lens-and-rowvalid", (5, 7, 11), 1, scale=2.0, lens=[7, 0, 3, 10], rowvalid=[1, 1, 0, 1, 1], rows=False))
    out.append(_sm("strided-inner11-backward", (3, 7, 11), 1, scale=2.0, rows=False, backward=True))
    out.append(_sm("strided-second-grid-stride-trip-inner525000", (1, 3, 525000), 1, scale=1.0, rows=False, backward=True))
    return out


SOFTMAX_CASES = _softmax_cases()
SOFTMAX_SPAN = 80.0          # scale * x spans +-80


def softmax_aux(case, device):
    lens = None if case["lens"] is None else torch.tensor(case["lens"], dtype=torch.int32, device=device)
    rowvalid = None if case["rowvalid"] is None else torch.tensor(case["rowvalid"], dtype=torch.uint8, device=device)
    return lens, rowvalid


def run_softmax(ns, case, dtype, device):
    g = _gen(case)
    x = (torch.rand(case["shape"], generator=g) * 2 - 1) * (SOFTMAX_SPAN / case["scale"])
    # a few entries close to each row's maximum, so that a row is more than a single 1 among zeros
    near = x.amax(dim=case["dim"], keepdim=True) - torch.rand(x.shape, generator=g) * 3.0 / case["scale"]
    x = torch.where(torch.rand(x.shape, generator=g) < 0.2, near, x)
    flat = x.view(-1)
    flat[0] = SOFTMAX_SPAN / case["scale"]
    flat[-1] = -SOFTMAX_SPAN / case["scale"]
    x = _to(x, dtype, device, case["backward"])
    gy = _to(torch.randn(case["shape"], generator=g), dtype, device)
    lens, rowvalid = softmax_aux(case, device)
    y = ns.softmax_strided(x, case["dim"], case["scale"], lens=lens, rowvalid=rowvalid)
    out = {"y": y}
    if case["backward"]:
        (y * gy).sum().backward()
        out["dx"] = x.grad
    return out


BMM_CASES = [dict(id="Bt%d-M%d-N%d-K%d-A-broadcast-batch-stride0" % s, shape=s) for s in ((2, 64, 65, 16), (1, 65, 64, 0), (3, 5, 3, 1))]


def run_bmm(ns, case, dtype, device):
    Bt, Mm, Nn, K = case["shape"]
    g = _gen(case)
    A0 = _to(torch.randn(1, Mm, K, generator=g), dtype, device, True)
    Bm = _to(torch.randn(Bt, K, Nn, generator=g), dtype, device, True)
    gc = _to(torch.randn(Bt, Mm, Nn, generator=g), dtype, device)
    C = ns.bmm(A0.expand(Bt, Mm, K), Bm)
    (C * gc).sum().backward()
    return {"C": C, "dA": A0.grad, "dB": Bm.grad}


BCE_CASES = [dict(id="n%d-target%d%s" % (n, t, "-" + sp if sp else ""), n=n, target=t, special=sp)
             for n, sp in ((1, "p-1-2^-24"), (1, "p-1e-30"), (20000, "")) for t in (0, 1)]
# n = 20000: bce_const_bwd_kernel's grid is capped at 64 workgroups, the elements from 16384 on are a second grid-stride
# trip.  p stays in [0.01, 0.99] there (|dp| within a factor 100 over the tensor), so that the maximum metric, which
# divides by max |dp|, sees a wrong element of that trip; the special probabilities are the n = 1 cases.


def run_bce(ns, case, dtype, device):
    n = case["n"]
    g = _gen(case)
    p = torch.rand(n, 1, generator=g) * 0.98 + 0.01
    if n == 1:
        p[0] = 1.0 - 2.0 ** -24 if case["special"] == "p-1-2^-24" else 1e-30
    p = _to(p, dtype, device, True)
    loss = ns.bce_const(p, case["target"])
    (loss * 1.7).backward()
    return {"loss": loss, "dp": p.grad}


# =====================================================================================================================
# pooling, resize, folds
# =====================================================================================================================
def _pool(cid, op, H, W, k=2, s=1, p=0, special=None, shape=None):
    return dict(id=cid, op=op, shape=shape or (2, 3, H, W), k=k, s=s, p=p, special=special)


POOL_CASES = [
    _pool("max-k2-s2-9x8", "max", 9, 8, 2, 2),
    _pool("max-k3-s1-6x7-nine-windows-per-pixel", "max", 6, 7, 3, 1),
    _pool("avg-k3-s2-p1-7x10-padded-rectangle", "avg", 7, 10, 3, 2, 1),
    _pool("avgpool2s1-6x6-backward", "avgs1", 6, 6),
    _pool("avgpool2s1-5x9-backward", "avgs1", 5, 9),
    _pool("max-k3-s2-nan-and-minus-inf-plateau", "max", 9, 11, 3, 2, special="nan"),
    _pool("max-k3-s2-second-grid-stride-trip-1500x1500", "max", 1500, 1500, 3, 2, shape=(1, 1, 1500, 1500)),
]


def run_pool(ns, case, dtype, device):
    g = _gen(case)
    x = torch.randn(case["shape"], generator=g)
    if case["special"] == "nan":
        x[0, 0, 2, 3] = float("nan")
        x[0, 1, 8, 10] = float("nan")
        x[1, 2, 4, 4] = float("nan")
        x[1, 0, 0:5, 0:5] = float("-inf")        # windows that hold nothing else: the first element wins
    x = _to(x, dtype, device, True)
    if case["op"] == "max":
        y = ns.max_pool2d(x, case["k"], case["s"])
    elif case["op"] == "avg":
        y = ns.avg_pool2d(x, case["k"], case["s"], case["p"])
    else:
        y = ns.avgpool2s1(x)
    gy = _to(torch.randn(y.shape, generator=g), dtype, device)
    y.backward(gy)
    return {"y": y, "dx": x.grad}


BILINEAR_CASES = [dict(id=cid, shape=shape, out=out) for cid, shape, out in (
    ("downscale-20x13-to-7x5", (2, 3, 20, 13), (7, 5)),
    ("to-1x1-scale0", (2, 3, 9, 9), (1, 1)),
    ("IH1-1x6-to-4x12", (2, 3, 1, 6), (4, 12)),
    ("identity-5x5", (2, 3, 5, 5), (5, 5)),
    ("second-grid-stride-trip-400-to-750", (1, 1, 400, 400), (750, 750)))]


def run_bilinear(ns, case, dtype, device):
    g = _gen(case)
    x = _to(torch.randn(case["shape"], generator=g), dtype, device, True)
    y = ns.bilinear_resize(x, case["out"][0], case["out"][1])
    y.backward(_to(torch.randn(y.shape, generator=g), dtype, device))
    return {"y": y, "dx": x.grad}


FOLD_CASES = [dict(id="%s-%dx%d" % (op, h, w), op=op, h=h, w=w)
              for op in ("sum2x2", "reflect_fold") for (h, w) in ((3, 3), (3, 8), (17, 5))]
FOLD_PLANES = 6


def run_fold(ns, case, dtype, device):
    g = _gen(case)
    h, w = case["h"], case["w"]
    if case["op"] == "sum2x2":
        return {"y": ns.sum2x2(_to(torch.randn(FOLD_PLANES, 2 * h, 2 * w, generator=g), dtype, device), h, w)}
    return {"y": ns.reflect_fold(_to(torch.randn(FOLD_PLANES, h + 2, w + 2, generator=g), dtype, device), h, w)}


# =====================================================================================================================
# flat-arena optimiser kernels (second trip of the grid-stride loop), LSTM
# =====================================================================================================================
STREAM_CASES = [dict(id="adam-n600001-second-grid-stride-trip", op="adam", n=600001),
                dict(id="ema-n600001-second-grid-stride-trip", op="ema", n=600001)]
# (lr 1e-2: the update stays far above the fp32 rounding of p, so that comparing it is well conditioned)
ADAM_HYPER = dict(lr=1e-2, beta1=0.5, beta2=0.999, eps=1e-8, step=3, grad_scale=0.5)


def run_stream(ns, case, dtype, device):
    g = _gen(case)
    n = case["n"]
    p0 = torch.randn(n, generator=g)
    if case["op"] == "ema":
        avg = _to(torch.randn(n, generator=g), dtype, device)
        ns.ema_update_(avg, _to(p0, dtype, device), 0.999)
        return {"avg": avg}
    p = _to(p0.clone(), dtype, device)
    grad = _to(torch.randn(n, generator=g), dtype, device)
    m = _to(torch.randn(n, generator=g) * 0.1, dtype, device)
    v = _to(torch.rand(n, generator=g) * 0.01, dtype, device)
    h = ADAM_HYPER
    ns.adam_step_(p, grad, m, v, h["lr"], h["beta1"], h["beta2"], h["eps"], h["step"], h["grad_scale"])
    # the update itself as well: p moves by ~lr, which a comparison of p alone (values of order 1) would not see
    return {"p": p, "m": m, "v": v, "update": p.detach().double().cpu() - p0.double()}


LSTM_DIMS = dict(I=7, H=20, L=5, ntoken=11)        # 4H = 80 gate rows on 128 threads: idle threads j >= G
# lens 0 (no step), lens > L and < 0 (clamped); caption 4 holds the ids -1 and 11 (clamped to 0 and 10)
LSTM_LENS = [5, 3, 1, 0, 4, 9, -2]
LSTM_CASES = [dict(id="max_len%d-%s" % (ml, what), max_len=ml)
              for ml, what in ((3, "shorter-than-captions"), (5, "equal-L"), (8, "Lout-above-L"))]


def lstm_inputs(case):
    d = LSTM_DIMS
    g = _gen(dict(id="lstm"))                       # the same weights and captions for every max_len
    I, H, L, nt = d["I"], d["H"], d["L"], d["ntoken"]
    table = torch.randn(nt, I, generator=g)
    captions = torch.randint(0, nt, (len(LSTM_LENS), L), generator=g)
    captions[4] = torch.tensor([-1, 11, 3, 11, 0])
    wt_ih = torch.randn(2, I, 4 * H, generator=g) * 0.3
    wt_hh = torch.randn(2, H, 4 * H, generator=g) * 0.3
    b_ih = torch.randn(2, 4 * H, generator=g) * 0.1
    b_hh = torch.randn(2, 4 * H, generator=g) * 0.1
    return table, captions, torch.tensor(LSTM_LENS, dtype=torch.int32), wt_ih, wt_hh, b_ih, b_hh


def run_lstm(ns, case, dtype, device):
    table, captions, lens, wt_ih, wt_hh, b_ih, b_hh = lstm_inputs(case)
    f = lambda t: _to(t, dtype, device)
    words, sent = ns.lstm_bidir_forward(f(table), captions.to(device), lens.to(device), f(wt_ih), f(wt_hh), f(b_ih), f(b_hh),
                                        case["max_len"])
    return {"words": words, "sent": sent}


# =====================================================================================================================
# ROIAlign: the ordered backward's per-image / per-slab decisions, and the scatter it falls back to
# =====================================================================================================================
# Boxes (`boxes`), in image coordinates (feature coordinates / scale), from the case's seeded generator:
#   ("inside", n)    n boxes with every sample inside the map: x1, y1 >= 0 and x2 + 1, y2 + 1 <= W - 0.5, H - 0.5
#   ("generic", n)   corners from -2 to 0.7 of the map, sizes up to 0.6 of it (as test_roi_align_bit_exact): partly outside
#   ("tiny", n)      boxes of at most half a feature pixel, inside the map: their 36 samples share one to four anchors
#   a list           explicit (x1, y1, x2, y2) rows
# and their concatenation.  `imgs`: "sorted" (equal runs per image, as the existing tests), "random", or the explicit
# list of image indices.  What the ordered backward decides for a case -- `table` (the workspace query is non-zero),
# `staged` (per slab: "all", "none", or "last" = only the short last slab), `start_lds`, `taps` (the touched pixels have
# at most ROI_SEQ taps: "seq", more: "many", or there are pixels of both regimes: "both") and `at_seq` (a pixel has
# EXACTLY ROI_SEQ taps: the last one the one-lane loop takes) -- is stated here and proven from the geometry in
# tests/test_kernel_edges_cpu.py.
def _roi(cid, B, C, H, W, AH, AW, scale, boxes, imgs="sorted", table=True, staged="all", start_lds=True, taps="both",
         at_seq=False, cols=5):
    return dict(id=cid, B=B, C=C, H=H, W=W, AH=AH, AW=AW, scale=scale, boxes=boxes, imgs=imgs, table=table, staged=staged,
                start_lds=start_lds, taps=taps, at_seq=at_seq, cols=cols)


def _corner_box(H, W):
    """samples at W - 3 .. W - 0.5 and H - 3 .. H - 0.5 (bin 0.5, exact in fp32): the last ones lie in the last row and
    column, where hstart = H - 2 is the clamp and h_ratio = 1.5"""
    return (W - 3.0, H - 3.0, W - 1.5, H - 1.5)


ROI_CASES = [
    _roi("unstaged-n_e-above-1024", 1, 2, 16, 16, 6, 6, 1.0, [("inside", 29)], staged="none", at_seq=True),
    _roi("staged-n_e-exactly-1024", 1, 2, 16, 16, 4, 4, 1.0, [("inside", 64)]),
    _roi("unstaged-n_e-1040", 1, 2, 16, 16, 4, 4, 1.0, [("inside", 65)], staged="none", at_seq=True),
    # more than one image on the global-memory form of the tap: a roi's position in its image's list (g.x) is not its index
    _roi("unstaged-rois-interleaved-1-0-1-0", 2, 2, 16, 16, 4, 4, 1.0, [("inside", 132)], imgs=[1, 0] * 66, staged="none",
         at_seq=True),
    _roi("unstaged-gradient-slab-C68-last-slab-nc4-staged", 1, 68, 8, 8, 6, 6, 1.0, [("generic", 15)], staged="last",
         at_seq=True),
    _roi("unstaged-many-taps", 1, 3, 16, 16, 6, 6, 1.0 / 16, [("tiny", 6), ("inside", 23)], staged="none", at_seq=True),
    _roi("start-in-lds-at-limit-hw4607", 1, 2, 17, 271, 6, 6, 1.0, [("generic", 5), [_corner_box(17, 271)]], at_seq=True),
    _roi("start-global-hw4608", 1, 2, 64, 72, 6, 6, 1.0, [("generic", 5), [_corner_box(64, 72)]], start_lds=False, at_seq=True),
    _roi("C70-cpb8-last-slab-nc6", 2, 70, 8, 8, 6, 6, 0.5, [("generic", 6)], taps="seq"),
    _roi("C63-cpb1", 2, 63, 8, 8, 6, 6, 0.5, [("generic", 6)], taps="seq"),
    _roi("C64", 2, 64, 8, 8, 6, 6, 0.5, [("generic", 6)], at_seq=True),
    _roi("images-0-and-1-own-no-roi", 3, 4, 8, 9, 6, 6, 1.0, [("generic", 5)], imgs=[2, 2, 2, 2, 2]),
    _roi("rois-interleaved-2-0-1-2-0", 3, 4, 8, 9, 3, 3, 1.0, [("generic", 5)], imgs=[2, 0, 1, 2, 0], taps="seq"),
    _roi("AH2xAW7", 2, 3, 12, 10, 2, 7, 1.0, [("generic", 4)], taps="seq"),
    _roi("AH7xAW2", 2, 3, 12, 10, 7, 2, 1.0, [("generic", 4)], taps="seq"),
    _roi("AH2xAW2", 2, 3, 12, 10, 2, 2, 1.0, [("generic", 4)], taps="seq"),
    _roi("S256-16x16", 2, 3, 12, 10, 16, 16, 1.0, [("generic", 4)], at_seq=True),
    # any valid sample has 0 <= h < 2: hstart = min(floor(h), 0) = 0, h_ratio up to 2
    _roi("H2xW2-smallest-map", 2, 3, 2, 2, 6, 6, 1.0,
         [[(0, 0, 0, 0), (0.2, 0.3, 0.5, 0.6), (-1, -1, 1.5, 1.5), (0.5, 0.5, 0.9, 0.8), (1, 1, 3, 3), (-3, 0, 0.5, 0.25)]],
         taps="many"),
    # integer boxes with bin 1: samples ON the pixels, from exactly 0 and up to exactly H - 1 = W - 1 = 7 (hstart = 6 by
    # the clamp, h_ratio = 1); a box from -2 (its two leading rows and columns of samples are invalid); x2 < x1 - 1 (the
    # width is clamped to 0: six samples per row on one column); the all-zero box slot (bin 0.2 from pixel 0)
    _roi("last-row-and-column-exact", 1, 2, 8, 8, 6, 6, 1.0,
         [[(2, 2, 6, 6), (0, 0, 4, 4), (0, 2, 4, 6), (-2, -2, 2, 2), (5, 1, 2, 5), (0, 0, 0, 0)]], at_seq=True),
    _roi("every-sample-outside", 2, 2, 8, 8, 6, 6, 1.0,
         [("generic", 2), [(9, 9, 12, 12), (-10, -10, -4, -4), (8, 2, 11, 5)]], imgs=[0, 0, 1, 1, 1], taps="seq"),
    _roi("scatter-fallback-513-rois", 2, 2, 8, 8, 2, 2, 1.0, [("generic", 513)], imgs="random", table=False),
    _roi("scatter-fallback-hw9216-lds", 1, 2, 96, 96, 6, 6, 1.0, [("generic", 4)], table=False),
    _roi("table-path-320-rois-second-compaction-pass", 2, 2, 8, 8, 2, 2, 1.0, [("generic", 320)], imgs="random",
         at_seq=True),
]
_ONE_BOX = [[(1, 1, 5, 5)]]
ROI_REJECTED = [
    _roi("17x16-S272-rejected", 1, 2, 8, 8, 17, 16, 1.0, _ONE_BOX),
    _roi("AH1-rejected", 1, 2, 8, 8, 1, 6, 1.0, _ONE_BOX),
    _roi("roi_cols4-rejected", 1, 2, 8, 8, 6, 6, 1.0, _ONE_BOX, cols=4),
    _roi("map-1x8-rejected", 1, 2, 1, 8, 6, 6, 1.0, [[(1, 0, 5, 0)]]),
    _roi("map-8x1-rejected", 1, 2, 8, 1, 6, 6, 1.0, [[(0, 1, 0, 5)]]),
]


def roi_inputs(case):
    """(features [B, C, H, W], rois [n, cols], top gradient [n, C, AH, AW]) of a case, float32 on the CPU"""
    g = _gen(case)
    B, C, H, W, scale = case["B"], case["C"], case["H"], case["W"], case["scale"]
    u = lambda n, lo, hi: lo + (hi - lo) * torch.rand(n, generator=g)
    parts = []
    for spec in case["boxes"]:
        if isinstance(spec, list):
            parts.append(torch.tensor(spec, dtype=torch.float32))
            continue
        kind, n = spec
        if kind == "generic":
            x1, y1 = u(n, -2.0, 0.7 * W), u(n, -2.0, 0.7 * H)
            x2, y2 = x1 + u(n, 0.0, 0.6 * W), y1 + u(n, 0.0, 0.6 * H)
        elif kind == "inside":
            x1, y1 = u(n, 0.0, (W - 1.5) / 2), u(n, 0.0, (H - 1.5) / 2)
            x2, y2 = x1 + u(n, 0.0, (W - 1.5) / 2), y1 + u(n, 0.0, (H - 1.5) / 2)
        else:
            x1, y1 = u(n, 1.0, W - 3.0), u(n, 1.0, H - 3.0)
            x2, y2 = x1 + u(n, 0.0, 0.5), y1 + u(n, 0.0, 0.5)
        parts.append(torch.stack([x1, y1, x2, y2], dim=1) / scale)
    boxes = torch.cat(parts)
    n = boxes.shape[0]
    if case["imgs"] == "sorted":
        img = torch.arange(n) * B // n
    elif case["imgs"] == "random":
        img = torch.randint(0, B, (n,), generator=g)
    else:
        img = torch.tensor(case["imgs"])
    assert img.numel() == n and int(img.min()) >= 0 and int(img.max()) < B
    rois = torch.cat([img.float().unsqueeze(1), boxes], dim=1)[:, :case["cols"]].contiguous()
    feat = torch.randn(B, C, H, W, generator=g)
    gtop = torch.randn(n, C, case["AH"], case["AW"], generator=g)
    return feat, rois, gtop


def run_roi(ns, case, dtype, device):
    feat, rois, gtop = roi_inputs(case)
    feat = _to(feat, dtype, device, True)
    y = ns.roi_align(feat, rois.to(device), case["AH"], case["AW"], case["scale"])
    y.backward(_to(gtop, dtype, device))
    return {"y": y, "dfeat": feat.grad}


def roi_facts(case):
    """What roi_tap_table_kernel builds for every image of a case, from the geometry: nlist (its rois), n_e (their valid
    samples), and of its touched pixels, by the length of their tap list (the four anchor ranges ranges() concatenates):
    n_seq with at most ROI_SEQ taps, n_many with more, n_at_seq with exactly ROI_SEQ."""
    _, rois, _ = roi_inputs(case)
    H, W = case["H"], case["W"]
    geo = roi_geometry_np(rois.numpy(), H, W, case["AH"], case["AW"], case["scale"])
    out = []
    for b in range(case["B"]):
        mine = geo["image"] == b
        ok = geo["valid"][mine]
        cnt = np.bincount(geo["off"][mine][ok], minlength=H * W)
        assert cnt.shape[0] == H * W
        taps = cnt.copy()
        for back in (1, W, W + 1):
            taps[back:] += cnt[:H * W - back]
        taps = taps[taps > 0]
        out.append(dict(nlist=int(mine.sum()), n_e=int(ok.sum()), n_seq=int((taps <= ROI_SEQ).sum()),
                        n_many=int((taps > ROI_SEQ).sum()), n_at_seq=int((taps == ROI_SEQ).sum())))
    return out


def roi_slabs(case):
    """nc of every channel slab of roi_align_bwd_gather_kernel's grid"""
    cpb = roi_cpb(case["C"])
    return [min(cpb, case["C"] - c0) for c0 in range(0, case["C"], cpb)]


def roi_slab_is_staged(case, facts, nc):
    return facts["n_e"] <= ROI_LDS_SMP and facts["nlist"] * nc * case["AH"] * case["AW"] <= ROI_LDS_G


def check_roi_backward_paths(ns, device, case, scatter, note=None):
    """For a case of the table path: the ordered backward gives the same bits twice, and the atomic scatter
    (`scatter(gtop, rois, case)` -> dfeat: objgan_roi_align_backward called directly on the same inputs) meets the fp64
    reference under the bounds the ordered kernel meets -- so that neither path is only ever compared with the other."""
    assert case["table"]
    first = run_roi(ns, case, torch.float32, device)["dfeat"]
    second = run_roi(ns, case, torch.float32, device)["dfeat"]
    assert torch.equal(first, second), "roi:%s the ordered backward is not bit-reproducible" % case["id"]
    _, rois, gtop = roi_inputs(case)
    got = {"dfeat": scatter(gtop.to(device), rois.to(device), case)}
    worst = compare("roi", case, got, note, only=("dfeat",), tag="scatter ")
    exact_properties("roi", case, got)
    return worst


# =====================================================================================================================
# layout-map stem: the four lift kernels alone (lift_taps), and behind the 1x1 convolution (lift_stem)
# =====================================================================================================================
# `longest`: the longest CSR row of ops._lift_axis_tables per axis (rows, columns) -- LIFT_MAXE entries are what an
# adjoint thread keeps; tests/test_kernel_edges_cpu.py recomputes them.
def _lift(cid, N, Mo, h, w, SH, SW, longest, bias=True):
    return dict(id=cid, N=N, Mo=Mo, h=h, w=w, SH=SH, SW=SW, longest=longest, bias=bias)


LIFT_TAPS_CASES = [
    _lift("rows-3-to-8-longest-8", 2, 3, 3, 5, 8, 12, (8, 7)),
    _lift("cols-4-to-11-longest-8", 1, 2, 6, 4, 13, 11, (6, 8)),
    _lift("h1-rows-1-to-4-longest-8", 2, 2, 1, 3, 4, 4, (8, 4)),
    _lift("identity-5-to-5", 2, 3, 5, 5, 5, 5, (4, 4)),
    _lift("downscale-9x12-to-4x5", 2, 2, 9, 12, 4, 5, (2, 2)),
    _lift("S2-smallest", 1, 1, 2, 2, 2, 2, (3, 3), bias=False),
    _lift("second-grid-stride-trip", 4, 1, 363, 363, 726, 726, (6, 6)),
]
LIFT_TAPS_REJECTED = [
    _lift("rows-3-to-9-longest-9-rejected", 1, 1, 3, 3, 9, 9, (9, 9)),
    _lift("rows-1-to-5-longest-10-rejected", 1, 1, 1, 3, 5, 4, (10, 4)),
    _lift("S1-rejected", 1, 1, 3, 3, 1, 1, (1, 1)),
]


def run_lift_taps(ns, case, dtype, device):
    g = _gen(case)
    N, Mo, h, w, SH, SW = (case[k] for k in ("N", "Mo", "h", "w", "SH", "SW"))
    z = _to(torch.randn(N, 9 * Mo, h, w, generator=g), dtype, device, True)
    bias = _to(torch.randn(Mo, generator=g), dtype, device, True) if case["bias"] else None
    gy = _to(torch.randn(N, Mo, SH, SW, generator=g), dtype, device)
    y = ns._LiftTapsFn.apply(z, bias, SH, SW)
    y.backward(gy)
    out = {"y": y, "dz": z.grad}
    if bias is not None:
        out["dbias"] = bias.grad
    return out


def _stem(cid, N, C, Mo, h, w, S, longest):
    return dict(id=cid, N=N, C=C, Mo=Mo, h=h, w=w, SH=S, SW=S, longest=longest)


LIFT_STEM_CASES = [
    _stem("3x3-to-8-C7-Mo5-longest-8", 2, 7, 5, 3, 3, 8, (8, 8)),
    _stem("5x9-to-12-C3-Mo2-rectangular-map", 2, 3, 2, 5, 9, 12, (7, 4)),
    _stem("1x3-to-4-h1", 2, 4, 3, 1, 3, 4, (8, 4)),
]


def run_lift_stem(ns, case, dtype, device):
    """data as test_lift_stem_conv_matches_the_reference_formulation: a layout map in [0, 1), a bank of unit response"""
    g = _gen(case)
    N, C, Mo, h, w, S = (case[k] for k in ("N", "C", "Mo", "h", "w", "SH"))
    seg = _to(torch.rand(N, C, h, w, generator=g), dtype, device, True)
    wt = _to(torch.randn(Mo, C, 3, 3, generator=g) / (C * 9) ** 0.5, dtype, device, True)
    b = _to(torch.randn(Mo, generator=g), dtype, device, True)
    gy = _to(torch.randn(N, Mo, S, S, generator=g), dtype, device)
    y = ns.lift_stem_conv(seg, wt, b, S)
    y.backward(gy)
    return {"y": y, "dseg": seg.grad, "dw": wt.grad, "db": b.grad}


# =====================================================================================================================
# tables, references, the comparison
# =====================================================================================================================
FAMILIES = {
    "norm": (NORM_CASES, run_norm), "norm_eval": (NORM_EVAL_CASES, run_norm_eval),
    "attn_general": (ATTN_GENERAL_CASES, run_attn_general), "attn_bu": (ATTN_BU_CASES, run_attn_bu),
    "masked_max": (MASKED_MAX_CASES, run_masked_max), "softmax": (SOFTMAX_CASES, run_softmax),
    "bmm": (BMM_CASES, run_bmm), "bce": (BCE_CASES, run_bce), "pool": (POOL_CASES, run_pool),
    "bilinear": (BILINEAR_CASES, run_bilinear), "fold": (FOLD_CASES, run_fold),
    "stream": (STREAM_CASES, run_stream), "lstm": (LSTM_CASES, run_lstm),
    "roi": (ROI_CASES, run_roi), "lift_taps": (LIFT_TAPS_CASES, run_lift_taps), "lift_stem": (LIFT_STEM_CASES, run_lift_stem),
}


def all_cases():
    return [(fam, case) for fam, (cases, _) in FAMILIES.items() for case in cases]


def case_ids(pairs):
    return ["%s:%s" % (fam, case["id"]) for fam, case in pairs]


_CACHE = {}


class _RoiOracle32(object):
    """the fp32 oracle of ROIAlign stays the C restatement (oracle/roi_align_oracle.c), as the existing tests and
    tests/cpu_ops_shim.roi_align use it: the forward is bit-equal to it"""

    @staticmethod
    def roi_align(*args):
        import cpu_ops_shim
        return cpu_ops_shim.roi_align(*args)


ORACLE32 = {"roi": _RoiOracle32()}


def _cached(kind, fam, case, dtype):
    key = (kind, fam, case["id"])
    if key not in _CACHE:
        ns = ORACLE32.get(fam, REF) if kind == "oracle32" else REF
        out = FAMILIES[fam][1](ns, case, dtype, torch.device("cpu"))
        _CACHE[key] = {k: v.detach().clone() for k, v in out.items()}
    return _CACHE[key]


def reference(fam, case):
    """float64 reference of a case, computed once and shared (never modified by the tests)"""
    return _cached("ref64", fam, case, torch.float64)


def oracle32(fam, case):
    return _cached("oracle32", fam, case, torch.float32)


def compare(fam, case, got, note=None, only=None, tag=""):
    """e_k <= M * max(e_o, 2^-23) and the family's rel_l2 bound, for every tensor of the case (or those of `only`; `tag`
    marks their lines in the log).  Every figure is noted before anything is asserted.  Returns the largest ratio
    e_k / max(e_o, 2^-23)."""
    ref, o32 = reference(fam, case), oracle32(fam, case)
    names = sorted(ref) if only is None else sorted(only)
    assert set(got) == set(names) <= set(ref), (sorted(got), sorted(ref))
    bad, worst = [], 0.0
    for name in names:
        e_k, e_o = max_err(got[name], ref[name]), max_err(o32[name], ref[name])
        ratio = e_k / max(e_o, EPS32)
        r2 = rel_l2(got[name], ref[name])
        worst = max(worst, ratio)
        if note is not None:
            note("edge %s%s:%s %s" % (tag, fam, case["id"], name), "e_k %.3g e_o %.3g ratio %.3g rel_l2 %.3g" % (e_k, e_o, ratio, r2))
        bound, mb = rl2_bound(fam, case, name), m_bound(fam, name)
        if not (e_k <= mb * max(e_o, EPS32)):
            bad.append("%s: e_k %.3g > %g * max(e_o %.3g, 2^-23)" % (name, e_k, mb, e_o))
        if not (r2 <= bound):
            bad.append("%s: rel_l2 %.3g > %g" % (name, r2, bound))
    if note is not None:
        note("edge-max %s%s:%s" % (tag, fam, case["id"]), "ratio %.3g" % worst)
    assert not bad, "%s:%s  %s" % (fam, case["id"], "; ".join(bad))
    return worst


def exact_properties(fam, case, got):
    """what must hold as an equality"""
    o32 = oracle32(fam, case)
    if fam == "softmax":
        y = got["y"].detach().cpu()
        d = case["dim"]
        n = y.shape[d]
        rows = y.reshape(int(math.prod(y.shape[:d])), n, -1)
        for o in range(rows.shape[0]):
            if case["lens"] is not None:
                span = max(0, min(n, case["lens"][o % len(case["lens"])]))
                assert float(rows[o, span:].abs().sum()) == 0.0, ("beyond lens", o)
            if case["rowvalid"] is not None and not case["rowvalid"][o]:
                assert float(rows[o].abs().sum()) == 0.0, ("rowvalid == 0", o)
    elif fam == "lstm":
        words = got["words"].detach().cpu()
        for b, n in enumerate(LSTM_LENS):
            n = max(0, min(LSTM_DIMS["L"], n))
            assert float(words[b, :, n:].abs().sum()) == 0.0, ("t >= len", b)
            if n == 0:
                assert float(got["sent"].detach().cpu()[b].abs().sum()) == 0.0
    elif fam == "pool" and case["op"] == "max":
        y, yo = got["y"].detach().cpu(), o32["y"]
        assert torch.equal(torch.isnan(y), torch.isnan(yo)), "NaN at different positions"
        assert torch.equal(torch.nan_to_num(y, nan=0.0), torch.nan_to_num(yo, nan=0.0)), "max_pool2d forward is not bit-equal"
    elif fam == "masked_max":
        assert torch.equal(got["out"].detach().cpu(), o32["out"]), "masked_max forward is not the fp32 product-then-max"
        if case["tie"]:
            # slot 3's mask lives on the tied rectangle only, under slot 1's: the first maximum (slot 1) takes it all
            assert float(got["df"].detach().cpu()[:, :, 3].abs().sum()) == 0.0, "the second of two tied slots received gradient"
    elif fam == "roi":
        if "y" in got:
            assert torch.equal(got["y"].detach().cpu(), o32["y"]), "roi_align forward is not bit-equal to the C oracle"
        # a pixel no valid sample touches (a whole image without rois or with every sample outside; a tap whose weight
        # is exactly 0) receives exactly nothing
        untouched = reference(fam, case)["dfeat"] == 0
        assert float(got["dfeat"].detach().cpu()[untouched].abs().sum()) == 0.0, "gradient where the reference has exactly 0"


def work_items(fam, case):
    """work items of the streaming launch a `second-grid-stride-trip` case is there for"""
    if fam == "norm":
        N, C, H, W = case["shape"]
        return N * (C // 2 if case["mode"] == "glu" else C) * H * W
    if fam == "softmax":
        return int(math.prod(case["shape"])) // case["shape"][case["dim"]]
    if fam == "pool":
        N, C, H, W = case["shape"]
        return N * C * ((H - case["k"]) // case["s"] + 1) * ((W - case["k"]) // case["s"] + 1)
    if fam == "bilinear":
        return case["shape"][0] * case["shape"][1] * case["out"][0] * case["out"][1]
    if fam == "lift_taps":
        return min(lift_launch_items(case))
    return case["n"]


def lift_launch_items(case):
    """work items of the four launches of the lift kernels: columns forward / rows backward, rows forward, columns backward"""
    N, h, w, SH, SW = (case[k] for k in ("N", "h", "w", "SH", "SW"))
    return (N * h * SW, N * SH * SW, N * h * SW, N * h * w)


def check_case(ns, device, fam, case, note=None):
    """The body of one edge-case test: run the operators of `ns` on `device` in float32, compare every output and
    gradient with the float64 reference, then the exact properties.  `ns` is objgan_hip.ops on the MI355X and the CPU
    definitions of the same API on a machine without one."""
    got = FAMILIES[fam][1](ns, case, torch.float32, device)
    if device.type == "cuda":
        torch.cuda.synchronize()
    failed = None
    try:
        worst = compare(fam, case, got, note)
    except AssertionError as e:             # (every figure is noted by now; the exact properties are still looked at)
        failed, worst = e, None
    exact_properties(fam, case, got)
    if failed is not None:
        raise failed
    return worst


def check_rejected(ns, device, case_pair, error):
    """The body of one rejection test: the operator raises `error` for a size the library has no kernel for."""
    fam, case = case_pair
    try:
        FAMILIES[fam][1](ns, case, torch.float32, device)
    except error:
        return
    finally:
        if device.type == "cuda":
            torch.cuda.synchronize()
    raise AssertionError("%s:%s was not rejected" % (fam, case["id"]))

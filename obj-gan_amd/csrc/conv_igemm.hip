// Implicit-GEMM convolution on the CDNA4 matrix cores, forward + data gradient: plan, launch and entry points.
//
// One kernel family serves every convolution of the Obj-GAN image_generation hot path
// (reference image_generation/model.py:30-81 conv1x1/conv3x3/upBlock/downBlock_G/
// HmapResBlock, :589-617 G_HMAP, :708-719 GET_IMAGE_G, :986-1048 D encoders and heads,
// :1184-1312 object discriminators), which the reference hands to cuDNN:
//
//   y[n, m, oh, ow] = sum_{c, t}  Wp[m][c*T + t] * x[n, c, a*s + dh[t], b*s + dw[t]]
//   (oh, ow) = (a*osh + ooh, b*osw + oow),   (a, b) in a PH x PW grid per image
//
// * forward conv      : m = cout, c = cin, taps t = (kh, kw), dh = kh - pad
// * dgrad, stride 1   : m = cin,  c = cout, flipped taps (host passes dh/dw + tap map)
// * dgrad, stride 2   : one launch per output parity phase, 2x2 (k=4) or <=2x2 (k=3)
//                       taps each, osh = osw = 2 -- no zero-multiplies
// * nearest x2 upsample (upBlock) and ReflectionPad2d are folded into the gather
//   (the up-sampled / padded tensor never exists in HBM)
// * epilogue: + bias, LeakyReLU(0.2) / tanh / sigmoid
//
// GEMM view: M = output channels, N = pixels (n, a, b), K = T*Cp (TAP-MAJOR: k = t*Cp + c with
// Cp = C rounded up to the K step of 16, so that one K step of the main loop touches ONE tap:
// the tap geometry -- bounds / reflect / upsample / offset -- is evaluated once per tap and lane).
//
// objgan_conv_igemm asks og_bank_layout (conv_igemm_pack.hip) which family serves a call:
//   class 2   M <= 32 outputs on large maps: direct fp32 VALU convolution        run_thin, conv_igemm_thin.hip
//   class 0   tensors beyond the 2 GiB reach of a buffer descriptor              run_igemm, conv_igemm_v1.hip
//   else      conv_igemm3_kernel<TM, ..> (conv_igemm3.h): (32*TM) x 128 tile, pixel fragments straight from the gather
//             registers, filter rows via LDS; launched here (launch_igemm2), its record instances in conv_igemm_rec.hip
// Kernels in this file: bias_act_kernel, reflect_ring_fold_kernel (splitk_combine_kernel: conv_igemm_pack.hip).
// Host: igemm2_plan (pure: block rows, waves, splits), run_igemm2, launch_igemm2.  Entry points: objgan_conv_igemm,
// objgan_conv_igemm_ws_floats, objgan_conv_igemm_plan, objgan_conv_dgrad_s2_phases, objgan_conv_dgrad_s2_phases_ws_floats,
// objgan_conv_dgrad_s2_phases_plan, objgan_reflect_ring_fold.  The weight gradient lives in conv_igemm_wgrad.hip.
#include "conv_igemm_host.h"

// y[n, m, i] = act(y[n, m, i] + bias[m]) -- epilogue of the split-K path
__global__ __launch_bounds__(256) void bias_act_kernel(float* __restrict__ y, const float* __restrict__ bias,
                                                       long total, int M, int HW, int act) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long)gridDim.x * blockDim.x) {
        float v = y[e];
        if (bias) v += bias[(e / HW) % M];
        y[e] = og_act(v, act);
    }
}

// Adds the ring of a padded-grid data gradient (IgemmArgs::ring) onto the unpadded gradient: padded index p mirrors to
// 1 (p = 0) / H - 2 (p = H + 1), interior p to p - 1.  Gather form: one thread per DESTINATION element of rows 1 / H-2
// and columns 1 / W-2 adds its (up to four) ring entries in a fixed order -- top row, bottom row, left column, right
// column -- to y: single writer, no atomics, bit-reproducible.
__global__ __launch_bounds__(256) void reflect_ring_fold_kernel(const float* __restrict__ ring, float* __restrict__ y,
                                                                long planes, int H, int W) {
    const int PH = H + 2, PW = W + 2, R = 2 * PW + 2 * PH;
    const int D = 2 * W + 2 * H;                      // candidate destinations per plane (segments below)
    const long total = planes * D;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long p = e / D;
        const int d = (int)(e - p * D);
        int oh, ow;
        if (d < W) { oh = 1; ow = d; }
        else if (d < 2 * W) { oh = H - 2; ow = d - W; if (oh == 1) continue; }
        else if (d < 2 * W + H) { oh = d - 2 * W; ow = 1; if (oh == 1 || oh == H - 2) continue; }
        else { oh = d - 2 * W - H; ow = W - 2; if (oh == 1 || oh == H - 2 || ow == 1) continue; }
        const float* rg = ring + p * R;
        const float* top = rg, *bot = rg + PW, *lef = rg + 2 * PW, *rig = rg + 2 * PW + PH;
        float v = 0.f;
        if (oh == 1) {                                   // padded row 0: columns pb with mirror(pb) == ow
            v += top[ow + 1];
            if (ow == 1) v += top[0];
            if (ow == W - 2) v += top[PW - 1];
        }
        if (oh == H - 2) {                               // padded row PH - 1
            v += bot[ow + 1];
            if (ow == 1) v += bot[0];
            if (ow == W - 2) v += bot[PW - 1];
        }
        if (ow == 1) v += lef[oh + 1];                   // padded column 0 (corners belong to the row arrays)
        if (ow == W - 2) v += rig[oh + 1];               // padded column PW - 1
        y[p * (long)H * W + (long)oh * W + ow] += v;
    }
}

template <int TM, bool ADIRECT, int MATH, int NW = 4>
static inline void ig3(const IgemmArgs& a, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((conv_igemm3_kernel<TM, ADIRECT, MATH, NW>), grid, dim3(64 * NW), 0, s, a);
}

static int launch_igemm2(const IgemmArgs& a, int TM, dim3 grid, hipStream_t s, int nw = 4, int ng = 1) {
    if (a.math == 5) {
        if (og_trace())
            fprintf(stderr, "OGTRACE igemm-rec TM=%d NW=%d NG=%d M=%d rows=%d C=%d T=%d Npix=%d grid=%u,%u H=%d W=%d stride=%d\n", TM, nw, ng,
                    a.M, a.m_end - a.m_begin, a.C, a.T, a.N * a.PH * a.PW, grid.x, grid.y, a.H, a.W, a.stride);
        return og_launch_igemm3_rec(a, TM, nw, ng, grid, s);
    }
    if (og_trace())
        fprintf(stderr, "OGTRACE igemm TM=%d NW=%d M=%d rows=%d C=%d T=%d Npix=%d grid=%u,%u,%u H=%d W=%d stride=%d\n", TM, nw, a.M,
                a.m_end - a.m_begin, a.C, a.T, a.N * a.PH * a.PW, grid.x, grid.y, grid.z, a.H, a.W, a.stride);
    og_with_tm<1, 7>(TM, [&](auto tmc) {        // (out-of-range heights run the 7-group instance)
        constexpr int T = decltype(tmc)::value;
        // TM = 1, M <= 32: the LDS-free ADIRECT instance reads the filter rows directly, which only pays while the
        // bank is tiny (4 waves whatever nw says; the bf16 channel-blocked and 8-wave bf16x3 forms have none)
        const bool direct = T == 1 && a.M <= 32;
        if (a.math == 1 && a.nhwc) {           // bf16, channel-blocked pixel operand
            if (nw == 8) ig3<T, false, 3, 8>(a, grid, s); else ig3<T, false, 3, 4>(a, grid, s);
        } else if (a.math == 4) {              // fp16x2
            if (direct) ig3<1, true, 4>(a, grid, s);
            else if (nw == 8) ig3<T, false, 4, 8>(a, grid, s);
            else ig3<T, false, 4, 4>(a, grid, s);
        } else if (a.math == 2 && nw == 8) {   // bf16x3, 8-wave workgroups: 32 * TM rows x 256 pixels
            ig3<T, false, 2, 8>(a, grid, s);
        } else if (a.math == 1) {
            if (direct) ig3<1, true, 1>(a, grid, s); else ig3<T, false, 1>(a, grid, s);
        } else if (a.math == 2) {
            if (direct) ig3<1, true, 2>(a, grid, s); else ig3<T, false, 2>(a, grid, s);
        } else {
            if (direct) ig3<1, true, 0>(a, grid, s); else ig3<T, false, 0>(a, grid, s);
        }
    });
    return og_launch_status();
}

struct Igemm2Plan { int nw, ng, TM, full_rows, rest, tiles_n, splits, ksplit_steps, full_cover; };

// Launch plan of run_igemm2 (also behind objgan_conv_igemm_ws_floats: the caller sizes the split-K workspace from it).
// Rows are covered by block rows of TM 32-row groups (og_row_plan): the full-height block rows in one launch, plus one
// launch with a smaller TM for the remaining groups.
static Igemm2Plan igemm2_plan(const IgemmArgs& a) {
    Igemm2Plan p;
    const int groups = og_cdiv(a.M, 32);
    const int Npix = a.N * a.PH * a.PW;
    const int nph = a.nphase > 1 ? a.nphase : 1;
    // bf16x3 runs against the L2 -> L1 fill rate (6 TB/s of fills at 190 TFLOP/s, profiles/r03_x3_pmc_objd_l3.txt),
    // and 2/3 of a workgroup's fills are its row tile: 8-wave workgroups (256 pixels per row tile) wherever the
    // grid still covers the chip twice
    // (tall tiles only: at TM <= 3 a 4-wave workgroup leaves room for three per CU and wins -- r03 A/B, 96-row
    // layers 179 vs 158 TFLOP/s; with 8 waves the block rows are as tall as the row count allows)
    p.nw = 4;
    p.ng = 1;
    const int tm_tall = og_cdiv(groups, og_cdiv(groups, 7));
    const int tm_cap = a.math == 5 ? og_rec_tmmax() : 7;
    if ((a.math == 2 || a.math >= 4 || (a.math == 1 && a.nhwc)) &&
        tm_tall >= (a.math == 5 ? og_rec_nw8_tm() : (a.math == 4 ? og_h2_nw8_tm() : 4)) &&
        og_nw8_min() > 0 &&
        (long)og_cdiv(groups, 7) * og_cdiv(Npix, 256) * nph >= og_nw8_min()) p.nw = 8;
    p.tiles_n = og_cdiv(Npix, 32 * p.nw);
    // (Carrying the 2 / 4 rows that 194 / 388 channels have beyond a multiple of 32 on the VALU next to the
    // MFMA stream -- as the weight-gradient kernels do -- was measured here in round 2 and bought nothing:
    // 106.0 vs 107.8 TFLOP/s on res1_128; interleaving the FMAs with the MFMAs cost 20 %.)
    og_row_plan(groups, p.tiles_n * nph, p.nw == 8, &p.TM, &p.full_rows, &p.rest, a.math >= 4 ? og_h2_pen_pct() : 100, tm_cap);
    if (a.math == 5 && (p.nw == 4 || og_rec_ng2_nw8()) && og_rec_ng2_maxtm() > 0) {
        // record form, short block rows: two 32-pixel groups per wave (every LDS row fragment feeds two MFMAs per
        // product) while the grid still fills the chip
        const int tn2 = og_cdiv(Npix, 64 * p.nw);
        int TM2, full2, rest2;
        const int cap2 = og_rec_ng2_maxtm() < 4 ? og_rec_ng2_maxtm() : 4;
        og_row_plan(groups, tn2 * nph, p.nw == 8, &TM2, &full2, &rest2, og_h2_pen_pct(), p.nw == 8 ? cap2 : tm_cap);
        if (TM2 <= og_rec_ng2_maxtm() && TM2 <= 4 && (long)(full2 + (rest2 ? 1 : 0)) * tn2 * nph >= og_rec_ng2_min()) {
            p.ng = 2; p.tiles_n = tn2; p.TM = TM2; p.full_rows = full2; p.rest = rest2;
        }
    }
    const int tiles = (p.full_rows + (p.rest ? 1 : 0)) * p.tiles_n;
    const int nk = a.math == 1 ? a.Krow / 32 : a.Kpad / 16;      // loop iterations of the kernel
    p.full_cover = ((a.osh == 1 && a.osw == 1 && a.PH == a.OHf && a.PW == a.OWf) || a.ring != nullptr) ? 1 : 0;
    int splits = 1;
    // (partial-coverage launches -- strided output phases into a pre-zeroed y -- are not split: their partials would
    // have to be accumulated with atomics; they are the two 3x3 stride-2 layers of G_HMAP, 0.1 ms per step)
    if (tiles < 128 && nk >= 16 && p.full_cover && nph == 1) {
        splits = og_cdiv(512, tiles);
        if (splits > nk / 4) splits = nk / 4;
    } else if (og_split_target() > 0 && p.TM == 1 && p.rest == 0 && tiles < og_split_target() && nk >= 16 &&
               p.full_cover && nph == 1) {
        splits = og_cdiv(og_split_target(), tiles);
        if (splits > nk / 8) splits = nk / 8;
        if (splits < 1) splits = 1;
    }
    p.ksplit_steps = 0;
    if (splits > 1) {
        p.ksplit_steps = og_cdiv(nk, splits);
        splits = og_cdiv(nk, p.ksplit_steps);
    }
    p.splits = splits;
    return p;
}

// bf16 mode: floats of workspace the channel-blocked bf16 copy of the source takes (0: not this mode / too large for
// the 32-bit buffer range)
static long igemm2_nhwc_floats(int math, int N, int H, int W, int Cp) {
    if (math != 1 || (double)N * H * W * Cp * 2.0 >= 4.0e9) return 0;
    return og_nhwc_bf16_floats(N, H, W, Cp);
}
// floats of workspace run_igemm2 wants for this plan: the bf16 copy of the source, then the split-K slots (none: one
// split, or a partial-coverage launch that accumulates into the pre-zeroed output)
static long igemm2_ws_floats(const IgemmArgs& a, const Igemm2Plan& p) {
    const long nh = a.nhwc == 1 ? igemm2_nhwc_floats(a.math, a.N, a.H, a.W, a.Cp) : 0;
    if (p.splits <= 1 || !p.full_cover) return nh;
    const long seg = (long)a.N * a.M * a.OHf * a.OWf + (a.ring ? (long)a.N * a.M * (2 * a.PW + 2 * a.PH) : 0);
    return nh + seg * p.splits;
}

static int run_igemm2(IgemmArgs a, hipStream_t s, float* ws, long ws_floats, float* ymax = nullptr) {
    a.ymax = nullptr;
    if (a.nhwc == 1 && !ws) a.nhwc = 0;         // no workspace: fp32 NCHW gathers (conv_igemm3_kernel<.., 1, ..>)
    const Igemm2Plan p = igemm2_plan(a);
    if (a.nhwc == 1) {                          // bf16 channel-blocked copy of the source: first part of the workspace
        const long nh = igemm2_nhwc_floats(a.math, a.N, a.H, a.W, a.Cp);
        if (ws_floats < igemm2_ws_floats(a, p)) return OG_BAD_ARGS;
        og_launch_nhwc_bf16(a.x, ws, a.N, a.C, a.H * a.W, a.Cp, s);
        a.x = ws;
        ws += nh; ws_floats -= nh;
    }
    const int Npix = a.N * a.PH * a.PW;
    const int nph = a.nphase > 1 ? a.nphase : 1;
    const int TM = p.TM, full_rows = p.full_rows, rest = p.rest, tiles_n = p.tiles_n, nw = p.nw, ng = p.ng;
    int splits = p.splits;
    const bool full_cover = p.full_cover != 0;
    const float* bias = a.bias;
    const int act = a.act;
    const bool act_later = (act == OG_ACT_TANH || act == OG_ACT_SIGMOID);
    const long y_elems = (long)a.N * a.M * a.OHf * a.OWf;
    const long ring_elems = a.ring ? (long)a.N * a.M * (2 * a.PW + 2 * a.PH) : 0;
    a.ws = nullptr; a.ws_stride = 0;
    if (splits > 1) {
        a.ksplit_steps = p.ksplit_steps;
        a.bias = nullptr; a.act = OG_ACT_NONE;
        const long need = igemm2_ws_floats(a, p) - (a.nhwc == 1 ? igemm2_nhwc_floats(a.math, a.N, a.H, a.W, a.Cp) : 0);
        // two-level reduction through the caller's workspace (need > 0: the plan splits only launches that cover their output)
        if (need <= 0 || !ws || ws_floats < need) return OG_BAD_ARGS;
        a.ws = ws; a.ws_stride = y_elems + ring_elems;
    } else {
        a.ksplit_steps = 0;
        if (act_later) { a.bias = nullptr; a.act = OG_ACT_NONE; }
    }
    // |y| maxima in the epilogue: unsplit launches that write their final values and cover y (else a pass over y below)
    const bool emit = ymax && splits <= 1 && !act_later && full_cover && !a.ring;
    if (emit) a.ymax = ymax;
    // one launch per block-row height: the full-height block rows, then the remaining groups
    const auto launch_rows = [&](int tm, int brows) {
        // the category follows the launch: 8-wave instances have no LDS-free form
        const OgFamily fam = (nw != 8 && tm == 1 && a.M <= 32) ? OG_FAM_IGEMM3_DIRECT : OG_FAM_IGEMM3;
        ProfRec* pr = prof_begin(og_prof_cat(fam, tm, nw, a.math, ng), 2.0 * (a.m_end - a.m_begin) * (double)a.K * (double)Npix * nph, s);
        prof_meta(pr, 0, tm, a.m_end - a.m_begin, a.C, a.T, a.N, a.PH * nph, a.PW, a.stride * (a.osh > 1 ? -1 : 1), splits);
        const int rc = launch_igemm2(a, tm, dim3(brows * tiles_n * nph, splits, 1), s, nw, ng);
        prof_end(pr, s);
        return rc;
    };
    if (full_rows > 0) {
        a.m_begin = 0; a.m_end = min(a.M, full_rows * TM * 32);
        const int rc = launch_rows(TM, full_rows);
        if (rc != OG_OK) return rc;
    }
    if (rest > 0) {
        a.m_begin = full_rows * TM * 32; a.m_end = a.M;
        const int rc = launch_rows(rest, 1);
        if (rc != OG_OK) return rc;
    }
    if (a.ws) {         // second level: sum the splits in order, + bias, activation
        // (the maxima of y ride in the combine unless a later pass changes y: tanh / sigmoid heads, ring mode)
        const bool ymax_in_combine = ymax && !act_later && ring_elems == 0;
        og_launch_splitk_combine(a.ws, splits, a.ws_stride, 0L, a.y, y_elems, bias, a.M, a.OHf * a.OWf, act,
                                 ymax_in_combine ? ymax : nullptr, s);
        if (ring_elems > 0)
            og_launch_splitk_combine(a.ws, splits, a.ws_stride, y_elems, a.ring, ring_elems, nullptr, 1, 1, OG_ACT_NONE, nullptr, s);
        if (ymax && !ymax_in_combine) og_absmax_launch(a.y, y_elems, ymax, s);
        return og_launch_status();
    }
    if ((splits > 1 || act_later) && (bias || act != OG_ACT_NONE) && full_cover) {
        hipLaunchKernelGGL(bias_act_kernel, dim3(og_stream_grid(y_elems, 256)), dim3(256), 0, s, a.y, bias,
                           y_elems, a.M, a.OHf * a.OWf, act);
    }
    if (ymax && !emit) og_absmax_launch(a.y, y_elems, ymax, s);
    return og_launch_status();
}

// Geometry and arithmetic fields of the four-phase launch (everything igemm2_plan reads; the pointers and taps are the
// caller's): shared by objgan_conv_dgrad_s2_phases and its plan query.
static void og_phases_args(IgemmArgs& a, int N, int Cout, int OH, int OW, int Cin, int Tg, int PH, int PW, int math) {
    const int M = Cin, C = Cout;
    const int Cp = (C + 15) / 16 * 16;
    const int Kpad = Tg * Cp;
    a.x = nullptr; a.wt = nullptr; a.bias = nullptr; a.y = nullptr;
    a.N = N; a.C = C; a.H = OH; a.W = OW; a.LH = OH; a.LW = OW;
    a.M = M; a.Mpad = (M + 127) / 128 * 128; a.K = C * Tg; a.Kpad = Kpad; a.T = Tg; a.Cp = Cp;
    a.kgroup = og_kgroup_phases(C);
    a.math = math; a.Krow = og_krow(Kpad, math); a.xmax = nullptr; a.wmax = nullptr;
    a.nhwc = igemm2_nhwc_floats(math, N, OH, OW, Cp) > 0 ? 1 : 0;
    a.m_begin = 0; a.m_end = M;
    a.PH = PH; a.PW = PW; a.OHf = 2 * PH; a.OWf = 2 * PW;
    a.osh = 2; a.osw = 2; a.ooh = 0; a.oow = 0;
    a.stride = 1; a.pad_mode = 0; a.upsample = 0; a.act = OG_ACT_NONE;
    a.ksplit_steps = 0;
    a.ring = nullptr;
    a.ws = nullptr; a.ws_stride = 0;
    a.nphase = 4;
#ifdef OG_DEV
    a.ablate = og_ablate();
#endif
}

extern "C" {

// General entry: see the formula at the top of this file.
//   w        PyTorch-layout conv weight [Cout][Cin][Torig]
//   wt       scratch of objgan_conv_packed_floats(M, C*Tg) floats (overwritten)
//   transpose 0: M = Cout, C = Cin ; 1: M = Cin, C = Cout (data gradient)
//   src_tap[t] index of GEMM tap t in the Torig taps of w (or -1 for a zero tap)
// Fills the PackArgs / IgemmArgs of objgan_conv_igemm (shared with objgan_conv_igemm_ws_floats); returns OG_OK,
// OG_BAD_ARGS or 2 for "nothing to do".
static int og_igemm_setup(PackArgs& p, IgemmArgs& a, int& MT, const float* x, const float* w, const float* bias, float* y,
                          float* wt, int N, int C, int H, int W, int upsample, int pad_mode, int Cout, int Cin, int Torig,
                          int transpose, int Tg, const int* dh, const int* dw, const int* src_tap, int PH, int PW,
                          int stride, int OHf, int OWf, int osh, int osw, int ooh, int oow, int act, int math, float* ring,
                          const float* xmax = nullptr) {
    if (Tg < 1 || Tg > OG_MAX_TAPS) return OG_BAD_ARGS;
    if (ring && !(osh == 1 && osw == 1 && ooh == 0 && oow == 0 && PH == OHf + 2 && PW == OWf + 2 && !bias && !act))
        return OG_BAD_ARGS;
    if (math < 0 || math > 5) return OG_BAD_ARGS;
    // math 3 (round 6): the arithmetic of math 1 (bf16-rounded operands) with the pixel operand handed over AS its bf16
    // channel-blocked copy (objgan_nhwc_bf16) -- the copy of a tensor is made once and serves every convolution that reads it
    // (the forward call AND the weight gradient of the layer, every branch of an Inception block) instead of once per call
    const bool copy_in = math == 3;
    if (copy_in) math = 1;
    if (Torig < 1 || Torig > 127) return OG_BAD_ARGS;
    const int M = transpose ? Cin : Cout;
    const int Ck = transpose ? Cout : Cin;
    if (Ck != C) return OG_BAD_ARGS;
    if (N <= 0 || PH <= 0 || PW <= 0 || M <= 0) return 2;
    MT = 32;
    og_fill_pack(p, w, wt, N, C, H, W, Cout, Cin, Torig, transpose, Tg, src_tap, PH, PW, act, math, &MT);
    if (math == 5 && p.m_major != 5) return OG_BAD_ARGS;       // records: the MFMA implicit-GEMM kernel only (ask objgan_conv_bank_layout)
    const int kmath = p.m_major == 3 ? 1 : (p.m_major == 4 ? 2 : (p.m_major == 5 ? (math == 5 ? 5 : 4) : 0));   // arithmetic of the kernel that runs
    a.x = x; a.wt = wt; a.bias = bias; a.y = y;
    a.N = N; a.C = C; a.H = H; a.W = W;
    a.LH = upsample ? 2 * H : H; a.LW = upsample ? 2 * W : W;
    a.M = M; a.Mpad = p.Mpad; a.K = C * Tg; a.Kpad = Tg * p.Cp; a.T = Tg; a.Cp = p.Cp; a.kgroup = p.kgroup;
    a.math = kmath;
    a.xmax = xmax; a.wmax = p.wmax;
    if (kmath >= 4 && x && !xmax) return OG_BAD_ARGS;      // fp16x2 needs the maxima of its pixel operand (x == NULL: size query)
    a.nhwc = igemm2_nhwc_floats(kmath, N, H, W, p.Cp) > 0 ? 1 : 0;
    if (copy_in) {
        if (p.m_major != 3 || !a.nhwc) return OG_BAD_ARGS;    // the bf16 MFMA kernel only (ask objgan_conv_bank_layout: class 3)
        a.nhwc = 2;                                            // x IS the copy: nothing to make, nothing in the workspace
    }
    a.Krow = og_krow(a.Kpad, kmath);
    a.m_begin = 0; a.m_end = M;
    a.PH = PH; a.PW = PW; a.OHf = OHf; a.OWf = OWf;
    a.osh = osh; a.osw = osw; a.ooh = ooh; a.oow = oow;
    a.stride = stride; a.pad_mode = pad_mode; a.upsample = upsample; a.act = act;
    a.ksplit_steps = 0;
    a.nphase = 0;
    a.ring = ring;
    a.ws = nullptr; a.ws_stride = 0;
#ifdef OG_DEV
    a.ablate = og_ablate();
#endif
    for (int t = 0; t < OG_MAX_TAPS; ++t) {
        const int h = t < Tg ? dh[t] : 0, w_ = t < Tg ? dw[t] : 0;
        a.tap[t] = (int)(((unsigned)w_ << 16) | ((unsigned)h & 0xffffu));
    }
    if (!(osh == 1 && osw == 1 && PH == OHf && PW == OWf) && (bias || act)) return OG_BAD_ARGS;
    if (ring && p.m_major != 1 && p.m_major != 3 && p.m_major != 4 && p.m_major != 5) return OG_BAD_ARGS;     // ring mode: conv_igemm3_kernel only (ask objgan_conv_bank_layout)
    return OG_OK;
}

// Floats of split-K workspace objgan_conv_igemm needs for these arguments (0: none).  Small-grid / long-K launches
// are split along K: every split stores its partial output tile into its own workspace slot and a second kernel sums
// the slots in split order (+ bias, activation) -- bit-reproducible, no zero-fill of y, no atomics.  Host-only.
long objgan_conv_igemm_ws_floats(int N, int C, int H, int W, int upsample, int pad_mode,
                                 int Cout, int Cin, int Torig, int transpose, int Tg,
                                 int PH, int PW, int stride, int OHf, int OWf, int osh, int osw,
                                 int act, int y_prezeroed, int math, int ring) {
    PackArgs p;
    IgemmArgs a;
    int MT = 32;
    int zeros[OG_MAX_TAPS] = {0};
    float dummy = 0.f;
    memset(&p, 0, sizeof(p));
    const int rc = og_igemm_setup(p, a, MT, nullptr, nullptr, nullptr, nullptr, nullptr, N, C, H, W, upsample, pad_mode, Cout, Cin,
                                  Torig, transpose, Tg, zeros, zeros, zeros, PH, PW, stride, OHf, OWf, osh, osw, 0, 0, act,
                                  math, ring ? &dummy : nullptr);
    if (rc != OG_OK || p.m_major == 0 || p.m_major == 2) return 0;
    return igemm2_ws_floats(a, igemm2_plan(a));
}

// out[0..10] <- {bank layout class, kernel math, nw, ng, TM, full_rows, rest, tiles_n, splits, full_cover, direct} of a
// launch plan (direct: the block rows of height 1 run the LDS-free instance); a class without a plan (0 first
// generation, 2 thin VALU) leaves the fields behind the class at 0.
static void og_plan_fields(int cls, const IgemmArgs& a, int* out) {
    for (int i = 0; i < 11; ++i) out[i] = 0;
    out[0] = cls;
    if (cls == 0 || cls == 2) return;
    const Igemm2Plan q = igemm2_plan(a);
    const int f[10] = {a.math, q.nw, q.ng, q.TM, q.full_rows, q.rest, q.tiles_n, q.splits, q.full_cover,
                       (q.nw != 8 && a.M <= 32 && (q.TM == 1 || q.rest == 1)) ? 1 : 0};
    for (int i = 0; i < 10; ++i) out[1 + i] = f[i];
}

// The launch plan objgan_conv_igemm follows for these arguments (those of objgan_conv_igemm_ws_floats), for tests and
// tools: which block rows, waves, pixel groups and splits.  Host-only, launches nothing.  OG_BAD_ARGS where the call
// itself would refuse the arguments.
int objgan_conv_igemm_plan(int N, int C, int H, int W, int upsample, int pad_mode,
                           int Cout, int Cin, int Torig, int transpose, int Tg,
                           int PH, int PW, int stride, int OHf, int OWf, int osh, int osw,
                           int act, int y_prezeroed, int math, int ring, int* out) {
    PackArgs p;
    IgemmArgs a;
    int MT = 32;
    int zeros[OG_MAX_TAPS] = {0};
    float dummy = 0.f;
    if (!out) return OG_BAD_ARGS;
    memset(&p, 0, sizeof(p));
    const int rc = og_igemm_setup(p, a, MT, nullptr, nullptr, nullptr, nullptr, nullptr, N, C, H, W, upsample, pad_mode, Cout, Cin,
                                  Torig, transpose, Tg, zeros, zeros, zeros, PH, PW, stride, OHf, OWf, osh, osw, 0, 0, act,
                                  math, ring ? &dummy : nullptr);
    if (rc != OG_OK) return OG_BAD_ARGS;
    og_plan_fields(p.m_major, a, out);
    return OG_OK;
}

int objgan_conv_igemm(const float* x, const float* w, const float* bias, float* y, float* wt,
                      int N, int C, int H, int W, int upsample, int pad_mode,
                      int Cout, int Cin, int Torig, int transpose,
                      int Tg, const int* dh, const int* dw, const int* src_tap,
                      int PH, int PW, int stride,
                      int OHf, int OWf, int osh, int osw, int ooh, int oow,
                      int act, int y_prezeroed, int wt_packed, int math, float* ring, const float* xmax, float* ymax,
                      float* ws, long ws_floats, void* stream) {
    OG_ENTRY();
    PackArgs p;
    IgemmArgs a;
    int MT = 32;
    const int rc0 = og_igemm_setup(p, a, MT, x, w, bias, y, wt, N, C, H, W, upsample, pad_mode, Cout, Cin, Torig, transpose,
                                   Tg, dh, dw, src_tap, PH, PW, stride, OHf, OWf, osh, osw, ooh, oow, act, math, ring, xmax);
    if (rc0 == 2) return OG_OK;
    if (rc0 != OG_OK) return rc0;
    hipStream_t s = (hipStream_t)stream;
    const bool v2 = p.m_major != 0, thin = p.m_major == 2;
    if (!wt_packed) {       // wt_packed: the caller kept wt from an earlier call with the same
        if (p.m_major == 5) og_launch_absmax_w(w, (long)Cout * Cin * Torig, const_cast<float*>(p.wmax), s);
        og_launch_pack(p, (long)Tg * p.Cp * p.Mpad, s);   // filter bank, taps, math and geometry class
        int rc = og_launch_status();
        if (rc != OG_OK) return rc;
    }
    if (thin || !v2) {
        a.ymax = nullptr;
        const int rc = thin ? run_thin(a, MT, s) : run_igemm(a, s);
        if (rc == OG_OK && ymax) og_absmax_launch(y, (long)N * a.M * OHf * OWf, ymax, s);
        return rc == OG_OK ? og_launch_status() : rc;
    }
    return run_igemm2(a, s, ws, ws_floats, ymax);
}

// Data gradient of a stride-2 convolution whose four output parity phases have the same tap count
// (k = 4, pad 1, even sizes: 2x2 taps each): ONE launch, the phase is the fastest digit of the workgroup id.  x = dY [N, Cout, OH, OW],
// y = dX [N, Cin, 2*PH, 2*PW] (every element is written by exactly one phase: no pre-zeroing).
// dh/dw/src_tap: 4 phases x Tg entries, phase p = (row parity << 1) | column parity.
// wt: 4 * ceil(1.5 * Cin * Tg * ceil16(Cout)) + 1024 floats (the four phase banks, then the partial maxima of |w|).
int objgan_conv_dgrad_s2_phases(const float* x, const float* w, float* y, float* wt,
                                int N, int Cout, int OH, int OW, int Cin, int Torig,
                                int Tg, const int* dh, const int* dw, const int* src_tap,
                                int PH, int PW, int wt_packed, int math, const float* xmax, float* ws, long ws_floats,
                                void* stream) {
    OG_ENTRY();
    if (Tg < 1 || Tg > 8) return OG_BAD_ARGS;
    if (math < 0 || math > 5 || math == 3 || (math >= 4 && !xmax)) return OG_BAD_ARGS;
    if (Torig < 1 || Torig > 127) return OG_BAD_ARGS;
    if (N <= 0 || PH <= 0 || PW <= 0 || Cin <= 0) return OG_OK;
    const int M = Cin, C = Cout;
    const int Cp = (C + 15) / 16 * 16;
    if ((double)N * C * OH * OW * 4.0 >= 4.0e9 || (double)M * Tg * Cp * 4.0 >= 4.0e9) return OG_BAD_ARGS;
    hipStream_t s = (hipStream_t)stream;
    const int Kpad = Tg * Cp;
    const int Krow = og_krow(Kpad, math);
    if (!wt_packed) {
        if (math >= 4) og_launch_absmax_w(w, (long)Cout * Cin * Torig, wt + og_phase_wmax_offset(M, Tg, Cp), s);
        for (int ph = 0; ph < 4; ++ph) {
            PackArgs p;
            og_fill_pack_phase(p, w, wt, Cout, Cin, Torig, Tg, src_tap + ph * Tg, ph, math);
            og_launch_pack(p, (long)M * Krow, s);
            int rc = og_launch_status();
            if (rc != OG_OK) return rc;
        }
    }
    IgemmArgs a;
    og_phases_args(a, N, Cout, OH, OW, Cin, Tg, PH, PW, math);
    a.x = x; a.wt = wt; a.y = y;
    a.xmax = xmax; a.wmax = wt + og_phase_wmax_offset(M, Tg, Cp);
    for (int t = 0; t < OG_MAX_TAPS; ++t) a.tap[t] = 0;
    for (int ph = 0; ph < 4; ++ph)
        for (int t = 0; t < Tg; ++t)
            a.tap[ph * 8 + t] = (int)(((unsigned)dw[ph * Tg + t] << 16) | ((unsigned)dh[ph * Tg + t] & 0xffffu));
    return run_igemm2(a, s, ws, ws_floats);  // (four phases in one launch: never split along K)
}

// floats of workspace objgan_conv_dgrad_s2_phases takes (bf16 mode: the channel-blocked bf16 copy of dY; else 0)
long objgan_conv_dgrad_s2_phases_ws_floats(int N, int Cout, int OH, int OW, int math) {
    return igemm2_nhwc_floats(math, N, OH, OW, (Cout + 15) / 16 * 16);
}

// The launch plan of objgan_conv_dgrad_s2_phases (the nphase = 4 launch), fields as objgan_conv_igemm_plan.  Host-only.
int objgan_conv_dgrad_s2_phases_plan(int N, int Cout, int OH, int OW, int Cin, int Tg, int PH, int PW, int math, int* out) {
    if (!out || Tg < 1 || Tg > 8) return OG_BAD_ARGS;
    if (math < 0 || math > 5 || math == 3) return OG_BAD_ARGS;
    if (N <= 0 || PH <= 0 || PW <= 0 || Cin <= 0 || Cout <= 0) return OG_BAD_ARGS;
    const int Cp = (Cout + 15) / 16 * 16;
    if ((double)N * Cout * OH * OW * 4.0 >= 4.0e9 || (double)Cin * Tg * Cp * 4.0 >= 4.0e9) return OG_BAD_ARGS;
    IgemmArgs a;
    og_phases_args(a, N, Cout, OH, OW, Cin, Tg, PH, PW, math);
    og_plan_fields(math == 1 ? 3 : (math == 2 ? 4 : (math >= 4 ? 5 : 1)), a, out);
    return OG_OK;
}

// y [planes, H, W] += mirror of ring [planes, 2*(W+2) + 2*(H+2)] (written by objgan_conv_igemm in ring mode).
int objgan_reflect_ring_fold(const float* ring, float* y, long planes, int H, int W, void* stream) {
    OG_ENTRY();
    if (H < 3 || W < 3) return OG_BAD_ARGS;
    if (planes <= 0) return OG_OK;
    const long total = planes * (2 * W + 2 * H);
    hipLaunchKernelGGL(reflect_ring_fold_kernel, dim3(og_stream_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       ring, y, planes, H, W);
    return og_launch_status();
}

}  // extern "C"

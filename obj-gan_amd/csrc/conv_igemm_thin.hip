// Direct fp32 VALU convolutions for thin outputs (M <= 32 channels).
//
// Kernels:  conv_thin_kernel<MT, T, PX>    generic, T = 9 or 4 taps (forward, stride-1 data gradient, one phase of a
//                                          stride-2 data gradient)
//           conv_thin3x3_kernel<MT, R>     3x3 / stride 1 / pad 1 with canonical taps: R output rows per thread
//           conv_thin_ph4_kernel<MT, PX>   data gradient of a 4x4 / stride-2 / pad-1 convolution, four phases in one launch
// Host:     run_thin (called by objgan_conv_igemm when og_bank_layout answers class 2: M <= 32, 9 or 4 taps, at least
//           65 536 output pixels, no tanh / sigmoid epilogue above 4 channels)
// Entry points: objgan_conv_dgrad_s2_thin, objgan_conv_dgrad_s2_thin_floats, objgan_conv_pack_job_thin_phase
#include "conv_igemm_host.h"

// =============================================================================================
// Thin outputs (M <= 32 channels: the 80->12 / 80->24 layout-map stems, to-RGB, data gradients
// down to the 3- / 15-channel discriminator inputs).  A 32-row MFMA tile would spend most of its
// rows on padding; the fp32 VALU has the same peak rate as the fp32 MFMA, so these run as a direct
// convolution: one thread = one output pixel with all M accumulators in registers, the filter bank
// (packed [c][t][MT]) read through the scalar cache into SGPR operands of v_fmac, the T taps of a
// channel as T coalesced buffer loads whose per-lane offsets (bounds / reflection / upsample) are
// computed once per thread.  No LDS, no barriers.
template <int MT, int T, int PX>
__global__ __launch_bounds__(256) void conv_thin_kernel(const IgemmArgs a) {
    // PX output pixels per thread (256 apart): every SGPR filter operand feeds PX FMAs, which
    // keeps the scalar cache (shared between CUs) off the critical path.
    const int Npix = a.N * a.PH * a.PW;
    const int HW = a.H * a.W;
    const int ppi = a.PH * a.PW;
    const int us = a.upsample ? 1 : 0;
    const bool refl = a.pad_mode == 1;
    __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.x, 0, (int)((unsigned)a.N * a.C * HW * 4u), OG_BUF_FLAGS);

    unsigned voff[PX][T];
    bool pix_ok[PX];
    int on[PX], oa[PX], ob[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        const int pix = (blockIdx.x * PX + j) * 256 + threadIdx.x;
        pix_ok[j] = pix < Npix;
        const int pp = pix_ok[j] ? pix : 0;
        const int n = pp / ppi;
        const int rem = pp - n * ppi;
        const int pa = rem / a.PW;
        const int pb = rem - pa * a.PW;
        on[j] = n; oa[j] = pa; ob[j] = pb;
        const int ihb = pa * a.stride, iwb = pb * a.stride;
        const unsigned img_off = (unsigned)n * (unsigned)a.C * (unsigned)HW;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int tp = a.tap[t];
            const int ih = ihb + ((tp << 16) >> 16);
            const int iw = iwb + (tp >> 16);
            int ihr = ih < 0 ? -ih : ih;
            int iwr = iw < 0 ? -iw : iw;
            ihr = ihr >= a.LH ? 2 * (a.LH - 1) - ihr : ihr;
            iwr = iwr >= a.LW ? 2 * (a.LW - 1) - iwr : iwr;
            const bool inb = ((unsigned)ih < (unsigned)a.LH) && ((unsigned)iw < (unsigned)a.LW);
            const bool ok = pix_ok[j] && (refl || inb);
            const int ihs = (refl ? ihr : ih) >> us;
            const int iws = (refl ? iwr : iw) >> us;
            voff[j][t] = ok ? (img_off + (unsigned)(ihs * a.W + iws)) * 4u : OG_OOB;
        }
    }

    float acc[PX][MT];
#pragma unroll
    for (int j = 0; j < PX; ++j)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[j][m] = 0.f;
    const float* __restrict__ wp = a.wt;
    // the taps of the next channel are always in flight behind the FMAs of the current one (the
    // bank carries one zero channel of padding, so an odd C needs no branch)
    auto load_taps = [&](float (&xv)[PX][T], int c) {
        const int so = min(c, a.C - 1) * HW * 4;
#pragma unroll
        for (int j = 0; j < PX; ++j)
#pragma unroll
            for (int t = 0; t < T; ++t)
                xv[j][t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xres, voff[j][t], so, 0));
    };
    auto fma_taps = [&](const float (&xv)[PX][T], int c) {
        const float* __restrict__ wc = wp + (size_t)c * (T * MT);
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float wv = wc[t * MT + m];
#pragma unroll
                for (int j = 0; j < PX; ++j) acc[j][m] = fmaf(wv, xv[j][t], acc[j][m]);
            }
    };
    float xa[PX][T], xb[PX][T];
    load_taps(xa, 0);
    for (int c = 0; c < a.C; c += 2) {
        load_taps(xb, c + 1);
        fma_taps(xa, c);
        load_taps(xa, c + 2);
        fma_taps(xb, c + 1);
    }

    const size_t plane = (size_t)a.OHf * a.OWf;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        if (!pix_ok[j]) continue;
        const int oh = oa[j] * a.osh + a.ooh;
        const int ow = ob[j] * a.osw + a.oow;
        float* yb = a.y + (size_t)on[j] * a.M * plane + (size_t)oh * a.OWf + ow;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < a.M) {
                float v = acc[j][m];
                if (a.bias) v += a.bias[m];
                if (MT <= 4) v = og_act(v, a.act);
                else v = a.act == OG_ACT_LRELU ? (v > 0.f ? v : 0.2f * v) : (a.act == OG_ACT_RELU ? fmaxf(v, 0.f) : v);
                yb[(size_t)m * plane] = v;
            }
        }
    }
}

// 3x3 / stride 1 / pad 1 specialisation of the thin kernel (layout-map stems, to-RGB): one thread =
// one output COLUMN of R consecutive rows.  The (R+2) x 3 input window of a channel is loaded once
// (lanes = consecutive columns: fully coalesced dwords) and serves all R pixels -- (R+2)*3/R loads per
// pixel and channel instead of 9; the generic kernel is bound by the vector-memory issue rate of
// its nine tap loads, not by the FMAs.
template <int MT, int R>
__global__ __launch_bounds__(256) void conv_thin3x3_kernel(const IgemmArgs a) {
    const int HW = a.H * a.W;
    const int strips = (a.PH + R - 1) / R;
    const int per_img = strips * a.PW;
    const int total = a.N * per_img;
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const bool t_ok = gid < total;
    const int g = t_ok ? gid : 0;
    const int n = g / per_img;
    const int rem = g - n * per_img;
    const int sr = rem / a.PW;
    const int pb = rem - sr * a.PW;
    const int pa0 = sr * R;
    const int us = a.upsample ? 1 : 0;
    const bool refl = a.pad_mode == 1;
    __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.x, 0, (int)((unsigned)a.N * a.C * HW * 4u), OG_BUF_FLAGS);
    const unsigned img_off = (unsigned)n * (unsigned)a.C * (unsigned)HW;

    unsigned voff[R + 2][3];
#pragma unroll
    for (int r = 0; r < R + 2; ++r) {
        const int ih = pa0 + r - 1;
        int ihr = ih < 0 ? -ih : ih;
        ihr = ihr >= a.LH ? 2 * (a.LH - 1) - ihr : ihr;
        ihr = ihr < 0 ? 0 : ihr;                      // rows past the last strip row (unused)
        const bool rok = t_ok && (refl ? (ih <= a.LH) : ((unsigned)ih < (unsigned)a.LH));
        const int ihs = (refl ? ihr : ih) >> us;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int iw = pb + c - 1;
            int iwr = iw < 0 ? -iw : iw;
            iwr = iwr >= a.LW ? 2 * (a.LW - 1) - iwr : iwr;
            const bool ok = rok && (refl || (unsigned)iw < (unsigned)a.LW);
            const int iws = (refl ? iwr : iw) >> us;
            voff[r][c] = ok ? (img_off + (unsigned)(ihs * a.W + iws)) * 4u : OG_OOB;
        }
    }

    float acc[R][MT];
#pragma unroll
    for (int j = 0; j < R; ++j)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[j][m] = 0.f;
    const float* __restrict__ wp = a.wt;
    auto load_win = [&](float (&xv)[R + 2][3], int c) {
        const int so = min(c, a.C - 1) * HW * 4;
#pragma unroll
        for (int r = 0; r < R + 2; ++r)
#pragma unroll
            for (int q = 0; q < 3; ++q)
                xv[r][q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xres, voff[r][q], so, 0));
    };
    auto fma_win = [&](const float (&xv)[R + 2][3], int c) {
        const float* __restrict__ wc = wp + (size_t)c * (9 * MT);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const float wv = wc[(kh * 3 + kw) * MT + m];
#pragma unroll
                    for (int j = 0; j < R; ++j) acc[j][m] = fmaf(wv, xv[j + kh][kw], acc[j][m]);
                }
    };
    float xa[R + 2][3], xb[R + 2][3];
    load_win(xa, 0);
    for (int c = 0; c < a.C; c += 2) {
        load_win(xb, c + 1);
        fma_win(xa, c);
        load_win(xa, c + 2);
        fma_win(xb, c + 1);
    }

    if (!t_ok) return;
    const size_t plane = (size_t)a.OHf * a.OWf;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (pa0 + j >= a.PH) break;
        float* yb = a.y + (size_t)n * a.M * plane + (size_t)(pa0 + j) * a.OWf + pb;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < a.M) {
                float v = acc[j][m];
                if (a.bias) v += a.bias[m];
                if (MT <= 4) v = og_act(v, a.act);
                else v = a.act == OG_ACT_LRELU ? (v > 0.f ? v : 0.2f * v) : (a.act == OG_ACT_RELU ? fmaxf(v, 0.f) : v);
                yb[(size_t)m * plane] = v;
            }
        }
    }
}

// Data gradient of a 4x4 / stride-2 / pad-1 convolution w.r.t. an input of <= 32 channels (the first convolution of the
// shape / object discriminators: 12 layout-code channels, 3 image channels), all four output parity phases in ONE launch.
// The per-phase form (conv_thin_kernel, one launch per phase) reads dy four times -- every phase walks the whole
// gradient tensor for a quarter of the output pixels: 16 launches and 6.4 GB of reads per step for the 96 -> 12 layers at
// 256 x 256.  Here a thread owns a SOURCE position (n, a, b) of dy and one ROW parity pa = blockIdx.y: it loads the two
// rows a + pa - 1, a + pa of the 3-wide neighbourhood once per channel (6 values) and produces the two column phases of
// output row 2a + pa -- phase (pa, pb) uses both rows and columns b + {0, -1} (pb = 0) or b + {1, 0} (pb = 1).  dy is read
// twice instead of four times, every output element is written once (8-byte stores of the column pair), same fp32 VALU
// arithmetic: filter bank through the scalar cache (2 phases x 4 taps x MT scalars per channel -- all four phases in one
// thread would need 16 MT and spill SGPRs by the hundred), PX source positions per thread share every SGPR operand.
// Banks: the four phase banks of the thin layout, [Cout + 1][4 taps][MT] each (tap t = i * 2 + j: row choice i, column
// choice j; objgan_conv_dgrad_s2_thin packs them).
template <int MT, int PX>
__global__ __launch_bounds__(256) void conv_thin_ph4_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                            float* __restrict__ y, int N, int C, int H, int W, int M) {
    const int HW = H * W;
    const int Npos = N * HW;
    const int pa = blockIdx.y;                       // row parity of the output rows this workgroup writes
    __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc(
        (void*)x, 0, (int)((unsigned)N * C * HW * 4u), OG_BUF_FLAGS);
    unsigned voff[PX][6];
    bool pos_ok[PX];
    int pn[PX], pr[PX], pb_[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        const int pos = (blockIdx.x * PX + j) * 256 + threadIdx.x;
        pos_ok[j] = pos < Npos;
        const int pp = pos_ok[j] ? pos : 0;
        const int n = pp / HW;
        const int rem = pp - n * HW;
        const int a = rem / W;
        const int b = rem - a * W;
        pn[j] = n; pr[j] = a; pb_[j] = b;
        const unsigned img_off = (unsigned)n * (unsigned)C * (unsigned)HW;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int ih = a + pa - 1 + r, iw = b + c - 1;
                const bool ok = pos_ok[j] && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
                voff[j][r * 3 + c] = ok ? (img_off + (unsigned)(ih * W + iw)) * 4u : OG_OOB;
            }
    }
    float acc[PX][2][MT];
#pragma unroll
    for (int j = 0; j < PX; ++j)
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[j][pb][m] = 0.f;
    const long bank = (long)(C + 1) * 4 * MT;       // floats per phase bank (one zero channel of padding)
    const float* __restrict__ wp = wt + (long)(pa * 2) * bank;
    auto load_nb = [&](float (&xv)[PX][6], int c) {
        const int so = min(c, C - 1) * HW * 4;
#pragma unroll
        for (int j = 0; j < PX; ++j)
#pragma unroll
            for (int q = 0; q < 6; ++q)
                xv[j][q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xres, voff[j][q], so, 0));
    };
    auto fma_nb = [&](const float (&xv)[PX][6], int c) {
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            const float* __restrict__ wc = wp + pb * bank + (size_t)c * (4 * MT);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                // tap t = i * 2 + j: row choice i -> local row 1 - i (dh = 0, -1 for pa = 0; 1, 0 for pa = 1);
                // column choice j -> column pb ? 2 - j : 1 - j of the 3-wide neighbourhood
                const int r = 1 - (t >> 1);
                const int q = pb ? 2 - (t & 1) : 1 - (t & 1);
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const float wv = wc[t * MT + m];
#pragma unroll
                    for (int j = 0; j < PX; ++j) acc[j][pb][m] = fmaf(wv, xv[j][r * 3 + q], acc[j][pb][m]);
                }
            }
        }
    };
    float xa[PX][6], xb[PX][6];
    load_nb(xa, 0);
    for (int c = 0; c < C; c += 2) {                 // (an odd C runs one step into the bank's zero channel)
        load_nb(xb, c + 1);
        fma_nb(xa, c);
        load_nb(xa, c + 2);
        fma_nb(xb, c + 1);
    }
    const int OWf = 2 * W;
    const size_t plane = (size_t)(2 * H) * OWf;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        if (!pos_ok[j]) continue;
        float* yb = y + (size_t)pn[j] * M * plane + (size_t)(2 * pr[j] + pa) * OWf + 2 * pb_[j];
#pragma unroll
        for (int m = 0; m < MT; ++m)
            if (m < M) *reinterpret_cast<float2*>(yb + (size_t)m * plane) = make_float2(acc[j][0][m], acc[j][1][m]);
    }
}

// f(OgInt<MT>{}) for the accumulator count og_thin_mt() chose (4 / 12 / 16 / 24 / 32)
template <class F> static inline void og_with_mt(int MT, F&& f) {
    if (MT == 4) f(OgInt<4>{}); else if (MT == 12) f(OgInt<12>{}); else if (MT == 16) f(OgInt<16>{});
    else if (MT == 24) f(OgInt<24>{}); else f(OgInt<32>{});
}

int run_thin(IgemmArgs a, int MT, hipStream_t s) {
    const long Npix = (long)a.N * a.PH * a.PW;
    if (og_trace()) fprintf(stderr, "OGTRACE thin MT=%d M=%d C=%d T=%d Npix=%ld\n", MT, a.M, a.C, a.T, Npix);
    bool canon = a.T == 9 && a.stride == 1 && a.osh == 1 && a.osw == 1 && a.ooh == 0 && a.oow == 0
                 && a.PH == a.OHf && a.PW == a.OWf && a.PH == a.LH && a.PW == a.LW;
    for (int t = 0; canon && t < 9; ++t)
        canon = a.tap[t] == (int)((((unsigned)(t % 3 - 1)) << 16) | ((unsigned)(t / 3 - 1) & 0xffffu));
    a.m_begin = 0; a.m_end = a.M; a.ksplit_steps = 0;
    if (canon) {
        const int R = MT <= 16 ? 4 : 2;
        const long threads = (long)a.N * og_cdiv(a.PH, R) * a.PW;
        dim3 g3(og_cdiv(threads, 256));
        ProfRec* pr = prof_begin(og_prof_cat(OG_FAM_THIN3), 2.0 * a.M * (double)a.K * (double)Npix, s);
        prof_meta(pr, 2, MT, a.M, a.C, a.T, a.N, a.PH, a.PW, a.stride, 1);
        og_with_mt(MT, [&](auto mt) {
            constexpr int M_ = decltype(mt)::value;
            hipLaunchKernelGGL((conv_thin3x3_kernel<M_, (M_ <= 16 ? 4 : 2)>), g3, dim3(256), 0, s, a);
        });
        prof_end(pr, s);
        return og_launch_status();
    }
    const int PX = MT <= 16 ? 2 : 1;
    dim3 grid(og_cdiv(Npix, 256 * PX));
    ProfRec* pr = prof_begin(og_prof_cat(OG_FAM_THIN), 2.0 * a.M * (double)a.K * (double)Npix, s);
    prof_meta(pr, 2, MT, a.M, a.C, a.T, a.N, a.PH, a.PW, a.stride * (a.osh > 1 ? -1 : 1), 1);
    og_with_mt(MT, [&](auto mt) {
        constexpr int M_ = decltype(mt)::value;
        if (a.T == 9) hipLaunchKernelGGL((conv_thin_kernel<M_, 9, (M_ <= 16 ? 2 : 1)>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((conv_thin_kernel<M_, 4, (M_ <= 16 ? 2 : 1)>), grid, dim3(256), 0, s, a);
    });
    prof_end(pr, s);
    return og_launch_status();
}

static void og_thin_phase_taps(int phase, int* st) {      // source taps of phase (pa, pb), t = i * 2 + j (see the kernel)
    const int pa = phase >> 1, pb = phase & 1;
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
            const int kh = pa ? 2 * i : 1 + 2 * i, kw = pb ? 2 * j : 1 + 2 * j;     // dh = (pa + 1 - kh) / 2: 0, -1 | 1, 0
            st[i * 2 + j] = kh * 4 + kw;
        }
}
static void og_fill_pack_thin_phase(PackArgs& p, const float* w, float* wt, int Cout, int Cin, int phase) {
    int st[4];
    og_thin_phase_taps(phase, st);
    memset(&p, 0, sizeof(p));
    og_fill_pack_phase(p, w, wt, Cout, Cin, 16, 4, st, phase, -2);
}

extern "C" {

// Data gradient of a 4 x 4 / stride-2 / pad-1 convolution w.r.t. an input of Cin <= 32 channels, all four output parity
// phases in ONE launch of the fp32 VALU kernel (conv_thin_ph4_kernel: dy read twice instead of four times): dy [N, Cout, OH, OW]
// -> dx [N, Cin, 2 OH, 2 OW], every element written exactly once (no pre-zeroing).  w [Cout][Cin][16]; wt: objgan_conv_dgrad_s2_thin_floats(Cout, Cin) floats
// (the four phase banks of the thin layout), packed by the call unless wt_packed.
long objgan_conv_dgrad_s2_thin_floats(int Cout, int Cin) {
    if (Cout <= 0 || Cin <= 0 || Cin > 32) return 0;
    return 4L * (Cout + 1) * 4 * og_thin_mt(Cin);
}
// the pack job of phase `phase` of that bank set (for objgan_conv_pack_jobs_run)
int objgan_conv_pack_job_thin_phase(void* job, const float* w, float* wt, int Cout, int Cin, int phase) {
    if (!job || phase < 0 || phase > 3 || Cin > 32 || Cin <= 0 || Cout <= 0) return OG_BAD_ARGS;
    PackArgs p;
    og_fill_pack_thin_phase(p, w, wt, Cout, Cin, phase);
    memcpy(job, &p, sizeof(p));
    return OG_OK;
}
int objgan_conv_dgrad_s2_thin(const float* dy, const float* w, float* dx, float* wt, int N, int Cout, int OH, int OW,
                              int Cin, int wt_packed, void* stream) {
    OG_ENTRY();
    if (Cin <= 0 || Cin > 32 || Cout <= 0) return OG_BAD_ARGS;
    if (N <= 0 || OH <= 0 || OW <= 0) return OG_OK;
    if ((double)N * Cout * OH * OW * 4.0 >= 4.0e9 || (double)N * OH * OW >= 2.0e9) return OG_BAD_ARGS;
    hipStream_t s = (hipStream_t)stream;
    const int MT = og_thin_mt(Cin);
    if (!wt_packed) {
        for (int ph = 0; ph < 4; ++ph) {
            PackArgs p;
            og_fill_pack_thin_phase(p, w, wt, Cout, Cin, ph);
            og_launch_pack(p, (long)(Cout + 1) * 4 * MT, s);
            int rc = og_launch_status();
            if (rc != OG_OK) return rc;
        }
    }
    const long Npos = (long)N * OH * OW;
    const int PX = MT <= 16 ? 2 : 1;
    dim3 grid(og_cdiv(Npos, 256 * PX), 2);           // y: row parity of the output rows
    ProfRec* pr = prof_begin(og_prof_cat(OG_FAM_THIN), 2.0 * Cin * (double)Cout * 4.0 * (double)Npos * 4.0, s);
    prof_meta(pr, 2, MT, Cin, Cout, 4, N, 4 * OH, OW, -1, 1);
    og_with_mt(MT, [&](auto mt) {
        constexpr int M_ = decltype(mt)::value;
        hipLaunchKernelGGL((conv_thin_ph4_kernel<M_, (M_ <= 16 ? 2 : 1)>), grid, dim3(256), 0, s, dy, wt, dx, N, Cout, OH, OW, Cin);
    });
    prof_end(pr, s);
    return og_launch_status();
}

}  // extern "C"

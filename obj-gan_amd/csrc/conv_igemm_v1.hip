// First-generation implicit-GEMM kernels (both operands through LDS, fp32 MFMA, plain pointer loads).
//
// Kernels:  conv_igemm_kernel<WM, TM>      forward / data gradient: 128x128, 64x256 or 32x256 tiles (cfg 0 / 1 / 2)
//           conv_wgrad_kernel<KS, WM, TM>  weight gradient on the same three tile shapes
// Host:     run_igemm, og_launch_wgrad_v1 (called by objgan_conv_igemm / objgan_conv_wgrad); no entry point of its own.
// Chosen only where the buffer-descriptor kernels cannot go: a source or bank beyond the 2 GiB reach of a 32-bit
// buffer range (og_bank_layout class 0), weight gradients of maps whose width is not a multiple of 8 or whose pixel
// count is not a multiple of 16 (og_wgrad_plan: v2 = 0) -- or everywhere with OG_IGEMM_V1=1 in a development build.
#include "conv_igemm_host.h"

template <int WM, int TM>
__global__ __launch_bounds__(256) void conv_igemm_kernel(const IgemmArgs a) {
    constexpr int WN = 4 / WM;
    constexpr int TN = 2;
    constexpr int BM = WM * TM * 32;
    constexpr int BN = WN * TN * 32;
    constexpr int BK = 16;
    constexpr int BROWS = BK * BN / 256;   // gathered elements per thread per K step
    constexpr int KSTEP = 256 / BN;        // k rows covered by one pass of the workgroup
    constexpr int NA4 = BK * BM / 4;       // float4s in one A tile
    constexpr int NA_PER = (NA4 + 255) / 256;

    __shared__ float As[2][BK][BM];
    __shared__ float Bs[2][BK][BN];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid / WN, wn = wid % WN;

    const int Npix = a.N * a.PH * a.PW;
    const int tiles_m = (a.m_end - a.m_begin + BM - 1) / BM;
    const int tiles_n = (Npix + BN - 1) / BN;
    const int nwg = tiles_m * tiles_n;
    const int wg = og_xcd_remap(blockIdx.x, nwg);
    const int tile_m = wg % tiles_m;
    const int tile_n = wg / tiles_m;
    const int m0 = a.m_begin + tile_m * BM;
    const int n0 = tile_n * BN;

    // ---- per-thread gather geometry (the pixel of a thread is fixed for the whole K loop)
    const int kr0 = __builtin_amdgcn_readfirstlane(tid / BN);
    const int pix = n0 + (tid % BN);
    const bool pix_ok = pix < Npix;
    int ihb = 0, iwb = 0;
    const float* xb = a.x;
    {
        const int ppi = a.PH * a.PW;
        const int pp = pix_ok ? pix : 0;
        const int n = pp / ppi;
        const int rem = pp - n * ppi;
        const int pa = rem / a.PW;
        const int pb = rem - pa * a.PW;
        ihb = pa * a.stride;
        iwb = pb * a.stride;
        xb = a.x + (size_t)n * a.C * a.H * a.W;
    }
    const int HW = a.H * a.W;

    float rb[BROWS];
    float4 ra[NA_PER];
#pragma unroll
    for (int i = 0; i < NA_PER; ++i) ra[i] = make_float4(0.f, 0.f, 0.f, 0.f);

    // Branch-free gather.  One K step = 16 consecutive channels of ONE tap: the tap geometry is
    // evaluated once per step; every lane always issues its BROWS loads (from a clamped, in-range
    // address) so they are all in flight together; out-of-image / padded-channel elements are
    // zeroed by a bit mask when the tile is written to LDS.
    unsigned okmask = 0;
    const int us = a.upsample ? 1 : 0;
    const int steps_per_tap = a.Cp / BK;
    const bool refl = a.pad_mode == 1;
    auto load_b = [&](int kt) {
        const int t = kt / steps_per_tap;                // wave-uniform
        const int cb = (kt - t * steps_per_tap) * BK;
        const int tp = a.tap[t];
        const int ih = ihb + ((tp << 16) >> 16);
        const int iw = iwb + (tp >> 16);
        int ihr = ih < 0 ? -ih : ih;
        int iwr = iw < 0 ? -iw : iw;
        ihr = ihr >= a.LH ? 2 * (a.LH - 1) - ihr : ihr;
        iwr = iwr >= a.LW ? 2 * (a.LW - 1) - iwr : iwr;
        const bool inb = ((unsigned)ih < (unsigned)a.LH) && ((unsigned)iw < (unsigned)a.LW);
        const bool ok = pix_ok && (refl || inb);
        const int ihs = (refl ? ihr : ih) >> us;
        const int iws = (refl ? iwr : iw) >> us;
        const float* src = xb + (ok ? ihs * a.W + iws : 0);
        okmask = 0;
#pragma unroll
        for (int i = 0; i < BROWS; ++i) {
            const int c = cb + kr0 + KSTEP * i;          // wave-uniform
            const int cc = min(c, a.C - 1);
            rb[i] = src[(size_t)cc * HW];
            okmask |= ((ok && c < a.C) ? 1u : 0u) << i;
        }
    };
    constexpr bool A_FULL = (NA4 % 256) == 0;   // every thread loads NA_PER float4s
    const bool a_thread = A_FULL || tid < NA4;
    auto load_a = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NA_PER; ++i) {
            const int idx = tid + 256 * i;
            const int k = idx / (BM / 4);
            const int m4 = (idx - k * (BM / 4)) * 4;
            if (a_thread)
                ra[i] = *reinterpret_cast<const float4*>(a.wt + (size_t)(k0 + k) * a.Mpad + m0 + m4);
        }
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NA_PER; ++i) {
            const int idx = tid + 256 * i;
            const int k = idx / (BM / 4);
            const int m4 = (idx - k * (BM / 4)) * 4;
            if (a_thread) *reinterpret_cast<float4*>(&As[buf][k][m4]) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < BROWS; ++i)
            Bs[buf][kr0 + KSTEP * i][tid % BN] = ((okmask >> i) & 1u) ? rb[i] : 0.f;
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int kt0 = 0;                         // (this kernel is never split along K: no fp32 atomics in the library's convolutions)
    const int nk = a.Kpad / BK;
    load_a(kt0 * BK);
    load_b(kt0);
    store_tiles(0);
    __syncthreads();

    const int lrow = lane >> 5;          // k sub-index of the 32x32x2 MFMA operand
    const int lcol = lane & 31;
    int cur = 0;
    for (int kt = kt0; kt < nk; ++kt) {
        const bool more = (kt + 1) < nk;
        if (more) { load_a((kt + 1) * BK); load_b(kt + 1); }
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            float av[TM], bv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) av[i] = As[cur][2 * kk + lrow][(wm * TM + i) * 32 + lcol];
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[j] = Bs[cur][2 * kk + lrow][(wn * TN + j) * 32 + lcol];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        if (more) store_tiles(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    // ---- epilogue: C/D layout of the 32x32 MFMA: col = lane & 31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
    const int ppi = a.PH * a.PW;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int p = n0 + (wn * TN + j) * 32 + lcol;
        if (p >= Npix) continue;
        const int n = p / ppi;
        const int rem = p - n * ppi;
        const int pa = rem / a.PW;
        const int pb = rem - pa * a.PW;
        const int oh = pa * a.osh + a.ooh;
        const int ow = pb * a.osw + a.oow;
        float* yb = a.y + (size_t)n * a.M * a.OHf * a.OWf + (size_t)oh * a.OWf + ow;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lrow;
                if (m < a.m_end) {
                    float v = acc[i][j][r];
                    if (a.bias) v += a.bias[m];
                    v = og_act(v, a.act);
                    yb[(size_t)m * a.OHf * a.OWf] = v;
                }
            }
        }
    }
}

template <int KS, int WM, int TM>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradArgs a) {
    constexpr int T = KS * KS;
    constexpr int WN = 4 / WM;
    constexpr int TN = 2;
    constexpr int BM = WM * TM * 32;
    constexpr int BN = WN * TN * 32;
    constexpr int BK = 32;
    constexpr int LD = BK + 1;
    constexpr int AR = BM / 8;     // dy elements per thread per K step
    constexpr int BR = BN / 8;     // gathered x elements per thread per K step

    __shared__ float As[2][BM][LD];
    __shared__ float Bs[2][BN][LD];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid / WN, wn = wid % WN;

    const int tiles_m = (a.m_end - a.m_begin + BM - 1) / BM;
    const int tiles_n = (a.ncol + BN - 1) / BN;
    const int nwg = tiles_m * tiles_n;
    const int wg = og_xcd_remap(blockIdx.x, nwg);
    const int tile_m = wg % tiles_m;
    const int tile_n = wg / tiles_m;
    const int m0 = a.m_begin + tile_m * BM;
    const int c0 = tile_n * BN;

    const int Npix = a.N * a.OH * a.OW;
    const int p_begin = blockIdx.y * a.pix_per_split;
    const int p_end = min(Npix, p_begin + a.pix_per_split);
    if (p_begin >= p_end) return;

    const int kl = tid & 31;       // pixel within the K tile
    const int r0 = tid >> 5;       // first row handled by this thread (rows r0 + 8*i)
    const int OHW = a.OH * a.OW;
    const int HW = a.H * a.W;

    float ra[AR], rb[BR];

    unsigned amask = 0, bmask = 0;
    const int us = a.upsample ? 1 : 0;
    auto load_tiles = [&](int pk) {
        const int p = pk + kl;
        const bool ok = p < p_end;
        const int pp = ok ? p : p_begin;
        const int n = pp / OHW;
        const int rem = pp - n * OHW;
        const int oh = rem / a.OW;
        const int ow = rem - oh * a.OW;
        const float* dyb = a.dy + (size_t)n * a.Cout * OHW + rem;
        amask = 0; bmask = 0;
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int m = m0 + r0 + 8 * i;
            const bool mok = ok && m < a.m_end;
            ra[i] = dyb[(size_t)(mok ? m : m0) * OHW];
            amask |= (mok ? 1u : 0u) << i;
        }
        const float* xb = a.x + (size_t)n * a.Cin * HW;
        const int ihb = oh * a.stride - a.pad;
        const int iwb = ow * a.stride - a.pad;
        const bool refl = a.pad_mode == 1;
#pragma unroll
        for (int i = 0; i < BR; ++i) {
            const int col = c0 + r0 + 8 * i;
            const int cc = min(col, a.ncol - 1);
            const int ci = cc / T;
            const int t = cc - ci * T;
            const int kh = t / KS;
            const int kw = t - kh * KS;
            const int ih = ihb + kh, iw = iwb + kw;
            int ihr = ih < 0 ? -ih : ih;
            int iwr = iw < 0 ? -iw : iw;
            ihr = ihr >= a.LH ? 2 * (a.LH - 1) - ihr : ihr;
            iwr = iwr >= a.LW ? 2 * (a.LW - 1) - iwr : iwr;
            const bool inb = ((unsigned)ih < (unsigned)a.LH) && ((unsigned)iw < (unsigned)a.LW);
            const bool cok = ok && (col < a.ncol) && (refl || inb);
            const int ihs = (refl ? ihr : ih) >> us;
            const int iws = (refl ? iwr : iw) >> us;
            const int off = cok ? (ci * HW + ihs * a.W + iws) : 0;
            rb[i] = xb[off];
            bmask |= (cok ? 1u : 0u) << i;
        }
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int i = 0; i < AR; ++i) As[buf][r0 + 8 * i][kl] = ((amask >> i) & 1u) ? ra[i] : 0.f;
#pragma unroll
        for (int i = 0; i < BR; ++i) Bs[buf][r0 + 8 * i][kl] = ((bmask >> i) & 1u) ? rb[i] : 0.f;
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = (p_end - p_begin + BK - 1) / BK;
    load_tiles(p_begin);
    store_tiles(0);
    __syncthreads();

    const int lrow = lane >> 5;
    const int lcol = lane & 31;
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = (kt + 1) < nk;
        if (more) load_tiles(p_begin + (kt + 1) * BK);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            float av[TM], bv[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) av[i] = As[cur][(wm * TM + i) * 32 + lcol][2 * kk + lrow];
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[j] = Bs[cur][(wn * TN + j) * 32 + lcol][2 * kk + lrow];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        if (more) store_tiles(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = c0 + (wn * TN + j) * 32 + lcol;
        if (col >= a.ncol) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lrow;
                if (m < a.m_end) og_wgrad_store(a, m, col, acc[i][j][r], blockIdx.y);
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------
static int launch_igemm(const IgemmArgs& a, int cfg, hipStream_t s) {
    const int rows = a.m_end - a.m_begin, Npix = a.N * a.PH * a.PW;
    const dim3 grid(og_cdiv(rows, cfg == 0 ? 128 : (cfg == 1 ? 64 : 32)) * og_cdiv(Npix, cfg == 0 ? 128 : 256), 1);
    if (cfg == 0) hipLaunchKernelGGL((conv_igemm_kernel<2, 2>), grid, dim3(256), 0, s, a);
    else if (cfg == 1) hipLaunchKernelGGL((conv_igemm_kernel<1, 2>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((conv_igemm_kernel<1, 1>), grid, dim3(256), 0, s, a);
    return og_launch_status();
}

// Grids of thousands of workgroups, never split along K: no fp32 atomic is left in the library's convolutions.
int run_igemm(IgemmArgs a, hipStream_t s) {
    RowPart parts[3];
    const int np = og_row_parts(a.M, parts);
    a.ksplit_steps = 0;
    for (int i = 0; i < np; ++i) {
        a.m_begin = parts[i].m_begin; a.m_end = parts[i].m_end;
        const double fl = 2.0 * (a.m_end - a.m_begin) * (double)a.K * ((double)a.N * a.PH * a.PW);
        ProfRec* pr = prof_begin(og_prof_cat(OG_FAM_IGEMM1), fl, s);
        int rc = launch_igemm(a, parts[i].cfg, s);
        prof_end(pr, s);
        if (rc != OG_OK) return rc;
    }
    return OG_OK;
}

// one part of a v1 weight-gradient plan (objgan_conv_wgrad, conv_igemm_wgrad.hip)
void og_launch_wgrad_v1(const WgradArgs& a, int cfg, dim3 grid, int ksize, hipStream_t s) {
    const auto go = [&](auto ks) {
        constexpr int KS = decltype(ks)::value;
        if (cfg == 0) hipLaunchKernelGGL((conv_wgrad_kernel<KS, 2, 2>), grid, dim3(256), 0, s, a);
        else if (cfg == 1) hipLaunchKernelGGL((conv_wgrad_kernel<KS, 1, 2>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((conv_wgrad_kernel<KS, 1, 1>), grid, dim3(256), 0, s, a);
    };
    if (ksize == 1) go(OgInt<1>{}); else if (ksize == 3) go(OgInt<3>{}); else go(OgInt<4>{});
}

// Weight gradient of the implicit-GEMM convolution: dW[m][c][t] = sum over output pixels of dy[m][p] * x[c][p @ tap t].
// GEMM rows = output channels, columns = (channel, tap), K = pixels.  The reduction over pixels is split across
// gridDim.y; each split writes its partial tile into its own workspace slot and wgrad_combine_kernel sums the slots in
// split order into dw (stored, or added when `accumulate`): bit-reproducible, no atomics, dw needs no zero-fill.
//
// Kernels, in the order og_wgrad_plan chooses them:
//   conv_wgrad_rec_kernel / conv_wgrad_rec2_kernel (conv_igemm_rec.hip)   math 5 / 6 / 7: x as its fp16 record
//   conv_wgrad_bfb_kernel<TM, NW>    math 1 / 3 with a workspace, maps of 32+ pixels: x from its bf16 channel-blocked copy
//   conv_wgrad3_kernel<TM, ..>       register-fragment form (x straight from the gather registers): short tiles, wide stride-1
//                                    maps (16-byte gathers), bf16x3 / fp16x2 wherever the constant-stride gather applies
//   conv_wgrad2_kernel<TM, ..>       LDS-staged form: everything else
//   conv_wgrad_kernel (conv_igemm_v1.hip)   maps whose width is not a multiple of 8, tensors beyond 2 GiB
//   wgrad_combine_kernel             the second level of the pixel split
// Host: og_wgrad_plan (pure: form, operand copies, parts, workspace), launch_wgrad2; objgan_conv_wgrad walks the parts.
// Entry points: objgan_conv_wgrad, objgan_conv_wgrad_ws_floats, objgan_conv_wgrad_plan, objgan_conv_wgrad_rec_ok,
// objgan_conv_wgrad_bfb_ok.
#include "conv_igemm_host.h"

// dw rows <- sum over the splits of a weight-gradient launch (WgradArgs::ws): local row r of the slot is dw row
// m_begin + r for r < main_rows, extra row xr_begin + (r - main_rows) behind them.
// V4 (the host asks for it when ws is 16-byte aligned, ws_stride % 4 == 0 and total < 2^31): four consecutive elements per
// thread as one 16-byte load per slot, several slots in flight, every lane summed in the same slot order.  No division:
// the slot is two runs of consecutive dw elements -- the main rows from dw row m_begin, the extra rows from dw row
// xr_begin -- so an element's address is its index plus the offset of its run.  A group that lies in one run at a
// 16-byte aligned address is one 16-byte store (every group when ncol % 4 == 0 and dw is aligned; every main-row group
// of the 194-channel layers, ncol = 1 746, whose launches start at row 0); any other group stores its four elements one
// by one.  The scalar loop behind it takes the total % 4 tail, or everything.
template <bool V4>
__global__ __launch_bounds__(256) void wgrad_combine_kernel(const float* __restrict__ ws, int splits, long ws_stride,
                                                            float* __restrict__ dw, int ncol, int m_begin, int main_rows,
                                                            int xr_begin, long total, int accumulate) {
    long e0 = 0;
    if (V4) {
        const unsigned n4 = (unsigned)(total >> 2);
        const f32x4* p4 = reinterpret_cast<const f32x4*>(ws);
        const size_t stride4 = (size_t)ws_stride >> 2;
        const long main_end = (long)main_rows * ncol;                         // slot elements of the main rows
        // element e of the slot is dw[off_main + e], or dw[off_xr + e] from main_end on -- offsets, not pointers: a launch
        // without extra rows has no element from main_end on, and whatever xr_begin holds then never becomes an address
        const long off_main = (long)m_begin * ncol, off_xr = (long)xr_begin * ncol - main_end;
        for (unsigned g = blockIdx.x * 256u + threadIdx.x; g < n4; g += gridDim.x * 256u) {
            const f32x4 v = og_sum_slots4<8>(p4 + g, splits, stride4);
            const long e = (long)g << 2;
            float* o = dw + ((e < main_end ? off_main : off_xr) + e);
            if ((e + 3 < main_end || e >= main_end) && !((size_t)o & 15)) {
                f32x4* o4 = reinterpret_cast<f32x4*>(o);
                *o4 = accumulate ? *o4 + v : v;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float* oj = dw + ((e + j < main_end ? off_main : off_xr) + e + j);
                    *oj = accumulate ? *oj + v[j] : v[j];
                }
            }
        }
        e0 = (long)n4 << 2;
    }
    for (long e = e0 + (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const float* p = ws + e;
        float v = p[0];
        for (int k = 1; k < splits; ++k) v += p[(size_t)k * ws_stride];
        const long r = e / ncol;
        const int col = (int)(e - r * ncol);
        const long row = r < main_rows ? m_begin + r : xr_begin + (r - main_rows);
        float* o = dw + row * ncol + col;
        *o = accumulate ? *o + v : v;
    }
}

__device__ __forceinline__ void og_wgrad_store_xr(const WgradArgs& a, int j, int col, float v, int split) {
    if (a.ws) {
        a.ws[(size_t)split * a.ws_stride + (size_t)(a.m_end - a.m_begin + j) * a.ncol + col] = v;
    } else {
        float* p = a.dw + (size_t)(a.xr_begin + j) * a.ncol + col;
        *p = a.accumulate ? *p + v : v;
    }
}

// ---- weight gradient, v2 -----------------------------------------------------------------------
// Same tiling / LDS layout / buffer-load scheme as conv_igemm3_kernel (with both operands in LDS): tile (32*TM) x 128 columns
// (column = ci*T + t), K = 16 output pixels per step.  Requires OW % 8 == 0 and (OH*OW) % 16 == 0
// (every layer of the hot path above 4x4 maps), so that the eight pixels a thread gathers per step
// lie in one output row and a K step lies in one image: the pixel part of every address is then a
// SCALAR (n, oh, ow0 .. ow0+7), the per-lane part is the column's (ci, kh, kw) -- dy rows are read
// as aligned 16-byte pieces with a constant per-lane offset, x elements as dwords whose validity
// (zero padding) rides on the buffer range check.
template <int TM, int MATH = 0, int XR = 0>
__global__ __launch_bounds__(256) void conv_wgrad2_kernel(const WgradArgs a, const int KS) {
    // MATH as in conv_igemm3_kernel.  SP (bf16x3): both operands are activations, so both are split when they are
    // written to LDS -- by the thread that loaded them, once per element (not once per wave that reads them) --
    // into the row image [h 16 | m 16 | l 16] bf16 + 16 bytes of padding (112-byte pitch).
    constexpr bool BF = MATH == 1, SP = MATH == 2;
    constexpr int BM = 32 * TM;
    constexpr int BN = 128;
    constexpr int BK = 16;
    constexpr int LD = SP ? 28 : BK + 4;
    constexpr int NA4 = BM * 4;
    constexpr int NA_PER = (NA4 + 255) / 256;
    constexpr int AROWS = BM + XR;                     // dy rows in LDS (XR extra rows, see WgradArgs)
    constexpr int TILE = (AROWS + BN) * LD;
    static_assert(XR == 0 || MATH == 0, "extra rows: fp32 only");

    __shared__ __attribute__((aligned(16))) float lds[2 * TILE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);

    const int T = KS * KS;
    const int tiles_m = (a.m_end - a.m_begin + BM - 1) / BM;
    const int tiles_n = (a.ncol + BN - 1) / BN;
    // XCD placement over both grid dimensions: all tiles of a pixel split on one XCD (they read the same dy / x pixels),
    // an XCD takes a contiguous range of splits (see conv_wgrad_bfb_kernel)
    const int nwg = tiles_m * tiles_n;
    const int vid = og_xcd_remap(blockIdx.x + nwg * blockIdx.y, nwg * gridDim.y);
    const int split = vid / nwg;
    const int wg = vid - split * nwg;
    const int tile_m = wg % tiles_m;
    const int tile_n = wg / tiles_m;
    const int m0 = a.m_begin + tile_m * BM;
    const int c0 = tile_n * BN;

    const int OHW = a.OH * a.OW;
    const int HW = a.H * a.W;
    const int Npix = a.N * OHW;
    const int p_begin = split * a.pix_per_split;
    const int p_end = min(Npix, p_begin + a.pix_per_split);
    if (p_begin >= p_end) return;

    __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.x, 0, (int)((unsigned)a.N * a.Cin * HW * 4u), OG_BUF_FLAGS);
    __amdgpu_buffer_rsrc_t dyres = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.dy, 0, (int)((unsigned)a.N * a.Cout * OHW * 4u), OG_BUF_FLAGS);

    // ---- B (gathered x) geometry: thread = (column of the tile, k half)
    const int bc = tid & (BN - 1);
    const int bg = __builtin_amdgcn_readfirstlane(tid >> 7);
    const int col = c0 + bc;
    const bool col_ok = col < a.ncol;
    int dh, dw;
    unsigned ci_off;
    {
        const int cc = col_ok ? col : 0;
        const int ci = cc / T;
        const int t = cc - ci * T;
        const int kh = t / KS;
        dh = kh - a.pad;
        dw = (t - kh * KS) - a.pad;
        ci_off = (unsigned)ci * (unsigned)HW;
    }
    const int us = a.upsample ? 1 : 0;
    const bool refl = a.pad_mode == 1;

    // ---- A (dy) geometry: float4 idx -> (row, quarter); constant per-lane offset
    unsigned avoff[NA_PER];
    int alds[NA_PER];
#pragma unroll
    for (int i = 0; i < NA_PER; ++i) {
        const int idx = tid + 256 * i;
        const int row = idx >> 2, q = idx & 3;
        const bool on = (NA4 % 256 == 0 || idx < NA4) && (m0 + row) < a.m_end;
        avoff[i] = on ? ((unsigned)(m0 + row) * (unsigned)OHW + q * 4u) * 4u : OG_OOB;
        alds[i] = (NA4 % 256 == 0 || idx < NA4) ? row * LD + q * (SP ? 2 : 4) : -1;   // SP: 8-byte h piece of 4 pixels
    }

    const bool has_x = XR > 0 && tile_m == 0 && a.xr_count > 0;
    const bool x_loader = has_x && tid < XR * 4;
    const unsigned xvoff = (x_loader && (tid >> 2) < a.xr_count)
        ? ((unsigned)(a.xr_begin + (tid >> 2)) * (unsigned)OHW + (tid & 3) * 4u) * 4u : OG_OOB;
    f32x4 ra[NA_PER];
    f32x4 rax = {0.f, 0.f, 0.f, 0.f};
    float rb[8];
    // scalar pixel state of the next K step to load: image n, offset rem in the image, and the
    // (row, first column) of this wave's eight pixels; advanced incrementally (no divisions)
    int n_ld = p_begin / OHW;
    int rem_ld = p_begin - n_ld * OHW;
    int oh_ld = (rem_ld + bg * 8) / a.OW;
    int ow_ld = (rem_ld + bg * 8) - oh_ld * a.OW;
    auto load_step = [&]() {
        const int n = n_ld, oh = oh_ld, ow0 = ow_ld;
        const int asoff = (n * a.Cout * OHW + rem_ld) * 4;
#pragma unroll
        for (int i = 0; i < NA_PER; ++i)
            ra[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyres, avoff[i], asoff, 0));
        if (XR > 0 && has_x)
            rax = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyres, xvoff, asoff, 0));
        rem_ld += BK;
        ow_ld += BK;
        while (ow_ld >= a.OW) { ow_ld -= a.OW; oh_ld += 1; }
        if (rem_ld >= OHW) {                         // next step starts a new image
            rem_ld = 0; n_ld += 1;
            oh_ld = (bg * 8) / a.OW;
            ow_ld = (bg * 8) - oh_ld * a.OW;
        }
        const int ih = oh * a.stride + dh;
        int ihr = ih < 0 ? -ih : ih;
        ihr = ihr >= a.LH ? 2 * (a.LH - 1) - ihr : ihr;
        const bool row_ok = col_ok && (refl || (unsigned)ih < (unsigned)a.LH);
        const unsigned rbase = (unsigned)n * (unsigned)a.Cin * (unsigned)HW + ci_off
                             + (unsigned)(((refl ? ihr : ih) >> us) * a.W);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int iw = (ow0 + i) * a.stride + dw;
            int iwr = iw < 0 ? -iw : iw;
            iwr = iwr >= a.LW ? 2 * (a.LW - 1) - iwr : iwr;
            const bool ok = row_ok && (refl || (unsigned)iw < (unsigned)a.LW);
            const unsigned vo = ok ? (rbase + (unsigned)((refl ? iwr : iw) >> us)) * 4u : OG_OOB;
            rb[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xres, vo, 0, 0));
        }
    };
    auto store_step = [&](int buf) {
        float* As = lds + buf * TILE;
        float* Bs = As + AROWS * LD;
        if (SP) {
#pragma unroll
            for (int i = 0; i < NA_PER; ++i) {
                bf16x4 h, m, l;
                og_split4(ra[i], h, m, l);
                if (NA4 % 256 == 0 || alds[i] >= 0) {
                    *reinterpret_cast<bf16x4*>(As + alds[i]) = h;
                    *reinterpret_cast<bf16x4*>(As + alds[i] + 8) = m;
                    *reinterpret_cast<bf16x4*>(As + alds[i] + 16) = l;
                }
            }
            bf16x8 h, m, l;
            og_split8(rb, h, m, l);
            *reinterpret_cast<bf16x8*>(Bs + bc * LD + bg * 4) = h;
            *reinterpret_cast<bf16x8*>(Bs + bc * LD + bg * 4 + 8) = m;
            *reinterpret_cast<bf16x8*>(Bs + bc * LD + bg * 4 + 16) = l;
            return;
        }
#pragma unroll
        for (int i = 0; i < NA_PER; ++i)
            if (NA4 % 256 == 0 || alds[i] >= 0) *reinterpret_cast<f32x4*>(As + alds[i]) = ra[i];
        if (XR > 0 && x_loader) *reinterpret_cast<f32x4*>(As + (BM + (tid >> 2)) * LD + (tid & 3) * 4) = rax;
        f32x4 v0 = {rb[0], rb[1], rb[2], rb[3]}, v1 = {rb[4], rb[5], rb[6], rb[7]};
        *reinterpret_cast<f32x4*>(Bs + bc * LD + bg * 8) = v0;
        *reinterpret_cast<f32x4*>(Bs + bc * LD + bg * 8 + 4) = v1;
    };

    const int nk = (p_end - p_begin) / BK;
    load_step();
    store_step(0);
    if (nk > 1) load_step();
    __syncthreads();

    const int lrow = lane >> 5;
    const int lcol = lane & 31;
    const int a_rd = lcol * LD + lrow * (SP ? 4 : 8);
    const int b_rd = AROWS * LD + (wid * 32 + lcol) * LD + lrow * (SP ? 4 : 8);

    f32x16 acc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    float accx[XR > 0 ? XR : 1];
#pragma unroll
    for (int j = 0; j < (XR > 0 ? XR : 1); ++j) accx[j] = 0.f;
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const float* Tl = lds + cur * TILE;
        if (SP) {           // bf16x3: fragments are the pre-split LDS rows; refill behind the first TM MFMAs
            const bf16x8 bh = *reinterpret_cast<const bf16x8*>(Tl + b_rd);
            const bf16x8 bm = *reinterpret_cast<const bf16x8*>(Tl + b_rd + 8);
            const bf16x8 bl = *reinterpret_cast<const bf16x8*>(Tl + b_rd + 16);
            bf16x8 ah[TM], am[TM], al[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                al[i] = *reinterpret_cast<const bf16x8*>(Tl + a_rd + i * 32 * LD + 16);
                ah[i] = *reinterpret_cast<const bf16x8*>(Tl + a_rd + i * 32 * LD);
                am[i] = *reinterpret_cast<const bf16x8*>(Tl + a_rd + i * 32 * LD + 8);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i) OG_MFMA_BF(al[i], bh, acc[i]);
#pragma unroll
            for (int i = 0; i < TM; ++i) OG_MFMA_BF(ah[i], bl, acc[i]);
            __builtin_amdgcn_sched_barrier(0);
            if ((kt + 1) < nk) store_step(cur ^ 1);      // (splits the tile loaded one step ago: ~110 VALU)
            if ((kt + 2) < nk) load_step();
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < TM; ++i) OG_MFMA_BF(am[i], bm, acc[i]);
#pragma unroll
            for (int i = 0; i < TM; ++i) OG_MFMA_BF(am[i], bh, acc[i]);
#pragma unroll
            for (int i = 0; i < TM; ++i) OG_MFMA_BF(ah[i], bm, acc[i]);
#pragma unroll
            for (int i = 0; i < TM; ++i) OG_MFMA_BF(ah[i], bh, acc[i]);
        } else if (BF) {    // bf16 inputs (RNE of the fp32 tiles), one 32x32x16 MFMA per row group and K step
            if ((kt + 1) < nk) store_step(cur ^ 1);      // two-deep register -> LDS pipeline
            if ((kt + 2) < nk) load_step();
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(Tl + b_rd);
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(Tl + b_rd + 4);
            bf16x8 bq;
#pragma unroll
            for (int j = 0; j < 4; ++j) { bq[j] = (__bf16)b0[j]; bq[4 + j] = (__bf16)b1[j]; }
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const f32x4 x0 = *reinterpret_cast<const f32x4*>(Tl + a_rd + i * 32 * LD);
                const f32x4 x1 = *reinterpret_cast<const f32x4*>(Tl + a_rd + i * 32 * LD + 4);
                bf16x8 aq;
#pragma unroll
                for (int j = 0; j < 4; ++j) { aq[j] = (__bf16)x0[j]; aq[4 + j] = (__bf16)x1[j]; }
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq, bq, acc[i], 0, 0, 0);
            }
        } else {
            // fp32: the step's 8*TM MFMAs in two halves with the refill of the pipeline BETWEEN them --
            // LDS stores of the next tile, ~130 VALU instructions of gather addressing, 11 global loads.
            // Issue is in order: placed in front of the MFMAs (as the first version had it) that work
            // is exposed every step (98 TFLOP/s); behind the first half it runs in their shadow.
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(Tl + b_rd);
            f32x4 a0[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) a0[i] = *reinterpret_cast<const f32x4*>(Tl + a_rd + i * 32 * LD);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[i][kk], b0[kk], acc[i], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if ((kt + 1) < nk) store_step(cur ^ 1);      // two-deep register -> LDS pipeline
            if ((kt + 2) < nk) load_step();
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(Tl + b_rd + 4);
            f32x4 a1[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) a1[i] = *reinterpret_cast<const f32x4*>(Tl + a_rd + i * 32 * LD + 4);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[i][kk], b1[kk], acc[i], 0, 0, 0);
            if (XR > 0 && has_x) {
#pragma unroll
                for (int j = 0; j < XR; ++j) {
                    const f32x4 x0 = *reinterpret_cast<const f32x4*>(Tl + (BM + j) * LD + lrow * 8);
                    const f32x4 x1 = *reinterpret_cast<const f32x4*>(Tl + (BM + j) * LD + lrow * 8 + 4);
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) accx[j] = fmaf(x0[kk], b0[kk], accx[j]);
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) accx[j] = fmaf(x1[kk], b1[kk], accx[j]);
                }
            }
        }
        __syncthreads();
        cur ^= 1;
    }

    if (XR > 0 && has_x) {
#pragma unroll
        for (int j = 0; j < XR; ++j) accx[j] += __shfl_xor(accx[j], 32, 64);
    }
    const int ocol = c0 + wid * 32 + lcol;
    if (ocol >= a.ncol) return;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lrow;
            if (m < a.m_end) og_wgrad_store(a, m, ocol, acc[i][r], split);
        }
    }
    if (XR > 0 && has_x && lrow == 0) {
#pragma unroll
        for (int j = 0; j < XR; ++j)
            if (j < a.xr_count) og_wgrad_store_xr(a, j, ocol, accx[j], split);
    }
}

// Weight gradient on the v3 scheme: the gathered-x fragment goes straight to registers (lane =
// (column l & 31 of the wave, pixel half l >> 5)), dy rows through LDS (TM > 1) or direct (TM = 1).
// Requires OW % 8 == 0 and (OH*OW) % 16 == 0 like v2.
// B128: on the stride-1 interior fast path the eight consecutive pixels of a lane are fetched as two
// 16-byte loads (4-byte aligned) instead of eight dwords -- the lanes of a wave sit on different
// (channel, tap) planes, so every gather instruction touches ~20 cache lines.
template <int TM, int MATH = 0, bool B128 = false, int XR = 0, int NW = 4>
__global__ __launch_bounds__(64 * NW) void conv_wgrad3_kernel(const WgradArgs a, const int KS) {
    constexpr int NT = 64 * NW;                     // NW waves = NW 32-column groups sharing one dy row tile
    // MATH as in conv_igemm3_kernel.  SP (bf16x3): the dy rows are split by their loader thread on the way into
    // LDS (row image [h 16 | m 16 | l 16] bf16, 112-byte pitch), the gathered x fragment in registers; the gather
    // runs two steps ahead (three fragment sets), see conv_igemm3_kernel.
    // H2 (fp16x2, math 4): both operands scaled by their tensors' power-of-two scales, dy rows split into two fp16 pieces
    // on the way into LDS (row image [h 16 | l 16], 80-byte pitch), x in registers; three MFMAs per row group and step.
    constexpr bool BF = MATH == 1, SP = MATH == 2, H2 = MATH == 4, P3 = SP || H2;
    constexpr int BM = 32 * TM;
    constexpr int BN = 32 * NW;
    constexpr int BK = 16;
    constexpr int LD = SP ? 28 : BK + 4;
    constexpr int NA4 = BM * 4;
    constexpr int NA_PER = (NA4 + NT - 1) / NT;
    constexpr int TILE = (BM + XR) * LD;
    constexpr bool ALDS = TM > 1;
    static_assert(XR == 0 || (MATH == 0 && TM > 1), "extra rows: fp32 LDS form only");

    __shared__ __attribute__((aligned(16))) float lds[ALDS ? (P3 ? 3 : 2) * TILE : 4];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane >> 5;
    const int lcol = lane & 31;

    const int T = KS * KS;
    const int tiles_m = (a.m_end - a.m_begin + BM - 1) / BM;
    const int tiles_n = (a.ncol + BN - 1) / BN;
    // XCD placement over both grid dimensions: all tiles of a pixel split on one XCD (they read the same dy / x pixels),
    // an XCD takes a contiguous range of splits (see conv_wgrad_bfb_kernel)
    const int nwg = tiles_m * tiles_n;
    const int vid = og_xcd_remap(blockIdx.x + nwg * blockIdx.y, nwg * gridDim.y);
    const int split = vid / nwg;
    const int wg = vid - split * nwg;
    const int tile_m = wg % tiles_m;
    const int tile_n = wg / tiles_m;
    const int m0 = a.m_begin + tile_m * BM;
    const int c0 = tile_n * BN;

    const int OHW = a.OH * a.OW;
    const int HW = a.H * a.W;
    const int Npix = a.N * OHW;
    const int p_begin = split * a.pix_per_split;
    const int p_end = min(Npix, p_begin + a.pix_per_split);
    if (p_begin >= p_end) return;

    __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.x, 0, (int)((unsigned)a.N * a.Cin * HW * 4u), OG_BUF_FLAGS);
    __amdgpu_buffer_rsrc_t dyres = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.dy, 0, (int)((unsigned)a.N * a.Cout * OHW * 4u), OG_BUF_FLAGS);

    float h2_xs = 1.f, h2_dys = 1.f, h2_inv = 1.f;
    if (H2) {
        const int sx = og_h2_exponent(a.xmax, lane), sd = og_h2_exponent(a.dymax, lane);
        og_fp16_saturate();
        h2_xs = og_pow2(sx); h2_dys = og_pow2(sd); h2_inv = og_pow2_sum(-sx, -sd);
    }

    // ---- column of this lane
    const int col = c0 + wid * 32 + lcol;
    const bool col_ok = col < a.ncol;
    int dh, dw;
    unsigned ci_off;
    {
        const int cc = col_ok ? col : 0;
        const int ci = cc / T;
        const int t = cc - ci * T;
        const int kh = t / KS;
        dh = kh - a.pad;
        dw = (t - kh * KS) - a.pad;
        ci_off = (unsigned)ci * (unsigned)HW;
    }
    const int us = a.upsample ? 1 : 0;
    const bool refl = a.pad_mode == 1;

    // per-lane pixel state: the eight pixels (one output row) of this lane's k half in the next step
    int pn, poh, pow_;
    {
        const int p = p_begin + lrow * 8;
        pn = p / OHW;
        const int r = p - pn * OHW;
        poh = r / a.OW;
        pow_ = r - poh * a.OW;
    }
    auto load_b = [&](float (&rb)[8]) {
        const int ih = poh * a.stride + dh;
        int ihr = ih < 0 ? -ih : ih;
        ihr = ihr >= a.LH ? 2 * (a.LH - 1) - ihr : ihr;
        const bool row_ok = col_ok && (refl || (unsigned)ih < (unsigned)a.LH);
        const unsigned rbase = (unsigned)pn * (unsigned)a.Cin * (unsigned)HW + ci_off
                             + (unsigned)(((refl ? ihr : ih) >> us) * a.W);
        // Fast path (no upsampling; stride 1 or 2): when the eight taps of every lane of the wave are
        // interior -- or the whole row is padding -- they sit at a constant byte stride from the
        // first one, which folds into the instruction's immediate offset: no per-element address
        // arithmetic.  Spans touching the left / right border (2 of OW/8 per row) take the general path.
        const int iw0 = pow_ * a.stride + dw;
        const bool interior = iw0 >= 0 && iw0 + 7 * a.stride < a.LW;
        if (!us && (a.stride == 1 || a.stride == 2) && __all(interior || !row_ok)) {
            const unsigned vo = row_ok ? (rbase + (unsigned)iw0) * 4u : OG_OOB;
            if (B128 && a.stride == 1) {
                const f32x4 q0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xres, vo, 0, 0));
                const f32x4 q1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xres, vo + 16u, 0, 0));
#pragma unroll
                for (int i = 0; i < 4; ++i) { rb[i] = q0[i]; rb[4 + i] = q1[i]; }
            } else if (a.stride == 1) {
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    rb[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xres, vo + 4u * i, 0, 0));
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    rb[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xres, vo + 8u * i, 0, 0));
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int iw = (pow_ + i) * a.stride + dw;
                int iwr = iw < 0 ? -iw : iw;
                iwr = iwr >= a.LW ? 2 * (a.LW - 1) - iwr : iwr;
                const bool ok = row_ok && (refl || (unsigned)iw < (unsigned)a.LW);
                const unsigned vo = ok ? (rbase + (unsigned)((refl ? iwr : iw) >> us)) * 4u : OG_OOB;
                rb[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xres, vo, 0, 0));
            }
        }
        pow_ += BK;
        while (pow_ >= a.OW) { pow_ -= a.OW; poh += 1; }
        while (poh >= a.OH) { poh -= a.OH; pn += 1; }
    };

    // ---- dy rows
    unsigned avoff[NA_PER];
    int alds[NA_PER];
    if (ALDS) {
#pragma unroll
        for (int i = 0; i < NA_PER; ++i) {
            const int idx = tid + NT * i;
            const int row = idx >> 2, q = idx & 3;
            const bool on = (NA4 % NT == 0 || idx < NA4) && (m0 + row) < a.m_end;
            avoff[i] = on ? ((unsigned)(m0 + row) * (unsigned)OHW + q * 4u) * 4u : OG_OOB;
            alds[i] = (NA4 % NT == 0 || idx < NA4) ? row * LD + q * (P3 ? 2 : 4) : -1;
        }
    }
    const unsigned adir = (m0 + lcol) < a.m_end ? ((unsigned)(m0 + lcol) * (unsigned)OHW + lrow * 8u) * 4u : OG_OOB;
    int n_ld = p_begin / OHW;                        // scalar (image, offset) of the next dy step
    int rem_ld = p_begin - n_ld * OHW;
    auto a_soff = [&]() {
        const int so = (n_ld * a.Cout * OHW + rem_ld) * 4;
        rem_ld += BK;
        if (rem_ld >= OHW) { rem_ld = 0; n_ld += 1; }
        return so;
    };
    const bool has_x = XR > 0 && tile_m == 0 && a.xr_count > 0;
    const bool x_loader = has_x && tid < XR * 4;
    const unsigned xvoff = (x_loader && (tid >> 2) < a.xr_count)
        ? ((unsigned)(a.xr_begin + (tid >> 2)) * (unsigned)OHW + (tid & 3) * 4u) * 4u : OG_OOB;
    f32x4 ra[NA_PER];
    f32x4 rax = {0.f, 0.f, 0.f, 0.f};
    auto load_a = [&]() {
        const int so = a_soff();
#pragma unroll
        for (int i = 0; i < NA_PER; ++i)
            ra[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyres, avoff[i], so, 0));
        if (XR > 0 && has_x)
            rax = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyres, xvoff, so, 0));
    };
    auto store_a = [&](int buf) {
        float* As = lds + buf * TILE;
        if (H2) {
#pragma unroll
            for (int i = 0; i < NA_PER; ++i) {
                typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
                f16x4 h, l;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float sv = ra[i][j] * h2_dys;
                    h[j] = (_Float16)sv;
                    l[j] = (_Float16)og_sub(sv, (float)h[j]);
                }
                if (NA4 % NT == 0 || alds[i] >= 0) {
                    *reinterpret_cast<f16x4*>(As + alds[i]) = h;
                    *reinterpret_cast<f16x4*>(As + alds[i] + 8) = l;
                }
            }
            return;
        }
        if (SP) {
#pragma unroll
            for (int i = 0; i < NA_PER; ++i) {
                bf16x4 h, m, l;
                og_split4(ra[i], h, m, l);
                if (NA4 % NT == 0 || alds[i] >= 0) {
                    *reinterpret_cast<bf16x4*>(As + alds[i]) = h;
                    *reinterpret_cast<bf16x4*>(As + alds[i] + 8) = m;
                    *reinterpret_cast<bf16x4*>(As + alds[i] + 16) = l;
                }
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < NA_PER; ++i)
            if (NA4 % NT == 0 || alds[i] >= 0) *reinterpret_cast<f32x4*>(As + alds[i]) = ra[i];
        if (XR > 0 && x_loader) *reinterpret_cast<f32x4*>(As + (BM + (tid >> 2)) * LD + (tid & 3) * 4) = rax;
    };
    auto load_adir = [&](f32x4 (&ad)[2]) {
        const int so = a_soff();
        ad[0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyres, adir, so, 0));
        ad[1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyres, adir + 16u, so, 0));
    };

    f32x16 acc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const int a_rd = lcol * LD + lrow * (P3 ? 4 : 8);
    float accx[XR > 0 ? XR : 1];
#pragma unroll
    for (int j = 0; j < (XR > 0 ? XR : 1); ++j) accx[j] = 0.f;
    float rb0[8], rb1[8];
    f32x4 ad0[2], ad1[2];
    auto mma = [&](const float (&rb)[8], const f32x4 (&ad)[2], int cur, auto&& mid) {      // mid: see conv_igemm3_kernel
        if (BF || !ALDS) mid();
        if (H2) {                                       // order and pinning as SP
            f16x8 bh, bl;
            float sc[8];
            og_h2_split_h(rb, h2_xs, sc, bh);
            f16x8 ah[TM], al[TM];
            if (ALDS) {
                const float* Tl = lds + cur * TILE;
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    al[i] = *reinterpret_cast<const f16x8*>(Tl + a_rd + i * 32 * LD + 8);
                    ah[i] = *reinterpret_cast<const f16x8*>(Tl + a_rd + i * 32 * LD);
                }
            } else {
                const float d[8] = {ad[0][0], ad[0][1], ad[0][2], ad[0][3], ad[1][0], ad[1][1], ad[1][2], ad[1][3]};
                float dsc[8];
                og_h2_split_h(d, h2_dys, dsc, ah[0]);
                og_h2_split_l(dsc, ah[0], al[0]);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i) OG_MFMA_H(al[i], bh, acc[i]);
            if (ALDS) {
                __builtin_amdgcn_sched_barrier(0);
                mid();
                __builtin_amdgcn_sched_barrier(0);
            }
            og_h2_split_l(sc, bh, bl);
#pragma unroll
            for (int i = 0; i < TM; ++i) OG_MFMA_H(ah[i], bh, acc[i]);
            if (ALDS) og_interleave<TM, (16 + TM - 1) / TM>();
#pragma unroll
            for (int i = 0; i < TM; ++i) OG_MFMA_H(ah[i], bl, acc[i]);
            return;
        }
        if (SP) {                                       // order and pinning: see conv_igemm3_kernel
            bf16x8 bh, bm, bl;
            og_split8_h(rb, bh);
            bf16x8 ah[TM], am[TM], al[TM];
            if (ALDS) {
                const float* Tl = lds + cur * TILE;
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    al[i] = *reinterpret_cast<const bf16x8*>(Tl + a_rd + i * 32 * LD + 16);
                    am[i] = *reinterpret_cast<const bf16x8*>(Tl + a_rd + i * 32 * LD + 8);
                    ah[i] = *reinterpret_cast<const bf16x8*>(Tl + a_rd + i * 32 * LD);
                }
            } else {
                const float d[8] = {ad[0][0], ad[0][1], ad[0][2], ad[0][3], ad[1][0], ad[1][1], ad[1][2], ad[1][3]};
                og_split8(d, ah[0], am[0], al[0]);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i) OG_MFMA_BF(al[i], bh, acc[i]);
            if (ALDS) {
                __builtin_amdgcn_sched_barrier(0);
                mid();
                __builtin_amdgcn_sched_barrier(0);
            }
            og_split8_ml(rb, bh, bm, bl);
#pragma unroll
            for (int i = 0; i < TM; ++i) OG_MFMA_BF(am[i], bh, acc[i]);
#pragma unroll
            for (int i = 0; i < TM; ++i) OG_MFMA_BF(ah[i], bh, acc[i]);
            if (ALDS) og_interleave<2 * TM, (40 + 2 * TM - 1) / (2 * TM)>();
#pragma unroll
            for (int i = 0; i < TM; ++i) OG_MFMA_BF(am[i], bm, acc[i]);
#pragma unroll
            for (int i = 0; i < TM; ++i) OG_MFMA_BF(ah[i], bm, acc[i]);
#pragma unroll
            for (int i = 0; i < TM; ++i) OG_MFMA_BF(ah[i], bl, acc[i]);
            return;
        }
        if (BF) {
            bf16x8 bq;
#pragma unroll
            for (int j = 0; j < 8; ++j) bq[j] = (__bf16)rb[j];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                f32x4 x0, x1;
                if (ALDS) {
                    const float* Tl = lds + cur * TILE;
                    x0 = *reinterpret_cast<const f32x4*>(Tl + a_rd + i * 32 * LD);
                    x1 = *reinterpret_cast<const f32x4*>(Tl + a_rd + i * 32 * LD + 4);
                } else {
                    x0 = ad[0]; x1 = ad[1];
                }
                bf16x8 aq;
#pragma unroll
                for (int j = 0; j < 4; ++j) { aq[j] = (__bf16)x0[j]; aq[4 + j] = (__bf16)x1[j]; }
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq, bq, acc[i], 0, 0, 0);
            }
            return;
        }
        if (ALDS) {
            const float* Tl = lds + cur * TILE;
            f32x4 a0[TM], a1[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                a0[i] = *reinterpret_cast<const f32x4*>(Tl + a_rd + i * 32 * LD);
                a1[i] = *reinterpret_cast<const f32x4*>(Tl + a_rd + i * 32 * LD + 4);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[i][0], rb[0], acc[i], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            mid();
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 1; kk < 4; ++kk)
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[i][kk], rb[kk], acc[i], 0, 0, 0);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[i][kk], rb[4 + kk], acc[i], 0, 0, 0);
            if (XR > 0 && has_x) {
#pragma unroll
                for (int j = 0; j < XR; ++j) {
                    const f32x4 x0 = *reinterpret_cast<const f32x4*>(Tl + (BM + j) * LD + lrow * 8);
                    const f32x4 x1 = *reinterpret_cast<const f32x4*>(Tl + (BM + j) * LD + lrow * 8 + 4);
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) accx[j] = fmaf(x0[kk], rb[kk], accx[j]);
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) accx[j] = fmaf(x1[kk], rb[4 + kk], accx[j]);
                }
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ad[0][kk], rb[kk], acc[0], 0, 0, 0);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ad[1][kk], rb[4 + kk], acc[0], 0, 0, 0);
        }
    };

    const int nk = (p_end - p_begin) / BK;
    if (ALDS) {
        load_a();
        store_a(0);
        if (P3 || nk > 1) load_a();
    } else {
        load_adir(ad0);
    }
    load_b(rb0);
    if (P3 && ALDS) load_b(rb1);
    if (ALDS) __syncthreads();
    int cur = 0;
    int kt = 0;                                       // two steps per trip, see conv_igemm3_kernel
    if (P3 && ALDS) {               // three fragment sets / three LDS tiles, gather two steps ahead (conv_igemm3_kernel)
        float rb2[8];
        int ks = 0;
        if (ks + 2 < nk) {
            do {
                mma(rb0, ad0, 0, [&]() { store_a(1); load_a(); load_b(rb2); });
                __syncthreads();
                mma(rb1, ad0, 1, [&]() { store_a(2); load_a(); load_b(rb0); });
                __syncthreads();
                mma(rb2, ad0, 2, [&]() { store_a(0); load_a(); load_b(rb1); });
                __syncthreads();
                ks += 3;
            } while (ks + 2 < nk);
        }
        if (ks < nk) {
            mma(rb0, ad0, 0, [&]() { store_a(1); });
            __syncthreads();
        }
        if (ks + 1 < nk) mma(rb1, ad0, 1, [] {});
        kt = nk;
    }
    for (; kt + 1 < nk; kt += 2) {
        mma(rb0, ad0, cur, [&]() {
            if (ALDS) store_a(cur ^ 1); else load_adir(ad1);
            load_b(rb1);
            if (ALDS && kt + 2 < nk) load_a();
        });
        if (ALDS) __syncthreads();
        cur ^= 1;
        mma(rb1, ad1, cur, [&]() {
            if (kt + 2 < nk) {
                if (ALDS) store_a(cur ^ 1); else load_adir(ad0);
                load_b(rb0);
            }
            if (ALDS && kt + 3 < nk) load_a();
        });
        if (ALDS) __syncthreads();
        cur ^= 1;
    }
    if (kt < nk) mma(rb0, ad0, cur, [] {});

    if (XR > 0 && has_x) {
#pragma unroll
        for (int j = 0; j < XR; ++j) accx[j] += __shfl_xor(accx[j], 32, 64);
    }
    if (!col_ok) return;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lrow;
            if (m < a.m_end) og_wgrad_store(a, m, col, H2 ? acc[i][r] * h2_inv : acc[i][r], split);
        }
    }
    if (XR > 0 && has_x && lrow == 0) {
#pragma unroll
        for (int j = 0; j < XR; ++j)
            if (j < a.xr_count) og_wgrad_store_xr(a, j, col, accx[j], split);
    }
}

// ---- weight gradient of the bf16 mode: bf16 operands, x read from its channel-blocked copy -----------------------------
// dW[m][c][t] = sum over output pixels p = (n, oh, ow) of dy[n][m][p] * x[n][c][p @ tap t]: GEMM rows = output channels,
// K = pixels, columns = (tap, channel).  Both MFMA operands want eight consecutive K = pixels per lane; x arrives
// pixel-major -- its channel-blocked bf16 copy [N][Cp/16][H*W][16] (nchw_to_nhwc_bf16_kernel) holds 16 channels of a pixel
// as one 32-byte record -- so a wave copies the records of its 32 pixels x 32 channels (ONE tap, two chunks) into a
// wave-private LDS image [32 pixels][2 chunks][16 channels] (lane-linear 16-byte stores) and reads them back with
// ds_read_b64_tr_b16, the gfx950 transposing LDS read: lane (i = l & 15 of a 16-lane group) passes the address of row
// i >> 2, columns 4 (i & 3) .. +3 and receives column i of the 4 x 16 block -- four consecutive PIXELS of one channel.
// Two such reads are the lane's operand of one 32x32x16 MFMA (measured on the box: tools/tr_probe.hip).  No fp32
// gathers, no conversions of x, every geometry (zero / reflect padding, stride, nearest-x2 upsampling) is just the
// record address of the lane's pixel; records are 32 bytes, so every load is 16-byte aligned whatever the tap shift.
// dy rows: a bf16 copy of dy in its own NCHW layout (f32_to_bf16_kernel; pixels are already contiguous there), staged
// into LDS as 16-byte pieces (80-byte pitch: conflict-free ds_read_b128), shared by the NW waves of the workgroup --
// NW column groups (tap, 32 channels) per row tile.  (The first version read fp32 dy and rounded it on the way into
// LDS: the kernel runs against the L2 -> L1 fill rate -- 40 KB per workgroup and iteration at 353 TFLOP/s = 4.5 TB/s --
// and the fp32 rows were 24 of those 40 KB.)
// One iteration = 32 pixels = two MFMAs per row group.  Requires (OH * OW) % 32 == 0 and OH, OW <= 256.
// The record address of a lane's pixel costs VALU work every iteration (K = pixels: nothing is constant across the
// loop): the tap geometry -- stride, padding, reflection, upsampling, bounds -- sits in two small LDS tables per
// workgroup (source row offset per (kh, oh), source column per (kw, ow); 0xffff = outside), so an address is two
// 16-bit LDS reads and ~8 VALU instructions; the first version evaluated the geometry per record (~108 VALU per wave and
// iteration next to 12 MFMAs: VALU bound, 344 TFLOP/s).
template <int TM, int NW>
__global__ __launch_bounds__(64 * NW) void conv_wgrad_bfb_kernel(const WgradArgs a, const __bf16* __restrict__ xb,
                                                                 const __bf16* __restrict__ dyb, const int KS, const int Cp) {
    constexpr int NT = 64 * NW;
    constexpr int BM = 32 * TM;
    constexpr int BK = 32;
    constexpr int ALD = 20;                          // floats per dy row in LDS: 64 bytes of bf16 + 16 (odd multiple of 16)
    constexpr int ATILE = BM * ALD;
    constexpr int NA4 = BM * 4;                      // 16-byte bf16 pieces (8 pixels) of a row tile per iteration
    constexpr int NA_PER = (NA4 + NT - 1) / NT;
    constexpr int BTILE = 512;                       // floats: 32 pixels x 64 bytes per wave (wave-private, ONE buffer:
                                                     // a wave's LDS instructions execute in order, the store of the next
                                                     // image is issued behind the last transposing read of this one)
    constexpr int TAB = 256;                         // table pitch: OH, OW <= 256
    static_assert((2 * ATILE + NW * BTILE) * 4 + 2 * 4 * TAB * 2 <= 64 * 1024, "LDS");
    __shared__ __attribute__((aligned(16))) float ldsA[2 * ATILE];
    __shared__ __attribute__((aligned(16))) float ldsB[NW * BTILE];
    __shared__ unsigned short rtab[4 * TAB], ctab[4 * TAB];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lrow = lane >> 5;
    const int lcol = lane & 31;

    const int T = KS * KS;
    const int Cc = Cp >> 4;                          // 16-channel chunks
    const int CG = (Cc + 1) >> 1;                    // 32-channel column groups per tap
    const int ngroups = T * CG;
    const int tiles_m = (a.m_end - a.m_begin + BM - 1) / BM;
    const int tiles_n = (ngroups + NW - 1) / NW;
    // XCD placement over BOTH grid dimensions: the workgroups of one pixel split read the same dy / x records (every
    // (tap, channel group) walks the same pixels), so all tiles of a split go to ONE XCD -- one L2 -- and an XCD takes
    // a contiguous range of splits.  (With the remap over blockIdx.x alone the tiles of a split were spread over the
    // eight L2s: 39 % L2 misses, 2.2 GB from HBM / MALL per launch on objd_l3, profiles/r03_bf16_pmc_objd_l3.txt.)
    const int nwg = tiles_m * tiles_n;                // = gridDim.x
    const int vid = og_xcd_remap(blockIdx.x + nwg * blockIdx.y, nwg * gridDim.y);
    const int split = vid / nwg;
    const int wg = vid - split * nwg;
    const int tile_m = wg % tiles_m;
    const int tile_n = wg / tiles_m;
    const int m0 = a.m_begin + tile_m * BM;
    const int group = tile_n * NW + wid;
    const bool grp_ok = group < ngroups;
    const int t = grp_ok ? group / CG : 0;
    const int cg = grp_ok ? group - t * CG : 0;
    const int kh = t / KS;
    const int dh = kh - a.pad, dw = (t - kh * KS) - a.pad;

    const int OHW = a.OH * a.OW;
    const int HW = a.H * a.W;
    const int Npix = a.N * OHW;
    const int p_begin = split * a.pix_per_split;
    const int p_end = min(Npix, p_begin + a.pix_per_split);
    const int nk = (p_end - p_begin + BK - 1) / BK;

    __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc(
        (void*)xb, 0, (int)((unsigned)a.N * (unsigned)Cc * (unsigned)HW * 32u), OG_BUF_FLAGS);
    __amdgpu_buffer_rsrc_t dyres = __builtin_amdgcn_make_buffer_rsrc(
        (void*)dyb, 0, (int)((unsigned)a.N * a.Cout * OHW * 2u), OG_BUF_FLAGS);

    // ---- x records: lane = (pixel j = l >> 2 of a 16-pixel half, chunk (l >> 1) & 1, 16-byte half l & 1)
    const int chunk = cg * 2 + ((lane >> 1) & 1);
    const bool rec_ok = grp_ok && chunk < Cc;
    const unsigned rec_lane = (unsigned)chunk * (unsigned)HW;     // + n * Cc * HW + ih * W + iw, x 32 bytes + half
    const int us = a.upsample ? 1 : 0;
    const bool refl = a.pad_mode == 1;
    for (int i = tid; i < KS * (a.OH + a.OW); i += NT) {             // tap geometry tables (see the header comment)
        const bool is_row = i < KS * a.OH;
        const int e = is_row ? i : i - KS * a.OH;
        const int L = is_row ? a.OH : a.OW, LL = is_row ? a.LH : a.LW;
        const int kk = e / L, o = e - kk * L;
        const int iv = o * a.stride + kk - a.pad;
        int ivr = iv < 0 ? -iv : iv;
        ivr = ivr >= LL ? 2 * (LL - 1) - ivr : ivr;
        const bool ok = refl || ((unsigned)iv < (unsigned)LL);
        const int src = (refl ? ivr : iv) >> us;
        const unsigned short v = ok ? (unsigned short)(is_row ? src * a.W : src) : (unsigned short)0xffffu;
        if (is_row) rtab[kk * TAB + o] = v; else ctab[kk * TAB + o] = v;
    }
    const unsigned short* rt = rtab + kh * TAB;
    const unsigned short* ct = ctab + (t - kh * KS) * TAB;
    // pixel steps without divisions in the loop: 16 and 32 pixels = (rows, columns) of the output map
    const int rows16 = 16 / a.OW, cols16 = 16 - rows16 * a.OW;
    const int rows32 = 32 / a.OW, cols32 = 32 - rows32 * a.OW;
    int pn, poh, pow_;                               // output pixel of this lane in the first half of the next iteration
    {
        const int p = p_begin + (lane >> 2);
        pn = p / OHW;
        const int r = p - pn * OHW;
        poh = r / a.OW;
        pow_ = r - poh * a.OW;
    }
    int p_ld = p_begin + (lane >> 2);                // pixel index of (pn, poh, pow_)
    const unsigned half16 = (unsigned)((lane & 1) * 16);
    auto load_b = [&](f32x4 (&rb)[2]) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int n = pn, oh = poh, ow = pow_;
            if (h == 1) {                            // second half: 16 pixels further
                ow += cols16;
                const int c = ow >= a.OW ? 1 : 0;
                ow -= c ? a.OW : 0;
                oh += rows16 + c;
                while (oh >= a.OH) { oh -= a.OH; n += 1; }
            }
            const unsigned r = rt[oh], c = ct[ow];
            const bool ok = rec_ok && (p_ld + 16 * h < p_end) && r != 0xffffu && c != 0xffffu;
            const unsigned off = ok ? ((unsigned)n * (unsigned)Cc * (unsigned)HW + rec_lane + r + c) * 32u + half16 : OG_OOB;
            rb[h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xres, off, 0, 0));
        }
        p_ld += BK;
        pow_ += cols32;
        const int c = pow_ >= a.OW ? 1 : 0;
        pow_ -= c ? a.OW : 0;
        poh += rows32 + c;
        while (poh >= a.OH) { poh -= a.OH; pn += 1; }
    };
    auto store_b = [&](const f32x4 (&rb)[2]) {
        float* Bs = ldsB + wid * BTILE;
#pragma unroll
        for (int h = 0; h < 2; ++h) *reinterpret_cast<f32x4*>(Bs + h * 256 + lane * 4) = rb[h];
    };
    // transposing read: 16-lane group g = l >> 4: chunk g & 1, pixel half-octet g >> 1; see the header comment
    const int b_rd = ((lane >> 5) * 8 + ((lane & 15) >> 2)) * 64 + ((lane >> 4) & 1) * 32 + (lane & 3) * 8;   // bytes

    // ---- dy rows
    unsigned avoff[NA_PER];
    int alds[NA_PER];
#pragma unroll
    for (int i = 0; i < NA_PER; ++i) {
        const int idx = tid + NT * i;
        const int row = idx >> 2, q = idx & 3;
        const bool on = (NA4 % NT == 0 || idx < NA4) && (m0 + row) < a.m_end;
        avoff[i] = on ? ((unsigned)(m0 + row) * (unsigned)OHW + q * 8u) * 2u : OG_OOB;
        alds[i] = (NA4 % NT == 0 || idx < NA4) ? row * ALD + q * 4 : -1;
    }
    int n_ld = p_begin / OHW;                        // scalar (image, offset) of the next dy iteration
    int rem_ld = p_begin - n_ld * OHW;
    f32x4 ra[NA_PER];
    auto load_a = [&]() {
        const int so = (n_ld * a.Cout * OHW + rem_ld) * 2;
        rem_ld += BK;
        if (rem_ld >= OHW) { rem_ld = 0; n_ld += 1; }
#pragma unroll
        for (int i = 0; i < NA_PER; ++i)
            ra[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dyres, avoff[i], so, 0));
    };
    auto store_a = [&](int buf) {
        float* As = ldsA + buf * ATILE;
#pragma unroll
        for (int i = 0; i < NA_PER; ++i)
            if (NA4 % NT == 0 || alds[i] >= 0) *reinterpret_cast<f32x4*>(As + alds[i]) = ra[i];
    };

    f32x16 acc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    typedef __attribute__((__vector_size__(4 * sizeof(short)))) short s16x4;
    auto mma = [&](int buf, auto&& mid) {
        const char* Bs = reinterpret_cast<const char*>(ldsB + wid * BTILE) + b_rd;
        const float* As = ldsA + buf * ATILE + lcol * ALD + lrow * 4;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const s16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (s16x4 __attribute__((address_space(3)))*)(Bs + h * 1024));
            const s16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (s16x4 __attribute__((address_space(3)))*)(Bs + h * 1024 + 256));
            // (whole-vector casts: an element-wise short -> bf16 copy of the two halves came out of hipcc as
            // {b0.lo, b0.lo, b1.lo, b1.lo} -- found with tools/dbg_wgrad.py)
            const bf16x8 bq = __builtin_bit_cast(bf16x8, __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
            bf16x8 aq[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                aq[i] = *reinterpret_cast<const bf16x8*>(As + i * 32 * ALD + h * 8);
            if (h == 1) {                 // the refill behind the first TM MFMAs of the iteration
                __builtin_amdgcn_sched_barrier(0);
                mid();
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq[i], bq, acc[i], 0, 0, 0);
        }
    };

    // prologue: iteration 0 in LDS buffer 0, iteration 1 in registers
    f32x4 rb[2];
    __syncthreads();                                  // tables
    load_a(); load_b(rb);
    store_a(0); store_b(rb);
    load_a(); load_b(rb);
    __syncthreads();
    // two iterations per trip (literal buffer indices); the loads of iteration k + 2 are issued in iteration k and stored to
    // LDS in iteration k + 1 (unconditionally: past the end they hit the range check or unused records)
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
        mma(0, [&]() { store_a(1); store_b(rb); load_a(); load_b(rb); });
        __syncthreads();
        mma(1, [&]() { store_a(0); store_b(rb); load_a(); load_b(rb); });
        __syncthreads();
    }
    if (kt < nk) mma(0, [] {});

    // ---- epilogue: column = channel ci of tap t -> dw[m][ci * T + t]
    const int ci = cg * 32 + lcol;
    if (!grp_ok || ci >= a.Cin) return;
    const int ocol = ci * T + t;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lrow;
            if (m < a.m_end) {
                if (a.ws) a.ws[(size_t)split * a.ws_stride + (size_t)(m - a.m_begin) * a.ncol + ocol] = acc[i][r];
                else og_wgrad_store(a, m, ocol, acc[i][r], split);  // one split
            }
        }
    }
}

int og_launch_wgrad_combine(const WgradArgs& a, int splits, hipStream_t s) {
    const long slot = a.ws_stride;
    const bool v4 = !((size_t)a.ws & 15) && !(slot & 3) && slot >= 4 && slot < (1L << 31);
    if (v4)
        hipLaunchKernelGGL(wgrad_combine_kernel<true>, dim3(og_stream_grid(slot >> 2, 256)), dim3(256), 0, s, a.ws, splits,
                           slot, a.dw, a.ncol, a.m_begin, a.m_end - a.m_begin, a.xr_begin, slot, a.accumulate);
    else
        hipLaunchKernelGGL(wgrad_combine_kernel<false>, dim3(og_stream_grid(slot, 256)), dim3(256), 0, s, a.ws, splits,
                           slot, a.dw, a.ncol, a.m_begin, a.m_end - a.m_begin, a.xr_begin, slot, a.accumulate);
    return og_launch_status();
}

// ---- geometry predicates (each condition once: the plan and the *_ok entry points ask these) ---------------------
// The buffer-descriptor kernels (v2): OW % 8 == 0 and (OH*OW) % 16 == 0, so that the eight pixels a thread gathers lie
// in one output row and a K step lies in one image; both tensors within the 32-bit buffer range.
static bool og_wgrad_v2_geometry(int N, int Cin, int H, int W, int Cout, int OH, int OW) {
    const long OHW = (long)OH * OW;
    return !og_igemm_v1() && (OW % 8 == 0) && (OHW % 16 == 0)
           && (double)N * Cin * H * W * 4.0 < 4.0e9 && (double)N * Cout * OHW * 4.0 < 4.0e9;
}
// conv_wgrad_bfb_kernel / conv_wgrad_rec*_kernel: iterations of 32 pixels, 16-bit tap tables of 256 entries, and the
// copy of x they read (`bytes` per element, channels padded to 16) within the buffer range
static bool og_wgrad_table_geometry(int N, int Cin, int H, int W, int Cout, int OH, int OW, int ksize, double bytes) {
    const long OHW = (long)OH * OW;
    const long Cp = ((long)Cin + 15) / 16 * 16;
    return og_wgrad_v2_geometry(N, Cin, H, W, Cout, OH, OW) && OHW % 32 == 0 && OH <= 256 && OW <= 256
           && (long)(H - 1) * W < 65535 && (ksize == 1 || ksize == 3 || ksize == 4) && (double)N * Cp * H * W * bytes < 4.0e9;
}
// the bf16 copy (math 1 / 3) and the fp16 record (math 5 / 6 / 7: two pieces) of x
static bool og_wgrad_bfb_geometry(int N, int Cin, int H, int W, int Cout, int OH, int OW, int ksize) {
    return og_wgrad_table_geometry(N, Cin, H, W, Cout, OH, OW, ksize, 2.0);
}
static bool og_wgrad_rec_geometry(int N, int Cin, int H, int W, int Cout, int OH, int OW, int ksize) {
    return og_wgrad_table_geometry(N, Cin, H, W, Cout, OH, OW, ksize, 4.0);
}

// The launch plan of the weight gradient: a pure function of the geometry, the arithmetic and `have_ws` -- whether the
// run gets a workspace.  The size query plans WITH one; a run without falls back from conv_wgrad_bfb_kernel to the
// fp32-gather kernels (and fails if it then still needs slots).
//   math 3: math 1 with x handed over AS its bf16 channel-blocked copy (objgan_nhwc_bf16; usually the one the forward
//           call of the layer read): only the bf16 copy of dy is made.  objgan_conv_wgrad_bfb_ok says where.
//   math 5: x is the fp16 record of the source (conv_igemm_rec.hip), dy the fp32 tensor.  The caller asks
//           objgan_conv_wgrad_rec_ok first; a geometry the record kernel does not take is an argument error.
//   math 6: the same with dy pre-split too: its fp16 pair is written into the workspace by one pass (h2_pair_kernel).
//   math 7: the record form with TWO column groups per wave (conv_wgrad_rec2_kernel: block rows <= 128 rows, 8-wave
//           workgroups); launches of fewer than 16 384 pixels keep the one-group kernel.
static WgradPlan og_wgrad_plan(int N, int Cin, int H, int W, int upsample, int pad_mode, int Cout, int OH, int OW,
                               int ksize, int stride, int math, bool have_ws) {
    WgradPlan p;
    memset(&p, 0, sizeof(p));
    p.rc = OG_BAD_ARGS;
    if (ksize != 1 && ksize != 3 && ksize != 4) return p;
    if (math < 0 || math > 7) return p;
    p.x_copy_in = math == 3;
    if (p.x_copy_in) math = 1;
    if (N <= 0 || Cout <= 0 || Cin <= 0) { p.rc = 2; return p; }
    p.rec = math == 5 || math == 6 || math == 7;
    p.dyp = math == 6;
    p.rec2 = math == 7 && (long)N * OH * OW >= 16384;
    if (p.rec && !og_wgrad_rec_geometry(N, Cin, H, W, Cout, OH, OW, ksize)) return p;
    // fp16x2 lives in the register-fragment kernel; launches that plan the LDS-staged / first-generation kernels run
    // bf16x3 (both are fp32-result arithmetics)
    p.h2 = math == 4;
    if (p.h2 || p.rec) math = 2;
    p.kmath = math;
    const int Npix = N * OH * OW, OHW = OH * OW;
    const int ncol = Cin * ksize * ksize;
    p.v2 = og_wgrad_v2_geometry(N, Cin, H, W, Cout, OH, OW);
    if (p.x_copy_in && !p.v2) return p;
    // splits -> whole K steps per split, the slot of a split and where the part's slots start
    const auto place = [&](WgradPart& q, int splits, int step) {
        const int pps = (og_cdiv(Npix, splits) + step - 1) / step * step;
        q.pix_per_split = pps;
        q.splits = og_cdiv(Npix, pps);
        q.slot = (long)(q.m_end - q.m_begin + q.xr_count) * ncol;
        q.ws_off = p.total;
        if (q.splits > 1) p.total += q.slot * q.splits;
    };
    if (!p.v2) {
        RowPart parts[3];
        p.nparts = og_row_parts(Cout, parts);
        for (int i = 0; i < p.nparts; ++i) {
            WgradPart& q = p.part[i];
            q.m_begin = parts[i].m_begin; q.m_end = parts[i].m_end; q.cfg = parts[i].cfg; q.nw = 4;
            q.rows = og_cdiv(q.m_end - q.m_begin, q.cfg == 0 ? 128 : (q.cfg == 1 ? 64 : 32));
            q.tiles_n = og_cdiv(ncol, q.cfg == 0 ? 128 : 256);
            // split K (pixels) so that the grid covers the 256 CUs a few times over
            int splits = og_cdiv(256 * 4, q.rows * q.tiles_n);
            const int max_splits = og_cdiv(Npix, 256);   // >= 8 K steps per split
            if (splits > max_splits) splits = max_splits;
            if (splits < 1) splits = 1;
            place(q, splits, 32);
        }
        p.rc = OG_OK;
        return p;
    }
    const bool bf = math == 1, sp = math == 2;
    // bf16 mode: bf16 operands, x from its channel-blocked copy in the workspace (conv_wgrad_bfb_kernel); without a
    // workspace (or on maps of fewer than 32 pixels) the fp32-gather kernels below
    p.Cpb = (Cin + 15) / 16 * 16;
    p.bfb = bf && have_ws && og_wgrad_bfb_geometry(N, Cin, H, W, Cout, OH, OW, ksize);
    if (p.x_copy_in && !p.bfb) return p;
    p.xb_floats = (p.bfb && !p.x_copy_in) ? og_nhwc_bf16_floats(N, H, W, p.Cpb) : 0;
    p.dyb_floats = p.bfb ? (((long)N * Cout * OHW / 2 + 3) & ~3L) : 0;       // (OHW % 32 == 0: a multiple of 4)
    p.dyp_floats = p.dyp ? (((long)N * Cout * OHW + 3) & ~3L) : 0;           // the fp16 pair of dy
    p.total = p.xb_floats + p.dyb_floats + p.dyp_floats;
    int groups = og_cdiv(Cout, 32);
    const int tiles_n0 = og_cdiv(ncol, 128);
    // 1..4 output channels beyond a multiple of 32: on the VALU of block row 0 (see WgradArgs)
    const int tail_rows = Cout & 31;
    p.xrows = !og_no_xrows() && math == 0 && tail_rows >= 1 && tail_rows <= 4 && Cout >= 64;
    int TM, full_rows, rest;
    if (p.xrows) {
        og_row_plan(groups - 1, tiles_n0, 1, &TM, &full_rows, &rest);
        if (TM >= 2 && full_rows >= 1) groups -= 1; else p.xrows = 0;
    }
    og_row_plan(groups, tiles_n0, 1, &TM, &full_rows, &rest, 100, p.rec2 ? 4 : (p.rec ? og_wgrad_rec_tmmax() : 7));      // (tall tiles: independent of the column tiling)
    p.xr_begin = groups * 32;
    const int m_cap = p.xrows ? groups * 32 : Cout;
    for (int part = 0; part < 2; ++part) {
        const int tm = part == 0 ? TM : rest;
        const int rows = part == 0 ? full_rows : (rest ? 1 : 0);
        if (rows == 0) continue;
        WgradPart& q = p.part[p.nparts++];
        q.tm = tm; q.rows = rows;
        q.m_begin = part == 0 ? 0 : full_rows * TM * 32;
        q.m_end = part == 0 ? (m_cap < full_rows * TM * 32 ? m_cap : full_rows * TM * 32) : m_cap;
        q.xr_count = (part == 0 && p.xrows) ? tail_rows : 0;
        // Which form, and how many waves per workgroup (the column-tile count of the launch depends on it).  The
        // register-fragment kernel (wgrad3) takes the short tiles, and with 16-byte gathers the wide stride-1 maps
        // without upsampling (r02 A/B: res1_128 100 -> 107 TF, shp_512 33 -> 37); the LDS-staged kernel (wgrad2) the
        // rest: narrow maps spend half of their spans on the border path, the up-sampling / reflecting gathers keep
        // their per-element address math.
        const bool wide_s1 = stride == 1 && !upsample && OW >= 64;
        q.b128 = wide_s1 && !og_wgrad_nob128() && !bf;
        // (bf16x3: the LDS-staged form is instruction-issue bound -- 8 VALU per MFMA for per-element gather addresses
        // plus the split of both operands, profiles/r03_x3_pmc_objd_l3.txt -- so the register-fragment form also
        // takes the tall tiles wherever its constant-stride gather path applies: zero padding, no upsampling;
        // r03 A/B: objd_l2 / objd_l3 155 -> 170 TFLOP/s, upsampled sources 119 -> 109)
        const bool x3_frag = tm <= og_x3_wgrad3_maxtm() || q.b128 || (!upsample && !pad_mode && og_x3_wgrad3_maxtm() >= 0);
        q.use3 = bf ? tm <= 2 : (sp ? x3_frag : (tm <= og_wgrad3_maxtm() || q.b128));
        // bf16x3, register-fragment form: 8-wave workgroups (256 columns per dy row tile), as in run_igemm2
        q.nw = p.bfb ? ((tm <= 6 && Npix >= 16384) ? 8 : 4)
                     : (p.rec2 ? 8 : p.rec ? ((tm <= 6 && Npix >= 16384 && og_wgrad_rec_nw8()) ? 8 : 4)
                              : ((sp && q.use3 && tm >= 4 && og_nw8_min() > 0 && Npix >= 16384) ? 8 : 4));
        // column tiles: 32 columns (ci * T + t) per wave; bfb / rec: one (tap, 32-channel group) per wave
        q.tiles_n = (p.bfb || p.rec) ? og_cdiv(ksize * ksize * og_cdiv(p.Cpb, 32), p.rec2 ? 2 * q.nw : q.nw)
                                     : og_cdiv(ncol, 32 * q.nw);
        // split K (pixels): the launch takes about (workgroups per CU, rounded up) x (K steps per split + a fixed
        // prologue / epilogue cost); pick the split count that minimises it (r02: `slots / workgroups` left the
        // 288-workgroup launches of the 16x16 maps at 1 split -- 32 CUs with two workgroups, 224 with one -- 63 TFLOP/s)
        const int max_splits = og_cdiv(Npix, 512);       // >= 32 K steps per split
        const long wgs = (long)rows * q.tiles_n;
        const int nsteps = og_cdiv(Npix, 16);
        const int resident = q.nw == 8 ? 1 : (tm == 1 ? 6 : (tm <= 4 ? 3 : 2));
        double best = -1;
        int splits = 1;
        for (int k = 1; k <= max_splits && k <= 1024; ++k) {
            const long per_cu = og_cdiv(wgs * k, 256);
            // fewer co-resident workgroups than the CU can hold: nothing hides the memory latency
            const double lat = per_cu < resident ? 1.0 + 0.15 * (resident - per_cu) : 1.0;
            const double cost = (double)per_cu * (og_cdiv(nsteps, k) + 10.0) * lat;
            if (best < 0 || cost < best * 0.985) { best = cost; splits = k; }
        }
        place(q, splits, (p.bfb || p.rec) ? 32 : 16);
    }
    p.rc = OG_OK;
    return p;
}

template <int TM, int MATH, bool B128, int XR, int NW>
static inline void wg3(const WgradArgs& a, dim3 grid, int ksize, hipStream_t s) {
    hipLaunchKernelGGL((conv_wgrad3_kernel<TM, MATH, B128, XR, NW>), grid, dim3(64 * NW), 0, s, a, ksize);
}
template <int TM, int MATH, int XR>
static inline void wg2(const WgradArgs& a, dim3 grid, int ksize, hipStream_t s) {
    hipLaunchKernelGGL((conv_wgrad2_kernel<TM, MATH, XR>), grid, dim3(256), 0, s, a, ksize);
}

// One part of a v2 plan on the kernels of this file.
static void launch_wgrad2(const WgradArgs& a, const WgradPlan& p, const WgradPart& q, const __bf16* xb, const __bf16* dyb,
                          dim3 grid, int ksize, hipStream_t s) {
    const bool bf = a.math == 1, sp = a.math == 2, b128 = q.b128 != 0, use3 = q.use3 != 0;
    const int nw = q.nw;
    if (p.bfb) {
        og_with_tm<1, 7>(q.tm, [&](auto tmc) {
            constexpr int T = decltype(tmc)::value;
            constexpr int T8 = T <= 6 ? T : 6;          // 8 waves: the LDS of a 7-group row tile does not fit
            if (nw == 8) hipLaunchKernelGGL((conv_wgrad_bfb_kernel<T8, 8>), grid, dim3(512), 0, s, a, xb, dyb, ksize, p.Cpb);
            else hipLaunchKernelGGL((conv_wgrad_bfb_kernel<T, 4>), grid, dim3(256), 0, s, a, xb, dyb, ksize, p.Cpb);
        });
    } else if (a.xr_count > 0) {
        // extra rows on the VALU: fp32 only, LDS forms only (the plan grants them from TM = 2 on); XR = 4 rows
        og_with_tm<2, 7>(q.tm, [&](auto tmc) {
            constexpr int T = decltype(tmc)::value;
            if (use3 && b128) wg3<T, 0, true, 4, 4>(a, grid, ksize, s);
            else if (use3) wg3<T, 0, false, 4, 4>(a, grid, ksize, s);
            else wg2<T, 0, 4>(a, grid, ksize, s);
        });
    } else {
        og_with_tm<1, 7>(q.tm, [&](auto tmc) {
            constexpr int T = decltype(tmc)::value;
            constexpr int T8 = T > 1 ? T : 2;           // 8 waves: no LDS-free form, TM = 1 runs the 2-group instance
            const auto frag = [&](auto mc) {            // register-fragment form of the split arithmetics
                constexpr int MATH = decltype(mc)::value;
                if (nw == 8 && b128) wg3<T8, MATH, true, 0, 8>(a, grid, ksize, s);
                else if (nw == 8) wg3<T8, MATH, false, 0, 8>(a, grid, ksize, s);
                else if (b128) wg3<T, MATH, true, 0, 4>(a, grid, ksize, s);
                else wg3<T, MATH, false, 0, 4>(a, grid, ksize, s);
            };
            if (bf && T <= 2) wg3<T, 1, false, 0, 4>(a, grid, ksize, s);
            else if (bf) wg2<T, 1, 0>(a, grid, ksize, s);
            else if (sp && use3 && p.h2) frag(OgInt<4>{});
            else if (sp && use3) frag(OgInt<2>{});
            else if (sp) wg2<T, 2, 0>(a, grid, ksize, s);
            else if (use3 && b128) wg3<T, 0, true, 0, 4>(a, grid, ksize, s);
            else if (use3) wg3<T, 0, false, 0, 4>(a, grid, ksize, s);
            else wg2<T, 0, 0>(a, grid, ksize, s);
        });
    }
}

extern "C" {

// dw [Cout][Cin][k][k] = (accumulate ? dw : 0) + sum dy * x.  ws: objgan_conv_wgrad_ws_floats(...) floats of scratch.
// Checks the arguments against the plan, makes the operand copies and walks the parts.
int objgan_conv_wgrad(const float* x, const float* dy, float* dw,
                      int N, int Cin, int H, int W, int upsample, int pad_mode,
                      int Cout, int OH, int OW, int ksize, int stride, int pad,
                      int math, int accumulate, const float* xmax, const float* dymax, float* ws, long ws_floats,
                      void* stream) {
    OG_ENTRY();
    hipStream_t s = (hipStream_t)stream;
    const WgradPlan p = og_wgrad_plan(N, Cin, H, W, upsample, pad_mode, Cout, OH, OW, ksize, stride, math, ws != nullptr);
    if (p.rc == OG_BAD_ARGS) return OG_BAD_ARGS;
    if (math >= 4 && (!xmax || !dymax)) return OG_BAD_ARGS;
    if (p.rc != OG_OK) return OG_OK;                    // nothing to do
    if (p.total > 0 && (!ws || ws_floats < p.total)) return OG_BAD_ARGS;
    WgradArgs a;
    a.xmax = xmax; a.dymax = dymax;
    a.ws = nullptr; a.ws_stride = 0; a.accumulate = accumulate ? 1 : 0;
    a.x = x; a.dy = dy; a.dw = dw;
    a.N = N; a.Cin = Cin; a.H = H; a.W = W;
    a.LH = upsample ? 2 * H : H; a.LW = upsample ? 2 * W : W;
    a.Cout = Cout; a.OH = OH; a.OW = OW;
    a.stride = stride; a.pad = pad; a.pad_mode = pad_mode; a.upsample = upsample;
    a.ncol = Cin * ksize * ksize;
    a.xr_begin = p.xr_begin; a.xr_count = 0;
    a.math = p.kmath;
    if (!p.v2 && og_trace())
        fprintf(stderr, "OGTRACE wgrad(v1) Cout=%d Cin=%d k=%d N=%d OH=%d OW=%d stride=%d\n", Cout, Cin, ksize, N, OH, OW, stride);
    const long Npix = (long)N * OH * OW;
    const __bf16* xb = nullptr;
    const __bf16* dyb = nullptr;
    if (p.bfb) {
        if (!p.x_copy_in) og_launch_nhwc_bf16(x, ws, N, Cin, H * W, p.Cpb, s);
        og_launch_f32_to_bf16(dy, ws + p.xb_floats, (long)N * Cout * OH * OW / 4, s);
        xb = reinterpret_cast<const __bf16*>(p.x_copy_in ? x : ws);
        dyb = reinterpret_cast<const __bf16*>(ws + p.xb_floats);
    }
    if (p.dyp) {
        og_launch_h2_pair(dy, dymax, ws, (long)N * Cout * OH * OW, s);
        a.dy = ws;
    }
    for (int i = 0; i < p.nparts; ++i) {
        const WgradPart& q = p.part[i];
        a.m_begin = q.m_begin; a.m_end = q.m_end; a.xr_count = q.xr_count;
        a.pix_per_split = q.pix_per_split;
        a.ws = q.splits > 1 ? ws + q.ws_off : nullptr;
        a.ws_stride = q.splits > 1 ? q.slot : 0;
        const dim3 grid(q.rows * q.tiles_n, q.splits);
        if (p.v2 && og_trace())
            fprintf(stderr, "OGTRACE wgrad TM=%d NW=%d form=%d Cout=%d Cin=%d k=%d N=%d OH=%d OW=%d stride=%d grid=%u,%u math=%d\n", q.tm, q.nw,
                    q.use3 ? 3 : 2, Cout, Cin, ksize, N, OH, OW, stride, grid.x, grid.y, p.kmath);
        const OgFamily fam = !p.v2 ? OG_FAM_WGRAD1 : ((p.bfb || !(p.rec || q.use3)) ? OG_FAM_WGRAD2 : OG_FAM_WGRAD3);
        ProfRec* pr = prof_begin(og_prof_cat(fam, q.tm, q.nw, p.rec ? 5 : (p.h2 ? 4 : 0)),
                                 2.0 * (a.m_end - a.m_begin + a.xr_count) * (double)a.ncol * (double)Npix, s);
        prof_meta(pr, 1, q.tm, a.m_end - a.m_begin + a.xr_count, Cin, ksize * ksize, N, OH, OW,
                  p.v2 ? stride * (upsample ? 10 : 1) * (pad_mode ? -1 : 1) : stride, q.splits);
        int rc = OG_OK;
        if (p.rec2) rc = og_launch_wgrad_rec2(a, q.tm, grid, ksize, p.Cpb, s);
        else if (p.rec) rc = og_launch_wgrad_rec(a, q.tm, q.nw, grid, ksize, p.Cpb, p.dyp, s);
        else if (!p.v2) og_launch_wgrad_v1(a, q.cfg, grid, ksize, s);
        else launch_wgrad2(a, p, q, xb, dyb, grid, ksize, s);
        prof_end(pr, s);
        if (rc != OG_OK) return rc;
        rc = og_launch_status();
        if (rc != OG_OK) return rc;
        if (a.ws) {
            rc = og_launch_wgrad_combine(a, q.splits, s);
            if (rc != OG_OK) return rc;
        }
    }
    return OG_OK;
}

// Floats of workspace objgan_conv_wgrad needs for these arguments (0: every launch runs as one split).  Host-only.
long objgan_conv_wgrad_ws_floats(int N, int Cin, int H, int W, int upsample, int pad_mode,
                                 int Cout, int OH, int OW, int ksize, int stride, int pad, int math) {
    const WgradPlan p = og_wgrad_plan(N, Cin, H, W, upsample, pad_mode, Cout, OH, OW, ksize, stride, math, true);
    return p.rc == OG_OK ? p.total : 0;
}

// The launch plan objgan_conv_wgrad follows for these arguments (those of objgan_conv_wgrad_ws_floats, planned with a
// workspace), for tests and tools.  out[0..9] <- {rc, kmath, v2, bfb, rec, rec2, dyp, h2, xrows, nparts}, then 11 ints
// per part for three parts (unused parts 0): {tm, rows, cfg, m_begin, m_end, xr_count, nw, use3, b128, tiles_n, splits}.
// Host-only, launches nothing.
int objgan_conv_wgrad_plan(int N, int Cin, int H, int W, int upsample, int pad_mode,
                           int Cout, int OH, int OW, int ksize, int stride, int pad, int math, int* out) {
    if (!out) return OG_BAD_ARGS;
    const WgradPlan p = og_wgrad_plan(N, Cin, H, W, upsample, pad_mode, Cout, OH, OW, ksize, stride, math, true);
    for (int i = 0; i < 10 + 3 * 11; ++i) out[i] = 0;
    out[0] = p.rc;
    if (p.rc != OG_OK) return OG_OK;
    const int head[9] = {p.kmath, p.v2, p.bfb, p.rec, p.rec2, p.dyp, p.h2, p.xrows, p.nparts};
    for (int i = 0; i < 9; ++i) out[1 + i] = head[i];
    for (int i = 0; i < p.nparts; ++i) {
        const WgradPart& q = p.part[i];
        const int f[11] = {q.tm, q.rows, q.cfg, q.m_begin, q.m_end, q.xr_count, q.nw, q.use3, q.b128, q.tiles_n, q.splits};
        for (int j = 0; j < 11; ++j) out[10 + 11 * i + j] = f[j];
    }
    return OG_OK;
}

// 1 if objgan_conv_wgrad takes math 5 (x as its fp16 record, see objgan_h2_records) for this geometry.  Host-only.
int objgan_conv_wgrad_rec_ok(int N, int Cin, int H, int W, int Cout, int OH, int OW, int ksize) {
    if (N <= 0 || Cin <= 0 || Cout <= 0 || OH <= 0 || OW <= 0) return 0;
    return og_wgrad_rec_geometry(N, Cin, H, W, Cout, OH, OW, ksize) ? 1 : 0;
}

// 1 if objgan_conv_wgrad takes math 3 (x as its bf16 channel-blocked copy) for this geometry.  Host-only.
int objgan_conv_wgrad_bfb_ok(int N, int Cin, int H, int W, int Cout, int OH, int OW, int ksize) {
    if (N <= 0 || Cin <= 0 || Cout <= 0 || OH <= 0 || OW <= 0) return 0;
    return og_wgrad_bfb_geometry(N, Cin, H, W, Cout, OH, OW, ksize) ? 1 : 0;
}

}  // extern "C"

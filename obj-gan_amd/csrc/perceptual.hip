// Memory-bound glue of the shape generator's perceptual term (reference shape_generation/miscc/losses.py:140-160,
// model.py:299-312, miscc/utils.py:351-365): a frozen VGG-19-bn is run on the pooled fake and real masks and the L1
// distance of 19 taps is added to the generator's loss.  The convolutions are the MFMA implicit-GEMM kernels; here:
//   pcp_stem_forward  : x [N, 1, S, S] -> y [N, 3, OH, OW] = (bilinear_align_corners(x) - mean_c) / std_c.  The
//                       3-channel copy and the unnormalised 224 x 224 image never exist.  One thread per group of four
//                       output columns: 4 taps each, three 16-byte stores (scalar stores where OW % 4 != 0 or y is not
//                       16-byte aligned).
//   pcp_stem_backward : the transposed map in GATHER form -- every dx element is owned by one thread that walks the
//                       output pixels whose taps touch it (weights re-derived exactly as the forward derives them) and
//                       is written once; no atomics, no pre-zeroed buffer.
//   l1_tap_forward    : out[slot] = (1 / n) sum |f - r|.  Per-thread and per-workgroup sums in fp64, one fp64 partial
//                       per workgroup, added in workgroup order by a one-workgroup second launch: no float atomics, two
//                       runs give the same bits.
//   l1_tap_backward   : g = mask(f) * (gdown + coef * sign(f - r)) in one pass: the L1 gradient, the gradient that
//                       arrives from the deeper layers and the ReLU mask of the tap (the tap IS the in-place ReLU's
//                       output, so the mask is f > 0).  coef = upstream * lambda / n is read from device memory.  The
//                       launch leaves the partial maxima of |g| (common.h og_amax_own) for the fp16x2 data gradient
//                       that reads g next.
// All fp32; 16-byte accesses where the pointers allow, scalar otherwise and for the tail.
#include "common.h"

#define PCP_MEAN0 0.485f
#define PCP_MEAN1 0.456f
#define PCP_MEAN2 0.406f
#define PCP_STD0 0.229f
#define PCP_STD1 0.224f
#define PCP_STD2 0.225f
#define PCP_L1_MAX_GRID 1024

// align_corners=True: src = dst * (in - 1) / (out - 1), 0 when out == 1 (and when in == 1).  Kept as the integer quotient
// and remainder of dst * num / den (num = in - 1, den = out - 1; den == 0: everything reads input 0), so that the tap
// index is exact and the weight is ONE rounding: torch's fp32 form, scale * dst with a rounded scale, is off by up to
// 4e-6 in the weight at 64 -> 224, above the 1e-6 the stem is held to against fp64.
__device__ __forceinline__ void pcp_src(int o, int num, int den, int in_size, int& i0, int& i1, float& l0, float& l1) {
    const int p = den > 0 ? o * num : 0;
    const int d = den > 0 ? den : 1;
    i0 = p / d;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = (float)(p - i0 * d) / (float)d;
    l0 = 1.0f - l1;
}

__device__ __forceinline__ float pcp_weight(int o, int i, int num, int den, int in_size) {
    int i0, i1;
    float l0, l1;
    pcp_src(o, num, den, in_size, i0, i1, l0, l1);
    float w = 0.f;
    if (i == i0) w += l0;
    if (i == i1) w += l1;
    return w;
}

// groups of four consecutive output columns of one output row: e = (n * OH + oh) * G4 + g, G4 = ceil(OW / 4)
template <bool V4>
__global__ __launch_bounds__(256) void pcp_stem_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long groups,
                                                           int S, int OH, int OW, int G4) {
    const float mean[3] = {PCP_MEAN0, PCP_MEAN1, PCP_MEAN2};
    const float stdv[3] = {PCP_STD0, PCP_STD1, PCP_STD2};
    const long plane = (long)OH * OW;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < groups; e += (long)gridDim.x * blockDim.x) {
        const int g = (int)(e % G4);
        const long r = e / G4;
        const int oh = (int)(r % OH);
        const long n = r / OH;
        int h0, h1;
        float lh0, lh1;
        pcp_src(oh, S - 1, OH - 1, S, h0, h1, lh0, lh1);
        const float* xp = x + n * (long)S * S;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ow = min(4 * g + j, OW - 1);
            int w0, w1;
            float lw0, lw1;
            pcp_src(ow, S - 1, OW - 1, S, w0, w1, lw0, lw1);
            v[j] = lh0 * (lw0 * xp[h0 * S + w0] + lw1 * xp[h0 * S + w1]) +
                   lh1 * (lw0 * xp[h1 * S + w0] + lw1 * xp[h1 * S + w1]);
        }
        float* yp = y + n * 3 * plane + (long)oh * OW + 4 * g;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (V4) {
                *reinterpret_cast<float4*>(yp + c * plane) = make_float4((v[0] - mean[c]) / stdv[c], (v[1] - mean[c]) / stdv[c],
                                                                         (v[2] - mean[c]) / stdv[c], (v[3] - mean[c]) / stdv[c]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * g + j < OW) yp[c * plane + j] = (v[j] - mean[c]) / stdv[c];
            }
        }
    }
}

// one thread per dx element: dx[n, ih, iw] = sum_{oh, ow} wh(oh, ih) ww(ow, iw) sum_c dy[n, c, oh, ow] / std_c
__global__ __launch_bounds__(256) void pcp_stem_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, long total,
                                                           int S, int OH, int OW) {
    const int num = S - 1;
    const bool sh = num > 0 && OH > 1, sw = num > 0 && OW > 1;          // a non-zero scale
    const long plane = (long)OH * OW;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int iw = (int)(e % S);
        const int ih = (int)((e / S) % S);
        const long n = e / ((long)S * S);
        // candidate outputs: o * num / den in (i - 1, i + 1), i.e. o in ((i - 1) den / num, (i + 1) den / num), widened by
        // one on each side (the weights decide); every output when the scale is 0 (S == 1 or a one-pixel output: all of
        // them read input 0)
        int oh_lo = sh ? max(ih - 1, 0) * (OH - 1) / num - 1 : 0;
        int oh_hi = sh ? ((ih + 1) * (OH - 1) + num - 1) / num + 1 : OH - 1;
        int ow_lo = sw ? max(iw - 1, 0) * (OW - 1) / num - 1 : 0;
        int ow_hi = sw ? ((iw + 1) * (OW - 1) + num - 1) / num + 1 : OW - 1;
        oh_lo = max(oh_lo, 0); ow_lo = max(ow_lo, 0);
        oh_hi = min(oh_hi, OH - 1); ow_hi = min(ow_hi, OW - 1);
        const float* gp = dy + n * 3 * plane;
        float acc = 0.f;
        for (int oh = oh_lo; oh <= oh_hi; ++oh) {
            const float wh = pcp_weight(oh, ih, num, OH - 1, S);
            if (wh == 0.f) continue;
            float row = 0.f;
            for (int ow = ow_lo; ow <= ow_hi; ++ow) {
                const float ww = pcp_weight(ow, iw, num, OW - 1, S);
                if (ww == 0.f) continue;
                const long o = (long)oh * OW + ow;
                const float d = gp[o] / PCP_STD0 + gp[plane + o] / PCP_STD1 + gp[2 * plane + o] / PCP_STD2;
                row = fmaf(ww, d, row);
            }
            acc = fmaf(wh, row, acc);
        }
        dx[e] = acc;
    }
}

// fp64 sum of the block's values in a fixed order: lanes by butterfly, waves in wave order
__device__ __forceinline__ double pcp_block_sum_f64(double v, double* red /* >= 4 doubles of LDS */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    const int nw = (blockDim.x + 63) >> 6;
    double r = red[0];
    for (int w = 1; w < nw; ++w) r += red[w];
    return r;
}

template <bool V4>
__global__ __launch_bounds__(256) void l1_tap_partial_kernel(const float* __restrict__ f, const float* __restrict__ r, long n,
                                                             double* __restrict__ part) {
    __shared__ double red[4];
    double acc = 0.0;
    long e0 = 0;
    if (V4) {
        const long n4 = n >> 2, step = (long)gridDim.x * 256;
        const float4* f4 = reinterpret_cast<const float4*>(f);
        const float4* r4 = reinterpret_cast<const float4*>(r);
        for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < n4; g += 2 * step) {
            const long g1 = g + step;
            const bool two = g1 < n4;
            const float4 fa = f4[g], ra = r4[g];
            const float4 fb = f4[two ? g1 : g], rb = r4[two ? g1 : g];
            const float sa = (fabsf(fa.x - ra.x) + fabsf(fa.y - ra.y)) + (fabsf(fa.z - ra.z) + fabsf(fa.w - ra.w));
            const float sb = (fabsf(fb.x - rb.x) + fabsf(fb.y - rb.y)) + (fabsf(fb.z - rb.z) + fabsf(fb.w - rb.w));
            acc += (double)sa;
            if (two) acc += (double)sb;
        }
        e0 = n4 << 2;
    }
    for (long e = e0 + (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x)
        acc += (double)fabsf(f[e] - r[e]);
    const double s = pcp_block_sum_f64(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one wave, a fixed order: lane l adds partials l, l + 64, ... (<= 16 loads, coalesced across the wave), then the butterfly
__global__ __launch_bounds__(64) void l1_tap_final_kernel(const double* __restrict__ part, int nparts, double inv_n,
                                                          float* __restrict__ out) {
    double s = 0.0;
    for (int k = threadIdx.x; k < nparts; k += 64) s += part[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) out[0] = (float)(s * inv_n);
}

__device__ __forceinline__ float l1_bwd_one(float f, float r, float gd, float coef, int relu_mask) {
    const float sgn = f > r ? 1.f : (f < r ? -1.f : 0.f);
    const float v = gd + coef * sgn;                   // coef * sgn is exact: one rounding with or without contraction
    return (relu_mask && !(f > 0.f)) ? 0.f : v;
}

template <bool V4, bool DOWN>
__global__ __launch_bounds__(256) void l1_tap_bwd_kernel(const float* __restrict__ f, const float* __restrict__ r,
                                                         const float* __restrict__ gdown, const float* __restrict__ coef_p,
                                                         float* __restrict__ g, long n, int relu_mask, float* __restrict__ amax) {
    __shared__ float amax_red[4];
    const float coef = coef_p[0];
    float vmax = 0.f;
    long e0 = 0;
    if (V4) {
        const long n4 = n >> 2, step = (long)gridDim.x * 256;
        const float4* f4 = reinterpret_cast<const float4*>(f);
        const float4* r4 = reinterpret_cast<const float4*>(r);
        const float4* d4 = reinterpret_cast<const float4*>(gdown);
        float4* g4 = reinterpret_cast<float4*>(g);
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += 2 * step) {
            const long i1 = i + step < n4 ? i + step : i;          // (the last trip of a thread may hold one group: twice)
            const float4 fa = f4[i], ra = r4[i], fb = f4[i1], rb = r4[i1];
            const float4 da = DOWN ? d4[i] : zero, db = DOWN ? d4[i1] : zero;
            const float va[4] = {l1_bwd_one(fa.x, ra.x, da.x, coef, relu_mask), l1_bwd_one(fa.y, ra.y, da.y, coef, relu_mask),
                                 l1_bwd_one(fa.z, ra.z, da.z, coef, relu_mask), l1_bwd_one(fa.w, ra.w, da.w, coef, relu_mask)};
            const float vb[4] = {l1_bwd_one(fb.x, rb.x, db.x, coef, relu_mask), l1_bwd_one(fb.y, rb.y, db.y, coef, relu_mask),
                                 l1_bwd_one(fb.z, rb.z, db.z, coef, relu_mask), l1_bwd_one(fb.w, rb.w, db.w, coef, relu_mask)};
            g4[i] = make_float4(va[0], va[1], va[2], va[3]);
            if (i1 != i) g4[i1] = make_float4(vb[0], vb[1], vb[2], vb[3]);
#pragma unroll
            for (int j = 0; j < 4; ++j) vmax = fmaxf(vmax, fmaxf(fabsf(va[j]), fabsf(vb[j])));
        }
        e0 = n4 << 2;
    }
    for (long e = e0 + (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const float v = l1_bwd_one(f[e], r[e], DOWN ? gdown[e] : 0.f, coef, relu_mask);
        g[e] = v;
        vmax = fmaxf(vmax, fabsf(v));
    }
    if (amax) og_amax_own(og_block_max(vmax, amax_red), amax, blockIdx.x, gridDim.x);      // grid <= OG_AMAX_SLOTS
}

extern "C" {

// y[N, 3, OH, OW] = (F.interpolate(x[N, 1, S, S], (OH, OW), 'bilinear', align_corners=True) - mean_c) / std_c
int objgan_pcp_stem_forward(const float* x, float* y, int N, int S, int OH, int OW, void* stream) {
    OG_ENTRY();
    if (N < 0 || S < 1 || OH < 1 || OW < 1) return OG_BAD_ARGS;
    if (N == 0) return OG_OK;
    if (!x || !y) return OG_BAD_ARGS;
    const int G4 = (OW + 3) / 4;
    const long groups = (long)N * OH * G4;
    const bool v4 = !(OW & 3) && !((size_t)y & 15);
    if ((long)(S - 1) * (long)((OH > OW ? OH : OW) + 1) >= (1L << 30)) return OG_BAD_ARGS;      // index products stay in int
    if (v4)
        hipLaunchKernelGGL(pcp_stem_fwd_kernel<true>, dim3(og_stream_grid(groups, 256)), dim3(256), 0, (hipStream_t)stream,
                           x, y, groups, S, OH, OW, G4);
    else
        hipLaunchKernelGGL(pcp_stem_fwd_kernel<false>, dim3(og_stream_grid(groups, 256)), dim3(256), 0, (hipStream_t)stream,
                           x, y, groups, S, OH, OW, G4);
    return og_launch_status();
}

// dx[N, 1, S, S]: every element written once
int objgan_pcp_stem_backward(const float* dy, float* dx, int N, int S, int OH, int OW, void* stream) {
    OG_ENTRY();
    if (N < 0 || S < 1 || OH < 1 || OW < 1) return OG_BAD_ARGS;
    if (N == 0) return OG_OK;
    if (!dy || !dx) return OG_BAD_ARGS;
    if ((long)(S + 1) * (long)((OH > OW ? OH : OW) + 1) >= (1L << 30)) return OG_BAD_ARGS;      // index products stay in int
    const long total = (long)N * S * S;
    hipLaunchKernelGGL(pcp_stem_bwd_kernel, dim3(og_stream_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       dy, dx, total, S, OH, OW);
    return og_launch_status();
}

// doubles of workspace objgan_l1_tap_forward needs (one partial per workgroup): the same for every n > 0, so one
// workspace serves all the taps of a network
long objgan_l1_tap_ws_doubles(long n) {
    return n > 0 ? PCP_L1_MAX_GRID : 0;
}

// out[slot] = (1 / n) sum_i |f[i] - r[i]|; ws: objgan_l1_tap_ws_doubles(n) doubles
int objgan_l1_tap_forward(const float* f, const float* r, long n, float* out, int slot, double* ws, void* stream) {
    OG_ENTRY();
    if (n <= 0 || slot < 0 || !f || !r || !out || !ws) return OG_BAD_ARGS;
    const bool v4 = !(((size_t)f | (size_t)r) & 15) && n >= 4;
    int grid = og_stream_grid(v4 ? (n + 7) >> 3 : n, 256);
    if (grid > PCP_L1_MAX_GRID) grid = PCP_L1_MAX_GRID;
    hipStream_t s = (hipStream_t)stream;
    if (v4) hipLaunchKernelGGL(l1_tap_partial_kernel<true>, dim3(grid), dim3(256), 0, s, f, r, n, ws);
    else hipLaunchKernelGGL(l1_tap_partial_kernel<false>, dim3(grid), dim3(256), 0, s, f, r, n, ws);
    hipLaunchKernelGGL(l1_tap_final_kernel, dim3(1), dim3(64), 0, s, ws, grid, 1.0 / (double)n, out + slot);
    return og_launch_status();
}

// g[i] = mask(f[i]) * (gdown[i] + coef[0] * sign(f[i] - r[i])); gdown may be NULL (zero); relu_mask != 0: mask = f > 0,
// else 1; coef: one float in device memory; amax (may be NULL): the 1024 partial maxima of |g|
int objgan_l1_tap_backward(const float* f, const float* r, const float* gdown, const float* coef, float* g, long n,
                           int relu_mask, float* amax, void* stream) {
    OG_ENTRY();
    if (n <= 0 || !f || !r || !coef || !g) return OG_BAD_ARGS;
    const bool v4 = !(((size_t)f | (size_t)r | (size_t)g | (size_t)gdown) & 15) && n >= 4;
    int grid = og_stream_grid(v4 ? (n + 7) >> 3 : n, 256);
    if (grid > OG_AMAX_SLOTS) grid = OG_AMAX_SLOTS;              // every workgroup owns a slot
    hipStream_t s = (hipStream_t)stream;
    const int m = relu_mask ? 1 : 0;
    if (v4 && gdown) hipLaunchKernelGGL((l1_tap_bwd_kernel<true, true>), dim3(grid), dim3(256), 0, s, f, r, gdown, coef, g, n, m, amax);
    else if (v4) hipLaunchKernelGGL((l1_tap_bwd_kernel<true, false>), dim3(grid), dim3(256), 0, s, f, r, gdown, coef, g, n, m, amax);
    else if (gdown) hipLaunchKernelGGL((l1_tap_bwd_kernel<false, true>), dim3(grid), dim3(256), 0, s, f, r, gdown, coef, g, n, m, amax);
    else hipLaunchKernelGGL((l1_tap_bwd_kernel<false, false>), dim3(grid), dim3(256), 0, s, f, r, gdown, coef, g, n, m, amax);
    return og_launch_status();
}

}  // extern "C"

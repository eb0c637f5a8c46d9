// Operand preparation for the convolution kernels: packed filter banks, operand copies, partial maxima.
//
// Kernels:  pack_weights_kernel, pack_weights_batched_kernel   PyTorch conv weight -> the bank layout of PackArgs::m_major
//           absmax_w_kernel, absmax_w_jobs_kernel               partial maxima of |w| behind an fp16x2 bank
//           absmax_partials_kernel                              partial maxima of |x| over a tensor
//           nchw_to_nhwc_bf16_kernel                            fp32 NCHW -> bf16 channel-blocked copy (bf16 mode)
//           f32_to_bf16_kernel                                  fp32 -> bf16, same layout (dy of conv_wgrad_bfb_kernel)
//           splitk_combine_kernel                               second level of the forward split-K (emits maxima of |y|)
// Host:     og_bank_layout (which layout a call uses), og_fill_pack, og_fill_pack_phase, one launcher per kernel for
//           the other convolution sources (og_launch_*, og_absmax_launch)
// Entry points: objgan_absmax_partials, objgan_conv_pack_job_bytes, objgan_conv_pack_job, objgan_conv_pack_job_phase,
//           objgan_conv_pack_jobs_run, objgan_conv_bank_layout, objgan_conv_packed_floats, objgan_nhwc_bf16{,_floats}
#include "conv_igemm_host.h"

// ---- weight packing (PackArgs: conv_igemm_host.h) -----------------------------------------------------
// K walk order of conv_igemm3_kernel and of its banks.  Tap-major (all channels of tap 0, then tap 1, ...) keeps the
// tap geometry out of the inner steps, but every tap re-reads the SAME source pixels one full channel sweep later: at
// 128 x 128 x 194..388 channels a sweep of the workgroups of one XCD is 6-16 MB, the 4 MB L2 has long lost the lines
// and every tap fetches them again from HBM / MALL (r03 PMC: 3.9-4.1x the algorithmic bytes).  Walking the channels in
// GROUPS of G chunks -- all taps of a group back to back -- bounds the reuse distance to T * G steps.
//   step(t, chunk c): g = c / G; steps of the full groups before it + t * (chunks in group g) + (c - g * G)
__host__ __device__ __forceinline__ int og_kstep(int t, int c16, int spt, int T, int G) {
    const int g = c16 / G;
    const int Gg = min(G, spt - g * G);
    return g * T * G + t * Gg + (c16 - g * G);
}

// Work items of a job.  Row-major banks (m_major 1 / 3: wt[m][t*Cp + ck]) are packed per (m, ck) PAIR: a
// thread reads the Torig taps of its pair -- one contiguous 36..64-byte run of w, adjacent pairs adjacent runs
// for the forward banks -- and writes one element per GEMM tap, adjacent threads adjacent addresses.  The first
// version walked the bank element by element: for the transposed (data-gradient) banks adjacent elements are a
// whole filter apart in w, every 4-byte read pulled its own 64-byte line and the line was gone from the L2
// before its neighbours were wanted (PMC: 1.2 GB fetched per launch for 0.1 GB of banks; 2.2 ms per step).
__device__ __forceinline__ long pack_total(const PackArgs& a, int Kpad, int Krow) {
    return a.m_major == 2 ? (long)(a.Ck + 1) * a.Tg * a.Mpad        // + one zero channel
                          : (a.m_major ? (long)a.M * a.Cp : (long)Kpad * a.Mpad);
}

// element i of the small layouts (0: wt[k][Mpad], 2: wt[ck][t][MT])
__device__ __forceinline__ void pack_element(const PackArgs& a, unsigned i, int Kpad) {
    int m, t, ck;
    if (a.m_major == 2) {
        const unsigned r = i / (unsigned)a.Mpad;
        m = (int)(i - r * (unsigned)a.Mpad);
        t = (int)(r % (unsigned)a.Tg);
        ck = (int)(r / (unsigned)a.Tg);
    } else {
        const unsigned k = i / (unsigned)a.Mpad;
        m = (int)(i - k * (unsigned)a.Mpad);
        t = (int)(k / (unsigned)a.Cp);
        ck = (int)k - t * a.Cp;
    }
    float v = 0.f;
    if (m < a.M && ck < a.Ck) {
        const int st = a.src_tap[t];
        if (st >= 0) {
            const int co = a.transpose ? ck : m;
            const int ci = a.transpose ? m : ck;
            v = a.w[((size_t)co * a.Cin + ci) * a.Torig + st];
        }
    }
    a.wt[i] = v;
}

// element k of the bank row starting at `row` (element units of the layout)
__device__ __forceinline__ void pack_store(const PackArgs& a, size_t row, int k, float v) {
    if (a.m_major == 4) {
        __bf16* o = reinterpret_cast<__bf16*>(a.wt) + row + (size_t)(k >> 4) * 48 + (k & 15);
        const __bf16 h = (__bf16)v;
        const float r1 = v - (float)h;
        const __bf16 m = (__bf16)r1;
        o[0] = h; o[16] = m; o[32] = (__bf16)(r1 - (float)m);
    } else if (a.m_major == 5) {         // fp16x2: w * 2^wexp = h + l (max |w| * 2^wexp in [2^14, 2^15))
        _Float16* o = reinterpret_cast<_Float16*>(a.wt) + row + (size_t)(k >> 4) * 32 + (k & 15);
        const float sv = v * og_pow2(a.wexp);
        const _Float16 h = (_Float16)sv;
        o[0] = h; o[16] = (_Float16)(sv - (float)h);
    } else if (a.m_major == 3) {
        reinterpret_cast<__bf16*>(a.wt)[row + k] = (__bf16)v;
    } else {
        a.wt[row + k] = v;
    }
}

// pair i = m * Cp + ck of the row-major layouts
__device__ __forceinline__ void pack_pair(const PackArgs& a, unsigned i, int Kpad, int Krow) {
    const unsigned m = i / (unsigned)a.Cp;
    const int ck = (int)(i - m * (unsigned)a.Cp);
    const bool live = ck < a.Ck;
    const int co = a.transpose ? ck : (int)m;
    const int ci = a.transpose ? (int)m : ck;
    const float* src = a.w + ((size_t)co * a.Cin + ci) * a.Torig;
    const size_t row = (size_t)m * Krow;
    if (a.Torig == 16) {
        // 4x4 filters (most of the bank bytes): the pair's 16 taps are one aligned 64-byte line -- four 16-byte
        // loads instead of sixteen 4-byte ones that each walk 64 different lines per wave
        float r[16];
        const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 f = live ? s4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            r[4 * q] = f.x; r[4 * q + 1] = f.y; r[4 * q + 2] = f.z; r[4 * q + 3] = f.w;
        }
        for (int t = 0; t < a.Tg; ++t) {
            const int st = a.src_tap[t];                 // uniform: a select chain, no register indexing
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) v = st == j ? r[j] : v;
            pack_store(a, row, og_kstep(t, ck >> 4, a.Cp >> 4, a.Tg, a.kgroup) * 16 + (ck & 15), v);
        }
    } else {
        for (int t = 0; t < a.Tg; ++t) {
            const int st = a.src_tap[t];
            const float v = (live && st >= 0) ? src[st] : 0.f;
            pack_store(a, row, og_kstep(t, ck >> 4, a.Cp >> 4, a.Tg, a.kgroup) * 16 + (ck & 15), v);
        }
    }
    if (a.m_major == 3 && ck < Krow - Kpad)               // bf16 rows are padded to a multiple of 32
        reinterpret_cast<__bf16*>(a.wt)[row + Kpad + ck] = (__bf16)0.f;
}

__device__ __forceinline__ void pack_item(const PackArgs& a, long i, int Kpad, int Krow) {
    if (a.m_major == 1 || a.m_major >= 3) pack_pair(a, (unsigned)i, Kpad, Krow);
    else pack_element(a, (unsigned)i, Kpad);
}

// fp32 [N][C][HW] -> bf16 (RNE) channel-blocked [N][Cp/16][HW][16], channels C..Cp-1 zero: the pixel operand of the
// bf16 mode (16 channels of a pixel = 32 contiguous bytes, neighbouring pixels of a chunk contiguous).
// 64 channels x 64 pixels per workgroup through LDS: 256-byte rows in, 1 KiB runs per wave out.
__global__ __launch_bounds__(256) void nchw_to_nhwc_bf16_kernel(const float* __restrict__ x, __bf16* __restrict__ out,
                                                                int C, int HW, int Cp) {
    __shared__ float tile[64][65];
    const int n = blockIdx.z;
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const float* xn = x + (size_t)n * C * HW;
#pragma unroll 4
    for (int cc = ty; cc < 64; cc += 4) {
        const int c = c0 + cc, p = p0 + tx;
        tile[cc][tx] = (c < C && p < HW) ? xn[(size_t)c * HW + p] : 0.f;
    }
    __syncthreads();
    const int cg = threadIdx.x >> 5;                   // 8 channels = one 16-byte store; a wave = one 16-channel chunk
    if (c0 + cg * 8 >= Cp) return;
    const int chunk = (c0 + cg * 8) >> 4, half = cg & 1;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int pp = (threadIdx.x & 31) + 32 * it;
        const int p = p0 + pp;
        if (p >= HW) continue;
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (__bf16)tile[cg * 8 + j][pp];
        *reinterpret_cast<bf16x8*>(out + (((size_t)n * (Cp / 16) + chunk) * HW + p) * 16 + half * 8) = v;
    }
}

// Partial maxima of |w| for the fp16x2 banks: 64 workgroups own the OG_AMAX_SLOTS slots (common.h og_amax_own)
__device__ __forceinline__ void absmax_w_block(const float* __restrict__ w, long n, float* __restrict__ out) {
    __shared__ float red[4];
    float m = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += 64L * 256) m = fmaxf(m, fabsf(w[i]));
    og_amax_own(og_block_max(m, red), out, blockIdx.x, 64);
}
__global__ __launch_bounds__(256) void absmax_w_kernel(const float* __restrict__ w, long n, float* __restrict__ out) {
    absmax_w_block(w, n, out);
}
__global__ __launch_bounds__(256) void pack_weights_kernel(const PackArgs a_in) {
    PackArgs a = a_in;
    if (a.m_major == 5) { og_fp16_saturate(); a.wexp = og_h2_exponent(a.wmax, threadIdx.x & 63); }
    const int Kpad = a.Tg * a.Cp;
    const int Krow = a.m_major == 3 ? (Kpad + 31) / 32 * 32 : (a.m_major == 4 ? 3 * Kpad : (a.m_major == 5 ? 2 * Kpad : Kpad));
    const long total = pack_total(a, Kpad, Krow);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x)
        pack_item(a, i, Kpad, Krow);
}

// Many banks in one launch: blockIdx.y = job.  After an optimizer step every cached bank of the updated
// network is stale at once -- ~60 banks per network, 499 7-us launches per training step when each is
// re-packed at its next use; the host keeps the jobs of a network in a device table instead and refreshes
// them right behind the Adam kernel (objgan_conv_pack_jobs_run).  Bank sizes span three orders of magnitude
// (a 3-channel to-RGB bank .. 768 x 1024 x 9): a workgroup takes OG_PACK_CHUNK consecutive work items per
// sweep and workgroups beyond a small bank's end leave at once.
#define OG_PACK_BLOCKS 256
#define OG_PACK_CHUNK 512
__global__ __launch_bounds__(256) void absmax_w_jobs_kernel(const PackArgs* __restrict__ jobs) {
    const PackArgs a = jobs[blockIdx.y];
    if (a.m_major != 5) return;
    absmax_w_block(a.w, (long)a.Cout * a.Cin * a.Torig, const_cast<float*>(a.wmax));
}

__global__ __launch_bounds__(256) void pack_weights_batched_kernel(const PackArgs* __restrict__ jobs) {
    PackArgs a = jobs[blockIdx.y];
    if (a.m_major == 5) { og_fp16_saturate(); a.wexp = og_h2_exponent(a.wmax, threadIdx.x & 63); }
    const int Kpad = a.Tg * a.Cp;
    const int Krow = a.m_major == 3 ? (Kpad + 31) / 32 * 32 : (a.m_major == 4 ? 3 * Kpad : (a.m_major == 5 ? 2 * Kpad : Kpad));
    const long total = pack_total(a, Kpad, Krow);
    for (long base = (long)blockIdx.x * OG_PACK_CHUNK; base < total; base += (long)gridDim.x * OG_PACK_CHUNK) {
#pragma unroll
        for (int u = 0; u < OG_PACK_CHUNK / 256; ++u) {
            const long i = base + u * 256 + threadIdx.x;
            if (i < total) pack_item(a, i, Kpad, Krow);
        }
    }
}

// (This kernel of the forward path sits here, behind the other kernels that inline og_block_max, on purpose: the code
// hipcc emits for such a kernel depends on whether an earlier kernel of the translation unit inlined the helper before
// it.  tools/kernel_diff.py shows it when a move changes the instructions.)
// out[e] = act(bias[(e / HW) % M] + sum_{s < splits} ws[s * ws_stride + seg_off + e]): the second level of split-K
// (conv_igemm3_kernel writes the partial tiles), splits summed in order.
// ymax (may be null; zeroed by the caller): the partial maxima of |out| for an fp16x2 consumer, added with one integer
// atomicMax per workgroup -- round 6: this was a separate pass over the output behind every split launch with a fused
// ReLU / LeakyReLU (the Inception chain's small maps).
// V4 (the host asks for it when ws + seg_off is 16-byte aligned, ws_stride % 4 == 0 and total < 2^31): four consecutive
// elements per thread as one 16-byte load per slot, eight slots in flight (a one-workgroup launch behind a long-K head is
// as long as the latency of its chain of slot loads), every lane summed in the same slot order, one 16-byte store where
// out allows it.  The bias channel (e / HW) % M is derived once per group in 32-bit arithmetic and stepped with a carry
// where a group straddles channels (HW = 289, 25, 1 225).  The scalar loop behind it takes the total % 4 tail, or
// everything.
template <bool V4>
__global__ __launch_bounds__(256) void splitk_combine_kernel(const float* __restrict__ ws, int splits, long ws_stride,
                                                             long seg_off, float* __restrict__ out, long total,
                                                             const float* __restrict__ bias, int M, int HW, int act,
                                                             float* __restrict__ ymax) {
    __shared__ float red[4];
    float vmax = 0.f;
    long e0 = 0;
    if (V4) {
        const unsigned n4 = (unsigned)(total >> 2), uHW = (unsigned)HW, uM = (unsigned)M;
        const f32x4* p4 = reinterpret_cast<const f32x4*>(ws + seg_off);
        const size_t stride4 = (size_t)ws_stride >> 2;
        const bool one_channel = (HW & 3) == 0;
        for (unsigned g = blockIdx.x * 256u + threadIdx.x; g < n4; g += gridDim.x * 256u) {
            f32x4 v = og_sum_slots4<8>(p4 + g, splits, stride4);
            if (bias) {
                const unsigned q = (g * 4u) / uHW;
                unsigned rem = g * 4u - q * uHW, ch = q % uM;
                if (one_channel) {
                    v += bias[ch];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v[j] += bias[ch];
                        if (++rem == uHW) { rem = 0; ch = ch + 1 == uM ? 0 : ch + 1; }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = og_act(v[j], act);
            float* o = out + ((size_t)g << 2);
            if (!((size_t)o & 15)) {
                *reinterpret_cast<f32x4*>(o) = v;
            } else {                                   // (an output view that starts off a 16-byte boundary)
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = v[j];
            }
            vmax = fmaxf(fmaxf(vmax, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
        }
        e0 = (long)n4 << 2;
    }
    for (long e = e0 + (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const float* p = ws + seg_off + e;
        float v = p[0];
        for (int k = 1; k < splits; ++k) v += p[(size_t)k * ws_stride];
        if (bias) v += bias[(e / HW) % M];
        v = og_act(v, act);
        out[e] = v;
        vmax = fmaxf(vmax, fabsf(v));
    }
    if (ymax) og_amax_atomic(og_block_max(vmax, red), ymax, blockIdx.x);
}
void og_launch_splitk_combine(const float* ws, int splits, long ws_stride, long seg_off, float* out, long total,
                              const float* bias, int M, int HW, int act, float* ymax, hipStream_t s) {
    const bool v4 = !((size_t)(ws + seg_off) & 15) && !(ws_stride & 3) && total >= 4 && total < (1L << 31);
    if (v4)
        hipLaunchKernelGGL(splitk_combine_kernel<true>, dim3(og_stream_grid((total + 3) >> 2, 256)), dim3(256), 0, s, ws, splits,
                           ws_stride, seg_off, out, total, bias, M, HW, act, ymax);
    else
        hipLaunchKernelGGL(splitk_combine_kernel<false>, dim3(og_stream_grid(total, 256)), dim3(256), 0, s, ws, splits,
                           ws_stride, seg_off, out, total, bias, M, HW, act, ymax);
}

// fp32 -> bf16 (RNE), same layout: the dy operand of conv_wgrad_bfb_kernel.  n4 = elements / 4.
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* __restrict__ x, __bf16* __restrict__ out, long n4) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i);
        bf16x4 h;
#pragma unroll
        for (int j = 0; j < 4; ++j) h[j] = (__bf16)v[j];
        *reinterpret_cast<bf16x4*>(out + 4 * i) = h;
    }
}

// Partial maxima of |x| over a tensor: out[0..OG_AMAX_SLOTS) (fp16x2's scale input; the consumers reduce the slots
// themselves -- no zeroed accumulator, no atomics, one launch; grid <= OG_AMAX_SLOTS workgroups own the slots).
__global__ __launch_bounds__(256) void absmax_partials_kernel(const float* __restrict__ x, long n, float* __restrict__ out) {
    __shared__ float red[4];
    float m = 0.f;
    const long n4 = n >> 2;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += 256L * gridDim.x) {
        const f32x4 v = x4[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) m = fmaxf(m, fabsf(x[(n4 << 2) + threadIdx.x]));
    og_amax_own(og_block_max(m, red), out, blockIdx.x, gridDim.x);
}

void og_absmax_launch(const float* x, long n, float* out, hipStream_t s) {
    long g = (n / 4 + 255) / 256;                   // one float4 per thread and trip
    g = g < 1 ? 1 : (g > OG_AMAX_SLOTS ? OG_AMAX_SLOTS : g);
    hipLaunchKernelGGL(absmax_partials_kernel, dim3((int)g), dim3(256), 0, s, x, n, out);
}
void og_launch_absmax_w(const float* w, long n, float* out, hipStream_t s) { hipLaunchKernelGGL(absmax_w_kernel, dim3(64), dim3(256), 0, s, w, n, out); }
void og_launch_pack(const PackArgs& p, long work_items, hipStream_t s) {
    hipLaunchKernelGGL(pack_weights_kernel, dim3(og_stream_grid(work_items, 256)), dim3(256), 0, s, p);
}
void og_launch_nhwc_bf16(const float* x, float* out, int N, int C, int HW, int Cp, hipStream_t s) {
    hipLaunchKernelGGL(nchw_to_nhwc_bf16_kernel, dim3(og_cdiv(HW, 64), og_cdiv(Cp, 64), N), dim3(256), 0, s,
                       x, reinterpret_cast<__bf16*>(out), C, HW, Cp);
}
void og_launch_f32_to_bf16(const float* x, float* out, long n4, hipStream_t s) {
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(og_stream_grid(n4, 256)), dim3(256), 0, s, x, reinterpret_cast<__bf16*>(out), n4);
}

// Which packed-bank layout (PackArgs::m_major) a call with these arguments uses, i.e. which kernel family serves it:
// 0 first generation (conv_igemm_v1.hip), 2 thin VALU (conv_igemm_thin.hip), 1 / 3 / 4 / 5 conv_igemm3_kernel in fp32 /
// bf16 / bf16x3 / fp16x2.  MT_out = accumulator count of the thin kernel when the answer is 2.  The single source of
// truth for objgan_conv_igemm and objgan_conv_bank_layout.
static int og_bank_layout(int N, int C, int H, int W, int M, int Tg, int PH, int PW, int act, int math,
                          int* MT_out) {
    const long Cp = ((long)C + 15) / 16 * 16;
    const bool v2 = !og_igemm_v1() && (double)N * C * H * W * 4.0 < 4.0e9 && (double)M * Tg * Cp * 4.0 < 4.0e9;
    const int MT = og_thin_mt(M);
    if (MT_out) *MT_out = MT;
    if (!v2) return 0;
    // thin outputs: direct VALU kernel (full-coverage or strided-phase launches alike), always fp32
    const bool thin = !og_nothin() && M <= 32 && (Tg == 9 || Tg == 4) && (long)N * PH * PW >= 65536
                      && (MT <= 4 || (act != OG_ACT_TANH && act != OG_ACT_SIGMOID));
    if (thin) return 2;
    return math == 1 ? 3 : (math == 2 ? 4 : (math >= 4 ? 5 : 1));
}

// The PackArgs of objgan_conv_igemm for these arguments (single source of truth for the call itself and for
// objgan_conv_pack_job); returns the bank layout class, MT_out as og_bank_layout.
int og_fill_pack(PackArgs& p, const float* w, float* wt, int N, int C, int H, int W, int Cout, int Cin,
                 int Torig, int transpose, int Tg, const int* src_tap, int PH, int PW, int act, int math,
                 int* MT_out) {
    const int M = transpose ? Cin : Cout;
    p.w = w; p.wt = wt; p.Cout = Cout; p.Cin = Cin; p.Torig = Torig; p.Tg = Tg;
    p.M = M; p.Mpad = (M + 127) / 128 * 128; p.Ck = C; p.Cp = (C + 15) / 16 * 16;
    p.transpose = transpose;
    int MT = 32;
    p.m_major = og_bank_layout(N, C, H, W, M, Tg, PH, PW, act, math, &MT);
    p.kgroup = og_kgroup(C, Tg, H, PH);
    p.wmax = wt ? wt + objgan_conv_packed_floats(M, C, Tg) - OG_AMAX_SLOTS : nullptr; p.wexp = 0;
    if (p.m_major == 2) p.Mpad = MT;
    for (int t = 0; t < OG_MAX_TAPS; ++t) p.src_tap[t] = (signed char)(t < Tg ? src_tap[t] : -1);
    if (MT_out) *MT_out = MT;
    return p.m_major;
}

void og_fill_pack_phase(PackArgs& p, const float* w, float* wt, int Cout, int Cin, int Torig, int Tg,
                        const int* src_tap_phase, int phase, int math) {
    const int M = Cin, C = Cout;
    const int Cp = (C + 15) / 16 * 16;
    const bool thin = math == -2;           // thin layout of conv_thin_ph4_kernel: [C + 1][Tg][MT] per phase
    const int MT = og_thin_mt(M), Krow = og_krow(Tg * Cp, math);
    // phase banks back to back (Krow counts 16-bit elements in the bf16 / fp16 modes)
    const long bank = thin ? (long)(C + 1) * Tg * MT : (math ? (long)M * Krow / 2 : (long)M * Krow);
    p.w = w; p.wt = wt + phase * bank; p.Cout = Cout; p.Cin = Cin; p.Torig = Torig; p.Tg = Tg;
    p.M = M; p.Mpad = thin ? MT : (M + 127) / 128 * 128; p.Ck = C; p.Cp = Cp;
    p.transpose = 1; p.m_major = thin ? 2 : (math == 1 ? 3 : (math == 2 ? 4 : (math >= 4 ? 5 : 1)));
    p.kgroup = thin ? 0 : og_kgroup_phases(C);
    p.wmax = thin ? nullptr : wt + og_phase_wmax_offset(M, Tg, Cp); p.wexp = 0;
    for (int t = 0; t < OG_MAX_TAPS; ++t) p.src_tap[t] = (signed char)(t < Tg ? src_tap_phase[t] : -1);
}

extern "C" {

// out[1024] = partial maxima of |x[0..n)| (x 16-byte aligned): the scale input of the fp16x2 arithmetic (math 4).
// (Consumers reduce the slots themselves -- no zeroed accumulator, no atomics, one launch.)
int objgan_absmax_partials(const float* x, long n, float* out, void* stream) {
    OG_ENTRY();
    if (!x || !out || n <= 0 || ((size_t)x & 15)) return OG_BAD_ARGS;
    og_absmax_launch(x, n, out, (hipStream_t)stream);
    return og_launch_status();
}

// ---- batched re-packing of cached filter banks ---------------------------------------------------
// A job is an opaque blob of objgan_conv_pack_job_bytes() bytes describing "pack w into wt exactly as
// objgan_conv_igemm (or phase `phase` of objgan_conv_dgrad_s2_phases) would for these arguments".  The
// caller keeps the blobs of all banks it caches for a network back to back in DEVICE memory and refreshes
// them with one launch after the network's weights changed.
int objgan_conv_pack_job_bytes() { return (int)sizeof(PackArgs); }

int objgan_conv_pack_job(void* job, const float* w, float* wt, int N, int C, int H, int W, int Cout, int Cin,
                         int Torig, int transpose, int Tg, const int* src_tap, int PH, int PW, int act, int math) {
    if (!job || Tg < 1 || Tg > OG_MAX_TAPS || Torig < 1 || Torig > 127) return OG_BAD_ARGS;
    if ((transpose ? Cout : Cin) != C) return OG_BAD_ARGS;
    PackArgs p;
    memset(&p, 0, sizeof(p));
    og_fill_pack(p, w, wt, N, C, H, W, Cout, Cin, Torig, transpose, Tg, src_tap, PH, PW, act, math, nullptr);
    memcpy(job, &p, sizeof(p));
    return OG_OK;
}

int objgan_conv_pack_job_phase(void* job, const float* w, float* wt, int Cout, int Cin, int Torig, int Tg,
                               const int* src_tap_phase, int phase, int math) {
    if (!job || Tg < 1 || Tg > 8 || phase < 0 || phase > 3 || Torig < 1 || Torig > 127) return OG_BAD_ARGS;
    PackArgs p;
    memset(&p, 0, sizeof(p));
    og_fill_pack_phase(p, w, wt, Cout, Cin, Torig, Tg, src_tap_phase, phase, math);
    memcpy(job, &p, sizeof(p));
    return OG_OK;
}

// jobs_dev: njobs blobs in device memory.
int objgan_conv_pack_jobs_run(const void* jobs_dev, int njobs, void* stream) {
    OG_ENTRY();
    if (njobs <= 0) return OG_OK;
    if (!jobs_dev || njobs > 65535) return OG_BAD_ARGS;
    // (fp16x2 jobs first leave the partial maxima of their weights behind their banks: the scale of the pack)
    hipLaunchKernelGGL(absmax_w_jobs_kernel, dim3(64, njobs), dim3(256), 0, (hipStream_t)stream, (const PackArgs*)jobs_dev);
    hipLaunchKernelGGL(pack_weights_batched_kernel, dim3(OG_PACK_BLOCKS, njobs), dim3(256), 0, (hipStream_t)stream,
                       (const PackArgs*)jobs_dev);
    return og_launch_status();
}

// Layout of the packed bank objgan_conv_igemm would write / expect for these arguments: low byte = layout class
// (0..4), bits 8.. = chunks per K group of the row-major classes (og_kstep).  A caller that keeps packed banks
// (wt_packed = 1) must key them on this value as well: the same filter can be served by different kernels and K
// orders -- hence different bank layouts -- at different sizes.
int objgan_conv_bank_layout(int N, int C, int H, int W, int M, int Tg, int PH, int PW, int act, int math) {
    const int cls = og_bank_layout(N, C, H, W, M, Tg, PH, PW, act, math, nullptr);
    return (cls == 1 || cls >= 3) ? (cls | (og_kgroup(C, Tg, H, PH) << 8)) : cls;
}

// Size (in floats) of the packed-weight scratch for an M x K GEMM.
long objgan_conv_packed_floats(int M, int C, int T) {
    const long Mpad = ((long)M + 127) / 128 * 128;
    const long Cp = ((long)C + 15) / 16 * 16;
    // the pre-split bank of the bf16x3 mode takes 6 bytes per element; + OG_AMAX_SLOTS floats: partial maxima of |w| (fp16x2)
    return (Mpad * Cp * T * 3 + 1) / 2 + OG_AMAX_SLOTS;
}

// The bf16 channel-blocked copy [N][Cp/16][HW][16] (RNE) of an fp32 [N][C][HW] tensor: what the bf16-mode kernels read
// (math 3).  objgan_nhwc_bf16_floats: its size in floats (0: too large for the 32-bit buffer range -- use math 1).
long objgan_nhwc_bf16_floats(int N, int C, long HW) {
    const long Cp = ((long)C + 15) / 16 * 16;
    if (N <= 0 || C <= 0 || HW <= 0 || (double)N * HW * Cp * 2.0 >= 4.0e9 || HW >= (1L << 31)) return 0;
    return ((long)N * HW * Cp / 2 + 3) & ~3L;
}
int objgan_nhwc_bf16(const float* x, float* out, int N, int C, long HW, void* stream) {
    OG_ENTRY();
    if (!x || !out || objgan_nhwc_bf16_floats(N, C, HW) == 0) return OG_BAD_ARGS;
    og_launch_nhwc_bf16(x, out, N, C, (int)HW, (C + 15) / 16 * 16, (hipStream_t)stream);
    return og_launch_status();
}

}  // extern "C"

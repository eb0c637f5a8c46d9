// Evaluation statistics on the device (reference image_generation/model.py:433-441 and miscc/utils.py:644-657).
//   bilinear_halfpixel : the input preparation of the FID feature network -- F.upsample(mode='bilinear'), i.e. half-pixel
//                        sampling (align_corners=False, no antialiasing), followed by one per-channel affine (the
//                        reference's [-1, 1] -> [0, 1] -> ImageNet re-normalisation, folded).  HBM-bound, one thread
//                        per output element.
//   moments_accumulate : streaming first and second moments of the 2048-d activations in fp64.  The reference keeps
//                        every activation on the host and calls np.cov at the end; here sum [D] and the upper triangle
//                        of outer [D, D] live on the device and every call adds a block of rows.  Every output element
//                        is owned by ONE thread that starts from the stored value and adds the rows in row order:
//                        no atomics, so the result is bit-reproducible and does not depend on how a sequence of rows
//                        is cut into calls.  (The product of two fp32 values is exact in fp64, so each step rounds once.)
//   moments_finalize   : mu = sum / n, sigma = (outer - n mu mu^T) / (n - 1), mirrored to the full symmetric matrix.
#include "common.h"

__global__ __launch_bounds__(256) void bilinear_halfpixel_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                 long total, int C, int H, int W, int OH, int OW,
                                                                 float rh, float rw, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int ow = (int)(e % OW);
        const long r = e / OW;
        const int oh = (int)(r % OH);
        const long plane = r / OH;
        // source index: max(0, (dst + 0.5) * in / out - 0.5); the upper neighbour is clamped to in - 1
        const float sh = fmaxf(rh * ((float)oh + 0.5f) - 0.5f, 0.f);
        const float sw = fmaxf(rw * ((float)ow + 0.5f) - 0.5f, 0.f);
        const int h0 = min((int)sh, H - 1), w0 = min((int)sw, W - 1);
        const int h1 = h0 + (h0 < H - 1 ? 1 : 0), w1 = w0 + (w0 < W - 1 ? 1 : 0);
        const float lh1 = sh - (float)h0, lw1 = sw - (float)w0;
        const float lh0 = 1.f - lh1, lw0 = 1.f - lw1;
        const float* xp = x + plane * (long)H * W;
        float v = lh0 * (lw0 * xp[h0 * W + w0] + lw1 * xp[h0 * W + w1]) +
                  lh1 * (lw0 * xp[h1 * W + w0] + lw1 * xp[h1 * W + w1]);
        if (scale) {
            const int c = (int)(plane % C);
            v = v * scale[c] + shift[c];
        }
        y[e] = v;
    }
}

// One workgroup owns a MT x MT tile of `outer` (tile row bi <= tile column bj); thread (ty, tx) of the 16 x 16 grid owns
// rows bi*MT + 4*ty + {0..3} and columns bj*MT + tx + 16*{0..3} (lanes of a wave walk consecutive columns: conflict-free
// 8-byte LDS reads, 128-byte store segments).  Rows arrive MR at a time through LDS, already converted to fp64.
#define MT 64
#define MR 16

__global__ __launch_bounds__(256) void moments_accumulate_kernel(const float* __restrict__ x, int rows, int D,
                                                                 double* __restrict__ sum, double* __restrict__ outer) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;                                   // entirely below the diagonal (uniform: before any barrier)
    __shared__ double sA[MR][MT];
    __shared__ double sB[MR][MT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = bi * MT, j0 = bj * MT;

    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + 4 * ty + a, j = j0 + tx + 16 * b;
            acc[a][b] = (i < D && j < D && i <= j) ? outer[(long)i * D + j] : 0.0;
        }
    const bool own_sum = (bi == bj) && tid < MT && (i0 + tid) < D;
    double s = own_sum ? sum[i0 + tid] : 0.0;

    for (int r0 = 0; r0 < rows; r0 += MR) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < (MR * MT) / 256; ++k) {
            const int idx = tid + k * 256, r = idx / MT, c = idx % MT;
            const bool row_ok = (r0 + r) < rows;
            const float* xr = x + (long)(r0 + r) * D;
            sA[r][c] = (row_ok && (i0 + c) < D) ? (double)xr[i0 + c] : 0.0;
            sB[r][c] = (row_ok && (j0 + c) < D) ? (double)xr[j0 + c] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < MR; ++r) {                     // rows past the end are zero: fma(0, 0, acc) == acc
            double a[4], b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { a[k] = sA[r][4 * ty + k]; b[k] = sB[r][tx + 16 * k]; }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = fma(a[p], b[q], acc[p][q]);
            if (own_sum) s += sA[r][tid];
        }
    }

#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + 4 * ty + a, j = j0 + tx + 16 * b;
            if (i < D && j < D && i <= j) outer[(long)i * D + j] = acc[a][b];
        }
    if (own_sum) sum[i0 + tid] = s;
}

__global__ __launch_bounds__(256) void moments_finalize_kernel(const double* __restrict__ sum,
                                                               const double* __restrict__ outer, double n, int D,
                                                               double* __restrict__ mu, double* __restrict__ sigma) {
    const long total = (long)D * D;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int i = (int)(e / D), j = (int)(e % D);
        const int lo = min(i, j), hi = max(i, j);          // both mirror images evaluate the SAME expression
        const double mlo = sum[lo] / n, mhi = sum[hi] / n;
        sigma[e] = (outer[(long)lo * D + hi] - n * (mlo * mhi)) / (n - 1.0);
        if (i == j) mu[i] = mlo;
    }
}

extern "C" {

// y[N, C, OH, OW] = F.interpolate(x[N, C, H, W], (OH, OW), 'bilinear', align_corners=False) * scale[c] + shift[c]
// (scale / shift: C floats in device memory, both given or both NULL).
int objgan_bilinear_halfpixel_forward(const float* x, float* y, int N, int C, int H, int W, int OH, int OW,
                                      const float* scale, const float* shift, void* stream) {
    OG_ENTRY();
    if (N < 0 || C < 1 || H < 1 || W < 1 || OH < 1 || OW < 1 || ((scale == nullptr) != (shift == nullptr)))
        return OG_BAD_ARGS;
    const long total = (long)N * C * OH * OW;
    if (total <= 0) return OG_OK;
    if (!x || !y) return OG_BAD_ARGS;
    hipLaunchKernelGGL(bilinear_halfpixel_kernel, dim3(og_stream_grid(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       x, y, total, C, H, W, OH, OW, (float)H / (float)OH, (float)W / (float)OW, scale, shift);
    return og_launch_status();
}

// sum[D] += sum_r x[r], outer[D, D] (upper triangle, diagonal included) += sum_r x[r]^T x[r]; x fp32 [rows, D].
int objgan_moments_accumulate(const float* x, int rows, int D, double* sum, double* outer, void* stream) {
    OG_ENTRY();
    if (rows < 0 || D < 1 || !sum || !outer) return OG_BAD_ARGS;
    if (rows == 0) return OG_OK;
    if (!x) return OG_BAD_ARGS;
    const int T = og_cdiv(D, MT);
    if (T > 65535) return OG_BAD_ARGS;
    hipLaunchKernelGGL(moments_accumulate_kernel, dim3(T, T), dim3(256), 0, (hipStream_t)stream, x, rows, D, sum, outer);
    return og_launch_status();
}

// mu[D] = sum / n; sigma[D, D] = (outer - n mu mu^T) / (n - 1), full symmetric matrix (np.cov's default normalisation).
int objgan_moments_finalize(const double* sum, const double* outer, long n, int D, double* mu, double* sigma,
                            void* stream) {
    OG_ENTRY();
    if (n < 2 || D < 1 || !sum || !outer || !mu || !sigma) return OG_BAD_ARGS;
    hipLaunchKernelGGL(moments_finalize_kernel, dim3(og_stream_grid((long)D * D, 256)), dim3(256), 0,
                       (hipStream_t)stream, sum, outer, (double)n, D, mu, sigma);
    return og_launch_status();
}

}  // extern "C"

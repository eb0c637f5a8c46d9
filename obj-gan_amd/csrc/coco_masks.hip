// Instance masks of the annotation preprocessing on the device (reference image_generation/miscc/load.py:608-622 and
// shape_generation/datasets.py:347-361): per instance
//     COCO.segToMask(rings, H, W)  ->  astype(float)  ->  skimage.transform.resize(mask, [S, S])
// i.e. one full-size polygon rasterisation and one full-size float64 Gaussian blur per instance on the host.  Here a
// batch of instances of different image sizes goes through three launches and only out[A][S][S] comes back:
//   1. poly_raster_kernel: the even-odd rule of skimage's point_in_polygon, in float64 at integer pixel coordinates.  For
//      an edge (i, j = i - 1) that straddles row y, the pixels x < (xp[j] - xp[i]) * (y - yp[i]) / (yp[j] - yp[i]) + xp[i]
//      toggle; the abscissa does not depend on x, and for integer x `x < a` is `x < ceil(a)`, so an edge toggles the prefix
//      [0, ceil(a)) of the row.  One thread owns one 32-pixel word of the bit plane: XOR per ring, OR over the rings.
//   2. poly_range_kernel: whether the mask has a set and a clear pixel (its maximum and minimum, the clip bounds).
//   3. poly_resize_kernel: one workgroup per output row.  The order-1 zoom reads two rows and 2 S columns of the blurred
//      image; axis 0 of the Gaussian is evaluated for those two rows only (all columns, in LDS), axis 1 at the 2 S
//      columns, then the four-term interpolation and the clip -- each value by the operations scipy.ndimage performs, in
//      its order (NI_Correlate1D symmetric branch; NI_ZoomShift order 1, grid_mode, mode 'mirror'; see
//      oracle/mask_resize.py for the square case).  Built with -ffp-contract=off: no fused multiply-add.
// No atomics; every element of out is written.
#include "common.h"

#define POLY_MAX_S 64
#define POLY_MAX_SIDE 1024
#define POLY_MAX_TAPS 65

struct PolyArgs {
    const double* verts;
    const int* ring_off;
    const int* inst_ring;
    const int* hs;
    const int* ws;
    const double* taps;
    const int* tap_off;
    double* out;
    unsigned* bits;         // [A][Hmax * wprmax]: instance a's rows packed at its own ceil(W / 32) words per row
    int* range;             // [A][2] = {some pixel set, every pixel set}
    long nverts;
    int nrings, A, Hmax, Wmax, S, ntaps_total, wprmax;
};

__device__ __forceinline__ bool poly_size_ok(const PolyArgs& a, int H, int W) {
    return H >= 1 && H <= a.Hmax && W >= 1 && W <= a.Wmax;
}

__global__ __launch_bounds__(256) void poly_raster_kernel(const PolyArgs a) {
    const int inst = blockIdx.y;
    const int H = a.hs[inst], W = a.ws[inst];
    if (!poly_size_ok(a, H, W)) return;
    const int wpr = (W + 31) >> 5;
    const int item = blockIdx.x * 256 + threadIdx.x;
    if (item >= H * wpr) return;
    const int row = item / wpr, word = item - row * wpr;
    const double y = (double)row;
    const int x0 = word * 32;
    int r0 = a.inst_ring[inst], r1 = a.inst_ring[inst + 1];
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > a.nrings ? a.nrings : r1;
    unsigned acc = 0u;
    for (int r = r0; r < r1; ++r) {
        const long v0 = a.ring_off[r], v1 = a.ring_off[r + 1];
        if (v0 < 0 || v1 > a.nverts || v1 <= v0) continue;
        unsigned m = 0u;
        double xj = a.verts[2 * (v1 - 1)], yj = a.verts[2 * (v1 - 1) + 1];
        for (long i = v0; i < v1; ++i) {
            const double xi = a.verts[2 * i], yi = a.verts[2 * i + 1];
            if ((yi <= y && y < yj) || (yj <= y && y < yi)) {
                const double kd = ceil((xj - xi) * (y - yi) / (yj - yi) + xi);
                int k = kd <= 0.0 ? 0 : (kd >= (double)W ? W : (int)kd);
                k -= x0;
                if (k > 0) m ^= k >= 32 ? 0xffffffffu : (1u << k) - 1u;
            }
            xj = xi;
            yj = yi;
        }
        acc |= m;
    }
    a.bits[(size_t)inst * a.Hmax * a.wprmax + item] = acc;
}

__global__ __launch_bounds__(256) void poly_range_kernel(const PolyArgs a) {
    __shared__ unsigned red[2][4];
    const int inst = blockIdx.x, tid = threadIdx.x;
    const int H = a.hs[inst], W = a.ws[inst];
    if (!poly_size_ok(a, H, W)) return;             // uniform over the workgroup
    const int wpr = (W + 31) >> 5;
    const unsigned* bits = a.bits + (size_t)inst * a.Hmax * a.wprmax;
    const unsigned tail = (W & 31) ? ~((1u << (W & 31)) - 1u) : 0u;      // the bits past column W - 1 of a row's last word
    unsigned any = 0u, all = 0xffffffffu;
    for (int i = tid; i < H * wpr; i += 256) {
        const unsigned w = bits[i];
        any |= w;
        all &= (i % wpr == wpr - 1) ? (w | tail) : w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        any |= __shfl_xor(any, o, 64);
        all &= __shfl_xor(all, o, 64);
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = any; red[1][tid >> 6] = all; }
    __syncthreads();
    if (tid == 0) {
        a.range[inst * 2 + 0] = (red[0][0] | red[0][1] | red[0][2] | red[0][3]) != 0u;
        a.range[inst * 2 + 1] = (red[1][0] & red[1][1] & red[1][2] & red[1][3]) == 0xffffffffu;
    }
}

__device__ __forceinline__ int poly_mirror(int i, int n) {      // d c b | a b c d | c b a
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

__device__ __forceinline__ double poly_map_mirror(double c, int n) {      // map_coordinate, NI_EXTEND_MIRROR
    if (n <= 1) return 0.0;
    const int sz2 = 2 * n - 2;
    if (c < 0) {
        c = sz2 * (double)(int)(-c / sz2) + c;
        c = c <= 1 - n ? c + sz2 : -c;
    } else if (c > n - 1) {
        c -= sz2 * (double)(int)(c / sz2);
        if (c >= n) c = sz2 - c;
    }
    return c;
}

// the two source indices and weights of output index o of an axis of n samples zoomed to S
__device__ __forceinline__ void poly_zoom_taps(int o, int n, int S, int* i0, int* i1, double* w0, double* w1) {
    const double zoom = (double)n / (double)S;
    const double c = poly_map_mirror(((double)o + 0.5) * zoom - 0.5, n);
    const int i = (int)floor(c);
    *w1 = c - i;
    *w0 = 1.0 - *w1;
    *i0 = poly_mirror(i, n);
    *i1 = poly_mirror(i + 1, n);
}

__global__ __launch_bounds__(256) void poly_resize_kernel(const PolyArgs a) {
    __shared__ double T[2][POLY_MAX_SIDE];              // axis-0 filtered rows i0, i1 of this output row
    __shared__ double Bc[2][POLY_MAX_S][2];             // then axis 1 at the columns j0, j1 of every output column
    __shared__ double tap[2][POLY_MAX_TAPS];
    __shared__ int rowidx[2][POLY_MAX_TAPS];            // mirrored source rows i + jj, jj = -c .. c, of i0 and i1
    const int oy = blockIdx.x, inst = blockIdx.y, tid = threadIdx.x;
    const int S = a.S;
    double* out = a.out + ((size_t)inst * S + oy) * S;
    const int H = a.hs[inst], W = a.ws[inst];
    const int* to = a.tap_off + inst * 4;
    const int off0 = to[0], nt0 = to[1], off1 = to[2], nt1 = to[3];
    const bool taps_ok = nt0 >= 0 && nt0 <= POLY_MAX_TAPS && nt1 >= 0 && nt1 <= POLY_MAX_TAPS &&
                         (nt0 == 0 || ((nt0 & 1) && off0 >= 0 && off0 + nt0 <= a.ntaps_total)) &&
                         (nt1 == 0 || ((nt1 & 1) && off1 >= 0 && off1 + nt1 <= a.ntaps_total));
    if (!poly_size_ok(a, H, W) || !taps_ok) {           // uniform over the workgroup: a table that contradicts the call
        if (tid < S) out[tid] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const int wpr = (W + 31) >> 5;
    const unsigned* bits = a.bits + (size_t)inst * a.Hmax * a.wprmax;
    int i0, i1;
    double wy0, wy1;
    poly_zoom_taps(oy, H, S, &i0, &i1, &wy0, &wy1);
    const int c0 = nt0 / 2, c1 = nt1 / 2;
    if (tid < nt0) tap[0][tid] = a.taps[off0 + tid];
    if (tid >= 64 && tid - 64 < nt1) tap[1][tid - 64] = a.taps[off1 + tid - 64];
    for (int e = tid; e < 2 * nt0; e += 256) {
        const int s = e >= nt0, t = e - s * nt0;
        rowidx[s][t] = poly_mirror((s ? i1 : i0) + t - c0, H);
    }
    __syncthreads();
    for (int e = tid; e < 2 * W; e += 256) {
        const int s = e >= W, q = e - s * W;
        const unsigned sh = q & 31;
        const unsigned* col = bits + (q >> 5);
        double tmp;
        if (nt0 > 0) {
            tmp = (double)((col[(size_t)rowidx[s][c0] * wpr] >> sh) & 1u) * tap[0][c0];
            for (int jj = -c0; jj < 0; ++jj) {
                const double x0 = (double)((col[(size_t)rowidx[s][c0 + jj] * wpr] >> sh) & 1u);
                const double x1 = (double)((col[(size_t)rowidx[s][c0 - jj] * wpr] >> sh) & 1u);
                tmp = tmp + (x0 + x1) * tap[0][jj + c0];
            }
        } else {
            tmp = (double)((col[(size_t)(s ? i1 : i0) * wpr] >> sh) & 1u);
        }
        T[s][q] = tmp;
    }
    __syncthreads();
    if (tid < 4 * S) {                                  // 4 S <= 256: one value per thread
        const int s = tid / (2 * S), ox = (tid - s * 2 * S) >> 1, k = tid & 1;
        int j0, j1;
        double wx0, wx1;
        poly_zoom_taps(ox, W, S, &j0, &j1, &wx0, &wx1);
        const int j = k ? j1 : j0;
        double tmp;
        if (nt1 > 0) {
            tmp = T[s][j] * tap[1][c1];
            for (int jj = -c1; jj < 0; ++jj)
                tmp = tmp + (T[s][poly_mirror(j + jj, W)] + T[s][poly_mirror(j - jj, W)]) * tap[1][jj + c1];
        } else {
            tmp = T[s][j];
        }
        Bc[s][ox][k] = tmp;
    }
    __syncthreads();
    if (tid < S) {
        int j0, j1;
        double wx0, wx1;
        poly_zoom_taps(tid, W, S, &j0, &j1, &wx0, &wx1);
        const double lo = a.range[inst * 2 + 1] ? 1.0 : 0.0, hi = a.range[inst * 2 + 0] ? 1.0 : 0.0;
        double t = 0.0;
        t += (Bc[0][tid][0] * wy0) * wx0;
        t += (Bc[0][tid][1] * wy0) * wx1;
        t += (Bc[1][tid][0] * wy1) * wx0;
        t += (Bc[1][tid][1] * wy1) * wx1;
        t = t < lo ? lo : t;
        t = t > hi ? hi : t;
        out[tid] = t;
    }
}

extern "C" {

int objgan_poly_masks_covers(int H, int W, int S, int ntaps0, int ntaps1) {
    return H >= 1 && W >= 1 && H <= POLY_MAX_SIDE && W <= POLY_MAX_SIDE && S >= 1 && S <= POLY_MAX_S && ntaps0 >= 0 &&
           ntaps1 >= 0 && ntaps0 <= POLY_MAX_TAPS && ntaps1 <= POLY_MAX_TAPS && (ntaps0 == 0 || (ntaps0 & 1)) &&
           (ntaps1 == 0 || (ntaps1 & 1));
}

static long poly_bits_bytes(int A, int Hmax, int Wmax) {
    return (((long)A * Hmax * ((Wmax + 31) >> 5) * 4) + 255) / 256 * 256;
}

long objgan_poly_masks_plan(int A, int Hmax, int Wmax) {
    if (A < 1 || A > 65535 || Hmax < 1 || Wmax < 1 || Hmax > POLY_MAX_SIDE || Wmax > POLY_MAX_SIDE) return 0;
    return poly_bits_bytes(A, Hmax, Wmax) + (long)A * 2 * sizeof(int);
}

int objgan_poly_masks(const double* verts, long nverts, const int* ring_off, const int* inst_ring, int nrings,
                      const int* hs, const int* ws, int A, int Hmax, int Wmax, int S, const double* taps,
                      const int* tap_off, int ntaps_total, double* out, void* ws_buf, long ws_bytes, void* stream) {
    OG_ENTRY();
    if (A == 0) return OG_OK;
    const long need = objgan_poly_masks_plan(A, Hmax, Wmax);
    if (need == 0 || S < 1 || S > POLY_MAX_S || !ring_off || !inst_ring || !hs || !ws || !tap_off || !out || !ws_buf ||
        ws_bytes < need || nrings < 0 || nverts < 0 || ntaps_total < 0 || (nverts > 0 && !verts) ||
        (ntaps_total > 0 && !taps))
        return OG_BAD_ARGS;
    PolyArgs a;
    a.verts = verts; a.ring_off = ring_off; a.inst_ring = inst_ring; a.hs = hs; a.ws = ws; a.taps = taps;
    a.tap_off = tap_off; a.out = out;
    a.bits = (unsigned*)ws_buf;
    a.range = (int*)((char*)ws_buf + poly_bits_bytes(A, Hmax, Wmax));
    a.nverts = nverts; a.nrings = nrings; a.A = A; a.Hmax = Hmax; a.Wmax = Wmax; a.S = S; a.ntaps_total = ntaps_total;
    a.wprmax = (Wmax + 31) >> 5;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(poly_raster_kernel, dim3(og_cdiv((long)Hmax * a.wprmax, 256), A), dim3(256), 0, s, a);
    hipLaunchKernelGGL(poly_range_kernel, dim3(A), dim3(256), 0, s, a);
    hipLaunchKernelGGL(poly_resize_kernel, dim3(S, A), dim3(256), 0, s, a);
    return og_launch_status();
}

}  // extern "C"

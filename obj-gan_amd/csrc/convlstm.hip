// Shape generator training (reference shape_generation/model.py:81-128, miscc/losses.py:58-60, datasets.py:99-111):
// the point-wise part of the ConvLSTM cell, forward and backward, the max over the box axis with its first-argmax
// gradient, and the one-hot box maps written on the device.  fp32 VALU, 16-byte accesses where the extents allow them
// (V = 4: HW and every stride a multiple of four floats, every pointer 16-byte aligned), scalar accesses otherwise.
// No float atomics: every output element is written by exactly one lane.
#include "common.h"

namespace {

// V floats moved as one access: 16 bytes for V = 4
template <int V> struct alignas(4 * V) vecf { float a[V]; };
template <int V> struct vec_t { typedef vecf<V> type; };

template <int V> __device__ __forceinline__ vecf<V> ld(const float* p) { return *reinterpret_cast<const vecf<V>*>(p); }
template <int V> __device__ __forceinline__ void st(float* p, const vecf<V>& v) { *reinterpret_cast<vecf<V>*>(p) = v; }
template <int V> __device__ __forceinline__ float& el(vecf<V>& v, int i) { return v.a[i]; }
template <int V> __device__ __forceinline__ void add(vecf<V>& v, const vecf<V>& w) {
#pragma unroll
    for (int j = 0; j < V; ++j) v.a[j] += w.a[j];
}

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// One item = V consecutive pixels of one (image, hidden channel) plane.
//   gates (pre-activation) = gx[b][k Ch + ch] (+ gh[b][k Ch + ch]), k = in, remember, out, cell
//   c = sig(rem) c_prev + sig(in) tanh(cell);  h = sig(out) tanh(c)
//   acts[b][5 Ch]: the four activated gates, then tanh(c)
template <int V>
__global__ __launch_bounds__(256) void cell_forward_kernel(
    const float* __restrict__ gx, const float* __restrict__ gh, const float* __restrict__ c_prev,
    float* __restrict__ h_out, float* __restrict__ h_slab, float* __restrict__ c_out, float* __restrict__ acts,
    int B, int Ch, int HW, long gx_bs, long slab_bs) {
    typedef typename vec_t<V>::type vt;
    const int HWv = HW / V;
    const long items = (long)B * Ch * HWv;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < items; idx += (long)gridDim.x * blockDim.x) {
        const int p = (int)(idx % HWv) * V;
        const long bc = idx / HWv;
        const int ch = (int)(bc % Ch);
        const long b = bc / Ch;
        const long plane = (long)ch * HW + p;
        const long chw = (long)Ch * HW;
        vt g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            g[k] = ld<V>(gx + b * gx_bs + k * chw + plane);
            if (gh) add<V>(g[k], ld<V>(gh + b * 4 * chw + k * chw + plane));
        }
        vt cp;
        if (c_prev) cp = ld<V>(c_prev + b * chw + plane);
        vt c, h, tc;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float gi = sigm(el<V>(g[0], j)), gf = sigm(el<V>(g[1], j)), go = sigm(el<V>(g[2], j));
            const float gc = tanhf(el<V>(g[3], j));
            const float cv = (c_prev ? gf * el<V>(cp, j) : 0.f) + gi * gc;
            const float t = tanhf(cv);
            el<V>(g[0], j) = gi; el<V>(g[1], j) = gf; el<V>(g[2], j) = go; el<V>(g[3], j) = gc;
            el<V>(c, j) = cv; el<V>(tc, j) = t; el<V>(h, j) = go * t;
        }
        st<V>(h_out + b * chw + plane, h);
        st<V>(h_slab + b * slab_bs + plane, h);
        st<V>(c_out + b * chw + plane, c);
#pragma unroll
        for (int k = 0; k < 4; ++k) st<V>(acts + b * 5 * chw + k * chw + plane, g[k]);
        st<V>(acts + b * 5 * chw + 4 * chw + plane, tc);
    }
}

// dh = dh_slab[b] (+ dh_rec[b]);  dc = dc_in + dh o (1 - tanh(c)^2);  pre-activation gate gradients in the gate order
// of the forward pass, written twice: into slot t of the batch-major slab (dg_slab, batch stride dg_bs) and into the
// contiguous [B][4 Ch] block the hidden-part convolutions of this step read;  dc_prev = dc f.
template <int V>
__global__ __launch_bounds__(256) void cell_backward_kernel(
    const float* __restrict__ dh_slab, const float* __restrict__ dh_rec, const float* __restrict__ dc_in,
    const float* __restrict__ acts, const float* __restrict__ c_prev,
    float* __restrict__ dg_slab, float* __restrict__ dg_out, float* __restrict__ dc_out,
    int B, int Ch, int HW, long dh_bs, long dg_bs) {
    typedef typename vec_t<V>::type vt;
    const int HWv = HW / V;
    const long items = (long)B * Ch * HWv;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < items; idx += (long)gridDim.x * blockDim.x) {
        const int p = (int)(idx % HWv) * V;
        const long bc = idx / HWv;
        const int ch = (int)(bc % Ch);
        const long b = bc / Ch;
        const long plane = (long)ch * HW + p;
        const long chw = (long)Ch * HW;
        vt dh = ld<V>(dh_slab + b * dh_bs + plane);
        if (dh_rec) add<V>(dh, ld<V>(dh_rec + b * chw + plane));
        vt a[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) a[k] = ld<V>(acts + b * 5 * chw + k * chw + plane);
        vt dci, cp;
        if (dc_in) dci = ld<V>(dc_in + b * chw + plane);
        if (c_prev) cp = ld<V>(c_prev + b * chw + plane);
        vt d[4], dcp;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float gi = el<V>(a[0], j), gf = el<V>(a[1], j), go = el<V>(a[2], j), gc = el<V>(a[3], j);
            const float t = el<V>(a[4], j), dhv = el<V>(dh, j);
            const float dc = (dc_in ? el<V>(dci, j) : 0.f) + dhv * go * (1.f - t * t);
            el<V>(d[0], j) = dc * gc * gi * (1.f - gi);
            el<V>(d[1], j) = c_prev ? dc * el<V>(cp, j) * gf * (1.f - gf) : 0.f;
            el<V>(d[2], j) = dhv * t * go * (1.f - go);
            el<V>(d[3], j) = dc * gi * (1.f - gc * gc);
            el<V>(dcp, j) = dc * gf;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            st<V>(dg_slab + b * dg_bs + k * chw + plane, d[k]);
            st<V>(dg_out + b * 4 * chw + k * chw + plane, d[k]);
        }
        st<V>(dc_out + b * chw + plane, dcp);
    }
}

// y[b][i] = max_r x[b][r][i], arg[b][i] = the FIRST r that attains it (torch.max on the CPU); a NaN, once met, stays
// (torch propagates NaN).  i runs over the CSS elements of a box's maps.
template <int V>
__global__ __launch_bounds__(256) void box_max_forward_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                              uint8_t* __restrict__ arg, int B, int R, long CSS) {
    typedef typename vec_t<V>::type vt;
    const long per = CSS / V, items = (long)B * per;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < items; idx += (long)gridDim.x * blockDim.x) {
        const long b = idx / per, i = (idx % per) * V;
        const float* xb = x + b * R * CSS + i;
        vt m = ld<V>(xb);
        uint8_t am[V];
#pragma unroll
        for (int j = 0; j < V; ++j) am[j] = 0;
        for (int r = 1; r < R; ++r) {
            vt v = ld<V>(xb + (long)r * CSS);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float cur = el<V>(m, j), nv = el<V>(v, j);
                if ((nv > cur || nv != nv) && cur == cur) { el<V>(m, j) = nv; am[j] = (uint8_t)r; }
            }
        }
        st<V>(y + b * CSS + i, m);
        if (arg) {
#pragma unroll
            for (int j = 0; j < V; ++j) arg[b * CSS + i + j] = am[j];
        }
    }
}

// dx[b][r][i] = dy[b][i] where r == arg[b][i], zero elsewhere: every element of dx is written.
template <int V>
__global__ __launch_bounds__(256) void box_max_backward_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ arg,
                                                               float* __restrict__ dx, int B, int R, long CSS) {
    typedef typename vec_t<V>::type vt;
    const long per = CSS / V, items = (long)B * R * per;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < items; idx += (long)gridDim.x * blockDim.x) {
        const long i = (idx % per) * V;
        const long br = idx / per;
        const int r = (int)(br % R);
        const long b = br / R;
        vt g = ld<V>(dy + b * CSS + i);
        vt o;
#pragma unroll
        for (int j = 0; j < V; ++j) el<V>(o, j) = (arg[b * CSS + i + j] == r) ? el<V>(g, j) : 0.f;
        st<V>(dx + br * CSS + i, o);
    }
}

// fwd[b][r][c] = raw[b][r] if r < num[b] and c == cat[b][r], else 0;  bwd[b][r] = fwd over all NB slots reversed
// (slot NB - 1 - r), then cut to R: an image with fewer than NB boxes sees leading zero maps there.
template <int V>
__global__ __launch_bounds__(256) void boxmaps_onehot_kernel(const float* __restrict__ raw, const int* __restrict__ cat,
                                                             const int* __restrict__ num, float* __restrict__ fwd,
                                                             float* __restrict__ bwd, int B, int NB, int R, int C, int SS) {
    typedef typename vec_t<V>::type vt;
    const int SSv = SS / V;
    const long items = (long)B * R * C * SSv;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < items; idx += (long)gridDim.x * blockDim.x) {
        const int p = (int)(idx % SSv) * V;
        long q = idx / SSv;
        const int c = (int)(q % C); q /= C;
        const int r = (int)(q % R);
        const int b = (int)(q / R);
        const int n = num[b];
        vt f, w;
#pragma unroll
        for (int j = 0; j < V; ++j) { el<V>(f, j) = 0.f; el<V>(w, j) = 0.f; }
        if (r < n && r < NB && cat[b * NB + r] == c) f = ld<V>(raw + ((long)b * NB + r) * SS + p);
        const int s = NB - 1 - r;
        if (s >= 0 && s < n && cat[b * NB + s] == c) w = ld<V>(raw + ((long)b * NB + s) * SS + p);
        st<V>(fwd + idx * V, f);
        st<V>(bwd + idx * V, w);
    }
}

inline bool al16(const void* p) { return p == nullptr || (((uintptr_t)p) & 15) == 0; }

}  // namespace

extern "C" int objgan_convlstm_cell_forward(const float* gx, const float* gh, const float* c_prev, float* h_out,
                                            float* h_slab, float* c_out, float* acts, int B, int Ch, int HW,
                                            long gx_bstride, long slab_bstride, void* stream) {
    OG_ENTRY();
    if (!gx || !h_out || !h_slab || !c_out || !acts || B <= 0 || Ch <= 0 || HW <= 0) return OG_BAD_ARGS;
    if (gx_bstride < 4L * Ch * HW || slab_bstride < (long)Ch * HW) return OG_BAD_ARGS;
    const bool v4 = HW % 4 == 0 && gx_bstride % 4 == 0 && slab_bstride % 4 == 0 && al16(gx) && al16(gh) && al16(c_prev) &&
                    al16(h_out) && al16(h_slab) && al16(c_out) && al16(acts);
    const long items = (long)B * Ch * (v4 ? HW / 4 : HW);
    const int grid = og_stream_grid(items, 256);
    hipStream_t s = (hipStream_t)stream;
    if (v4)
        hipLaunchKernelGGL(cell_forward_kernel<4>, dim3(grid), dim3(256), 0, s, gx, gh, c_prev, h_out, h_slab, c_out, acts,
                           B, Ch, HW, gx_bstride, slab_bstride);
    else
        hipLaunchKernelGGL(cell_forward_kernel<1>, dim3(grid), dim3(256), 0, s, gx, gh, c_prev, h_out, h_slab, c_out, acts,
                           B, Ch, HW, gx_bstride, slab_bstride);
    return og_launch_status();
}

extern "C" int objgan_convlstm_cell_backward(const float* dh_slab, const float* dh_rec, const float* dc_in,
                                             const float* acts, const float* c_prev, float* dg_slab, float* dg_out,
                                             float* dc_out, int B, int Ch, int HW, long dh_bstride, long dg_bstride,
                                             void* stream) {
    OG_ENTRY();
    if (!dh_slab || !acts || !dg_slab || !dg_out || !dc_out || B <= 0 || Ch <= 0 || HW <= 0) return OG_BAD_ARGS;
    if (dh_bstride < (long)Ch * HW || dg_bstride < 4L * Ch * HW) return OG_BAD_ARGS;
    const bool v4 = HW % 4 == 0 && dh_bstride % 4 == 0 && dg_bstride % 4 == 0 && al16(dh_slab) && al16(dh_rec) &&
                    al16(dc_in) && al16(acts) && al16(c_prev) && al16(dg_slab) && al16(dg_out) && al16(dc_out);
    const long items = (long)B * Ch * (v4 ? HW / 4 : HW);
    const int grid = og_stream_grid(items, 256);
    hipStream_t s = (hipStream_t)stream;
    if (v4)
        hipLaunchKernelGGL(cell_backward_kernel<4>, dim3(grid), dim3(256), 0, s, dh_slab, dh_rec, dc_in, acts, c_prev,
                           dg_slab, dg_out, dc_out, B, Ch, HW, dh_bstride, dg_bstride);
    else
        hipLaunchKernelGGL(cell_backward_kernel<1>, dim3(grid), dim3(256), 0, s, dh_slab, dh_rec, dc_in, acts, c_prev,
                           dg_slab, dg_out, dc_out, B, Ch, HW, dh_bstride, dg_bstride);
    return og_launch_status();
}

extern "C" int objgan_box_max_forward(const float* x, float* y, unsigned char* arg, int B, int R, long CSS, void* stream) {
    OG_ENTRY();
    if (!x || !y || B <= 0 || R <= 0 || R > 255 || CSS <= 0) return OG_BAD_ARGS;
    const bool v4 = CSS % 4 == 0 && al16(x) && al16(y);
    const long items = (long)B * (v4 ? CSS / 4 : CSS);
    const int grid = og_stream_grid(items, 256);
    hipStream_t s = (hipStream_t)stream;
    if (v4) hipLaunchKernelGGL(box_max_forward_kernel<4>, dim3(grid), dim3(256), 0, s, x, y, arg, B, R, CSS);
    else hipLaunchKernelGGL(box_max_forward_kernel<1>, dim3(grid), dim3(256), 0, s, x, y, arg, B, R, CSS);
    return og_launch_status();
}

extern "C" int objgan_box_max_backward(const float* dy, const unsigned char* arg, float* dx, int B, int R, long CSS,
                                       void* stream) {
    OG_ENTRY();
    if (!dy || !arg || !dx || B <= 0 || R <= 0 || R > 255 || CSS <= 0) return OG_BAD_ARGS;
    const bool v4 = CSS % 4 == 0 && al16(dy) && al16(dx);
    const long items = (long)B * R * (v4 ? CSS / 4 : CSS);
    const int grid = og_stream_grid(items, 256);
    hipStream_t s = (hipStream_t)stream;
    if (v4) hipLaunchKernelGGL(box_max_backward_kernel<4>, dim3(grid), dim3(256), 0, s, dy, arg, dx, B, R, CSS);
    else hipLaunchKernelGGL(box_max_backward_kernel<1>, dim3(grid), dim3(256), 0, s, dy, arg, dx, B, R, CSS);
    return og_launch_status();
}

extern "C" int objgan_boxmaps_onehot(const float* raw, const int* cat, const int* num, float* fwd, float* bwd, int B,
                                     int NB, int R, int C, int SS, void* stream) {
    OG_ENTRY();
    if (!raw || !cat || !num || !fwd || !bwd || B <= 0 || NB <= 0 || R <= 0 || R > NB || C <= 0 || SS <= 0)
        return OG_BAD_ARGS;
    const bool v4 = SS % 4 == 0 && al16(raw) && al16(fwd) && al16(bwd);
    const long items = (long)B * R * C * (v4 ? SS / 4 : SS);
    const int grid = og_stream_grid(items, 256);
    hipStream_t s = (hipStream_t)stream;
    if (v4) hipLaunchKernelGGL(boxmaps_onehot_kernel<4>, dim3(grid), dim3(256), 0, s, raw, cat, num, fwd, bwd, B, NB, R, C, SS);
    else hipLaunchKernelGGL(boxmaps_onehot_kernel<1>, dim3(grid), dim3(256), 0, s, raw, cat, num, fwd, bwd, B, NB, R, C, SS);
    return og_launch_status();
}

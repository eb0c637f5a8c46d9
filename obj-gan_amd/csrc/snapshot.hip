// Caption / attention snapshot grids composed on the device (reference image_generation/miscc/utils.py:59-306,
// build_super_images and build_super_shape_images): only the finished uint8 grid leaves the device.
//
// For each of the first `nvis` images the grid holds `font_max` rows of caption strip (copied from an uploaded buffer), one
// line  [lr image | 2-px pad | panel 0 | pad | ... | panel max_word_num | pad]  and one line  [image | pad | merged 0 | ...];
// panel 0 is the maximum over the attention maps of the image, panels 1..T are the maps, panels past T are zeros.
//
//   expansion      skimage.transform.pyramid_expand(map, sigma=20, upscale=vis / a) as scipy.ndimage evaluates it: an
//                  order-1 grid-mode zoom (mode 'mirror') followed by gaussian_filter(sigma 20, truncate 4, mode 'mirror').
//                  Both are linear and separable, so an a x a map expands to M A M^T with one [vis, a] fp64 matrix M that
//                  the caller builds once per (a, vis) -- zoom weights and the 161-tap Gaussian with all its mirror
//                  reflections folded in.  Two small tiled fp64 products per panel: R = A M^T, E = M R.
//   normalisation  (v - min) / (max - min) * 255, truncated; min / max over all maps of an image with the reference's
//                  starting values 1 / 0 (build_super_images), or per panel and skipped where max == min
//                  (build_super_shape_images).  Expanded maps are normalised in fp64 (scipy's result type); maps drawn at
//                  their own size (vis == a) in fp32, the reference's numpy dtype on that path.  Minima and maxima are
//                  exact whatever the order; they are still combined in a fixed order, tile by tile, without atomics.
//                  max == min in the global form: the reference divides 0 by 0 and casts NaN to uint8 (undefined); here
//                  the panel is written as 0.
//                  The shape stage's two forms (reference shape_generation/miscc/utils.py:59-300), maps drawn at their own
//                  size only: raw, trunc(v * 255) in fp32 with no minimum or maximum (build_super_images2; masks are in
//                  [0, 1], outside it the reference's cast is undefined and the byte saturates to 0 / 255 here), and per
//                  panel without the guard (build_super_images there): a panel with max == min is the reference's 0 / 0
//                  and is written as 0, like the global form -- every empty box slot is such a panel.
//   image panels   nn.Upsample(size=vis, mode='bilinear'), i.e. half-pixel sampling (the arithmetic of
//                  objgan_bilinear_halfpixel_forward), then (x + 1) / 2 * 255 as three separately rounded fp32 operations
//                  (the build sets -ffp-contract=off for this file), truncated.
//   merged panels  Pillow's paste(att, (0, 0), mask = L 210) over the image byte: og_paste_blend_210 below, the integer
//                  blend of Pillow's Paste.c (tests pin the table it generates against the installed Pillow, all pairs).
#include "common.h"

#define SNAP_TILE 16
#define SNAP_MASK 210

// Pillow's BLEND8(mask, in1, in2) = DIV255(in1 * (255 - mask) + in2 * mask) with DIV255(a) = ((t >> 8) + t) >> 8,
// t = a + 128: the image byte `im` under the attention byte `att` pasted through a constant mask of 210.
__host__ __device__ static inline unsigned char og_paste_blend_210(unsigned im, unsigned att) {
    const unsigned t = im * (255u - SNAP_MASK) + att * SNAP_MASK + 128u;
    return (unsigned char)(((t >> 8) + t) >> 8);
}

// maps of image n: counts[n] clamped to [1, T], or T without a table
__device__ __forceinline__ int snap_count(const int* __restrict__ counts, int n, int T) {
    return counts ? max(1, min(counts[n], T)) : T;
}

// value of map `j` of image n at flat position e of its a x a grid: j = 0 is the maximum over the T maps
__device__ __forceinline__ double snap_map_value(const float* __restrict__ attn_n, int T, int aa, int j, int e) {
    if (j > 0) return (double)attn_n[(long)(j - 1) * aa + e];
    float m = attn_n[e];
    for (int t = 1; t < T; ++t) m = fmaxf(m, attn_n[(long)t * aa + e]);
    return (double)m;
}

// min / max of a workgroup's values (256 threads), written by thread 0 into part[0 .. 1]
__device__ __forceinline__ void snap_block_minmax(double mn, double mx, double* __restrict__ part) {
    __shared__ double smn[256], smx[256];
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    smn[tid] = mn;
    smx[tid] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            smn[tid] = fmin(smn[tid], smn[tid + s]);
            smx[tid] = fmax(smx[tid], smx[tid + s]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        part[0] = smn[0];
        part[1] = smx[0];
    }
}

// R[n][j][p][x] = sum_q A[n][j][p][q] * M[x][q]            (p < a, x < vis)
__global__ __launch_bounds__(256) void snap_expand_cols_kernel(const float* __restrict__ attn, const double* __restrict__ M,
                                                               double* __restrict__ R, const int* __restrict__ counts,
                                                               int T, int a, int vis) {
    __shared__ double sA[SNAP_TILE][SNAP_TILE + 1];
    __shared__ double sM[SNAP_TILE][SNAP_TILE + 1];
    const int P = T + 1, panel = blockIdx.z, n = panel / P, j = panel % P;
    const int Tn = snap_count(counts, n, T);
    if (j > Tn) return;                                             // (whole workgroup: no map in this slot)
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int x = blockIdx.x * SNAP_TILE + tx, p = blockIdx.y * SNAP_TILE + ty;
    const float* attn_n = attn + (long)n * T * a * a;
    double acc = 0.0;
    for (int q0 = 0; q0 < a; q0 += SNAP_TILE) {
        const int qa = q0 + tx;                                     // sA[ty][tx] = A[p][q0 + tx]
        sA[ty][tx] = (p < a && qa < a) ? snap_map_value(attn_n, Tn, a * a, j, p * a + qa) : 0.0;
        const int xm = blockIdx.x * SNAP_TILE + ty;                 // sM[ty][tx] = M[x-tile row ty][q0 + tx]
        sM[ty][tx] = (xm < vis && qa < a) ? M[(long)xm * a + qa] : 0.0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SNAP_TILE; ++k) acc = fma(sA[ty][k], sM[tx][k], acc);
        __syncthreads();
    }
    if (p < a && x < vis) R[((long)panel * a + p) * vis + x] = acc;
}

// E[n][j][y][x] = sum_p M[y][p] * R[n][j][p][x]; the tile's minimum / maximum -> part[panel][tile][2]
__global__ __launch_bounds__(256) void snap_expand_rows_kernel(const double* __restrict__ M, const double* __restrict__ R,
                                                               double* __restrict__ E, double* __restrict__ part,
                                                               const int* __restrict__ counts, int T, int a, int vis) {
    __shared__ double sM[SNAP_TILE][SNAP_TILE + 1];
    __shared__ double sR[SNAP_TILE][SNAP_TILE + 1];
    const int panel = blockIdx.z, tx = threadIdx.x, ty = threadIdx.y;
    const int x = blockIdx.x * SNAP_TILE + tx, y = blockIdx.y * SNAP_TILE + ty;
    const long tile = ((long)panel * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (panel % (T + 1) > snap_count(counts, panel / (T + 1), T)) {     // no map in this slot: neutral statistics
        if (tx == 0 && ty == 0) {
            part[2 * tile] = INFINITY;
            part[2 * tile + 1] = -INFINITY;
        }
        return;
    }
    const double* Rp = R + (long)panel * a * vis;
    double acc = 0.0;
    for (int p0 = 0; p0 < a; p0 += SNAP_TILE) {
        sM[ty][tx] = (y < vis && p0 + tx < a) ? M[(long)y * a + p0 + tx] : 0.0;
        sR[ty][tx] = (p0 + ty < a && x < vis) ? Rp[(long)(p0 + ty) * vis + x] : 0.0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SNAP_TILE; ++k) acc = fma(sM[ty][k], sR[k][tx], acc);
        __syncthreads();
    }
    const bool in = y < vis && x < vis;
    if (in) E[((long)panel * vis + y) * vis + x] = acc;
    snap_block_minmax(in ? acc : INFINITY, in ? acc : -INFINITY, part + 2 * tile);
}

// maps drawn at their own size (vis == a): E = the maps as they are (panel 0: their maximum), same tile statistics
__global__ __launch_bounds__(256) void snap_copy_maps_kernel(const float* __restrict__ attn, double* __restrict__ E,
                                                             double* __restrict__ part, const int* __restrict__ counts,
                                                             int T, int a) {
    const int P = T + 1, panel = blockIdx.z, n = panel / P, j = panel % P;
    const int x = blockIdx.x * SNAP_TILE + threadIdx.x, y = blockIdx.y * SNAP_TILE + threadIdx.y;
    const int Tn = snap_count(counts, n, T);
    const bool in = y < a && x < a && j <= Tn;
    double v = 0.0;
    if (in) {
        v = snap_map_value(attn + (long)n * T * a * a, Tn, a * a, j, y * a + x);
        E[((long)panel * a + y) * a + x] = v;
    }
    const long tile = ((long)panel * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    snap_block_minmax(in ? v : INFINITY, in ? v : -INFINITY, part + 2 * tile);
}

// mm[n][j] = (min, max) of panel j, tiles in tile order; mm[n][P] = (min(1, ...), max(0, ...)) over the panels in panel order
__global__ void snap_minmax_kernel(const double* __restrict__ part, double* __restrict__ mm, int P, int ntiles) {
    const int n = blockIdx.x;
    for (int j = threadIdx.x; j < P; j += blockDim.x) {
        const double* pp = part + 2 * ((long)(n * P + j) * ntiles);
        double mn = pp[0], mx = pp[1];
        for (int t = 1; t < ntiles; ++t) {
            mn = fmin(mn, pp[2 * t]);
            mx = fmax(mx, pp[2 * t + 1]);
        }
        mm[2 * ((long)n * (P + 1) + j)] = mn;
        mm[2 * ((long)n * (P + 1) + j) + 1] = mx;
    }
    __syncthreads();                                     // (the panel entries above are this workgroup's own writes)
    if (threadIdx.x == 0) {
        const double* s = mm + 2 * (long)n * (P + 1);
        double mn = 1.0, mx = 0.0;
        for (int j = 0; j < P; ++j) {
            if (mn > s[2 * j]) mn = s[2 * j];
            if (mx < s[2 * j + 1]) mx = s[2 * j + 1];
        }
        mm[2 * ((long)n * (P + 1) + P)] = mn;
        mm[2 * ((long)n * (P + 1) + P) + 1] = mx;
    }
}

__device__ __forceinline__ unsigned char snap_trunc_u8(double v) {       // np.uint8 of a value in [0, 255]: truncation
    return v >= 0.0 ? (unsigned char)(int)fmin(v, 255.0) : (unsigned char)0;
}

// one colour byte of the image panel: half-pixel bilinear sample, then (x + 1) / 2 * 255 in three fp32 roundings
__device__ __forceinline__ unsigned char snap_image_byte(const float* __restrict__ xp, int H, int W, int h0, int h1, int w0,
                                                         int w1, float lh0, float lh1, float lw0, float lw1) {
    float v = lh0 * (lw0 * xp[h0 * W + w0] + lw1 * xp[h0 * W + w1]) + lh1 * (lw0 * xp[h1 * W + w0] + lw1 * xp[h1 * W + w1]);
    v = v + 1.f;
    v = v / 2.f;
    v = v * 255.f;
    return snap_trunc_u8((double)v);
}

struct SnapGeom {
    int nvis, P, draw, max_word_num, font_max, vis, H, W, LH, LW, norm, fp32_norm;
};

// normalisation modes of objgan_snapshot_grid: the panel statistics used and what a panel with max == min becomes
#define SNAP_NORM_GLOBAL 0            // image-wide min(1, .) / max(0, .); max == min: 0
#define SNAP_NORM_PANEL 1             // per panel; max == min: the panel as it is
#define SNAP_NORM_RAW 2               // none: v * 255
#define SNAP_NORM_PANEL_UNGUARDED 3   // per panel; max == min: 0

__global__ __launch_bounds__(256) void snap_compose_kernel(const float* __restrict__ imgs, const float* __restrict__ lr,
                                                           const double* __restrict__ E, const double* __restrict__ mm,
                                                           const unsigned char* __restrict__ strip,
                                                           const int* __restrict__ counts,
                                                           unsigned char* __restrict__ out, SnapGeom g) {
    const int cell = g.vis + 2, Wg = (g.max_word_num + 2) * cell, rowH = g.font_max + 2 * g.vis;
    const long total = (long)g.nvis * rowH * Wg;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int x = (int)(e % Wg);
        const long yy = e / Wg;
        const int n = (int)(yy / rowH), ry = (int)(yy % rowH);
        unsigned char* o = out + 3 * e;
        if (ry < g.font_max) {
            const unsigned char* s = strip + 3 * (((long)n * g.font_max + ry) * Wg + x);
            o[0] = s[0];
            o[1] = s[1];
            o[2] = s[2];
            continue;
        }
        const int r = ry - g.font_max, line = r / g.vis, py = r % g.vis;
        const int col = x / cell, px = x % cell;
        unsigned char b0 = 0, b1 = 0, b2 = 0;
        if (px < g.vis && col <= min(snap_count(counts, n, g.P - 1) + 1, g.draw)) {
            // image bytes: the first line's own panel shows the low-resolution image, everything else the image
            const bool need_img = (col == 0 || line == 1);
            unsigned char i0 = 0, i1 = 0, i2 = 0;
            if (need_img) {
                const bool use_lr = (col == 0 && line == 0 && lr != nullptr);
                const float* src = use_lr ? lr : imgs;
                const int H = use_lr ? g.LH : g.H, W = use_lr ? g.LW : g.W;
                const float rh = (float)H / (float)g.vis, rw = (float)W / (float)g.vis;
                const float sh = fmaxf(rh * ((float)py + 0.5f) - 0.5f, 0.f);
                const float sw = fmaxf(rw * ((float)px + 0.5f) - 0.5f, 0.f);
                const int h0 = min((int)sh, H - 1), w0 = min((int)sw, W - 1);
                const int h1 = h0 + (h0 < H - 1 ? 1 : 0), w1 = w0 + (w0 < W - 1 ? 1 : 0);
                const float lh1 = sh - (float)h0, lw1 = sw - (float)w0;
                const float lh0 = 1.f - lh1, lw0 = 1.f - lw1;
                const float* xp = src + (long)n * 3 * H * W;
                i0 = snap_image_byte(xp, H, W, h0, h1, w0, w1, lh0, lh1, lw0, lw1);
                i1 = snap_image_byte(xp + (long)H * W, H, W, h0, h1, w0, w1, lh0, lh1, lw0, lw1);
                i2 = snap_image_byte(xp + 2L * H * W, H, W, h0, h1, w0, w1, lh0, lh1, lw0, lw1);
            }
            if (col == 0) {
                b0 = i0;
                b1 = i1;
                b2 = i2;
            } else {
                const int j = col - 1;
                const double v = E[(((long)n * g.P + j) * g.vis + py) * g.vis + px];
                const bool per_panel = g.norm == SNAP_NORM_PANEL || g.norm == SNAP_NORM_PANEL_UNGUARDED;
                const double* m2 = mm + 2 * ((long)n * (g.P + 1) + (per_panel ? j : g.P));
                const double mn = m2[0], mx = m2[1];
                unsigned char att;
                if (g.norm == SNAP_NORM_RAW) {
                    att = snap_trunc_u8((double)((float)v * 255.f));         // (fp32 path only: the entry refuses M)
                } else if (mx == mn) {
                    // guarded shape form: the map is drawn unnormalised; the other forms: 0 (the reference's 0 / 0)
                    att = g.norm == SNAP_NORM_PANEL
                              ? (g.fp32_norm ? snap_trunc_u8((double)((float)v * 255.f)) : snap_trunc_u8(v * 255.0))
                              : (unsigned char)0;
                } else if (g.fp32_norm) {
                    float t = (float)v - (float)mn;
                    t = t / ((float)mx - (float)mn);
                    t = t * 255.f;
                    att = snap_trunc_u8((double)t);
                } else {
                    double t = v - mn;
                    t = t / (mx - mn);
                    t = t * 255.0;
                    att = snap_trunc_u8(t);
                }
                if (line == 0) {
                    b0 = b1 = b2 = att;
                } else {
                    b0 = og_paste_blend_210(i0, att);
                    b1 = og_paste_blend_210(i1, att);
                    b2 = og_paste_blend_210(i2, att);
                }
            }
        }
        o[0] = b0;
        o[1] = b1;
        o[2] = b2;
    }
}

// ---- mask dump (reference shape_generation/trainer.py:389-397): plane -> (v - min) / (max - min) * 255, three channels ----
#define MASK_THREADS 256

__device__ __forceinline__ unsigned mask_byte(float v, float mn, float den) {
    float t = v - mn;
    t = t / den;
    t = t * 255.f;
    return (unsigned)snap_trunc_u8((double)t);
}

// One workgroup per selected plane: pass 1 reduces min / max (per thread, then a fixed-order tree in LDS), pass 2 reads the
// plane again (L2) and writes the bytes.  VEC: 16-byte loads and 4-byte stores of the 12 bytes of four pixels.
template <bool VEC>
__global__ __launch_bounds__(MASK_THREADS) void mask_to_rgb8_kernel(const float* __restrict__ masks,
                                                                    const int* __restrict__ sel,
                                                                    unsigned char* __restrict__ out, int HW) {
    __shared__ float smn[MASK_THREADS], smx[MASK_THREADS];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* src = masks + (long)(sel ? sel[n] : n) * HW;
    unsigned char* dst = out + (long)n * HW * 3;
    float mn = INFINITY, mx = -INFINITY;
    if (VEC) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        for (int i = tid; i < HW / 4; i += MASK_THREADS) {
            const float4 v = s4[i];
            mn = fminf(fminf(mn, v.x), fminf(v.y, fminf(v.z, v.w)));
            mx = fmaxf(fmaxf(mx, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
        }
    } else {
        for (int i = tid; i < HW; i += MASK_THREADS) {
            mn = fminf(mn, src[i]);
            mx = fmaxf(mx, src[i]);
        }
    }
    smn[tid] = mn;
    smx[tid] = mx;
    __syncthreads();
    for (int s = MASK_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            smn[tid] = fminf(smn[tid], smn[tid + s]);
            smx[tid] = fmaxf(smx[tid], smx[tid + s]);
        }
        __syncthreads();
    }
    mn = smn[0];
    mx = smx[0];
    const bool flat = !(mx > mn);                                   // max == min: the reference's 0 / 0 -> zeros
    const float den = mx - mn;
    if (VEC) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        uint3* d3 = reinterpret_cast<uint3*>(dst);                  // (12 bytes per four pixels, 4-byte aligned)
        for (int i = tid; i < HW / 4; i += MASK_THREADS) {
            uint3 w = make_uint3(0u, 0u, 0u);
            if (!flat) {
                const float4 v = s4[i];
                const unsigned a = mask_byte(v.x, mn, den), b = mask_byte(v.y, mn, den);
                const unsigned c = mask_byte(v.z, mn, den), d = mask_byte(v.w, mn, den);
                w.x = a * 0x010101u | b << 24;                      // a a a b
                w.y = b * 0x0101u | c << 16 | c << 24;              // b b c c
                w.z = c | d * 0x01010100u;                          // c d d d
            }
            d3[i] = w;
        }
    } else {
        for (int i = tid; i < HW; i += MASK_THREADS) {
            const unsigned char b = flat ? (unsigned char)0 : (unsigned char)mask_byte(src[i], mn, den);
            dst[3 * i] = b;
            dst[3 * i + 1] = b;
            dst[3 * i + 2] = b;
        }
    }
}

static inline long snap_tiles(int vis) { return (long)og_cdiv(vis, SNAP_TILE) * og_cdiv(vis, SNAP_TILE); }

extern "C" {

// table[im * 256 + att] = the merged-panel byte of image byte `im` under attention byte `att` (host only)
int objgan_snapshot_blend_table(unsigned char* table65536) {
    if (!table65536) return OG_BAD_ARGS;
    for (unsigned im = 0; im < 256; ++im)
        for (unsigned att = 0; att < 256; ++att) table65536[im * 256 + att] = og_paste_blend_210(im, att);
    return OG_OK;
}

// doubles of workspace objgan_snapshot_grid needs: expanded maps, the half product, tile and panel statistics (host only)
long objgan_snapshot_ws_doubles(int nvis, int T, int a, int vis) {
    if (nvis < 1 || T < 1 || T > 1023 || a < 1 || vis < a) return 0;
    const long panels = (long)nvis * (T + 1);
    return panels * vis * vis + panels * a * vis + 2 * panels * snap_tiles(vis) + 2L * nvis * (T + 2);
}

int objgan_snapshot_grid(const float* imgs, const float* lr_imgs, const float* attn, const int* counts, const double* M,
                         const unsigned char* strip, unsigned char* out, double* ws, long ws_doubles,
                         int nvis, int T, int a, int vis, int H, int W, int LH, int LW,
                         int max_word_num, int font_max, int per_panel_norm, void* stream) {
    OG_ENTRY();
    if (nvis < 1 || T < 1 || T > 1023 || a < 1 || vis < 1 || H < 1 || W < 1 || max_word_num < 0 || font_max < 0) return OG_BAD_ARGS;
    if (!imgs || !attn || !out || !ws || (font_max > 0 && !strip)) return OG_BAD_ARGS;
    if (lr_imgs && (LH < 1 || LW < 1)) return OG_BAD_ARGS;
    // an expansion needs its matrix and a whole ratio of at least 2; maps drawn as they are have the panel's size
    if (M ? (vis / a < 2) : (vis != a)) return OG_BAD_ARGS;
    // the shape stage's forms are fp32 arithmetic on maps of the panel's size: no expansion
    if (per_panel_norm < SNAP_NORM_GLOBAL || per_panel_norm > SNAP_NORM_PANEL_UNGUARDED) return OG_BAD_ARGS;
    if (M && per_panel_norm >= SNAP_NORM_RAW) return OG_BAD_ARGS;
    const long need = objgan_snapshot_ws_doubles(nvis, T, a, vis);
    if (need <= 0 || ws_doubles < need) return OG_BAD_ARGS;
    const int P = T + 1;
    const long panels = (long)nvis * P;
    const int tv = og_cdiv(vis, SNAP_TILE), ta = og_cdiv(a, SNAP_TILE);
    if (panels > 65535 || (long)a * a * T > 0x7fffffffL) return OG_BAD_ARGS;
    double* E = ws;
    double* R = E + panels * vis * vis;
    double* part = R + panels * a * vis;
    double* mm = part + 2 * panels * snap_tiles(vis);
    hipStream_t st = (hipStream_t)stream;
    const dim3 blk(SNAP_TILE, SNAP_TILE);
    if (M) {
        hipLaunchKernelGGL(snap_expand_cols_kernel, dim3(tv, ta, (unsigned)panels), blk, 0, st, attn, M, R, counts, T, a, vis);
        hipLaunchKernelGGL(snap_expand_rows_kernel, dim3(tv, tv, (unsigned)panels), blk, 0, st, M, R, E, part, counts, T, a, vis);
    } else {
        hipLaunchKernelGGL(snap_copy_maps_kernel, dim3(tv, tv, (unsigned)panels), blk, 0, st, attn, E, part, counts, T, a);
    }
    hipLaunchKernelGGL(snap_minmax_kernel, dim3(nvis), dim3(64), 0, st, part, mm, P, (int)snap_tiles(vis));
    SnapGeom g;
    g.nvis = nvis; g.P = P; g.draw = P < max_word_num + 1 ? P : max_word_num + 1; g.max_word_num = max_word_num;
    g.font_max = font_max; g.vis = vis; g.H = H; g.W = W; g.LH = LH; g.LW = LW;
    g.norm = per_panel_norm; g.fp32_norm = M ? 0 : 1;
    const long total = (long)nvis * (font_max + 2 * vis) * (max_word_num + 2) * (vis + 2);
    hipLaunchKernelGGL(snap_compose_kernel, dim3(og_stream_grid(total, 256)), dim3(256), 0, st, imgs, lr_imgs, E, mm, strip,
                       counts, out, g);
    return og_launch_status();
}

int objgan_mask_to_rgb8(const float* masks, const int* sel, unsigned char* out, int N, int HW, void* stream) {
    OG_ENTRY();
    if (!masks || !out || N < 1 || HW < 1 || (long)N * HW * 3 > 0x7fffffffL) return OG_BAD_ARGS;
    hipStream_t st = (hipStream_t)stream;
    // every selected plane starts a multiple of HW floats behind `masks`, every output plane 3 HW bytes behind `out`
    const bool vec = HW % 4 == 0 && ((uintptr_t)masks & 15) == 0 && ((uintptr_t)out & 3) == 0;
    if (vec)
        hipLaunchKernelGGL(mask_to_rgb8_kernel<true>, dim3(N), dim3(MASK_THREADS), 0, st, masks, sel, out, HW);
    else
        hipLaunchKernelGGL(mask_to_rgb8_kernel<false>, dim3(N), dim3(MASK_THREADS), 0, st, masks, sel, out, HW);
    return og_launch_status();
}

}  // extern "C"

// Layout stage: the decoder's samples -> the image generator's box tables and the shape generator's box maps, on the
// device.  It restates, without the files in between, what the file route does per caption on the host:
//   stage A  seq2seq/evaluator/evaluator.py Evaluator.postprocess (reference box_generation evaluator.py:74-139)
//   stage B  write_layouts ('%.2f' rows of boxes.txt) -> miscc/load.py _read_boxes -> load_gen_insanns -> get_gen_rois
//            (reference image_generation miscc/load.py:653-776, 194-214)
//
// Kernel 1 (tables): one wave per caption, lane t owns decode step t (T <= 17).  The positivity filter, the dropped
// last entry, the per-category cap and the area ranking are ballots, popcounts and shuffles over the wave; a slot -> lane table in
// LDS turns them into ordered rows.  Kernel 2 (maps): a grid-stride fill of the per-box rectangles from the integer
// bounds kernel 1 left in the scratch table.  No atomics, no host read, ordinary vector stores.
//
// This file is compiled with -ffp-contract=off: the fp64 chain of stage A rounds operation by operation, as numpy
// does.  The one fused operation is the explicit fma of lt_int2 (see there).
#include "common.h"

namespace {

constexpr int LT_MAX_T = 17;        // up to 16 boxes reach np.argsort: the two orders of equal keys known for that many
constexpr int LT_MAX_R = 64, LT_MAX_NB = 4;

struct LayoutArgs {
    const int* labels; const int* lengths; const double* samples; const double* mean_std;
    const int* label_to_cat; const int* cat_to_rel; const int* thresholds;
    double* boxes; int* nbox; double* rois; double* fm_rois; int* num_rois; int* cats; int* bounds;
    double scale[LT_MAX_NB];
    int B, T, L, ncat, R, NB, S, F, min_size, tie_rule;
};

// int(float('%.2f' % v)) for v >= 0: floor(v), plus 1 when the exact fractional part is >= 0.995.  v - floor(v) is
// exact in fp64, and fma(frac, 200, -199) is the exact value of 200 frac - 199 rounded once, so its sign is exact
// (0.995 is no binary fraction: there is no tie).
__device__ __forceinline__ int lt_int2(double v) {
    const double f = floor(v);
    const double frac = v - f;
    return (int)f + (fma(frac, 200.0, -199.0) >= 0.0 ? 1 : 0);
}

// One compare-exchange stage of numpy's argsort network for 64-bit keys (see lt_argsort16): the lane keeps the smaller
// or the larger key of itself and its partner, and the partner's index only when the kept key is not its own.
__device__ __forceinline__ void lt_cmp(int& key, int& idx, int partner, bool take_max) {
    const int k2 = __shfl(key, partner, 64), i2 = __shfl(idx, partner, 64);
    const int r = take_max ? (key > k2 ? key : k2) : (key < k2 ? key : k2);
    idx = r == key ? idx : i2;
    key = r;
}

// np.argsort of n <= 16 keys as numpy computes it where it dispatches its AVX-512 sorting network (64-bit keys, eight per
// register): lanes 16 g .. 16 g + 15 hold positions 0 .. 15 (key, index; positions >= n padded with the largest key),
// afterwards position p holds the index that np.argsort returns at p.  Bitonic sort of each register (six stages), then,
// for n > 8, the merge of the two: register 0 against register 1 reversed, the larger halves reversed, three
// half-cleaner stages each.  Equal keys never exchange, so the order of equal keys is the network's (not stable).
// Checked against numpy 2.2 on 30000 random arrays with ties (n = 2 .. 16): identical.
__device__ __forceinline__ void lt_argsort16(int& key, int& idx, int n) {
    const int t = threadIdx.x, p = t & 15, l = t & 7, v = t & ~7;
    const bool aa = l & 1, cc = (l >> 1) & 1, f0 = (l >> 2) & 1;
    lt_cmp(key, idx, v + (l ^ 1), aa);
    lt_cmp(key, idx, v + (l ^ 3), cc);
    lt_cmp(key, idx, v + (l ^ 1), aa);
    lt_cmp(key, idx, v + (l ^ 7), f0);
    lt_cmp(key, idx, v + (l ^ 2), cc);
    lt_cmp(key, idx, v + (l ^ 1), aa);
    if (n <= 8) return;                                        // (uniform)
    {
        const int partner = (t & ~15) + 15 - p;
        const int k2 = __shfl(key, partner, 64), i2 = __shfl(idx, partner, 64);
        if (p < 8) {                                           // the smaller of (register 0, register 1 reversed)
            const int r = key < k2 ? key : k2;
            idx = r == key ? idx : i2;
            key = r;
        } else {                                               // the larger, already in reversed order
            const bool first_is_min = k2 <= key;               // the partner sits in register 0
            idx = first_is_min ? idx : i2;
            key = key > k2 ? key : k2;
        }
    }
    lt_cmp(key, idx, v + (l ^ 4), f0);
    lt_cmp(key, idx, v + (l ^ 2), cc);
    lt_cmp(key, idx, v + (l ^ 1), aa);
}

// min(int(round(v)), side - 1) with Python's round (half to even)
__device__ __forceinline__ int lt_bound(double v, int side) {
    const int i = (int)rint(v);
    return i < side - 1 ? i : side - 1;
}

// grid = B, block = 64
__global__ void __launch_bounds__(64) layout_tables_kernel(LayoutArgs a) {
    __shared__ int owner[LT_MAX_R];            // roi slot -> lane, -1: empty
    __shared__ int bown[LT_MAX_T];             // box row -> lane
    __shared__ double vals[64][5];             // per lane: x, y, w, h, category
    __shared__ int ivals[64][5];               // per lane: the integers of boxes.txt and the relative category
    __shared__ int skey[16], sown[16];         // the usable boxes in file order: area, lane
    const int b = blockIdx.x, t = threadIdx.x;
    const int T = a.T, R = a.R;
    const unsigned long long below = t == 0 ? 0ull : (~0ull >> (64 - t));

    if (t < LT_MAX_R) owner[t] = -1;
    if (t < LT_MAX_T) bown[t] = -1;

    // ---- stage A ----
    int len = a.lengths[b];
    len = len < 0 ? 0 : (len > T ? T : len);
    double x = 0.0, y = 0.0, w = 0.0, h = 0.0;
    int label = -1;
    bool valid = false;
    if (t < len) {
        const double* s = a.samples + ((size_t)b * T + t) * 4;
        x = s[0] * a.mean_std[1] + a.mean_std[0];
        y = s[1] * a.mean_std[3] + a.mean_std[2];
        w = s[2] * a.mean_std[5] + a.mean_std[4];
        const double r = s[3] * a.mean_std[7] + a.mean_std[6];
        h = w * r;
        label = a.labels[(size_t)b * T + t];
        valid = x > 0.0 && y > 0.0 && w > 0.0 && h > 0.0;
    }
    unsigned long long m = __ballot(valid);
    if (__popcll(m) <= 1) m = 0ull;
    else m &= ~(1ull << (63 - __clzll(m)));                  // the last surviving entry goes
    int cat = -1;
    if ((m >> t) & 1ull) cat = (label >= 0 && label < a.L) ? a.label_to_cat[label] : -1;
    bool kept = cat >= 0;                                      // (a label that names no category: postprocess raises)
    int occ = 0;                                               // earlier entries of the same category
    for (int j = 0; j < T; ++j) {
        const int cj = __shfl(cat, j, 64);
        occ += (j < t && cj == cat) ? 1 : 0;
    }
    if (kept) kept = occ < a.thresholds[(size_t)b * a.L + label];
    if (kept) {
        const double x0 = fmin(fmax(x - w / 2.0, 1.0), 255.0);
        const double y0 = fmin(fmax(y - h / 2.0, 1.0), 255.0);
        w = fmin(w, 256.0 - x0);
        h = fmin(h, 256.0 - y0);
        x = x0;
        y = y0;
    }
    const unsigned long long km = __ballot(kept);
    const int nb = __popcll(km);
    if (kept) bown[__popcll(km & below)] = t;
    vals[t][0] = x; vals[t][1] = y; vals[t][2] = w; vals[t][3] = h; vals[t][4] = (double)cat;

    // ---- stage B ----
    int ix = 0, iy = 0, iw = 0, ih = 0, rel = -1;
    bool roi = false;
    if (kept) {
        ix = lt_int2(x); iy = lt_int2(y); iw = lt_int2(w); ih = lt_int2(h);
        rel = cat < a.ncat ? a.cat_to_rel[cat] : -1;           // (an unknown category id: load_gen_insanns raises)
        roi = rel >= 0 && !(iw < a.min_size && ih < a.min_size);
    }
    const unsigned long long rm = __ballot(roi);
    const int n2 = __popcll(rm);
    int slot = __popcll(rm & below);
    if (n2 > R && a.tie_rule == 1) {
        // np.argsort(area)[::-1] where numpy sorts with its AVX-512 network: the largest first, equal areas as it leaves them
        if (roi) { skey[slot] = iw * ih; sown[slot] = t; }
        __syncthreads();
        const int p = t & 15;
        int key = p < n2 ? skey[p] : 0x7fffffff;
        int idx = p < n2 ? p : 0;
        lt_argsort16(key, idx, n2);
        if (t < n2 && n2 - 1 - t < R) owner[n2 - 1 - t] = sown[idx];
        slot = R;                                              // (placed above)
    } else if (n2 > R) {
        // np.argsort(area)[::-1] where numpy sorts <= 16 values by insertion (stable), reversed -- the largest first,
        // equal areas with the LATER box first
        const int area = iw * ih;
        int rank = 0;
        for (int j = 0; j < T; ++j) {
            const int aj = __shfl(area, j, 64);
            const bool rj = (rm >> j) & 1ull;
            rank += (rj && (aj > area || (aj == area && j > t))) ? 1 : 0;
        }
        slot = rank;
    }
    if (roi && slot < R) owner[slot] = t;
    ivals[t][0] = ix; ivals[t][1] = iy; ivals[t][2] = iw; ivals[t][3] = ih; ivals[t][4] = rel;
    __syncthreads();

    if (t == 0) {
        a.nbox[b] = nb;
        a.num_rois[b] = n2 < R ? n2 : R;
    }
    if (t < T) {                                               // box rows in order, the rest zero
        const int o = bown[t];
        double* row = a.boxes + ((size_t)b * T + t) * 5;
        for (int k = 0; k < 5; ++k) row[k] = o >= 0 ? vals[o][k] : 0.0;
    }
    for (int r = t; r < R; r += 64) {                          // roi rows in order, the rest zero
        const int o = owner[r];
        const size_t br = (size_t)b * R + r;
        double q[4] = {0.0, 0.0, 0.0, 0.0};
        double relv = 0.0;
        if (o >= 0) {
            for (int k = 0; k < 4; ++k) q[k] = (double)ivals[o][k];
            relv = (double)ivals[o][4];
        }
        double r0[4];
        for (int br_i = 0; br_i < a.NB; ++br_i) {
            double* row = a.rois + ((size_t)br_i * a.B * R + br) * 6;
            for (int k = 0; k < 4; ++k) {
                const double v = q[k] * a.scale[br_i];
                row[k] = v;
                if (br_i == 0) r0[k] = v;
            }
            row[4] = relv;
            row[5] = 0.0;
        }
        double* frow = a.fm_rois + br * 6;
        double f[4];
        for (int k = 0; k < 4; ++k) { f[k] = r0[k] / 2.0; frow[k] = f[k]; }
        frow[4] = relv;
        frow[5] = 0.0;
        a.cats[br] = o >= 0 ? ivals[o][4] : 0;
        int* bd = a.bounds + br * 8;                            // x0, x1, y0, y1 of the map, then of the feature map
        if (o >= 0) {
            bd[0] = lt_bound(r0[0], a.S);
            bd[1] = lt_bound(r0[0] + r0[2], a.S);
            bd[2] = lt_bound(r0[1], a.S);
            bd[3] = lt_bound(r0[1] + r0[3], a.S);
            bd[4] = lt_bound(f[0] / 2.0, a.F);
            bd[5] = lt_bound(f[0] / 2.0 + f[2] / 2.0, a.F);
            bd[6] = lt_bound(f[1] / 2.0, a.F);
            bd[7] = lt_bound(f[1] / 2.0 + f[3] / 2.0, a.F);
        } else {
            for (int k = 0; k < 8; ++k) bd[k] = 0;
        }
    }
}

// maps [B R][S][S] and fmaps [B R][F][F]: 1 on [y0:y1, x0:x1], 0 elsewhere; V floats per store
template <int V>
__global__ void __launch_bounds__(256) layout_maps_kernel(const int* __restrict__ bounds, float* __restrict__ maps,
                                                          float* __restrict__ fmaps, long BR, int S, int F) {
    typedef float vt __attribute__((ext_vector_type(V)));
    const long per_m = (long)S * S / V, per_f = (long)F * F / V;
    const long per = per_m + per_f;
    const long items = BR * per;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < items; idx += (long)gridDim.x * blockDim.x) {
        const long br = idx / per;
        long e = idx % per;
        const bool fm = e >= per_m;
        if (fm) e -= per_m;
        const int side = fm ? F : S;
        const int* bd = bounds + br * 8 + (fm ? 4 : 0);
        const int p = (int)e * V;
        const int yy = p / side, xx = p % side;
        const bool row_in = yy >= bd[2] && yy < bd[3];
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = (row_in && xx + j >= bd[0] && xx + j < bd[1]) ? 1.f : 0.f;
        float* dst = (fm ? fmaps + br * (long)F * F : maps + br * (long)S * S) + p;
        if (V == 1) dst[0] = o[0];
        else {
            vt v;
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = o[j];
            *reinterpret_cast<vt*>(dst) = v;
        }
    }
}

}  // namespace

extern "C" {

// labels [B][T] int32, lengths [B] int32, samples [B][T][4] doubles: what objgan_box_decode wrote.
// mean_std [8] doubles: (mean, std) of x, y, w, r.  label_to_cat [L]: decoder label -> category id, -1 where the label
// names none.  cat_to_rel [ncat]: category id -> row of categories.txt, -1 for an unknown id.  thresholds [B][L]: the
// per-caption, per-label count caps.
// boxes [B][T][5] doubles (x, y, w, h, category id; rows past nbox[b] zero), nbox [B]: Evaluator.postprocess.
// rois [NB][B][R][6], fm_rois [B][R][6] doubles, num_rois [B], cats [B][R] (relative category, 0 in unused slots),
// maps [B][R][S][S], fmaps [B][R][F][F] floats: load_gen_insanns / get_gen_rois on the '%.2f' rows of those boxes.
// sizes [NB]: the branch sides, S = sizes[0]; min_size: cfg.ROI.ROI_MIN_SIZE.  bounds: scratch of 8 B R ints.
// tie_rule: how np.argsort orders EQUAL areas when more than R boxes are left, which decides the boxes kept and their
// order -- 0: insertion sort (numpy's generic code for <= 16 values; stable, so the later box comes first after the
// reversal), 1: numpy's AVX-512 network for 64-bit keys (lt_argsort16).  The file route runs on the host's numpy: the
// caller passes the rule that numpy follows there.
// T > 17 is refused: beyond 16 boxes neither rule describes numpy's argsort.
int objgan_layout_from_decode(const int* labels, const int* lengths, const double* samples, const double* mean_std,
                              const int* label_to_cat, const int* cat_to_rel, const int* thresholds,
                              double* boxes, int* nbox, double* rois, double* fm_rois, int* num_rois, int* cats,
                              float* maps, float* fmaps, int* bounds, const int* sizes, int NB, int F, int R,
                              int min_size, int tie_rule, int B, int T, int L, int ncat, void* stream) {
    OG_ENTRY();
    if (!labels || !lengths || !samples || !mean_std || !label_to_cat || !cat_to_rel || !thresholds || !boxes || !nbox ||
        !rois || !fm_rois || !num_rois || !cats || !maps || !fmaps || !bounds || !sizes)
        return OG_BAD_ARGS;
    if (tie_rule != 0 && tie_rule != 1) return OG_BAD_ARGS;
    if (T < 1 || T > LT_MAX_T || R < 1 || R > LT_MAX_R || NB < 1 || NB > LT_MAX_NB || F < 1 || L < 1 || ncat < 1)
        return OG_BAD_ARGS;
    for (int i = 0; i < NB; ++i)
        if (sizes[i] < 1) return OG_BAD_ARGS;
    if (B <= 0) return OG_OK;
    LayoutArgs a = {labels, lengths, samples, mean_std, label_to_cat, cat_to_rel, thresholds,
                    boxes, nbox, rois, fm_rois, num_rois, cats, bounds, {0.0, 0.0, 0.0, 0.0},
                    B, T, L, ncat, R, NB, sizes[0], F, min_size, tie_rule};
    for (int i = 0; i < NB; ++i) a.scale[i] = sizes[i] / (double)sizes[NB - 1];
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(layout_tables_kernel, dim3(B), dim3(64), 0, s, a);
    int rc = og_launch_status();
    if (rc != OG_OK) return rc;
    const int S = sizes[0];
    const long BR = (long)B * R;
    const bool v4 = S % 4 == 0 && F % 4 == 0 && (((uintptr_t)maps | (uintptr_t)fmaps) & 15) == 0;
    const long items = BR * ((long)S * S + (long)F * F) / (v4 ? 4 : 1);
    const int grid = og_stream_grid(items, 256);
    if (v4) hipLaunchKernelGGL(layout_maps_kernel<4>, dim3(grid), dim3(256), 0, s, bounds, maps, fmaps, BR, S, F);
    else hipLaunchKernelGGL(layout_maps_kernel<1>, dim3(grid), dim3(256), 0, s, bounds, maps, fmaps, BR, S, F);
    return og_launch_status();
}

}  // extern "C"

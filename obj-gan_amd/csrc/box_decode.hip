// Box generator, sampling path (reference box_generation/seq2seq/models/DecoderRNN.py:81-183 forward_step with
// is_training=0, and the loop of DecoderRNN.forward:261-292): caption state -> label and box sequence.
//
// The reference decodes one caption per host iteration and crosses to the host several times per step.  Here ONE launch
// decodes a batch: a workgroup owns a tile of CPW captions and walks the <= T steps inside the kernel with all per-caption
// state in LDS.  Thread j owns gate row j of the 4H gates (as lstm.hip) and streams column j of the transposed
// weight_ih / weight_hh ONCE per step for the whole tile, accumulating CPW sums with the operands broadcast from LDS
// (stored [element][caption], so one LDS read serves the tile).  The sum of one caption is a fixed chain of fmaf over
// the elements in order: it depends neither on the caption's position in the tile, nor on CPW, nor on the batch.
// Captions that ended are masked (their state is frozen, nothing of theirs is written), not compacted.
//
// No random numbers are drawn here: the caller passes noise[B][T][6] doubles (uniform, normal, normal for the (x, y)
// draw, then the same for (w, h)), so a layout is a pure function of (weights, caption state, noise row).
//   component  p = exp(log(pi) / 0.4 - max) normalised in fp32 (sample_next_state.adjust_temp on an fp32 array);
//              np.random.choice: fp64 running sum divided by its last element, index = #entries <= u, clamped to K-1
//   point      sigma *= sqrt(0.4) in fp32, the 2x2 covariance from fp32 products (as the reference hands them to
//              multivariate_normal), then its Cholesky factor in fp64:
//              x = u_x + sqrt(c00) z1,  y = u_y + c01 / sqrt(c00) z1 + sqrt(c11 - c01^2 / c00) z2
// This file is compiled with -ffp-contract=off: the dot products use fmaf explicitly, the draw rounds per operation.
#include "common.h"

namespace {

constexpr int BD_MAX_L = 256, BD_MAX_K = 8, BD_MAX_T = 32, BD_MAX_A = 64;

struct BoxDecodeArgs {
    const float* h0; const float* c0; const double* noise;
    const float* l_emb;                                   // [L][H]
    const float* xy_w; const float* xy_b;                 // [A][2], [A]
    const float* wh_w; const float* wh_b;
    const float* nxy_w; const float* nxy_b;
    const float* wt_ih; const float* wt_hh;               // [2A + H][4H], [H][4H]
    const float* b_ih; const float* b_hh;                 // [4H]
    const float* lo_wt; const float* lo_b;                // [H][L], [L]
    const float* xyo_wt; const float* xyo_b;              // [H + L][6K], [6K]
    const float* who_wt; const float* who_b;              // [H + L + A][6K], [6K]
    int* labels; int* lengths; double* samples; float* trace;
    float x0, y0, w0, r0;
    int B, T, H, L, K, A, sos, eos;
};

__device__ __forceinline__ float bd_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// One mixture draw by one lane.  raw: the 6K outputs of xy_out / wh_out; par: where the activated parameters go
// (pi, u_a, u_b, sigma_a, sigma_b, rho; K each) or null.  Not inlined: one lane per caption runs it twice a step, and
// its fp64 temporaries would otherwise cost the streaming loops registers (the block has 128 per lane).
__device__ __noinline__ void bd_draw(const float* raw, int K, double u, double z1, double z2, float* par, double* oa, double* ob) {
    float pi[BD_MAX_K], p[BD_MAX_K];
    float mx = raw[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, raw[k]);
    float s = 0.f;
    for (int k = 0; k < K; ++k) { pi[k] = expf(raw[k] - mx); s += pi[k]; }
    for (int k = 0; k < K; ++k) pi[k] = pi[k] / s;
    if (par) {
        for (int k = 0; k < K; ++k) {
            par[k] = pi[k];
            par[K + k] = raw[K + k];
            par[2 * K + k] = raw[2 * K + k];
            par[3 * K + k] = expf(raw[3 * K + k]);
            par[4 * K + k] = expf(raw[4 * K + k]);
            par[5 * K + k] = tanhf(raw[5 * K + k]);
        }
    }
    float pm = 0.f;
    for (int k = 0; k < K; ++k) { p[k] = logf(pi[k]) / 0.4f; pm = k == 0 ? p[0] : fmaxf(pm, p[k]); }
    float ps = 0.f;
    for (int k = 0; k < K; ++k) { p[k] = expf(p[k] - pm); ps += p[k]; }
    double cdf[BD_MAX_K], run = 0.0;
    for (int k = 0; k < K; ++k) { run += (double)(p[k] / ps); cdf[k] = run; }
    int idx = 0;
    for (int k = 0; k < K; ++k) idx += (cdf[k] / run <= u) ? 1 : 0;
    idx = idx > K - 1 ? K - 1 : idx;
    const float ua = raw[K + idx], ub = raw[2 * K + idx];
    const float t = 0.63245553203367588f;                              // (float)sqrt(0.4)
    const float sa = expf(raw[3 * K + idx]) * t, sb = expf(raw[4 * K + idx]) * t;
    const float rho = tanhf(raw[5 * K + idx]);
    const double c00 = (double)(sa * sa), c01 = (double)((rho * sa) * sb), c11 = (double)(sb * sb);
    const double l00 = sqrt(c00), l10 = c01 / l00, l11 = sqrt(c11 - l10 * l10);
    *oa = (double)ua + l00 * z1;
    *ob = (double)ub + (l10 * z1 + l11 * z2);
}

// grid = ceil(B / CPW), block = 4H rounded up to a wave (<= 1024).
// Dynamic LDS, floats: xs [I][CPW] | hs [H][CPW] | ps [L][CPW] | es [A][CPW] | cs [CPW][H] | gs [CPW][4H] |
//                      m1 [CPW][6K] | m2 [CPW][6K] | st [CPW][4] | then ints lab [CPW] | alive [CPW] | len [CPW]
template <int CPW>
__global__ void __launch_bounds__(1024) box_decode_kernel(BoxDecodeArgs a) {
    extern __shared__ float4 sm4[];
    const int H = a.H, L = a.L, K = a.K, A = a.A, T = a.T;
    const int G = 4 * H, I = 2 * A + H, Q = 6 * K;
    float* xs = reinterpret_cast<float*>(sm4);
    float* hs = xs + (size_t)I * CPW;
    float* ps = hs + (size_t)H * CPW;
    float* es = ps + (size_t)L * CPW;
    float* cs = es + (size_t)A * CPW;
    float* gs = cs + (size_t)CPW * H;
    float* m1 = gs + (size_t)CPW * G;
    float* m2 = m1 + CPW * Q;
    float* st = m2 + CPW * Q;
    int* lab = reinterpret_cast<int*>(st + CPW * 4);
    int* alive = lab + CPW;
    int* len = alive + CPW;

    const int j = threadIdx.x, nthr = blockDim.x;
    const int lane = j & 63, wid = j >> 6, nw = nthr >> 6;
    const int b0 = blockIdx.x * CPW;
    const int TR = L + 2 * Q;

    for (int e = j; e < CPW * H; e += nthr) {
        const int c = e / H, k = e % H;
        const bool in = b0 + c < a.B;
        hs[k * CPW + c] = in ? a.h0[(size_t)(b0 + c) * H + k] : 0.f;
        cs[c * H + k] = in ? a.c0[(size_t)(b0 + c) * H + k] : 0.f;
    }
    if (j < CPW) {
        st[j * 4 + 0] = a.x0; st[j * 4 + 1] = a.y0; st[j * 4 + 2] = a.w0; st[j * 4 + 3] = a.r0;
        lab[j] = a.sos;
        alive[j] = b0 + j < a.B ? 1 : 0;
        len[j] = 0;
    }
    const float gbias = j < G ? a.b_ih[j] + a.b_hh[j] : 0.f;
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        int any = 0;
#pragma unroll
        for (int c = 0; c < CPW; ++c) any |= alive[c];
        if (!any) break;                                   // uniform: alive[] is written before the step's last barrier

        // 1. input = cat(xy_embedding(x, y), wh_embedding(w, h), l_embedding[label])
        for (int e = j; e < I * CPW; e += nthr) {
            const int i = e / CPW, c = e % CPW;
            float v;
            if (i < A) v = fmaf(a.xy_w[2 * i + 1], st[c * 4 + 1], fmaf(a.xy_w[2 * i], st[c * 4 + 0], a.xy_b[i]));
            else if (i < 2 * A) {
                const int q = i - A;
                v = fmaf(a.wh_w[2 * q + 1], st[c * 4 + 3], fmaf(a.wh_w[2 * q], st[c * 4 + 2], a.wh_b[q]));
            } else {
                int l = lab[c];
                l = l < 0 ? 0 : (l >= L ? L - 1 : l);
                v = a.l_emb[(size_t)l * H + (i - 2 * A)];
            }
            xs[e] = v;
        }
        __syncthreads();

        // 2. the 4H gate pre-activations: one pass over the weights for the tile
        if (j < G) {
            float acc[CPW];
#pragma unroll
            for (int c = 0; c < CPW; ++c) acc[c] = gbias;
#pragma unroll 4
            for (int i = 0; i < I; ++i) {
                const float w = a.wt_ih[(size_t)i * G + j];
#pragma unroll
                for (int c = 0; c < CPW; ++c) acc[c] = fmaf(w, xs[i * CPW + c], acc[c]);
            }
#pragma unroll 4
            for (int k = 0; k < H; ++k) {
                const float w = a.wt_hh[(size_t)k * G + j];
#pragma unroll
                for (int c = 0; c < CPW; ++c) acc[c] = fmaf(w, hs[k * CPW + c], acc[c]);
            }
#pragma unroll
            for (int c = 0; c < CPW; ++c) gs[c * G + j] = acc[c];
        }
        __syncthreads();
        if (j < H) {
#pragma unroll
            for (int c = 0; c < CPW; ++c) {
                if (!alive[c]) continue;
                const float* g = gs + c * G;
                const float ig = bd_sigmoid(g[j]);
                const float fg = bd_sigmoid(g[H + j]);
                const float gg = tanhf(g[2 * H + j]);
                const float og = bd_sigmoid(g[3 * H + j]);
                const float cc = fg * cs[c * H + j] + ig * gg;
                cs[c * H + j] = cc;
                hs[j * CPW + c] = og * tanhf(cc);
            }
        }
        __syncthreads();

        // 3. label logits, then softmax / clamp / first maximum by one wave per caption
        for (int e = j; e < CPW * L; e += nthr) {              // one thread per (caption, label)
            const int c = e / L, l = e % L;
            float acc = a.lo_b[l];
#pragma unroll 4
            for (int k = 0; k < H; ++k) acc = fmaf(a.lo_wt[(size_t)k * L + l], hs[k * CPW + c], acc);
            ps[l * CPW + c] = acc;
        }
        __syncthreads();
        for (int c = wid; c < CPW; c += nw) {
            float mx = -INFINITY;
            for (int l = lane; l < L; l += 64) mx = fmaxf(mx, ps[l * CPW + c]);
            mx = og_wave_max(mx);
            float s = 0.f;
            for (int l = lane; l < L; l += 64) s += expf(ps[l * CPW + c] - mx);
            s = og_wave_sum(s);
            float bv = -1.f;
            int bi = 0x7fffffff;
            for (int l = lane; l < L; l += 64) {
                float v = expf(ps[l * CPW + c] - mx) / s;
                v = fminf(fmaxf(v, 1e-5f), 1.0f);
                ps[l * CPW + c] = v;
                if (v > bv) { bv = v; bi = l; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if (lane == 0 && alive[c]) lab[c] = bi;
        }
        __syncthreads();

        // 4. xy_out(cat(h, label_softmax)) and the (x, y) draw
        // (one thread per (caption, output): these heads are a long chain per output, so the tile runs them side by side)
        for (int e = j; e < CPW * Q; e += nthr) {
            const int c = e / Q, q = e % Q;
            float acc = a.xyo_b[q];
#pragma unroll 4
            for (int k = 0; k < H; ++k) acc = fmaf(a.xyo_wt[(size_t)k * Q + q], hs[k * CPW + c], acc);
#pragma unroll 4
            for (int l = 0; l < L; ++l) acc = fmaf(a.xyo_wt[(size_t)(H + l) * Q + q], ps[l * CPW + c], acc);
            m1[c * Q + q] = acc;
        }
        __syncthreads();
        if (j < CPW && alive[j]) {
            const size_t bt = (size_t)(b0 + j) * T + t;
            const double* nz = a.noise + bt * 6;
            double x, y;
            bd_draw(m1 + j * Q, K, nz[0], nz[1], nz[2], a.trace ? a.trace + bt * TR + L : nullptr, &x, &y);
            a.samples[bt * 4 + 0] = x;
            a.samples[bt * 4 + 1] = y;
            // next_xy_embedding sees the drawn x and the step's INPUT y (DecoderRNN.py:166-170); the drawn values
            // become the next step's input only after the (w, h) draw
            gs[j * G + 0] = (float)x;
            gs[j * G + 1] = (float)y;
        }
        __syncthreads();
        for (int e = j; e < A * CPW; e += nthr) {
            const int i = e / CPW, c = e % CPW;
            es[e] = fmaf(a.nxy_w[2 * i + 1], st[c * 4 + 1], fmaf(a.nxy_w[2 * i], gs[c * G + 0], a.nxy_b[i]));
        }
        if (a.trace) {
            for (int e = j; e < L * CPW; e += nthr) {
                const int l = e / CPW, c = e % CPW;
                if (alive[c]) a.trace[((size_t)(b0 + c) * T + t) * TR + l] = ps[e];
            }
        }
        __syncthreads();

        // 5. wh_out(cat(h, label_softmax, next_xy_embedding)) and the (w, h) draw
        for (int e = j; e < CPW * Q; e += nthr) {
            const int c = e / Q, q = e % Q;
            float acc = a.who_b[q];
#pragma unroll 4
            for (int k = 0; k < H; ++k) acc = fmaf(a.who_wt[(size_t)k * Q + q], hs[k * CPW + c], acc);
#pragma unroll 4
            for (int l = 0; l < L; ++l) acc = fmaf(a.who_wt[(size_t)(H + l) * Q + q], ps[l * CPW + c], acc);
#pragma unroll 4
            for (int i = 0; i < A; ++i) acc = fmaf(a.who_wt[(size_t)(H + L + i) * Q + q], es[i * CPW + c], acc);
            m2[c * Q + q] = acc;
        }
        __syncthreads();
        if (j < CPW && alive[j]) {
            const size_t bt = (size_t)(b0 + j) * T + t;
            const double* nz = a.noise + bt * 6;
            double w, h;
            bd_draw(m2 + j * Q, K, nz[3], nz[4], nz[5], a.trace ? a.trace + bt * TR + L + Q : nullptr, &w, &h);
            a.samples[bt * 4 + 2] = w;
            a.samples[bt * 4 + 3] = h;
            a.labels[bt] = lab[j];
            // 6. the label and the four drawn values, rounded to fp32, are the next input
            st[j * 4 + 0] = gs[j * G + 0];
            st[j * 4 + 1] = gs[j * G + 1];
            st[j * 4 + 2] = (float)w;
            st[j * 4 + 3] = (float)h;
            len[j] = t + 1;
            if (lab[j] == a.eos) alive[j] = 0;
        }
        __syncthreads();
    }

    // entries past a caption's length are zero
    for (int c = 0; c < CPW; ++c) {
        const int b = b0 + c;
        if (b >= a.B) break;
        const int n = len[c];
        if (j == 0) a.lengths[b] = n;
        for (int e = n + j; e < T; e += nthr) a.labels[(size_t)b * T + e] = 0;
        for (int e = n * 4 + j; e < T * 4; e += nthr) a.samples[(size_t)b * T * 4 + e] = 0.0;
        if (a.trace)
            for (int e = n * TR + j; e < T * TR; e += nthr) a.trace[(size_t)b * T * TR + e] = 0.f;
    }
}

template <int CPW>
int bd_launch(const BoxDecodeArgs& a, hipStream_t stream) {
    const int H = a.H, G = 4 * H, I = 2 * a.A + H, Q = 6 * a.K;
    const size_t floats = (size_t)CPW * (I + H + a.L + a.A + H + G + 2 * Q + 4 + 3);
    const size_t lds = sizeof(float) * floats;
    if (lds > 64 * 1024) return OG_BAD_ARGS;
    const int threads = (G + 63) / 64 * 64;
    hipLaunchKernelGGL(box_decode_kernel<CPW>, dim3((a.B + CPW - 1) / CPW), dim3(threads), lds, stream, a);
    return og_launch_status();
}

}  // namespace

extern "C" {

int objgan_box_decode_default_cpw(void) { return 4; }

// h0, c0 [B][H]: the encoder's final (h_n, c_n), directions concatenated.  noise [B][T][6] doubles.
// l_emb [L][H]; xy_w / wh_w / nxy_w [A][2] and their biases [A] (nn.Linear layout); wt_ih [2A + H][4H], wt_hh [H][4H],
// lo_wt [H][L], xyo_wt [H + L][6K], who_wt [H + L + A][6K] are TRANSPOSED nn weights; gate order i, f, g, o.
// x0, y0, w0, r0: the first step's box input; sos / eos: label ids.  cpw: captions per workgroup (1, 2, 4, 8).
// labels [B][T] int32, lengths [B] int32 (steps taken, the <eos> step included), samples [B][T][4] doubles (x, y, w, h),
// trace (nullable) [B][T][L + 12K]: label softmax, then (pi, u, u, sigma, sigma, rho) of the xy and of the wh mixture.
// Entries past a caption's length are written as zero.
int objgan_box_decode(const float* h0, const float* c0, const double* noise,
                      const float* l_emb, const float* xy_w, const float* xy_b, const float* wh_w, const float* wh_b,
                      const float* nxy_w, const float* nxy_b, const float* wt_ih, const float* wt_hh,
                      const float* b_ih, const float* b_hh, const float* lo_wt, const float* lo_b,
                      const float* xyo_wt, const float* xyo_b, const float* who_wt, const float* who_b,
                      float x0, float y0, float w0, float r0,
                      int* labels, int* lengths, double* samples, float* trace,
                      int B, int T, int H, int L, int K, int A, int sos, int eos, int cpw, void* stream) {
    OG_ENTRY();
    if (H < 1 || 4 * H > 1024 || L < 1 || L > BD_MAX_L || K < 1 || K > BD_MAX_K || T < 1 || T > BD_MAX_T ||
        A < 1 || A > BD_MAX_A || sos < 0 || sos >= L || eos < 0 || eos >= L)
        return OG_BAD_ARGS;
    if (cpw != 1 && cpw != 2 && cpw != 4 && cpw != 8) return OG_BAD_ARGS;
    if (B <= 0) return OG_OK;
    BoxDecodeArgs a = {h0, c0, noise, l_emb, xy_w, xy_b, wh_w, wh_b, nxy_w, nxy_b, wt_ih, wt_hh, b_ih, b_hh,
                       lo_wt, lo_b, xyo_wt, xyo_b, who_wt, who_b, labels, lengths, samples, trace,
                       x0, y0, w0, r0, B, T, H, L, K, A, sos, eos};
    hipStream_t s = (hipStream_t)stream;
    switch (cpw) {
        case 1: return bd_launch<1>(a, s);
        case 2: return bd_launch<2>(a, s);
        case 4: return bd_launch<4>(a, s);
        default: return bd_launch<8>(a, s);
    }
}

}  // extern "C"

// Box generator, training step (reference box_generation/seq2seq/models/DecoderRNN.py:220-259 forward with is_training=1,
// loss/loss.py:142-150 Perplexity and :162-223 BBLoss, trainer/supervised_trainer.py:99-105 backward / clip / Adam).
//
// The reference trains one caption per step.  Here a step is a batch of B captions of lens[b] steps each:
//   objgan_box_train_forward   teacher-forced decode; tiling of box_decode.hip (a workgroup owns CPW captions, thread j
//                              owns gate row j, every sum of one caption is a fixed fmaf chain over its elements: a
//                              caption's rows depend neither on CPW, nor on its place, nor on B or T).  What the backward
//                              pass needs is left in a caller-owned workspace in global memory (T goes to 256).
//   objgan_box_train_loss      both losses over the trace, per-caption fp64 sums in step order, and dtrace = the gradient
//                              of  (lamda1 sum_b label_b + lamda2 sum_b box_b) / sum_b n_b  w.r.t. the activated trace.
//   objgan_box_train_backward  head deltas per (caption, step), BPTT per caption from its own last step, input deltas,
//                              then every weight gradient as ONE thread per element adding (caption, step) rows in
//                              (b, t) order: no float atomics, two runs give the same bits, rows past a caption's length
//                              are never read.
//   objgan_box_train_clip      global L2 norm of a flat gradient arena (ordered fp64 partials) and the divisor
//                              max(1, (norm + 1e-6) / max_norm) that objgan_adam_step_gated(grad_scale < 0) applies.
// All of it is fp32 VALU work.  Compiled with -ffp-contract=off: the dot products call fmaf explicitly.
#include "common.h"

namespace {

constexpr int BT_MAX_L = 256, BT_MAX_K = 8, BT_MAX_T = 256, BT_MAX_A = 64;
constexpr int BT_BX = 8;          // per-row box record: x_t, y_t, w_t, r_t, x_{t+1}, y_t, 1, 0

// workspace: B * T rows of RW floats, then hall [B][T + 1][H] (slot 0 = h0, slot t + 1 = h after step t)
struct BtLayout {
    int I, G, Q, RW;
    int xin, gat, cst, sm, es, bx, dlog, dm1, dm2, dhh, de, dg, dx;
};
__host__ __device__ inline BtLayout bt_layout(int H, int L, int K, int A) {
    BtLayout o;
    o.I = 2 * A + H; o.G = 4 * H; o.Q = 6 * K;
    int p = 0;
    o.xin = p; p += o.I;
    o.gat = p; p += o.G;
    o.cst = p; p += H;
    o.sm = p; p += L;
    o.es = p; p += A;
    o.bx = p; p += BT_BX;
    o.dlog = p; p += L;
    o.dm1 = p; p += o.Q;
    o.dm2 = p; p += o.Q;
    o.dhh = p; p += H;
    o.de = p; p += A;
    o.dg = p; p += o.G;
    o.dx = p; p += o.I;
    o.RW = p;
    return o;
}

struct BoxTrainArgs {
    const float* h0; const float* c0; const int* labels; const float* boxes; const int* lens;
    const float* l_emb;
    const float* xy_w; const float* xy_b;
    const float* wh_w; const float* wh_b;
    const float* nxy_w; const float* nxy_b;
    const float* wt_ih; const float* wt_hh;
    const float* b_ih; const float* b_hh;
    const float* lo_wt; const float* lo_b;
    const float* xyo_wt; const float* xyo_b;
    const float* who_wt; const float* who_b;
    float* trace; float* ws;
    float x0, y0, w0, r0;
    int B, T, H, L, K, A;
};

__device__ __forceinline__ float bt_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ int bt_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// raw [6K] -> activated (pi, u_a, u_b, sigma_a, sigma_b, rho), as bd_draw of box_decode.hip
__device__ __noinline__ void bt_activate(const float* raw, int K, float* par) {
    float e[BT_MAX_K];
    float mx = raw[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, raw[k]);
    float s = 0.f;
    for (int k = 0; k < K; ++k) { e[k] = expf(raw[k] - mx); s += e[k]; }
    for (int k = 0; k < K; ++k) {
        par[k] = e[k] / s;
        par[K + k] = raw[K + k];
        par[2 * K + k] = raw[2 * K + k];
        par[3 * K + k] = expf(raw[3 * K + k]);
        par[4 * K + k] = expf(raw[4 * K + k]);
        par[5 * K + k] = tanhf(raw[5 * K + k]);
    }
}

// grid = ceil(B / CPW), block = 4H rounded up to a wave.
// Dynamic LDS, floats: xs [I][CPW] | hs [H][CPW] | ps [L][CPW] | es [A][CPW] | cs [CPW][H] | gs [CPW][4H] |
//                      m1 [CPW][6K] | m2 [CPW][6K] | st [CPW][8] | then ints lab [CPW] | nlab [CPW] | len [CPW]
template <int CPW>
__global__ void __launch_bounds__(1024) bt_forward_kernel(BoxTrainArgs a) {
    extern __shared__ float4 sm4[];
    const int H = a.H, L = a.L, K = a.K, A = a.A, T = a.T;
    const BtLayout lo = bt_layout(H, L, K, A);
    const int G = lo.G, I = lo.I, Q = lo.Q;
    float* xs = reinterpret_cast<float*>(sm4);
    float* hs = xs + (size_t)I * CPW;
    float* ps = hs + (size_t)H * CPW;
    float* es = ps + (size_t)L * CPW;
    float* cs = es + (size_t)A * CPW;
    float* gs = cs + (size_t)CPW * H;
    float* m1 = gs + (size_t)CPW * G;
    float* m2 = m1 + CPW * Q;
    float* st = m2 + CPW * Q;
    int* lab = reinterpret_cast<int*>(st + CPW * 8);
    int* nlab = lab + CPW;
    int* len = nlab + CPW;

    const int j = threadIdx.x, nthr = blockDim.x;
    const int lane = j & 63, wid = j >> 6, nw = nthr >> 6;
    const int b0 = blockIdx.x * CPW;
    const int TR = L + 2 * Q;
    float* hall = a.ws + (size_t)a.B * T * lo.RW;

    for (int e = j; e < CPW * H; e += nthr) {
        const int c = e / H, k = e % H;
        const bool in = b0 + c < a.B;
        const float hv = in ? a.h0[(size_t)(b0 + c) * H + k] : 0.f;
        hs[k * CPW + c] = hv;
        cs[c * H + k] = in ? a.c0[(size_t)(b0 + c) * H + k] : 0.f;
        if (in) hall[(size_t)(b0 + c) * (T + 1) * H + k] = hv;
    }
    if (j < CPW) {
        st[j * 8 + 0] = a.x0; st[j * 8 + 1] = a.y0; st[j * 8 + 2] = a.w0; st[j * 8 + 3] = a.r0; st[j * 8 + 4] = a.x0;
        lab[j] = 0; nlab[j] = 0;
        len[j] = b0 + j < a.B ? bt_clampi(a.lens[b0 + j], 0, T) : 0;
    }
    const float gbias = j < G ? a.b_ih[j] + a.b_hh[j] : 0.f;
    __syncthreads();
    int maxlen = 0;
#pragma unroll
    for (int c = 0; c < CPW; ++c) maxlen = len[c] > maxlen ? len[c] : maxlen;

    for (int t = 0; t < maxlen; ++t) {
        // 0. the step's inputs: targets of column t (the means at t = 0), the next label, the next x
        if (j < CPW && t < len[j]) {
            const size_t bt1 = (size_t)(b0 + j) * (T + 1) + t;
            lab[j] = bt_clampi(a.labels[bt1], 0, L - 1);
            nlab[j] = bt_clampi(a.labels[bt1 + 1], 0, L - 1);
            if (t > 0) {
                st[j * 8 + 0] = a.boxes[bt1 * 4 + 0]; st[j * 8 + 1] = a.boxes[bt1 * 4 + 1];
                st[j * 8 + 2] = a.boxes[bt1 * 4 + 2]; st[j * 8 + 3] = a.boxes[bt1 * 4 + 3];
            }
            st[j * 8 + 4] = a.boxes[(bt1 + 1) * 4 + 0];
            float* bx = a.ws + ((size_t)(b0 + j) * T + t) * lo.RW + lo.bx;
            bx[0] = st[j * 8 + 0]; bx[1] = st[j * 8 + 1]; bx[2] = st[j * 8 + 2]; bx[3] = st[j * 8 + 3];
            bx[4] = st[j * 8 + 4]; bx[5] = st[j * 8 + 1]; bx[6] = 1.f; bx[7] = 0.f;
        }
        __syncthreads();

        // 1. input = cat(xy_embedding(x, y), wh_embedding(w, r), l_embedding[label])
        for (int e = j; e < I * CPW; e += nthr) {
            const int i = e / CPW, c = e % CPW;
            float v;
            if (i < A) v = fmaf(a.xy_w[2 * i + 1], st[c * 8 + 1], fmaf(a.xy_w[2 * i], st[c * 8 + 0], a.xy_b[i]));
            else if (i < 2 * A) {
                const int q = i - A;
                v = fmaf(a.wh_w[2 * q + 1], st[c * 8 + 3], fmaf(a.wh_w[2 * q], st[c * 8 + 2], a.wh_b[q]));
            } else v = a.l_emb[(size_t)lab[c] * H + (i - 2 * A)];
            xs[e] = v;
            if (t < len[c]) a.ws[((size_t)(b0 + c) * T + t) * lo.RW + lo.xin + i] = v;
        }
        // next_xy_embedding(x[t + 1], y[t]): the CURRENT y (DecoderRNN.py:149-150)
        for (int e = j; e < A * CPW; e += nthr) {
            const int i = e / CPW, c = e % CPW;
            const float v = fmaf(a.nxy_w[2 * i + 1], st[c * 8 + 1], fmaf(a.nxy_w[2 * i], st[c * 8 + 4], a.nxy_b[i]));
            es[e] = v;
            if (t < len[c]) a.ws[((size_t)(b0 + c) * T + t) * lo.RW + lo.es + i] = v;
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
                if (t >= len[c]) continue;
                const float* g = gs + c * G;
                const float ig = bt_sigmoid(g[j]);
                const float fg = bt_sigmoid(g[H + j]);
                const float gg = tanhf(g[2 * H + j]);
                const float og = bt_sigmoid(g[3 * H + j]);
                const float cc = fg * cs[c * H + j] + ig * gg;
                const float hh = og * tanhf(cc);
                cs[c * H + j] = cc;
                hs[j * CPW + c] = hh;
                float* row = a.ws + ((size_t)(b0 + c) * T + t) * lo.RW;
                row[lo.gat + j] = ig; row[lo.gat + H + j] = fg; row[lo.gat + 2 * H + j] = gg; row[lo.gat + 3 * H + j] = og;
                row[lo.cst + j] = cc;
                hall[((size_t)(b0 + c) * (T + 1) + t + 1) * H + j] = hh;
            }
        }
        __syncthreads();

        // 3. label logits, softmax (kept unclamped for the backward pass), clamp into the trace
        for (int e = j; e < CPW * L; e += nthr) {
            const int c = e / L, l = e % L;
            float acc = a.lo_b[l];
#pragma unroll 4
            for (int k = 0; k < H; ++k) acc = fmaf(a.lo_wt[(size_t)k * L + l], hs[k * CPW + c], acc);
            ps[l * CPW + c] = acc;
        }
        // 4. xy_out(cat(h, onehot(next label))) and wh_out(cat(h, onehot, next_xy_embedding))
        for (int e = j; e < CPW * Q; e += nthr) {
            const int c = e / Q, q = e % Q;
            float acc = a.xyo_b[q];
#pragma unroll 4
            for (int k = 0; k < H; ++k) acc = fmaf(a.xyo_wt[(size_t)k * Q + q], hs[k * CPW + c], acc);
            acc = fmaf(a.xyo_wt[(size_t)(H + nlab[c]) * Q + q], 1.0f, acc);
            m1[c * Q + q] = acc;
            float acc2 = a.who_b[q];
#pragma unroll 4
            for (int k = 0; k < H; ++k) acc2 = fmaf(a.who_wt[(size_t)k * Q + q], hs[k * CPW + c], acc2);
            acc2 = fmaf(a.who_wt[(size_t)(H + nlab[c]) * Q + q], 1.0f, acc2);
#pragma unroll 4
            for (int i = 0; i < A; ++i) acc2 = fmaf(a.who_wt[(size_t)(H + L + i) * Q + q], es[i * CPW + c], acc2);
            m2[c * Q + q] = acc2;
        }
        __syncthreads();
        for (int c = wid; c < CPW; c += nw) {
            float mx = -INFINITY;
            for (int l = lane; l < L; l += 64) mx = fmaxf(mx, ps[l * CPW + c]);
            mx = og_wave_max(mx);
            float s = 0.f;
            for (int l = lane; l < L; l += 64) s += expf(ps[l * CPW + c] - mx);
            s = og_wave_sum(s);
            if (t < len[c]) {
                float* row = a.ws + ((size_t)(b0 + c) * T + t) * lo.RW + lo.sm;
                float* tr = a.trace + ((size_t)(b0 + c) * T + t) * TR;
                for (int l = lane; l < L; l += 64) {
                    const float v = expf(ps[l * CPW + c] - mx) / s;
                    row[l] = v;
                    tr[l] = fminf(fmaxf(v, 1e-5f), 1.0f);
                }
            }
        }
        if (j < 2 * CPW) {
            const int c = j >> 1;
            if (t < len[c]) {
                float* tr = a.trace + ((size_t)(b0 + c) * T + t) * TR + L;
                if (j & 1) bt_activate(m2 + c * Q, K, tr + Q);
                else bt_activate(m1 + c * Q, K, tr);
            }
        }
        __syncthreads();
    }

    // entries past a caption's length are zero
    for (int c = 0; c < CPW; ++c) {
        const int b = b0 + c;
        if (b >= a.B) break;
        for (int e = len[c] * TR + j; e < T * TR; e += nthr) a.trace[(size_t)b * T * TR + e] = 0.f;
    }
}

template <int CPW>
int bt_fwd_launch(const BoxTrainArgs& a, hipStream_t stream) {
    const BtLayout lo = bt_layout(a.H, a.L, a.K, a.A);
    const size_t floats = (size_t)CPW * (lo.I + a.H + a.L + a.A + a.H + lo.G + 2 * lo.Q + 8 + 3);
    const size_t lds = sizeof(float) * floats;
    if (lds > 64 * 1024) return OG_BAD_ARGS;
    const int threads = (lo.G + 63) / 64 * 64;
    hipLaunchKernelGGL(bt_forward_kernel<CPW>, dim3((a.B + CPW - 1) / CPW), dim3(threads), lds, stream, a);
    return og_launch_status();
}

// ---- loss ----------------------------------------------------------------------------------------------------------
// sums [B][4] doubles (label term, box term, non-pad steps, arg-max matches), then sums[4B] = sum_b n_b.
__global__ void __launch_bounds__(256) bt_count_kernel(const int* labels, const int* lens, double* sums, int B, int T, int pad) {
    __shared__ long red[256];
    long n = 0;
    for (int b = threadIdx.x; b < B; b += 256) {
        const int len = bt_clampi(lens[b], 0, T);
        for (int t = 0; t < len; ++t) n += labels[(size_t)b * (T + 1) + t + 1] != pad ? 1 : 0;
    }
    red[threadIdx.x] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        long s = 0;
        for (int i = 0; i < 256; ++i) s += red[i];
        sums[(size_t)4 * B] = (double)s;
    }
}

// One mixture of the box term (loss.py:203-223) and its gradient.  par / dpar: (pi, u_a, u_b, s_a, s_b, rho) x K.
// gout: d loss / d pdf-value.  Returns the pdf value log(sum + 1e-5) + a_max.
__device__ __noinline__ float bt_pdf(const float* par, int K, float x, float y, float gout, float* dpar) {
    float av[BT_MAX_K], rv[BT_MAX_K];
    float amax = 0.f;
    int kmax = 0;
    for (int k = 0; k < K; ++k) {
        const float dx = x - par[K + k], dy = y - par[2 * K + k], sx = par[3 * K + k], sy = par[4 * K + k];
        const float rho = par[5 * K + k];
        const float qx = dx / sx, qy = dy / sy;
        const float z = qx * qx + qy * qy - 2.f * rho * (dx * dy / (sx * sy));
        av[k] = -z / (2.f * (1.f - rho * rho));
        if (k == 0 || av[k] > amax) { amax = av[k]; kmax = k; }
    }
    float S = 0.f;
    for (int k = 0; k < K; ++k) {
        const float sx = par[3 * K + k], sy = par[4 * K + k], rho = par[5 * K + k];
        const float nraw = 6.283185307179586f * sx * sy * sqrtf(1.f - rho * rho);
        rv[k] = par[k] * expf(av[k] - amax) / fmaxf(nraw, 1e-5f);
        S += rv[k];
    }
    const float gr = gout / (S + 1e-5f);
    const float gmax = gout * (1.f - S / (S + 1e-5f));        // through a_max: it does not cancel because of the 1e-5
    for (int k = 0; k < K; ++k) {
        const float dx = x - par[K + k], dy = y - par[2 * K + k], sx = par[3 * K + k], sy = par[4 * K + k];
        const float rho = par[5 * K + k], om = 1.f - rho * rho;
        const float zx = (dx / sx) * (dx / sx), zy = (dy / sy) * (dy / sy), zxy = dx * dy / (sx * sy);
        const float z = zx + zy - 2.f * rho * zxy;
        const float nraw = 6.283185307179586f * sx * sy * sqrtf(om);
        const float norm = fmaxf(nraw, 1e-5f);
        const float ga = gr * rv[k] + (k == kmax ? gmax : 0.f);
        const float gn = nraw >= 1e-5f ? -gr * rv[k] / norm : 0.f;
        const float gz = -ga / (2.f * om);
        dpar[k] = gr * expf(av[k] - amax) / norm;
        dpar[K + k] = gz * (-2.f * dx / (sx * sx) + 2.f * rho * dy / (sx * sy));
        dpar[2 * K + k] = gz * (-2.f * dy / (sy * sy) + 2.f * rho * dx / (sx * sy));
        dpar[3 * K + k] = gz * (-2.f * zx / sx + 2.f * rho * zxy / sx) + gn * nraw / sx;
        dpar[4 * K + k] = gz * (-2.f * zy / sy + 2.f * rho * zxy / sy) + gn * nraw / sy;
        dpar[5 * K + k] = ga * (zxy / om - z * rho / (om * om)) - gn * nraw * rho / om;
    }
    return logf(S + 1e-5f) + amax;
}

// grid = B, block = 64: lane handles steps lane, lane + 64, ...; thread 0 then adds the steps in order.
__global__ void __launch_bounds__(64) bt_loss_kernel(const float* trace, const int* labels, const float* boxes,
                                                     const int* lens, const float* weight, float lamda1, float lamda2,
                                                     double* sums, float* dtrace, int B, int T, int L, int K, int pad) {
    __shared__ float sl[BT_MAX_T], sb[BT_MAX_T];
    __shared__ int sn[BT_MAX_T], sa[BT_MAX_T];
    const int b = blockIdx.x, Q = 6 * K, TR = L + 2 * Q;
    const int len = bt_clampi(lens[b], 0, T);
    const float N = (float)sums[(size_t)4 * B];
    const float inv = N > 0.f ? 1.0f / N : 0.f;
    for (int t = threadIdx.x; t < T; t += 64) {
        float* d = dtrace + ((size_t)b * T + t) * TR;
        if (t >= len) {
            for (int e = 0; e < TR; ++e) d[e] = 0.f;
            continue;
        }
        const float* tr = trace + ((size_t)b * T + t) * TR;
        const size_t bt1 = (size_t)b * (T + 1) + t + 1;
        const int raw = labels[bt1];
        const int lab = bt_clampi(raw, 0, L - 1);
        const float w = lab == pad ? 0.f : weight[lab];
        const float mask = raw != 0 ? 1.f : 0.f;
        // nn.NLLLoss on the clamped probabilities themselves: -w[label] p[label], summed
        int best = 0;
        float bv = tr[0];
        for (int l = 0; l < L; ++l) {
            d[l] = 0.f;
            if (tr[l] > bv) { bv = tr[l]; best = l; }
        }
        const float p = tr[lab];
        sl[t] = -w * p;
        if (p > 1e-5f) d[lab] = -w * lamda1 * inv;
        const float gout = -mask * lamda2 * inv;
        const float v1 = bt_pdf(tr + L, K, boxes[bt1 * 4 + 0], boxes[bt1 * 4 + 1], gout, d + L);
        const float v2 = bt_pdf(tr + L + Q, K, boxes[bt1 * 4 + 2], boxes[bt1 * 4 + 3], gout, d + L + Q);
        sb[t] = -mask * v1 - mask * v2;
        sn[t] = raw != pad ? 1 : 0;
        sa[t] = (raw != pad && best == raw) ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double l = 0.0, bb = 0.0;
        int n = 0, acc = 0;
        for (int t = 0; t < len; ++t) { l += (double)sl[t]; bb += (double)sb[t]; n += sn[t]; acc += sa[t]; }
        sums[(size_t)b * 4 + 0] = l; sums[(size_t)b * 4 + 1] = bb;
        sums[(size_t)b * 4 + 2] = (double)n; sums[(size_t)b * 4 + 3] = (double)acc;
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------
// A. head deltas of one (caption, step): grid = B * T, block = 256.
__global__ void __launch_bounds__(256) bt_heads_bwd_kernel(BoxTrainArgs a, const float* dtrace) {
    __shared__ float dl[BT_MAX_L], d1[6 * BT_MAX_K], d2[6 * BT_MAX_K];
    __shared__ float dotp;
    const int H = a.H, L = a.L, K = a.K, A = a.A, T = a.T;
    const BtLayout lo = bt_layout(H, L, K, A);
    const int Q = lo.Q, TR = L + 2 * Q;
    const int b = blockIdx.x / T, t = blockIdx.x % T;
    if (t >= bt_clampi(a.lens[b], 0, T)) return;
    const int j = threadIdx.x;
    float* row = a.ws + ((size_t)b * T + t) * lo.RW;
    const float* tr = a.trace + ((size_t)b * T + t) * TR;
    const float* dt = dtrace + ((size_t)b * T + t) * TR;
    // label: clamp (gradient passes inside [1e-5, 1]) then softmax
    for (int l = j; l < L; l += 256) {
        const float s = row[lo.sm + l];
        dl[l] = (s >= 1e-5f && s <= 1.0f) ? dt[l] : 0.f;
    }
    __syncthreads();
    if (j < 64) {
        float acc = 0.f;
        for (int l = j; l < L; l += 64) acc = fmaf(dl[l], row[lo.sm + l], acc);
        acc = og_wave_sum(acc);
        if (j == 0) dotp = acc;
    }
    // mixtures: softmax over pi, identity, exp, tanh
    if (j >= 64 && j < 64 + 2 * K) {
        const int m = (j - 64) / K, k = (j - 64) % K;
        const float* par = tr + L + m * Q;
        const float* g = dt + L + m * Q;
        float* out = m ? d2 : d1;
        float s = 0.f;
        for (int q = 0; q < K; ++q) s = fmaf(g[q], par[q], s);
        out[k] = par[k] * (g[k] - s);
        out[K + k] = g[K + k];
        out[2 * K + k] = g[2 * K + k];
        out[3 * K + k] = g[3 * K + k] * par[3 * K + k];
        out[4 * K + k] = g[4 * K + k] * par[4 * K + k];
        out[5 * K + k] = g[5 * K + k] * (1.f - par[5 * K + k] * par[5 * K + k]);
    }
    __syncthreads();
    for (int l = j; l < L; l += 256) {
        const float v = row[lo.sm + l] * (dl[l] - dotp);
        row[lo.dlog + l] = v;
        dl[l] = v;
    }
    for (int q = j; q < Q; q += 256) { row[lo.dm1 + q] = d1[q]; row[lo.dm2 + q] = d2[q]; }
    __syncthreads();
    for (int k = j; k < H; k += 256) {
        float acc = 0.f;
        for (int l = 0; l < L; ++l) acc = fmaf(a.lo_wt[(size_t)k * L + l], dl[l], acc);
        for (int q = 0; q < Q; ++q) acc = fmaf(a.xyo_wt[(size_t)k * Q + q], d1[q], acc);
        for (int q = 0; q < Q; ++q) acc = fmaf(a.who_wt[(size_t)k * Q + q], d2[q], acc);
        row[lo.dhh + k] = acc;
    }
    for (int i = j; i < A; i += 256) {
        float acc = 0.f;
        for (int q = 0; q < Q; ++q) acc = fmaf(a.who_wt[(size_t)(H + L + i) * Q + q], d2[q], acc);
        row[lo.de + i] = acc;
    }
}

// B. BPTT: a workgroup owns CPW captions and walks them backwards, each from its own last step.
// LDS floats: dh [CPW][H] | dc [CPW][H] | dg [CPW][4H]
template <int CPW>
__global__ void __launch_bounds__(1024) bt_bptt_kernel(BoxTrainArgs a) {
    extern __shared__ float4 sm4[];
    const int H = a.H, T = a.T;
    const BtLayout lo = bt_layout(H, a.L, a.K, a.A);
    const int G = lo.G;
    float* dh = reinterpret_cast<float*>(sm4);
    float* dc = dh + CPW * H;
    float* dg = dc + CPW * H;
    const int j = threadIdx.x, nthr = blockDim.x, lane = j & 63, wid = j >> 6, nw = nthr >> 6;
    const int b0 = blockIdx.x * CPW;
    int len[CPW];
    int maxlen = 0;
#pragma unroll
    for (int c = 0; c < CPW; ++c) {
        len[c] = b0 + c < a.B ? bt_clampi(a.lens[b0 + c], 0, T) : 0;
        maxlen = len[c] > maxlen ? len[c] : maxlen;
    }
    for (int e = j; e < CPW * H; e += nthr) { dh[e] = 0.f; dc[e] = 0.f; }
    for (int e = j; e < CPW * G; e += nthr) dg[e] = 0.f;
    __syncthreads();
    for (int t = maxlen - 1; t >= 0; --t) {
        if (j < H) {
#pragma unroll
            for (int c = 0; c < CPW; ++c) {
                if (t >= len[c]) continue;
                float* row = a.ws + ((size_t)(b0 + c) * T + t) * lo.RW;
                const float ig = row[lo.gat + j], fg = row[lo.gat + H + j], gg = row[lo.gat + 2 * H + j];
                const float og = row[lo.gat + 3 * H + j];
                const float cprev = t > 0 ? (row - lo.RW)[lo.cst + j] : a.c0[(size_t)(b0 + c) * H + j];
                const float tc = tanhf(row[lo.cst + j]);
                const float dht = row[lo.dhh + j] + dh[c * H + j];
                const float dct = dc[c * H + j] + dht * og * (1.f - tc * tc);
                const float di = dct * gg * ig * (1.f - ig);
                const float df = dct * cprev * fg * (1.f - fg);
                const float dgg = dct * ig * (1.f - gg * gg);
                const float dO = dht * tc * og * (1.f - og);
                dc[c * H + j] = dct * fg;
                dg[c * G + j] = di; dg[c * G + H + j] = df; dg[c * G + 2 * H + j] = dgg; dg[c * G + 3 * H + j] = dO;
                row[lo.dg + j] = di; row[lo.dg + H + j] = df; row[lo.dg + 2 * H + j] = dgg; row[lo.dg + 3 * H + j] = dO;
            }
        }
        __syncthreads();
        // dh_rec[k] = sum_j weight_hh[j][k] dg[j]: one wave per k, lanes along j, a fixed reduction tree
        for (int k = wid; k < H; k += nw) {
            float acc[CPW];
#pragma unroll
            for (int c = 0; c < CPW; ++c) acc[c] = 0.f;
            for (int q = lane; q < G; q += 64) {
                const float w = a.wt_hh[(size_t)k * G + q];
#pragma unroll
                for (int c = 0; c < CPW; ++c) acc[c] = fmaf(w, dg[c * G + q], acc[c]);
            }
#pragma unroll
            for (int c = 0; c < CPW; ++c) {
                const float s = og_wave_sum(acc[c]);
                if (lane == 0 && t < len[c]) dh[c * H + k] = s;
            }
        }
        __syncthreads();
    }
}

// C. input deltas dx[i] = sum_j weight_ih[j][i] dg[j] of one (caption, step): grid = B * T, block = 256, a wave per i.
__global__ void __launch_bounds__(256) bt_dx_kernel(BoxTrainArgs a) {
    const int H = a.H, T = a.T;
    const BtLayout lo = bt_layout(H, a.L, a.K, a.A);
    const int b = blockIdx.x / T, t = blockIdx.x % T;
    if (t >= bt_clampi(a.lens[b], 0, T)) return;
    float* row = a.ws + ((size_t)b * T + t) * lo.RW;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int i = wid; i < lo.I; i += 4) {
        float acc = 0.f;
        for (int q = lane; q < lo.G; q += 64) acc = fmaf(a.wt_ih[(size_t)i * lo.G + q], row[lo.dg + q], acc);
        acc = og_wave_sum(acc);
        if (lane == 0) row[lo.dx + i] = acc;
    }
}

// D. weight gradients: out[r][c] = sum over (b, t < lens[b]) in that order of lft(b, t, r) * rgt(b, t, c).
// lft is a float row (base + b * bs + t * ts + r) or, with `hot` set, the one-hot of labels[b][t + hot - 1].
struct BtJob {
    const float* lft; long lbs, lts;
    const float* rgt; long rbs, rts;
    float* out;
    int R, C, hot;
};
constexpr int BT_JOBS = 20;
struct BtJobs { BtJob job[BT_JOBS]; };

__global__ void __launch_bounds__(256) bt_reduce_kernel(BtJobs js, const int* labels, const int* lens, int B, int T, int L) {
    const BtJob jb = js.job[blockIdx.y];
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)jb.R * jb.C) return;
    const int r = (int)(e / jb.C), c = (int)(e % jb.C);
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
        const int len = bt_clampi(lens[b], 0, T);
        const float* rg = jb.rgt + (size_t)b * jb.rbs + c;
        if (jb.hot) {
            const int* lb = labels + (size_t)b * (T + 1) + (jb.hot - 1);
            for (int t = 0; t < len; ++t)
                if (bt_clampi(lb[t], 0, L - 1) == r) acc = fmaf(1.0f, rg[(size_t)t * jb.rts], acc);
        } else {
            const float* lf = jb.lft + (size_t)b * jb.lbs + r;
#pragma unroll 4
            for (int t = 0; t < len; ++t) acc = fmaf(lf[(size_t)t * jb.lts], rg[(size_t)t * jb.rts], acc);
        }
    }
    jb.out[e] = acc;
}

// ---- global norm ---------------------------------------------------------------------------------------------------
constexpr int BT_NORM_BLOCKS = 256;
__global__ void __launch_bounds__(256) bt_sumsq_kernel(const float* g, long n, double* partial) {
    __shared__ double red[256];
    const long chunk = (n + BT_NORM_BLOCKS - 1) / BT_NORM_BLOCKS;
    const long lo = (long)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    double s = 0.0;
    for (long i = lo + threadIdx.x; i < hi; i += 256) s += (double)g[i] * (double)g[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
__global__ void bt_clip_kernel(const double* partial, float* out, float max_norm) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < BT_NORM_BLOCKS; ++i) s += partial[i];
    const float norm = (float)sqrt(s);
    // clip_grad_norm_: coefficient max_norm / (norm + 1e-6), capped at 1; out[0] is its reciprocal (a divisor >= 1)
    const float div = (norm + 1e-6f) / max_norm;
    out[0] = div > 1.f ? div : 1.f;
    out[1] = norm;
}

bool bt_shape_ok(int B, int T, int H, int L, int K, int A) {
    return B >= 0 && H >= 1 && 4 * H <= 1024 && L >= 1 && L <= BT_MAX_L && K >= 1 && K <= BT_MAX_K && T >= 1 &&
           T <= BT_MAX_T && A >= 1 && A <= BT_MAX_A;
}

}  // namespace

extern "C" {

// floats of the workspace shared by the three launches of one step (host-only query; 0 for a refused shape)
long objgan_box_train_ws_floats(int B, int T, int H, int L, int K, int A) {
    if (!bt_shape_ok(B, T, H, L, K, A)) return 0;
    const BtLayout lo = bt_layout(H, L, K, A);
    return (long)B * T * lo.RW + (long)B * (T + 1) * H;
}

int objgan_box_train_forward(const float* h0, const float* c0, const int* labels, const float* boxes, const int* lens,
                             const float* l_emb, const float* xy_w, const float* xy_b, const float* wh_w,
                             const float* wh_b, const float* nxy_w, const float* nxy_b, const float* wt_ih,
                             const float* wt_hh, const float* b_ih, const float* b_hh, const float* lo_wt,
                             const float* lo_b, const float* xyo_wt, const float* xyo_b, const float* who_wt,
                             const float* who_b, float x0, float y0, float w0, float r0, float* trace, float* ws,
                             long ws_floats, int B, int T, int H, int L, int K, int A, int cpw, void* stream) {
    OG_ENTRY();
    if (!bt_shape_ok(B, T, H, L, K, A)) return OG_BAD_ARGS;
    if (cpw != 1 && cpw != 2 && cpw != 4 && cpw != 8) return OG_BAD_ARGS;
    if (ws_floats < objgan_box_train_ws_floats(B, T, H, L, K, A)) return OG_BAD_ARGS;
    BoxTrainArgs a = {h0, c0, labels, boxes, lens, l_emb, xy_w, xy_b, wh_w, wh_b, nxy_w, nxy_b, wt_ih, wt_hh, b_ih, b_hh,
                      lo_wt, lo_b, xyo_wt, xyo_b, who_wt, who_b, trace, ws, x0, y0, w0, r0, B, T, H, L, K, A};
    hipStream_t s = (hipStream_t)stream;
    // the LDS limit is checked before the empty batch returns, so a refused tile is refused for every B
    const BtLayout lo = bt_layout(H, L, K, A);
    if (sizeof(float) * (size_t)cpw * (lo.I + H + L + A + H + lo.G + 2 * lo.Q + 8 + 3) > 64 * 1024) return OG_BAD_ARGS;
    if (B == 0) return OG_OK;
    if (!h0 || !c0 || !labels || !boxes || !lens || !trace || !ws) return OG_BAD_ARGS;
    switch (cpw) {
        case 1: return bt_fwd_launch<1>(a, s);
        case 2: return bt_fwd_launch<2>(a, s);
        case 4: return bt_fwd_launch<4>(a, s);
        default: return bt_fwd_launch<8>(a, s);
    }
}

// trace [B][T][L + 12K] (of objgan_box_train_forward), labels [B][T + 1] int32, boxes [B][T + 1][4], lens [B],
// weight [L] (the label weights; `pad` gets weight 0).  sums: 4B + 1 doubles -- per caption (label term, box term,
// non-pad steps, arg-max matches), then sum_b n_b.  dtrace [B][T][L + 12K], zero past each length and where the label
// clamp is active.
int objgan_box_train_loss(const float* trace, const int* labels, const float* boxes, const int* lens,
                          const float* weight, float lamda1, float lamda2, double* sums, float* dtrace,
                          int B, int T, int L, int K, int pad, void* stream) {
    OG_ENTRY();
    if (B < 0 || T < 1 || T > BT_MAX_T || L < 1 || L > BT_MAX_L || K < 1 || K > BT_MAX_K || pad < 0 || pad >= L)
        return OG_BAD_ARGS;
    if (B == 0) return OG_OK;
    if (!trace || !labels || !boxes || !lens || !weight || !sums || !dtrace) return OG_BAD_ARGS;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bt_count_kernel, dim3(1), dim3(256), 0, s, labels, lens, sums, B, T, pad);
    hipLaunchKernelGGL(bt_loss_kernel, dim3(B), dim3(64), 0, s, trace, labels, boxes, lens, weight, lamda1, lamda2,
                       sums, dtrace, B, T, L, K, pad);
    return og_launch_status();
}

// grads: the 17 gradient tensors in the kernel's layout and order, every element written.
int objgan_box_train_backward(const float* dtrace, const float* trace, const float* c0, const int* labels,
                              const int* lens, const float* wt_ih, const float* wt_hh, const float* lo_wt,
                              const float* xyo_wt, const float* who_wt, float* const* grads, float* ws, long ws_floats,
                              int B, int T, int H, int L, int K, int A, int cpw, void* stream) {
    OG_ENTRY();
    if (!bt_shape_ok(B, T, H, L, K, A)) return OG_BAD_ARGS;
    if (cpw != 1 && cpw != 2 && cpw != 4 && cpw != 8) return OG_BAD_ARGS;
    if (ws_floats < objgan_box_train_ws_floats(B, T, H, L, K, A)) return OG_BAD_ARGS;
    const BtLayout lo = bt_layout(H, L, K, A);
    const size_t lds = sizeof(float) * (size_t)cpw * (2 * H + lo.G);
    if (lds > 64 * 1024) return OG_BAD_ARGS;
    if (B == 0) return OG_OK;
    if (!dtrace || !trace || !c0 || !labels || !lens || !wt_ih || !wt_hh || !lo_wt || !xyo_wt || !who_wt || !grads || !ws)
        return OG_BAD_ARGS;
    for (int i = 0; i < 17; ++i)
        if (!grads[i]) return OG_BAD_ARGS;
    hipStream_t s = (hipStream_t)stream;
    BoxTrainArgs a = {};
    a.c0 = c0; a.labels = labels; a.lens = lens; a.wt_ih = wt_ih; a.wt_hh = wt_hh; a.lo_wt = lo_wt; a.xyo_wt = xyo_wt;
    a.who_wt = who_wt; a.trace = const_cast<float*>(trace); a.ws = ws;
    a.B = B; a.T = T; a.H = H; a.L = L; a.K = K; a.A = A;
    hipLaunchKernelGGL(bt_heads_bwd_kernel, dim3(B * T), dim3(256), 0, s, a, dtrace);
    const int threads = (lo.G + 63) / 64 * 64;
    const dim3 grid((B + cpw - 1) / cpw);
    switch (cpw) {
        case 1: hipLaunchKernelGGL(bt_bptt_kernel<1>, grid, dim3(threads), lds, s, a); break;
        case 2: hipLaunchKernelGGL(bt_bptt_kernel<2>, grid, dim3(threads), lds, s, a); break;
        case 4: hipLaunchKernelGGL(bt_bptt_kernel<4>, grid, dim3(threads), lds, s, a); break;
        default: hipLaunchKernelGGL(bt_bptt_kernel<8>, grid, dim3(threads), lds, s, a); break;
    }
    hipLaunchKernelGGL(bt_dx_kernel, dim3(B * T), dim3(256), 0, s, a);

    const long rs = (long)T * lo.RW, ts = lo.RW, hbs = (long)(T + 1) * H;
    const float* hall = ws + (size_t)B * T * lo.RW;
    const float* one = ws + lo.bx + 6;
    const int I = lo.I, G = lo.G, Q = lo.Q;
    BtJobs js;
    int n = 0;
    auto add = [&](const float* lft, long lbs, long lts, const float* rgt, float* out, int R, int C, int hot) {
        js.job[n++] = BtJob{lft, lbs, lts, rgt, rs, ts, out, R, C, hot};
    };
    add(ws + lo.dx + 2 * A, rs, ts, ws + lo.dx + 2 * A, grads[0], L, H, 1);              // l_emb: one-hot(label[t]) x dx
    add(ws + lo.dx, rs, ts, ws + lo.bx + 0, grads[1], A, 2, 0);                          // xy_w
    add(ws + lo.dx, rs, ts, one, grads[2], A, 1, 0);                                     // xy_b
    add(ws + lo.dx + A, rs, ts, ws + lo.bx + 2, grads[3], A, 2, 0);                      // wh_w
    add(ws + lo.dx + A, rs, ts, one, grads[4], A, 1, 0);                                 // wh_b
    add(ws + lo.de, rs, ts, ws + lo.bx + 4, grads[5], A, 2, 0);                          // nxy_w
    add(ws + lo.de, rs, ts, one, grads[6], A, 1, 0);                                     // nxy_b
    add(ws + lo.xin, rs, ts, ws + lo.dg, grads[7], I, G, 0);                             // wt_ih
    add(hall, hbs, H, ws + lo.dg, grads[8], H, G, 0);                                    // wt_hh: h before the step
    add(one, rs, ts, ws + lo.dg, grads[9], 1, G, 0);                                     // b_ih
    add(one, rs, ts, ws + lo.dg, grads[10], 1, G, 0);                                    // b_hh
    add(hall + H, hbs, H, ws + lo.dlog, grads[11], H, L, 0);                             // lo_wt: h after the step
    add(one, rs, ts, ws + lo.dlog, grads[12], 1, L, 0);                                  // lo_b
    add(hall + H, hbs, H, ws + lo.dm1, grads[13], H, Q, 0);                              // xyo_wt rows of h
    add(one, rs, ts, ws + lo.dm1, grads[13] + (size_t)H * Q, L, Q, 2);                   //        rows of the next label
    add(one, rs, ts, ws + lo.dm1, grads[14], 1, Q, 0);                                   // xyo_b
    add(hall + H, hbs, H, ws + lo.dm2, grads[15], H, Q, 0);                              // who_wt
    add(one, rs, ts, ws + lo.dm2, grads[15] + (size_t)H * Q, L, Q, 2);
    add(ws + lo.es, rs, ts, ws + lo.dm2, grads[15] + (size_t)(H + L) * Q, A, Q, 0);
    add(one, rs, ts, ws + lo.dm2, grads[16], 1, Q, 0);                                   // who_b
    long most = 0;
    for (int i = 0; i < n; ++i) most = (long)js.job[i].R * js.job[i].C > most ? (long)js.job[i].R * js.job[i].C : most;
    hipLaunchKernelGGL(bt_reduce_kernel, dim3((unsigned)((most + 255) / 256), n), dim3(256), 0, s, js, labels, lens, B, T, L);
    return og_launch_status();
}

// g: n floats (a flat gradient arena); partials: >= 256 doubles of scratch; out: 2 floats -- the divisor
// max(1, (norm + 1e-6) / max_norm) (objgan_adam_step_gated with grad_scale < 0 divides by it) and the norm.
int objgan_box_train_clip(const float* g, long n, float max_norm, double* partials, float* out, void* stream) {
    OG_ENTRY();
    if (n <= 0 || !(max_norm > 0.f) || !g || !partials || !out) return OG_BAD_ARGS;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bt_sumsq_kernel, dim3(BT_NORM_BLOCKS), dim3(256), 0, s, g, n, partials);
    hipLaunchKernelGGL(bt_clip_kernel, dim3(1), dim3(64), 0, s, partials, out, max_norm);
    return og_launch_status();
}

}  // extern "C"

// Trainable bidirectional LSTM text encoder (DAMSM pretraining; reference model.py:85-179 RNN_ENCODER in training
// mode: nn.Embedding -> nn.Dropout -> nn.LSTM(batch_first, bidirectional) on a packed sequence).
//
//   objgan_lstm_bidir_train_forward   the pass of csrc/lstm.hip (same tiling, same per-caption fmaf chains: with a null
//                                     keep-mask `out` and `hn` are its bits), with the embedding dropout applied to the
//                                     word vector and a trace left for the backward pass
//   objgan_lstm_bidir_backward        (a) BPTT per (caption, direction) -> gate deltas, (b) input deltas per position,
//                                     (c) weight and bias gradients, one thread per element adding its (b, t) rows in
//                                     (b, t) order, (d) the embedding table's gradient: the first occurrence of a token
//                                     adds the rows of all its occurrences in (b, t) order
//
// fp32 VALU work, compiled with -ffp-contract=off: every fused multiply-add is an explicit fmaf.  No float atomics:
// two runs give the same bits, and a caption's trace and gate deltas do not depend on the batch around it.
//
// Workspace (objgan_lstm_bidir_train_ws_floats floats, sections in this order):
//   gates [B][2][L][4H]   activated gates i, f, g, o           (forward)
//   cell  [B][2][L][H]    cell state after the step at t       (forward)
//   hid   [B][2][L][H]    hidden state after the step at t     (forward; `out` may be truncated to Lout < L)
//   x     [B][L][I]       the word vectors after dropout       (forward)
//   dgate [B][2][L][4H]   deltas of the gate pre-activations   (backward a)
//   dx    [B][L][I]       deltas of the embedded words         (backward b)
// Everything at positions t >= len is zero.
#include "common.h"

__device__ __forceinline__ float lstm_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

struct LstmWs {
    long gates, cell, hid, x, dgate, dx, total;
};

static LstmWs lstm_ws(long B, long L, long I, long H) {
    LstmWs w;
    w.gates = 0;
    w.cell = w.gates + B * 2 * L * 4 * H;
    w.hid = w.cell + B * 2 * L * H;
    w.x = w.hid + B * 2 * L * H;
    w.dgate = w.x + B * L * I;
    w.dx = w.dgate + B * 2 * L * 4 * H;
    w.total = w.dx + B * L * I;
    return w;
}

// grid = (B, 2), block = 4H threads rounded up to a wave (<= 1024); dynamic LDS = (I + 2H + 4H) floats
__global__ void lstm_bidir_train_fwd_kernel(const float* __restrict__ table, const long* __restrict__ captions,
                                            const int* __restrict__ lens, const unsigned char* __restrict__ keep,
                                            float scale,
                                            const float* __restrict__ wt_ih, const float* __restrict__ wt_hh,
                                            const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                            float* __restrict__ out, float* __restrict__ hn,
                                            float* __restrict__ gates, float* __restrict__ cell,
                                            float* __restrict__ hid, float* __restrict__ xw,
                                            int L, int Lout, int I, int H, int ntoken) {
    extern __shared__ float sm[];
    float* xs = sm;             // [I]
    float* hs = xs + I;         // [H]
    float* cs = hs + H;         // [H]
    float* gs = cs + H;         // [4H]
    const int b = blockIdx.x, dir = blockIdx.y;
    const int j = threadIdx.x;
    const int G = 4 * H;
    int len = lens[b];
    len = len < 0 ? 0 : (len > L ? L : len);
    const float* wi = wt_ih + (size_t)dir * I * G;
    const float* wh = wt_hh + (size_t)dir * H * G;
    const float bias = j < G ? b_ih[dir * G + j] + b_hh[dir * G + j] : 0.f;
    if (j < H) { hs[j] = 0.f; cs[j] = 0.f; }
    float* ob = out + ((size_t)b * 2 * H + (size_t)dir * H) * Lout;
    float* gb = gates + ((size_t)b * 2 + dir) * L * G;
    float* cb = cell + ((size_t)b * 2 + dir) * L * H;
    float* hb = hid + ((size_t)b * 2 + dir) * L * H;
    float* xb = xw + (size_t)b * L * I;
    // positions past the caption length are zero (pad_packed_sequence + post_process_words), in the trace as well
    for (int e = j; e < H * Lout; e += blockDim.x) {
        const int t = e % Lout;
        if (t >= len) ob[(size_t)(e / Lout) * Lout + t] = 0.f;
    }
    for (int e = len * G + j; e < L * G; e += blockDim.x) gb[e] = 0.f;
    for (int e = len * H + j; e < L * H; e += blockDim.x) { cb[e] = 0.f; hb[e] = 0.f; }
    if (dir == 0)
        for (int e = len * I + j; e < L * I; e += blockDim.x) xb[e] = 0.f;
    for (int s = 0; s < len; ++s) {
        const int t = dir == 0 ? s : len - 1 - s;
        long tok = captions[(size_t)b * L + t];
        tok = tok < 0 ? 0 : (tok >= ntoken ? ntoken - 1 : tok);
        __syncthreads();
        for (int i = j; i < I; i += blockDim.x) {
            float v = table[(size_t)tok * I + i];
            if (keep) v = keep[((size_t)b * L + t) * I + i] ? v * scale : 0.f;
            xs[i] = v;
            if (dir == 0) xb[(size_t)t * I + i] = v;
        }
        __syncthreads();
        if (j < G) {
            float acc = bias;
            for (int i = 0; i < I; ++i) acc = fmaf(wi[(size_t)i * G + j], xs[i], acc);
            for (int k = 0; k < H; ++k) acc = fmaf(wh[(size_t)k * G + j], hs[k], acc);
            gs[j] = acc;
        }
        __syncthreads();
        if (j < H) {
            const float ig = lstm_sigmoid(gs[j]);
            const float fg = lstm_sigmoid(gs[H + j]);
            const float gg = tanhf(gs[2 * H + j]);
            const float og = lstm_sigmoid(gs[3 * H + j]);
            const float c = fmaf(ig, gg, fg * cs[j]);       // the contraction csrc/lstm.hip compiles to
            const float h = og * tanhf(c);
            cs[j] = c;
            hs[j] = h;
            if (t < Lout) ob[(size_t)j * Lout + t] = h;
            float* g = gb + (size_t)t * G;
            g[j] = ig;
            g[H + j] = fg;
            g[2 * H + j] = gg;
            g[3 * H + j] = og;
            cb[(size_t)t * H + j] = c;
            hb[(size_t)t * H + j] = h;
        }
    }
    __syncthreads();
    if (j < H) hn[(size_t)b * 2 * H + dir * H + j] = hs[j];
}

// (a) grid = (B, 2), block = 4H threads rounded up to a wave; dynamic LDS = 4H floats.  Thread j < H owns hidden unit j:
// its cell delta and its recurrent hidden delta stay in registers; the four gate deltas of the step go through LDS to
// the W_hh^T product, which reads row r of the UNTRANSPOSED w_hh [4H][H] as consecutive floats across threads.
__global__ void lstm_bptt_kernel(const float* __restrict__ d_out, const float* __restrict__ d_hn,
                                 const float* __restrict__ gates, const float* __restrict__ cell,
                                 const int* __restrict__ lens, const float* __restrict__ w_hh,
                                 float* __restrict__ dgate, int L, int Lout, int H) {
    extern __shared__ float sm[];
    float* dgs = sm;            // [4H]
    const int b = blockIdx.x, dir = blockIdx.y;
    const int j = threadIdx.x;
    const int G = 4 * H;
    int len = lens[b];
    len = len < 0 ? 0 : (len > L ? L : len);
    const float* wh = w_hh + (size_t)dir * G * H;
    const float* gb = gates + ((size_t)b * 2 + dir) * L * G;
    const float* cb = cell + ((size_t)b * 2 + dir) * L * H;
    float* db = dgate + ((size_t)b * 2 + dir) * L * G;
    for (int e = len * G + j; e < L * G; e += blockDim.x) db[e] = 0.f;
    float dh_rec = 0.f, dc = 0.f;
    for (int s = len - 1; s >= 0; --s) {
        const int t = dir == 0 ? s : len - 1 - s;
        const int tp = dir == 0 ? t - 1 : t + 1;        // the position of the step before (s > 0)
        if (j < H) {
            float dh = dh_rec;
            if (d_out && t < Lout) dh += d_out[((size_t)b * 2 * H + (size_t)dir * H + j) * Lout + t];
            if (d_hn && s == len - 1) dh += d_hn[(size_t)b * 2 * H + dir * H + j];
            const float* g = gb + (size_t)t * G;
            const float ig = g[j], fg = g[H + j], gg = g[2 * H + j], og = g[3 * H + j];
            const float c = cb[(size_t)t * H + j];
            const float cp = s > 0 ? cb[(size_t)tp * H + j] : 0.f;
            const float tc = tanhf(c);
            const float d_o = dh * tc;
            const float dct = fmaf(dh * og, 1.0f - tc * tc, dc);
            const float a_i = (dct * gg) * (ig * (1.0f - ig));
            const float a_f = (dct * cp) * (fg * (1.0f - fg));
            const float a_g = (dct * ig) * (1.0f - gg * gg);
            const float a_o = d_o * (og * (1.0f - og));
            dc = dct * fg;
            dgs[j] = a_i;
            dgs[H + j] = a_f;
            dgs[2 * H + j] = a_g;
            dgs[3 * H + j] = a_o;
            float* d = db + (size_t)t * G;
            d[j] = a_i;
            d[H + j] = a_f;
            d[2 * H + j] = a_g;
            d[3 * H + j] = a_o;
        }
        __syncthreads();
        if (j < H && s > 0) {
            float acc = 0.f;
            for (int r = 0; r < G; ++r) acc = fmaf(wh[(size_t)r * H + j], dgs[r], acc);
            dh_rec = acc;
        }
        __syncthreads();
    }
}

// (b) grid = B L positions, block = 256; dynamic LDS = 8H floats (the gate deltas of both directions at the position).
// dx[b][t][i] = keep scale sum_dir sum_j w_ih[dir][j][i] dgate[b][dir][t][j]; w_ih [2][4H][I] untransposed.
__global__ __launch_bounds__(256) void lstm_dx_kernel(const float* __restrict__ dgate, const int* __restrict__ lens,
                                                      const unsigned char* __restrict__ keep, float scale,
                                                      const float* __restrict__ w_ih, float* __restrict__ dx,
                                                      int L, int I, int H) {
    extern __shared__ float sm[];
    const int G = 4 * H;
    const int b = blockIdx.x / L, t = blockIdx.x % L;
    int len = lens[b];
    len = len < 0 ? 0 : (len > L ? L : len);
    float* row = dx + (size_t)blockIdx.x * I;
    if (t >= len) {
        for (int i = threadIdx.x; i < I; i += blockDim.x) row[i] = 0.f;
        return;
    }
    for (int e = threadIdx.x; e < 2 * G; e += blockDim.x)
        sm[e] = dgate[(((size_t)b * 2 + e / G) * L + t) * G + e % G];
    __syncthreads();
    for (int i = threadIdx.x; i < I; i += blockDim.x) {
        float acc = 0.f;
        for (int r = 0; r < 2 * G; ++r) acc = fmaf(w_ih[(size_t)r * I + i], sm[r], acc);
        if (keep) acc = keep[(size_t)blockIdx.x * I + i] ? acc * scale : 0.f;
        row[i] = acc;
    }
}

// (c) grid = 2 * 4H gate rows (dir, j), block = 256 threads over the I + H columns of the row: columns < I belong to
// weight_ih (x the word vector of the position), the others to weight_hh (x the hidden state of the step before).
// Every element is one thread's sum over the positions in (b, t) order; thread 0 also sums the row's bias gradient.
__global__ __launch_bounds__(256) void lstm_wgrad_kernel(const float* __restrict__ dgate, const float* __restrict__ xw,
                                                         const float* __restrict__ hid, const int* __restrict__ lens,
                                                         float* __restrict__ d_w_ih, float* __restrict__ d_w_hh,
                                                         float* __restrict__ d_b_ih, float* __restrict__ d_b_hh,
                                                         int B, int L, int I, int H) {
    const int G = 4 * H;
    const int dir = blockIdx.x / G, j = blockIdx.x % G;
    for (int col = threadIdx.x; col < I + H; col += blockDim.x) {
        const bool ih = col < I;
        const int k = col - I;
        float acc = 0.f, bsum = 0.f;
        for (int b = 0; b < B; ++b) {
            int len = lens[b];
            len = len < 0 ? 0 : (len > L ? L : len);
            const float* dg = dgate + ((size_t)b * 2 + dir) * L * G + j;
            const float* hb = hid + ((size_t)b * 2 + dir) * L * H;
            for (int t = 0; t < len; ++t) {
                const float d = dg[(size_t)t * G];
                bsum += d;
                if (ih) {
                    acc = fmaf(d, xw[((size_t)b * L + t) * I + col], acc);
                } else {
                    const int tp = dir == 0 ? t - 1 : t + 1;
                    if (tp >= 0 && tp < len) acc = fmaf(d, hb[(size_t)tp * H + k], acc);
                }
            }
        }
        if (ih) d_w_ih[(size_t)blockIdx.x * I + col] = acc;
        else d_w_hh[(size_t)blockIdx.x * H + k] = acc;
        if (col == 0) { d_b_ih[blockIdx.x] = bsum; d_b_hh[blockIdx.x] = bsum; }
    }
}

__global__ __launch_bounds__(256) void lstm_zero_kernel(float* __restrict__ p, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = 0.f;
}

__device__ __forceinline__ long lstm_token_at(const long* captions, const int* lens, int p, int L, int ntoken) {
    int len = lens[p / L];
    len = len < 0 ? 0 : (len > L ? L : len);
    if (p % L >= len) return -1;                        // not a word of its caption
    const long tok = captions[p];
    return tok < 0 ? 0 : (tok >= ntoken ? ntoken - 1 : tok);
}

// (d) grid = B L positions, block = 256, after lstm_zero_kernel over the table's gradient.  The position that is the
// first occurrence of its token in (b, t) order adds the dx rows of the later occurrences in that order and writes
// the token's row; no other block writes that row.
__global__ __launch_bounds__(256) void lstm_table_grad_kernel(const float* __restrict__ dx,
                                                              const long* __restrict__ captions,
                                                              const int* __restrict__ lens, float* __restrict__ d_table,
                                                              int P, int L, int I, int ntoken) {
    __shared__ int seen;
    const int p = blockIdx.x;
    const long tok = lstm_token_at(captions, lens, p, L, ntoken);
    if (tok < 0) return;
    if (threadIdx.x == 0) seen = 0;
    __syncthreads();
    for (int q = threadIdx.x; q < p; q += blockDim.x)
        if (lstm_token_at(captions, lens, q, L, ntoken) == tok) seen = 1;
    __syncthreads();
    if (seen) return;
    for (int i = threadIdx.x; i < I; i += blockDim.x) {
        float acc = dx[(size_t)p * I + i];
        for (int q = p + 1; q < P; ++q)
            if (lstm_token_at(captions, lens, q, L, ntoken) == tok) acc += dx[(size_t)q * I + i];
        d_table[(size_t)tok * I + i] = acc;
    }
}

// what lstm_bidir_launch of csrc/lstm.hip refuses
static bool lstm_train_shape_ok(int L, int Lout, int I, int H, int ntoken) {
    if (4 * H > 1024 || H < 1 || I < 1 || L < 1 || Lout < 1 || ntoken < 1) return false;
    return sizeof(float) * (size_t)(I + 6 * H) <= 64 * 1024;
}

extern "C" {

long objgan_lstm_bidir_train_ws_floats(int B, int L, int I, int H) {
    if (B < 0 || L < 1 || I < 1 || H < 1) return 0;
    return lstm_ws(B, L, I, H).total;
}

int objgan_lstm_bidir_train_forward(const float* table, const long* captions, const int* lens,
                                    const unsigned char* keep, float scale,
                                    const float* wt_ih, const float* wt_hh, const float* b_ih, const float* b_hh,
                                    float* out, float* hn, float* ws, long ws_floats,
                                    int B, int L, int Lout, int I, int H, int ntoken, void* stream) {
    OG_ENTRY();
    if (!lstm_train_shape_ok(L, Lout, I, H, ntoken)) return OG_BAD_ARGS;
    if (B <= 0) return OG_OK;
    const LstmWs w = lstm_ws(B, L, I, H);
    if (!ws || ws_floats < w.total) return OG_BAD_ARGS;
    const int threads = (4 * H + 63) / 64 * 64;
    const size_t lds = sizeof(float) * (size_t)(I + 6 * H);
    hipLaunchKernelGGL(lstm_bidir_train_fwd_kernel, dim3(B, 2), dim3(threads), lds, (hipStream_t)stream,
                       table, captions, lens, keep, scale, wt_ih, wt_hh, b_ih, b_hh, out, hn,
                       ws + w.gates, ws + w.cell, ws + w.hid, ws + w.x, L, Lout, I, H, ntoken);
    return og_launch_status();
}

int objgan_lstm_bidir_backward(const float* d_out, const float* d_hn, const long* captions, const int* lens,
                               const unsigned char* keep, float scale, const float* w_ih, const float* w_hh,
                               float* ws, long ws_floats, float* d_w_ih, float* d_w_hh, float* d_b_ih, float* d_b_hh,
                               float* d_table, int B, int L, int Lout, int I, int H, int ntoken, void* stream) {
    OG_ENTRY();
    if (!lstm_train_shape_ok(L, Lout, I, H, ntoken)) return OG_BAD_ARGS;
    if (B < 0 || !d_w_ih || !d_w_hh || !d_b_ih || !d_b_hh || !d_table) return OG_BAD_ARGS;
    const LstmWs w = lstm_ws(B, L, I, H);
    if (B > 0 && (!ws || ws_floats < w.total)) return OG_BAD_ARGS;
    hipStream_t st = (hipStream_t)stream;
    const int G = 4 * H;
    if (B > 0) {
        hipLaunchKernelGGL(lstm_bptt_kernel, dim3(B, 2), dim3((G + 63) / 64 * 64), sizeof(float) * (size_t)G, st,
                           d_out, d_hn, ws + w.gates, ws + w.cell, lens, w_hh, ws + w.dgate, L, Lout, H);
        hipLaunchKernelGGL(lstm_dx_kernel, dim3(B * L), dim3(256), sizeof(float) * (size_t)(2 * G), st,
                           ws + w.dgate, lens, keep, scale, w_ih, ws + w.dx, L, I, H);
    }
    hipLaunchKernelGGL(lstm_wgrad_kernel, dim3(2 * G), dim3(256), 0, st, ws + w.dgate, ws + w.x, ws + w.hid, lens,
                       d_w_ih, d_w_hh, d_b_ih, d_b_hh, B, L, I, H);
    const long nt = (long)ntoken * I;
    hipLaunchKernelGGL(lstm_zero_kernel, dim3(og_stream_grid(nt, 256)), dim3(256), 0, st, d_table, nt);
    if (B > 0)
        hipLaunchKernelGGL(lstm_table_grad_kernel, dim3(B * L), dim3(256), 0, st, ws + w.dx, captions, lens, d_table,
                           B * L, L, I, ntoken);
    return og_launch_status();
}

}  // extern "C"

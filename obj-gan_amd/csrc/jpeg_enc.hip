// Baseline JPEG ENCODE on the device: the files Pillow's default `Image.save(path)` / `save(format='JPEG', quality=q)`
// writes (libjpeg-turbo: YCbCr 4:2:0, the Annex-K Huffman tables, one interleaved scan), BYTE FOR BYTE, for a batch of
// RGB images of one size whose sides are multiples of 16.  Replaces the per-image host loop of evaluator.py
// save_singleimages (reference image_generation/evaluator.py:225-233): what crosses PCIe is the compressed files.
//
//   jpeg_enc_transform_kernel  one lane per 8 x 8 block: bytes (uint8 input, or the fp32 [-1, 1] generator output through
//       the host's add(1) div(2) mul(255) clamp truncate, one fp32 rounding each), jccolor.c's 16-bit fixed-point YCbCr,
//       jcsample.c's h2v2 box filter with its alternating 1 / 2 bias, level shift, jfdctint.c's forward DCT (CONST_BITS 13,
//       PASS1_BITS 2, output scaled by 8) and jcdctmgr.c's quantisation (|c| + 4q) / 8q -> int16 in zigzag order, blocks in
//       scan order (Y00 Y01 Y10 Y11 Cb Cr per MCU).  Integer arithmetic only.
//   jpeg_enc_entropy_kernel    one workgroup per image.  Every lane owns a run of consecutive blocks: it sums the bit
//       lengths of their code strings (the DC predictor is the previous block of the same component, read from the
//       coefficient buffer), a workgroup scan turns the sums into bit offsets, and the lane writes its bits at its offset
//       into the image's raw stream (whole 32-bit words stored, the shared word at either seam OR-ed in).  The last byte
//       is padded with ones.  Byte stuffing is the same shape again: FF bytes counted per run of words, scanned, final
//       bytes written behind the header, FF D9 behind them.  The Huffman code tables are derived in LDS from the header
//       itself, so header and stream cannot disagree.
//
// Slot size (bytes per image in the output buffer), from the code tables:
//   DC: the longest code is 11 bits (chroma, category 11) and carries 11 value bits: 22 bits.
//   AC: the longest code is 16 bits and the largest category 10: 26 bits per nonzero coefficient.  A block with k < 63
//   nonzero AC coefficients spends at most 26 k bits on them, at most 11 bits on each of its <= floor((63 - k) / 16) ZRLs
//   and at most 4 on its EOB; turning a zero into a nonzero adds 26 bits and removes at most one ZRL and the EOB (15), so
//   the maximum is at k = 63: 22 + 63 * 26 = 1660 bits per block (OG_JE_BLOCK_BITS).
//   raw bytes <= ceil(blocks * 1660 / 8); stuffing at most doubles them; header 623, EOI 2.
// The kernel does not rely on that arithmetic for memory safety: every store into the raw stream and into the slot is
// bounds-checked, and an image that would not fit reports length -1.
#include "common.h"
#include <string.h>

#define OG_JE_HEADER 623
#define OG_JE_BLOCK_BITS 1660
#define OG_JE_THREADS 1024
// offsets inside the header (jcmarker.c's fixed layout for these settings)
#define OG_JE_QL 25
#define OG_JE_QC 94
#define OG_JE_DHT0 182      // bits[16] of the luma DC table; its symbols follow
#define OG_JE_DHT1 215      // luma AC
#define OG_JE_DHT2 398      // chroma DC
#define OG_JE_DHT3 431      // chroma AC

namespace {

__device__ __forceinline__ int je_byte_f32(float x) {
    float v = x + 1.0f;
    v = v / 2.0f;
    v = v * 255.0f;
    v = fminf(fmaxf(v, 0.0f), 255.0f);
    return (int)v;
}

template <bool F32>
__device__ __forceinline__ void je_rgb(const void* __restrict__ img, int H, int W, int y, int x, int& r, int& g, int& b) {
    if (F32) {
        const float* p = reinterpret_cast<const float*>(img) + (size_t)y * W + x;
        const size_t plane = (size_t)H * W;
        r = je_byte_f32(p[0]);
        g = je_byte_f32(p[plane]);
        b = je_byte_f32(p[2 * plane]);
    } else {
        const unsigned char* p = reinterpret_cast<const unsigned char*>(img) + ((size_t)y * W + x) * 3;
        r = p[0];
        g = p[1];
        b = p[2];
    }
}

__device__ __forceinline__ int je_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jfdctint.c over d[0], d[S], .. d[7 S]
template <int S, bool FIRST>
__device__ __forceinline__ void je_fdct8(int* d) {
    constexpr int N = FIRST ? 11 : 15;
    int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S];
    int t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
    int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S];
    int t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) << 2;
        d[4 * S] = (t10 - t11) << 2;
    } else {
        d[0] = je_descale(t10 + t11, 2);
        d[4 * S] = je_descale(t10 - t11, 2);
    }
    int z1 = (t12 + t13) * 4433;
    d[2 * S] = je_descale(z1 + t13 * 6270, N);
    d[6 * S] = je_descale(z1 - t12 * 15137, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446;
    t5 *= 16819;
    t6 *= 25172;
    t7 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7 * S] = je_descale(t4 + z1 + z3, N);
    d[5 * S] = je_descale(t5 + z2 + z4, N);
    d[3 * S] = je_descale(t6 + z2 + z3, N);
    d[S] = je_descale(t7 + z1 + z4, N);
}

__device__ const unsigned char je_zigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38,
    31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// images: image i at images + i * H * W * 3 elements; coef: image i at coef + i * nblocks * 64
template <bool F32>
__global__ __launch_bounds__(64) void jpeg_enc_transform_kernel(const void* __restrict__ images, int H, int W,
                                                                const unsigned char* __restrict__ header,
                                                                short* __restrict__ coef, int nblocks) {
    __shared__ unsigned short q8[2][64];            // 8 q, zigzag order, as the header holds it
    for (int i = threadIdx.x; i < 128; i += 64) q8[i >> 6][i & 63] = (unsigned short)(header[(i < 64 ? OG_JE_QL : OG_JE_QC - 64) + i] * 8);
    __syncthreads();
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nblocks) return;
    const int img = blockIdx.y;
    const void* src = F32 ? (const void*)(reinterpret_cast<const float*>(images) + (size_t)img * H * W * 3)
                          : (const void*)(reinterpret_cast<const unsigned char*>(images) + (size_t)img * H * W * 3);
    const int mcux = W >> 4;
    const int mcu = b / 6, j = b - mcu * 6;
    const int y0 = (mcu / mcux) * 16, x0 = (mcu % mcux) * 16;
    int d[64];
    if (j < 4) {
        const int yb = y0 + (j >> 1) * 8, xb = x0 + (j & 1) * 8;
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            int r, g, bl;
            je_rgb<F32>(src, H, W, yb + (i >> 3), xb + (i & 7), r, g, bl);
            d[i] = ((19595 * r + 38470 * g + 7471 * bl + 32768) >> 16) - 128;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            int sum = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int r, g, bl;
                je_rgb<F32>(src, H, W, y0 + 2 * (i >> 3) + (k >> 1), x0 + 2 * (i & 7) + (k & 1), r, g, bl);
                sum += j == 4 ? (-11059 * r - 21709 * g + 32768 * bl + (128 << 16) + 32767) >> 16
                              : (32768 * r - 27439 * g - 5329 * bl + (128 << 16) + 32767) >> 16;
            }
            d[i] = ((sum + 1 + (i & 1)) >> 2) - 128;       // bias 1, 2, 1, 2 .. along the output row (MCU starts are even)
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) je_fdct8<1, true>(d + 8 * r);
#pragma unroll
    for (int c = 0; c < 8; ++c) je_fdct8<8, false>(d + c);
    const unsigned short* q = q8[j < 4 ? 0 : 1];
    unsigned w[32];
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int c = d[je_zigzag[k]];
        const int qv = q[k];
        int m = ((c < 0 ? -c : c) + (qv >> 1)) / qv;
        m = c < 0 ? -m : m;
        if (k & 1) w[k >> 1] |= (unsigned)(m & 0xffff) << 16;
        else w[k >> 1] = (unsigned)(m & 0xffff);
    }
    uint4* o = reinterpret_cast<uint4*>(coef + ((size_t)img * nblocks + b) * 64);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// ---- entropy stage ----------------------------------------------------------------------------------------------
struct JeTables {
    unsigned dc[2][32];      // (size << 16) | code by category; entries no table defines stay 0
    unsigned ac[2][256];     // by (run << 4) | category
};

// exclusive scan of one unsigned per lane over the workgroup; total in `total`.  `red` >= 17 unsigned of LDS.
__device__ __forceinline__ unsigned je_exscan(unsigned v, unsigned* red, unsigned& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) red[wid] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned run = 0;
        for (int w = 0; w < OG_JE_THREADS / 64; ++w) {
            const unsigned t = red[w];
            red[w] = run;
            run += t;
        }
        red[16] = run;
    }
    __syncthreads();
    total = red[16];
    return red[wid] + inc - v;
}

struct JeCount {
    unsigned bits;
    __device__ __forceinline__ void put(unsigned, int n) { bits += n; }
};

struct JeWrite {
    unsigned* raw;
    unsigned cap;            // words the raw stream of this image holds
    unsigned long long acc;
    unsigned widx;
    int cnt;
    bool seam;               // the next word flushed is shared with the lane in front
    __device__ __forceinline__ void start(unsigned* r, unsigned cap_, unsigned bit_off) {
        raw = r;
        cap = cap_;
        acc = 0;
        widx = bit_off >> 5;
        cnt = bit_off & 31;
        seam = cnt != 0;
    }
    __device__ __forceinline__ void put(unsigned v, int n) {    // n <= 32 - cnt is not required: cnt < 32, n <= 32
        acc = (acc << n) | v;
        cnt += n;
        if (cnt >= 32) {
            const unsigned word = (unsigned)(acc >> (cnt - 32));
            if (widx < cap) {
                if (seam) atomicOr(raw + widx, word);
                else raw[widx] = word;
            }
            seam = false;
            ++widx;
            cnt -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (cnt > 0 && widx < cap) atomicOr(raw + widx, (unsigned)(acc << (32 - cnt)));
    }
};

// jchuff.c encode_one_block on the zigzag coefficients of one block
template <class Sink>
__device__ __forceinline__ void je_block(const short* __restrict__ c, int pred, const unsigned* dct, const unsigned* act,
                                         Sink& sink) {
    const uint4* p = reinterpret_cast<const uint4*>(c);
    int run = 0;
#pragma unroll 1
    for (int g = 0; g < 8; ++g) {
        const uint4 q = p[g];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int v = (int)(short)(w[e >> 1] >> ((e & 1) * 16));
            if (g == 0 && e == 0) {
                v -= pred;
                const int a = v < 0 ? -v : v;
                const int cat = 32 - __clz(a);
                const unsigned t = dct[cat & 31];
                sink.put(((t & 0xffff) << cat) | ((unsigned)(v - (v < 0)) & ((1u << cat) - 1)), (int)(t >> 16) + cat);
            } else if (v == 0) {
                ++run;
            } else {
                while (run > 15) {
                    const unsigned z = act[0xF0];
                    sink.put(z & 0xffff, (int)(z >> 16));
                    run -= 16;
                }
                const int a = v < 0 ? -v : v;
                const int cat = 32 - __clz(a);
                const unsigned t = act[((run << 4) | cat) & 255];
                sink.put(((t & 0xffff) << cat) | ((unsigned)(v - (v < 0)) & ((1u << cat) - 1)), (int)(t >> 16) + cat);
                run = 0;
            }
        }
    }
    if (run > 0) sink.put(act[0] & 0xffff, (int)(act[0] >> 16));
}

__device__ __forceinline__ int je_pred(const short* __restrict__ coef, int b) {
    const int mcu = b / 6, j = b - mcu * 6;
    if (j >= 1 && j <= 3) return coef[(size_t)(b - 1) * 64];
    if (mcu == 0) return 0;
    return coef[(size_t)(j == 0 ? b - 3 : b - 6) * 64];
}

// jpeg_make_c_derived_tbl from a DHT segment's bits[16] + its nsym symbols (never reads past them, whatever bits says)
__device__ void je_derive(const unsigned char* bits, unsigned* out, int mask, int nsym) {
    const unsigned char* vals = bits + 16;
    unsigned code = 0;
    int k = 0;
    for (int ln = 1; ln <= 16; ++ln) {
        for (int i = 0; i < bits[ln - 1] && k < nsym; ++i, ++k) out[vals[k] & mask] = ((unsigned)ln << 16) | (code++ & 0xffff);
        code <<= 1;
    }
}

__global__ __launch_bounds__(OG_JE_THREADS) void jpeg_enc_entropy_kernel(const short* __restrict__ coef_all, int nblocks,
                                                                         const unsigned char* __restrict__ header,
                                                                         unsigned* __restrict__ raw_all, unsigned raw_cap,
                                                                         unsigned char* __restrict__ out_all, long slot,
                                                                         int* __restrict__ lengths) {
    __shared__ unsigned char hdr[OG_JE_HEADER + 1];
    __shared__ JeTables tab;
    __shared__ unsigned red[17];
    const int img = blockIdx.x, tid = threadIdx.x;
    const short* coef = coef_all + (size_t)img * nblocks * 64;
    unsigned* raw = raw_all + (size_t)img * raw_cap;
    unsigned char* out = out_all + (size_t)img * slot;
    for (int i = tid; i < OG_JE_HEADER; i += OG_JE_THREADS) {
        const unsigned char h = header[i];
        hdr[i] = h;
        if (i < slot) out[i] = h;
    }
    for (int i = tid; i < (int)(sizeof(JeTables) / 4); i += OG_JE_THREADS) reinterpret_cast<unsigned*>(&tab)[i] = 0;
    __syncthreads();
    if (tid == 0) je_derive(hdr + OG_JE_DHT0, tab.dc[0], 31, 12);
    if (tid == 64) je_derive(hdr + OG_JE_DHT1, tab.ac[0], 255, 162);
    if (tid == 128) je_derive(hdr + OG_JE_DHT2, tab.dc[1], 31, 12);
    if (tid == 192) je_derive(hdr + OG_JE_DHT3, tab.ac[1], 255, 162);
    __syncthreads();

    // (1) bits of this lane's blocks, (2) scan, (3) write
    const int per = (nblocks + OG_JE_THREADS - 1) / OG_JE_THREADS;
    const int b0 = min(tid * per, nblocks), b1 = min(b0 + per, nblocks);
    JeCount cnt = {0};
    for (int b = b0; b < b1; ++b) {
        const int ch = (b % 6) >= 4;
        je_block(coef + (size_t)b * 64, je_pred(coef, b), tab.dc[ch], tab.ac[ch], cnt);
    }
    unsigned total_bits;
    const unsigned off = je_exscan(cnt.bits, red, total_bits);
    const unsigned raw_bytes = (total_bits + 7) >> 3;
    const unsigned raw_words = min((raw_bytes + 3) >> 2, raw_cap);
    for (unsigned i = tid; i < raw_words; i += OG_JE_THREADS) raw[i] = 0;
    __syncthreads();
    JeWrite wr;
    wr.start(raw, raw_cap, off);
    for (int b = b0; b < b1; ++b) {
        const int ch = (b % 6) >= 4;
        je_block(coef + (size_t)b * 64, je_pred(coef, b), tab.dc[ch], tab.ac[ch], wr);
    }
    wr.finish();
    if (tid == 0 && (total_bits & 7)) {                                  // pad the last byte with ones
        const unsigned pad = 8 - (total_bits & 7), w = total_bits >> 5;
        if (w < raw_cap) atomicOr(raw + w, ((1u << pad) - 1) << (32 - (total_bits & 31) - pad));
    }
    __syncthreads();

    // byte stuffing: count FF per run of words, scan, write
    const unsigned wper = (raw_words + OG_JE_THREADS - 1) / OG_JE_THREADS;
    const unsigned w0 = min(tid * wper, raw_words), w1 = min(w0 + wper, raw_words);
    unsigned nff = 0;
    for (unsigned w = w0; w < w1; ++w) {
        const unsigned v = raw[w];
#pragma unroll
        for (int k = 0; k < 4; ++k) nff += (4 * w + k < raw_bytes) && ((v >> (24 - 8 * k)) & 0xff) == 0xff;
    }
    unsigned total_ff;
    unsigned o = OG_JE_HEADER + 4 * w0 + je_exscan(nff, red, total_ff);
    const long fits = slot - 2;                                          // FF D9 stays behind the data
    for (unsigned w = w0; w < w1; ++w) {
        const unsigned v = raw[w];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned byte = (v >> (24 - 8 * k)) & 0xff;
            if (4 * w + k < raw_bytes) {
                if ((long)o < fits) out[o] = (unsigned char)byte;
                ++o;
                if (byte == 0xff) {
                    if ((long)o < fits) out[o] = 0;
                    ++o;
                }
            }
        }
    }
    if (tid == 0) {
        const long end = (long)OG_JE_HEADER + raw_bytes + total_ff;
        const bool ok = end <= fits && (size_t)raw_bytes <= (size_t)raw_cap * 4;
        if (ok) {
            out[end] = 0xff;
            out[end + 1] = 0xd9;
        }
        lengths[img] = ok ? (int)(end + 2) : -1;
    }
}

// ---- host: tables, header, plan --------------------------------------------------------------------------------
const unsigned char h_zigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27,
    20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46,
    53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.1
const unsigned char h_q_luma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103,
    121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const unsigned char h_q_chroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99,
    99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K.3: code counts per length, then the symbols
const unsigned char h_dc_luma_bits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const unsigned char h_dc_chroma_bits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const unsigned char h_dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char h_ac_luma_bits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
const unsigned char h_ac_luma_vals[162] = {1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8,
    35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55,
    56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116,
    117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162,
    163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200,
    201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243,
    244, 245, 246, 247, 248, 249, 250};
const unsigned char h_ac_chroma_bits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
const unsigned char h_ac_chroma_vals[162] = {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145,
    161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53,
    54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106,
    115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152,
    153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197,
    198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242,
    243, 244, 245, 246, 247, 248, 249, 250};

// 0: the device encodes it; else why not (ops.JpegEncodeRefused.REASONS)
int je_refusal(int n, int H, int W, int quality, int form) {
    if (n < 1) return 1;
    if (H < 16 || W < 16 || (H & 15) || (W & 15)) return 2;
    if (H > 4096 || W > 4096) return 3;                 // bit offsets and byte counts of one image stay well inside 32 bits
    if (quality < 1 || quality > 100) return 4;
    if (form != 0 && form != 1) return 5;
    return 0;
}

long je_blocks(int H, int W) { return (long)(H >> 4) * (W >> 4) * 6; }
long je_raw_words(int H, int W) { return (je_blocks(H, W) * OG_JE_BLOCK_BITS + 31) / 32 + 1; }

}  // namespace

extern "C" {

long objgan_jpeg_enc_header_bytes(void) { return OG_JE_HEADER; }

int objgan_jpeg_enc_header(int H, int W, int quality, unsigned char* out) {
    if (!out || je_refusal(1, H, W, quality, 0) != 0) return OG_BAD_ARGS;
    // jcparam.c jpeg_quality_scaling, jpeg_add_quant_table with force_baseline
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    unsigned char* p = out;
    static const unsigned char app0[20] = {0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    memcpy(p, app0, 20);
    p += 20;
    for (int t = 0; t < 2; ++t) {
        const unsigned char* base = t ? h_q_chroma : h_q_luma;
        *p++ = 0xff; *p++ = 0xdb; *p++ = 0; *p++ = 67; *p++ = (unsigned char)t;
        for (int k = 0; k < 64; ++k) {
            long v = ((long)base[h_zigzag[k]] * scale + 50) / 100;
            v = v < 1 ? 1 : (v > 255 ? 255 : v);
            *p++ = (unsigned char)v;
        }
    }
    const unsigned char sof[19] = {0xff, 0xc0, 0, 17, 8, (unsigned char)(H >> 8), (unsigned char)(H & 255), (unsigned char)(W >> 8),
                                   (unsigned char)(W & 255), 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1};
    memcpy(p, sof, 19);
    p += 19;
    struct { int id; const unsigned char* bits; const unsigned char* vals; int n; } dht[4] = {
        {0x00, h_dc_luma_bits, h_dc_vals, 12}, {0x10, h_ac_luma_bits, h_ac_luma_vals, 162},
        {0x01, h_dc_chroma_bits, h_dc_vals, 12}, {0x11, h_ac_chroma_bits, h_ac_chroma_vals, 162}};
    for (int t = 0; t < 4; ++t) {
        const int len = 19 + dht[t].n;
        *p++ = 0xff; *p++ = 0xc4; *p++ = (unsigned char)(len >> 8); *p++ = (unsigned char)(len & 255); *p++ = (unsigned char)dht[t].id;
        memcpy(p, dht[t].bits, 16);
        p += 16;
        memcpy(p, dht[t].vals, dht[t].n);
        p += dht[t].n;
    }
    static const unsigned char sos[14] = {0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    memcpy(p, sos, 14);
    p += 14;
    return (p - out) == OG_JE_HEADER ? OG_OK : OG_BAD_ARGS;
}

long objgan_jpeg_enc_plan(int n, int H, int W, int quality, int form, long* slot_bytes) {
    const int why = je_refusal(n, H, W, quality, form);
    if (why != 0) return -(long)why;
    const long raw_bytes = (je_blocks(H, W) * OG_JE_BLOCK_BITS + 7) / 8;
    if (slot_bytes) *slot_bytes = (OG_JE_HEADER + 2 * raw_bytes + 2 + 15) / 16 * 16;
    return (long)n * je_blocks(H, W) * 128 + (long)n * je_raw_words(H, W) * 4;
}

int objgan_jpeg_encode(const void* images, int form, int n, int H, int W, const unsigned char* header_dev, unsigned char* out,
                       long slot_bytes, int* lengths, void* ws, long ws_bytes, int stages, void* stream) {
    // a refusal touches neither the runtime nor a pointer
    long slot = 0;
    const long need = objgan_jpeg_enc_plan(n, H, W, 75, form, &slot);
    if (need <= 0 || !images || !header_dev || !out || !lengths || !ws || ws_bytes < need || slot_bytes < slot ||
        (stages & 3) == 0)
        return OG_BAD_ARGS;
    if ((reinterpret_cast<uintptr_t>(ws) & 15) != 0) return OG_BAD_ARGS;
    OG_ENTRY();
    hipStream_t s = (hipStream_t)stream;
    const int nblocks = (int)je_blocks(H, W);
    short* coef = reinterpret_cast<short*>(ws);
    unsigned* raw = reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(ws) + (size_t)n * nblocks * 128);
    if (stages & 1) {
        const dim3 grid(og_cdiv(nblocks, 64), n);
        if (form == 1)
            hipLaunchKernelGGL(jpeg_enc_transform_kernel<true>, grid, dim3(64), 0, s, images, H, W, header_dev, coef, nblocks);
        else
            hipLaunchKernelGGL(jpeg_enc_transform_kernel<false>, grid, dim3(64), 0, s, images, H, W, header_dev, coef, nblocks);
    }
    if (stages & 2)
        hipLaunchKernelGGL(jpeg_enc_entropy_kernel, dim3(n), dim3(OG_JE_THREADS), 0, s, coef, nblocks, header_dev, raw,
                           (unsigned)je_raw_words(H, W), out, slot_bytes, lengths);
    return og_launch_status();
}

}  // extern "C"

// What the host sides of conv_igemm*.hip share: development switches, profiler interface and categories, block-row
// planner, packed-bank descriptor, tile-height dispatch, weight-gradient plan, and the launchers that cross a file
// boundary (a kernel template is launched only from the file that defines it).
#pragma once
#include "conv_igemm3.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// ---- development switches (OG_KNOB: common.h -- constants in the shipped library; a development build caches the
// environment value once per translation unit that includes this header: harmless, all read the same environment)
OG_KNOB(og_igemm_v1, "OG_IGEMM_V1", 0)             // 1: first-generation kernels everywhere
OG_KNOB(og_igemm_tmmax_raw, "OG_IGEMM_TMMAX", 8)   // tallest forward / data-gradient tile
OG_KNOB(og_nothin, "OG_NO_THIN", 0)                // 1: no direct VALU kernels for thin outputs
OG_KNOB(og_trace, "OG_TRACE", 0)                   // 1: print every launch plan to stderr
OG_KNOB(og_wgrad3_maxtm, "OG_WGRAD3_MAXTM", 2)     // register-fragment weight-gradient form up to this tile height
OG_KNOB(og_wgrad_nob128, "OG_WGRAD_NOB128", 0)     // 1: dword gathers on wide stride-1 maps
OG_KNOB(og_split_target, "OG_SPLIT_TARGET", 1024)
OG_KNOB(og_no_xrows, "OG_NO_XROWS", 0)
OG_KNOB(og_nw8_min, "OG_NW8_MIN", 512)             // bf16x3: 8-wave workgroups from this many workgroups on (0: never)
OG_KNOB(og_ablate, "OG_ABLATE", 0)                 // development builds: IgemmArgs::ablate
OG_KNOB(og_kgroup_s1, "OG_KGROUP_S1", 4)           // chunks per K group (og_kstep), stride-1 multi-tap launches (0: tap-major)
OG_KNOB(og_kgroup_s2, "OG_KGROUP_S2", 0)           // ... stride-2 forward launches
OG_KNOB(og_kgroup_ph, "OG_KGROUP_PH", 4)           // ... the four-phase stride-2 data gradient / up-convolution
OG_KNOB(og_h2_nw8_tm, "OG_H2_NW8_TM", 4)           // fp16x2: 8-wave workgroups from this block-row height on
OG_KNOB(og_h2_pen_pct, "OG_H2_PEN_PCT", 100)        // fp16x2: re-read penalty of short block rows in og_row_plan, % of the table
OG_KNOB(og_x3_wgrad3_maxtm, "OG_X3_WGRAD3_MAXTM", 2)   // bf16x3: register-fragment weight gradient up to this tile height
OG_KNOB(og_rec_ng2_maxtm, "OG_REC_NG2_MAXTM", 3)    // fp16x2 on records: two pixel groups per wave up to this block-row height (0: never)
OG_KNOB(og_rec_ng2_min, "OG_REC_NG2_MIN", 1024)     // ... while the grid keeps this many workgroups (r5c_tileplans: 256 loses on 32x32 maps, 1024 >= 512)
OG_KNOB(og_rec_nw8_tm, "OG_REC_NW8_TM", 4)          // fp16x2 on records: 8-wave workgroups from this block-row height on
OG_KNOB(og_rec_tmmax, "OG_REC_TMMAX", 7)            // ... tallest block row
OG_KNOB(og_rec_ng2_nw8, "OG_REC_NG2_NW8", 0)        // ... 1: two pixel groups per wave also in 8-wave workgroups
OG_KNOB(og_wgrad_rec_tmmax, "OG_WGRAD_REC_TMMAX", 6)  // weight gradient on records: tallest block row (7: one wave per SIMD)
OG_KNOB(og_wgrad_rec_nw8, "OG_WGRAD_REC_NW8", 1)      // ... 8-wave workgroups for block rows <= 6 on >= 16384 pixels
static inline int og_igemm_tmmax() { const int v = og_igemm_tmmax_raw(); return (v < 1 || v > 8) ? 8 : v; }

// ---- optional per-launch timing (conv_igemm_prof.hip): when enabled, every conv launch is bracketed by hipEvents on
// its stream and tagged with a category and its ALGORITHMIC flops 2*M*K*Npix; prof_begin returns nullptr while off.
// meta: {kind (0 forward / data-gradient GEMM, 1 weight gradient, 2 thin VALU), tile height TM, rows M,
//        K channels C, taps T, images N, pixel-grid rows, pixel-grid columns, stride, grid.y splits}
struct ProfRec;
ProfRec* prof_begin(int cat, double flops, hipStream_t s);
void prof_meta(ProfRec* r, int kind, int tm, int M, int C, int T, int N, int ph, int pw, int stride, int splits);
void prof_end(ProfRec* r, hipStream_t s);

// Categories = kernel instances, so that they line up with the kernel names rocprofv3 reports (OG_PROF_CATS = 192):
//   0..6   conv_igemm3_kernel<1..7>            7..13  conv_wgrad2_kernel<1..7> (and conv_wgrad_bfb_kernel)
//   14 conv_thin_kernel / conv_thin_ph4_kernel   15 conv_thin3x3_kernel   16 conv_igemm_kernel (v1)   17 conv_wgrad_kernel (v1)
//   18 conv_igemm3_kernel<1, true> (LDS-free form for thin outputs)     19..25 conv_wgrad3_kernel<1..7>
//   26..32 conv_igemm3_kernel<1..7> in 8-wave workgroups                 33..39 conv_wgrad3_kernel<1..7> in 8-wave workgroups
//   + 48: their fp16x2 instances (math 4); + 96: on fp16 records (math 5); + 144: records, two pixel groups per wave
#define OG_PROF_CATS 192
enum OgFamily { OG_FAM_IGEMM3, OG_FAM_IGEMM3_DIRECT, OG_FAM_WGRAD2, OG_FAM_WGRAD3, OG_FAM_THIN, OG_FAM_THIN3,
                OG_FAM_IGEMM1, OG_FAM_WGRAD1 };
static inline int og_prof_cat(OgFamily fam, int tm = 0, int nw = 4, int math = 0, int ng = 1) {
    const int block = math == 5 ? (ng == 2 ? 144 : 96) : (math == 4 ? 48 : 0);
    switch (fam) {
        case OG_FAM_IGEMM3:        return block + (nw == 8 ? 25 + tm : tm - 1);
        case OG_FAM_IGEMM3_DIRECT: return block + 18;
        case OG_FAM_WGRAD2:        return 6 + tm;
        case OG_FAM_WGRAD3:        return block + (nw == 8 ? 32 + tm : 18 + tm);
        default:                   return 14 + (fam - OG_FAM_THIN);     // 14 thin, 15 thin3x3, 16 / 17 first generation
    }
}

// Tile-height dispatch: calls f(OgInt<tm>{}) with the run-time tile height as a compile-time constant; anything outside [LO, HI] ends at HI.
template <int LO, int HI, class F> static inline void og_with_tm(int tm, F&& f) {
    if constexpr (LO == HI) f(OgInt<LO>{});
    else if (tm == LO) f(OgInt<LO>{});
    else og_with_tm<LO + 1, HI>(tm, f);
}

// ---- block-row plan: M = `groups` 32-row groups over `tiles_n` column tiles run as block rows of height TM (<= 7:
// two workgroups per CU) plus one lower block row for the remainder in its own launch (388 rows = 13 groups -> 7 + 6,
// 194 -> 7, 768 -> 4 x 6), so that no block computes an empty row group.  The MFMA time of a launch is ~ (workgroups
// per CU) x TM: whole rounds while the grid is small, fractional once it spans many rounds; short tiles re-read the
// pixel operand more (pen).  The weight gradient always takes the tallest tiles (`tall`): its gather is the expensive part.
static inline double og_rounds(long blocks) {
    if (blocks <= 256) return 1.25;                 // one workgroup per CU: nothing to overlap with
    if (blocks < 1024) return (double)og_cdiv(blocks, 256);
    return (double)blocks / 256.0;
}
static inline void og_row_plan(int groups, int tiles_n, int tall, int* TM_out, int* full_rows_out, int* rest_out,
                               int pen_pct = 100, int tm_cap = 7) {
    int tmmax = og_igemm_tmmax();
    if (tmmax > 7) tmmax = 7;
    if (tmmax > tm_cap && tm_cap >= 1) tmmax = tm_cap;
    int bt = 1;
    if (tall) {
        const int brows = og_cdiv(groups, tmmax);
        bt = og_cdiv(groups, brows);
    } else {
        // TM = 1 re-reads the pixel operand once per 32 rows and runs against the L2 (~7 TB/s of
        // fills, 86 TFLOP/s at best -- profiles/r01_tm1_l2_bound.txt); TM = 3 reaches ~114, TM >= 4 ~120
        static const double pen[8] = {0, 1.40, 1.15, 1.06, 1.02, 1.0, 1.0, 1.0};
        double best = -1;
        for (int tm = 1; tm <= tmmax && tm <= groups; ++tm) {
            const int full = groups / tm, rest = groups - full * tm;
            const double pt = 1.0 + (pen[tm] - 1.0) * pen_pct / 100.0;
            const double pr = rest ? 1.0 + (pen[rest] - 1.0) * pen_pct / 100.0 : 0.0;
            double cost = og_rounds((long)full * tiles_n) * tm * pt
                        + (rest ? og_rounds(tiles_n) * rest * pr + 0.3 : 0.0);
            if (best < 0 || cost < best - 1e-9 || (cost < best + 1e-9 && tm > bt)) { best = cost; bt = tm; }
        }
    }
    *TM_out = bt; *full_rows_out = groups / bt; *rest_out = groups - (groups / bt) * bt;
}

// Row parts of the first-generation kernels: greedily 128-row tiles (cfg 0), one 64-row tile (1), 32-row tiles (2) for
// the ragged remainder (388 -> 384 + 4; 194 -> 128 + 64 + 32; 96 -> 64 + 32): padding waste stays below ~15 %.
struct RowPart { int m_begin, m_end, cfg; };
static inline int og_row_parts(int M, RowPart* parts) {
    int n = 0, m = 0;
    if (M >= 128) { parts[n++] = {0, (M / 128) * 128, 0}; m = (M / 128) * 128; }
    if (M - m >= 64) { parts[n++] = {m, m + 64, 1}; m += 64; }
    if (M - m > 0) { parts[n++] = {m, M, 2}; }
    return n;
}

// ---- packed filter banks (conv_igemm_pack.hip) -----------------------------------------------------------
// wt[(t*Cp + ck) * Mpad + cm] = src_tap[t] >= 0 ? w[...] : 0, zero padded to [T*Cp][Mpad].
// w is the PyTorch conv weight [Cout][Cin][Torig].  transpose = 0: cm = cout, ck = cin
// (forward);  transpose = 1: cm = cin, ck = cout (data gradient).
struct PackArgs {
    const float* w;
    float* wt;
    int Cout, Cin, Torig, Tg;
    int M, Mpad, Ck, Cp;
    int transpose;
    int m_major;         // 0: wt[K][Mpad] (v1 kernels), 1: wt[M][Kpad] (k contiguous, v2 kernel),
                         // 2: wt[Ck][Tg][Mpad] with Mpad = MT (thin direct kernel)
                         // 3: bf16 wt[M][Krow], Krow = Kpad rounded up to 32 (bf16 MFMA kernels)
                         // 4: bf16x3 split wt[M][Kpad/16][3][16]: every fp32 entry as its exact three-way bf16
                         //    split h + m + l (og_split8), the three pieces of a 16-deep K step back to back
                         // 5: fp16x2 split wt[M][Kpad/16][2][16] fp16: w * 2^10 = h + l
    int kgroup;          // row-major banks (m_major 1 / 3 / 4 / 5): chunks per K group (see og_kstep)
    const float* wmax;   // m_major 5: the OG_AMAX_SLOTS partial maxima of |w| (behind the bank, written by absmax_w_* before the pack)
    int wexp;            // m_major 5: scale exponent derived from them (set inside the pack kernels)
    signed char src_tap[OG_MAX_TAPS];
};

// Row pitch of a packed bank in elements: fp32 Kpad floats; bf16 Kpad rounded up to 32 (one iteration = 32 k);
// bf16x3 three bf16 per k (the h / m / l pieces of a 16-deep step back to back: 96 bytes).
static inline int og_krow(int Kpad, int math) {
    return math == 1 ? (Kpad + 31) / 32 * 32 : (math == 2 ? 3 * Kpad : (math >= 4 ? 2 * Kpad : Kpad));
}

// Chunks per K group (og_kstep) of a row-major bank / conv_igemm3_kernel launch: a function of what both the pack job
// and the launch know (channels, taps, source and pixel-grid heights).  The resident workgroups of an XCD cover ~8192
// output pixels; one 16-channel chunk of their source pixels is ~0.8 MB at stride 1 (3 MB at stride 2), and the groups
// are sized so that a group's taps find their lines in the 4 MB L2.
static inline int og_kgroup(int C, int Tg, int H, int PH) {
    const int spt = (C + 15) / 16;
    if (Tg <= 1) return spt;
    const int G = (H > PH + PH / 2) ? og_kgroup_s2() : og_kgroup_s1();
    return (G <= 0 || G > spt) ? spt : G;
}
static inline int og_kgroup_phases(int C) {
    const int spt = (C + 15) / 16, G = og_kgroup_ph();
    return (G <= 0 || G > spt) ? spt : G;
}

// accumulator count of the thin VALU kernels for M <= 32 output channels
static inline int og_thin_mt(int M) { return M <= 4 ? 4 : (M <= 12 ? 12 : (M <= 16 ? 16 : (M <= 24 ? 24 : 32))); }

// the four phase banks of objgan_conv_dgrad_s2_phases share one buffer of 4 * ceil(1.5 * M * Tg * Cp) + 1024 floats: the
// partial maxima of |w| sit behind the largest (bf16x3) bank size, whatever the arithmetic
static inline long og_phase_wmax_offset(int M, int Tg, int Cp) { return 4 * (((long)M * Tg * Cp * 3 + 1) / 2); }

// bf16 mode: floats the channel-blocked bf16 copy [N][Cp/16][H*W][16] of a source takes
static inline long og_nhwc_bf16_floats(int N, int H, int W, int Cp) { return ((long)N * H * W * Cp / 2 + 3) & ~3L; }

// conv_igemm_pack.hip
int og_fill_pack(PackArgs& p, const float* w, float* wt, int N, int C, int H, int W, int Cout, int Cin, int Torig,
                 int transpose, int Tg, const int* src_tap, int PH, int PW, int act, int math, int* MT_out);
void og_fill_pack_phase(PackArgs& p, const float* w, float* wt, int Cout, int Cin, int Torig, int Tg,
                        const int* src_tap_phase, int phase, int math);
void og_launch_pack(const PackArgs& p, long work_items, hipStream_t s);                    // pack_weights_kernel
void og_launch_absmax_w(const float* w, long n, float* out, hipStream_t s);                // absmax_w_kernel
void og_absmax_launch(const float* x, long n, float* out, hipStream_t s);                  // absmax_partials_kernel
void og_launch_nhwc_bf16(const float* x, float* out, int N, int C, int HW, int Cp, hipStream_t s);
void og_launch_f32_to_bf16(const float* x, float* out, long n4, hipStream_t s);
void og_launch_splitk_combine(const float* ws, int splits, long ws_stride, long seg_off, float* out, long total,
                              const float* bias, int M, int HW, int act, float* ymax, hipStream_t s);
// conv_igemm_thin.hip / conv_igemm_v1.hip: the launches objgan_conv_igemm and objgan_conv_wgrad hand on
int run_thin(IgemmArgs a, int MT, hipStream_t s);
int run_igemm(IgemmArgs a, hipStream_t s);
void og_launch_wgrad_v1(const WgradArgs& a, int cfg, dim3 grid, int ksize, hipStream_t s);
// conv_igemm_wgrad.hip: dw rows <- the split slots of one weight-gradient launch, summed in split order
int og_launch_wgrad_combine(const WgradArgs& a, int splits, hipStream_t s);
// conv_igemm_rec.hip: the instances of conv_igemm3_kernel that read pre-split fp16 records (math 5), the record forms
// of the weight gradient and the fp16 pair of dy they read
int og_launch_igemm3_rec(const IgemmArgs& a, int TM, int nw, int ng, dim3 grid, hipStream_t s);
int og_launch_wgrad_rec(const WgradArgs& a, int tm, int nw, dim3 grid, int ksize, int Cp, int dyp, hipStream_t s);
int og_launch_wgrad_rec2(const WgradArgs& a, int tm, dim3 grid, int ksize, int Cp, hipStream_t s);
void og_launch_h2_pair(const float* x, const float* xmax, float* out, long n, hipStream_t s);

// ---- weight-gradient plan (og_wgrad_plan, conv_igemm_wgrad.hip).  A part = one launch: rows [m_begin, m_end) of dy
// (+ xr_count extra rows on the VALU) against all columns, the pixel reduction cut into `splits` slices; splits > 1:
// every slice writes its tile into its own slot of `slot` floats from workspace offset ws_off, a combine sums them.
struct WgradPart {
    int tm, rows;                       // tile height in 32-row groups (v1: 0) and block rows
    int cfg;                            // v1 only: tile shape of og_row_parts
    int m_begin, m_end, xr_count;
    int nw, use3, b128;                 // v2: waves per workgroup, register-fragment form, 16-byte gathers
    int tiles_n, splits, pix_per_split;
    long slot, ws_off;
};
struct WgradPlan {
    int rc;                             // OG_OK, OG_BAD_ARGS (nothing else is valid then), or 2: nothing to do
    int kmath;                          // arithmetic of the kernels (WgradArgs::math)
    int v2, bfb, rec, rec2, dyp, h2, xrows, x_copy_in;
    int Cpb, xr_begin;
    long xb_floats, dyb_floats, dyp_floats;    // operand copies at the head of the workspace
    int nparts;
    WgradPart part[3];                  // at most two for v2, three for v1
    long total;                         // floats of workspace the run takes
};

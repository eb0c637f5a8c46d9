/*
 * objgan_hip.h -- C ABI of libobjgan_hip.so: the MI355X (gfx950) native kernels behind the
 * Obj-GAN image_generation G+D training step.
 *
 * This is the drop-in boundary of the hot path.  The reference's only native boundary is the
 * cffi module `models/roi_align/_ext/roi_align` (reference
 * image_generation/models/roi_align/src/roi_align.h:1-5, src/roi_align_cuda.h:1-5):
 *
 *     int roi_align_forward_cuda (int aligned_height, int aligned_width, float spatial_scale,
 *                                 THCudaTensor* features, THCudaTensor* rois, THCudaTensor* output);
 *     int roi_align_backward_cuda(int aligned_height, int aligned_width, float spatial_scale,
 *                                 THCudaTensor* top_grad, THCudaTensor* rois, THCudaTensor* bottom_grad);
 *
 * objgan_roi_align_forward / _backward replace exactly those two (same argument meaning; the
 * TH tensor handles become raw device pointers + sizes, the implicit THC "current stream"
 * becomes an explicit hipStream_t).  Everything else the reference step obtains from
 * cuDNN / cuBLAS / THC through PyTorch (conv, norms, attention bmm+softmax, masked max,
 * bilinear resize, Adam) is exported here with the same conventions so that the host side
 * (Python, ctypes) stays a thin binding.  This file is compiled into every kernel source (csrc/common.h includes it) and
 * read by the Python binding (objgan_hip/_lib.py derives its ctypes table from the declarations below), so a declaration
 * is written here and nowhere else: `int` or `long` result, parameters that are pointers or int / long / float / double.
 *
 * Conventions (identical to the reference FFI, roi_align_cuda.c:7-40):
 *   - the library never allocates, frees or retains memory; the caller owns every buffer,
 *     including scratch / workspace buffers named in the signatures;
 *   - all tensors are contiguous fp32, NCHW, device memory;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), re-entrant, reads no environment
 *     variable (development builds, -DOG_DEV, do) and keeps no global state -- with one opt-in exception: the
 *     measurement window of objgan_prof_enable / _collect / _dump (a host-side table of hipEvents, off by default,
 *     touched by the calling thread only);
 *   - return value: 1 = launched, 0 = argument error (the reference returns 0 when
 *     rois.size(1) != 5), < 0 = -(hipError_t) of a failed launch (the reference calls exit(-1)).
 */
#ifndef OBJGAN_HIP_H
#define OBJGAN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ROIAlign (reference models/roi_align/src/roi_align_kernel.cu:15-143) ------------------ */
/* features [B, C, H, W], rois [num_rois, roi_cols = 5] = (batch_idx, x1, y1, x2, y2),
 * output [num_rois, C, aligned_height, aligned_width].  Returns 0 if roi_cols != 5.
 * All three ROIAlign entry points refuse a map with height < 2 or width < 2 (as they refuse aligned_height < 2 or
 * aligned_width < 2), before any launch: the reference's kernels index row height - 2 / column width - 2
 * (hstart = min(floor(h), height - 2) = -1 for a valid sample) and read before the tensor there. */
int objgan_roi_align_forward(const float* features, const float* rois, float* output,
                             int num_rois, int roi_cols, int channels, int height, int width,
                             int aligned_height, int aligned_width, float spatial_scale,
                             void* stream);
/* bottom_grad [batch_size, C, H, W] must be zero-filled by the caller (it is accumulated with
 * atomics, exactly like the reference kernel). */
int objgan_roi_align_backward(const float* top_grad, const float* rois, float* bottom_grad,
                              int batch_size, int num_rois, int roi_cols, int channels,
                              int height, int width, int aligned_height, int aligned_width,
                              float spatial_scale, void* stream);

/* The same adjoint with a FIXED summation order (bit-reproducible): the taps of an image's ROI samples are sorted once
 * by anchor pixel (stable) into a table in `ws`, and every (pixel, channel) gathers its taps in a fixed order.  The
 * reference's kernel (and objgan_roi_align_backward) leaves the order of its atomicAdds unspecified.  ws: at least
 * objgan_roi_align_backward_ws_floats(...) floats; shapes the query returns 0 for (more than 512 rois, maps over
 * ~5K pixels) and ws == NULL take objgan_roi_align_backward's path. */
long objgan_roi_align_backward_ws_floats(int batch_size, int num_rois, int channels, int height, int width,
                                         int aligned_height, int aligned_width);
int objgan_roi_align_backward_ordered(const float* top_grad, const float* rois, float* bottom_grad,
                                      int batch_size, int num_rois, int roi_cols, int channels,
                                      int height, int width, int aligned_height, int aligned_width,
                                      float spatial_scale, float* ws, long ws_floats, void* stream);
/* avg_pool2d(kernel_size=2, stride=1) tail of RoIAlignAvg (modules/roi_align.py:26-29). */
int objgan_avgpool2s1_forward(const float* in, float* out, long planes, int ih, int iw, void* stream);
int objgan_avgpool2s1_backward(const float* grad_out, float* grad_in, long planes, int ih, int iw,
                               void* stream);

/* ---- implicit-GEMM convolution on MFMA (reference model.py conv stacks, via cuDNN) ---------- */
long objgan_conv_packed_floats(int M, int C, int T);
/* layout of the packed bank objgan_conv_igemm uses for these arguments -- low byte: layout class (0..5), bits 8..:
 * channel chunks per K group of the row-major classes 1 / 3 / 4 / 5 -- : part of the key of any caller-side bank cache
 * (the same filter is served by different kernels and K orders at different sizes) */
int objgan_conv_bank_layout(int N, int C, int H, int W, int M, int Tg, int PH, int PW, int act, int math);
/* y[n,m,a*osh+ooh,b*osw+oow] = act(bias[m] + sum_{c,t} Wp[m][c*Tg+t] * x[n,c,a*s+dh[t],b*s+dw[t]])
 * for (a,b) in PH x PW.  w: [Cout][Cin][Torig]; transpose=0 -> m=cout,c=cin; 1 -> m=cin,c=cout.
 * src_tap[t]: which of the Torig taps GEMM tap t uses (-1 = zero).  1 <= Tg <= 32.
 * upsample=1: taps address a nearest-x2 upsampled view of x; pad_mode 0 zeros, 1 reflect.
 * act: 0 none, 1 LeakyReLU(0.2), 2 tanh, 3 sigmoid, 4 ReLU.  wt: scratch of
 * objgan_conv_packed_floats(M, C, Tg) floats.  y_prezeroed=1 tells the library that y already
 * holds zeros (lets partial-coverage launches, i.e. stride-2 dgrad phases, use split-K).
 * wt_packed=1: wt still holds the packed bank written by an earlier call with the same w, taps,
 * transpose flag, math and input size class (the caller caches it while w is unchanged); 0: pack now.
 * math: 0 = fp32 MFMA (exact fp32 fmaf chains); 1 = mixed precision (BASELINE config 5): operands rounded
 * to bf16 (RNE), fp32 accumulation, fp32 tensors at the boundary -- the call first writes a bf16 channel-blocked copy
 * [N][ceil16(C)/16][H][W][16] of x into ws and the matrix kernel reads its pixel operand from that copy as 16-byte vectors
 * (without ws: channel-strided fp32 gathers converted in registers, same values); 2 = "bf16x3": fp32 results on
 * the bf16 matrix pipe -- every fp32 operand is split exactly into three bf16 pieces (24 = 8 + 8 + 8 significand
 * bits) and the six largest of the nine partial products are accumulated in fp32; what is dropped is below 2^-24
 * of a product.  Outputs with <= 32 channels always run on the fp32 VALU kernels. */
int objgan_conv_igemm(const float* x, const float* w, const float* bias, float* y, float* wt,
                      int N, int C, int H, int W, int upsample, int pad_mode,
                      int Cout, int Cin, int Torig, int transpose,
                      int Tg, const int* dh, const int* dw, const int* src_tap,
                      int PH, int PW, int stride,
                      int OHf, int OWf, int osh, int osw, int ooh, int oow,
                      int act, int y_prezeroed, int wt_packed, int math, float* ring, const float* xmax, float* ymax,
                      float* ws, long ws_floats, void* stream);
/* math: 0 fp32 operands on the fp32 MFMA; 1 operands rounded to bf16; 2 "bf16x3" (fp32 operands split exactly three ways
 * on the bf16 MFMA, six products); 4 "fp16x2" (fp32 operands as two fp16 pieces of x * 2^s on the fp16 MFMA, three
 * products: residual <= 2^-23 |x| for every element within 2^-10 of its tensor's maximum, 2^-39 of that maximum below;
 * the filter bank's scale comes from partial maxima the pack path leaves behind the bank).  xmax: math 4 only -- the 1024
 * partial maxima of |x| (the kernel derives 2^s from them), written by objgan_absmax_partials or by the producer of x
 * itself (objgan_norm_forward / objgan_norm_backward / objgan_act_backward `amax`, this call's `ymax`); NULL otherwise.
 * ymax (may be NULL): 1024 ZERO-FILLED floats that receive the partial maxima of |y| -- from the kernel's epilogue where the
 * launch writes final values, from a pass over y otherwise. */
int objgan_absmax_partials(const float* x, long n, float* out1024, void* stream);
/* math 5: the arithmetic of math 4 with the pixel operand handed over as its PRE-SPLIT fp16 record instead of the fp32
 * tensor: `x` points to rec[n][c / 16][h | l][pixel][c % 16] fp16 with x * 2^s = h + l (channels C..ceil16(C)-1 zero), s
 * derived from the same `xmax` slots the call is given (they still undo the scale in the epilogue).  The kernel reads two
 * 16-byte loads per lane and K step instead of eight channel-strided dwords + the split on the VALU, and short block rows run
 * two 32-pixel groups per wave; results are bit-identical to math 4.  Only where objgan_conv_bank_layout answers class 5
 * (the MFMA implicit-GEMM kernel); the filter bank is the math-4 bank.  objgan_h2_records writes a record in one pass
 * (4 B read + 4 B written per element); objgan_h2_records_floats: its size in 4-byte units (= N * ceil16(C) * HW). */
long objgan_h2_records_floats(int N, int C, long HW);
int objgan_h2_records(const float* x, const float* xmax1024, void* rec, int N, int C, long HW, void* stream);
/* ws: the bf16 channel-blocked copy of x (math 1), then the split-K workspace.  Small-grid / long-K launches are split along K: every split stores its partial output into
 * its own slot of ws and a second kernel sums the slots in split order (+ bias, activation) -- bit-reproducible, no
 * zero-fill of y, no atomics.  objgan_conv_igemm_ws_floats (host-only, same geometry arguments; ring != 0 when a ring
 * buffer is passed) says how many floats a call needs (math 0 / 2: 0 for most); a call that needs them and gets fewer returns 0. */
long objgan_conv_igemm_ws_floats(int N, int C, int H, int W, int upsample, int pad_mode,
                                 int Cout, int Cin, int Torig, int transpose, int Tg,
                                 int PH, int PW, int stride, int OHf, int OWf, int osh, int osw,
                                 int act, int y_prezeroed, int math, int ring);
/* The launch plan objgan_conv_igemm follows for the same arguments (host-only, launches nothing; for tests and tools):
 * out[0..10] <- {bank layout class, kernel math, nw (waves per workgroup), ng (pixel groups per wave), TM (32-row groups
 * per block row of the main launch), full_rows (its block rows), rest (height of the second launch's one block row, 0:
 * none), tiles_n (pixel tiles), splits (K), full_cover, direct (1: a block row of height 1 runs the LDS-free instance)}.
 * Classes 0 and 2 have no such plan: the fields behind the class are 0.  Returns 0 where the call would refuse. */
int objgan_conv_igemm_plan(int N, int C, int H, int W, int upsample, int pad_mode,
                           int Cout, int Cin, int Torig, int transpose, int Tg,
                           int PH, int PW, int stride, int OHf, int OWf, int osh, int osw,
                           int act, int y_prezeroed, int math, int ring, int* out);
/* ring (may be NULL): data gradient of a ReflectionPad2d(1) convolution without the padded intermediate -- the
 * GEMM runs over the padded pixel grid (PH = OHf + 2, PW = OWf + 2, y is the UNPADDED gradient), interior
 * pixels are stored into y, the one-pixel border into ring [N*M][2*PW + 2*PH]; objgan_reflect_ring_fold then
 * adds the border back at its mirror positions.  Only for calls whose objgan_conv_bank_layout class (low byte) is
 * 1, 3, 4 or 5. */
int objgan_reflect_ring_fold(const float* ring, float* y, long planes, int H, int W, void* stream);
/* Data gradient of a stride-2 convolution whose four output parity phases have the same number
 * of taps (k=4, pad 1, even sizes): one launch for all phases.  x = dY [N,Cout,OH,OW],
 * y = dX [N,Cin,2*PH,2*PW], fully written (no pre-zeroing).  dh/dw/src_tap: 4 x Tg entries, phase
 * p = (row parity << 1) | column parity.  wt: 4*ceil(1.5*Cin*Tg*ceil16(Cout)) + 1024 floats (four phase banks,
 * then the partial maxima of |w| the fp16x2 pack leaves for its scale); wt_packed as above.
 * ws: objgan_conv_dgrad_s2_phases_ws_floats floats (math 1: the bf16 channel-blocked copy of dY, see objgan_conv_igemm; else 0). */
long objgan_conv_dgrad_s2_phases_ws_floats(int N, int Cout, int OH, int OW, int math);
/* the plan of its one four-phase launch, fields as objgan_conv_igemm_plan (host-only) */
int objgan_conv_dgrad_s2_phases_plan(int N, int Cout, int OH, int OW, int Cin, int Tg, int PH, int PW, int math, int* out);
/* Data gradient of a 4x4 / stride-2 / pad-1 convolution w.r.t. an input of Cin <= 32 channels (the first convolution of the
 * shape / object discriminators, reference model.py:1119-1128, 1217-1220), all four output parity phases in ONE launch of the
 * fp32 VALU kernel: dy [N, Cout, OH, OW] is read twice (the per-phase form read it four times), dx [N, Cin, 2 OH, 2 OW] is fully
 * written.  wt: objgan_conv_dgrad_s2_thin_floats(Cout, Cin) floats, packed by the call unless wt_packed;
 * objgan_conv_pack_job_thin_phase: the pack job of one of its four phase banks for objgan_conv_pack_jobs_run. */
long objgan_conv_dgrad_s2_thin_floats(int Cout, int Cin);
int objgan_conv_pack_job_thin_phase(void* job, const float* w, float* wt, int Cout, int Cin, int phase);
int objgan_conv_dgrad_s2_thin(const float* dy, const float* w, float* dx, float* wt, int N, int Cout, int OH, int OW,
                              int Cin, int wt_packed, void* stream);
int objgan_conv_dgrad_s2_phases(const float* x, const float* w, float* y, float* wt,
                                int N, int Cout, int OH, int OW, int Cin, int Torig,
                                int Tg, const int* dh, const int* dw, const int* src_tap,
                                int PH, int PW, int wt_packed, int math, const float* xmax, float* ws, long ws_floats,
                                void* stream);
/* dw[co][ci][kh][kw] = (accumulate ? dw : 0) + sum dy * x; ksize in {1,3,4}.  The reduction over pixels is split
 * across workgroups; the partial tiles go through ws (objgan_conv_wgrad_ws_floats floats, host-only query) and are
 * summed in split order: the weight gradient is bit-reproducible and dw needs no zero-fill.  math 1: the workspace also
 * holds the bf16 copies the kernel reads (x channel-blocked as in objgan_conv_igemm, dy in its own layout); without a
 * workspace the call gathers the fp32 tensors and rounds them in registers (same values). */
long objgan_conv_wgrad_ws_floats(int N, int Cin, int H, int W, int upsample, int pad_mode,
                                 int Cout, int OH, int OW, int ksize, int stride, int pad, int math);
/* The launch plan objgan_conv_wgrad follows for the same arguments (host-only, launches nothing; for tests and tools):
 * out[0..9] <- {rc (1: a plan follows), kmath, v2, bfb, rec, rec2, dyp, h2, xrows, nparts}, then for each of three parts
 * (one launch each; unused parts 0) {tm, rows, cfg, m_begin, m_end, xr_count, nw, use3, b128, tiles_n, splits}: 43 ints. */
int objgan_conv_wgrad_plan(int N, int Cin, int H, int W, int upsample, int pad_mode,
                           int Cout, int OH, int OW, int ksize, int stride, int pad, int math, int* out);
int objgan_conv_wgrad(const float* x, const float* dy, float* dw,
                      int N, int Cin, int H, int W, int upsample, int pad_mode,
                      int Cout, int OH, int OW, int ksize, int stride, int pad, int math,
                      int accumulate, const float* xmax, const float* dymax, float* ws, long ws_floats, void* stream);
/* (math 4: xmax / dymax = objgan_absmax_partials of x / dy; launches planned on the LDS-staged or first-generation
 * kernels run bf16x3 instead -- both are fp32-result arithmetics) */
/* math 5: `x` is the fp16 RECORD of the source (objgan_h2_records under xmax; dy stays the fp32 tensor): the lanes read
 * half records and transpose them through LDS (ds_read_b64_tr_b16) instead of gathering 32 (channel, tap) planes per
 * wave from the fp32 tensor and splitting on the VALU.  Same products per 16-pixel step as math 4 (fp32 results; the
 * pixel splits differ, so the two are equal up to summation order).  Only where objgan_conv_wgrad_rec_ok says so
 * (OH * OW % 32 == 0, OH, OW <= 256, (H - 1) * W < 65535).
 * math 6 (round 6): as 5, and dy is ALSO read pre-split -- its fp16 pair (plane h, plane l, same layout) is written into
 * the workspace by one pass and the K loop carries no operand split; bit-identical to math 5.  math 7 (round 6): as 5 with
 * two (tap, 32-channel) column groups per wave and block rows of at most 128 rows (launches of fewer than 16 384 pixels
 * take math 5's kernel).  Both measured no faster in the training step (profiles/r06_ab_variants.txt): kept for the
 * record, not used by the Python layer's default. */
int objgan_conv_wgrad_rec_ok(int N, int Cin, int H, int W, int Cout, int OH, int OW, int ksize);
/* bf16 mode (math 1, BASELINE config 5) with the operand copy made ONCE per tensor (round 6).  math 1 writes a bf16
 * channel-blocked copy [N][Cp/16][HW][16] of its pixel operand into the call's workspace on every call: the forward
 * convolution and the weight gradient of a layer each copy the same x, every branch of an Inception block copies its shared
 * input (32.9 ms of 216 per B = 32 step were such copies).  objgan_nhwc_bf16 makes that copy on its own
 * (objgan_nhwc_bf16_floats floats; 0 = too large, stay on math 1), and math 3 is math 1 with `x` pointing to it:
 * objgan_conv_igemm(..., math = 3) where objgan_conv_bank_layout(..., math = 1) answers class 3, objgan_conv_wgrad(...,
 * math = 3) where objgan_conv_wgrad_bfb_ok says so (dy is still copied per call).  Same values, same kernels: bit-identical
 * to math 1. */
long objgan_nhwc_bf16_floats(int N, int C, long HW);
int objgan_nhwc_bf16(const float* x, float* out, int N, int C, long HW, void* stream);
int objgan_conv_wgrad_bfb_ok(int N, int Cin, int H, int W, int Cout, int OH, int OW, int ksize);

/* ---- frozen text encoder (reference model.py:85-179 RNN_ENCODER: Embedding + bidirectional LSTM on
 * a packed sequence).  table [ntoken][I]; captions [B][L] int64; lens [B] int32; wt_ih [2][I][4H] and
 * wt_hh [2][H][4H] are the transposed weight_ih_l0(_reverse) / weight_hh_l0(_reverse); b_* [2][4H]
 * (gate order i, f, g, o).  out [B][2H][Lout] = words_emb (zero past each length), hn [B][2H] = sent_emb. */
int objgan_lstm_bidir_forward(const float* table, const long* captions, const int* lens,
                              const float* wt_ih, const float* wt_hh, const float* b_ih, const float* b_hh,
                              float* out, float* hn, int B, int L, int Lout, int I, int H, int ntoken,
                              void* stream);
/* the same pass, also returning the final cell state cn [B][2H] (layout of hn) */
int objgan_lstm_bidir_forward_state(const float* table, const long* captions, const int* lens,
                                    const float* wt_ih, const float* wt_hh, const float* b_ih, const float* b_hh,
                                    float* out, float* hn, float* cn, int B, int L, int Lout, int I, int H,
                                    int ntoken, void* stream);

/* ---- trainable text encoder (csrc/lstm_train.hip; DAMSM pretraining).  Same tensors and limits as the frozen pass.
 * keep (nullable) [B][L][I] uint8 is the embedding dropout's keep-mask and scale = 1 / (1 - p): the embedded word is
 * multiplied by keep * scale before the gate sums.  With keep = NULL, out and hn are bit for bit those of
 * objgan_lstm_bidir_forward.  ws: objgan_lstm_bidir_train_ws_floats(B, L, I, H) floats (host-only query), sections in
 * this order: gates [B][2][L][4H] (activated i, f, g, o), cell [B][2][L][H], hidden [B][2][L][H], x [B][L][I] (the
 * words after dropout) -- written by the forward pass -- then dgate [B][2][L][4H] (gate pre-activation deltas) and
 * dx [B][L][I], written by the backward pass of the same step; all zero at positions past a caption's length.
 * backward: d_out [B][2H][Lout] and d_hn [B][2H] (either may be NULL: zero); w_ih [2][4H][I] and w_hh [2][4H][H] are
 *     the UNTRANSPOSED weight_ih_l0(_reverse) / weight_hh_l0(_reverse).  Gradients in the same layouts: d_w_ih
 *     [2][4H][I], d_w_hh [2][4H][H], d_b_ih == d_b_hh [2][4H], d_table [ntoken][I] (rows of tokens not in the batch are
 *     zero).  Every element is written; no float atomics, bit-reproducible. */
long objgan_lstm_bidir_train_ws_floats(int B, int L, int I, int H);
int objgan_lstm_bidir_train_forward(const float* table, const long* captions, const int* lens,
                                    const unsigned char* keep, float scale,
                                    const float* wt_ih, const float* wt_hh, const float* b_ih, const float* b_hh,
                                    float* out, float* hn, float* ws, long ws_floats,
                                    int B, int L, int Lout, int I, int H, int ntoken, void* stream);
int objgan_lstm_bidir_backward(const float* d_out, const float* d_hn, const long* captions, const int* lens,
                               const unsigned char* keep, float scale, const float* w_ih, const float* w_hh,
                               float* ws, long ws_floats, float* d_w_ih, float* d_w_hh, float* d_b_ih, float* d_b_hh,
                               float* d_table, int B, int L, int Lout, int I, int H, int ntoken, void* stream);

/* ---- box generator, sampling path (reference box_generation DecoderRNN.forward_step, is_training=0): one launch
 * decodes B captions from the encoder's (h_n, c_n) to label / box sequences of <= T steps.  h0, c0 [B][H];
 * noise [B][T][6] doubles (uniform, normal, normal for the xy draw, then for the wh draw).  l_emb [L][H]; xy_w, wh_w,
 * nxy_w [A][2] with biases [A]; wt_ih [2A+H][4H], wt_hh [H][4H], lo_wt [H][L], xyo_wt [H+L][6K], who_wt [H+L+A][6K] are
 * transposed nn weights.  Limits: 4H <= 1024, L <= 256, K <= 8, T <= 32, A <= 64, cpw in {1, 2, 4, 8} with the
 * tile's state within 64 KiB of LDS.  labels [B][T] int32, lengths [B] int32, samples [B][T][4] doubles (x, y, w, h),
 * trace (nullable) [B][T][L + 12K]; entries past a caption's length are zero. */
int objgan_box_decode_default_cpw(void);
int objgan_box_decode(const float* h0, const float* c0, const double* noise,
                      const float* l_emb, const float* xy_w, const float* xy_b, const float* wh_w, const float* wh_b,
                      const float* nxy_w, const float* nxy_b, const float* wt_ih, const float* wt_hh,
                      const float* b_ih, const float* b_hh, const float* lo_wt, const float* lo_b,
                      const float* xyo_wt, const float* xyo_b, const float* who_wt, const float* who_b,
                      float x0, float y0, float w0, float r0,
                      int* labels, int* lengths, double* samples, float* trace,
                      int B, int T, int H, int L, int K, int A, int sos, int eos, int cpw, void* stream);

/* ---- box generator, training step (csrc/box_train.hip; reference DecoderRNN.forward with is_training=1, loss.py
 * Perplexity / BBLoss, the trainer's backward and clip).  The 17 weight tensors and their layout are those of
 * objgan_box_decode.  labels [B][T+1] int32 and boxes [B][T+1][4] (x, y, w, r; the <sos> column first) are the
 * targets, lens [B] int32 the decode steps of each caption (<= T).  Limits: 4H <= 1024, L <= 256, K <= 8, T <= 256,
 * A <= 64, cpw in {1, 2, 4, 8} with the tile's state within 64 KiB of LDS.  ws: objgan_box_train_ws_floats floats,
 * written by the forward pass and read and extended by the backward pass of the same step.
 * forward: trace [B][T][L + 12K] in objgan_box_decode's layout, zero past each length; a caption's rows do not depend
 *     on cpw, its place, B or T.
 * loss: sums = 4B + 1 doubles (per caption: label term, box term, non-pad steps, arg-max matches; then sum_b n_b);
 *     dtrace = d[(lamda1 sum label + lamda2 sum box) / sum n] / d(trace).
 * backward: grads = HOST array of the 17 device pointers (kernel layout), every element written, bit-reproducible.
 * clip: out[0] = max(1, (norm + 1e-6) / max_norm), out[1] = the L2 norm of the n floats at g; partials >= 256 doubles.
 *     objgan_adam_step_gated(flag = out, grad_scale < 0) then applies clip_grad_norm_ and Adam without a host read. */
long objgan_box_train_ws_floats(int B, int T, int H, int L, int K, int A);
int objgan_box_train_forward(const float* h0, const float* c0, const int* labels, const float* boxes, const int* lens,
                             const float* l_emb, const float* xy_w, const float* xy_b, const float* wh_w,
                             const float* wh_b, const float* nxy_w, const float* nxy_b, const float* wt_ih,
                             const float* wt_hh, const float* b_ih, const float* b_hh, const float* lo_wt,
                             const float* lo_b, const float* xyo_wt, const float* xyo_b, const float* who_wt,
                             const float* who_b, float x0, float y0, float w0, float r0, float* trace, float* ws,
                             long ws_floats, int B, int T, int H, int L, int K, int A, int cpw, void* stream);
int objgan_box_train_loss(const float* trace, const int* labels, const float* boxes, const int* lens,
                          const float* weight, float lamda1, float lamda2, double* sums, float* dtrace,
                          int B, int T, int L, int K, int pad, void* stream);
int objgan_box_train_backward(const float* dtrace, const float* trace, const float* c0, const int* labels,
                              const int* lens, const float* wt_ih, const float* wt_hh, const float* lo_wt,
                              const float* xyo_wt, const float* who_wt, float* const* grads, float* ws, long ws_floats,
                              int B, int T, int H, int L, int K, int A, int cpw, void* stream);
int objgan_box_train_clip(const float* g, long n, float max_norm, double* partials, float* out, void* stream);

/* ---- normalisation + GLU / LeakyReLU / residual (BatchNorm train mode, InstanceNorm) -------- */
/* `sums` (forward) / `bsums` (backward): statistics workspace of objgan_norm_ws_floats(N, C, HW, per_channel) floats
 * (host-only query): every workgroup of the statistics launch stores its partial pair into its own slot, a second
 * one-thread-per-group kernel (norm_partials_sum_kernel) adds the slots in slot order -- bit-reproducible statistics, no
 * fp32 atomics, nothing to pre-zero; the totals are the first 2G floats. */
long objgan_norm_ws_floats(int N, int C, int HW, int per_channel);
int objgan_norm_forward(const float* x, float* y, const float* residual,
                        const float* gamma, const float* beta,
                        float* running_mean, float* running_var,
                        float* sums, float* mean, float* rstd,
                        int N, int C, int HW, int per_channel, int mode,
                        float eps, float momentum, float* amax, void* stream);
/* amax (may be NULL; only where objgan_norm_amax_supported is non-zero -- 2: the caller passes the slots ZERO-FILLED): the 1024 partial maxima of |y| (forward) / |dx|
 * (backward), filled inside the call's own launches -- the scale input of an fp16x2 convolution that reads the tensor
 * next, instead of a separate pass over it (objgan_absmax_partials). */
int objgan_norm_amax_supported(int N, int C, int HW, int per_channel, int affine);
/* apply with given statistics (eval-mode BatchNorm: mean = running_mean, rstd = 1/sqrt(running_var+eps)) */
int objgan_norm_apply(const float* x, float* y, const float* residual, const float* gamma, const float* beta,
                      const float* mean, const float* rstd, int N, int C, int HW, int per_channel, int mode,
                      void* stream);
int objgan_norm_backward(const float* x, const float* dy, const float* mean, const float* rstd,
                         const float* gamma, const float* beta, float* bsums,
                         float* dx, float* dgamma, float* dbeta,
                         int N, int C, int HW, int per_channel, int mode, float* amax, void* stream);
int objgan_act_backward(const float* dy, const float* y, float* dz, long total, int kind, float* amax, void* stream);
/* out[c] = sum over (n, i) of x[n, c, i] (bias gradients); ws: objgan_channel_sum_ws_floats floats (ordered combine) */
long objgan_channel_sum_ws_floats(int N, int C, int HW);
int objgan_channel_sum(const float* x, float* out, int N, int C, int HW, float* ws, void* stream);

/* ---- attention (reference GlobalAttention.py:32-181, miscc/utils.py:401-413) ---------------- */
int objgan_attn_general_forward(const float* x, const float* src, const unsigned char* mask,
                                float* wc, float* attn, int B, int idf, int Q, int L, void* stream);
/* dsrc is fully written (no zero-fill): every wave stores its partial tile into ws
 * (objgan_attn_general_backward_ws_floats floats, host-only query) and a second kernel sums the waves in order */
long objgan_attn_general_backward_ws_floats(int B, int idf, int Q, int L);
int objgan_attn_general_backward(const float* x, const float* src, const float* attn,
                                 const float* dwc, const float* dattn, float* dx, float* dsrc,
                                 int B, int idf, int Q, int L, float* ws, void* stream);
int objgan_attn_bu_forward(const float* tgt, const float* ctx1, const float* src,
                           const unsigned char* mask, float* wc, float* attn,
                           int B, int d2, int idf, int R, int L, int normalize, float eps,
                           void* stream);
int objgan_attn_bu_backward(const float* dwc, const float* attn, float* dsrc,
                            int B, int idf, int R, int L, void* stream);
int objgan_masked_max_forward(const float* f, const float* m, float* out, int B, int num, int R,
                              int P, long m_stride_b, long m_stride_r, long m_stride_c, void* stream);
/* df is fully written (no zero-fill); ws: objgan_masked_max_backward_ws_floats floats (ordered two-level sum) */
long objgan_masked_max_backward_ws_floats(int B, int num, int R, int P);
int objgan_masked_max_backward(const float* f, const float* m, const float* dout, float* df,
                               int B, int num, int R, int P, long m_stride_b, long m_stride_r,
                               long m_stride_c, float* ws, void* stream);
int objgan_softmax_strided_forward(const float* x, float* y, long outer, int dim, long inner,
                                   float scale, const int* lens, int nlens,
                                   const unsigned char* rowvalid, void* stream);
int objgan_softmax_strided_backward(const float* y, const float* dy, float* dx, long outer, int dim,
                                    long inner, float scale, void* stream);

/* ---- resize, gradient folds, optimiser ------------------------------------------------------ */
int objgan_bilinear_forward(const float* x, float* y, long planes, int ih, int iw, int oh, int ow,
                            void* stream);
int objgan_bilinear_backward(const float* dy, float* dx, long planes, int ih, int iw, int oh, int ow,
                             void* stream);
int objgan_sum2x2(const float* dy, float* dx, long planes, int h, int w, void* stream);
int objgan_reflect_fold(const float* dxp, float* dx, long planes, int h, int w, void* stream);
/* nn.BCELoss()(p, constant target t) on the small probability maps of the discriminator heads (reference
 * miscc/losses.py:182-204 and every other adversarial term): mean over n elements -> out[0]; log clamped at
 * -100 and gradient (p - t) / max(p (1 - p), 1e-12) like torch.  g: the upstream scalar gradient (device). */
int objgan_bce_const_forward(const float* p, float* out, int n, float t, void* stream);
int objgan_bce_const_backward(const float* p, const float* g, float* dp, int n, float t, void* stream);
/* Batched re-packing of cached filter banks.  A job is an opaque blob (objgan_conv_pack_job_bytes() bytes) that
 * says "pack w into wt exactly as objgan_conv_igemm -- or phase `phase` of objgan_conv_dgrad_s2_phases --
 * does for these arguments"; a caller that keeps packed banks (wt_packed = 1) stores the blobs of a network
 * back to back in device memory and refreshes all of them with ONE launch after an optimizer step (the
 * per-use re-pack was 499 launches per training step).  Replaces nothing in the reference: cuDNN transforms
 * filters internally. */
int objgan_conv_pack_job_bytes();
int objgan_conv_pack_job(void* job, const float* w, float* wt, int N, int C, int H, int W, int Cout, int Cin,
                         int Torig, int transpose, int Tg, const int* src_tap, int PH, int PW, int act, int math);
int objgan_conv_pack_job_phase(void* job, const float* w, float* wt, int Cout, int Cin, int Torig, int Tg,
                               const int* src_tap_phase, int phase, int math);
int objgan_conv_pack_jobs_run(const void* jobs_dev, int njobs, void* stream);
/* Batched small matrix product C[b] = A[b] . B[b] with arbitrary element strides (transposes are free): the
 * per-image region-context products of the DAMSM word loss (reference GlobalAttention.py:62-68 inside the
 * caption loop of losses.py:87-127: B torch.bmm calls) in one launch, likewise both of its gradients. */
int objgan_bmm_strided(const float* A, const float* B, float* C, int batch, int M, int N, int K,
                       long sab, long sam, long sak, long sbb, long sbk, long sbn,
                       long scb, long scm, long scn, void* stream);
/* Layout-map stem of the object discriminators without the 512x512 lift (reference
 * image_generation/model.py:1217-1226: shp_code(F.interpolate(seg, 512, bilinear, align_corners))).  The channel
 * contraction runs at low resolution (a 1x1 convolution C -> 9*Mo through objgan_conv_igemm); these two entry
 * points apply the separable per-axis operator "shift by the tap offset o reflect-pad o bilinear lift" to its
 * result, forward and adjoint.  z [N, 9*Mo, h, w] (channel (dh*3+dw)*Mo + co), y / dy [N, Mo, SH, SW],
 * scratch N*3*Mo*h*SW floats.  Tables live in device memory and are built by the caller:
 *   forward  [3][S] per axis: source indices i0, i1 and the weight l1 of i1 (l0 = 1 - l1), per tap offset;
 *   backward CSR transposes: off [3][len+1], idx, wt. */
int objgan_lift_taps_forward(const float* z, const float* bias, float* y, float* scratch, int N, int Mo, int h,
                             int w, int SH, int SW, const int* ci0, const int* ci1, const float* cl1,
                             const int* ri0, const int* ri1, const float* rl1, void* stream);
int objgan_lift_taps_backward(const float* dy, float* dz, float* scratch, int N, int Mo, int h, int w, int SH,
                              int SW, const int* roff, const int* ridx, const float* rwt, const int* coff,
                              const int* cidx, const float* cwt, void* stream);
/* Pooling layers of the frozen Inception-v3 encoder (reference image_generation/model.py:203-287:
 * F.max_pool2d(k3, s2), F.avg_pool2d(k3, s1, p1), F.avg_pool2d(k8)); planes = N*C NCHW planes.
 * mode 0 = max (no padding; idx receives the plane-local arg-max of every output for the backward pass,
 * first maximum in row-major order like torch), 1 = average with divisor k*k (count_include_pad). */
int objgan_pool2d_forward(const float* x, float* y, int* idx, long planes, int H, int W, int OH, int OW,
                          int k, int s, int p, int mode, void* stream);
int objgan_pool2d_backward(const float* dy, const int* idx, float* dx, long planes, int H, int W, int OH,
                           int OW, int k, int s, int p, int mode, void* stream);
/* torch.optim.Adam update over flat arenas; the gradient is pre-multiplied by grad_scale
 * (1/world_size under data parallelism: the RCCL all-reduce is a plain sum).  Hyper-parameters are
 * doubles like torch's python floats: 1 - beta and lr / (1 - beta1^t) are evaluated in double. */
int objgan_adam_step(float* p, const float* g, float* m, float* v, long n, double lr, double beta1,
                     double beta2, double eps, int step, float grad_scale, void* stream);
/* The same update, taken only when the DEVICE flag flag[0] > 0, with the step counter on the device
 * (state: 3 doubles {steps, beta1^steps, beta2^steps}, initialised {0, 1, 1}; coef: 3 floats scratch).
 * Replaces the host-side `if float(errObjSSD) > 0:` of reference image_generation/trainer.py:429,440
 * under data parallelism: the flag rides behind the gradient arena through the all-reduce, so every
 * rank takes or skips the same update without a device->host read.  grad_scale < 0: the gradient is divided by
 * flag[0] -- after the all-reduce the number of ranks that contributed one -- instead of a fixed 1 / world size. */
int objgan_adam_step_gated(float* p, const float* g, float* m, float* v, long n, double lr, double beta1,
                           double beta2, double eps, double* state, const float* flag, float* coef,
                           float grad_scale, void* stream);
int objgan_ema_update(float* avg, const float* p, long n, float decay, float one_minus_decay,
                      void* stream);

/* ---- training images on the device (the loader side of the path) -------------------------
 * Replaces, per batch, the host-side `transforms.Resize((s, s))(img)` + ToTensor + Normalize(0.5, 0.5) of
 * reference image_generation/miscc/load.py:141-150 (Pillow's antialiased bilinear Image.resize, once per
 * branch size and image): the decoded 8-bit RGB images of a batch arrive back to back in one byte buffer
 * (rows of W*3 bytes; image b at byte offs[b], hs[b] x ws[b] pixels; offs / hs / ws are DEVICE arrays) and
 * out [B, 3, S, S] is bit for bit what Pillow + torch compute on the host.  Hmax >= every height,
 * kmax >= objgan_resize_pil_kmax(largest side of the batch, S) (the tap count Pillow allots per pixel).
 * coef_scratch: B*2*S*(kmax+2) ints, tmp_scratch: B*Hmax*S*3 bytes. */
int objgan_resize_pil_kmax(int max_in, int S);
int objgan_resize_pil_rgb8(const unsigned char* src, const long* offs, const int* hs, const int* ws, int B,
                           int Hmax, int kmax, int S, int* coef_scratch, unsigned char* tmp_scratch, float* out,
                           void* stream);

/* ---- training images: baseline JPEG decode on the device ------------------------------
 * Replaces the host decode `Image.open(BytesIO(img_bytes)).convert('RGB')` of reference
 * image_generation/miscc/load.py:141-151 (get_imgs; Pillow = libjpeg-turbo with the library defaults: JDCT_ISLOW, fancy
 * upsampling, RGB output): the FILE bytes cross PCIe, the decoded image never exists on the host.  Bit for bit Pillow's
 * output (integer arithmetic throughout: jdhuff.c entropy decode, jidctint.c inverse DCT, jdsample.c triangle-filter
 * upsampling, jdcolor.c fixed-point colour conversion).
 *
 * objgan_jpeg_parse     HOST ONLY.  Markers, quantisation and Huffman tables of one file -> a descriptor of
 *                       objgan_jpeg_desc_bytes() bytes whose first ten ints are {width, height, components, hmax, vmax,
 *                       MCUs per row, MCU rows, restart interval, reason, scan offset}.  Returns 1 for a file the device
 *                       decodes (baseline / sequential Huffman, 8 bit, one interleaved scan, grey or YCbCr 4:4:4 / 4:2:2 /
 *                       4:2:0) and 0 with reason != 0 for anything else (1 not JPEG, 2 progressive / arithmetic / lossless,
 *                       3 precision, 4 components, 5 sampling, 6 scan, 7 tables, 8 truncated, 9 RGB-coded): the caller routes that file
 *                       to its host decoder knowingly.
 * objgan_jpeg_plan      HOST ONLY.  Lays a batch out: descs[i] gets its file's byte offset in the batch buffer
 *                       (file_offsets[i], multiples of 16), its output byte offset, its workspace slices and the slice of
 *                       the entropy index handed in (nsegs[i] entries; NULL / 0: none).
 *                       -> workspace bytes (0: a refused descriptor in the batch).
 * objgan_jpeg_decode    files: the batch's files back to back (device, buffer padded to 16 bytes); descs_host: the planned
 *                       descriptors (launch geometry), descs_dev: a device copy of the same bytes (what the kernels read);
 *                       out: image i as [height][width][3] RGB bytes at its output offset; ws: objgan_jpeg_plan's byte
 *                       count.  The Huffman scan of a file is serial: a file without index is walked by ONE lane, which
 *                       writes its state at every MCU-row start to index_out (objgan_jpeg_seg_bytes() bytes per MCU row,
 *                       image i at the sum of the MCU rows of the images before it; NULL: not wanted); handed back in
 *                       as index_in (NULL: none) the same file is decoded by one lane per MCU row -- a training set is
 *                       decoded once per epoch, so the index of the first epoch serves all later ones. */
long objgan_jpeg_desc_bytes(void);
long objgan_jpeg_seg_bytes(void);
int objgan_jpeg_parse(const unsigned char* file, long nbytes, void* desc_out);
long objgan_jpeg_plan(void* descs, int n, const long* file_offsets, const long* out_offsets, const int* nsegs);
int objgan_jpeg_decode(const unsigned char* files, const void* descs_host, const void* descs_dev, int n,
                       unsigned char* out, void* ws, long ws_bytes, const void* index_in, void* index_out, void* stream);

/* ---- generated images: baseline JPEG encode on the device (csrc/jpeg_enc.hip) -------------------------------------
 * Replaces the per-image host loop of reference image_generation/evaluator.py:225-233 (save_singleimages: four fp32
 * elementwise ops, .byte(), .cpu(), Image.fromarray(...).save('<key>_<sent>.jpg')): a batch of n RGB images of one size,
 * H and W multiples of 16, -> the files Pillow's default save writes (JFIF 1.1, YCbCr 4:2:0, the Annex-K Huffman tables,
 * one interleaved scan), BYTE FOR BYTE; integer arithmetic throughout (jccolor.c, jcsample.c h2v2, jfdctint.c, jcdctmgr.c,
 * jchuff.c).  Nothing is encoded approximately: what the device does not encode is refused before any launch.
 *
 * objgan_jpeg_enc_header  HOST ONLY.  The objgan_jpeg_enc_header_bytes() = 623 bytes in front of the entropy-coded data
 *                         for (H, W, quality 1..100: jpeg_quality_scaling, force_baseline).  The kernels read the
 *                         quantisation and Huffman tables from a device copy of it.
 * objgan_jpeg_enc_plan    HOST ONLY.  -> workspace bytes, *slot_bytes = bytes per image in the output buffer (the worst
 *                         case the code tables allow; derivation in the source); or -reason for what is refused: 1 empty
 *                         batch, 2 H or W no multiple of 16, 3 a side over 4096, 4 quality outside 1..100, 5 form.
 * objgan_jpeg_encode      images: form 0 uint8 [n][H][W][3], form 1 fp32 [n][3][H][W] in [-1, 1] (bytes as the host loop
 *                         makes them: add 1, div 2, mul 255, clamp, truncate, one fp32 rounding each).  out: image i's file
 *                         at out + i * slot_bytes, lengths[i] its byte count (-1: it did not fit its slot -- cannot happen
 *                         with the plan's slot size, and is bounds-checked all the same).  stages: 1 transform
 *                         (-> int16 zigzag coefficients in ws), 2 entropy coding, 3 both.  Asynchronous on `stream`. */
long objgan_jpeg_enc_header_bytes(void);
int objgan_jpeg_enc_header(int H, int W, int quality, unsigned char* out);
long objgan_jpeg_enc_plan(int n, int H, int W, int quality, int form, long* slot_bytes);
int objgan_jpeg_encode(const void* images, int form, int n, int H, int W, const unsigned char* header_dev, unsigned char* out,
                       long slot_bytes, int* lengths, void* ws, long ws_bytes, int stages, void* stream);

/* ---- per-box instance masks on the device (the loader side of the path) --------------------
 * Replaces the four `skimage.transform.resize(mask, [s, s])` calls per box of reference
 * image_generation/miscc/load.py:160-176 (s = 32, 64, 128, 256 from the 64 x 64 instance mask): `count` square
 * float64 masks src[count][n][n] (n <= 64) -> out[k][count][sizes[k]][sizes[k]] float64 for nsizes <= 4 sizes (out: HOST
 * array of device pointers).  skimage's defaults as scipy.ndimage evaluates them (Gaussian anti-aliasing when
 * shrinking, order-1 zoom, mode 'mirror', grid_mode, clip to the input range), in float64 and in scipy's operation
 * order: bit for bit scipy's results.  taps[k * 17 ..]: the ntaps[k] = 2 radius + 1 <= 17 normalised weights of the
 * anti-aliasing filter of size k (host array; ntaps[k] = 0 when sizes[k] >= n). */
int objgan_mask_resize(const double* src, int count, int n, int nsizes, const int* sizes, double* const* out,
                       const int* ntaps, const double* taps, void* stream);

/* ---- instance masks from COCO polygons (csrc/coco_masks.hip) ------------------------------------------------
 * The mask step of the reference's annotation preprocessing (image_generation/miscc/load.py:608-622,
 * shape_generation/datasets.py:347-361): per instance `COCO.segToMask(rings, H, W)` (skimage.draw.polygon per ring,
 * OR-ed) -> astype(float) -> skimage.transform.resize(mask, [S, S]).  One call takes a batch of A instances of
 * different image sizes and returns out[A][S][S] float64, bit for bit what obj-gan_amd/miscc/coco_prep.py computes on
 * the host with numpy + scipy.ndimage (even-odd crossing rule of skimage's point_in_polygon in float64 at integer pixel
 * coordinates; per-axis Gaussian, axis 0 then axis 1, mode mirror; order-1 zoom with grid_mode, mode mirror; clip to
 * the rasterised mask's own minimum and maximum).  The full-size mask exists only as a bit plane in the workspace, and
 * the filter is evaluated only at the <= 2 S rows and columns the zoom reads.
 *   verts      [nverts][2] float64 (x, y), already clipped by the caller; ring r is verts[ring_off[r] .. ring_off[r + 1])
 *   ring_off   [nrings + 1], inst_ring [A + 1]: instance a owns rings inst_ring[a] .. inst_ring[a + 1] (none: empty mask)
 *   hs, ws     [A] image height and width, 1 .. Hmax / Wmax
 *   taps       float64 table of normalised Gaussian weights (computed by the caller as scipy computes them);
 *   tap_off    [A][2][2] = per instance and axis {first index in taps, count}; count = 2 radius + 1, or 0: no filter on
 *              that axis (it does not shrink)
 * All arrays are device memory.  An instance whose table entries contradict the scalar arguments is answered with NaN.
 * objgan_poly_masks_covers  HOST ONLY.  1 when the kernels cover an instance of this size: S <= 64, sides <= 1024, tap
 *                           counts <= 65 (radius 32; COCO's 640 -> 64 has radius 18).  What is not covered is refused
 *                           by objgan_poly_masks (returns 0) and is left to the caller's host route.
 * objgan_poly_masks_plan    HOST ONLY.  -> workspace bytes for a batch (0: refused). */
int objgan_poly_masks_covers(int H, int W, int S, int ntaps0, int ntaps1);
long objgan_poly_masks_plan(int A, int Hmax, int Wmax);
int objgan_poly_masks(const double* verts, long nverts, const int* ring_off, const int* inst_ring, int nrings,
                      const int* hs, const int* ws, int A, int Hmax, int Wmax, int S, const double* taps,
                      const int* tap_off, int ntaps_total, double* out, void* ws_buf, long ws_bytes, void* stream);

/* ---- evaluation statistics on the device (csrc/eval_stats.hip) -------------------------------------------
 * objgan_bilinear_halfpixel_forward  the input preparation of the FID feature network (reference
 *     image_generation/model.py:433-441): y[N, C, OH, OW] = F.interpolate(x, (OH, OW), 'bilinear',
 *     align_corners=False) -- source index max(0, (dst + 0.5) * in / out - 0.5), upper neighbour clamped to in - 1, no
 *     antialiasing -- then y = y * scale[c] + shift[c] when the two C-float device tables are given (both or neither).
 * objgan_moments_accumulate  x fp32 [rows, D]: sum[D] += sum_r x[r], outer[D, D] += sum_r x[r]^T x[r] in fp64; only the
 *     upper triangle of outer (diagonal included) is read and written.  One thread owns each output element and adds
 *     the rows in row order (no atomics): bit-reproducible, and independent of how a row sequence is cut into calls.
 *     The caller zeroes sum / outer once.  A call streams the whole accumulator: hand over several batches at a time.
 * objgan_moments_finalize  mu[D] = sum / n, sigma[D, D] = (outer - n mu mu^T) / (n - 1) (np.cov's normalisation),
 *     mirrored to the full, exactly symmetric matrix; n >= 2 rows were accumulated. */
int objgan_bilinear_halfpixel_forward(const float* x, float* y, int N, int C, int H, int W, int OH, int OW,
                                      const float* scale, const float* shift, void* stream);
int objgan_moments_accumulate(const float* x, int rows, int D, double* sum, double* outer, void* stream);
int objgan_moments_finalize(const double* sum, const double* outer, long n, int D, double* mu, double* sigma,
                            void* stream);

/* ---- caption / attention snapshot grids on the device (csrc/snapshot.hip) ---------------------------------
 * The grid of reference image_generation/miscc/utils.py:59-182 (build_super_images; per_panel_norm = 1: :184-306,
 * build_super_shape_images) for the first nvis images of a batch: per image font_max rows of caption strip, one line
 * [lr image | 2-px pad | panel 0 | pad | ... | panel max_word_num | pad] and one line [image | pad | merged 0 | ...].
 * imgs [>= nvis, 3, H, W] and lr_imgs [>= nvis, 3, LH, LW] (NULL: the image itself) in [-1, 1], resized to vis x vis with
 * half-pixel bilinear sampling, (x + 1) / 2 * 255 in three fp32 roundings, truncated.  attn [>= nvis, T, a, a], T <= 1023:
 * panel 0 is the maximum over the T maps, panels 1..T the maps, panels past T zeros; only the first max_word_num + 1 are
 * drawn, all take part in the image's minimum / maximum.  counts (device, nvis ints, may be NULL): image n has only
 * counts[n] <= T maps (the per-caption maps of the DAMSM word loss), the slots behind them are ignored.  M (device, fp64 [vis, a]; needs vis / a >= 2): a map expands
 * to M A M^T in fp64 -- skimage's pyramid_expand(sigma = 20) as scipy.ndimage evaluates it, see csrc/snapshot.hip; M NULL
 * (needs vis == a): the maps are drawn as they are and normalised in fp32, the reference's dtype on that path.  Normalisation
 * (v - min) / (max - min) * 255, truncated: min(1, .) / max(0, .) over all panels of the image, or per panel and skipped
 * where max == min (per_panel_norm).  max == min in the global form (the reference's 0 / 0, an undefined cast): the panel
 * is 0.  Merged panels: Pillow's paste(att, mask = L 210) over the image byte; objgan_snapshot_blend_table (HOST ONLY)
 * writes that blend for all 256 x 256 (image byte, attention byte) pairs.  strip: uint8 [nvis * font_max, Wg, 3],
 * out: uint8 [nvis * (font_max + 2 vis), Wg, 3], Wg = (max_word_num + 2) * (vis + 2); every byte of out is written.
 * ws: objgan_snapshot_ws_doubles doubles (HOST ONLY query; 0 = arguments out of range).  Statistics are combined in a
 * fixed order without atomics: the grid is bit-reproducible.
 * per_panel_norm also selects the shape stage's two forms (reference shape_generation/miscc/utils.py:59-300), both only
 * with M NULL (fp32 arithmetic on maps of the panel's size; with M the call returns 0):
 *   2  raw (build_super_images2): byte = trunc(v * 255) in fp32, no minimum or maximum.  Masks are in [0, 1]; outside
 *      that range the reference's cast is undefined, here the byte saturates to 0 / 255.
 *   3  per panel, unguarded (the shape stage's build_super_images): (v - min) / (max - min) * 255 per panel; a panel with
 *      max == min (the reference's 0 / 0 -- every empty box slot) is 0, where mode 1 draws it as it is.
 * Any other value returns 0.
 * objgan_mask_to_rgb8: the mask dump of reference shape_generation/trainer.py:389-397.  masks: fp32 planes of HW pixels;
 * sel (device, N ints, may be NULL: planes 0 .. N - 1): the planes to draw, in any order, repeats allowed -- the caller
 * vouches that each lies inside `masks`; out: uint8 [N][HW][3].  Per plane byte = trunc((v - min) / (max - min) * 255)
 * in three separately rounded fp32 operations (denormals kept), replicated to the three channels; max == min (the
 * reference's NaN cast): zeros.  One workgroup per plane, fixed-order reduction in LDS, no atomics: bit-reproducible.
 * 16-byte loads when HW % 4 == 0, masks is 16-byte and out 4-byte aligned; scalar accesses otherwise. */
long objgan_snapshot_ws_doubles(int nvis, int T, int a, int vis);
int objgan_snapshot_blend_table(unsigned char* table65536);
int objgan_snapshot_grid(const float* imgs, const float* lr_imgs, const float* attn, const int* counts, const double* M,
                         const unsigned char* strip, unsigned char* out, double* ws, long ws_doubles,
                         int nvis, int T, int a, int vis, int H, int W, int LH, int LW,
                         int max_word_num, int font_max, int per_panel_norm, void* stream);
int objgan_mask_to_rgb8(const float* masks, const int* sel, unsigned char* out, int N, int HW, void* stream);

/* ---- shape generator training (csrc/convlstm.hip; reference shape_generation/model.py:81-128, miscc/losses.py,
 * datasets.py:99-111).  The ConvLSTM recurrence is split: the input part of the gate convolution runs once over all
 * B R maps of a direction, only the hidden part stays in the loop; these entries are the point-wise rest of a step.
 * Ch hidden channels, HW pixels per map; gate order in, remember, out, cell.  16-byte accesses when HW and the strides
 * are multiples of four floats and the pointers are 16-byte aligned, scalar accesses otherwise; no float atomics.
 * cell_forward: gx = the input-part gates of this step, image b at gx + b gx_bstride ([4 Ch][HW]); gh [B][4 Ch][HW] the
 *     hidden-part convolution (NULL at t = 0); c_prev [B][Ch][HW] (NULL: zero).  Writes h twice -- h_out [B][Ch][HW]
 *     (the next step's convolution input) and image b's slot of the state slab at h_slab + b slab_bstride --, c_out
 *     [B][Ch][HW] and acts [B][5 Ch][HW]: the four activated gates, then tanh(c).
 * cell_backward: dh = dh_slab[b dh_bstride] (+ dh_rec [B][Ch][HW], NULL at the last step); dc_in (NULL: zero); writes
 *     the pre-activation gate gradients to dg_slab + b dg_bstride ([4 Ch][HW], the slot of the batch-major slab the
 *     input-part gradients are taken from in one launch) and to dg_out [B][4 Ch][HW], and dc_out = dc f.
 *     c_prev NULL (t = 0): the remember gate's gradient is zero.
 * box_max: y[b][i] = max over r of x[b][r][i], i < CSS; arg (uint8, may be NULL in the forward) the FIRST maximal r,
 *     which is where the backward puts dy; every element of dx is written.  R <= 255.
 * boxmaps_onehot: raw [B][NB][SS] per-box maps, cat [B][NB] category of each slot, num [B] boxes per image ->
 *     fwd, bwd [B][R][C][SS]: fwd[b][r][cat[b][r]] = raw[b][r] for r < num[b]; bwd[b][r] = fwd's slot NB - 1 - r (the
 *     sequence reversed over all NB slots, then cut to R <= NB). */
int objgan_convlstm_cell_forward(const float* gx, const float* gh, const float* c_prev, float* h_out, float* h_slab,
                                 float* c_out, float* acts, int B, int Ch, int HW, long gx_bstride, long slab_bstride,
                                 void* stream);
int objgan_convlstm_cell_backward(const float* dh_slab, const float* dh_rec, const float* dc_in, const float* acts,
                                  const float* c_prev, float* dg_slab, float* dg_out, float* dc_out, int B, int Ch, int HW,
                                  long dh_bstride, long dg_bstride, void* stream);
int objgan_box_max_forward(const float* x, float* y, unsigned char* arg, int B, int R, long CSS, void* stream);
int objgan_box_max_backward(const float* dy, const unsigned char* arg, float* dx, int B, int R, long CSS, void* stream);
int objgan_boxmaps_onehot(const float* raw, const int* cat, const int* num, float* fwd, float* bwd, int B, int NB, int R,
                          int C, int SS, void* stream);

/* ---- layout stage (csrc/layout.hip): decoder samples -> box tables and box maps, the file route of
 * seq2seq/evaluator (postprocess, write_layouts) and miscc/load.py (load_gen_insanns, get_gen_rois) without the files.
 * labels [B][T], lengths [B], samples [B][T][4]: the outputs of objgan_box_decode.  mean_std [8] doubles: (mean, std) of
 * x, y, w, r.  label_to_cat [L]: decoder label -> category id (-1: none); cat_to_rel [ncat]: category id -> row of
 * categories.txt (-1: unknown); thresholds [B][L]: count caps per caption and label.  All of these in device memory.
 * boxes [B][T][5] doubles (x, y, w, h, category id; zero past nbox[b]) and nbox [B]: bit for bit Evaluator.postprocess.
 * rois [NB][B][R][6], fm_rois [B][R][6] doubles, num_rois [B], cats [B][R] (relative category; 0 in unused slots),
 * maps [B][R][S][S] and fmaps [B][R][F][F] floats (1 inside a box's rectangle): what load_gen_insanns builds from the
 * '%.2f' rows of those boxes.  sizes: HOST array of the NB <= 4 branch sides, S = sizes[0]; min_size: boxes with both
 * sides below it are dropped; R <= 64.  bounds: scratch, 8 B R ints.  Two launches, no atomics, no host read.
 * tie_rule: the order np.argsort gives EQUAL areas when more than R boxes are left -- 0: insertion sort (numpy's generic
 * code up to 16 values; after the reversal the later box comes first), 1: numpy's AVX-512 network for 64-bit keys; other
 * values return 0.  T > 17 returns 0: past 16 boxes neither rule describes numpy's argsort. */
int objgan_layout_from_decode(const int* labels, const int* lengths, const double* samples, const double* mean_std,
                              const int* label_to_cat, const int* cat_to_rel, const int* thresholds,
                              double* boxes, int* nbox, double* rois, double* fm_rois, int* num_rois, int* cats,
                              float* maps, float* fmaps, int* bounds, const int* sizes, int NB, int F, int R,
                              int min_size, int tie_rule, int B, int T, int L, int ncat, void* stream);

/* ---- perceptual term of the shape generator's loss (csrc/perceptual.hip) -------------------------
 * pcp_stem_forward: y[N][3][OH][OW] = (bilinear_align_corners(x[N][1][S][S]) - mean_c) / std_c with the ImageNet
 *     constants mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225); S == 1 and OH / OW == 1 are scale 0.
 * pcp_stem_backward: dx[N][1][S][S], gather form, every element written once.
 * l1_tap_forward: out[slot] = (1 / n) sum |f[i] - r[i]|, fp64 partial sums combined in workgroup order (no atomics);
 *     ws: objgan_l1_tap_ws_doubles(n) doubles.
 * l1_tap_backward: g[i] = mask(f[i]) (gdown[i] + coef[0] sign(f[i] - r[i])), sign(0) = 0; gdown NULL: zero;
 *     relu_mask != 0: mask = f > 0, else 1; coef: ONE float in device memory; amax (may be NULL): the 1024 partial
 *     maxima of |g| as objgan_act_backward leaves them. */
int objgan_pcp_stem_forward(const float* x, float* y, int N, int S, int OH, int OW, void* stream);
int objgan_pcp_stem_backward(const float* dy, float* dx, int N, int S, int OH, int OW, void* stream);
long objgan_l1_tap_ws_doubles(long n);
int objgan_l1_tap_forward(const float* f, const float* r, long n, float* out, int slot, double* ws, void* stream);
int objgan_l1_tap_backward(const float* f, const float* r, const float* gdown, const float* coef, float* g, long n,
                           int relu_mask, float* amax, void* stream);

/* ---- measurement aid (bench.py roofline leg): hipEvent-bracketed conv launches ------------------ */
int objgan_prof_enable(int on);
int objgan_prof_collect(double* ms, double* flops, long* count);   /* arrays of 192 categories (48..95: fp16x2 instances; 96..191: fp16x2 on records, one / two pixel groups) */
/* per-launch records of the current window (call before objgan_prof_collect, which resets it):
 * meta[10*i..] = {kind 0 GEMM / 1 weight gradient / 2 thin, tile height, rows, K channels, taps, images,
 * pixel-grid rows, pixel-grid columns, stride (negative: strided output phases), K splits} */
int objgan_prof_dump(float* ms, double* flops, int* meta, int max_records, int* n_out);

#ifdef __cplusplus
}
#endif
#endif /* OBJGAN_HIP_H */

/* bdetr.h - C ABI of the MI355X-native DETR training-step hot path.
 *
 * One shared library, libbdetr.so (built from boosted_detr_amd/csrc with hipcc for
 * gfx950).  The reference (mvenouziou/Boosted_DETR) exposes no FFI: its seam is
 * the Keras object surface and all arithmetic is delegated to TensorFlow /
 * tensorflow_addons / scipy.  Each entry point below therefore cites the
 * reference CALL SITE (ModelComponents/<file>:<line>) whose third-party op it
 * replaces.  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer (HBM) unless named host_*; fp32 unless stated
 *  - the caller owns every buffer including workspaces; the library allocates nothing
 *  - `stream` is a hipStream_t passed as void*; all work is stream-ordered, no
 *    implicit synchronisation, safe to capture into a hipGraph
 *  - return value: 0 = ok, <0 = argument/shape error, >0 = hipError_t; the message
 *    is available from bdetr_last_error() (thread-local); nothing throws or aborts
 *  - activations are NHWC, conv weights are OHWI ([Cout][KH][KW][Cin]), dense
 *    weights are [out][in]; the Python host converts from/to the Keras layouts
 *    (HWIO, [in][out]) at set_weights/get_weights time
 */
#ifndef BDETR_H
#define BDETR_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BDETR_ABI_VERSION 8

int         bdetr_abi_version(void);
const char* bdetr_last_error(void);
/* number of CUs of the current device (used by the host to size split-K) */
int         bdetr_device_cus(void);
/* (additive) The cache policy of stream-once operands in force for this process: BDETR_STREAM_POLICY, read once - a sum of operand-class
 * bits (csrc/stream.h), 0 = every access uses the default policy; a value outside 0..63 is reported on stderr and the built-in default stays.  A policy
 * changes no result. */
int         bdetr_stream_policy(void);

/* A non-blocking stream of the lowest priority class of the device (never destroyed: process lifetime), for
 * work that must not delay the caller's critical path (the host's weight-gradient side stream), and the
 * device's priority range (numerically larger = lower priority). */
int         bdetr_low_priority_stream_create(void** stream_out);
int         bdetr_stream_priority_range(int* least, int* greatest);
/* (ABI 8) Candidates for a PLACED side stream: HIP binds a new stream to one of a few hardware queues in creation order, and the queue it
 * shares - or does not share - a dispatch pipe with decides how two streams overlap (measured: the same training step at 25.1 / 25.3 / 25.2 /
 * 44.3 ms on the four queues a low-priority stream can land on; engine.side_stream).  Creates `ncand` (1..8) lowest-priority non-blocking
 * streams (-> streams_out[ncand], process lifetime) and measures for each how long `ticks` one-workgroup kernels take back to back on
 * `main_stream` while the candidate runs `loads` launches of a streaming kernel over a 64-MB scratch buffer (-> scores_ms[ncand]; smaller
 * = the two streams get in each other's way less; unloaded_ms, may be null: the same ticks with no load beside them).  Allocates and
 * frees its scratch; synchronises the streams - not inside a capture.  bdetr_stream_destroy: for the candidates not kept. */
int         bdetr_side_stream_candidates(void* main_stream, int ncand, int loads, int ticks, void** streams_out, float* scores_ms, float* unloaded_ms);
int         bdetr_stream_destroy(void* stream);

/* Arithmetic of the conv/GEMM family (inputs and outputs are always fp32):
 *  BDETR_GEMM_FP32    every product on v_mfma_f32_32x32x2_f32 (exact fp32 products);
 *  BDETR_GEMM_BF16X3  every operand is split on the fly into hi + lo bf16 halves and a product is
 *                     hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation
 *                     (~2^-18 relative error per product; TensorFlow's TF32 default is 2^-11);
 *  BDETR_GEMM_MIXED   forward products - conv2d_fwd and GEMMs with grad == 0 - are exact fp32 (class
 *                     ids, match indices and ReLU masks are decided by them), gradient products -
 *                     conv2d_bwd_* and GEMMs with grad != 0 - are split-bf16;
 *  BDETR_GEMM_SPLIT   gradient products split-bf16; forward products split-fp16: hi + lo fp16 halves
 *                     (11 + 11 significant bits), three products on v_mfma_f32_32x32x16_f16 - fp32-grade
 *                     products (~2^-22), but forward operands must stay below 65504 in magnitude (a
 *                     larger value raises the range guard).  Since ABI 5 the pre-split (P16) operands keep
 *                     the lo half UNSCALED in ONE accumulator (the f16 MFMA keeps subnormal operands;
 *                     conv weights are packed as 2^8 w and the epilogue multiplies by 2^-8); only
 *                     igemm.hip's IN-KERNEL split (stem, neck, transformer Dense: operands without a
 *                     producer that could pre-scale them) still scales lo by 2^11 into a second accumulator.
 *  BDETR_GEMM_BF16X6  fp32-grade products ON the 16-bit MFMA with fp32's exponent range (round 4): every operand is split on the
 *                     fly into THREE bf16 terms (8 + 8 + 8 significant bits) and a product keeps the six terms down to 2^-16 of
 *                     it - six v_mfma_f32_32x32x16_bf16, ~2^-22.5 relative error per product.  Meant as the policy of a backward
 *                     pass behind a BDETR_GEMM_SPLIT forward (Python: Model.train_grad_precision = "bf16x6"); the attention core
 *                     runs exact fp32 under it.
 * The env variable BDETR_GEMM_PRECISION=fp32|bf16x3|mixed|split|bf16x6 picks the initial value.
 * This policy is the library's ONE piece of mutable state (a mode word like a rounding mode, not data): it is thread-local,
 * so a host thread's launches are unaffected by another thread's policy, and every launch reads it once on the host at
 * enqueue time - kernels already enqueued (or captured into a hipGraph) keep the arithmetic they were enqueued with. */
enum { BDETR_GEMM_FP32 = 0, BDETR_GEMM_BF16X3 = 1, BDETR_GEMM_MIXED = 2, BDETR_GEMM_SPLIT = 3, BDETR_GEMM_BF16X6 = 4 };
int         bdetr_set_gemm_precision(int mode);
int         bdetr_get_gemm_precision(void);

/* Live profiling of the MFMA (igemm) kernel family for bench.py's roofline leg: when enabled,
 * every conv/GEMM launch is bracketed by hipEvents on its own stream.  bdetr_prof_read (after a
 * stream synchronise) returns the summed kernel time, the launch count and the algorithmic FLOPs
 * (2*I*J*R per GEMM) of everything launched since bdetr_prof_enable(1). */
int bdetr_prof_enable(int on);
int bdetr_prof_read(double* total_ms, int64_t* launches, double* flops);
/* the same sums restricted to the launches that ran one arithmetic: 0 exact fp32, 1 split-bf16, 2 split-fp16 */
int bdetr_prof_read_arith(int arith, double* total_ms, int64_t* launches, double* flops);
/* debug aid: one CSV row per recorded launch (shape, tile, loader kinds, ms, GFLOP) */
int bdetr_prof_dump(const char* path);

/* ---- activation codes for the GEMM / conv epilogue ---- */
enum { BDETR_ACT_NONE = 0, BDETR_ACT_RELU = 1, BDETR_ACT_TANH = 2 };

/* ------------------------------------------------------------------------
 * K1  image preparation - backbone.py:49-56 (clip, Resizing, convert_image_dtype
 *     uint8 round trip, resnet50.preprocess_input caffe mode).
 *     in  : [B,h,w,3] fp32 in [0,1] (any h,w; bilinear half-pixel resize to HxW)
 *     out : [B,H,W,4] fp32, channels BGR minus mean, 4th channel = 0 (so the 7x7
 *           stem conv reads 16-byte pixels)
 * ---------------------------------------------------------------------- */
int bdetr_image_prep(const float* in, int B, int h, int w, float* out, int H, int W, void* stream);

/* Targets that are already tokenised and resident in HBM - tokenizers.py:40-82 minus the StringLookup
 * (strings never reach the device): category ids [rows] are range-checked against C, the attribute id
 * slots [rows][slots] become the multi-hot matrix [rows][A] (tf.one_hot + reduce_max over the slot axis,
 * tokenizers.py:72-82; <PAD> slots set bit 0).  An id outside its vocabulary maps to 1 (<OOV>), as
 * StringLookup maps an unknown string.  rows = B*M.  slots = 0: att_ids is not read and may be null; att_hot
 * is all zero. */
int bdetr_tokens_prepare(const int* cat_ids, const int* att_ids, int64_t rows, int slots, int C, int A,
                         int* cat_out, float* att_hot, void* stream);

/* Input-step augmentations (pipeline.py:274-341): per image, bilinear down-size to
 * (new_h,new_w), place at (off_h,off_w) on a zero canvas of the original size, then tf.image
 * adjust_contrast / adjust_brightness / adjust_saturation with the given factors.  in/out: [B,H,W,3]
 * (out != in); iparams int32 [B][4] = new_h,new_w,off_h,off_w; fparams [B][3] = contrast, brightness
 * delta, saturation; ws: bdetr_augment_ws_floats(B) floats.  The random draws are the host's. */
int bdetr_augment_ws_floats(int B);
int bdetr_augment(const float* in, float* out, const int32_t* iparams, const float* fparams,
                  int B, int H, int W, float* ws, void* stream);
/* tf.image.random_jpeg_quality / adjust_jpeg_quality (pipeline.py:319-325): per image, float [0,1] -> uint8 (x * 255.5 truncated,
 * saturating) -> baseline JPEG of quality[b] with 4:2:0 chroma -> decode -> / 255.  Only the lossy stages of the codec run (colour
 * conversion, chroma down-sampling, 8x8 integer DCT, quantisation with the quality-scaled Annex K tables, inverse DCT, fancy
 * up-sampling); entropy coding is lossless and skipped.  The codec is a third-party dependency of the reference (libjpeg-turbo inside
 * TensorFlow): bit-exact against a real libjpeg-turbo through oracle/jpeg_oracle.py (tests/test_jpeg_quality.py).  in == out allowed.
 * quality: int32 [B] on the device; ws: bdetr_jpeg_quality_ws_bytes(B, H, W) bytes. */
int64_t bdetr_jpeg_quality_ws_bytes(int B, int H, int W);
int bdetr_jpeg_quality(const float* in, float* out, const int32_t* quality, int B, int H, int W, void* ws, void* stream);
/* bdetr_augment with the JPEG round trip between brightness and saturation, where the reference has it (pipeline.py:364-383);
 * quality == NULL: exactly bdetr_augment */
int bdetr_augment_jpeg(const float* in, float* out, const int32_t* iparams, const float* fparams, const int32_t* quality,
                       int B, int H, int W, float* ws, void* jpeg_ws, void* stream);

/* ------------------------------------------------------------------------
 * K2/K5/K6  MFMA implicit-GEMM family (v_mfma_f32_32x32x2_f32, LDS-staged tiles).
 * ---------------------------------------------------------------------- */
typedef struct {
    int N, H, W, C;          /* input  NHWC  */
    int K, R, S;             /* output channels, kernel height, kernel width */
    int stride, pad;         /* symmetric zero padding */
    int OH, OW;              /* output spatial size */
} bdetr_conv_desc;

/* conv forward - Keras Conv2D inside keras.applications.ResNet50 (backbone.py:37-38,57)
 * and BackboneNeck.conv2d_downscaler (backbone.py:76-78).
 *   y[N,OH,OW,K] = act(conv(x, w) + bias)
 *   stat_sum/stat_sq (optional, may be NULL): per-row-chunk partial column sums of
 *   y and y*y, shape [bdetr_conv2d_fwd_stat_chunks(d)][K] each - consumed by bdetr_bn_stats_finalize */
int bdetr_conv2d_fwd(const float* x, const float* w, const float* bias, float* y,
                     const bdetr_conv_desc* d, int act, float* stat_sum, float* stat_sq, void* stream);
/* number of partial-statistics rows bdetr_conv2d_fwd writes for this geometry */
int bdetr_conv2d_fwd_stat_chunks(const bdetr_conv_desc* d);
/* dx[N,H,W,C] (+)= conv_transpose(dy, w).  accumulate!=0 adds into dx (residual merge).
 * For stride>1 only 1x1/pad 0 (Keras ResNet-50 v1 strides its 1x1s) and pad 0 with R, S <= stride (taps that do not
 * overlap: panoptic_neck.py:44's 3x3 stride-4 ConvOut) are supported; the untouched pixels of dx are written as zero
 * unless accumulate. */
int bdetr_conv2d_bwd_data(const float* dy, const float* w, float* dx,
                          const bdetr_conv_desc* d, int accumulate, void* stream);
/* dw[K,R,S,C] = sum over pixels; split-K partials are combined with fp32 atomics, so the
 * caller must zero dw first when splitk>1 (bdetr_zero).  splitk<=0 = choose automatically. */
int bdetr_conv2d_bwd_weight(const float* x, const float* dy, float* dw,
                            const bdetr_conv_desc* d, int splitk, void* stream);
int bdetr_conv2d_bwd_weight_splitk(const bdetr_conv_desc* d);
/* Deterministic split-K (ABI 6): the same launch, but every r-slice STORES its partial dw into its own slab of the caller's
 * workspace `ws` (16-byte aligned, ws_elems >= bdetr_splitk_workspace_elems(K, R*S*C, splitk) floats) and a second launch adds
 * the slabs to dw in the fixed order z = 0, 1, ...: two runs give bit-identical gradients.  ws == NULL: the atomic form above.
 * Replaces the same Keras autodiff call sites (backbone.py:37-38,57); the reference itself (TF on CPU) is deterministic. */
int bdetr_conv2d_bwd_weight_ws(const float* x, const float* dy, float* dw,
                               const bdetr_conv_desc* d, int splitk, float* ws, int64_t ws_elems, void* stream);
int64_t bdetr_splitk_workspace_elems(int64_t I, int64_t J, int splitk);

/* ------------------------------------------------------------------------
 * Pre-split ("P16") operand path of the same convolutions - csrc/sgemm.hip.  Replaces the same reference
 * call sites as bdetr_conv2d_* (Keras Conv2D + autodiff inside keras.applications ResNet-50,
 * backbone.py:37-38,57); used by the training step under BDETR_GEMM_SPLIT for every layer whose channel
 * counts allow it (bdetr_p16_supported).
 *
 * P16 layout of a row-major [rows][C] matrix, C % 8 == 0, 4 bytes per element like fp32: every group of 8
 * consecutive elements occupies 32 bytes = [8 x hi (16 bit)][8 x lo (16 bit)].
 *   f16 pair  (forward operands):  hi = f16(x),  lo = f16(x - hi), unscaled;  |x| < 65504 or the value is lost.  For |x| < 2^-3 the
 *             lo half is an f16 subnormal (absolute error <= 2^-25: fp32-grade against an operand tensor of RMS ~1; the MFMA keeps
 *             subnormal operands).  The forward copy of a conv WEIGHT holds 2^8 w (weights are ~1e-2: their lo halves stay normal);
 *             bdetr_p16_conv2d_fwd multiplies by 2^-8 in its epilogue.  All three split products share ONE accumulator.
 *   bf16 pair (gradient operands): hi = bf16(x), lo = bf16(x - hi);          fp32 range
 * The producer of a tensor writes it (bdetr_bn_apply_p16 / bdetr_bn_bwd_p16 / bdetr_p16_pack*), the GEMM moves
 * it HBM -> LDS with buffer_load ... lds and evaluates a product as three 16-bit MFMA products, fp32
 * accumulate - the arithmetic of BDETR_GEMM_SPLIT without the in-kernel split.
 *
 * overflow_flag (device int*, may be null): set to 1 when a value cannot be represented by the f16 pair
 * (|x| >= 65504 or not finite); never cleared by the library. */
/* BatchNormalization apply / backward of bdetr_bn_apply / bdetr_bn_bwd (same reference call sites, same fp32
 * arithmetic) with P16 outputs for the consumer convolutions: out_f16 = forward operand, out_bf16 = weight-
 * gradient operand, out32 = the fp32 tensor; any of the three may be null.  residual_p16 != 0: `residual` is the
 * f16 pair copy of the shortcut tensor (block outputs need not exist in fp32).  bdetr_bn_bwd_p16 writes the input
 * gradient as a bf16 pair (dx_bf16) and, when dx32 != null, in fp32 too.  ReLU mask source of the backward pass
 * (`out`, needed only when a residual was added - otherwise the mask is recomputed from x): out_p16 = 0 the fp32
 * forward output, 1 its bf16 pair copy (the hi half has fp32's range: hi > 0 <=> value > 0), 2 the bit mask that
 * bdetr_bn_apply_p16 writes to relu_mask (uint64 words, (rows*C/4 + 63)/64*4 of them: one bit per element instead of
 * re-reading a 4-byte-per-element tensor in both backward passes). */
/* residual_p16 = 2: `residual` is the RAW output of the projection shortcut's convolution and residual_bn its BatchNorm
 * (batch statistics already reduced): out = relu?(bn(x) + residual_bn(residual)) in one pass - the shortcut's normalised
 * tensor (Keras conv*_block1_0_bn) is never written or read back. */
typedef struct { const float* mean; const float* rstd; const float* gamma; const float* beta; } bdetr_bn_affine;
int bdetr_bn_apply_p16(const float* x, const float* mean, const float* rstd, const float* gamma,
                       const float* beta, const void* residual, int residual_p16, const bdetr_bn_affine* residual_bn, int relu, float* out32,
                       void* out_f16, void* out_bf16, uint64_t* relu_mask, int* overflow_flag, int64_t rows, int C,
                       void* stream);
/* The same pass over the pixels (2i, 2j) of an [N,H,W,C] map alone (rows = N*H*W): the closing BatchNorm + Add + ReLU of a stage's last
 * unit (keras ResNet50 conv2_block3_out, conv3_block4_out, conv4_block6_out), whose only readers are the next stage's stride-2 1x1
 * convolutions conv{3,4,5}_block1_{0,1}_conv and their weight gradients.  Every tensor keeps its full [N,H,W,C] shape and layout; the odd
 * pixels of x and residual are not read, those of out32 / out_f16 / out_bf16 and their relu_mask words are not written, and an even pixel
 * gets exactly what bdetr_bn_apply_p16 gives it - a quarter of the bytes.  Requires H and W even, C % 256 == 0 (a wave's 64 float4s lie
 * in one pixel: mask words and lane pairs are those of the dense pass) and rows*C/4 < 2^32; anything else is an argument error. */
int bdetr_bn_apply_p16_even_pixels(const float* x, const float* mean, const float* rstd, const float* gamma,
                                   const float* beta, const void* residual, int residual_p16, const bdetr_bn_affine* residual_bn, int relu,
                                   float* out32, void* out_f16, void* out_bf16, uint64_t* relu_mask, int* overflow_flag, int64_t rows, int C,
                                   int H, int W, void* stream);
int bdetr_bn_bwd_p16(const float* dout, const void* out, int out_p16, const float* x, const float* mean,
                     const float* rstd, const float* gamma, const float* beta, int relu, int frozen,
                     float* dx32, void* dx_bf16, float* dgamma, float* dbeta, float* dresidual,
                     float* ws, const float* pre_g, const float* pre_gx, int pre_n, int64_t rows, int C, void* stream);
/* pre_g / pre_gx [pre_n][C] (may be null): partial sums of g and g * xhat already produced by the backward-data
 * epilogue that wrote dout (bdetr_p16_conv2d_bwd_data_bnstats); the reduction pass over dout and x is skipped. */
/* The same for a dout [N,H,W,C] that is zero outside the pixels (2i, 2j): the gradient of a stage's last unit, which reaches it only
 * through the backward-data of the next stage's stride-2 1x1 convolutions (keras ResNet50 conv{3,4,5}_block1_{0,1}_conv).  The
 * reduction pass visits those N * ceil(H/2) * ceil(W/2) rows only - a quarter of the bytes; the apply pass is the dense one.  With
 * dout_compact neither pass reads the ReLU mask source at a pixel off (2i, 2j): its gradient is zero whatever the mask says, and after
 * bdetr_bn_apply_p16_even_pixels that part of the mask was never written. */
int bdetr_bn_bwd_p16_even_pixels(const float* dout, const void* out, int out_p16, const float* x, const float* mean,
                                 const float* rstd, const float* gamma, const float* beta, int relu, int frozen,
                                 float* dx32, void* dx_bf16, float* dgamma, float* dbeta, float* dresidual,
                                 float* ws, int N, int H, int W, int C,
                                 int dout_compact /* ABI 7: dout is the compact [N, H/2, W/2, C] tensor of those pixels alone (H, W even;
                                 dresidual must be null): see bdetr_p16_conv2d_bwd_data_masked_accum_compact */, void* stream);
int bdetr_p16_supported(const bdetr_conv_desc* d);
int bdetr_p16_pack(const float* x, int64_t n, void* f16_out, void* bf16_out, int* overflow_flag, void* stream);
int bdetr_p16_unpack(const void* p, int is_f16, int64_t n, float* out, void* stream);
/* w [K][R][S][C] fp32 -> w_f16 P16-f16 [K][R*S*C] (forward B operand) and wt_bf16 P16-bf16 [C][R*S][K] with
 * flipped taps, wt[c][r][s][k] = w[k][R-1-r][S-1-s][c] (backward-data B operand); either may be null */
int bdetr_p16_pack_conv_weights(const float* w, int K, int R, int S, int C, void* w_f16, void* wt_bf16,
                                int* overflow_flag, void* stream);
/* the same for many weight tensors in one launch: `table` (device) holds ntensors rows of 7 int64
 * {w, w_f16, wt_bf16, K, R, S, C}; null output pointers skip that copy */
int bdetr_p16_pack_conv_weights_multi(const int64_t* table, int ntensors, int* overflow_flag, void* stream);
/* y fp32 [N,OH,OW,K] = conv(x_f16 P16-f16 [N,H,W,C], w_f16) + bias, act, BatchNorm partial column sums as
 * bdetr_conv2d_fwd (stat_* sized with bdetr_p16_conv2d_fwd_stat_chunks rows) */
int bdetr_p16_conv2d_fwd_stat_chunks(const bdetr_conv_desc* d);
int bdetr_p16_conv2d_fwd(const void* x_f16, const void* w_f16, const float* bias, float* y,
                         const bdetr_conv_desc* d, int act, float* stat_sum, float* stat_sq, void* stream);
/* dx fp32 [N,H,W,C] (+)= conv_transpose(dy_bf16 P16-bf16 [N,OH,OW,K], wt_bf16) */
int bdetr_p16_conv2d_bwd_data(const void* dy_bf16, const void* wt_bf16, float* dx,
                              const bdetr_conv_desc* d, int accumulate, void* stream);
/* The same product with the BatchNorm-backward REDUCTION of the layer that produced this conv's input fused into the
 * epilogue: dx is the gradient of out = relu?(gamma * (y - mean) * rstd + beta) (no residual), and while the dx tile is
 * stored its per-column partial sums of g = dx * [out > 0] and g * xhat are written to part_g / part_gx
 * [bdetr_p16_conv2d_bwd_data_stat_chunks(d)][C] - the pass of bdetr_bn_bwd(_p16) that would re-read dx and y.  Hand
 * them to bdetr_bn_bwd_p16 (pre_g / pre_gx / pre_n). */
typedef struct {
    const float* y; const float* mean; const float* rstd; const float* gamma; const float* beta; int relu;
    float* part_g; float* part_gx;
    const uint64_t* relu_mask;      /* may be null; else out = relu(bn(y) + shortcut): the ReLU decision is bdetr_bn_apply_p16's bit mask (1x1 convs only) */
    /* A second BatchNorm over the SAME gradient (may be null; bdetr_p16_conv2d_bwd_data_masked_accum with relu_mask only): the projection
     * shortcut of a stage's first unit, out = relu(bn3(y3) + bn0(y0)) (keras.applications.resnet block1 with conv_shortcut, reference
     * backbone.py:37-38).  Its sum of g is part_g; part_gx2 receives its sum of g * xhat0, xhat0 = (y2 - mean2) * rstd2. */
    const float* y2; const float* mean2; const float* rstd2; float* part_gx2;
} bdetr_bn_bwd_fuse;
int bdetr_p16_conv2d_bwd_data_stat_chunks(const bdetr_conv_desc* d);
/* x <- x * relu_mask in place (n elements, n % 4 == 0): materialises a gradient that was handed on with its unit's ReLU mask
 * still to be applied, for consumers other than bdetr_p16_conv2d_bwd_data_masked_accum / bdetr_bn_bwd_p16(out_p16 = 2). */
int bdetr_relu_mask_apply(float* x, const uint64_t* relu_mask, int64_t n, void* stream);
/* 1x1 stride-1 backward-data that merges the skip branch of a residual unit: on entry dx holds the gradient of the unit's
 * OUTPUT (after the ReLU), on exit dx = conv_transpose(dy) + dx * relu_mask, relu_mask = the 1-bit-per-element mask
 * bdetr_bn_apply_p16 wrote for that unit.  The masked gradient of the skip branch (Keras: the Add + Activation of
 * keras.applications.resnet block1, reference backbone.py:37-38) is never materialised. */
int bdetr_p16_conv2d_bwd_data_masked_accum(const void* dy_bf16, const void* wt_bf16, float* dx, const uint64_t* relu_mask,
                                           const bdetr_conv_desc* d, const bdetr_bn_bwd_fuse* bn /* may be null: the BatchNorm-backward
                                           sums of the unit whose output gradient this launch completes */, void* stream);
/* (ABI 7) The same merge when the unit's output gradient exists only at the even pixels: old_even is the COMPACT fp32
 * [N, H/2, W/2, C] tensor that the stride-2 1x1 backward-data products of the next stage wrote densely (Keras: the stride-2 conv1 and
 * projection shortcut of the next stage's first block, reference backbone.py:37-38), zero everywhere else - no zero-filled dense
 * gradient is ever written.  dx (fp32 [N,H,W,C], uninitialised on entry) = conv_transpose(dy) + expand(old_even) * relu_mask. */
int bdetr_p16_conv2d_bwd_data_masked_accum_compact(const void* dy_bf16, const void* wt_bf16, float* dx, const float* old_even,
                                                   const uint64_t* relu_mask, const bdetr_conv_desc* d, const bdetr_bn_bwd_fuse* bn, void* stream);
int bdetr_p16_conv2d_bwd_data_bnstats(const void* dy_bf16, const void* wt_bf16, float* dx,
                                      const bdetr_conv_desc* d, const bdetr_bn_bwd_fuse* bn, void* stream);
/* dw fp32 [K][R][S][C] += sum over pixels of dy x patches(x); with splitk > 1 the slices add with float
 * atomics, so dw must hold zeros (or the running sum) on entry */
int bdetr_p16_conv2d_bwd_weight_splitk(const bdetr_conv_desc* d);
int bdetr_p16_conv2d_bwd_weight(const void* x_bf16, const void* dy_bf16, float* dw,
                                const bdetr_conv_desc* d, int splitk, void* stream);
/* The same with x given as the P16-f16 tensor the FORWARD of this convolution read: the kernel converts each fragment to a bf16 pair
 * in registers ((hi + lo) is exact in fp32, then the bf16 split), so a producer (bdetr_bn_apply_p16, bdetr_p16_pack) need not
 * write a bf16 copy of an activation at all: 4 bytes per element of HBM traffic and of saved-activation memory less. */
int bdetr_p16_conv2d_bwd_weight_xf16(const void* x_f16, const void* dy_bf16, float* dw,
                                     const bdetr_conv_desc* d, int splitk, void* stream);
/* deterministic split-K form of the two above (see bdetr_conv2d_bwd_weight_ws); x_is_f16 selects the xf16 operand flavour */
int bdetr_p16_conv2d_bwd_weight_ws(const void* x, int x_is_f16, const void* dy_bf16, float* dw,
                                   const bdetr_conv_desc* d, int splitk, float* ws, int64_t ws_elems, void* stream);

/* strided-batched GEMM - tf Dense / tf.linalg.matmul call sites
 * (transformers.py:41-48,62-65,86,97,101,174-177; prediction_heads.py:40-43,106-110,175-179)
 *   C[b][i][j] = act(alpha * sum_r A(b,i,r) * B(b,j,r) + bias[j])      (accumulate: C += ...)
 *   a_rcontig: A(b,i,r) at a + i*lda + r, else at a + r*lda + i           (same for B with j)
 *   batch index b = b0*nb1 + b1, operand offset = b0*s?0 + b1*s?1
 *   splitk>1 splits the r range over gridDim.z and combines with atomics (C must be zeroed,
 *   nb0*nb1 must be 1, bias/act must be off). */
typedef struct {
    int I, J, R;
    int nb0, nb1;
    const float* a; int64_t lda, sa0, sa1; int a_rcontig;
    const float* b; int64_t ldb, sb0, sb1; int b_rcontig;
    float*       c; int64_t ldc, sc0, sc1;
    const float* bias; float alpha; int act; int accumulate; int splitk;
    int grad;                /* != 0: a gradient (backward) product - see BDETR_GEMM_MIXED */
} bdetr_gemm_desc;
int bdetr_gemm(const bdetr_gemm_desc* g, void* stream);
/* bdetr_gemm with a deterministic split-K reduction (g->splitk > 1, dense C: ldc == J): slabs in `ws`
 * (>= bdetr_splitk_workspace_elems(I, J, splitk) floats), fixed-order fold into C (C += sum of the slices).  ws == NULL: bdetr_gemm. */
int bdetr_gemm_ws(const bdetr_gemm_desc* g, float* ws, int64_t ws_elems, void* stream);
/* n (1..4) independent GEMMs that share J, R, leading dimensions, operand flavours and epilogue flags
 * (their pointers, bias and row count I may differ) in ONE launch - the Q/K/V projections of an
 * attention block (transformers.py:68-70) and their input gradients.  No batching inside.  splitk > 1 (the same value in every
 * problem, problems of one shape, no bias / activation): every problem's r range is cut into the same slices, which ADD into C
 * with float atomics (C zeroed by the caller) - the weight gradients of one layer's Dense kernels in one launch. */
int bdetr_gemm_grouped(const bdetr_gemm_desc* g, int n, void* stream);

/* column sums: out[j] = sum_i x[i][j]  (bias gradients; Keras autodiff of Dense/Conv bias).
 * Deterministic two-level reduction; ws: cols * bdetr_colsum_chunks(rows) floats. */
int bdetr_colsum_chunks(int64_t rows);
int bdetr_colsum(const float* x, int64_t rows, int cols, float* out, float* ws, void* stream);
/* the same sum ADDED into out with float atomics in one launch (no workspace): out must hold zeros or the running
 * sum - the host's flat gradient buffer is zero-filled once per step */
int bdetr_colsum_accumulate(const float* x, int64_t rows, int cols, float* out, void* stream);
/* n <= 4 such column sums of one width in ONE launch (the bias gradients of an attention block's Q / K / V projections,
 * transformers.py:68-70 + autodiff).  xs / rows / outs are HOST arrays of n entries; outs[m] must hold zeros or the running sum. */
int bdetr_colsum_accumulate_group(const float* const* xs, const int64_t* rows, int cols, float* const* outs, int n, void* stream);

/* ------------------------------------------------------------------------
 * K3  BatchNormalization, training mode (keras BN inside ResNet-50, backbone.py:79-80,
 *     prediction_heads.py:42,108,177; semantics SURVEY S5).  x is [rows][C].
 * ---------------------------------------------------------------------- */
/* partial column sums of x and x*x over row chunks: part_* are [bdetr_bn_bwd_chunks(rows)][C].
 * (The conv/GEMM epilogue produces the same partials for free - see bdetr_conv2d_fwd.) */
int bdetr_colstats(const float* x, int64_t rows, int C, float* part_sum, float* part_sq, void* stream);
/* reduce nparts partial rows (from bdetr_colstats or a conv epilogue) in fp64, fixed order, into
 * mean[C], rstd[C] (biased variance); if moving_mean!=NULL update the moving statistics
 * (momentum; bessel!=0 uses the unbiased variance for the moving estimate).  x is unused. */
int bdetr_bn_stats(const float* x, int64_t rows, int C, const float* part_sum, const float* part_sq,
                   int nparts, float eps, float momentum, int bessel,
                   float* mean, float* rstd, float* moving_mean, float* moving_var, float* fold_ws,
                   int* guard_flag, void* stream);
/* guard_flag (device int*, may be null): the step's range guard.  The P16-f16 producers set it when a forward
 * activation leaves the f16 pair's range; bn_stats sets it when the batch statistics are not finite and skips
 * the moving-statistics update while it is set; bdetr_flag_nonfinite sets it for a non-finite loss; the
 * optimizer applies nothing while it is set.  The host reads and clears it and redoes the step on the
 * exact-fp32 forward (the reference's fp32 arithmetic has no such range limit). */
int bdetr_flag_nonfinite(const float* x, int64_t n, int* flag, void* stream);
/* The guard word logged per step without a host synchronisation.  ordinal: one device int, advanced by each call's kernel;
 * host_ring: 1 + ring_len ints of pinned, device-mapped HOST memory.  The kernel stores *flag at host_ring[1 + ordinal % ring_len]
 * and then the ordinal at host_ring[0], so a host that finds host_ring[0] >= k may read step k's entry (Model._guard_poll).
 * Capturable: it belongs to the step (the last launch of its optimizer segment), nothing is enqueued between steps. */
int bdetr_flag_snapshot(const int* flag, int* ordinal, int* host_ring, int ring_len, void* stream);
/* Diagnostic of the hipGraph replay path (no reference counterpart; tools/graph_segment_checksums.py): appends
 * {wrapping sum of x's bit patterns, count of non-finite elements, tag} to log[3 * (*cursor)++] (device memory, `cap` entries;
 * scratch: two zeroed device words).  Order-independent, stream-ordered, capturable: every replay of a segment appends an entry. */
int bdetr_debug_checksum(const float* x, int64_t n, uint64_t* scratch, uint64_t* log, int* cursor, int cap, uint64_t tag, void* stream);
/* Diagnostic of the hipGraph replay path (ABI 7; no reference counterpart): counts[t] = nodes of hipGraphNodeType t in `graph` (a
 * hipGraph_t; types >= ncounts are counted in the last slot).  The captured training step must hold kernel nodes only - a hipMemset node
 * replayed wrongly on this runtime (round 4) - and engine.SegmentedCapture enforces that with this call under BDETR_GRAPH_CENSUS=1. */
int bdetr_graph_node_census(void* graph, int64_t* counts, int ncounts);
/* fold_ws (optional): 2*C*bdetr_bn_stats_fold_rows() floats; lets bn_stats pre-reduce thousands of
 * epilogue partial rows with a wide grid before the fp64 finalise */
int bdetr_bn_stats_fold_rows(void);
/* inference-mode statistics: mean = moving_mean, rstd = 1/sqrt(moving_var+eps) */
int bdetr_bn_stats_frozen(const float* moving_mean, const float* moving_var, int C, float eps,
                          float* mean, float* rstd, void* stream);
/* out = [relu]( gamma*(x-mean)*rstd + beta [+ residual] ) */
int bdetr_bn_apply(const float* x, const float* mean, const float* rstd, const float* gamma,
                   const float* beta, const float* residual, int relu, float* out,
                   int64_t rows, int C, void* stream);
/* backward of bn_apply.  dout: gradient w.r.t. out; out: forward output (for the ReLU mask;
 * may be NULL when relu==0, or when relu==1 and there was no residual: the mask is then recomputed
 * from x with the forward's exact affine map, saving one full read of `out` per pass).  Produces dx, dgamma[C], dbeta[C] and, when dresidual!=NULL,
 * the masked gradient that flows to the residual branch (dresidual may alias dout).
 * frozen!=0: statistics were constants (inference-mode BN).  ws: 2*C*nchunks floats where
 * nchunks = bdetr_bn_bwd_chunks(rows). */
int bdetr_bn_bwd_chunks(int64_t rows);
int bdetr_bn_bwd(const float* dout, const float* out, const float* x, const float* mean,
                 const float* rstd, const float* gamma, const float* beta, int relu, int frozen,
                 float* dx, float* dgamma, float* dbeta, float* dresidual,
                 float* ws, int64_t rows, int C, void* stream);

/* ------------------------------------------------------------------------
 * K3b BatchNormalization over row groups (csrc/groupnorm_rows.hip): x is [G*R][C] and group g = rows [g*R, (g+1)*R) is
 *     normalised with its OWN batch statistics - what G separate keras BatchNormalization calls on [R][C] compute
 *     (the shared prediction heads behind every decoder layer, model.py:179-186 with use_intermediate_losses).
 *     One launch for the statistics, one for the apply, two for the backward, independent of G; no atomics, fixed
 *     summation order.  C % 4 == 0, G <= 65535, G*R < 2^31, tensors 16-byte aligned.  G = 1 is plain BatchNorm.
 * ---------------------------------------------------------------------- */
/* mean, rstd, var: [G][C] (biased variance, fp64 finalise).  guard_flag (may be null): set when a statistic is not finite. */
int bdetr_bn_rows_stats(const float* x, int G, int64_t R, int C, float eps, float* mean, float* rstd, float* var,
                        int* guard_flag, void* stream);
/* out = gamma*(x-mean_g)*rstd_g + beta.  grouped_stats != 0: mean/rstd are [G][C], else [C] shared by every group (moving
 * statistics).  moving_mean != NULL (needs grouped_stats and var): the moving statistics are updated G times in group order,
 * mm <- momentum*mm + (1-momentum)*mean_g (variance alike: biased) - unless guard_flag (may be null) is set. */
int bdetr_bn_rows_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float* out,
                        int G, int64_t R, int C, int grouped_stats, const float* var, float momentum, float* moving_mean,
                        float* moving_var, const int* guard_flag, void* stream);
/* backward: dgamma[C] / dbeta[C] = sums over ALL rows of g*xhat / g (xhat from the row's own group), dx from the row's own
 * group's sums; frozen != 0: the statistics were constants (dx = g*rstd*gamma).  ws: 2*G*C floats. */
int bdetr_bn_rows_bwd(const float* dout, const float* x, const float* mean, const float* rstd, const float* gamma,
                      int grouped_stats, int frozen, float* dx, float* dgamma, float* dbeta, float* ws, int G, int64_t R, int C,
                      void* stream);

/* ------------------------------------------------------------------------
 * K4 3x3/2 max-pool with 1-pixel zero pad (ResNet-50 pool1_pad + pool1_pool)
 * ---------------------------------------------------------------------- */
int bdetr_maxpool3x3s2_fwd(const float* x, float* y, int N, int H, int W, int C, int OH, int OW, void* stream);
int bdetr_maxpool3x3s2_bwd(const float* x, const float* y, const float* dy, float* dx,
                           int N, int H, int W, int C, int OH, int OW, void* stream);

/* The ResNet stem's tail in one pass each way (training, batch statistics): BatchNormalization -> ReLU -> ZeroPadding2D(1) ->
 * MaxPool 3x3/2 over the RAW conv1 output y [N,H,W,C] (keras ResNet50 conv1_bn .. pool1_pool, reached from backbone.py:79-80).
 * fwd: pooled tensor [N,PH,PW,C] (PH = (H-1)/2+1) as fp32 (out32) and / or as the f16 pair of the P16 layout (out_f16), plus
 *      tap [N,PH,PW,C] bytes: which of the window's 9 taps (row-major) held the maximum - the first one on a tie.
 * bwd: dpool [N,PH,PW,C] -> dy [N,H,W,C] (gradient of the raw conv output), dgamma, dbeta; the normalised full-resolution tensor
 *      and its gradient are never materialised.  ws: 2*C*bdetr_stem_pool_bwd_chunks(N*H*W) floats.  C % 8 == 0, N*H*W < 2^31. */
int bdetr_stem_pool_bwd_chunks(int64_t rows);
int bdetr_stem_pool_fwd(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                        int N, int H, int W, int C, float* out32, void* out_f16, uint8_t* tap, int* overflow_flag, void* stream);
int bdetr_stem_pool_bwd(const float* dpool, const uint8_t* tap, const float* y, const float* mean, const float* rstd, const float* gamma,
                        const float* beta, int N, int H, int W, int C, float* dy, int dy_p16 /* ABI 7: write dy as the P16 bf16 pair
                        (the operand of bdetr_p16_stem_bwd_weight) instead of fp32 */, float* dgamma, float* dbeta, float* ws, void* stream);
/* The stem's weight gradient on pre-split operands (ABI 7).  keras ResNet50 conv1_conv - 7x7 / stride 2 on the ZeroPadding2D(3) image,
 * reference backbone.py:37-38 - reads a 4-channel image, which the P16 layout (groups of 8 channels) cannot hold; space-to-depth makes it
 * a size-preserving stride-1 4x4 convolution over x2[n][i][j][(a,b,c)] = x[n][2i+a][2j+b][c] (16 channels, low-side padding 2), tap (r,s) =
 * (2r'+a-1, 2s'+b-1).  bdetr_p16_s2d_pack_bf16: x fp32 [N,H,W,4] (H, W even) -> x2 P16-bf16 [N,H/2,W/2,16].  bdetr_p16_stem_bwd_weight:
 * dw2 fp32 [K][4][4][16] += sum over pixels of dy x patches(x2) (dw2 must hold zeros: split-K float atomics; K % 64 == 0; dy P16-bf16
 * [N,H/2,W/2,K]).  bdetr_p16_s2d_unpack_dw: dw [K][7][7][4] <- dw2 (the r = -1 / s = -1 taps of the 4x4 form do not exist and are dropped). */
int bdetr_p16_s2d_pack_bf16(const float* x, int N, int H, int W, void* out_bf16, void* stream);
int bdetr_p16_stem_bwd_weight(const void* x2_bf16, const void* dy_bf16, float* dw2, int N, int H2, int W2, int K, void* stream);
int bdetr_p16_s2d_unpack_dw(const float* dw2, float* dw, int K, void* stream);

/* ------------------------------------------------------------------------
 * K7  attention softmax (transformers.py:88-94): p = softmax(scale*s) row-wise, in place ok.
 *     bwd: ds = scale * p * (dp - sum_k dp*p)
 * ---------------------------------------------------------------------- */
int bdetr_softmax_rows_fwd(const float* s, float* p, int64_t rows, int cols, float scale, void* stream);
int bdetr_softmax_rows_bwd(const float* p, const float* dp, float* ds, int64_t rows, int cols, float scale, void* stream);

/* Fused attention core for head dimension bdetr_attention_head_dim() (= 32): the [B,h,q,k] scores
 * never reach HBM (online softmax in registers, K/V streamed through LDS, fp32 MFMA).
 *   q [B,nq,h*32], k/v [B,nk,h*32]  ->  o [B,h,nq,32] (the layout transformers.py:100 reshapes
 *   without a permute), lse [B,h,nq] = log-sum-exp of the scaled scores (kept for the backward).
 *   bwd: dq [B,nq,h*32], dk/dv [B,nk,h*32]; dvec_ws: B*h*nq floats of workspace. */
int bdetr_attention_head_dim(void);
int bdetr_attention_fwd(const float* q, const float* k, const float* v, float* o, float* lse,
                        int B, int h, int nq, int nk, float scale, void* stream);
int bdetr_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                        const float* lse, float* dq, float* dk, float* dv, float* dvec_ws,
                        int B, int h, int nq, int nk, float scale, void* stream);

/* ------------------------------------------------------------------------
 * K8  residual + dropout + LayerNormalization (transformers.py:135-137,178-180)
 *     h = x + dropout(y) ; out = gamma*(h-mean)*rstd + beta   (eps 1e-3, biased var)
 *     dropout: inverted, keep-prob 1-rate, counter-based RNG keyed by (seed, element index);
 *     rate==0 disables.  seed_base (device uint64*, may be null): a per-step value kept in HBM and folded
 *     into `seed`, so that a captured hipGraph draws fresh masks on every replay (the host updates the word
 *     between replays); forward and backward of one layer must be given the same pair.
 * ---------------------------------------------------------------------- */
int bdetr_add_dropout_layernorm_fwd(const float* x, const float* y, const float* gamma, const float* beta,
                                    float* out, float* mean, float* rstd, int64_t rows, int D,
                                    float eps, float rate, uint64_t seed, const uint64_t* seed_base, void* stream);
/* given dout: dx (gradient to x, = dh), dy (gradient to y, = dh * dropout mask), dgamma, dbeta.
 * `out` is the forward output (h is recovered as (out-beta)/gamma is NOT used; xhat is
 * recomputed from x,y,mean,rstd).  ws: 2*D*bdetr_ln_bwd_chunks(rows) floats. */
int bdetr_ln_bwd_chunks(int64_t rows);
int bdetr_add_dropout_layernorm_bwd(const float* dout, const float* x, const float* y, const float* gamma,
                                    const float* mean, const float* rstd, float* dx, float* dy,
                                    float* dgamma, float* dbeta, float* ws, int64_t rows, int D,
                                    float rate, uint64_t seed, const uint64_t* seed_base, int accumulate_dx, void* stream);

/* ----------------------------------------------------------------------
 * Row chain (csrc/rowchain.hip, ABI 6): the row-local part of a transformer layer between two attention cores as ONE launch
 * per direction, model width 256 (bdetr_rowchain_width).  Replaces, for an AttentionBlock followed by a FeedForwardBlock
 * (transformers.py:101 OutputProjection, 135-137 Add + Dropout + LayerNormalization, 174-177 DenseRelu / DenseLinear, 178-180
 * Add + Dropout + LayerNormalization) the five forward and ~twenty backward launches of the unfused path:
 *     a = ctx Wo^T + bo;  x1 = LN1(resid + drop1(a));  h = relu(x1 W1^T + b1);  f = h W2^T + b2;  x2 = LN2(x1 + drop2(f))
 * nstages = 3: the whole chain; nstages = 1: stage 1 only (an AttentionBlock followed by another AttentionBlock:
 * DecoderBlock's self-attention, transformers.py:378-383).  All activations fp32 [M][256] row-major; weights PRE-PACKED by
 * bdetr_rowchain_pack_weights (per-optimizer-step, one launch for all matrices): forward copy = f16 pairs of 2^8 W in MFMA
 * fragment order, backward copy = bf16 pairs of W^T (the 'split' policy's arithmetic: BDETR_GEMM_SPLIT above; other policies
 * use the unfused path).  Dropout: the hash, seeds and element indices of bdetr_add_dropout_layernorm_* - same masks.
 * Forward saves what the backward needs: pre1 / pre2 (the LayerNorm inputs resid + drop(a), x1 + drop(f)), mean / rstd, h.
 * ---------------------------------------------------------------------- */
typedef struct {
    int64_t M; int nstages; float eps, rate;
    const float* ctx; const float* resid;
    const void* w[3];            /* packed forward copies of Wo, W1, W2 */
    const float* bias[3];
    const float* g1; const float* b1; const float* g2; const float* b2;      /* LayerNorm gamma / beta */
    float* pre1; float* x1; float* mean1; float* rstd1;                      /* x1 = the result when nstages == 1 */
    float* h; float* pre2; float* x2; float* mean2; float* rstd2;
    uint64_t seed1, seed2; const uint64_t* seed_base;
} bdetr_rowchain_fwd_desc;
int bdetr_rowchain_fwd(const bdetr_rowchain_fwd_desc* d, void* stream);
/* Backward of the same chain from dout = gradient of x2 (nstages 3) or x1 (nstages 1): writes dctx and dresid, the three Dense
 * layers' output gradients G0 (of a), G1 (of the ReLU's input), G2 (of f) - the operands of their weight gradients, which stay
 * GEMMs of their own (dW = G^T X: bdetr_gemm) - and one row of partial sums per 32-token workgroup for the seven vector
 * gradients {dgamma2, dbeta2, dbias2, dbias1, dgamma1, dbeta1, dbias0} (for nstages == 1 only the last three are written):
 * partials holds bdetr_rowchain_partial_rows(M) x 7 x 256 floats; bdetr_rowchain_reduce folds them in a fixed order into up to
 * seven destinations (dst7[v] may be null; accumulate7[v] != 0: add to what is there). */
typedef struct {
    int64_t M; int nstages; float rate;
    const float* dout;
    const float* pre2; const float* mean2; const float* rstd2; const float* g2;
    const float* h;
    const float* pre1; const float* mean1; const float* rstd1; const float* g1;
    const void* wt[3];           /* packed backward copies of Wo, W1, W2 */
    float* G2; float* G1; float* G0;
    float* dresid; float* dctx;
    float* partials;
    uint64_t seed1, seed2; const uint64_t* seed_base;
} bdetr_rowchain_bwd_desc;
int bdetr_rowchain_bwd(const bdetr_rowchain_bwd_desc* d, void* stream);
int bdetr_rowchain_reduce(const float* partials, int nparts, float* const* dst7, const int* accumulate7, void* stream);
int bdetr_rowchain_width(void);
int64_t bdetr_rowchain_pack_elems(void);                 /* floats (4-byte units) of one packed copy of a 256 x 256 matrix */
int bdetr_rowchain_partial_rows(int64_t M);
/* table: device int64 [n][3] rows {W fp32 [256 out][256 in], forward copy | 0, backward copy | 0}; overflow_flag: the range guard
 * (a weight whose 2^8 multiple leaves the f16 range raises it) */
int bdetr_rowchain_pack_weights(const int64_t* table, int n, int* overflow_flag, void* stream);

/* ------------------------------------------------------------------------
 * Panoptic head (the forward - the reference never wires it into a loss; its training: next block):
 * panoptic_neck.py:20-21 Resizing (bilinear, half-pixel centres), 118-121 / 164-167 channel LayerNormalization
 * (eps 1e-3) + ReLU(negative_slope), 33-47 Concatenate / transpose; transformers.py:519 LayerNormalization.
 * Channel counts of the head are arbitrary (66, 44, 29 ...): tensors are stored with the channel dimension
 * zero-padded to a multiple of 4 (ld), and the convolutions run on bdetr_conv2d_fwd with zero-padded weights.
 *   resize        in [B,h,w,C] -> out [B,H,W,C], C % 4 == 0
 *   layernorm_act out[r][c] = leaky_slope(gamma[c] * (x[r][c] - mean_r) * rstd_r + beta[c]) for c < C, 0 for C <= c < ldo
 *   copy_cols     dst[r][dst_col0 + c] = src[r][c], c < C            (channel concatenation / padding)
 *   nhwc_to_nchw  out[b][c][p] = in[b][p][c], c < C of ld_in columns
 * ---------------------------------------------------------------------- */
int bdetr_resize_bilinear_nhwc(const float* in, int B, int h, int w, int C, float* out, int H, int W, void* stream);
int bdetr_layernorm_act_fwd(const float* x, int64_t rows, int C, int ldx, const float* gamma, const float* beta,
                            float eps, float slope, float* out, int ldo, void* stream);
int bdetr_copy_cols(const float* src, int64_t rows, int C, int ld_src, float* dst, int ld_dst, int dst_col0, void* stream);
int bdetr_nhwc_to_nchw(const float* in, int B, int P, int C, int ld_in, float* out, void* stream);

/* ------------------------------------------------------------------------
 * Panoptic head training (DETR(train_panoptic_head=True)): the adjoints of the pieces above, the device pack of the head's
 * Keras-layout conv variables, and a mask loss.  The pack replaces a host-side repack of the Conv2D /
 * Conv2DTranspose kernels of panoptic_neck.py:91-186 (a pure copy); the rest adds what the reference lacks: it never trains
 * these layers and defines no mask loss (its model.py:4), so the loss is the DETR paper's
 * panoptic-head loss (sigmoid focal, alpha .25 gamma 2 as TFA sigmoid_focal_crossentropy, averaged over the pixels,
 * + DICE) on the matched queries.  Deterministic: no float atomics.
 *   layernorm_act_bwd   adjoint of layernorm_act (x = the forward's input, dout [rows][ldo]): dx [rows][ldx] (0 beyond C),
 *                       dgamma / dbeta [C]; part_g / part_b: workspaces of bdetr_layernorm_act_bwd_chunks(rows) x C floats
 *   resize_bwd          adjoint of resize (dout [B,H,W,C] -> din [B,h,w,C]) as a gather over the output pixels, C % 4 == 0
 *   nchw_to_nhwc        out[b][p][c] = in[b][c][p] for c < C, 0 for C <= c < ld_out (adjoint of nhwc_to_nchw)
 *   conv_weight_pack    w [Kp][R][S][Cp] = Keras kernel HWIO [R][S][Cin][K] (transpose: the Conv2DTranspose kernel [R][S][K][Cin]
 *                       with flipped taps), zeros beyond K / Cin; b [Kp] = bias, zeros beyond K
 *   conv_weight_unpack  its adjoint: dkernel (Keras layout) / dbias [K] from the padded dw / db (either output may be null)
 *   mask_loss           logits [B][N][P], masks [B][M][P], match int32 [B][M] (prediction per object, -1 none), num_objects [B]:
 *                       row_loss [B][N] (focal + dice of the query's matched object, 0 unmatched; workspace), loss [B] =
 *                       mask_weight * sum_n row_loss / max(n_b, 1), dlogits [B][N][P] = loss_scale * dloss / dlogits (null: none)
 * ---------------------------------------------------------------------- */
int bdetr_layernorm_act_bwd_chunks(int64_t rows);
int bdetr_layernorm_act_bwd(const float* x, int64_t rows, int C, int ldx, const float* gamma, const float* beta, float eps, float slope,
                            const float* dout, int ldo, float* dx, float* part_g, float* part_b, float* dgamma, float* dbeta, void* stream);
int bdetr_resize_bilinear_nhwc_bwd(const float* dout, int B, int H, int W, int C, float* din, int h, int w, void* stream);
int bdetr_nchw_to_nhwc(const float* in, int B, int P, int C, float* out, int ld_out, void* stream);
int bdetr_conv_weight_pack(const float* kernel, const float* bias, int R, int S, int Cin, int K, int transpose, int Cp, int Kp,
                           float* w, float* b, void* stream);
int bdetr_conv_weight_unpack(const float* dw, const float* db, int R, int S, int Cin, int K, int transpose, int Cp,
                             float* dkernel, float* dbias, void* stream);
int bdetr_mask_loss(const float* logits, const float* masks, const int* match, const int* num_objects, int B, int M, int N, int P,
                    float alpha, float gamma, float mask_weight, float loss_scale, float* row_loss, float* loss, float* dlogits, void* stream);

/* ------------------------------------------------------------------------
 * K9  head activations (prediction_heads.py:44,60-62,111,127-129,180,197-199)
 * ---------------------------------------------------------------------- */
int bdetr_softmax_lastdim_fwd(const float* logits, float* p, int64_t rows, int cols, void* stream);
int bdetr_softmax_lastdim_bwd(const float* p, const float* dp, float* dlogits, int64_t rows, int cols, void* stream);
int bdetr_sigmoid_fwd(const float* x, float* y, int64_t n, void* stream);
int bdetr_sigmoid_bwd(const float* y, const float* dy, float* dx, int64_t n, void* stream);
/* y = 3*sigmoid(x/100) - 1 */
int bdetr_boxsigmoid_fwd(const float* x, float* y, int64_t n, void* stream);
int bdetr_boxsigmoid_bwd(const float* y, const float* dy, float* dx, int64_t n, void* stream);

/* elementwise helpers */
int bdetr_zero(float* p, int64_t n, void* stream);
int bdetr_add(const float* a, const float* b, float* out, int64_t n, void* stream);          /* out = a + b */
int bdetr_add_bcast_rows(const float* a, const float* row, float* out, int64_t rows, int64_t rowlen, void* stream); /* out[r] = a[r] + row (batch broadcast) */
int bdetr_sum_over_batch(const float* x, float* out, int64_t batch, int64_t n, int accumulate, void* stream);       /* out = sum_b x[b] */
int bdetr_tanh_bwd(const float* y, const float* dy, float* dx, int64_t n, void* stream);
int bdetr_relu_bwd(const float* y, const float* dy, float* dx, int64_t n, void* stream);
int bdetr_axpy(float alpha, const float* x, float* y, int64_t n, void* stream);               /* y += alpha*x */

/* ------------------------------------------------------------------------
 * K10-K12  set criterion (losses_and_metrics.py:111-161, 176-192, 195-251)
 *   One workgroup per image.  Inputs:
 *     cat_pred [B,N,C] probabilities, att_pred [B,N,A], box_pred [B,N,4]
 *     cat_ids  int32 [B,M] (0=<PAD>), att_hot [B,M,A] multi-hot fp32 (may be NULL if A==0 or
 *     attribute_weight==0), bbox [B,M,4] COCO format, num_objects int32 [B]
 *   bdetr_cost_matrix : cost[B,M,N] = 1000*cat + box_w*box + att_w*att  (fp32, summed in the
 *                       reference's order, line 130); optional component outputs.  Rows
 *                       m >= num_objects[b] (never read by the matcher, masked out of the loss)
 *                       are written as 0 when num_objects != NULL
 *   bdetr_lsa         : exact rectangular shortest-augmenting-path (Crouse / scipy semantics,
 *                       fp64 in LDS, scipy's scan order and tie rule), rows i<num_objects[b];
 *                       match[b][m] = assigned prediction index or -1 ;  int32 [B,M]
 *   bdetr_set_loss    : masked reductions + existence BCE + IoU metric and the gradient of
 *                       sum_b total_b w.r.t. the three prediction tensors.
 *                       losses[6][B] = total, category, attribute, box, exist, iou
 *                       loss_scale multiplies the gradients (1/num_replicas under DP, S14).
 * ---------------------------------------------------------------------- */
typedef struct {
    int B, M, N, C, A;
    float category_weight, attribute_weight, box_weight, exist_weight;
} bdetr_loss_desc;
int bdetr_cost_matrix(const bdetr_loss_desc* d, const float* cat_pred, const float* att_pred,
                      const float* box_pred, const int32_t* cat_ids, const float* att_hot,
                      const float* bbox, const int32_t* num_objects, float* cost, float* cost_cat,
                      float* cost_att, float* cost_box, void* stream);
int bdetr_lsa(const float* cost, const int32_t* num_objects, int B, int M, int N,
              int32_t* match, void* stream);
int bdetr_set_loss(const bdetr_loss_desc* d, const float* cat_pred, const float* att_pred,
                   const float* box_pred, const int32_t* cat_ids, const float* att_hot,
                   const float* bbox, const int32_t* num_objects, const int32_t* match,
                   float* losses, float* d_cat, float* d_att, float* d_box, float loss_scale,
                   void* stream);
/* The same three over predictions of SEVERAL calls stacked along the batch axis (the decoder layers' heads, model.py:179-186 with
 * use_intermediate_losses): d->B = L * period prediction images, the targets (cat_ids, att_hot, bbox, num_objects) hold `period` images and
 * prediction image b is matched against target image b % period; each block of `period` images is one loss call of its own (its
 * 1 + sum(num_objects) normaliser runs over the `period` target images).  cost [B,M,N], match [B,M], losses [6][B]. */
int bdetr_cost_matrix_tiled(const bdetr_loss_desc* d, int period, const float* cat_pred, const float* att_pred,
                            const float* box_pred, const int32_t* cat_ids, const float* att_hot,
                            const float* bbox, const int32_t* num_objects, float* cost, void* stream);
int bdetr_lsa_tiled(const float* cost, const int32_t* num_objects, int B, int period, int M, int N,
                    int32_t* match, void* stream);
int bdetr_set_loss_tiled(const bdetr_loss_desc* d, int period, const float* cat_pred, const float* att_pred,
                         const float* box_pred, const int32_t* cat_ids, const float* att_hot,
                         const float* bbox, const int32_t* num_objects, const int32_t* match,
                         float* losses, float* d_cat, float* d_att, float* d_box, float loss_scale,
                         void* stream);
/* mask[B,M,N] = 1 where match[b][m]==n (MatchingAssignment output, for inspection/tests) */
int bdetr_match_to_mask(const int32_t* match, float* mask, int B, int M, int N, void* stream);

/* ------------------------------------------------------------------------
 * K13  optimizers: per-tensor clip-by-norm + Keras SGD(nesterov) (notebook cell 26, S15), and AdamW (same cell).
 *      Multi-tensor: `ptrs` is a device array of ntensors x {w,g,v} pointers, `sizes` the
 *      element counts; norms: ntensors floats of workspace.
 *      Work is split in slabs of bdetr_sgd_slab_elems() elements; the host builds the slab
 *      table once: slab_tensor[nslabs] (owning tensor of each slab) and slab_first[ntensors+1]
 *      (first slab of each tensor), both int64 on the device.  partial: nslabs floats.
 *      lr is read from device memory (so a captured graph sees schedule updates).
 *      ||g||: fp32 squares summed in fp32 within a slab (fixed order), the slabs' sums added in double, square root in double,
 *      rounded once to fp32.
 *      skip_flag (optional, the range guard's device int): nothing is applied while it is up, and the call itself raises it
 *      when a tensor's gradient norm is not finite (a NaN / Inf born in the backward pass) - no tensor is then updated. */
int bdetr_sgd_slab_elems(void);
int bdetr_sgd_nesterov_clipnorm(const uint64_t* ptrs, const int64_t* sizes, int ntensors,
                                const int64_t* slab_tensor, const int64_t* slab_first, int nslabs,
                                float* partial, float* norms, const float* lr, float momentum,
                                float clipnorm, float grad_scale, int* skip_flag, void* stream);

/*      AdamW = Keras Adam (non-amsgrad) + TFA's decoupled weight decay + Keras' per-tensor clipnorm (notebook cell 26:
 *      tfa.optimizers.AdamW).  Same conventions and the same slab table / partial / norms workspaces as the SGD call; `ptrs` holds
 *      ntensors x {w,g,m,v}.  Per element, every operation rounded to fp32 on its own, in this order (no fused multiply-add):
 *          scale = grad_scale ; if clipnorm > 0 and ||g|| * |grad_scale| > clipnorm: scale *= clipnorm / (||g|| * |grad_scale|)
 *          g' = g * scale
 *          w1 = decays[t] ? w - wd_t * w : w                        (decoupled: not multiplied by the learning rate)
 *          m' = beta1 * m + one_minus_beta1 * g'
 *          v' = beta2 * v + one_minus_beta2 * (g' * g')
 *          w' = w1 - (lr_t * m') / (sqrt(v') + epsilon)             (IEEE sqrt and division)
 *      step_scalars: device float[2] = {lr_t, wd_t}, read by the kernel (a captured graph sees this step's values); the caller folds
 *      the bias correction into lr_t in double: lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t).  one_minus_beta1/2 are arguments of
 *      their own because 1.0f - 0.999f is 9.9998713e-4 in fp32 (1.3e-5 off, relative): compute them in double.  decays: ntensors bytes on the device,
 *      non-zero = the tensor takes weight decay (NULL: all do).  skip_flag as above: while it is up w, m and v are all left
 *      untouched, and a non-finite gradient norm raises it. */
int bdetr_adamw_clipnorm(const uint64_t* ptrs, const int64_t* sizes, int ntensors,
                         const int64_t* slab_tensor, const int64_t* slab_first, int nslabs,
                         float* partial, float* norms, const float* step_scalars, const uint8_t* decays,
                         float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float epsilon,
                         float clipnorm, float grad_scale, int* skip_flag, void* stream);

/* ------------------------------------------------------------------------
 * K14  detection metric: COCO-style box AP without a host hop per batch (csrc/detmetric.hip; evaluation.py accumulates).
 *   The matching of K14-K17 and K22 is ONE kernel, csrc/coco_match.h: the five entries differ in where an IoU comes from and in
 *   whether the ignore class (K16) is compiled in, nothing else.  (K30 and K31 are the same kernel again, with the attribute F1
 *   gate as one more compile-time parameter.)
 *   The reference has no evaluation at all; the rule restated here is pycocotools' COCOeval.evaluateImg for the no-crowd,
 *   all-areas case with one max_dets.
 *   bdetr_det_postprocess : cat_pred [B,N,C] probabilities -> label[B,N] = first-max argmax over classes 2 .. C-1 (0 = <PAD>, "no
 *                           object", and 1 = <OOV> are never a detection's label), score[B,N] = that class's probability (copied).
 *                           Every query is a detection (DETR's convention).
 *   bdetr_det_match       : one workgroup per image, one wave per threshold.  box_pred [B,N,4], gt_box [B,M,4]: normalised COCO
 *                           [x,y,w,h]; gt_label int32 [B,M]; num_objects int32 [B].  thresholds: T doubles in HOST memory, read
 *                           during the call (they travel as kernel arguments).
 *       order      : detections in descending score, equal scores in ascending query index (stable);  order[B,N] int32
 *       truncation : a detection whose rank among the detections of its own class in its image is >= max_dets matches nothing
 *                    (keep bit 0)
 *       IoU        : fp64 from the fp32 inputs, every operation rounded on its own (no fused multiply-add):
 *                    w, h = max(w, 0), max(h, 0); corners x, x + w, y, y + h; iw, ih = max(min(hi) - max(lo), 0);
 *                    inter = iw * ih; union = (w_d * h_d + w_g * h_g) - inter; iou = union > 0 ? inter / union : 0
 *       valid gts  : rows m < num_objects[b] whose label is in [2, C)
 *       matching   : per threshold t, walking the kept detections in `order`: among the ground truths of the detection's label
 *                    not yet matched at t with iou >= min(thresholds[t], 1 - 1e-10), the one with the largest IoU; on equal IoU
 *                    the LARGER ground-truth index (COCOeval's `if ious < iou: continue` scan); a matched ground truth is
 *                    consumed for that t only
 *       tp_bits    : uint16 [B,N] in query order: bit t = true positive at threshold t, bit 15 = keep
 *       matched_gt : int32 [B,T,N], the matched ground-truth row or -1
 *       gt_count   : int32 [C], caller-owned and caller-zeroed: the valid ground truths of every image are ADDED per class
 *                    (integer atomics: the running total over an evaluation)
 *   Limits: N <= 1024, M <= 1024, 3 <= C <= 65536, 1 <= T <= 15, max_dets >= 1; anything else returns -1 (bdetr_last_error)
 *   without a launch.  Inputs are expected to be free of NaN.
 * ---------------------------------------------------------------------- */
int bdetr_det_postprocess(const float* cat_pred, int B, int N, int C, float* score, int32_t* label, void* stream);
int bdetr_det_match(const float* score, const int32_t* label, const float* box_pred, const int32_t* gt_label, const float* gt_box,
                    const int32_t* num_objects, const double* thresholds, int B, int N, int M, int C, int T, int max_dets,
                    int32_t* order, uint16_t* tp_bits, int32_t* matched_gt, int32_t* gt_count, void* stream);

/* ------------------------------------------------------------------------
 * K15  mask metric: COCO-style mask AP (pycocotools' iouType="segm") on packed bitmasks (csrc/maskmetric.hip; evaluation.py
 *   accumulates as for K14).  Masks are compared on the grid they are given on (the panoptic head's 23 x 23 = 529 pixels).
 *   bdetr_mask_binarize : x [rows,P] fp32 -> bits [rows,W] uint64, W = ceil(P / 64): bit (p mod 64) of word (p div 64) is set when
 *                         x[p] > threshold (NaN: not set); the bits of the last word at and past P are zero; area[rows] int32 =
 *                         the row's number of set bits.  One wave per row: the wave's 64-bit ballot of the predicate IS the word.
 *                         Mask logits are cut at 0 (sigmoid > 0.5 without the exponential), [0,1] targets at 0.5.
 *   bdetr_mask_match    : bdetr_det_match (the same kernel, csrc/coco_match.h) with another IoU source.  det_bits [B,N,W], det_area [B,N], gt_bits [B,M,W], gt_area [B,M]
 *                         as bdetr_mask_binarize leaves them, in place of the boxes; score / label / gt_label / num_objects /
 *                         thresholds and the outputs order, tp_bits, matched_gt, gt_count exactly as in K14: the same ranking,
 *                         truncation, valid ground truths and matching rule (on equal IoU the LARGER ground-truth index).
 *       IoU        : inter = sum over w of popcount(d[w] & g[w]);  union = area_d + area_g - inter, in integers;
 *                    iou = union > 0 ? (double)inter / (double)union : 0.  IEEE fp64 division of exact integers: equal rationals
 *                    (2/4 and 3/6) are equal doubles, and an IoU of exactly 1/2 meets the threshold 0.5.
 *   Limits: those of K14, W >= 1, and the image's staging must fit the default 64 KiB of dynamic LDS:
 *   20 Np + 8 Mp + roundup8(Np) + 8 W (Np + Mp) bytes with Np, Mp = N, M rounded up to 4 (17.3 KiB at N = M = 100, W = 9).
 *   Anything else returns -1 (bdetr_last_error names the limit) without a launch.
 * ---------------------------------------------------------------------- */
int bdetr_mask_binarize(const float* x, int64_t rows, int P, float threshold, uint64_t* bits, int32_t* area, void* stream);
int bdetr_mask_match(const float* score, const int32_t* label, const uint64_t* det_bits, const int32_t* det_area,
                     const int32_t* gt_label, const uint64_t* gt_bits, const int32_t* gt_area, const int32_t* num_objects,
                     const double* thresholds, int B, int N, int M, int W, int C, int T, int max_dets,
                     int32_t* order, uint16_t* tp_bits, int32_t* matched_gt, int32_t* gt_count, void* stream);

/* ------------------------------------------------------------------------
 * K16  detection metric, the full COCO protocol: K14's bdetr_det_match with crowd regions, area ranges and the class rank that
 *   several max_dets need (csrc/detmetric.hip; evaluation.py's CocoEvaluator accumulates).  The rule restated is pycocotools'
 *   COCOeval.evaluateImg.  bdetr_det_match itself is unchanged.  Grid (B, A): one workgroup per image and area range, one wave
 *   per threshold; every workgroup ranks its image again.
 *   Inputs beyond K14, all in HBM: gt_crowd uint8 [B,M] (0 / 1); gt_area float [B,M] in pixels or NULL; image_hw int32 [B,2]
 *   (original height, width); area_ranges double [A,2] (lo, hi).  thresholds stay in HOST memory.
 *       areas      : scale_b = (double)H_b * (double)W_b.  Detection: (w * h) * scale_b in fp64 on the clamped extents.  Ground
 *                    truth: (double)gt_area when given, otherwise the same formula on its box.
 *       ignore     : a valid ground truth is IGNORED in range a when it is crowd or its area is < lo_a or > hi_a (both bounds
 *                    inclusive: an area of exactly 32^2 is small and medium)
 *       crowd IoU  : inter / (w_d * h_d) (normalised), 0 when that is 0; every other IoU is K14's, operation for operation
 *       matching   : ranking, truncation (at max_dets, the LARGEST of the host's max_dets) and ties as K14.  Per range a and
 *                    threshold t, walking the kept detections in `order`: a non-crowd ground truth matched at (a,t) is
 *                    unavailable, a crowd ground truth is always available.  The detection takes the available NON-IGNORED
 *                    ground truth of its label with the largest IoU >= min(thresholds[t], 1 - 1e-10) (equal IoU: the larger
 *                    row); only if there is none, the available IGNORED one with the largest IoU >= the same bound (same tie
 *                    rule).  This is COCOeval's sort-by-ignore plus `break`.
 *       order      : int32 [B,N] as K14
 *       class_rank : int32 [B,N] in query order: the number of detections of the same label ranked before this one
 *       tp_bits    : uint16 [A,B,N]: bit t = matched to a non-ignored ground truth at (a,t); bit 15 = keep
 *       ig_bits    : uint16 [A,B,N]: bit t = the detection is ignored at (a,t): matched to an ignored ground truth, or unmatched
 *                    with its own area outside range a.  tp and ig are mutually exclusive.
 *       matched_gt : int32 [A,B,T,N], the matched ground-truth row or -1
 *       gt_count   : int32 [A,C], caller-owned and caller-zeroed: the NON-IGNORED valid ground truths are added per range and class
 *   Limits: those of K14, 1 <= A <= 4, B <= 65535; anything else returns -1 (bdetr_last_error) without a launch.
 *
 * K17  mask metric, the full COCO protocol: K15's bdetr_mask_match extended as K16 extends K14 (csrc/maskmetric.hip).
 *   det_pop / gt_pop int32 are the pixel counts bdetr_mask_binarize leaves (K15's det_area / gt_area); gt_area float [B,M] in
 *   pixels or NULL is the annotation's area; P is the masks' pixel count (W = ceil(P / 64) words per mask).
 *       areas      : detection (double)popcount * scale_b / (double)P; ground truth gt_area when given, else the same on gt_pop
 *       crowd IoU  : (double)inter / (double)popcount_det, 0 when that is 0; every other IoU is K15's
 *   Everything else as K16.  Limits: those of K16, P >= 1, and 24 Np + 8 Mp + roundup8(Np + Mp) + 8 W (Np + Mp) bytes of LDS
 *   within the default 64 KiB.
 * ---------------------------------------------------------------------- */
int bdetr_det_match_coco(const float* score, const int32_t* label, const float* box_pred, const int32_t* gt_label, const float* gt_box,
                         const uint8_t* gt_crowd, const float* gt_area, const int32_t* num_objects, const int32_t* image_hw,
                         const double* area_ranges, const double* thresholds, int B, int N, int M, int C, int T, int A, int max_dets,
                         int32_t* order, int32_t* class_rank, uint16_t* tp_bits, uint16_t* ig_bits, int32_t* matched_gt,
                         int32_t* gt_count, void* stream);
int bdetr_mask_match_coco(const float* score, const int32_t* label, const uint64_t* det_bits, const int32_t* det_pop,
                          const int32_t* gt_label, const uint64_t* gt_bits, const int32_t* gt_pop, const uint8_t* gt_crowd,
                          const float* gt_area, const int32_t* num_objects, const int32_t* image_hw, const double* area_ranges,
                          const double* thresholds, int B, int N, int M, int P, int C, int T, int A, int max_dets,
                          int32_t* order, int32_t* class_rank, uint16_t* tp_bits, uint16_t* ig_bits, int32_t* matched_gt,
                          int32_t* gt_count, void* stream);

/* ------------------------------------------------------------------------
 * K18  mask targets: COCO segmentations (polygons, RLE) -> the mask head's float grid targets (csrc/maskraster.hip; the host
 *   side is pipeline.pad_annotations(with_masks=True) / pipeline.mask_targets).  One workgroup per object, o = b M + m.
 *   Inputs, all int32 in HBM:
 *       kind      [B,M]     0 = none (padding, or an annotation without a segmentation), 1 = polygon, 2 = RLE
 *       hw        [B,M,2]   the source image's (h, w) of the object
 *       item_off  [B M + 1] object o owns items[item_off[o] : item_off[o+1]]
 *       items     [n_items] polygon: R, then the ring offsets e[0..R] counted in vertices (e[0] = 0, e[R] = V), then V vertices
 *                           (x, y) snapped to 1/256 pixel (q = rint(256 v), round half to even), 2 + R + 2 V items in all;
 *                           RLE: (start, length) of every one-run in COCO's column-major pixel order (idx = x h + y), ascending
 *                           and disjoint (the host's prefix sum of the counts)
 *       placement [B,6]     (H, W, new_h, new_w, off_h, off_w): the source stretched to new_h x new_w at (off_h, off_w) of an
 *                           H x W canvas; (1, 1, 1, 1, 0, 0) is "the whole canvas"
 *   Source mask.  Pixel (x, y) has the centre (256 x + 128, 256 y + 128).  A ring's edge with endpoints lo, hi (lo.y < hi.y) crosses
 *   the pixel's row when lo.y <= cy < hi.y (horizontal edges never do) and the crossing counts for the pixel when
 *   (cy - lo.y) (hi.x - lo.x) <= (cx - lo.x) (hi.y - lo.y) in int64; the pixel is inside the ring when the count is odd (even-odd;
 *   left and top boundaries inclusive, right and bottom exclusive); the mask is the OR over the rings; rings of fewer than 3
 *   vertices contribute nothing; vertices outside the image are legal.  RLE: the one-runs.
 *   Outputs: masks float [B,M,G,G], masks[i,j] = (float)((double)N[i,j] / (double)(H h W w)) with the int64 numerator
 *       N[i,j] = sum over set pixels of OY(y,i) OX(x,j),
 *       OY(y,i) = max(0, min(PY0 + G new_h, (i+1) H h) - max(PY0, i H h)),  PY0 = G (h off_h + y new_h),  OX likewise
 *   - the exact share of grid cell (i,j) the placed mask covers; area int32 [B,M] = the source mask's set pixels.  N is summed in
 *   LDS with 64-bit integer adds (no float atomics): two calls give the same bits.  Objects of kind 0 get zeros and area 0.
 *   Limits: 1 <= G <= 32, B M <= 2^24, n_items < 2^31: anything else returns -1 (bdetr_last_error) without a launch.  Per object
 *   1 <= h, w, H, W <= 4096, new >= 1, off >= 0, off + new <= canvas, offsets monotone and inside the buffer, coordinates within
 *   +-2^23: the kernel cannot report, so an object that breaks one of these gets zeros (coordinates are clamped, runs are clipped
 *   to the image) and never an out-of-range access; kernels.mask_targets checks all of them on the host before the launch.
 * ---------------------------------------------------------------------- */
int bdetr_mask_targets(const int32_t* items, int64_t n_items, const int32_t* item_off, const int32_t* kind, const int32_t* hw,
                       const int32_t* placement, int B, int M, int G, float* masks, int32_t* area, void* stream);

/* ------------------------------------------------------------------------
 * K19-K22  mask AP at image resolution (csrc/maskimage.hip; evaluation.CocoImageMaskEvaluator chains them, once per batch, and
 *   reads nothing back).  Additions to ABI 8: nothing that existed changed.
 *   Layout shared by all four.  For a batch Hm = max height, Wm = ceil(max width / 64).  A mask is uint64 [Hm, Wm], row-major at
 *   image resolution: pixel (x, y) of image b is bit (x mod 64) of word [y, x div 64]; the bits at x >= w_b and all words of the
 *   rows y >= h_b are zero.  K19 and K20 WRITE those zeros; no caller's memset is relied on.  1 <= Hm <= 4096, 1 <= Wm <= 64.
 *
 * K19  bdetr_mask_upsample_bits: logits float [B,N,G,G], image_hw int32 [B,2] (h_b, w_b; clamped to [0, Hm] x [0, 64 Wm])
 *   -> bits [B,N,Hm,Wm], pop int32 [B,N] (the set bits: an integer sum).  Bilinear with half-pixel centres, as
 *   torch.nn.functional.interpolate(mode="bilinear", align_corners=False) away from zero, but stated so that it can be reproduced
 *   bit for bit.  Along an axis with n target pixels, for the target pixel p:
 *       num = (2 p + 1) G - n;  D = 2 n;  i0 = floor(num / D) (floor division: -1 for a negative num);  r = num - i0 D;
 *       ia = max(i0, 0);  ib = min(i0 + 1, G - 1);  t = (double)r / (double)D
 *   and the value, in fp64 with every operation rounded on its own (no FMA: csrc/mask_upsample.h switches contraction off):
 *       top = (1 - tx) L[ia_y, ia_x] + tx L[ia_y, ib_x];  bot = the same on row ib_y;  v = (1 - ty) top + ty bot
 *   The bit is set when v > 0 (NaN: not set; an infinite logit next to a zero weight gives NaN, by IEEE).  One wave ballot of the
 *   predicate over 64 consecutive x is the output word.  At h = w = G the rule returns finite logits exactly.
 *   Limits: B N <= 2^24, 1 <= G <= 32; anything else returns -1 (bdetr_last_error) without a launch.
 *
 * K20  bdetr_mask_source_bits: K18's segments pack (items, item_off, kind, hw - see K18) -> bits [B,M,Hm,Wm], pop int32 [B,M].
 *   The mask is K18's SOURCE MASK by the rule stated there, from the same code (csrc/mask_scan.h) (vertices snapped to 1/256 pixel, even-odd fill sampled at pixel
 *   centres, rings ORed, RLE one-runs exact); nothing is placed and no coverage is computed.  pop = the set bits = K18's area.
 *   Objects of kind 0 get zeros and pop 0.  Limits: K18's (B M <= 2^24, n_items < 2^31), else -1 without a launch; per object
 *   K18's rules plus h <= Hm and ceil(w / 64) <= Wm: the kernel cannot report, so an object that breaks one of them gets zeros
 *   (coordinates are clamped, runs are clipped to the image) and never an out-of-range access.
 *
 * K21  bdetr_mask_inter: det_bits [B,N,Hm,Wm], gt_bits [B,M,Hm,Wm], num_objects int32 [B] -> inter int32 [B,N,M]:
 *       inter[b,n,m] = sum over the Hm Wm words of popcount(d[w] & g[w]) for m < min(max(num_objects[b], 0), M), else 0.
 *   The entry zeroes inter itself and the waves add into it with integer atomics only: two calls give the same bits.  A
 *   workgroup keeps 8 detections x 8 ground truths of counters in registers while its share of the words streams past (16-byte
 *   loads when Hm Wm is even and both bases are 16-byte aligned, else 8-byte loads); tiles at or past num_objects leave at once.
 *   Limits: B <= 65535, N, M <= 1024.
 *
 * K22  bdetr_mask_match_coco_inter: K17's rule (the same kernel, csrc/coco_match.h) with the IoU source replaced.  In place of det_bits /
 *   gt_bits and the scalar P it takes inter int32 [B,N,M] (K21), det_pop / gt_pop (K19 / K20) and pix int32 [B], the number of
 *   pixels a mask of image b has (image mode: h_b w_b; >= 1):
 *       IoU        : union = det_pop + gt_pop - inter, in integers; iou = union > 0 ? (double)inter / (double)union : 0
 *       crowd IoU  : (double)inter / (double)det_pop, 0 when that is 0
 *       areas      : (double)pop * scale_b / (double)pix[b], scale_b = (double)H_b (double)W_b from image_hw; ground truth:
 *                    gt_area when given
 *   Everything else - ranking, truncation, ignore, matching, ties, every output - as K17 / K16.  With inter from the grid's bits
 *   and pix = P it gives bdetr_mask_match_coco's outputs bit for bit.  The image's inter is staged in LDS when
 *   24 Np + 8 Mp + roundup8(Np + Mp) + 4 N M bytes fit the default 64 KiB (N = M = 100 does: 42.4 KiB), otherwise it is read from
 *   memory.  Limits: those of K17 without P and W; anything else returns -1 (bdetr_last_error) without a launch.
 * ---------------------------------------------------------------------- */
int bdetr_mask_upsample_bits(const float* logits, const int32_t* image_hw, int B, int N, int G, int Hm, int Wm, uint64_t* bits,
                             int32_t* pop, void* stream);
int bdetr_mask_source_bits(const int32_t* items, int64_t n_items, const int32_t* item_off, const int32_t* kind, const int32_t* hw,
                           int B, int M, int Hm, int Wm, uint64_t* bits, int32_t* pop, void* stream);
int bdetr_mask_inter(const uint64_t* det_bits, const uint64_t* gt_bits, const int32_t* num_objects, int B, int N, int M, int Hm, int Wm,
                     int32_t* inter, void* stream);
int bdetr_mask_match_coco_inter(const float* score, const int32_t* label, const int32_t* inter, const int32_t* det_pop,
                                const int32_t* gt_label, const int32_t* gt_pop, const uint8_t* gt_crowd, const float* gt_area,
                                const int32_t* num_objects, const int32_t* image_hw, const int32_t* pix, const double* area_ranges,
                                const double* thresholds, int B, int N, int M, int C, int T, int A, int max_dets, int32_t* order,
                                int32_t* class_rank, uint16_t* tp_bits, uint16_t* ig_bits, int32_t* matched_gt, int32_t* gt_count,
                                void* stream);

/* ------------------------------------------------------------------------
 * K23-K26  panoptic merge and panoptic quality at image resolution (csrc/panopticmerge.hip; evaluation.PanopticEvaluator chains
 *   K20, K25, K14's postprocess, K23, K24, K21 and K26 once per batch and reads nothing back).  Additions to ABI 8: nothing that
 *   existed changed.  Every mask uses the layout of K19-K22: uint64 [Hm, Wm], pixel (x, y) is bit (x mod 64) of word [y, x div 64],
 *   bits outside the image are zero and are WRITTEN as zero by K24 and K25.  1 <= Hm <= 4096, 1 <= Wm <= 64, B <= 65535,
 *   N <= 1024, M <= 1024, 3 <= C <= 65536, 1 <= G <= 32; anything else returns -1 (bdetr_last_error) without a launch.  No kernel
 *   reads or writes out of range, whatever its inputs hold (sizes are clamped, ids outside [0, N) count as "not kept").
 *
 * K23  bdetr_panoptic_select: score float [B,N], label int32 [B,N] (bdetr_det_postprocess), is_stuff uint8 [C] or NULL,
 *   0 <= threshold < 1 -> seg_of int32 [B,N]: which queries become segments.
 *       seg_of[n] = -1 when !(score[n] > threshold): a score equal to the threshold and a NaN score are dropped;
 *       otherwise, for a label in [0, C) with is_stuff[label] != 0, the LOWEST kept query index of that image with the same
 *       label (DETR's merging of same-class stuff: the kept queries of a stuff class are one segment); otherwise n itself.
 *   Above threshold 0.5 a kept query's class is also its argmax over ALL classes, "no object" included (the probabilities sum to
 *   1, so nothing else can reach 0.5); below 0.5 that is not guaranteed and a kept query can be one that DETR's own
 *   post-processing, which takes the argmax with "no object" first, would have dropped.
 *
 * K24  bdetr_panoptic_merge: logits float [B,N,G,G], seg_of int32 [B,N], image_hw int32 [B,2] (clamped as in K19)
 *   -> ids int16 [B,Hm,64 Wm] (16-byte aligned), bits uint64 [B,N,Hm,Wm] (may be NULL: not written), pop int32 [B,N].
 *   A query is KEPT when seg_of[n] is in [0, N).  For every pixel inside the image every kept query's value v is K19's v, by the
 *   same axis rule and the same three fp64 lines - both kernels call csrc/mask_upsample.h - (no FMA), bit for bit.
 *       winner : the kept query with the largest v among those with v > 0; on an exact tie the LOWEST query index; NaN never wins
 *       ids    : seg_of[winner]; -1 when no kept query has v > 0, and -1 outside the image (x >= w_b or y >= h_b)
 *       bits   : bits[b,s] = the pixels with id s - the masks of one image are pairwise disjoint; rows of queries that are no
 *                segment id are written as zeros
 *       pop    : the set bits of bits[b,s] (an integer sum; the entry zeroes it, the waves add): two calls give the same bits
 *   One wave ballot per 64 consecutive x gives one word, as in K19.  The kept queries are compacted once per workgroup, so a
 *   query that is not kept costs nothing per pixel; their logits are read through the caches and are not staged in LDS (100
 *   kept queries at G = 23 are 211 KB).
 *   Stated difference from DETR's PostProcessPanoptic: a pixel that no kept query claims with a positive logit stays void (the
 *   project's cut at 0, as in K19; DETR takes a softmax argmax over the kept queries and has no void), and small segments are
 *   dropped at matching time (min_area, K26) instead of re-running the argmax without them.
 *
 * K25  bdetr_panoptic_gt_exclusive: K20's gt_bits [B,M,Hm,Wm] IN PLACE -> the ground truth as a panoptic map; gt_label int32
 *   [B,M], num_objects int32 [B], C.  Rows with m >= num_objects[b] or a label outside [2, C) are zeroed: they are no segments
 *   and their pixels are void.  Among the remaining rows a pixel belongs to the lowest row that covers it:
 *       out[m] = in[m] & ~(in[0] | ... | in[m-1])   over segment rows only
 *   gt_pop int32 [B,M] is rewritten with the exclusive counts (integer adds).  Purely elementwise per word.
 *
 * bdetr_mask_inter (K21) is reused unchanged on the two disjoint sets: inter int32 [B,N,M].
 *
 * K26  bdetr_panoptic_match: panopticapi's pq_compute_single_core in integers, one workgroup per image.  inter int32 [B,N,M],
 *   pred_pop int32 [B,N], pred_label int32 [B,N], seg_of int32 [B,N], gt_pop int32 [B,M], gt_label int32 [B,M], gt_crowd uint8
 *   [B,M] or NULL, num_objects int32 [B], min_area >= 0.
 *       predicted segment : seg_of[n] == n and pred_pop[n] >= max(min_area, 1)
 *       gt segment        : m < num_objects[b], label in [2, C) (what K25 kept) and gt_pop[m] >= 1
 *       void_n            : pred_pop[n] - sum over m of inter[n,m]
 *       match (n, m)      : both are segments, m is not crowd, the labels are equal, and with
 *                           union = pred_pop[n] + gt_pop[m] - inter[n,m] - void_n:   2 inter[n,m] > union
 *                           - the integer form of IoU > 0.5.  On disjoint maps at most one m per n and one n per m can satisfy
 *                           it, so no ordering is involved (on other inputs the lowest index is taken)
 *       FN                : an unmatched non-crowd ground-truth segment
 *       FP                : an unmatched predicted segment, unless 2 (void_n + sum over the crowd segments m of n's label of
 *                           inter[n,m]) > pred_pop[n]: then it is excused
 *   Outputs, all int32: gt_state [B,M] (matched n >= 0; -1 FN; -2 crowd; -3 not a segment), pred_state [B,N] (matched m >= 0;
 *   -1 FP; -2 excused; -3 not a segment), match_inter [B,M] and match_union [B,M] (0 unless matched).
 *   The two differences from panopticapi: the crowd sum runs over ALL crowd segments of the class (identical whenever an image
 *   has at most one per class, as COCO panoptic files do), and a predicted segment below min_area is no segment at all - neither
 *   FP nor matchable - where DETR removes it before the maps are compared.
 * ---------------------------------------------------------------------- */
int bdetr_panoptic_select(const float* score, const int32_t* label, const uint8_t* is_stuff, int B, int N, int C, float threshold,
                          int32_t* seg_of, void* stream);
int bdetr_panoptic_merge(const float* logits, const int32_t* seg_of, const int32_t* image_hw, int B, int N, int G, int Hm, int Wm,
                         int16_t* ids, uint64_t* bits, int32_t* pop, void* stream);
int bdetr_panoptic_gt_exclusive(uint64_t* gt_bits, const int32_t* gt_label, const int32_t* num_objects, int B, int M, int C, int Hm, int Wm,
                                int32_t* gt_pop, void* stream);
int bdetr_panoptic_match(const int32_t* inter, const int32_t* pred_pop, const int32_t* pred_label, const int32_t* seg_of,
                         const int32_t* gt_pop, const int32_t* gt_label, const uint8_t* gt_crowd, const int32_t* num_objects, int B, int N,
                         int M, int C, int min_area, int32_t* gt_state, int32_t* pred_state, int32_t* match_inter, int32_t* match_union,
                         void* stream);

/* ------------------------------------------------------------------------
 * K27-K28  COCO run-length encoding of bitmasks, for result files (csrc/maskrle.hip; kernels.mask_rle_encode chains K27, a prefix
 *   sum on the device and K28; evaluation.CocoResults is the user).  Additions to ABI 8: nothing that existed changed.
 *   Input of both: bits uint64 [B,N,Hm,Wm] in the layout of K19-K22, exactly as bdetr_mask_upsample_bits (K19) and
 *   bdetr_panoptic_merge (K24) write it - pixel (x, y) of image b is bit (x mod 64) of word [y, x div 64] -; image_hw int32 [B,2]
 *   (h_b, w_b; clamped to [0, Hm] x [0, 64 Wm] as in K19); keep uint8 [B,N] or NULL (NULL: every mask is kept; a mask with keep == 0
 *   produces nothing).  Only the pixels with y < h_b and x < w_b are looked at: the kernels do not rely on the zero padding.
 *   Rule (COCO's rleEncode), in integers.  The h w pixels of a mask are taken in column-major order, p = x h + y.  `counts` holds
 *   the lengths of the alternating runs of 0 and 1, starting with a run of 0 - of length 0 when pixel p = 0 is set -, and the last
 *   run closes at h w.  With T = the number of p in [0, h w) whose pixel differs from pixel p - 1 (pixel -1 counts as 0) and
 *   pos[0] < ... < pos[T-1] those p:
 *       counts has T + 1 entries;  counts[i] = pos[i] - pos[i-1] with pos[-1] = 0 and pos[T] = h w;  they sum to h w;
 *       an all-zero mask is [h w], an all-one mask [0, h w].  A run is at most 2^24: int32 holds it.
 *
 * K27  bdetr_mask_rle_count -> n_counts int32 [B,N]: T + 1 for a kept mask, 0 otherwise.  Bit-parallel: the pixel before (x, y) is
 *   (x, y - 1) for y >= 1, so 64 columns of row y give popcount((row[y] ^ row[y-1]) & columns x < w); for y = 0 it is
 *   (x - 1, h - 1): row h - 1 moved up by one column (bit x takes bit x - 1, the carry crosses the word boundary, column 0 takes
 *   0).  One workgroup per mask; the rows 1 .. h - 1 stream from memory once (16-byte loads when Wm is even and the base is 16-byte
 *   aligned, else 8-byte loads), the row above comes through the caches; integer adds only.
 *
 * K28  bdetr_mask_rle_encode: the same operands plus offset int64 [B N + 1], the exclusive prefix sum of K27's n_counts, and
 *   total, the number of int32 the buffer `counts` holds (>= offset[B N]; counts may be NULL when total = 0, and nothing is launched
 *   then).  Mask o's run lengths go, in order, to counts[offset[o] : offset[o+1]].  One workgroup per mask; a wave takes a word
 *   column, loads 64 rows of it and transposes the 64 x 64 bits over its lanes, so that lane l holds 64 consecutive pixels of
 *   column 64 wd + l; the transitions are col ^ (col << 1 | carry).  A first walk counts them per column, a workgroup scan turns
 *   the counts into slots, a second walk writes every transition's p to its slot (and h w to slot T), and the differences are
 *   taken in place.  A pure function of the input: no atomics on the output, two calls give the same bits.  Nothing is written
 *   outside a mask's own span, nor outside [0, total), whatever offset holds (a span shorter than T + 1 is filled and the rest
 *   dropped).
 *   Limits of both: B N <= 2^24, 1 <= Hm <= 4096, 1 <= Wm <= 64; anything else returns -1 (bdetr_last_error) without a launch.
 * ---------------------------------------------------------------------- */
int bdetr_mask_rle_count(const uint64_t* bits, const int32_t* image_hw, const uint8_t* keep, int B, int N, int Hm, int Wm,
                         int32_t* n_counts, void* stream);
int bdetr_mask_rle_encode(const uint64_t* bits, const int32_t* image_hw, const uint8_t* keep, const int64_t* offset, int B, int N, int Hm,
                          int Wm, int64_t total, int32_t* counts, void* stream);

/* ------------------------------------------------------------------------
 * K29-K31  attribute-aware detection AP: AP with a joint constraint (csrc/attrmetric.hip; evaluation.AttributeEvaluator and
 *   AttributeMaskEvaluator accumulate).  Additions to ABI 8: nothing that existed changed.  A detection is a true positive only
 *   when its IoU with a ground truth reaches the IoU threshold AND the F1 of its predicted attribute set against that ground
 *   truth's reaches an F1 threshold; the result is averaged over a grid of both.  The rule is modelled on Fashionpedia's evaluation
 *   (COCOeval with an F1 gate, its AP_IoU+F1) and is stated here in this project's own words, as K18 and K19 are: it is NOT claimed
 *   to equal fashionpedia-api bit for bit.
 *
 * K29  bdetr_attr_pack: x float [rows,A] -> bits uint64 [rows,Wa], Wa = ceil(A / 64), and count int32 [rows].  The rows are
 *   attribute probabilities [B N, A] or the multi-hot targets [B M, A] the tokenizer leaves.  Bit (a mod 64) of word (a div 64) is
 *   set when a >= 2 and x[a] >= 0.5f - the reference's decode rule (InverseTokenization), not bdetr_mask_binarize's `>` -; NaN: not
 *   set; indices 0 (<PAD>) and 1 (<OOV>) are never an attribute; the bits at and past A are zero; count = the row's set bits.  One
 *   wave per row: the wave's 64-bit ballot of the predicate IS the word.  Limits: rows >= 1, 3 <= A <= 4096.
 *
 *   F1 of detection d against ground truth m, on K29's words and counts:
 *       tp = sum over w of popcount(d[w] & g[w]);  F1 = (double)(2 tp) / (double)(count_d + count_g): ONE IEEE fp64 division of
 *       exact integers, so equal rationals are equal doubles - 2 * 1 / (2 + 2) meets 0.5 and 2 * 3 / (4 + 4) meets 0.75;
 *       count_d + count_g == 0 (both sets empty): F1 = empty_f1, 0.0 or 1.0 (1.0: two empty sets agree);
 *       the gate at F1 threshold f: F1 >= min(f1_thresholds[f], 1 - 1e-10), the form the IoU test has.
 *
 * K30  bdetr_det_match_attr: K16's bdetr_det_match_coco with the gate (the same kernel, csrc/coco_match.h, with one more
 *   compile-time parameter).  A ground truth is a candidate for a detection at (t, f) only if it passes K16's tests AND the gate -
 *   whether it is ignored, crowd or neither.  Among the candidates nothing changes: non-ignored before ignored, the largest IoU,
 *   the larger row on equal IoU, a crowd is reusable, an unmatched detection with its own area outside the range is ignored.
 *   Every (t, f) pair is matched on its own.  Grid (B, A, F): one workgroup per image, area range and F1 threshold, one wave per
 *   IoU threshold; the attribute words and counts of the image's N detections and M ground truths are staged in LDS beside the
 *   boxes.
 *   Inputs beyond K16: det_attr uint64 [B,N,Wa] / det_count int32 [B,N] and gt_attr uint64 [B,M,Wa] / gt_attr_count int32 [B,M] as
 *   K29 leaves them; f1_thresholds: F doubles in HOST memory, read during the call; empty_f1.
 *       tp_bits, ig_bits : uint16 [F,A,B,N], K16's words per F1 threshold (bit 15 of tp_bits = keep, the same for every f)
 *       matched_gt       : int32 [F,A,B,T,N]
 *       order, class_rank: int32 [B,N] as K16 (they do not depend on f: the workgroups a = 0, f = 0 write them)
 *       gt_count         : int32 [A,C] as K16 (it does not depend on f: only the f = 0 workgroups add to it)
 *   Limits: those of K16, 1 <= F <= 16, 1 <= Wa <= 64, empty_f1 0 or 1, and the image's staging within the default 64 KiB of
 *   dynamic LDS: 36 Np + 20 Mp + roundup8(Np + Mp) + (8 Wa + 4) (Np + Mp) bytes with Np, Mp = N, M rounded up to 4 (14.3 KiB at
 *   N = M = 100, Wa = 5).  Anything else returns -1 (bdetr_last_error names the limit) without a launch.
 *
 * K31  bdetr_mask_match_attr: K17's bdetr_mask_match_coco with the same gate; operands as K17 plus K30's.  Limits: those of K17
 *   and of the gate, and 24 Np + 8 Mp + roundup8(Np + Mp) + 8 W (Np + Mp) + (8 Wa + 4) (Np + Mp) bytes of LDS within 64 KiB.
 *   (Image-resolution masks with the gate are not built: K22's source would take the same gate.)
 * ---------------------------------------------------------------------- */
int bdetr_attr_pack(const float* x, int64_t rows, int A, uint64_t* bits, int32_t* count, void* stream);
int bdetr_det_match_attr(const float* score, const int32_t* label, const float* box_pred, const uint64_t* det_attr,
                         const int32_t* det_count, const int32_t* gt_label, const float* gt_box, const uint64_t* gt_attr,
                         const int32_t* gt_attr_count, const uint8_t* gt_crowd, const float* gt_area, const int32_t* num_objects,
                         const int32_t* image_hw, const double* area_ranges, const double* thresholds, const double* f1_thresholds,
                         double empty_f1, int B, int N, int M, int C, int Wa, int T, int F, int A, int max_dets, int32_t* order,
                         int32_t* class_rank, uint16_t* tp_bits, uint16_t* ig_bits, int32_t* matched_gt, int32_t* gt_count,
                         void* stream);
int bdetr_mask_match_attr(const float* score, const int32_t* label, const uint64_t* det_bits, const int32_t* det_pop,
                          const uint64_t* det_attr, const int32_t* det_count, const int32_t* gt_label, const uint64_t* gt_bits,
                          const int32_t* gt_pop, const uint64_t* gt_attr, const int32_t* gt_attr_count, const uint8_t* gt_crowd,
                          const float* gt_area, const int32_t* num_objects, const int32_t* image_hw, const double* area_ranges,
                          const double* thresholds, const double* f1_thresholds, double empty_f1, int B, int N, int M, int P, int C,
                          int Wa, int T, int F, int A, int max_dets, int32_t* order, int32_t* class_rank, uint16_t* tp_bits,
                          uint16_t* ig_bits, int32_t* matched_gt, int32_t* gt_count, void* stream);

/* ------------------------------------------------------------------------
 * K32-K34  attention masks (csrc/attention.hip; kernels.attention_fwd / attention_bwd / ops.attention_core, mask=).  Additions to
 *   ABI 8: nothing that existed changed; bdetr_attention_fwd / _bwd launch the kernels they launched before, bit for bit.
 *
 *   mask: [B or 1, h or 1, nq or 1, nk], the key axis always full and of unit stride; mask_sb / mask_sh / mask_sq are the ELEMENT
 *   strides of the batch, head and query axes, 0 on a broadcast axis.  The mask is a constant: no gradient is computed for it.
 *   mask_mode selects the rule and the element type:
 *
 * K32  BDETR_ATTN_MASK_MULTIPLY, float mask M - the reference's rule (transformers.py:91-94, softmax THEN mask):
 *        P = softmax(scale Q K^T) over ALL keys;  O = (P * M) V;  lse = the log-sum-exp of the unmasked scaled scores.
 *      M holds any floats (0, negative, above 1); nothing is renormalised.  Backward, with D = rowdot(dO, O):
 *        dP = M * (dO V^T);  dS = P * (dP - D) * scale;  dV = (P * M)^T dO;  dQ = dS K;  dK = dS^T Q.
 *      (dS keeps its unmasked form because sum_k P_k M_k (dO . V_k) = dO . O.)
 *
 * K33  BDETR_ATTN_MASK_EXCLUDE, uint8 mask - this project's own rule, not the reference's: a key whose byte is 0 is excluded, any
 *      other value attends.  An excluded key takes no part in the softmax (its score is -inf); lse runs over the kept keys; the
 *      backward is the ordinary one over the kept keys.  A row with no kept key gives O = 0, lse = -inf and contributes nothing to
 *      dQ, dK, dV.  No NaN appears in any of these cases.
 *
 *   bdetr_attention_masked_fwd / _bwd: the operands of bdetr_attention_fwd / _bwd, then the mask.  Returns -1 before any launch
 *   (bdetr_last_error says why) on a null mask, an unknown mode, a negative stride, a float mask that is not 4-byte aligned, or
 *   when (B-1) sb + (h-1) sh + (nq-1) sq + nk does not fit the address arithmetic (the whole sum an int64 byte offset, one
 *   (image, head) plane (nq-1) sq + nk at most 2^31 - 1 elements).  No atomics: two calls give the same bits.  An all-ones float
 *   mask and an all-nonzero byte mask give the bits of the unmasked entry points.  A key-only mask (mask_sq == 0) runs its own
 *   instantiations, which keep the unmasked kernels' occupancy.
 *
 * K34  bdetr_attention_mask_apply: the same mask against a materialised contiguous [B,h,nq,nk] tensor, for the unfused attention path
 *      (head dimension other than 32).  fill == 0: out = x * M (float mask) or out = m ? x : 0 (byte mask).  fill != 0 (byte mask
 *      only): out = m ? x : BDETR_ATTN_MASK_FILL, a large finite negative put in front of bdetr_softmax_rows_fwd - a row with no
 *      kept key then has a finite (uniform) softmax, which the fill == 0 form zeroes afterwards.  out may be x.
 * ---------------------------------------------------------------------- */
#define BDETR_ATTN_MASK_MULTIPLY 1
#define BDETR_ATTN_MASK_EXCLUDE 2
#define BDETR_ATTN_MASK_FILL (-1.0e30f)
int bdetr_attention_masked_fwd(const float* q, const float* k, const float* v, float* o, float* lse,
                               int B, int h, int nq, int nk, float scale,
                               const void* mask, int64_t mask_sb, int64_t mask_sh, int64_t mask_sq, int mask_mode, void* stream);
int bdetr_attention_masked_bwd(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                               const float* lse, float* dq, float* dk, float* dv, float* dvec_ws,
                               int B, int h, int nq, int nk, float scale,
                               const void* mask, int64_t mask_sb, int64_t mask_sh, int64_t mask_sq, int mask_mode, void* stream);
int bdetr_attention_mask_apply(const float* x, float* out, int B, int h, int nq, int nk,
                               const void* mask, int64_t mask_sb, int64_t mask_sh, int64_t mask_sq, int mask_mode, int fill, void* stream);

/* ------------------------------------------------------------------------
 * K35  bdetr_token_key_mask (csrc/tokenmask.hip; kernels.token_key_mask; the batch key `valid_region` of DETR.call /
 *   BoostedDETR.call).  An addition to ABI 8.  Valid image regions -> the key mask of K33 over the tokens of an r x c feature grid.
 *
 *   region: int32 [B,4] in HBM, rows (top, left, height, width) in pixels of an h x w image: rows [top, top + height) and columns
 *   [left, left + width) hold picture, the rest is padding.  mask: uint8 [B, r*c], token (i, j) at index i*c + j; 1 = attends.
 *
 *   The rule is this project's own and is stated in integers (int64, no floats, nothing rounded).  Token (i, j) is kept iff its
 *   centre, taken in image pixels, lies in the region:
 *       2 r top  <= (2 i + 1) h < 2 r (top + height)     and     2 c left <= (2 j + 1) w < 2 c (left + width)
 *   i.e. (i + 1/2) h / r in [top, top + height): top and left inclusive, bottom and right exclusive.  This is "nearest" sampling with
 *   half-pixel centres, the convention of K19.  DETR proper interpolates its pixel mask to the feature size with mode="nearest";
 *   equality with that is NOT claimed (its index rule floors i h / r, without the half pixel).
 *
 *   The kernel reads `region` from HBM - one thread per token, one plain byte store each, no atomics, no memset or memcpy - so a
 *   captured step replayed after the region buffer changed makes the mask of the new regions.  Nothing in `region` is validated on
 *   the device: a row with no picture (height or width < 1), or one that covers no token centre, gives an all-zero mask row, which
 *   K33 answers with O = 0, lse = -inf and no NaN.  Returns -1 before the launch (bdetr_last_error says why) on a null pointer,
 *   B outside [1, 65535], h, w, r or c outside [1, 2^20] (every product of the rule then stays below 2^54), or r*c above 2^31 - 257.
 * ---------------------------------------------------------------------- */
int bdetr_token_key_mask(const int32_t* region, int B, int h, int w, int r, int c, uint8_t* mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BDETR_H */

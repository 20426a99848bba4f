/*
 * tfimm_hip.h -- C ABI of libtfimm_hip.so, the MI355X (gfx950) forward-path kernels that
 * stand in for the TensorFlow ops tfimm's model code calls.
 *
 * The reference (martinsbruveris/tensorflow-image-models) has no native layer: every
 * arithmetic op is a tf.* / tf.keras.layers.* call inside Python model code. Each entry
 * point below therefore replaces a *TF op call site* (cited per function, paths relative
 * to the reference checkout) rather than an existing FFI symbol.  INTEGRATION.md shows the
 * ctypes stub a tfimm maintainer would add.
 *
 * Conventions
 *   - plain C: pointers + ints, no C++/torch types.  All pointers are DEVICE pointers
 *     unless a name ends in _host.  The caller owns every buffer.
 *   - activations: bf16 (uint16 storage), NHWC / (rows, channels) row-major.
 *   - weights are pre-packed by the host side (see tfimm/engine/pack.py):
 *       GEMM/conv weights  Wt[N][ldw]  bf16, K contiguous ("B transposed"),
 *       bias / norm params  fp32.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     null stream).  Return value: 0 on success, otherwise a negative TFIMM_E* code or a
 *     positive hipError_t; tfimm_hip_last_error() returns a static message for the last
 *     failure on the calling thread.  Nothing throws or aborts across the boundary.
 */
#ifndef TFIMM_HIP_H
#define TFIMM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: tfimm_tha_desc grew (proj_dev), tfimm_hip_mlp_fused / tfimm_hip_plan_* / tfimm_hip_ref_* added (round 3) */
/* 4: tfimm_gemm_desc grew (a2 ...: a second A operand, the shortcut convolution folded into a block's last GEMM; round 6) */
#define TFIMM_HIP_ABI_VERSION 4

#if defined(__GNUC__)
#define TFIMM_API __attribute__((visibility("default")))
#else
#define TFIMM_API
#endif

#define TFIMM_EINVAL (-1)   /* bad descriptor (shape/alignment/flag)            */
#define TFIMM_EUNSUP (-2)   /* valid request this build has no kernel for       */

/* activation codes (reference tfimm/layers/factory.py:6-13 act_layer_factory) */
enum {
  TFIMM_ACT_NONE = 0,     /* "linear"                                   */
  TFIMM_ACT_RELU = 1,
  TFIMM_ACT_GELU = 2,     /* exact erf GELU (keras gelu approximate=False) */
  TFIMM_ACT_SWISH = 3,    /* x * sigmoid(x)                             */
  TFIMM_ACT_SIGMOID = 4,
  TFIMM_ACT_RELU6 = 5,
  TFIMM_ACT_TANH = 6
};

/* A-operand addressing modes of tfimm_hip_gemm */
enum {
  TFIMM_A_DENSE = 0,      /* A[m][k] = a[m*lda + k]                                   */
  TFIMM_A_CONV = 1,       /* implicit-GEMM gather from NHWC, Cin % 8 == 0             */
  TFIMM_A_CONV_C4 = 2     /* implicit-GEMM gather from NHWC with Cin == 4 (padded RGB) */
};

TFIMM_API int tfimm_hip_abi_version(void);
TFIMM_API const char* tfimm_hip_last_error(void);
/* Fills name[len] with e.g. "gfx950:sramecc+:xnack-" (always terminated, cut to len - 1 characters; name may be NULL, len <= 0
 * leaves it alone); returns the CU count (> 0).  A device that does not exist or cannot be queried: returns the negated
 * hipError_t (< 0), tfimm_hip_last_error() names the failed call and name[] is left as it was. */
TFIMM_API int tfimm_hip_device_info(int device, char* name, int len);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_gemm: out[M][N] = epilogue( A[M][K] . Wt[N][K]^T )            (MFMA, bf16->fp32)
 *
 *   epilogue(v)[m][n] = v + bias[n]                      (bias may be NULL)
 *                       -> act(.)  unless act_after_res
 *                       -> + residual[rm][n]             (residual may be NULL;
 *                                                         rm = res_mod ? m % res_mod : m)
 *                       -> act(.)  if act_after_res
 *   stored to out[om][n], om = remap_in ? (m / remap_in) * remap_out + m % remap_in + remap_off : m,
 *   as bf16 (out_f32 == 0) or fp32.
 *
 * Replaces, in the reference:
 *   tf.keras.layers.Dense                  vit.py:155,169  swin.py:167,197  transformers.py:209-212
 *   Conv2D 1x1 / kxk (+ZeroPadding2D) + BatchNormalization(inference, folded) + Activation
 *                                          resnet.py:220-258,315-330,505-512  efficientnet_blocks.py:18-63
 *   PatchEmbeddings conv                   layers/transformers.py:164-165
 *   residual adds                          vit.py:228,234  resnet.py:289  efficientnet_blocks.py:451
 *
 * mode TFIMM_A_CONV:  m = (b*OH + oy)*OW + ox,  k = (ky*KW + kx)*Cin + ci  (Cin % 8 != 0 takes a slow element-load path),
 *     A[m][k] = x[b][oy*stride - pad_t + ky][ox*stride - pad_l + kx][ci]  (0 outside the image)
 * mode TFIMM_A_CONV_C4: Cin == 4, k = (ky*KWp + kx)*4 + ci with KWp = KW rounded up to even
 *     (the packed weight has zero columns for kx >= KW).
 * a_scale (dense mode only, optional): A[m][k] is multiplied by a_scale[(m / rows_per_image)*K + k]
 *     before the product -- the SqueezeExcite gate  x * sigmoid(...)  of
 *     efficientnet_blocks.py:241-248 folded into the projection conv.
 * ------------------------------------------------------------------------------------- */
typedef struct tfimm_gemm_desc {
  const void* a;          /* bf16 */
  const void* wt;         /* bf16 [N][ldw], zero padded to ldw >= K, ldw % 8 == 0; with a second A operand (a2) K and every one of
                             its taps are zero padded to whole 64-wide k-tiles: ldw >= pad64(K) + taps * pad64(K2), else TFIMM_EINVAL */
  const float* bias;      /* [N] or NULL */
  const void* residual;   /* bf16 [.][ldr] or NULL */
  void* out;              /* bf16 or fp32 [.][ldc] */
  const float* a_scale;   /* fp32 [M/rows_per_image][K] or NULL */
  int32_t M, N, K;
  int32_t lda, ldw, ldr, ldc;
  int32_t out_f32;
  int32_t act, act_after_res;
  int32_t res_mod;
  int32_t remap_in, remap_out, remap_off;
  int32_t mode;
  int32_t B, H, W, Cin, KH, KW, stride, pad_t, pad_l, OH, OW;
  int32_t rows_per_image;
  int32_t tile_hint;      /* 0 = the library's cost model; otherwise a kernel-table index measured by the caller
                             (tfimm/engine/tune.py): 1..6 register-staged tiles, 11..16 one-tile LDS-DMA kernels,
                             21..29 persistent LDS-DMA kernels (28 = 256x256 deep ring, 29 = 256x32).  A hint the
                             problem cannot use (alignment, flavour not built) falls back to the cost model. */
  int32_t stride_w;       /* TFIMM_A_CONV only: horizontal stride if it differs from `stride` (0 = same).
                             Lets a stride-2 RGB stem / patch embedding run on the pixel-PAIR view of a
                             zero-padded 4-channel image ([B][Hp][Wp/2][8], see tfimm_hip_cast_input_pad):
                             vertical stride s, horizontal stride s/2, kernel width ceil(KW/2). */
  int32_t pix_pitch;      /* TFIMM_A_CONV only: elements between consecutive pixels of x if it differs from Cin
                             (0 = Cin).  With `a` pointing at channel c0 of a [B][H][W][C] tensor, Cin = w and
                             pix_pitch = C the convolution reads the channel slice [c0, c0 + w) -- one group of a
                             grouped convolution (resnet.py:229-236); ldc / the `out` pointer place its w output
                             channels the same way. */
  const float* ln_stats;  /* dense mode, no residual: fp32 [M][2] = (mean, rstd) of every row of `a` (tfimm_hip_row_stats).
                             With ln_c1 it folds a LayerNormalization over the K axis INTO this layer
                             (layers/factory.py:42-50 in front of a Dense, vit.py:226-233, swin.py:243-327):
                             out = act(rstd_m * (a . wt^T - mean_m * c1[n]) + bias[n]), where the caller has already
                             multiplied gamma into wt (W' = gamma * W, then rounded to bf16), c1[n] = sum_k W'[k][n] of the
                             ROUNDED weights and bias = beta . W + b.  The normalised tensor is never written. */
  const void* ln_c1;      /* bf16 [N][2][8]: c1[n] as the three-term bf16 split (ca, cb, cc), laid out as the MFMA fragment
                             pair {ca,cb,cc,ca,cb,cc,ca,cb} {cc,0,0,0,0,0,0,0} (tfimm/engine/pack.py: pack_ln_c1) */
  /* ---- ABI v4: a SECOND A operand whose product accumulates into the same output tile (mode TFIMM_A_DENSE or TFIMM_A_CONV for
   *      the first operand -- the 1x1 conv3 of a bottleneck, the 3x3 conv2 of a basic block -- no residual):
   *      out = act( a . wt[:, 0:K]^T + a2' . wt[:, Kp:Kp+K2]^T + bias ),   Kp = K rounded up to 64.
   * It is the shortcut convolution of a residual block folded into the block's last 1x1 convolution (resnet.py:282-290
   * `x = self.conv3(x) ... shortcut = self.downsample(shortcut) ... x += shortcut`, downsample_conv resnet.py:315-330: a 1x1
   * convolution of stride s + BatchNorm): instead of writing the shortcut tensor and reading it back as `residual`, its K2
   * input channels are more k-tiles of the same GEMM (the two folded BatchNorm shifts are added on the host).  a2' is the
   * strided row view of a2: output row m = (b, oy, ox) of an [a2_OH][a2_OW] image reads pixel (b, oy * a2_stride,
   * ox * a2_stride) of the [a2_H][a2_W][lda2] tensor a2 (a2_stride = 1: row m itself).  NULL = no second operand. */
  const void* a2;         /* bf16 [B * a2_H * a2_W][lda2] */
  int32_t K2, lda2;       /* channels of the second operand (multiple of 8) and its pixel pitch in elements */
  int32_t a2_stride, a2_H, a2_W, a2_OH, a2_OW;
  int32_t a2_window;      /* 0 / 1: the 1x1 view above.  w > 1: a w x w window of taps -- output row (b, oy, ox) reads the pixels
                             (b, oy * a2_stride + dy, ox * a2_stride + dx), dy, dx < w, as w * w further operands of K2 channels each
                             (taps in (dy, dx) order, each -- the last one too -- padded to whole 64-wide k-tiles in wt:
                             ldw >= pad64(K) + w * w * pad64(K2)): the average-pool shortcut of
                             ResNet-D, AveragePooling2D(2, 2) + 1x1 convolution (resnet.py:295-312) = a 2x2 / stride-2 convolution whose
                             taps are the 1x1 kernel / 4.  The window must lie inside the image for every output pixel. */
} tfimm_gemm_desc;

TFIMM_API int tfimm_hip_gemm(const tfimm_gemm_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_row_stats: stats[r] = (mean, 1 / sqrt(var + eps)) over the d channels of row r (fp32 two-pass, population
 * variance -- tf.keras.layers.LayerNormalization's statistics), for a LayerNorm that is folded into the following
 * tfimm_hip_gemm (ln_stats / ln_c1).  x: bf16 rows of x_stride elements.
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_row_stats(const void* x, float* stats, int64_t rows, int d, int64_t x_stride, float eps, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_cast_input: float32 / bf16 NHWC image batch -> bf16 NHWC with channels padded
 * to c_out (zeros).  in_dtype: 0 = fp32, 1 = bf16.  Replaces Keras' implicit input cast
 * (model(x) accepts float arrays, tests/models/test_factory.py:47-49).
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_cast_input(const void* in, int in_dtype, void* out, int64_t n_pixels,
                         int c_in, int c_out, void* stream);

/* tfimm_hip_cast_input_pad: as tfimm_hip_cast_input for c_in <= 4 -> 4 stored channels, but writes the
 * image into the interior of a zero border: out[B][H + pad_t + pad_b][W + pad_l + pad_r][4].  This is
 * the ZeroPadding2D / "same" padding in front of a stem convolution (resnet.py:505, layers/conv.py:61)
 * done once while the input is converted, so the convolution itself needs no bounds checks and its
 * operand tiles can be fetched by LDS-DMA. */
TFIMM_API int tfimm_hip_cast_input_pad(const void* in, int in_dtype, void* out, int B, int H, int W, int c_in,
                             int pad_t, int pad_b, int pad_l, int pad_r, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_stem_conv_pool: the ResNet stem in one kernel -- ZeroPadding2D(3) + Conv2D 7x7 stride 2 (BN folded into
 * weights and bias) + ReLU + ZeroPadding2D(1) + MaxPool2D 3x3 stride 2 (resnet.py:505-512, 538-540; forward_features
 * :572-576).  x: the zero-bordered 4-channel image tfimm_hip_cast_input_pad / tfimm_hip_preprocess_input_pad wrote,
 * viewed as pixel pairs [batch][Hp][Wp2][8] bf16 (Wp2 = padded width / 2 <= 116, Hp >= 2 (OH - 1) + 7).
 * wt: [64][ldw] bf16 with k = ky * 32 + (kx / 2) * 8 + (kx % 2) * 4 + c (kx = 7 and c = 3 are zero), the layout of the
 * unfused TFIMM_A_CONV call on the pair view; bias: 64 floats.  OH x OW (OW <= 112): size of the convolution output,
 * which exists only in LDS; out: [batch][PH][PW][64] bf16, PH = (OH - 1) / 2 + 1, PW = (OW - 1) / 2 + 1.
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const void* x;
  const void* wt;
  const float* bias;
  void* out;
  int32_t batch, Hp, Wp2, OH, OW, ldw;
  /* in_dtype 0: x is the padded pair view described above.  1 / 2: x is the caller's own [batch][H][W][3] image in
   * bf16 / float32 and the kernel applies the border (pad_t rows above, pad_l columns left, zeros to Hp x 2 Wp2), the
   * zero 4th channel and the bf16 rounding of tfimm_hip_cast_input_pad itself -- that launch and its 8 bytes per
   * pixel of HBM traffic disappear.  Hp, Wp2 describe the same (virtual) padded geometry in every mode. */
  int32_t in_dtype, H, W, pad_t, pad_l;
} tfimm_stem_desc;

TFIMM_API int tfimm_hip_stem_conv_pool(const tfimm_stem_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_preprocess_input / _pad: the two conversions above for a uint8 image with values in [0, 255], with the
 * model's preprocessing applied on the way: out = bf16(((float)v / 255 - mean[c]) / std[c]) -- the three float32
 * operations of create_preprocessing (models/factory.py:165-167; mean/std: utils/constants.py:3-6, tiled to c_in by
 * the caller as in factory.py:153-163), so the result is bit-identical to preprocessing in float32 on the host
 * followed by tfimm_hip_cast_input.  mean, std: HOST arrays of c_in floats (copied into the launch),
 * c_in <= TFIMM_PREPROCESS_MAX_CHANNELS (<= 4 for _pad); padded channels and the border are 0.
 * ------------------------------------------------------------------------------------- */
#define TFIMM_PREPROCESS_MAX_CHANNELS 8
TFIMM_API int tfimm_hip_preprocess_input(const void* in, void* out, int64_t n_pixels, int c_in, int c_out,
                               const float* mean, const float* std, void* stream);
TFIMM_API int tfimm_hip_preprocess_input_pad(const void* in, void* out, int B, int H, int W, int c_in,
                                   int pad_t, int pad_b, int pad_l, int pad_r,
                                   const float* mean, const float* std, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_preprocess_resize: resize + centre crop + normalise a uint8 batch of ANY source size in one launch, written in
 * exactly the two layouts of tfimm_hip_preprocess_input / _pad (csrc/resize.hip).  It is the evaluation transform in front
 * of create_preprocessing (models/factory.py:128-171) that the reference leaves to the caller: every model config carries
 * `crop_pct` and `interpolation` ("Parameters for inference", e.g. resnet.py ResNetConfig, vit.py ViTConfig) and nothing in
 * the reference reads them.  Geometry is timm's: resize so that the crop window is input_size / crop_pct, centre crop
 * (tfimm/models/factory.py resize_geometry); only the crop window is evaluated.
 *
 * Resampling is tf.image.resize(float32(img), (Rh, Rw), method, antialias=False), half-pixel centres:
 *   bicubic  (4 taps)  Keys kernel A = -0.5 from a 1024-entry table at the rounded fractional offset, taps outside the image
 *                      weigh 0 and the rest are renormalised; vertical pass first, then horizontal; each sum starts at 0.0
 *                      and adds w * x in tap order, multiply and add as separate float32 operations
 *   bilinear (2 taps)  top = tl + (tr - tl) * xf, bottom = bl + (br - bl) * xf, out = top + (bottom - top) * yf
 * then (r / 255 - mean[c]) / std[c] in three float32 operations and one rounding to bf16 (nearest-even): the result is
 * bit-equal to the host restatement (tfimm/models/model.py DeferredInput.numpy).  Downscaling is NOT antialiased --
 * TensorFlow's default, a fixed 4 x 4 or 2 x 2 source pixels per output pixel; PIL-style antialiasing is default off, see
 * tfimm_hip_preprocess_resize_aa below.
 *
 * The tap tables are built on the host and passed in as device arrays; the device computes no tap arithmetic:
 *   tfimm_hip_resize_taps  fills idx_host[n_out][taps] / w_host[n_out][taps] (taps = 2 for method 0 = bilinear, 4 for method
 *                          1 = bicubic) for the output positions [first, first + n_out) of an axis resized from n_in to
 *                          n_resized.  A tap outside the image has weight +0.0 and an index clamped into the image.
 *                          Bilinear: idx = (lo, hi), w = (1 - frac, frac) -- the kernel uses w[1] as the lerp fraction.
 *                          A plain host function: no GPU is needed or touched.
 * The kernel clamps every index it reads from a table to the image, so a bad table cannot read out of bounds.
 * ------------------------------------------------------------------------------------- */
typedef struct tfimm_resize_desc {
  const void* in;          /* uint8 [B][Hs][Ws][c_in] */
  void* out;               /* bf16 (tfimm_hip_ref_preprocess_resize: float32) [B][H + pad_t + pad_b][W + pad_l + pad_r][c_out];
                              channels >= c_in and the border are written as 0 */
  const int32_t* y_idx;    /* [H][taps] source row of every tap of every output row */
  const float* y_w;        /* [H][taps] its weight */
  const int32_t* x_idx;    /* [W][taps] */
  const float* x_w;        /* [W][taps] */
  const float* mean_host;  /* HOST arrays of c_in floats (copied into the launch) */
  const float* std_host;
  int32_t B, Hs, Ws, c_in; /* c_in <= TFIMM_PREPROCESS_MAX_CHANNELS */
  int32_t H, W;            /* the crop window = the model's input size */
  int32_t c_out;           /* >= c_in; 4 (8 bytes per pixel) and 8 (16 bytes) are stored as one vector */
  int32_t pad_t, pad_b, pad_l, pad_r;   /* the zero border of tfimm_hip_preprocess_input_pad; non-zero only with c_out == 4 */
  int32_t taps;            /* 2 = bilinear, 4 = bicubic */
} tfimm_resize_desc;

TFIMM_API int tfimm_hip_resize_taps(int n_in, int n_resized, int first, int n_out, int method, int32_t* idx_host,
                                    float* w_host);
TFIMM_API int tfimm_hip_preprocess_resize(const tfimm_resize_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_preprocess_resize_aa: the same launch with ANTIALIASED resampling (csrc/resize_aa.hip) -- what
 * create_preprocessing(..., resize=True, antialias=True) runs.  Same geometry, same two output layouts (border zeros
 * included), same normalisation and rounding as tfimm_hip_preprocess_resize.
 *
 * Resampling is tf.image.resize(float32(img), (Rh, Rw), method, antialias=True), the ScaleAndTranslate formulation.  No
 * TensorFlow binary stands behind it: the rule below IS the specification, every step a float32 operation of its own.  Per
 * axis, for the output positions o of an axis resized from n_in to n_res:
 *   radius = 2 (bicubic) or 1 (bilinear); inv = f32(n_in) / f32(n_res); ks = max(inv, 1.0f);
 *   T = min(2 * ceil(radius * ks) + 1, n_in)                              the span pitch
 *   s = (f32(o) + 0.5f) * inv;  a = ceil(s - radius * ks - 0.5f), b = floor(s + radius * ks - 0.5f), both clamped to
 *   [0, n_in - 1];  start = a, count = b - a + 1 <= T
 *   w_i = K(|(f32(i) + 0.5f - s) / ks|) for i = a..b;  total = their sum from 0.0f in order;  if |total| >= 1000 * FLT_MIN
 *   every w_i is multiplied by 1.0f / total;  table entries past count are +0.0
 *   K bicubic (Keys, A = -0.5, evaluated directly): x >= 2: 0;  x >= 1: ((-0.5 x + 2.5) x - 4) x + 2;  else ((1.5 x - 2.5) x) x + 1
 *   K bilinear: max(0, 1 - x)
 * The vertical pass runs first into a float32 intermediate, then the horizontal pass; each sum starts at 0.0f and adds w * x
 * in tap order, multiply and add as separate float32 operations; then (r / 255 - mean[c]) / std[c] and one rounding to bf16.
 * An axis that is upscaled uses the same rule with ks = 1 (5 or 3 taps): as in TensorFlow, that is not bit-identical to the
 * antialias=False launch.  An axis of scale 1 has weights (0, 0, 1, 0, 0) exactly.
 *
 *   tfimm_hip_resize_span_taps  returns T (or the invalid-argument code)
 *   tfimm_hip_resize_spans      fills start_host[n_out], count_host[n_out], w_host[n_out][T] for the output positions
 *                               [first, first + n_out); method 0 = bilinear, 1 = bicubic.  A plain host function: no GPU is
 *                               needed or touched.  Refuses first < 0, first + n_out > n_resized, non-positive sizes and
 *                               unknown methods with the invalid-argument code.
 * Supported domain of the launch: y_taps, x_taps <= TFIMM_RESIZE_AA_MAX_TAPS (bicubic down to ~15 x, bilinear to ~31 x),
 * c_in <= TFIMM_PREPROCESS_MAX_CHANNELS; anything else returns the invalid-argument code and launches nothing.  The kernel
 * clamps every start + t to the image, so a bad table cannot read out of bounds.  One workgroup computes a tile of at most
 * TFIMM_RESIZE_AA_TILE_ROWS x TFIMM_RESIZE_AA_TILE_COLS output pixels; at most TFIMM_RESIZE_AA_MAX_BLOCKS workgroups stride
 * over the tiles.  The result does not depend on the tiling.
 * ------------------------------------------------------------------------------------- */
#define TFIMM_RESIZE_AA_MAX_TAPS 64
#define TFIMM_RESIZE_AA_TILE_ROWS 16
#define TFIMM_RESIZE_AA_TILE_COLS 32
#define TFIMM_RESIZE_AA_MAX_BLOCKS 1024
typedef struct tfimm_resize_aa_desc {
  const void* in;          /* uint8 [B][Hs][Ws][c_in] */
  void* out;               /* bf16 (tfimm_hip_ref_preprocess_resize_aa: float32), the layouts of tfimm_resize_desc.out */
  const int32_t* y_start;  /* [H] first source row of the span of every output row */
  const int32_t* y_count;  /* [H] its number of taps, <= y_taps */
  const float* y_w;        /* [H][y_taps] the weights; entries past the count are +0.0 */
  const int32_t* x_start;  /* [W] */
  const int32_t* x_count;  /* [W] */
  const float* x_w;        /* [W][x_taps] */
  const float* mean_host;  /* HOST arrays of c_in floats (copied into the launch) */
  const float* std_host;
  int32_t B, Hs, Ws, c_in; /* c_in <= TFIMM_PREPROCESS_MAX_CHANNELS */
  int32_t H, W;            /* the crop window = the model's input size */
  int32_t c_out;           /* >= c_in; 4 (8 bytes per pixel) and 8 (16 bytes) are stored as one vector */
  int32_t pad_t, pad_b, pad_l, pad_r;   /* the zero border; non-zero only with c_out == 4 */
  int32_t y_taps, x_taps;  /* the span pitches T of the two axes, <= TFIMM_RESIZE_AA_MAX_TAPS */
} tfimm_resize_aa_desc;

TFIMM_API int tfimm_hip_resize_span_taps(int n_in, int n_resized, int method);
TFIMM_API int tfimm_hip_resize_spans(int n_in, int n_resized, int first, int n_out, int method, int32_t* start_host,
                                     int32_t* count_host, float* w_host);
TFIMM_API int tfimm_hip_preprocess_resize_aa(const tfimm_resize_aa_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_preprocess_resize_batch / _batch_aa: the two launches above for a batch whose images each have a SIZE OF THEIR
 * OWN (csrc/resize_batch.hip) -- what create_preprocessing(..., resize=True) runs for a LIST of images.
 * For image b they compute exactly what tfimm_hip_preprocess_resize[_aa] computes for that image alone at B = 1: the same
 * tables, the same float32 operations in the same order, the same normalisation, one rounding to bf16, the same two output
 * layouts (border zeros written by the kernel).
 *
 * Everything that varies with the sources lives in DEVICE memory; the descriptor holds pointers, the output geometry and
 * capacities only, and the grid and the LDS size are functions of those scalars.  A recording of the launch (hipGraph) is
 * therefore valid for any later contents of the buffers: one recording serves every mix of sizes.
 *   in     one uint8 arena of in_bytes bytes; image b is packed [Hs_b][Ws_b][c_in] at byte offset recs[b].in_offset --
 *          any offset, no alignment (source loads are byte loads)
 *   recs   B records tfimm_resize_batch_rec, one per image
 *   plain  idx / w arenas of B * (H + W) * taps entries: the tables of tfimm_hip_resize_taps, image b's rows at element
 *          recs[b].y_tab, its columns at recs[b].x_tab
 *   aa     start / count arenas of B * (H + W) entries (image b's rows at recs[b].y_tab, its columns at recs[b].x_tab) and
 *          a weight arena of w_floats floats: image b's row weights [H][y_taps] at float recs[b].y_w, its column weights
 *          [W][x_taps] at recs[b].x_w -- every image at its own pitches (the tables of tfimm_hip_resize_spans)
 * tfimm_hip_resize_batch_tables below builds records and arenas on the host.  The kernels trust none of it: every table
 * index is clamped into its image, every source byte offset into [0, in_bytes), every table offset into its arena, every
 * pitch into [1, taps_cap], every tile shape into the LDS allocation; all global offsets are 64-bit.  A stale or bad record
 * gives wrong pixels, never an access out of bounds.
 *
 * Plain launch: one thread per output pixel, at most 4096 workgroups stride over B * HP * WP pixels.  Antialiased launch:
 * workgroups (at most TFIMM_RESIZE_AA_MAX_BLOCKS) stride over the tiles of all images -- image b owns the tile indices
 * [tile0, tile0 + n_tiles) of its record, tile_rows x TFIMM_RESIZE_AA_TILE_COLS output pixels each, found by a binary
 * search over the records -- with lds_bytes of dynamic LDS (0 = the 64 KiB budget of the uniform launch; a caller that knows
 * its largest tile, tfimm_resize_batch_sizes.lds_floats, may pass less to raise occupancy: the size still depends on no
 * single batch as long as the caller keeps it a capacity).
 * Refused with the invalid-argument code, nothing launched: null pointers, non-positive sizes, c_in >
 * TFIMM_PREPROCESS_MAX_CHANNELS, c_out < c_in, a padded layout with c_out != 4, std == 0, taps not 2 or 4, taps_cap >
 * TFIMM_RESIZE_AA_MAX_TAPS, lds_bytes > 64 KiB.
 * ------------------------------------------------------------------------------------- */
typedef struct tfimm_resize_batch_rec {
  int64_t in_offset;       /* byte offset of the image in the pixel arena */
  int32_t Hs, Ws;          /* its size */
  int32_t y_tab, x_tab;    /* element offsets of its row / column tables: plain, into idx and w (taps entries per position);
                              aa, into start and count (one entry per position) */
  int32_t y_w, x_w;        /* aa: float offsets of its row / column weights in the weight arena (plain: = y_tab, x_tab) */
  int32_t y_taps, x_taps;  /* aa: its span pitches (plain: taps) */
  int32_t tile_rows;       /* aa: output rows of a tile of this image (the rule of the uniform launch; plain: 0) */
  int32_t cols_max;        /* aa: source columns an LDS row of its tiles holds */
  int32_t tile0, n_tiles;  /* aa: its first tile in the launch's numbering, and how many it has */
} tfimm_resize_batch_rec;

typedef struct tfimm_resize_batch_desc {
  const void* in;          /* uint8 arena, in_bytes bytes */
  const tfimm_resize_batch_rec* recs;   /* DEVICE [B] */
  void* out;               /* bf16 (tfimm_hip_ref_preprocess_resize_batch: float32), the layouts of tfimm_resize_desc.out */
  const int32_t* idx;      /* DEVICE [B * (H + W) * taps] */
  const float* w;          /* DEVICE [B * (H + W) * taps] */
  const float* mean_host;  /* HOST arrays of c_in floats (copied into the launch) */
  const float* std_host;
  int64_t in_bytes;
  int32_t B, c_in, H, W, c_out;
  int32_t pad_t, pad_b, pad_l, pad_r;
  int32_t taps;            /* 2 = bilinear, 4 = bicubic */
} tfimm_resize_batch_desc;

typedef struct tfimm_resize_batch_aa_desc {
  const void* in;          /* uint8 arena, in_bytes bytes */
  const tfimm_resize_batch_rec* recs;   /* DEVICE [B] */
  void* out;
  const int32_t* start;    /* DEVICE [B * (H + W)] */
  const int32_t* count;    /* DEVICE [B * (H + W)] */
  const float* w;          /* DEVICE [w_floats] */
  const float* mean_host;
  const float* std_host;
  int64_t in_bytes;
  int64_t w_floats;        /* capacity of the weight arena */
  int32_t B, c_in, H, W, c_out;
  int32_t pad_t, pad_b, pad_l, pad_r;
  int32_t taps_cap;        /* the largest pitch a record may name, <= TFIMM_RESIZE_AA_MAX_TAPS */
  int32_t lds_bytes;       /* dynamic LDS of a workgroup, a multiple of 4 and <= 64 KiB; 0 = 64 KiB */
} tfimm_resize_batch_aa_desc;

/* What a mixed batch needs, reported by tfimm_hip_resize_batch_tables */
typedef struct tfimm_resize_batch_sizes {
  int64_t in_bytes;        /* the images packed back to back in list order: the sum of Hs * Ws * c_in */
  int64_t tab_elems;       /* entries of idx and of w (plain) or of start and of count (aa) */
  int64_t w_floats;        /* floats of the weight arena (plain: = tab_elems) */
  int64_t n_tiles;         /* aa: tiles of the whole batch (plain: 0) */
  int32_t max_taps;        /* aa: the largest pitch of the batch (plain: taps) */
  int32_t lds_floats;      /* aa: the largest tile_rows * cols_max * c_in of the batch (plain: 0) */
  int32_t bad_image;       /* the first image one of whose axes needs more than TFIMM_RESIZE_AA_MAX_TAPS taps, or -1 */
  int32_t reserved;
} tfimm_resize_batch_sizes;

/* The ONE place in C where records and tables of a mixed batch are built -- over tfimm_hip_resize_taps and
 * tfimm_hip_resize_spans, which stay the only statements of the tap and span rules.  A plain host function: no GPU is needed
 * or touched.  src_hw: [B][2] = (Hs, Ws); geometry: [B][4] = (Rh, Rw, top, left) (tfimm/models/factory.py resize_geometry);
 * (H, W): the crop window; pad: the 4 border widths (t, b, l, r) of the output layout, or NULL for none -- c_in and pad
 * enter the tile bookkeeping only; method 0 = bilinear, 1 = bicubic.  *sizes is always filled.  With recs == NULL nothing
 * else is written (the sizing call); otherwise recs [B], tab_a and tab_b [tab_elems] (plain: idx and unused, may be NULL;
 * aa: start and count) and w [w_floats] are filled -- each array at EXACTLY the reported size.  An image outside the
 * antialias domain is named in sizes->bad_image and the call returns the invalid-argument code. */
TFIMM_API int tfimm_hip_resize_batch_tables(int B, const int32_t* src_hw, const int32_t* geometry, int H, int W, int c_in,
                                            const int32_t* pad, int method, int antialias, tfimm_resize_batch_sizes* sizes,
                                            tfimm_resize_batch_rec* recs, int32_t* tab_a, int32_t* tab_b, float* w);
TFIMM_API int tfimm_hip_preprocess_resize_batch(const tfimm_resize_batch_desc* d, void* stream);
TFIMM_API int tfimm_hip_preprocess_resize_batch_aa(const tfimm_resize_batch_aa_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_preprocess_regions / _regions_aa: the two launches above for BOXES inside larger frames (csrc/resize_regions.hip;
 * DESIGN.md 3.22) -- what create_preprocessing(..., resize=True) runs for pre(frames, boxes=...).  Box n with integer pixel
 * corners (y0, x0, y1, x1) covers rows [y0, y1) and columns [x0, x1) of frame box_frame[n] and is an image of its own: the
 * result is, bit for bit, what tfimm_hip_preprocess_resize_batch[_aa] computes for the slice packed on its own -- the same
 * geometry (of the box's size), the same tables, the same float32 operations, the same normalisation and rounding, the same
 * two output layouts.  Taps beyond the box edge clamp to the BOX: no pixel outside it contributes.
 *
 * What differs is the addressing.  Every frame lies ONCE in the arena, however many boxes name it, and a record says where
 * its box starts and how far apart two rows are:
 *   in     one uint8 arena of in_bytes bytes; frame f is packed [Hf][Wf][c_in] at any byte offset
 *   recs   B records tfimm_resize_region_rec, one per box: the fields of tfimm_resize_batch_rec with
 *            in_offset  the byte offset of the box's FIRST PIXEL: the frame's offset + (y0 * Wf + x0) * c_in
 *            row_pitch  the bytes between two rows: Wf * c_in of the box's frame
 *            Hs, Ws     the size of the BOX
 *   tables exactly those of tfimm_hip_preprocess_resize_batch[_aa] for images of the boxes' sizes
 * The kernels trust none of it, as above; the row pitch is clamped to [1, 2^24 * TFIMM_PREPROCESS_MAX_CHANNELS].  Launch
 * shapes, LDS size and refusals are those of tfimm_hip_preprocess_resize_batch[_aa].
 * ------------------------------------------------------------------------------------- */
typedef struct tfimm_resize_region_rec {
  int64_t in_offset;       /* byte offset of the box's first pixel in the pixel arena */
  int64_t row_pitch;       /* bytes between two rows of the box: a row of its frame */
  int32_t Hs, Ws;          /* the size of the box */
  int32_t y_tab, x_tab;    /* as in tfimm_resize_batch_rec, from here on */
  int32_t y_w, x_w;
  int32_t y_taps, x_taps;
  int32_t tile_rows;
  int32_t cols_max;
  int32_t tile0, n_tiles;
} tfimm_resize_region_rec;

typedef struct tfimm_resize_region_desc {
  const void* in;          /* uint8 arena, in_bytes bytes: the frames */
  const tfimm_resize_region_rec* recs;   /* DEVICE [B] */
  void* out;               /* bf16 (tfimm_hip_ref_preprocess_regions: float32), the layouts of tfimm_resize_desc.out */
  const int32_t* idx;      /* DEVICE [B * (H + W) * taps] */
  const float* w;          /* DEVICE [B * (H + W) * taps] */
  const float* mean_host;  /* HOST arrays of c_in floats (copied into the launch) */
  const float* std_host;
  int64_t in_bytes;
  int32_t B, c_in, H, W, c_out;   /* B: the number of boxes */
  int32_t pad_t, pad_b, pad_l, pad_r;
  int32_t taps;            /* 2 = bilinear, 4 = bicubic */
} tfimm_resize_region_desc;

typedef struct tfimm_resize_region_aa_desc {
  const void* in;          /* uint8 arena, in_bytes bytes: the frames */
  const tfimm_resize_region_rec* recs;   /* DEVICE [B] */
  void* out;
  const int32_t* start;    /* DEVICE [B * (H + W)] */
  const int32_t* count;    /* DEVICE [B * (H + W)] */
  const float* w;          /* DEVICE [w_floats] */
  const float* mean_host;
  const float* std_host;
  int64_t in_bytes;
  int64_t w_floats;        /* capacity of the weight arena */
  int32_t B, c_in, H, W, c_out;
  int32_t pad_t, pad_b, pad_l, pad_r;
  int32_t taps_cap;        /* the largest pitch a record may name, <= TFIMM_RESIZE_AA_MAX_TAPS */
  int32_t lds_bytes;       /* dynamic LDS of a workgroup, a multiple of 4 and <= 64 KiB; 0 = 64 KiB */
} tfimm_resize_region_aa_desc;

/* Records and tables of N boxes in F frames, built over tfimm_hip_resize_batch_tables (and so over tfimm_hip_resize_taps and
 * tfimm_hip_resize_spans).  A plain host function: no GPU is needed or touched.  frame_hw: [F][2] = (Hf, Wf); boxes: [N][4] =
 * (y0, x0, y1, x1); box_frame: [N] frame indices, in any order, repeats allowed; geometry: [N][4] = (Rh, Rw, top, left) of
 * every box's own size; the other arguments and the arrays written as in tfimm_hip_resize_batch_tables with B = N.  The
 * frames are packed ONCE each, back to back in list order: sizes->in_bytes is the sum of Hf * Wf * c_in over the F frames.
 * Refused with the invalid-argument code and nothing written: an empty box, a box outside its frame, a frame index out of
 * range (the message names the box).  A box outside the antialias domain is named in sizes->bad_image (sizes is filled,
 * nothing else written) and the call returns the invalid-argument code. */
TFIMM_API int tfimm_hip_resize_region_tables(int F, const int32_t* frame_hw, int N, const int32_t* boxes,
                                             const int32_t* box_frame, const int32_t* geometry, int H, int W, int c_in,
                                             const int32_t* pad, int method, int antialias, tfimm_resize_batch_sizes* sizes,
                                             tfimm_resize_region_rec* recs, int32_t* tab_a, int32_t* tab_b, float* w);
TFIMM_API int tfimm_hip_preprocess_regions(const tfimm_resize_region_desc* d, void* stream);
TFIMM_API int tfimm_hip_preprocess_regions_aa(const tfimm_resize_region_aa_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_layernorm: y[r][:] = (x[r][:] - mean) * rsqrt(var + eps) * gamma + beta,
 * population variance, fp32 statistics.  x row r starts at x + r*x_stride (elements),
 * y row r at y + r*y_stride.  Replaces tf.keras.layers.LayerNormalization
 * (layers/factory.py:42-50; call sites vit.py:222,231,452  swin.py:295,322,504).
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_layernorm(const void* x, void* y, const float* gamma, const float* beta,
                        int64_t rows, int d, int64_t x_stride, int64_t y_stride, float eps,
                        void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_attention: fused softmax(scale * Q K^T [+ bias] [+ mask]) V per (sequence, head),
 * reading q/k/v straight out of the packed QKV projection  qkv[row][3][heads][hd]  and
 * writing out[row][heads*hd].  fp32 softmax, bf16 P.  Head dims: global attention 1..128 (vit_huge_patch14: 80),
 * windows 1..64; anything else returns TFIMM_EUNSUP.
 *
 * window == 0: global attention, sequence s = image, token t -> row s*n_tokens + t.
 *     Replaces vit.py:156-167 (reshape/transpose, scale*matmul, softmax, matmul, merge).
 * window  > 0: Swin (shifted-)window attention on a res_h x res_w token grid, sequence =
 *     (image, window); token (ty,tx) of window (wy,wx) is grid position
 *     ((wy*window+ty+shift) % res_h, (wx*window+tx+shift) % res_w) -- i.e. tf.roll(-shift),
 *     window_partition, window_reverse and tf.roll(+shift) (swin.py:72-108,295-318) are
 *     folded into the load/store index map.  rel_bias[heads][n][n] (fp32, n = window^2) is
 *     the gathered relative_position_bias (swin.py:175-184); when shift > 0 the -100 mask of
 *     swin.py:249-273 is recomputed from region ids.
 * ------------------------------------------------------------------------------------- */
typedef struct tfimm_attn_desc {
  const void* qkv;        /* bf16 [rows][3*heads*hd] */
  void* out;              /* bf16 [rows][heads*hd]   */
  const float* rel_bias;  /* fp32 [heads][n][n] or NULL (NULL: no bias, and then no bias_log2 either) */
  int32_t batch;          /* images */
  int32_t n_tokens;       /* tokens per image (global) / res_h*res_w (window) */
  int32_t heads, hd;
  float scale;
  int32_t window, shift, res_h, res_w;
  const float* bias_log2; /* optional (window > 0), accompanies rel_bias and never replaces it (some kernels read the
                             tiles, others rel_bias: tiles with rel_bias == NULL return TFIMM_EINVAL):
                             rel_bias with the shift mask already added and everything
                             multiplied by log2(e), one tile per window kind:
                             [kinds][heads][n][ceil64(n)], kinds = 1 (shift == 0) or 4 (shift > 0; kind =
                             2 * (last window row) + (last window column) -- the only four distinct
                             patterns of the mask of swin.py:249-273).  Built once on the host
                             (tfimm/engine/pack.py: swin_bias_tiles); when NULL the kernel combines
                             rel_bias and the mask itself for every workgroup. */
} tfimm_attn_desc;

TFIMM_API int tfimm_hip_attention(const tfimm_attn_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_talking_heads_attention: CaiT self-attention with the two head-mixing Dense layers
 * around the softmax (TalkingHeadAttention.call, cait.py:233-262):
 *     s[b,h,i,j]  = scale * q[b,i,h,:] . k[b,j,h,:]
 *     a[b,h',i,j] = softmax_j( sum_h s[b,h,i,j] * proj_l_w[h][h'] + proj_l_b[h'] )
 *     w[b,g,i,j]  = sum_h' a[b,h',i,j] * proj_w_w[h'][g] + proj_w_b[g]
 *     out[b,i,g,:] = sum_j w[b,g,i,j] * v[b,j,g,:]
 * qkv packed as for tfimm_hip_attention (bf16 [rows][3*heads*hd], rows = batch * n_tokens);
 * proj_*_w / proj_*_b are the Keras kernels [heads_in][heads_out] and biases in fp32 and are HOST
 * pointers (heads <= 16): the library copies them into the kernel's argument segment at launch, so
 * they are read with scalar loads -- they are layer weights, known on the host when the plan is built.  MFMA kernel for hd in {32, 48} (every
 * CaiT configuration has hd = 48) and heads in {1, 2, 3, 4, 6, 8, 16}; any other shape takes a plain
 * fp32 kernel (one workgroup per query row) as long as 2 * heads * n_tokens floats fit in LDS.
 * ------------------------------------------------------------------------------------- */
typedef struct tfimm_tha_desc {
  const void* qkv;
  void* out;                /* bf16 [rows][heads*hd] */
  const float* proj_l_w;    /* HOST fp32 [heads][heads] */
  const float* proj_l_b;    /* HOST fp32 [heads] */
  const float* proj_w_w;
  const float* proj_w_b;
  int32_t batch, n_tokens, heads, hd;
  float scale;
  const float* proj_dev;    /* optional DEVICE fp32 [proj_l_w | proj_l_b | proj_w_w | proj_w_b] (2 * (heads^2 + heads) values): the
                               MFMA kernel then takes the mixing layers from there instead of its argument segment (what
                               plans do; results are the same either way) */
} tfimm_tha_desc;

TFIMM_API int tfimm_hip_talking_heads_attention(const tfimm_tha_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_class_attention: the class token of every image attends to all of its tokens
 * (ClassAttention.call, cait.py:118-146 between the q/k/v and proj layers):
 *     out[b, h*hd + d] = sum_j softmax_j( q[b, h, :] . k[b, j, h, :] ) * v[b, j, h, d]
 * q: bf16, one row per image with row stride ldq (ALREADY scaled: the caller folds
 * (D/H)^-0.5 into the q layer); kv: bf16 [B*n_tokens][ldkv] holding k in columns
 * [0, heads*hd) and v in [heads*hd, 2*heads*hd); out: bf16, one row per image, stride ldo.
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_class_attention(const void* q, const void* kv, void* out, int B, int n_tokens, int heads,
                              int hd, int ldq, int ldkv, int ldo, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_copy_rows: dst[b][dst_row0 + r][:] = src[b][r][:] for r < src_rows -- one input of
 * a tf.concat along the token axis (cait.py:425-426: class token in front of the patch tokens).
 * bf16 rows of d elements (16-byte vectors when d % 8 == 0 and both buffers are 16-byte aligned).
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_copy_rows(const void* src, void* dst, int B, int src_rows, int dst_rows, int dst_row0,
                        int d, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_maxpool: k x k / stride max pool with symmetric zero padding `pad`, NHWC bf16.
 * Padding contributes ZEROS (the reference pads with ZeroPadding2D and pools VALID,
 * resnet.py:538-540), not -inf.
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_maxpool(const void* x, void* y, int B, int H, int W, int C, int k, int stride,
                      int pad, int OH, int OW, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_mean_rows: y[b][c] = mean_r x[b][r][c], r < R.  out_f32: 0 bf16, 1 fp32.
 * GlobalAveragePooling2D / 1D (layers/classifier.py:35, swin.py:506) and the SE squeeze
 * (efficientnet_blocks.py:242).
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_mean_rows(const void* x, void* y, int B, int R, int C, int out_f32, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_bcast_rows: dst[(b*dst_rows_per_image + t)][:] = src[t][:], t < n_rows, b < B.
 * Writes the (cls [, dist]) token rows, already summed with their pos_embed rows on the
 * host (vit.py:427-434 tf.repeat / tf.concat / + pos_embed).
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_bcast_rows(const void* src, void* dst, int B, int n_rows, int d,
                         int dst_rows_per_image, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_dwconv: depthwise k x k conv, stride s, explicit (pad_t, pad_l) zero padding,
 * NHWC bf16, folded-BN scale already in w, + bias, + activation.  w: fp32 [k*k][C].
 * Optionally accumulates per-(image, channel) sums of the OUTPUT into sum_out -- the SE squeeze fused into the
 * producer: int64 [B][C] FIXED-POINT accumulators in units of 2^-20 (zeroed by the caller; read them with
 * tfimm_hip_se_gate(sums_fixed = 1)).  Integer adds commute, so the sums -- and everything computed from them -- are
 * bit-identical from launch to launch whatever order the workgroups arrive in (float atomics were not), and from batch
 * size to batch size: a thread converts the partial sum of every finished output row (four pixels of one channel, rounded
 * to 2^-16; partials beyond +-32768 saturate) before it adds, so the way a launch splits an image into row segments
 * does not show in the result.
 * Replaces DepthwiseConv2D + BatchNormalization + Activation
 * (efficientnet_blocks.py:350-352,443-445; convnext.py:191-197 with act none).
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_dwconv(const void* x, const float* w, const float* bias, void* y, void* sum_out,
                     int B, int H, int W, int C, int k, int stride, int pad_t, int pad_l,
                     int OH, int OW, int act, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_se_gate: gate[b][c] = gate_act( W2 . act( W1 . mean[b] + b1 ) + b2 )[c]
 * with mean[b][c] = sums[b][c] * inv_count.  sums: fp32 [B][C] (sums_fixed = 0: e.g. the means of tfimm_hip_mean_rows
 * with inv_count = 1) or the int64 fixed-point accumulators of tfimm_hip_dwconv / tfimm_hip_expand_dwconv (sums_fixed = 1).
 * w1: fp32 [rd][C] (reduce conv, transposed), w2: fp32 [rd][C]
 * (expand conv as Keras stores it) -- both are walked along C by consecutive threads.
 * SqueezeExcite.call (efficientnet_blocks.py:241-248) / SEModule.call (layers/attention.py:66-74)
 * minus the final multiply, which is fused into the consumer (a_scale of tfimm_hip_gemm)
 * or done by tfimm_hip_scale_channels.
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_se_gate(const void* sums, int sums_fixed, float inv_count, const float* w1, const float* b1,
                      const float* w2, const float* b2, float* gate, int B, int C, int rd,
                      int act, int gate_act, void* stream);

/* y[b][r][c] = x[b][r][c] * gate[b][c] (+ residual, then relu if act_after != 0) */
TFIMM_API int tfimm_hip_scale_channels(const void* x, const float* gate, const void* residual, void* y,
                             int B, int R, int C, int act_after, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_patch_merge_ln: Swin PatchMerging front half (swin.py:352-359): gather the 2x2
 * neighbourhood in the order (0,0),(1,0),(0,1),(1,1) -> 4C channels, LayerNorm(4C).
 * x: bf16 [B][H*W][C]; y: bf16 [B][(H/2)*(W/2)][4C].
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_patch_merge_ln(const void* x, void* y, const float* gamma, const float* beta,
                             int B, int H, int W, int C, float eps, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_conv_chain: the tail of a ResNet bottleneck block in ONE launch,
 *     mid = act1( conv_{KH x KW, stride, pad}(x) * W1 + b1 )            [M][C1]   never written to memory
 *     out = act2( mid . W2^T + b2 + residual )                          [M][N2]
 * i.e. pad2 / conv2 / bn2 / act2 / conv3 / bn3 / += shortcut / act3 of Bottleneck.call (resnet.py:273-290), BatchNorm
 * folded into (W, b) by the host.  x: bf16 NHWC [B][H][W][Cin], Cin % 64 == 0; w1: bf16 [C1][ldw1 = KH*KW*Cin] in
 * (ky, kx, ci) order; w2: bf16 [N2][ldw2] with its K (= C1) axis PERMUTED: within every 16 channels the two middle
 * quads are swapped (k-slot 16t + s holds channel 16t + {0..3, 8..11, 4..7, 12..15}[s]) -- the order in which a wave's
 * GEMM-1 accumulators become the register operand of GEMM 2 (tfimm/engine/pack.py chain_k_order); residual (may be
 * NULL) / out: bf16 rows of ldr / ldc elements (multiples of 8); M = B*OH*OW.  Built for the ResNet stage-1 shape --
 * 3x3 / stride 1 / pad 1, Cin = C1 = 64, W <= 63, N2 in {256, 512} (csrc/gemm_chain_kernel.h) -- and the stage-2 shape --
 * Cin = C1 = 128, W <= 31, N2 in {256, 512}, no shortcut convolution (csrc/conv_strip.hip); anything else returns TFIMM_EUNSUP and the caller
 * runs the two convolutions as two tfimm_hip_gemm launches (same arithmetic: fp32 accumulation, the intermediate
 * rounded to bf16 once; only the summation order inside GEMM 2's 16-wide k-steps differs).
 * ------------------------------------------------------------------------------------- */
typedef struct tfimm_chain_desc {
  const void* x;
  const void* w1;
  const float* b1;
  const void* w2;
  const float* b2;
  const void* residual;
  void* out;
  int32_t B, H, W, Cin, KH, KW, stride, pad_t, pad_l, OH, OW;
  int32_t C1, N2;
  int32_t ldw1, ldw2, ldr, ldc;
  int32_t act1, act2;       /* TFIMM_ACT_*; act2 is applied after the residual add */
  const void* ds_x;         /* optional: the shortcut is a 1x1 convolution + BN of the block INPUT (first block of a stage,
                               resnet.py:315-330): bf16 [M][ds_cin], ds_cin = 64.  Its product accumulates into the second
                               GEMM's accumulators -- out = act2(mid . W2^T + ds_x . Wds^T + b2), the caller adding the
                               shortcut's folded-BN shift to b2 -- so neither that launch nor its tensor exists.
                               residual must be NULL, activations relu. */
  const void* ds_w;         /* its weights (BN scale folded) as MFMA fragments: bf16 [N2/32][4][64][8], element
                               [blk][t][lane][e] = Wds[k = 16 t + 8 (lane >> 5) + e][n = 32 blk + (lane & 31)] */
  int32_t ds_cin;
} tfimm_chain_desc;

TFIMM_API int tfimm_hip_conv_chain(const tfimm_chain_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_conv_chain_next: tfimm_hip_conv_chain with the 1x1 convolution that READS its result -- conv1 / bn1 / act1 of
 * the following bottleneck block (resnet.py:269-271) -- as a second output of the same launch,
 *     out  = as tfimm_hip_conv_chain computes it from `chain`                [M][N2]   bit-identical to that call
 *     out2 = relu( out . W3^T + b3 )                                         [M][N3]
 * so that convolution never re-reads the N2-channel tensor from memory: every slice of `out` is multiplied with W3 where it
 * is formed, from the bf16 values that are stored (fp32 accumulation over all N2 channels, one rounding to bf16 -- the
 * arithmetic of tfimm_hip_gemm on `out`, in another summation order).  w3: bf16 [N3][ldw3], K = N2 in natural order, BN
 * folded; b3: fp32 [N3]; out2: bf16 rows of ldc2 elements (a multiple of 8).  Built for the plain stage-1 tail: C1 = 64,
 * N2 = 256, N3 = 64, relu activations, no shortcut convolution (ds_x NULL).  TFIMM_EUNSUP for C1 = 128, the ds_* flavour,
 * other activations and any other N2 / N3: the caller then runs tfimm_hip_conv_chain and tfimm_hip_gemm.
 * A new entry point and a new descriptor: nothing that existed changed, the ABI version stays as it is.
 * ------------------------------------------------------------------------------------- */
typedef struct tfimm_chain_next_desc {
  tfimm_chain_desc chain;
  const void* w3;
  const float* b3;
  void* out2;
  int32_t N3, ldw3, ldc2;
} tfimm_chain_next_desc;

TFIMM_API int tfimm_hip_conv_chain_next(const tfimm_chain_next_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_expand_dwconv: the front half of an inverted-residual block in one launch --
 *   conv_pw (1x1, Cin -> C) + bn1 + act1, then conv_dw (k x k depthwise, stride) + bn2 + act2, optionally the
 *   squeeze sums of the result (efficientnet_blocks.py:438-445, InvertedResidual.call up to `se`).
 * The expanded tensor exists only in LDS, rounded to bf16 exactly where the two-launch path (tfimm_hip_gemm +
 * tfimm_hip_dwconv) rounds the tensor it stores; depthwise accumulation is fp32.
 *   x    bf16 [B][H][W][Cin], Cin % 8 == 0, Cin <= 32
 *   w1   expand weights (BN scale folded) as MFMA fragments: bf16 [Cpad/32][2][64][8], element
 *        [cc][ks][lane][j] = W1[k = 16 ks + 8 (lane >> 5) + j][c = 32 cc + (lane & 31)], zero for k >= Cin, c >= C
 *   b1, b2  fp32 [Cpad] folded BN shifts;  wdw  fp32 [k*k][Cpad] depthwise taps (BN scale folded), zero padded
 *   y    bf16 [B][OH][OW][C];  sum_out  int64 [B][C] fixed-point squeeze sums as in tfimm_hip_dwconv (zeroed by the caller) or NULL
 * k in {3, 5}, stride in {1, 2}, explicit top / left zero padding of the EXPANDED tensor (bottom / right follow from
 * OH, OW); at stride 1 at most 512 expanded channels (their bias is staged in LDS once); one image of the output below 2 GiB.
 * Anything else returns TFIMM_EUNSUP and the caller runs the two launches.
 * ------------------------------------------------------------------------------------- */
typedef struct tfimm_expand_dw_desc {
  const void* x;
  const void* w1;
  const float* b1;
  const float* wdw;
  const float* b2;
  void* y;
  void* sum_out;
  int32_t B, H, W, Cin, C, Cpad, k, stride, pad_t, pad_l, OH, OW;
  int32_t act1, act2;
  int32_t stem;           /* 1: the "expansion" is the network's 3 x 3 / stride 2 RGB stem convolution (conv_stem + bn1 + act,
                             efficientnet.py:300-302) in front of the first block's depthwise layer: x is the zero-bordered
                             4-channel image [B][img_h][img_w][4] of tfimm_hip_cast_input_pad (the convolution itself pads
                             nothing), Cin = 4, H x W the convolution's OUTPUT size, k = 3 / stride = 1 the depthwise layer,
                             and w1 is bf16 [Cpad/32][3][64][8] with element [cc][ks][lane][j] = W[tap][c][32 cc + (lane & 31)],
                             tap = 4 ks + 2 (lane >> 5) + j / 4, c = j % 4 (zero for tap >= 9, c >= 3) */
  int32_t img_h, img_w;
} tfimm_expand_dw_desc;

TFIMM_API int tfimm_hip_expand_dwconv(const tfimm_expand_dw_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_attention_probs: probs[b][h][i][j] = softmax_j(scale * q[b,i,h,:] . k[b,j,h,:]) in fp32 --
 * the attention map ViTMultiHeadAttention.call returns as features["attn"] when return_features=True
 * (vit.py:160-163; ViT.forward_features stores it as "block_<j>/attn", vit.py:447-450).  qkv: bf16
 * [B*n_tokens][3*heads*hd] as tfimm_hip_attention reads it.  Feature path only: the plain forward never
 * materialises the map.
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_attention_probs(const void* qkv, void* probs, int B, int n_tokens, int heads, int hd,
                              float scale, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_group_norm: GroupNormalization over NHWC (layers/norm.py:37-165, group_normalize): per (image, group)
 * mean / population variance over (H, W, C/groups), y = (x - mean)*inv + beta, inv = rsqrt(var+eps)*gamma
 * (tf.nn.batch_normalization), then act, then (+ residual, act_after_res) when residual != NULL -- the
 * norm + activation + shortcut add of a ResNet block whose norm_layer is "group_norm" (resnet.py:269-290).
 * x / residual / y: bf16 [B][rows][C]; gamma / beta: fp32 [C]; stats_ws: int64 [B][groups][2] scratch (zeroed here): sum and
 * sum of squares of x minus the group's first value, in 2^-28 fixed point, so the statistics do not depend on the order the
 * workgroups add them in.
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_group_norm(const void* x, const float* gamma, const float* beta, const void* residual, void* y,
                         void* stats_ws, int B, int rows, int C, int groups, float eps, int act,
                         int act_after_res, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_blur_pool: BlurPool2D(kernel_size=3, stride) (layers/blurpool.py:5-66): tf.pad(REFLECT) by
 * p = (3 + stride) / 2 - 1, then the depthwise [1 2 1] x [1 2 1] / 16 filter at `stride`, VALID.
 * x: bf16 [B][H][W][C] -> y: bf16 [B][OH][OW][C], OH = (H + 2p - 3) / stride + 1.
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_blur_pool(const void* x, void* y, int B, int H, int W, int C, int stride, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_avg_pool: AveragePooling2D(pool_size=k, strides=stride, padding="same") (resnet.py:299-301):
 * OH = ceil(H / stride); windows clipped at the border average over their VALID elements only.
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_avg_pool(const void* x, void* y, int B, int H, int W, int C, int k, int stride, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_eca_gate: gate[b][c] = gate_act( sum_t w[t] * mean[b][c + t - (k-1)/2] ), zero padded over the
 * channel axis, mean = sums * inv_count -- EcaModule.call between the channel mean and the final multiply
 * (ZeroPadding1D + Conv1D(1, k, no bias) + gate, layers/attention.py:110-126).  All fp32; w: [k].
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_eca_gate(const float* sums, float inv_count, const float* w, float* gate, int B, int C, int k,
                       int gate_act, void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_grouped_conv3x3: ZeroPadding2D(1) + Conv2D(3x3, stride, groups) (+ folded BatchNorm + activation) for
 * groups of at most 32 channels with equal input and output width -- ResNeXt's conv2 (resnet.py:229-241).  Runs as
 * 32-channel super-groups: 32 / (C / groups) times the useful multiply-accumulates instead of `groups` times for the
 * dense block-diagonal expansion.  x / y: bf16 NHWC, C % 32 == 0; wfrag: the kernel packed per MFMA lane by
 * tfimm/engine/pack.py pack_grouped3x3 ([C / 32][18][64] 16-byte fragments); bias: fp32 [C].
 * ------------------------------------------------------------------------------------- */
TFIMM_API int tfimm_hip_grouped_conv3x3(const void* x, const void* wfrag, const float* bias, void* y, int B, int H, int W,
                              int C, int stride, int act, void* stream);

/* hipMemsetAsync on the library's own HIP runtime (zeroing accumulation buffers such as the
 * dwconv sum_out) -- avoids a second runtime instance being loaded by the host language. */
TFIMM_API int tfimm_hip_memset_async(void* dst, int value, size_t bytes, void* stream);

/* Elementwise y = act(x + bias?)  -- used by paths with no producer to fuse into. */
TFIMM_API int tfimm_hip_bias_act(const void* x, const float* bias, void* y, int64_t rows, int C, int act,
                       void* stream);

/* ---------------------------------------------------------------------------------------
 * tfimm_hip_mlp_fused: out = residual + fc2( act( fc1( LayerNormalization(x) ) ) ) in ONE launch -- norm2 / mlp.fc1 / GELU /
 * mlp.fc2 / shortcut add of a Swin block (swin.py:322-325, layers/transformers.py:208-214), norm / fc1 / GELU / fc2 (/ LayerScale,
 * folded into w2 / b2) / shortcut add of a ConvNeXt block (convnext.py:226-232).  The hidden tensor is never written: the bf16-packed
 * accumulators of the first GEMM are the register operand of the second (csrc/mlp.hip).  Built for C = 128, hidden = 512.
 *   x, residual, out  bf16 [M][C] (residual may alias x)
 *   w1   bf16 [hidden][C], LayerNorm gamma folded in (W1' = gamma * W1, then rounded);  b1 fp32 [hidden] = beta . W1 + b1;  the
 *        kernel normalises the rows itself: (x - mean) * rstd (two-pass statistics, eps), rounded to bf16, is what W1' multiplies
 *   w2   bf16 [C][hidden] with its K axis in tfimm/engine/pack.py chain_k_order (within every 16 channels the two middle quads
 *        swapped);  b2 fp32 [C]
 * Anything else returns TFIMM_EUNSUP and the caller runs tfimm_hip_row_stats + two tfimm_hip_gemm launches.
 * ------------------------------------------------------------------------------------- */
typedef struct tfimm_mlp_desc {
  const void* x;
  const void* w1;
  const float* b1;
  const void* w2;
  const float* b2;
  const void* residual;
  void* out;
  int64_t M;
  int32_t C, hidden, act;
  float eps;
} tfimm_mlp_desc;
TFIMM_API int tfimm_hip_mlp_fused(const tfimm_mlp_desc* d, void* stream);

/* =======================================================================================
 * MXFP8 PATH (csrc/mx.hip; selected by TFIMM_PRECISION=fp8, tfimm/engine/precision.py)
 *
 * OCP microscaling FP8: e4m3fn elements (OCP encoding, not fnuz) in blocks of 32 along K, one E8M0 scale byte per block
 * (2^(byte - 127)).  An MXFP8 matrix [rows][C] is two arrays: data uint8 [rows][ld] and scales uint8 [rows][ld / 32]; the
 * columns [C, ld) hold zero elements.  Scale rule: the smallest power of two s with amax / s <= 448 (an all-zero block gets
 * 2^-127), elements x / s rounded to nearest-even -- nothing saturates (tfimm/engine/pack.py mx_quantize is the reference).
 * ======================================================================================= */

/* tfimm_hip_quantize_mx: bf16 rows [rows][x_stride] -> MXFP8 rows (q [rows][ldq], q_scale [rows][ldq / 32]).
 * gamma / beta (fp32 [C], both or neither): a LayerNormalization over the C channels is applied first -- the two-pass fp32
 * statistics of tfimm_hip_row_stats, y = (x - mean) * rstd * gamma + beta -- so the normalised tensor is never written.
 * C % 32 == 0, C <= 4096 (TFIMM_EUNSUP beyond), ldq % 32 == 0, x 16-byte aligned.
 * Replaces, in the reference (fp8 mode): the LayerNormalization in front of a Dense layer
 *     vit.py:222,231  swin.py:317,322  cait.py:186-190  convnext.py:226-228
 * and the operand cast of a Dense layer whose input has no LayerNorm (attn/proj: vit.py:169, swin.py:197). */
TFIMM_API int tfimm_hip_quantize_mx(const void* x, int64_t rows, int C, int64_t x_stride, const float* gamma,
                                    const float* beta, float eps, void* q, void* q_scale, int ldq, void* stream);

/* tfimm_hip_gemm_mx: out[M][N] = epilogue( deq(A)[M][K] . deq(W)[N][K]^T ), fp32 accumulation (v_mfma_scale_f32_32x32x64_f8f6f4).
 *   A: MXFP8 [M][lda] + a_scale [M][lda / 32];  W: MXFP8 [N][ldw] + w_scale [N][ldw / 32] (tfimm/engine/pack.py pack_dense_mx)
 *   K % 32 == 0, N % 32 == 0; lda, ldw multiples of 128 and >= K rounded up to 128, elements [K, that) zero.
 *   epilogue as tfimm_hip_gemm: + bias[n], act unless act_after_res, + bf16 residual[m][n] (ldr), act if act_after_res;
 *   stored as out_fmt 0 = bf16, 1 = fp32 ([M][ldc]) or 2 = MXFP8 (out [M][N] + out_scale [M][N / 32]; ldc == N, N % 128 == 0:
 *   the result is quantized per 32-column block in the epilogue, the A operand of the next tfimm_hip_gemm_mx).
 *   Offsets are 64-bit: any size that fits the int32 fields is accepted.
 * Replaces, in the reference (fp8 mode): tf.keras.layers.Dense of the transformer blocks
 *     vit.py:155,169  swin.py:167,197  cait.py:59-79  transformers.py:209-212  convnext.py:229-231
 * and their residual adds (vit.py:228,234, swin.py:318,325, cait.py:187-190, convnext.py:232). */
typedef struct tfimm_gemm_mx_desc {
  const void* a;          /* e4m3 [M][lda]         */
  const void* a_scale;    /* e8m0 [M][lda / 32]    */
  const void* w;          /* e4m3 [N][ldw]         */
  const void* w_scale;    /* e8m0 [N][ldw / 32]    */
  const float* bias;      /* [N] or NULL           */
  const void* residual;   /* bf16 [M][ldr] or NULL */
  void* out;              /* bf16 / fp32 [M][ldc], or e4m3 [M][N] */
  void* out_scale;        /* e8m0 [M][N / 32] (out_fmt 2), else ignored */
  int32_t M, N, K;
  int32_t lda, ldw, ldr, ldc;
  int32_t out_fmt;        /* 0 bf16, 1 fp32, 2 MXFP8 */
  int32_t act, act_after_res;
} tfimm_gemm_mx_desc;
TFIMM_API int tfimm_hip_gemm_mx(const tfimm_gemm_mx_desc* d, void* stream);

/* =======================================================================================
 * OUTPUT END (csrc/topk.hip): top-k classes and their softmax probabilities of float32 logits
 * ======================================================================================= */

/* tfimm_hip_topk: per row of logits [B][ld] (float32, N <= ld valid columns) the k largest entries.
 *   values  float32 [B][k]  the selected logits, bit for bit
 *   indices int32   [B][k]  their columns
 *   probs   float32 [B][k]  exp(v - m) / sum_i exp(x_i - m), m the row maximum, the sum over all N columns; may be NULL.
 *                           Specified for rows whose entries are all finite; for other rows it may hold anything.
 * Order (tf.math.top_k): by value descending, compared as floats; equal values by ascending column.  -0.0 == +0.0 (the
 * column decides).  A NaN orders above +inf whatever its sign or payload, NaNs among themselves by column: a poisoned row
 * shows in the answer.  tests/topk_ref.py restates the rule on the CPU.
 * One workgroup of 256 threads per row; the row is read once and kept in LDS, hence N <= TFIMM_TOPK_MAX_N; k selection
 * rounds, k <= TFIMM_TOPK_MAX_K.  No alignment is required (16-byte loads where base and ld allow, scalar otherwise); offsets
 * are 64-bit; no atomics, no scratch memory; every reduction has a fixed order: results are bit-reproducible and a row's
 * result does not depend on B.  B == 0 launches nothing.  The logits are float32 under every precision mode, so there is no
 * tfimm_hip_ref_* twin.
 * Replaces, behind `model(x)` in a caller of the reference: tf.nn.softmax(logits) + tf.math.top_k(probs, k). */
#define TFIMM_TOPK_MAX_K 64
#define TFIMM_TOPK_MAX_N 32768
TFIMM_API int tfimm_hip_topk(const float* logits, int64_t ld, int B, int N, int k, float* values, int32_t* indices,
                             float* probs, void* stream);

/* tfimm_hip_score: per row of logits [B][ld] (float32, N <= ld valid columns) and its label labels[b], each [B]:
 *   loss  float32  log(sum_i exp(x_i - m)) - (x_y - m), m the row maximum: tf.nn.sparse_softmax_cross_entropy_with_logits.
 *                  sum >= 1 (the maximum's own term is exp(0)), so loss >= +0, and loss == 0 exactly for N == 1.  Specified
 *                  for rows whose entries are all finite; other rows get whatever float this arithmetic gives.
 *   rank  int32    the number of columns that beat column y in the order of tfimm_hip_topk (a larger value, or an equal value
 *                  in a lower column; NaN above +inf, -0.0 == +0.0): rank < k exactly when y is in tfimm_hip_topk(..., k)'s
 *                  indices, at position rank.  tf.math.in_top_k counts every tie with the k-th value as a hit; this follows
 *                  tf.math.top_k instead, so that the library's two answers agree: in an all-equal row only class 0 has rank 0.
 *   pred  int32    the first maximum (tf.argmax); indices[b][0] of tfimm_hip_topk
 *   prob  float32  exp(x_y - m) / sum: the arithmetic of tfimm_hip_topk, bit-equal to its probs[b][rank] whenever rank < k
 * Labels: y == TFIMM_SCORE_IGNORE (the padded tail of a dataset's last batch) is not scored: loss = 0, prob = 0, rank = -1;
 * y < -1 or y >= N likewise with rank = -2.  pred is written for every row.  No column outside [0, N) is read whatever the
 * label holds.  tests/score_ref.py restates the rule on the CPU.
 * Accumulators, each updated by the same launch when its pointer is not NULL, with 64- / 32-bit INTEGER atomic adds issued by
 * one thread per row -- integer adds commute, so the contents after any sequence of launches are bit-identical whatever the
 * split into batches, the order of the rows, or the scheduling.  The caller zeroes them.
 *   state      int64 [TFIMM_SCORE_STATE_WORDS]:
 *                [TFIMM_SCORE_SCORED]  rows with a label in [0, N)     [TFIMM_SCORE_IGNORED]  rows with label -1
 *                [TFIMM_SCORE_INVALID] rows with any other label       [TFIMM_SCORE_LOSS_EXCLUDED]  scored rows for which
 *                loss < 1024.0f is false (NaN, inf, absurd): left out of the loss sum, their rank still counts
 *                [TFIMM_SCORE_LOSS_Q]  sum of rint((double)loss * 2^32) over the other scored rows: at most 2^42 units per
 *                row, so the int64 sum cannot overflow within 2^21 rows at that cap (at a loss of 16 per row: 2^27 rows)
 *                [TFIMM_SCORE_RANK_HIST + r]  rows with rank == r < 64; [TFIMM_SCORE_RANK_HIST + 64] every higher rank
 *   per_class  int64 [2][N]: [0][y] += 1, [1][y] += (rank == 0), over scored rows
 *   confusion  uint32 [N][N]: [y][pred] += 1 over scored rows; N <= TFIMM_SCORE_MAX_CONFUSION_N (64 MB)
 * One workgroup of 256 threads per row, the row read once and kept in LDS (the loader, the keys and the sum of
 * tfimm_hip_topk: csrc/topk_row.h), hence N <= TFIMM_SCORE_MAX_N; one selection round, then one pass over LDS for the sum and
 * the rank.  No allocation, capturable; a row's four outputs do not depend on B.  TFIMM_EINVAL before any launch, naming the
 * argument: NULL logits / labels / loss / rank / pred / prob; a pointer that is not 4-byte (state, per_class: 8-byte)
 * aligned; N outside [1, TFIMM_SCORE_MAX_N]; ld < N; B < 0; confusion with N > TFIMM_SCORE_MAX_CONFUSION_N.  B == 0 returns 0
 * and launches nothing.  Float32 logits under every precision mode: no tfimm_hip_ref_* twin.
 * Replaces, in a caller of the reference (tfimm/train/problems/classification.py): logits to the host, softmax_loss and
 * tf.argmax there. */
#define TFIMM_SCORE_MAX_N TFIMM_TOPK_MAX_N
#define TFIMM_SCORE_MAX_CONFUSION_N 4096
#define TFIMM_SCORE_IGNORE (-1)
#define TFIMM_SCORE_SCORED 0
#define TFIMM_SCORE_IGNORED 1
#define TFIMM_SCORE_INVALID 2
#define TFIMM_SCORE_LOSS_EXCLUDED 3
#define TFIMM_SCORE_LOSS_Q 4
#define TFIMM_SCORE_RANK_HIST 5
#define TFIMM_SCORE_RANK_BINS 65
#define TFIMM_SCORE_STATE_WORDS 70
TFIMM_API int tfimm_hip_score(const float* logits, int64_t ld, int B, int N, const int32_t* labels, float* loss, int32_t* rank,
                              int32_t* pred, float* prob, int64_t* state, int64_t* per_class, uint32_t* confusion, void* stream);

/* =======================================================================================
 * HEAD FIT (csrc/head_fit.hip): one optimizer step of a classifier head on frozen features, in two launches behind the
 * logits product -- the linear probe of a pretrained backbone (tfimm.LinearProbe; the CPU restatement of
 * both rules is tests/head_fit_ref.py).  Both are asynchronous on `stream` and capturable, allocate nothing, use no atomics
 * and are bit-reproducible from launch to launch; offsets are 64-bit; B == 0 returns 0 and launches nothing.  Float32
 * logits and master weights under every precision mode: no tfimm_hip_ref_* twin.
 * ======================================================================================= */

/* tfimm_hip_softmax_grad: per row of logits [B][ld] (float32, N <= ld valid columns) and its label labels[b]:
 *   grad  bf16 [B][ldg]  grad[b][c] = bf16_rne(p_c - [c == y_b]), p_c = exp(x_c - m) / sum: the softmax of tfimm_hip_score
 *                        (loader, maximum and sum of csrc/topk_row.h, prob's expression).  A row whose label is -1 or
 *                        outside [0, N) gets +0.0 in every column.  Only columns [0, N) are written.
 *   loss  float32 [B], pred int32 [B]: tfimm_hip_score's loss and pred, bit for bit.
 * One workgroup of 256 threads per row, the row read once and kept in LDS, hence N <= TFIMM_SCORE_MAX_N.
 * TFIMM_EINVAL before any launch, naming the argument: a NULL pointer; logits / labels / loss / pred not 4-byte aligned; grad
 * not 16-byte aligned; N outside [1, TFIMM_SCORE_MAX_N]; ld < N; ldg < N or ldg % 8 != 0; B < 0.
 * Replaces, in a caller of the reference (tfimm/train/problems/classification.py): the backward pass of softmax_loss. */
TFIMM_API int tfimm_hip_softmax_grad(const float* logits, int64_t ld, int B, int N, const int32_t* labels, void* grad, int64_t ldg,
                                     float* loss, int32_t* pred, void* stream);

/* tfimm_hip_head_update: the weight gradient of a Dense head and the optimizer step on it in ONE launch; the gradient lives in
 * the matrix unit's accumulators only.
 *   f        bf16    [B][ldf]     features, D columns
 *   g        bf16    [B][ldg]     tfimm_hip_softmax_grad's rows, C columns
 *   labels   int32   [B]          read only to count n = labels in [0, C)
 *   w        float32 [C][ldw]     master weights, the head's kernel transposed (the Wt[N][K] layout of tfimm_hip_gemm); in place
 *   w16      bf16    [C][ldw16]   the shadow tfimm_hip_gemm reads; rewritten
 *   s1, s2   float32 [C][ldw]     optimizer slots, in place (sgd: momentum, s2 unused and may be NULL; adam: m and v)
 *   bias, bias_s1, bias_s2  float32 [C]   the same for the bias (no shadow)
 *   grad_out float32 [C][ldw], bias_grad_out float32 [C]: optional, receive gd
 *
 *   acc[c][d] = sum_b g[b][c] * f[b][d]    matrix unit, float32 accumulation, b ascending
 *   accb[c]   = sum_b g[b][c]              float32, in a fixed order
 *   inv_n = 1.0f / (float)max(n, 1)
 *   gd = acc * inv_n
 *   gr = gd + wd2 * w                      wd2 = 2 * weight_decay
 *   opt == TFIMM_HEAD_SGD   s1 = mom * s1 - lr * gr ;  w = w + s1                                 (keras SGD, no nesterov)
 *   opt == TFIMM_HEAD_ADAM  s1 = s1 + (gr - s1) * one_minus_b1 ;  s2 = s2 + (gr * gr - s2) * one_minus_b2 ;
 *                           w = w - (s1 * lr) / (sqrt(s2) + eps)          (keras Adam; lr is the caller's alpha_t)
 *   w16 = bf16_rne(w)
 * Behind acc every operation is one correctly rounded float32 operation in the order written: nothing contracts to a fused
 * multiply-add, division and square root are the IEEE ones.  mom_or_one_minus_b1 is mom for sgd and 1 - beta1 for adam.
 * An all-ignored batch (n == 0) is a defined step: gd is zero, weight decay and slot decay act.
 * Each workgroup owns one 32 x 128 tile of w, walks the whole batch with the accumulators in registers and updates its tile
 * in place.  Rows >= B and columns >= C / >= D of a ragged tile are masked: no element outside [0, B) x [0, C) of g or
 * [0, B) x [0, D) of f is read, padding columns of every output are left alone.
 * TFIMM_EUNSUP: D % 8 != 0 or outside [8, TFIMM_HEAD_MAX_D], C outside [1, TFIMM_HEAD_MAX_C], B > TFIMM_HEAD_MAX_B.
 * TFIMM_EINVAL: a NULL descriptor or required pointer (adam: s2 and bias_s2), B < 0, an unknown opt, a pitch below its row,
 * ldf / ldg / ldw16 not a multiple of 8, ldw not a multiple of 4, f / g / w / w16 / s1 / s2 / grad_out not 16-byte aligned,
 * labels / bias* not 4-byte aligned, any output overlapping another operand.  No launch is made in either case. */
#define TFIMM_HEAD_SGD 0
#define TFIMM_HEAD_ADAM 1
#define TFIMM_HEAD_MAX_D 8192
#define TFIMM_HEAD_MAX_C 32768
#define TFIMM_HEAD_MAX_B 65535
typedef struct tfimm_head_update_desc {
  const void* f;
  const void* g;
  const int32_t* labels;
  float* w;
  void* w16;
  float* s1;
  float* s2;
  float* bias;
  float* bias_s1;
  float* bias_s2;
  float* grad_out;
  float* bias_grad_out;
  int32_t B, D, C;
  int32_t ldf, ldg, ldw, ldw16;
  int32_t opt;
  float lr, mom_or_one_minus_b1, one_minus_b2, eps, wd2;
} tfimm_head_update_desc;
TFIMM_API int tfimm_hip_head_update(const tfimm_head_update_desc* d, void* stream);

/* tfimm_hip_distill_grad (csrc/distill.hip; the CPU restatement is tests/distill_ref.py): the loss of the
 * reference's DistillationProblem behind a student's embedding head and its gradient with respect to the student's
 * embeddings, as the bf16 rows tfimm_hip_head_update takes for g -- the launch between tfimm_hip_gemm and
 * tfimm_hip_head_update in a step of tfimm.EmbeddingProbe.  Per row b, student s[b][0:E] and teacher t[b][0:E], float32:
 *   inv_s = 1 / sqrt(max(sum_e s_e^2, 1e-12)),  u = s * inv_s ;  inv_t and v from t alike (tfimm_hip_l2_normalize's rule,
 *   IEEE square root and division)
 *   cosine[b] = sum_e u_e v_e, formed as c = ((sum_e s_e t_e) * inv_s) * inv_t, under either value of `normalize`
 *   normalize == 1:  loss[b] = sum_e (u_e - v_e)^2 ;  d loss / d s_e = 2 * inv_s * (c * u_e - v_e).
 *                    A row with sum s^2 < 1e-12 is under the clamp: inv_s is the constant 1e6 there and the derivative is the
 *                    clamp's own, 2 * inv_s * (u_e - v_e).
 *   normalize == 0:  loss[b] = sum_e (s_e - t_e)^2 ;  d loss / d s_e = 2 * (s_e - t_e)
 *   grad  bf16 [B][ldg]   grad[b][e] = bf16_rne(d loss / d s_e) for e < E; columns [E, ldg) are never written
 *   loss, cosine  float32 [B]
 *   valid int32 [B]       0: train on the row; -1: ignore it.  An ignored row gets +0.0 in every gradient column, loss = 0
 *                         and cosine = 0, and its s and t are not read.  The same array is handed to tfimm_hip_head_update
 *                         as `labels` with C = E, and the division by the number of trained rows is done THERE, not here;
 *                         so that the two launches can never disagree about a row, this one trains on exactly the rows
 *                         head_update counts: valid[b] in [0, E).
 * One wave per row; each of the four sums of a row is formed in a fixed order (per lane over its columns ascending, then a
 * six-step butterfly) that depends on E alone -- not on B, not on the workgroup that holds the row, not on the alignment of
 * s and t.  Asynchronous on `stream` and capturable, no allocation, no atomics, 64-bit offsets, bit-reproducible.
 * Non-finite inputs are not detected: they propagate into the row's outputs (and from there into the weights).
 * TFIMM_EINVAL before any launch, naming the argument: a NULL pointer; s / t / valid / loss / cosine not 4-byte aligned; grad
 * not 16-byte aligned; ld_s < E; ld_t < E; ldg < E or ldg % 8 != 0; E outside [1, TFIMM_DISTILL_MAX_E]; B < 0; normalize
 * outside {0, 1}.  B == 0 returns 0 and launches nothing.  Float32 under every precision mode: no tfimm_hip_ref_* twin.
 * Replaces, in a caller of the reference (tfimm/train/problems/distillation.py): the loss of train_step_inner and its
 * backward pass down to the embeddings. */
#define TFIMM_DISTILL_MAX_E 4096
TFIMM_API int tfimm_hip_distill_grad(const float* s, int64_t ld_s, const float* t, int64_t ld_t, int B, int E, const int32_t* valid,
                                     int normalize, void* grad, int64_t ldg, float* loss, float* cosine, void* stream);

/* =======================================================================================
 * EMBEDDING END (csrc/embed.hip): row normalisation of float32 embeddings, and the search of a bf16 gallery
 * ======================================================================================= */

/* tfimm_hip_l2_normalize: y[b][:] = x[b][:] * (1 / sqrt(max(sum_e x[b][e]^2, 1e-12))) for B rows of E float32 values
 * (tf.math.l2_normalize, axis = -1); x [B][ld_x], y [B][ld_y], ld >= E; y may be x.
 * One wave per row: per-lane partial sums over columns lane, lane + 64, ... in ascending order, a fixed six-step butterfly,
 * correctly rounded square root and division.  No atomics, no allocation, capturable; bit-reproducible, a row's result does
 * not depend on B.  TFIMM_EINVAL before any launch for null x / y, E < 1, ld_x < E, ld_y < E, B < 0; B == 0 launches nothing.
 * Float32 under every precision mode: no tfimm_hip_ref_* twin. */
TFIMM_API int tfimm_hip_l2_normalize(const float* x, int64_t ld_x, int B, int E, float* y, int64_t ld_y, void* stream);

/* tfimm_hip_embed_search: for each of B float32 queries q [B][ld_q] the k rows of the bf16 gallery g [N][ld_g] with the largest
 * inner product.  The queries are rounded to bf16 (nearest even), score[b][n] = sum_e q16[b][e] * g[n][e] accumulated in
 * float32 by the matrix unit.
 *   scores  float32 [B][k]   the selected scores
 *   indices int32   [B][k]   their gallery rows
 * Order: score descending, equal scores by ascending gallery row (the order of tfimm_hip_topk).  Specified for finite
 * inputs; others do not fault.  tests/embed_ref.py restates the rule on the CPU.
 * Two launches on `stream`: pass 1 scores `chunk` gallery rows per workgroup against 32 queries and leaves k candidates per
 * (query, chunk) in `workspace`; pass 2 selects k of them per query.  The B x N score matrix never exists.  chunk == 0: the
 * library chooses; otherwise a positive multiple of 32 with ceil(N / chunk) * k <= 16384.  The result does not depend on
 * chunk, on B, or on which queries share a call: bit-reproducible, no atomics, no scratch memory, capturable.
 * Limits: E a multiple of 16 in [TFIMM_EMBED_MIN_E, TFIMM_EMBED_MAX_E]; 1 <= k <= min(N, TFIMM_EMBED_MAX_K); 1 <= N < 2^31;
 * 0 <= B <= TFIMM_EMBED_MAX_B (query tiles of 32 are one grid dimension);
 * ld_q >= E; ld_g >= E and a multiple of 8 elements; g 16-byte aligned, q / scores / indices / workspace 4-byte aligned;
 * workspace_bytes >= tfimm_hip_embed_search_workspace(B, N, E, k, chunk); offsets are 64-bit.  Everything else is
 * TFIMM_EINVAL before any launch, with a message naming the argument.  B == 0 returns 0 and launches nothing.
 * tfimm_hip_embed_search_workspace returns the bytes of workspace a call with these arguments needs (TFIMM_EINVAL, negative,
 * for arguments the search would refuse).
 * Replaces, behind an embedding model: tf.matmul(emb, gallery, transpose_b=True) + tf.math.top_k. */
#define TFIMM_EMBED_MIN_E 16
#define TFIMM_EMBED_MAX_E 2048
#define TFIMM_EMBED_MAX_K 64
#define TFIMM_EMBED_MAX_B 2097120 /* 65535 * 32 */
TFIMM_API int64_t tfimm_hip_embed_search_workspace(int B, int N, int E, int k, int chunk);
TFIMM_API int tfimm_hip_embed_search(const float* q, int64_t ld_q, int B, const void* g, int64_t ld_g, int N, int E, int k, int chunk,
                                     float* scores, int32_t* indices, void* workspace, int64_t workspace_bytes, void* stream);

/* tfimm_hip_embed_search_wide (csrc/embed_wide.hip): tfimm_hip_embed_search for up to
 * TFIMM_EMBED_WIDE_MAX_K neighbours per query -- the same arguments, the same rule (tests/embed_ref.py), the same order, and
 * the same bits: the scores come from the same loop (csrc/embed_score.h) and the selection is by the same total order, so
 * wherever both entry points accept a call their scores and indices are bit-equal.
 * Two launches on `stream`.  Pass 1 scores `chunk` gallery rows per workgroup against 32 queries; every query owns an unsorted
 * buffer of cap (key, row) pairs in LDS with a threshold, a score that beats the threshold takes a slot by an integer LDS
 * atomic, and the workgroup prunes every buffer to its k best whenever one could overflow in the next 128 rows; k pairs per
 * (query, chunk) go to `workspace`, unsorted.  Pass 2 streams them through one buffer per query and orders the k survivors by
 * rank.  What a prune keeps is the k best of the buffer's content under a total order, whatever the order of arrival: the
 * result does not depend on chunk, on B, on which queries share a call or on timing; bit-reproducible, no float atomics, no
 * scratch memory, no allocation, capturable.  The B x N score matrix never exists.
 * chunk == 0: the library chooses (never fewer than 4 k rows, in multiples of 128); otherwise a positive multiple of 32.  There
 * is no limit on ceil(N / chunk).
 * Limits: 1 <= k <= min(N, TFIMM_EMBED_WIDE_MAX_K); E, N, B, ld_q, ld_g and alignment as for tfimm_hip_embed_search; and the
 * buffers must fit LDS next to the query tile: 32 (2 E + 16) + 32 * 8 * cap <= 160 KiB with cap >= k + 128 (the library takes
 * cap = k + 256 where that fits without costing a workgroup per CU) -- every k <= 256 up to E = 768, k <= 254 at E = 1024, none at E = 2048.
 * tfimm_hip_embed_search_wide_max_k(E) returns the largest k this E allows, 0 or less where there is none (and 0 for an E
 * outside the domain); a (E, k) pair that does not fit is TFIMM_EINVAL with a message naming both.
 * workspace_bytes >= tfimm_hip_embed_search_wide_workspace(B, N, E, k, chunk) (TFIMM_EINVAL, negative, for arguments the
 * search would refuse).  Everything else is TFIMM_EINVAL before any launch, with a message naming the argument.  B == 0
 * returns 0 and launches nothing. */
#define TFIMM_EMBED_WIDE_MAX_K 256
TFIMM_API int tfimm_hip_embed_search_wide_max_k(int E);
TFIMM_API int64_t tfimm_hip_embed_search_wide_workspace(int B, int N, int E, int k, int chunk);
TFIMM_API int tfimm_hip_embed_search_wide(const float* q, int64_t ld_q, int B, const void* g, int64_t ld_g, int N, int E, int k,
                                          int chunk, float* scores, int32_t* indices, void* workspace, int64_t workspace_bytes,
                                          void* stream);

/* tfimm_hip_embed_quantize_rows / tfimm_hip_embed_search_coarse (csrc/embed_coarse.hip; the CPU restatement of
 * the rule is tests/coarse_ref.py): a coarse-to-fine search.  The gallery is scanned as one OCP e4m3fn byte per element, the
 * scan keeps `candidates` rows per query, and only those are scored in bf16 by the loop of tfimm_hip_embed_search: a returned
 * score has the bits the exact searches give for that row, and where the candidates contain the true top k the whole result
 * is bit-equal to theirs.  The order of rows is untouched and nothing depends on a clustering.
 *
 * tfimm_hip_embed_quantize_rows: for each of N bf16 rows g [N][ld_g] of E values, a = max |g_e|, exps[n] = 0 if a == 0 and
 * otherwise ceil(log2(a / 448)) clamped to [-126, 126], codes[n][e] = e4m3fn(g[n][e] * 2^-exps[n]), round to nearest even.
 * The scale is a power of two, so scaling is exact, and nothing saturates.  codes uint8 [N][ld_c], ld_c >= E bytes and a
 * multiple of 16; exps int8 [N].  One wave per row, every row read once, nothing written behind E code bytes of a row.  A
 * non-finite entry becomes the NaN code 0x7f with its sign.  g and codes 16-byte aligned; E and ld_g as for
 * tfimm_hip_embed_search; 0 <= N < 2^31, N == 0 launches nothing.  Rows may be quantised in any number of calls.
 *
 * tfimm_hip_embed_search_coarse: q, g, scores, indices as for tfimm_hip_embed_search; codes / exps the quantised rows of g.
 *   coarse key (b, n) = (float32 MFMA sum over e of code(q16[b])[e] * codes[n][e], from a zero accumulator) * 2^exps[n], the
 *   query rounded to bf16 and quantised by the rule above (its own exponent, a positive constant per query, is not applied);
 *   the `candidates` best rows per query by key descending, equal keys by ascending row; their exact scores; the k best of
 *   those by score descending, equal scores by ascending row.
 * Three launches on `stream`: pass 1 is pass 1 of tfimm_hip_embed_search_wide over the codes with k = candidates (the query
 * tile as fp8 in LDS, v_mfma_f32_32x32x16_fp8_fp8), pass 2 merges the chunks, pass 3 scores the candidates of a query with
 * the bf16 loop and ranks the k best by counting.  The result does not depend on B, on chunk, on which queries share a call
 * or on timing; no float atomics, no scratch memory, no allocation, capturable.
 * Gallery rows are assumed finite.  A row with a non-finite entry has a NaN key, which orders above every number, as a NaN
 * score does in the exact searches: it is a candidate of every query (while there are no more than `candidates` such rows) and
 * is then scored exactly; nothing faults or hangs.
 * Limits: E, B, N, ld_q, ld_g, chunk and alignment as for tfimm_hip_embed_search_wide; ld_c >= E and a multiple of 16 bytes,
 * codes 16-byte and exps 4-byte aligned; 1 <= k <= candidates <= min(N, tfimm_hip_embed_search_coarse_max_candidates(E)), which
 * is what LDS holds next to the fp8 query tile -- 32 (E + 16) + 32 * 8 * cap <= 160 KiB with cap >= candidates + 128, at most
 * TFIMM_EMBED_COARSE_MAX_CANDIDATES: 256 up to E = 2032, 254 at E = 2048 (0 for an E outside the domain).
 * workspace_bytes >= tfimm_hip_embed_search_coarse_workspace(B, N, E, k, candidates, chunk) (TFIMM_EINVAL, negative, for
 * arguments the search would refuse).  Everything else is TFIMM_EINVAL before any launch, with a message naming the
 * argument.  B == 0 returns 0 and launches nothing. */
#define TFIMM_EMBED_COARSE_MAX_CANDIDATES 256
TFIMM_API int tfimm_hip_embed_quantize_rows(const void* g, int64_t ld_g, int N, int E, void* codes, int64_t ld_c, int8_t* exps,
                                            void* stream);
TFIMM_API int tfimm_hip_embed_search_coarse_max_candidates(int E);
TFIMM_API int64_t tfimm_hip_embed_search_coarse_workspace(int B, int N, int E, int k, int candidates, int chunk);
TFIMM_API int tfimm_hip_embed_search_coarse(const float* q, int64_t ld_q, int B, const void* g, int64_t ld_g, const void* codes,
                                            int64_t ld_c, const int8_t* exps, int N, int E, int k, int candidates, int chunk,
                                            float* scores, int32_t* indices, void* workspace, int64_t workspace_bytes, void* stream);

/* tfimm_hip_embed_search_lists (csrc/embed_lists.hip; the CPU restatement of the rule is tests/index_ref.py): the
 * gallery search over INVERTED LISTS -- only the rows of the lists a query names are scored.  The caller holds the index:
 *   g       bf16  [N][ld_g]  the gallery rows IN LIST ORDER: list l is positions offsets[l] : offsets[l + 1]
 *   ids     int32 [N]        the original row of every position, ascending inside a list
 *   offsets int32 [L + 1]    ascending (a CSR form)
 *   probes  int32 [B][ld_p]  per query the nprobe lists to search; an entry outside [0, L) (-1: "no list") contributes nothing
 * q, scores, indices as for tfimm_hip_embed_search.  The candidates of a query are the rows of its lists; the result is the k
 * best of them by score descending, equal scores by ascending ORIGINAL row (indices holds ids, not positions), the score
 * being sum_e q16[b][e] * row[e] from the loop of tfimm_hip_embed_search (csrc/embed_score.h): a returned score has the bits
 * that entry point gives for that row.  Where the lists hold fewer than k rows the remaining slots hold index -1 and score
 * -inf.  The lists of one query are meant to be distinct; a list named more than once counts ONCE (every later entry that
 * repeats an earlier one of the same query is "no list"), so a row is never returned twice.
 * Out-of-range input does not fault: offsets are clamped to [0, N], a list whose end is below its begin is empty, ids are
 * copied and never used as an address.  The order is specified for ids that ascend inside every list.
 * Two launches on `stream`.  Pass 1, grid (nprobe * parts, B): one workgroup scores the p-th of `parts` equal cuts
 * (ceil(len / parts) rows each) of one list against one query held in LDS as bf16, keeps ONE unsorted buffer of k + 256
 * (key, position) pairs with a threshold (csrc/embed_buffer.h; the step structure of tfimm_hip_embed_search_wide) and leaves
 * its k best, with ids in place of positions, in `workspace`; it also writes the query's outputs as "none".  LDS is
 * 2 E + 16 + 8 (k + 256) bytes, about 8 KiB at most: many workgroups per CU.  Pass 2 merges the nprobe * parts * k pairs of a
 * query and orders the survivors by rank, as in tfimm_hip_embed_search_wide.
 * The result does not depend on B, on parts, on which queries share a call or on timing; bit-reproducible, no float atomics,
 * no scratch memory, no allocation, capturable; offsets are 64-bit.
 * parts == 0: the library chooses (1: it does not know the lists' lengths; the caller who does passes about len / 2048 of the
 * longest list).
 * Limits: E, ld_q, ld_g and alignment as for tfimm_hip_embed_search; 1 <= N < 2^31; 1 <= k <= TFIMM_EMBED_WIDE_MAX_K (k may
 * exceed the rows probed, and N); 1 <= nprobe <= TFIMM_EMBED_LISTS_MAX_PROBE; ld_p >= nprobe; 1 <= L <= TFIMM_CLUSTER_MAX_C;
 * 0 <= parts <= 64; 0 <= B <= 65535 (B is a grid dimension; nprobe * parts, the other, is at most 16384); ids / offsets / probes 4-byte aligned;
 * workspace_bytes >= tfimm_hip_embed_search_lists_workspace(B, N, E, L, nprobe, k, parts) = max(B, 1) * nprobe * parts * k * 8
 * (TFIMM_EINVAL, negative, for arguments the search would refuse).  Everything else is TFIMM_EINVAL before any launch, with a
 * message naming the argument.  B == 0 returns 0 and launches nothing. */
#define TFIMM_EMBED_LISTS_MAX_PROBE 256
TFIMM_API int64_t tfimm_hip_embed_search_lists_workspace(int B, int N, int E, int L, int nprobe, int k, int parts);
TFIMM_API int tfimm_hip_embed_search_lists(const float* q, int64_t ld_q, int B, const void* g, int64_t ld_g, int N, int E,
                                           const int32_t* ids, const int32_t* offsets, int L, const int32_t* probes, int64_t ld_p,
                                           int nprobe, int k, int parts, float* scores, int32_t* indices, void* workspace,
                                           int64_t workspace_bytes, void* stream);

/* tfimm_hip_embed_search_lists_grouped (csrc/embed_lists_grouped.hip): tfimm_hip_embed_search_lists -- the same
 * arguments in the same order, the same rule, the same result BIT FOR BIT -- with every probed list scored once for up to 32 of
 * the queries that name it: the 32 columns of the MFMA's B operand hold 32 different queries where the single-query kernel
 * repeats one.  For large batches (B * nprobe well above L) the gallery bytes read fall by up to 32.
 * A PAIR is (query b, probe slot s), P = B * nprobe of them; it is LIVE when probes[b][s] is in [0, L), no earlier slot of the
 * query names the same list and the list is not empty (offsets clamped to [0, N]).  Six launches on `stream`:
 *   fill    count[L] = 0 and every query's k outputs "none" (-1, -inf) -- a kernel, no memset;
 *   rank    every live pair takes a rank among the pairs of its list (an integer atomicAdd on count);
 *   scan    a list has ceil(count / 32) TILES: the first tile of every list and the total, one workgroup;
 *   place   a live pair becomes member rank % 32 of tile first[l] + rank / 32; any other pair writes its k * parts workspace
 *           entries as empty (key 0, row INT_MAX);
 *   pass 1  grid (T_max, parts): the number of tiles exists on the device only, so the launch takes the bound
 *           T_max = min(P / 32 + min(L, P), min(L, P) * ceil(B / 32)) (integer division; tfimm_hip_embed_search_lists_grouped_tiles)
 *           and a workgroup whose tile is not below the total returns at once.  A workgroup gathers the tile's queries into LDS
 *           as bf16, scores cut `part` (ceil(len / parts) rows, as in tfimm_hip_embed_search_lists) of the tile's list with the
 *           step loop of tfimm_hip_embed_search_wide -- one buffer of (key, position) pairs per query -- and leaves every
 *           member's k best at workspace[b][s * parts + part][k], the address and the set of the single-query kernel;
 *   pass 2  as in tfimm_hip_embed_search_lists.
 * The ranks differ from run to run; they move queries between tiles and lanes and no result bit depends on them.  No float
 * atomics, no scratch memory, no allocation, nothing goes to the host, capturable; offsets are 64-bit.
 * Limits: those of tfimm_hip_embed_search_lists, and k <= tfimm_hip_embed_search_wide_max_k(E) -- 32 buffers share LDS with the
 * query tile: 256 up to E = 768, 254 at E = 1024, none at E = 2048 (refused with a message that names that function).
 * workspace_bytes >= tfimm_hip_embed_search_lists_grouped_workspace(B, N, E, L, nprobe, k, parts)
 *   = max(B, 1) * nprobe * parts * k * 8 + 4 * (L + (L + 1) + P + T_max + 32 * T_max), P and T_max taken at max(B, 1):
 * the pair arrays of tfimm_hip_embed_search_lists, then count [L], first tile [L + 1] (the last entry: the total), rank [P], list
 * per tile [T_max] and members [T_max][32], all int32.  TFIMM_EINVAL (negative) for arguments the search would refuse; every
 * refusal comes before any launch with a message naming the argument.  B == 0 returns 0 and launches nothing.
 * tfimm_hip_embed_search_lists_grouped_tiles(B, L, nprobe) returns T_max (0 for B == 0), TFIMM_EINVAL for B, L or nprobe outside
 * the limits above. */
TFIMM_API int64_t tfimm_hip_embed_search_lists_grouped_tiles(int B, int L, int nprobe);
TFIMM_API int64_t tfimm_hip_embed_search_lists_grouped_workspace(int B, int N, int E, int L, int nprobe, int k, int parts);
TFIMM_API int tfimm_hip_embed_search_lists_grouped(const float* q, int64_t ld_q, int B, const void* g, int64_t ld_g, int N, int E,
                                                   const int32_t* ids, const int32_t* offsets, int L, const int32_t* probes,
                                                   int64_t ld_p, int nprobe, int k, int parts, float* scores, int32_t* indices,
                                                   void* workspace, int64_t workspace_bytes, void* stream);

/* tfimm_hip_matches_merge (csrc/embed_merge.hip; the CPU restatement of the rule is tests/live_ref.py::merge): the
 * k best of S SETS of matches per query -- what the searches of two galleries, of the shards of one, or of a GalleryIndex and of
 * the rows added behind it leave -- joined on the device.  Set s holds, for each of the B queries, k_s (index, score) entries at
 * pitch ld: `sets` is a HOST array that is read during the call; its contents travel as kernel arguments, so nothing of it is
 * referenced after the call returns.
 *   Entry j of set s in row b is a CANDIDATE iff indices[b][j] >= 0.  Its row is indices[b][j] + base_s (the caller keeps it
 *   below 2^31), its key the order-preserving key of its score (csrc/topk_select.h: every NaN ranks above +inf, the two zeros
 *   are equal).  scores / indices [b][0:k] receive the k best candidates of all sets, key descending, equal keys by ascending
 *   row; a score is written as the float its key stands for -- the bits every search here writes pass through unchanged, -0.0
 *   becomes +0.0 and any NaN the one quiet NaN --; the slots behind the last candidate hold index -1 and score -inf.  A
 *   candidate with score -inf is a candidate and comes before that fill.
 * Preconditions, documented and NOT checked: every set's row is as the searches leave it -- the valid entries first, in the
 * order above, -1 entries behind them --, and the rows of one query are pairwise distinct after `base`.  Where they do not hold
 * the result is unspecified; even then nothing outside scores / indices [B][k] is written.  Columns >= k_s of a set and columns
 * >= k of the outputs are never touched.  Outputs must not alias inputs.
 * One launch on `stream`, no workspace: one wave per query, four queries per workgroup, a grid-stride loop over the queries
 * (B is no grid dimension); the first min(k_s, k) entries of every set stand in LDS as 64-bit words, 8 * sum_s min(k_s, k) bytes
 * per wave (at most 64 KiB per workgroup), and an entry's place in the result is its position in its own set plus, per other
 * set, the entries that beat it: a binary search.  The result is a function of the candidate set alone: bit-reproducible,
 * independent of B and of which queries share a call; no atomics, no scratch memory, no allocation, capturable; offsets are
 * 64-bit.
 * TFIMM_EINVAL before any launch, with a message naming the argument: sets, scores or indices NULL; a set's scores or indices
 * NULL ("sets[1].indices is null"); any of those pointers not 4-byte aligned; S outside [1, TFIMM_MERGE_MAX_SETS]; k or a set's k
 * outside [1, TFIMM_EMBED_WIDE_MAX_K]; a set's ld < its k; ld_out < k; a negative base; B outside [0, TFIMM_EMBED_MAX_B].
 * B == 0 returns 0 and launches nothing. */
#define TFIMM_MERGE_MAX_SETS 8
typedef struct tfimm_match_set {
  const float*   scores;   /* [B][ld] */
  const int32_t* indices;  /* [B][ld] */
  int64_t ld;              /* >= k    */
  int32_t k;               /* columns of this set, 1 .. TFIMM_EMBED_WIDE_MAX_K */
  int32_t base;            /* >= 0: added to every valid index */
} tfimm_match_set;         /* 32 bytes */
TFIMM_API int tfimm_hip_matches_merge(const tfimm_match_set* sets, int S, int B, int k, float* scores, int32_t* indices,
                                      int64_t ld_out, void* stream);

/* =======================================================================================
 * KNN END (csrc/knn.hip; the CPU restatement of the rule is tests/knn_ref.py): the matches of a gallery
 * search turned into classes through a label per gallery row, in one launch behind tfimm_hip_embed_search.
 * Both entry points read, per query b, the candidates indices[b][0:k] (int32) and scores[b][0:k] (float32) of rows with
 * pitch ld -- columns >= k are never read -- the labels glabels[0:N] (int32) of the gallery rows and, when exclude is not
 * NULL, exclude[b] (int32; a value no candidate holds, -1 for one, excludes nothing).  Candidate j is VALID when
 * 0 <= indices[j] < N, indices[j] != exclude[b] and glabels[indices[j]] >= 0 (tfimm_hip_knn_score: and < nb_classes); no
 * label is read for an index outside [0, N); a candidate that is not valid contributes nothing.  Specified for finite scores.
 * One wave per query, four queries per workgroup of 256 threads, lane j owns candidate j; registers and cross-lane operations
 * only: no LDS, no float atomics, no allocation, capturable, 64-bit offsets.  Every sum runs over the candidates in ascending
 * j: results are bit-reproducible and a query's outputs do not depend on B.  Float32 under every precision mode: no
 * tfimm_hip_ref_* twin.
 * TFIMM_EINVAL before any launch, with a message naming the argument: a NULL required pointer; a pointer that is not 4-byte
 * (state, per_class: 8-byte) aligned; k outside [1, TFIMM_KNN_MAX_K]; ld < k; N < 1; B < 0; inv_temperature negative, NaN or
 * infinite; and what each entry point adds below.  B == 0 returns 0 and launches nothing.
 * ======================================================================================= */
#define TFIMM_KNN_MAX_K TFIMM_EMBED_MAX_K
#define TFIMM_KNN_MAX_TOP 64
#define TFIMM_KNN_SUM 0
#define TFIMM_KNN_MAX 1

/* tfimm_hip_knn_vote: per query the `top` best classes among its valid candidates.
 *   reduce == TFIMM_KNN_SUM: m = the largest valid score, w_j = expf((s_j - m) * inv_temperature) -- one float32
 *     subtraction, one float32 product, expf; inv_temperature == 0 makes every weight exactly 1, the majority vote --
 *     value[c] = the float32 sum of w_j over the valid candidates of class c in ascending j, count[c] their number,
 *     total[b] = the float32 sum of w_j over all valid candidates in ascending j.
 *   reduce == TFIMM_KNN_MAX: value[c] = the largest raw score among the candidates of class c (-0.0 == +0.0; of equal maxima
 *     the one at the lowest j is written), count[c] as above, total[b] = +0.0; inv_temperature is not used.  When the
 *     candidates are the k best rows of the whole gallery in the search's order, the classes of this list are exactly the top
 *     distinct identities of the gallery: an identity absent from the list has its best row below the k-th score.
 *   classes int32 [B][top], values float32 [B][top], counts int32 [B][top]: the classes by value descending, equal values by
 *     ascending class; slots beyond the number of distinct classes hold class -1, value +0.0, count 0.  total float32 [B].
 * Labels are any non-negative int32.  Also refused: NULL classes / values / counts / total; reduce not one of the two;
 * top outside [1, TFIMM_KNN_MAX_TOP].
 * Replaces, in a caller of the search: indices to the host, the label lookup and the vote (or the de-duplication) there. */
TFIMM_API int tfimm_hip_knn_vote(const int32_t* indices, const float* scores, int64_t ld, int B, int k, const int32_t* glabels,
                                 int N, const int32_t* exclude, float inv_temperature, int reduce, int top, int32_t* classes,
                                 float* values, int32_t* counts, float* total, void* stream);

/* tfimm_hip_knn_score: the TFIMM_KNN_SUM vote of each query scored against its true label labels[b], as tfimm_hip_score
 * scores a row of logits.  With v[0:nb_classes) the dense vote vector (v[c] = value[c] for voted classes, 0 otherwise):
 *   pred  int32    the first class in the order (value descending, equal values by ascending class): tfimm_hip_score's pred
 *                  on the row v; 0 when no candidate is valid
 *   rank  int32    the number of classes that beat class y in that order: tfimm_hip_score's rank on the row v.  An unvoted
 *                  class ties with a voted class whose weights underflowed to 0.  Counted from the (at most k) voted classes
 *                  alone -- those that beat y, and, when v[y] == 0, y minus the voted classes below y -- never by a loop over
 *                  nb_classes, which may be as large as 2^31 - 1.  With no valid candidate rank = y.
 *   prob  float32  v[y] / total, correctly rounded; 0 when total == 0
 *   loss  float32  0 - logf(prob): +inf at prob == 0 (nobody voted for the true class), +0.0 at prob == 1
 * y == TFIMM_SCORE_IGNORE is not scored: loss = 0, prob = 0, rank = -1; any other y outside [0, nb_classes) likewise with
 * rank = -2.  pred is written for every row.
 * state / per_class / confusion: the accumulators of tfimm_hip_score with N = nb_classes -- its layouts, its constants, its
 * integer atomic adds issued by one lane per query -- so that one meter can be fed by both; a +inf loss is counted in
 * TFIMM_SCORE_LOSS_EXCLUDED by that function's rule.  Each may be NULL.
 * Also refused: NULL labels / loss / rank / pred / prob; nb_classes < 1; confusion with nb_classes >
 * TFIMM_SCORE_MAX_CONFUSION_N.
 * Replaces, in a kNN evaluation of an embedding: indices to the host, the vote and the accuracy counters there. */
TFIMM_API int tfimm_hip_knn_score(const int32_t* indices, const float* scores, int64_t ld, int B, int k, const int32_t* glabels,
                                  int N, const int32_t* exclude, float inv_temperature, int nb_classes, const int32_t* labels,
                                  float* loss, int32_t* rank, int32_t* pred, float* prob, int64_t* state, int64_t* per_class,
                                  uint32_t* confusion, void* stream);

/* =======================================================================================
 * CLUSTER END (csrc/cluster.hip; the CPU restatement of both rules is tests/cluster_ref.py): the two device
 * operations of grouping a bf16 gallery -- every row to its best centroid, and the mean of the rows of every group.  The
 * Lloyd loop, class prototypes and pseudo-labels are host code over them (tfimm.Gallery.assign / prototypes / kmeans).
 * Both follow the conventions of the embedding and kNN ends: TFIMM_EINVAL before any launch, with a message naming the
 * argument; 64-bit offsets; no allocation, no float atomics, no scratch memory; capturable and bit-reproducible; float32 /
 * bf16 under every precision mode: no tfimm_hip_ref_* twin.
 * ======================================================================================= */
#define TFIMM_CLUSTER_MAX_C 65536
#define TFIMM_SEGMENT_RUN 256

/* tfimm_hip_cluster_assign: for each of the N rows of the bf16 gallery g [N][ld_g] (read in place) the best of the C bf16
 * centroids c [C][ld_c]: s[n][j] = sum_e g[n][e] * c[j][e], accumulated in float32 by the matrix unit;
 *   assign int32   [N]   the j with the largest s[n][j]; of equal scores the lowest j (-0.0 == +0.0)
 *   score  float32 [N]   that score
 * Specified for finite inputs; others do not fault.  One launch: a workgroup owns 128 gallery rows and streams the centroids
 * through LDS in tiles of 128; the running best of a row stays in registers, the N x C score matrix never exists, a row's 8
 * bytes are written once.  A score is a function of its row, its centroid and E alone: a row's outputs do not depend on N, on
 * which rows share a call or on how the centroids are tiled, and a centroid's score does not depend on C.
 * Limits: E a multiple of 16 in [TFIMM_EMBED_MIN_E, TFIMM_EMBED_MAX_E]; 1 <= C <= TFIMM_CLUSTER_MAX_C; 0 <= N < 2^31;
 * ld_g, ld_c >= E and multiples of 8 elements; g / c 16-byte aligned; assign / score 4-byte aligned.  N == 0 returns 0 and
 * launches nothing.
 * Replaces, in a k-means or nearest-class-mean loop: tf.matmul(gallery, centroids, transpose_b=True) + tf.argmax / reduce_max. */
TFIMM_API int tfimm_hip_cluster_assign(const void* g, int64_t ld_g, int N, const void* c, int64_t ld_c, int C, int E, int32_t* assign,
                                       float* score, void* stream);

/* tfimm_hip_segment_mean: the mean of the gallery rows of each of C segments.  Segment c is the list
 * rows[offsets[c] : offsets[c + 1]] of gallery row indices (rows int32 [M], offsets int32 [C + 1]: a CSR form).
 *   counts int32   [C]         the number of VALID entries of the segment: those inside [0, N)
 *   mean   float32 [C][ld_m]   the float32 sum of the segment's valid rows divided by float(count) in one correctly rounded
 *                              float32 division; an empty segment (or one without a valid entry): +0.0 and counts[c] = 0
 * Out-of-range input does not fault: an entry of rows outside [0, N) contributes nothing, is not counted, and no gallery row
 * is read for it; offsets are clamped to [0, M], and a segment whose end is below its begin is empty.  mean and counts are
 * specified for offsets that ascend from segment to segment (a CSR form); any other content does not fault, but the run slots
 * of two segments may then coincide and their sums mix.
 * THE ORDER OF THE ADDITIONS, per column, with R = TFIMM_SEGMENT_RUN: the segment's entries, valid or not, are cut into runs of
 * R counted from the segment's own begin -- run r holds the entries [begin + r R, min(begin + (r + 1) R, end)).  A run's
 * partial sum starts at +0.0 and adds the run's valid rows one by one in list order; the segment's sum starts at +0.0 and adds
 * the partial sums one by one in ascending run order.  Every addition is a single float32 addition.  The order is a function of
 * the segment's own entries in their list order alone: it does not depend on N, M, C, the other segments or the launch.
 * Two launches on `stream`: the partial sums of all runs -- the work is split by runs, not by segments, so one long segment
 * costs what many short ones do -- go to `workspace` (segment c owns the run slots from begin / R + c on; at most M / R + C
 * slots), then one pass per segment combines them.
 * Limits: E a multiple of 16 in [TFIMM_EMBED_MIN_E, TFIMM_EMBED_MAX_E]; 1 <= C < 2^31; 0 <= M < 2^31; 0 <= N < 2^31; ld_g >= E
 * and a multiple of 8 elements; ld_m >= E; g and workspace 16-byte aligned, rows / offsets / mean / counts 4-byte aligned;
 * rows may be NULL when M == 0; workspace_bytes >= tfimm_hip_segment_mean_workspace(M, C, E), which returns the bytes needed
 * (TFIMM_EINVAL, negative, for an M, C or E the call would refuse).
 * Replaces, in a k-means or class-prototype loop: tf.math.unsorted_segment_mean over gathered rows. */
TFIMM_API int64_t tfimm_hip_segment_mean_workspace(int M, int C, int E);
TFIMM_API int tfimm_hip_segment_mean(const void* g, int64_t ld_g, int N, int E, const int32_t* rows, int M, const int32_t* offsets,
                                     int C, float* mean, int64_t ld_m, int32_t* counts, void* workspace, int64_t workspace_bytes,
                                     void* stream);

/* =======================================================================================
 * LOW-RANK ADAPTER (csrc/lora.hip): the LoRA term of a Dense layer as an op of its own
 * ======================================================================================= */

/* tfimm_hip_lora_delta:
 *     t   = bf16( x[M][K] . A[K][R] )                      fp32 accumulation, ONE rounding of t
 *     out = bf16( residual[M][N] + t[M][R] . B'[R][N] )    fp32 accumulation, residual optional
 * in ONE launch; t lives in registers only (the accumulators of the first product are the matrix unit's operand of the
 * second).  The unmerged form of LoRADense.call (reference architectures/lora/layers.py:81-113): the caller folds
 * scaling = lora_alpha / lora_rank (and a LayerScale behind the layer) into B' and hands `out` to tfimm_hip_gemm as the
 * residual of the layer's full-rank product, so the adapter's weights stay apart from the layer's.
 *   x        bf16 [M][lda]
 *   a        bf16 [Rp][lda_a]   A transposed; rows >= the true rank are zero.  Rp a multiple of 16, 16 <= Rp <= TFIMM_LORA_MAX_RP
 *   b        bf16 [N][Rp]       B' transposed; columns >= the true rank are zero
 *   residual bf16 [M][ldr] or NULL
 *   out      bf16 [M][ldc]
 * Limits: K % 8 == 0, N % 8 == 0, 8 <= K, N <= TFIMM_LORA_MAX_DIM (TFIMM_EUNSUP otherwise, and for an Rp outside its set).
 * TFIMM_EINVAL: a null x / a / b / out, M < 0, a pitch below its row or not a multiple of 8 elements, a pointer that is not
 * 16-byte aligned, `out` overlapping any input.  No launch is made in either case; M == 0 returns 0 and launches nothing.
 * A row's result does not depend on M: no atomics, no workspace, capturable, bit-reproducible.  Offsets are 64-bit.
 * tests/lora_ref.py restates the contract in float64. */
#define TFIMM_LORA_MAX_RP 64
#define TFIMM_LORA_MAX_DIM 8192
typedef struct tfimm_lora_desc {
  const void* x;
  const void* a;
  const void* b;
  const void* residual;
  void* out;
  int64_t M;
  int32_t K, N, Rp;
  int32_t lda, lda_a, ldr, ldc;
} tfimm_lora_desc;
TFIMM_API int tfimm_hip_lora_delta(const tfimm_lora_desc* d, void* stream);

/* =======================================================================================
 * FLOAT32 VERIFICATION PATH (csrc/ref32.hip; selected by TFIMM_PRECISION=fp32, tfimm/engine/precision.py)
 *
 * The reference is float32 end to end and pins values at 1e-3 relative to the maximum (tests/test_timm.py:71).  The
 * entry points below run the SAME layer program as the bf16 kernels above -- same host-side lowering and weight
 * transformations, minus the cross-layer fusions -- with float32 activations, float32 GEMM weights (Wt[N][ldw] float)
 * and float32 accumulation, so that the engine's arithmetic can be held to the reference's own bar.  Plain kernels
 * (one thread / wave per output), 20-50x slower than the product path: a checker, not a fallback -- nothing selects
 * them unless the caller asks for fp32.  Every signature is the bf16 entry point's with `bf16` tensors replaced by
 * `float` (descriptor fields keep their meaning; tile_hint / ln_* / bias_log2 are ignored or refused).
 * tfimm_hip_se_gate and tfimm_hip_eca_gate are float32 already and serve both paths.
 * ======================================================================================= */
TFIMM_API int tfimm_hip_ref_gemm(const tfimm_gemm_desc* d, void* stream);   /* TFIMM_A_DENSE and TFIMM_A_CONV (any Cin) */
/* in_dtype: 0 float32, 1 bf16, 2 uint8 with out = ((float)v / 255 - mean[c]) / std[c] (models/factory.py:165-167);
 * mean / std: HOST arrays of c_in floats for uint8, NULL otherwise.  out: float32 [n_pixels][c_out], channels >= c_in zero. */
TFIMM_API int tfimm_hip_ref_cast_input(const void* in, int in_dtype, void* out, int64_t n_pixels, int c_in, int c_out,
                                       const float* mean, const float* std, void* stream);
/* tfimm_hip_preprocess_resize with a float32 `out` (same descriptor, same arithmetic minus the rounding to bf16) */
TFIMM_API int tfimm_hip_ref_preprocess_resize(const tfimm_resize_desc* d, void* stream);
/* tfimm_hip_preprocess_resize_aa with a float32 `out` */
TFIMM_API int tfimm_hip_ref_preprocess_resize_aa(const tfimm_resize_aa_desc* d, void* stream);
/* tfimm_hip_preprocess_resize_batch / _batch_aa with a float32 `out` (same descriptors, same device code) */
TFIMM_API int tfimm_hip_ref_preprocess_resize_batch(const tfimm_resize_batch_desc* d, void* stream);
TFIMM_API int tfimm_hip_ref_preprocess_resize_batch_aa(const tfimm_resize_batch_aa_desc* d, void* stream);
/* tfimm_hip_preprocess_regions / _regions_aa with a float32 `out` (same descriptors, same device code) */
TFIMM_API int tfimm_hip_ref_preprocess_regions(const tfimm_resize_region_desc* d, void* stream);
TFIMM_API int tfimm_hip_ref_preprocess_regions_aa(const tfimm_resize_region_aa_desc* d, void* stream);
TFIMM_API int tfimm_hip_ref_layernorm(const void* x, void* y, const float* gamma, const float* beta, int64_t rows, int d,
                                      int64_t x_stride, int64_t y_stride, float eps, void* stream);
TFIMM_API int tfimm_hip_ref_patch_merge_ln(const void* x, void* y, const float* gamma, const float* beta, int B, int H, int W,
                                           int C, float eps, void* stream);
TFIMM_API int tfimm_hip_ref_copy_rows(const void* src, void* dst, int B, int src_rows, int dst_rows, int dst_row0, int d,
                                      void* stream);
TFIMM_API int tfimm_hip_ref_bcast_rows(const void* src, void* dst, int B, int n_rows, int d, int dst_rows_per_image,
                                       void* stream);
TFIMM_API int tfimm_hip_ref_mean_rows(const void* x, void* y, int B, int R, int C, int out_f32, void* stream);
TFIMM_API int tfimm_hip_ref_scale_channels(const void* x, const float* gate, const void* residual, void* y, int B, int R,
                                           int C, int act_after, void* stream);
TFIMM_API int tfimm_hip_ref_maxpool(const void* x, void* y, int B, int H, int W, int C, int k, int stride, int pad, int OH,
                                    int OW, void* stream);
TFIMM_API int tfimm_hip_ref_avg_pool(const void* x, void* y, int B, int H, int W, int C, int k, int stride, void* stream);
TFIMM_API int tfimm_hip_ref_blur_pool(const void* x, void* y, int B, int H, int W, int C, int stride, void* stream);
/* sum_out must be NULL: on this path the SqueezeExcite mean is a tfimm_hip_ref_mean_rows launch */
TFIMM_API int tfimm_hip_ref_dwconv(const void* x, const float* w, const float* bias, void* y, void* sum_out, int B, int H,
                                   int W, int C, int k, int stride, int pad_t, int pad_l, int OH, int OW, int act,
                                   void* stream);
TFIMM_API int tfimm_hip_ref_group_norm(const void* x, const float* gamma, const float* beta, const void* residual, void* y,
                                       void* stats_ws, int B, int rows, int C, int groups, float eps, int act,
                                       int act_after_res, void* stream);
TFIMM_API int tfimm_hip_ref_attention(const tfimm_attn_desc* d, void* stream);
TFIMM_API int tfimm_hip_ref_attention_probs(const void* qkv, void* probs, int B, int n_tokens, int heads, int hd, float scale,
                                            void* stream);
TFIMM_API int tfimm_hip_ref_talking_heads_attention(const tfimm_tha_desc* d, void* stream);
TFIMM_API int tfimm_hip_ref_class_attention(const void* q, const void* kv, void* out, int B, int n_tokens, int heads, int hd,
                                            int ldq, int ldkv, int ldo, void* stream);
/* tfimm_hip_lora_delta on float32 tensors (x, a, b, residual, out all float, same descriptor, 4-byte alignment): t is NOT
 * rounded.  Same limits and refusals. */
TFIMM_API int tfimm_hip_ref_lora_delta(const tfimm_lora_desc* d, void* stream);

/* =======================================================================================
 * PROGRAM-LEVEL ENTRY POINTS (csrc/plan.hip): a whole forward behind three calls, for hosts without Python.
 *
 * Lowering a model configuration to the call sequence above (weight packing, buffer plan, tile selection) is host logic
 * (tfimm/engine/graph.py).  `Plan.export()` serialises the FINISHED plan of one (model, batch size) -- every call with its
 * arguments, the packed constants, the slab sizes, the named outputs -- into a self-contained blob; these functions run it
 * by calling the very same op-level entry points with the very same arguments (bit-identical results).  Conventions as
 * everywhere else: the caller owns the device memory (ONE workspace of tfimm_plan_info.workspace_bytes, 256-byte aligned),
 * every launch is asynchronous on `stream` and capturable into a hipGraph, nothing allocates on the device.
 *
 *   tfimm_hip_plan_query    parse the blob: workspace size, batch, input geometry
 *   tfimm_hip_plan_create   upload the constants into `workspace` (synchronises `stream` once; the blob may be freed
 *                           afterwards) and resolve every pointer of the call list
 *   tfimm_hip_plan_forward  input: [batch][in_h][in_w][in_c] NHWC, in_dtype 0 = float32, 1 = bf16 (device pointer)
 *   tfimm_hip_plan_output   where a named result lies ("logits", a feature name of a plan exported with features, or
 *                           "topk_values" / "topk_indices" / "topk_probs" of a plan exported with top_k):
 *                           device pointer into the workspace, rows (= batch * rows per image), columns, dtype (0 bf16, 1 f32,
 *                           2 int32)
 * A plan object is not re-entrant (one forward at a time); distinct plans are independent.
 * ======================================================================================= */
typedef void* tfimm_plan_t;
typedef struct tfimm_plan_info {
  uint64_t workspace_bytes;
  int32_t batch, in_h, in_w, in_c;
  int32_t n_calls, n_outputs;
} tfimm_plan_info;
TFIMM_API int tfimm_hip_plan_query(const void* blob, size_t bytes, tfimm_plan_info* info);
TFIMM_API int tfimm_hip_plan_create(const void* blob, size_t bytes, void* workspace, void* stream, tfimm_plan_t* plan);
TFIMM_API int tfimm_hip_plan_forward(tfimm_plan_t plan, const void* input, int in_dtype, void* stream);
TFIMM_API int tfimm_hip_plan_output(tfimm_plan_t plan, const char* name, void** ptr, int64_t* rows, int64_t* cols, int* dtype);
TFIMM_API int tfimm_hip_plan_destroy(tfimm_plan_t plan);

#ifdef __cplusplus
}
#endif
#endif /* TFIMM_HIP_H */

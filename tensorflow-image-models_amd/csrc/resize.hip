// Resize + centre crop + normalise of a uint8 image batch in ONE launch, written in the layouts of the input conversion
// kernels (rowops.hip: tfimm_hip_preprocess_input[_pad]).  Reference call sites: include/tfimm_hip.h.
//
// The arithmetic is fully specified (tf.image.resize(float32(img), method, antialias=False) restated tap by tap, then the
// three float32 operations of create_preprocessing), so the result is BIT-EQUAL to the host restatement:
//   * the tap tables -- source index and float32 weight of every output row / column -- are built on the HOST by
//     tfimm_hip_resize_taps below, the one place in C where the tap rule is written; the kernel computes none of it;
//   * every product and every sum is a separate float32 operation in the restatement's order.  This file is built with
//     -ffp-contract=off (csrc/Makefile) and carries the pragma below: nothing may contract to an FMA;
//   * a tap that falls outside the image is carried as weight +0.0 with its index clamped into the image: adding +0.0 is
//     exact, so dropping the tap (what the restatement does) and carrying it give the same bits.
// One thread per OUTPUT pixel and all its channels, no LDS: neighbouring threads re-read the same source row segments,
// which live in L2.  All offsets are 64-bit; every table index is clamped before use, so a bad table cannot read outside
// the image.
#include "common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int kResizeMaxBlocks = 256 * 16;  // grid-stride cap: 16 blocks per CU

struct ResizeArgs {
  const uint8_t* in;
  void* out;
  const int32_t* y_idx;
  const float* y_w;
  const int32_t* x_idx;
  const float* x_w;
  int B, Hs, Ws, c_in, H, W, c_out, pad_t, pad_l, HP, WP;
  int vec;  // bf16 only: 1 = one 8-byte store per pixel (c_out == 4), 2 = one 16-byte store (c_out == 8), 0 = element stores
  float mean[TFIMM_PREPROCESS_MAX_CHANNELS];
  float std[TFIMM_PREPROCESS_MAX_CHANNELS];
};

// TAPS == 4: bicubic, vertical pass first (sum over the 4 rows of every tap column), then the horizontal sum; each sum
//            starts at 0.0f and adds w * x in tap order (oracle/ops.py resize_bicubic_tf).
// TAPS == 2: bilinear as TensorFlow's compute_lerp: the two rows are interpolated horizontally, then vertically; the
//            weight of tap 1 is the fractional offset, the weight of tap 0 (its complement) is not used.
template <int TAPS, bool F32>
__global__ void __launch_bounds__(256) resize_kernel(ResizeArgs a) {
  constexpr int MAXC = TFIMM_PREPROCESS_MAX_CHANNELS;
  const int64_t total = (int64_t)a.B * a.HP * a.WP;
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (int64_t)gridDim.x * blockDim.x) {
    const int xp = (int)(id % a.WP);
    const int64_t t = id / a.WP;
    const int yp = (int)(t % a.HP);
    const int b = (int)(t / a.HP);
    const int y = yp - a.pad_t, x = xp - a.pad_l;
    float v[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) v[c] = 0.f;
    if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W) {
      float wy[TAPS], wx[TAPS];
      int64_t row[TAPS], col[TAPS];
#pragma unroll
      for (int k = 0; k < TAPS; ++k) {
        const int iy = min(max(a.y_idx[(int64_t)y * TAPS + k], 0), a.Hs - 1);
        const int ix = min(max(a.x_idx[(int64_t)x * TAPS + k], 0), a.Ws - 1);
        wy[k] = a.y_w[(int64_t)y * TAPS + k];
        wx[k] = a.x_w[(int64_t)x * TAPS + k];
        row[k] = (((int64_t)b * a.Hs + iy) * a.Ws) * a.c_in;
        col[k] = (int64_t)ix * a.c_in;
      }
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        if (c < a.c_in) {
          float r;
          if (TAPS == 4) {
            r = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float s = 0.f;
#pragma unroll
              for (int i = 0; i < 4; ++i) s = s + wy[i] * (float)a.in[row[i] + col[j] + c];
              r = r + wx[j] * s;
            }
          } else {
            const float tl = (float)a.in[row[0] + col[0] + c], tr = (float)a.in[row[0] + col[TAPS - 1] + c];
            const float bl = (float)a.in[row[TAPS - 1] + col[0] + c], br = (float)a.in[row[TAPS - 1] + col[TAPS - 1] + c];
            const float top = tl + (tr - tl) * wx[TAPS - 1];
            const float bottom = bl + (br - bl) * wx[TAPS - 1];
            r = top + (bottom - top) * wy[TAPS - 1];
          }
          v[c] = (r / 255.0f - a.mean[c]) / a.std[c];
        }
      }
    }
    if (F32) {
      float* o = reinterpret_cast<float*>(a.out) + id * a.c_out;
#pragma unroll
      for (int c = 0; c < MAXC; ++c)
        if (c < a.c_out) o[c] = v[c];
      for (int c = MAXC; c < a.c_out; ++c) o[c] = 0.f;
    } else if (a.vec == 1) {
      reinterpret_cast<uint2*>(a.out)[id] = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
    } else if (a.vec == 2) {
      reinterpret_cast<uint4*>(a.out)[id] = pack8(v);
    } else {
      bf16_t* o = reinterpret_cast<bf16_t*>(a.out) + id * a.c_out;
#pragma unroll
      for (int c = 0; c < MAXC; ++c)
        if (c < a.c_out) o[c] = (bf16_t)f2bf(v[c]);
      for (int c = MAXC; c < a.c_out; ++c) o[c] = (bf16_t)0;
    }
  }
}

int resize_launch(const tfimm_resize_desc* d, void* stream, bool f32, const char* who) {
  if (!d) TFIMM_FAIL(TFIMM_EINVAL, "%s: null descriptor", who);
  if (!d->in || !d->out || !d->y_idx || !d->y_w || !d->x_idx || !d->x_w || !d->mean_host || !d->std_host)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: null pointer", who);
  if (d->B <= 0 || d->Hs <= 0 || d->Ws <= 0 || d->c_in <= 0 || d->H <= 0 || d->W <= 0 || d->c_out <= 0)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: sizes must be positive (B=%d Hs=%d Ws=%d c_in=%d H=%d W=%d c_out=%d)", who, d->B, d->Hs,
               d->Ws, d->c_in, d->H, d->W, d->c_out);
  if (d->taps != 2 && d->taps != 4) TFIMM_FAIL(TFIMM_EINVAL, "%s: taps=%d, must be 2 (bilinear) or 4 (bicubic)", who, d->taps);
  if (d->c_in > TFIMM_PREPROCESS_MAX_CHANNELS || d->c_out < d->c_in)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: c_in=%d must be <= %d and <= c_out=%d", who, d->c_in, TFIMM_PREPROCESS_MAX_CHANNELS, d->c_out);
  if (d->pad_t < 0 || d->pad_b < 0 || d->pad_l < 0 || d->pad_r < 0) TFIMM_FAIL(TFIMM_EINVAL, "%s: negative pad", who);
  const bool padded = (d->pad_t | d->pad_b | d->pad_l | d->pad_r) != 0;
  if (padded && d->c_out != 4)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: the zero-bordered layout has 4 stored channels (c_in <= 4), got c_out=%d", who, d->c_out);
  ResizeArgs a;
  for (int c = 0; c < TFIMM_PREPROCESS_MAX_CHANNELS; ++c) {
    a.mean[c] = c < d->c_in ? d->mean_host[c] : 0.f;
    a.std[c] = c < d->c_in ? d->std_host[c] : 1.f;
    if (!(a.std[c] != 0.f)) TFIMM_FAIL(TFIMM_EINVAL, "%s: std[%d] == 0", who, c);
  }
  a.in = (const uint8_t*)d->in;
  a.out = d->out;
  a.y_idx = d->y_idx; a.y_w = d->y_w; a.x_idx = d->x_idx; a.x_w = d->x_w;
  a.B = d->B; a.Hs = d->Hs; a.Ws = d->Ws; a.c_in = d->c_in; a.H = d->H; a.W = d->W; a.c_out = d->c_out;
  a.pad_t = d->pad_t; a.pad_l = d->pad_l;
  a.HP = d->H + d->pad_t + d->pad_b;
  a.WP = d->W + d->pad_l + d->pad_r;
  a.vec = 0;
  if (!f32 && d->c_out == 4 && ((uintptr_t)d->out & 7) == 0) a.vec = 1;
  if (!f32 && d->c_out == 8 && ((uintptr_t)d->out & 15) == 0) a.vec = 2;
  const int64_t total = (int64_t)a.B * a.HP * a.WP;
  int64_t blocks = (total + 255) / 256;
  if (blocks > kResizeMaxBlocks) blocks = kResizeMaxBlocks;
  const dim3 grid((unsigned)blocks), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (d->taps == 4) {
    if (f32) TFIMM_LAUNCH((resize_kernel<4, true>), grid, block, 0, st, a);
    else TFIMM_LAUNCH((resize_kernel<4, false>), grid, block, 0, st, a);
  } else {
    if (f32) TFIMM_LAUNCH((resize_kernel<2, true>), grid, block, 0, st, a);
    else TFIMM_LAUNCH((resize_kernel<2, false>), grid, block, 0, st, a);
  }
  return 0;
}

// Keys cubic convolution kernel, A = -0.5, at table position i / 1024 (tensorflow/core/kernels/image/resize_bicubic_op.cc;
// oracle/ops.py resize_bicubic_tf: near / far) -- float32 operation by float32 operation
inline float keys_near(int i) {
  const float t = (float)i / 1024.0f;
  return (1.5f * t - 2.5f) * t * t + 1.0f;
}
inline float keys_far(int i) {
  const float t = (float)i / 1024.0f + 1.0f;
  return ((-0.5f * t + 2.5f) * t - 4.0f) * t + 2.0f;
}

}  // namespace

extern "C" int tfimm_hip_resize_taps(int n_in, int n_resized, int first, int n_out, int method, int32_t* idx_host,
                                     float* w_host) {
  if (!idx_host || !w_host) TFIMM_FAIL(TFIMM_EINVAL, "resize_taps: null pointer");
  if (n_in <= 0 || n_resized <= 0 || first < 0 || n_out <= 0 || (int64_t)first + n_out > n_resized)
    TFIMM_FAIL(TFIMM_EINVAL, "resize_taps: bad window (n_in=%d n_resized=%d first=%d n_out=%d)", n_in, n_resized, first, n_out);
  if (method != 0 && method != 1) TFIMM_FAIL(TFIMM_EINVAL, "resize_taps: method=%d, must be 0 (bilinear) or 1 (bicubic)", method);
  const float scale = (float)n_in / (float)n_resized;
  for (int k = 0; k < n_out; ++k) {
    const float loc = ((float)(first + k) + 0.5f) * scale - 0.5f;   // half-pixel centres
    const float fl = floorf(loc);
    const int base = (int)fl;
    if (method == 0) {
      // lo = max(floor(loc), 0), hi = min(ceil(loc), n_in - 1), frac = loc - floor(loc): the kernel evaluates
      // lo + (hi - lo) * frac (compute_lerp); the weight of tap 0 is the complement, for readers of the table
      const int hi = (int)ceilf(loc);
      const float frac = loc - fl;
      idx_host[2 * k] = base > 0 ? base : 0;
      idx_host[2 * k + 1] = hi < n_in - 1 ? hi : n_in - 1;
      w_host[2 * k] = 1.0f - frac;
      w_host[2 * k + 1] = frac;
    } else {
      const int off = (int)nearbyintf((loc - fl) * 1024.0f);          // table position: the ROUNDED fractional offset
      const float raw[4] = {keys_far(off), keys_near(off), keys_near(1024 - off), keys_far(1024 - off)};
      float tot = 0.f;
      for (int j = 0; j < 4; ++j)
        if (base - 1 + j >= 0 && base - 1 + j < n_in) tot = tot + raw[j];
      for (int j = 0; j < 4; ++j) {
        const int i = base - 1 + j;
        const bool kept = i >= 0 && i < n_in;                         // taps outside weigh 0, the rest are renormalised
        idx_host[4 * k + j] = i < 0 ? 0 : (i > n_in - 1 ? n_in - 1 : i);
        w_host[4 * k + j] = kept ? raw[j] / tot : 0.f;
      }
    }
  }
  return 0;
}

extern "C" int tfimm_hip_preprocess_resize(const tfimm_resize_desc* d, void* stream) {
  return resize_launch(d, stream, false, "preprocess_resize");
}

extern "C" int tfimm_hip_ref_preprocess_resize(const tfimm_resize_desc* d, void* stream) {
  return resize_launch(d, stream, true, "ref_preprocess_resize");
}

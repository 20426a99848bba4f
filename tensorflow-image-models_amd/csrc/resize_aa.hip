// ANTIALIASED resize + centre crop + normalise of a uint8 image batch in ONE launch, written in the layouts of resize.hip
// (tfimm_hip_preprocess_resize).  Reference call sites: include/tfimm_hip.h.
//
// The arithmetic is tf.image.resize(float32(img), method, antialias=True) -- the ScaleAndTranslate formulation, a span of
// source pixels per output position whose length grows with the scale -- restated operation by operation (include/tfimm_hip.h,
// DESIGN.md 3.15), then the three float32 operations of create_preprocessing, so the result is BIT-EQUAL to the host
// restatement:
//   * the span tables -- first source index, tap count and float32 weights of every output row / column -- are built on the
//     HOST by tfimm_hip_resize_spans below, the one place in C where the span rule is written; the kernel computes none of it;
//   * every product and every sum is a separate float32 operation in the restatement's order: the vertical sums first, into a
//     float32 intermediate, then the horizontal sums, each from 0.0f in tap order.  This file is built with -ffp-contract=off
//     (csrc/Makefile) and carries the pragma below: nothing may contract to an FMA.
// A footprint of y_taps x x_taps source pixels per output pixel (9 x 9 for 1.875 x bicubic, up to 64 x 64) rules out the
// one-thread-per-pixel gather of resize.hip, so the resample is separable and tiled: one workgroup computes a tile of output
// rows x output columns of one image.  Phase 1 sums the y-taps of the uint8 source into a float32 LDS buffer
// [rows][source columns the tile's x-spans cover][c_in] -- consecutive threads read consecutive bytes of a source row; after a
// barrier, phase 2 has each thread take output pixels, sum their x-taps out of LDS, normalise and store one vector per pixel
// (border pixels of the padded layout: zeros).  Every pixel's sums run over its own span in tap order whatever tile it falls
// in, so the result does not depend on the tiling.  All global offsets are 64-bit; every start + t is clamped into the image
// and every LDS column into the staged range before use, so a bad table cannot read out of bounds.
#include "common.h"
#include "resize_tile.h"

#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int kTileCols = TFIMM_RESIZE_AA_TILE_COLS;      // output columns of a tile
constexpr int kMaxBlocks = TFIMM_RESIZE_AA_MAX_BLOCKS;    // grid cap: workgroups stride over the tiles
constexpr int kThreads = 256;
using tfimm_resize::kLdsFloats;   // the LDS budget of a workgroup and the tile rule: resize_tile.h

struct ResizeAAArgs {
  const uint8_t* in;
  void* out;
  const int32_t* y_start;
  const int32_t* y_count;
  const float* y_w;
  const int32_t* x_start;
  const int32_t* x_count;
  const float* x_w;
  int B, Hs, Ws, c_in, H, W, c_out, pad_t, pad_l, HP, WP;
  int y_taps, x_taps;
  int tile_rows, cols_max;   // rows of a tile; capacity of an LDS row in source columns
  int tiles_y, tiles_x;
  int vec;                   // as in resize.hip: 1 = 8-byte store per pixel (bf16, c_out == 4), 2 = 16-byte store, 0 = element stores
  float mean[TFIMM_PREPROCESS_MAX_CHANNELS];
  float std[TFIMM_PREPROCESS_MAX_CHANNELS];
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <bool F32>
__global__ void __launch_bounds__(kThreads) resize_aa_kernel(ResizeAAArgs a) {
  constexpr int MAXC = TFIMM_PREPROCESS_MAX_CHANNELS;
  extern __shared__ float rows_lds[];   // [tile rows][ncols][c_in]: the vertical sums
  const int tid = threadIdx.x;
  const int64_t n_tiles = (int64_t)a.B * a.tiles_y * a.tiles_x;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int tx = (int)(tile % a.tiles_x);
    const int64_t tt = tile / a.tiles_x;
    const int ty = (int)(tt % a.tiles_y);
    const int b = (int)(tt / a.tiles_y);
    const int yp0 = ty * a.tile_rows, xp0 = tx * kTileCols;            // the tile in the padded output
    // its part inside the image: output rows [y0, y1), columns [x0, x1)
    const int y0 = max(yp0 - a.pad_t, 0), y1 = min(yp0 + a.tile_rows - a.pad_t, a.H);
    const int x0 = max(xp0 - a.pad_l, 0), x1 = min(xp0 + kTileCols - a.pad_l, a.W);
    int c_lo = 0, ncols = 0;
    if (y0 < y1 && x0 < x1) {
      // spans start and end in ascending order along an axis: the tile's x-spans cover [start of the first, end of the last]
      c_lo = clampi(a.x_start[x0], 0, a.Ws - 1);
      const int last = a.x_start[x1 - 1] + clampi(a.x_count[x1 - 1], 1, a.x_taps) - 1;
      ncols = min(clampi(last, c_lo, a.Ws - 1) - c_lo + 1, a.cols_max);
      // ---- phase 1: vertical sums of ncols * c_in consecutive source bytes per output row
      const int nbytes = ncols * a.c_in;
      const int items = (y1 - y0) * nbytes;
      for (int i = tid; i < items; i += kThreads) {
        const int r = i / nbytes, j = i - r * nbytes;
        const int y = y0 + r;
        const int ys = a.y_start[y];
        const int cnt = clampi(a.y_count[y], 0, a.y_taps);
        const float* w = a.y_w + (int64_t)y * a.y_taps;
        float s = 0.f;
        for (int t = 0; t < cnt; ++t) {
          const int iy = clampi(ys + t, 0, a.Hs - 1);
          const int64_t off = (((int64_t)b * a.Hs + iy) * a.Ws + c_lo) * a.c_in + j;
          s = s + w[t] * (float)a.in[off];
        }
        rows_lds[i] = s;
      }
    }
    __syncthreads();
    // ---- phase 2: horizontal sums out of LDS, normalise, store; pixels outside the image are the zero border
    const int n_pix = a.tile_rows * kTileCols;
    for (int p = tid; p < n_pix; p += kThreads) {
      const int pr = p / kTileCols, pc = p - pr * kTileCols;
      const int yp = yp0 + pr, xp = xp0 + pc;
      if (yp >= a.HP || xp >= a.WP) continue;
      const int y = yp - a.pad_t, x = xp - a.pad_l;
      float v[MAXC];
#pragma unroll
      for (int c = 0; c < MAXC; ++c) v[c] = 0.f;
      if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W) {
        const int xs = a.x_start[x];
        const int cnt = clampi(a.x_count[x], 0, a.x_taps);
        const float* w = a.x_w + (int64_t)x * a.x_taps;
        const float* row = rows_lds + (y - y0) * ncols * a.c_in;
        for (int t = 0; t < cnt; ++t) {
          const int col = clampi(clampi(xs + t, 0, a.Ws - 1) - c_lo, 0, ncols - 1);
          const float wt = w[t];
          const float* px = row + col * a.c_in;
#pragma unroll
          for (int c = 0; c < MAXC; ++c)
            if (c < a.c_in) v[c] = v[c] + wt * px[c];
        }
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < a.c_in) v[c] = (v[c] / 255.0f - a.mean[c]) / a.std[c];
      }
      const int64_t id = ((int64_t)b * a.HP + yp) * a.WP + xp;
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
    __syncthreads();   // the next tile's phase 1 overwrites the buffer
  }
}

int resize_aa_launch(const tfimm_resize_aa_desc* d, void* stream, bool f32, const char* who) {
  if (!d) TFIMM_FAIL(TFIMM_EINVAL, "%s: null descriptor", who);
  if (!d->in || !d->out || !d->y_start || !d->y_count || !d->y_w || !d->x_start || !d->x_count || !d->x_w || !d->mean_host ||
      !d->std_host)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: null pointer", who);
  if (d->B <= 0 || d->Hs <= 0 || d->Ws <= 0 || d->c_in <= 0 || d->H <= 0 || d->W <= 0 || d->c_out <= 0)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: sizes must be positive (B=%d Hs=%d Ws=%d c_in=%d H=%d W=%d c_out=%d)", who, d->B, d->Hs,
               d->Ws, d->c_in, d->H, d->W, d->c_out);
  if (d->y_taps <= 0 || d->x_taps <= 0 || d->y_taps > TFIMM_RESIZE_AA_MAX_TAPS || d->x_taps > TFIMM_RESIZE_AA_MAX_TAPS)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: y_taps=%d x_taps=%d, must be in [1, TFIMM_RESIZE_AA_MAX_TAPS = %d]", who, d->y_taps, d->x_taps,
               TFIMM_RESIZE_AA_MAX_TAPS);
  if (d->y_taps > d->Hs || d->x_taps > d->Ws)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: y_taps=%d x_taps=%d exceed the source (Hs=%d Ws=%d)", who, d->y_taps, d->x_taps, d->Hs, d->Ws);
  if (d->c_in > TFIMM_PREPROCESS_MAX_CHANNELS || d->c_out < d->c_in)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: c_in=%d must be <= %d and <= c_out=%d", who, d->c_in, TFIMM_PREPROCESS_MAX_CHANNELS, d->c_out);
  if (d->pad_t < 0 || d->pad_b < 0 || d->pad_l < 0 || d->pad_r < 0) TFIMM_FAIL(TFIMM_EINVAL, "%s: negative pad", who);
  const bool padded = (d->pad_t | d->pad_b | d->pad_l | d->pad_r) != 0;
  if (padded && d->c_out != 4)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: the zero-bordered layout has 4 stored channels (c_in <= 4), got c_out=%d", who, d->c_out);
  ResizeAAArgs a;
  for (int c = 0; c < TFIMM_PREPROCESS_MAX_CHANNELS; ++c) {
    a.mean[c] = c < d->c_in ? d->mean_host[c] : 0.f;
    a.std[c] = c < d->c_in ? d->std_host[c] : 1.f;
    if (!(a.std[c] != 0.f)) TFIMM_FAIL(TFIMM_EINVAL, "%s: std[%d] == 0", who, c);
  }
  a.in = (const uint8_t*)d->in;
  a.out = d->out;
  a.y_start = d->y_start; a.y_count = d->y_count; a.y_w = d->y_w;
  a.x_start = d->x_start; a.x_count = d->x_count; a.x_w = d->x_w;
  a.B = d->B; a.Hs = d->Hs; a.Ws = d->Ws; a.c_in = d->c_in; a.H = d->H; a.W = d->W; a.c_out = d->c_out;
  a.pad_t = d->pad_t; a.pad_l = d->pad_l;
  a.HP = d->H + d->pad_t + d->pad_b;
  a.WP = d->W + d->pad_l + d->pad_r;
  a.y_taps = d->y_taps; a.x_taps = d->x_taps;
  a.vec = 0;
  if (!f32 && d->c_out == 4 && ((uintptr_t)d->out & 7) == 0) a.vec = 1;
  if (!f32 && d->c_out == 8 && ((uintptr_t)d->out & 15) == 0) a.vec = 2;
  // the tile: kTileCols output columns, and as many output rows (kTileRows at most) as the LDS budget holds of their
  // vertical sums (resize_tile.h)
  a.tile_rows = tfimm_resize::tile_rows(d->Ws, d->W, d->x_taps, a.c_in, a.HP, &a.cols_max);
  if (a.tile_rows < 1) TFIMM_FAIL(TFIMM_EINVAL, "%s: a tile row of %d columns x %d channels exceeds the LDS budget", who, a.cols_max, a.c_in);
  a.tiles_y = (a.HP + a.tile_rows - 1) / a.tile_rows;
  a.tiles_x = (a.WP + kTileCols - 1) / kTileCols;
  const size_t lds = (size_t)a.tile_rows * a.cols_max * a.c_in * sizeof(float);
  int64_t blocks = (int64_t)a.B * a.tiles_y * a.tiles_x;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  const dim3 grid((unsigned)blocks), block(kThreads);
  hipStream_t st = (hipStream_t)stream;
  if (f32) TFIMM_LAUNCH((resize_aa_kernel<true>), grid, block, lds, st, a);
  else TFIMM_LAUNCH((resize_aa_kernel<false>), grid, block, lds, st, a);
  return 0;
}

// Keys cubic convolution kernel, A = -0.5, evaluated directly (not from the 1024-entry table of resize.hip)
inline float keys(float x) {
  if (x >= 2.0f) return 0.0f;
  if (x >= 1.0f) return ((-0.5f * x + 2.5f) * x - 4.0f) * x + 2.0f;
  return ((1.5f * x - 2.5f) * x) * x + 1.0f;
}
inline float triangle(float x) {
  const float v = 1.0f - x;
  return v > 0.0f ? v : 0.0f;
}

struct SpanAxis {
  float inv, ks, reach;   // n_in / n_resized; max(inv, 1); radius * ks
  int taps;               // the span pitch T
};

SpanAxis span_axis(int n_in, int n_resized, int method) {
  SpanAxis s;
  const float radius = method == 1 ? 2.0f : 1.0f;
  s.inv = (float)n_in / (float)n_resized;
  s.ks = s.inv > 1.0f ? s.inv : 1.0f;
  s.reach = radius * s.ks;
  const int64_t full = 2 * (int64_t)ceilf(s.reach) + 1;
  s.taps = full < n_in ? (int)full : n_in;
  return s;
}

}  // namespace

extern "C" int tfimm_hip_resize_span_taps(int n_in, int n_resized, int method) {
  if (n_in <= 0 || n_resized <= 0) TFIMM_FAIL(TFIMM_EINVAL, "resize_span_taps: sizes must be positive (n_in=%d n_resized=%d)", n_in, n_resized);
  if (method != 0 && method != 1) TFIMM_FAIL(TFIMM_EINVAL, "resize_span_taps: method=%d, must be 0 (bilinear) or 1 (bicubic)", method);
  return span_axis(n_in, n_resized, method).taps;
}

extern "C" int tfimm_hip_resize_spans(int n_in, int n_resized, int first, int n_out, int method, int32_t* start_host,
                                      int32_t* count_host, float* w_host) {
  if (!start_host || !count_host || !w_host) TFIMM_FAIL(TFIMM_EINVAL, "resize_spans: null pointer");
  if (n_in <= 0 || n_resized <= 0 || first < 0 || n_out <= 0 || (int64_t)first + n_out > n_resized)
    TFIMM_FAIL(TFIMM_EINVAL, "resize_spans: bad window (n_in=%d n_resized=%d first=%d n_out=%d)", n_in, n_resized, first, n_out);
  if (method != 0 && method != 1) TFIMM_FAIL(TFIMM_EINVAL, "resize_spans: method=%d, must be 0 (bilinear) or 1 (bicubic)", method);
  const SpanAxis ax = span_axis(n_in, n_resized, method);
  const int T = ax.taps;
  for (int k = 0; k < n_out; ++k) {
    const float s = ((float)(first + k) + 0.5f) * ax.inv;                 // the span's centre in source coordinates
    int a = (int)ceilf(s - ax.reach - 0.5f), b = (int)floorf(s + ax.reach - 0.5f);
    a = a < 0 ? 0 : (a > n_in - 1 ? n_in - 1 : a);
    b = b < 0 ? 0 : (b > n_in - 1 ? n_in - 1 : b);
    const int count = b - a + 1;
    if (count < 1 || count > T)
      TFIMM_FAIL(TFIMM_EINVAL, "resize_spans: span [%d, %d] of position %d does not fit the pitch %d", a, b, first + k, T);
    float* w = w_host + (int64_t)k * T;
    float total = 0.0f;
    for (int i = a; i <= b; ++i) {
      const float x = fabsf(((float)i + 0.5f - s) / ax.ks);
      w[i - a] = method == 1 ? keys(x) : triangle(x);
      total = total + w[i - a];
    }
    if (fabsf(total) >= 1000.0f * FLT_MIN) {
      const float scale = 1.0f / total;
      for (int t = 0; t < count; ++t) w[t] = w[t] * scale;
    }
    for (int t = count; t < T; ++t) w[t] = 0.0f;                           // entries past count: +0.0
    start_host[k] = a;
    count_host[k] = count;
  }
  return 0;
}

extern "C" int tfimm_hip_preprocess_resize_aa(const tfimm_resize_aa_desc* d, void* stream) {
  return resize_aa_launch(d, stream, false, "preprocess_resize_aa");
}

extern "C" int tfimm_hip_ref_preprocess_resize_aa(const tfimm_resize_aa_desc* d, void* stream) {
  return resize_aa_launch(d, stream, true, "ref_preprocess_resize_aa");
}

// The device bodies and the launch code of the resize launches that read their per-image quantities from RECORDS in device
// memory: resize_batch.hip (every image packed on its own, tfimm_resize_batch_rec) and resize_regions.hip (boxes inside
// larger frames, tfimm_resize_region_rec).  Written once, as templates over the record, so that a box is computed by the very
// operations that compute the packed slice: the two record types differ in ONE integer -- the bytes between two source rows
// (row_pitch below) -- and in nothing that touches a float.  DESIGN.md 3.16, 3.22.
//
// Every file that includes this header is built with -ffp-contract=off (csrc/Makefile) and the header carries the pragma
// below: nothing may contract to an FMA.
//
// Nothing read from device memory is trusted: sizes are clamped to [1, 2^24], the row pitch to [1, 2^24 * MAX_CHANNELS], span
// pitches to [1, taps_cap], table offsets into their arenas, table indices into their image, tile shapes into the LDS
// allocation and every source byte offset into [0, in_bytes).  All global offsets are 64-bit.  A stale or bad record gives
// wrong pixels, never an access out of bounds.
#pragma once

#include "common.h"
#include "resize_tile.h"

#include <climits>

#pragma clang fp contract(off)

namespace {

constexpr int kResizeMaxBlocks = 256 * 16;                // plain launch: the grid-stride cap of resize.hip
constexpr int kTileRows = TFIMM_RESIZE_AA_TILE_ROWS;
constexpr int kTileCols = TFIMM_RESIZE_AA_TILE_COLS;
constexpr int kMaxBlocks = TFIMM_RESIZE_AA_MAX_BLOCKS;
constexpr int kThreads = 256;
constexpr int kMaxSide = 1 << 24;                         // a side read from a record is clamped here: offsets cannot overflow
constexpr int64_t kMaxPitch = (int64_t)kMaxSide * TFIMM_PREPROCESS_MAX_CHANNELS;   // and a row pitch here
using tfimm_resize::kLdsFloats;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int64_t clampl(int64_t v, int64_t lo, int64_t hi) { return min(max(v, lo), hi); }

// bytes between two source rows of the image of a record: a packed image's rows follow each other, a region's lie a row of
// its FRAME apart
__device__ __forceinline__ int64_t row_pitch(const tfimm_resize_batch_rec*, int Ws, int c_in) { return (int64_t)Ws * c_in; }
__device__ __forceinline__ int64_t row_pitch(const tfimm_resize_region_rec* r, int, int) {
  return clampl(r->row_pitch, 1, kMaxPitch);
}

// the store of one output pixel `id` (an index into [B][HP][WP]) in the layouts of resize.hip
template <bool F32>
__device__ __forceinline__ void store_pixel(void* out, int64_t id, const float* v, int c_out, int vec) {
  constexpr int MAXC = TFIMM_PREPROCESS_MAX_CHANNELS;
  if (F32) {
    float* o = reinterpret_cast<float*>(out) + id * c_out;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < c_out) o[c] = v[c];
    for (int c = MAXC; c < c_out; ++c) o[c] = 0.f;
  } else if (vec == 1) {
    reinterpret_cast<uint2*>(out)[id] = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
  } else if (vec == 2) {
    reinterpret_cast<uint4*>(out)[id] = pack8(v);
  } else {
    bf16_t* o = reinterpret_cast<bf16_t*>(out) + id * c_out;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < c_out) o[c] = (bf16_t)f2bf(v[c]);
    for (int c = MAXC; c < c_out; ++c) o[c] = (bf16_t)0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// plain launch: one thread per output pixel and all its channels (resize.hip resize_kernel)
// ---------------------------------------------------------------------------------------------------------------------
template <class Rec>
struct BatchArgs {
  const uint8_t* in;
  const Rec* recs;
  void* out;
  const int32_t* idx;
  const float* w;
  int64_t in_bytes, tab_cap;   // bytes of the pixel arena; entries of idx and of w
  int B, c_in, H, W, c_out, pad_t, pad_l, HP, WP;
  int vec;
  float mean[TFIMM_PREPROCESS_MAX_CHANNELS];
  float std[TFIMM_PREPROCESS_MAX_CHANNELS];
};

template <int TAPS, bool F32, class Rec>
__global__ void __launch_bounds__(256) resize_batch_kernel(BatchArgs<Rec> a) {
  constexpr int MAXC = TFIMM_PREPROCESS_MAX_CHANNELS;
  const int64_t total = (int64_t)a.B * a.HP * a.WP;
  // the last byte offset at which a pixel of c_in channels still lies inside the arena (in_bytes >= c_in: checked on the host)
  const int64_t limit = a.in_bytes - a.c_in;
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
      const Rec* r = a.recs + b;
      const int Hs = clampi(r->Hs, 1, kMaxSide), Ws = clampi(r->Ws, 1, kMaxSide);
      const int64_t pitch = row_pitch(r, Ws, a.c_in);
      const int64_t base = clampl(r->in_offset, 0, limit);
      const int64_t yt = clampl(r->y_tab, 0, a.tab_cap - (int64_t)a.H * TAPS) + (int64_t)y * TAPS;
      const int64_t xt = clampl(r->x_tab, 0, a.tab_cap - (int64_t)a.W * TAPS) + (int64_t)x * TAPS;
      float wy[TAPS], wx[TAPS];
      int64_t row[TAPS], col[TAPS];
#pragma unroll
      for (int k = 0; k < TAPS; ++k) {
        const int iy = clampi(a.idx[yt + k], 0, Hs - 1);
        const int ix = clampi(a.idx[xt + k], 0, Ws - 1);
        wy[k] = a.w[yt + k];
        wx[k] = a.w[xt + k];
        // every weight in a register of its own: read as a pair, the compiler folds the high half into packed multiplies as an
        // operand select (v_pk_mul_f32 ... op_sel), which tools/isa_lint.py rules out on gfx950
        asm volatile("" : "+v"(wy[k]));
        asm volatile("" : "+v"(wx[k]));
        row[k] = base + (int64_t)iy * pitch;
        col[k] = (int64_t)ix * a.c_in;
      }
      // byte offset of every tap's pixel, clamped into the arena
      int64_t off[TAPS][TAPS];
#pragma unroll
      for (int i = 0; i < TAPS; ++i)
#pragma unroll
        for (int j = 0; j < TAPS; ++j) off[i][j] = min(row[i] + col[j], limit);
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
              for (int i = 0; i < 4; ++i) s = s + wy[i] * (float)a.in[off[i][j] + c];
              r = r + wx[j] * s;
            }
          } else {
            const float tl = (float)a.in[off[0][0] + c], tr = (float)a.in[off[0][TAPS - 1] + c];
            const float bl = (float)a.in[off[TAPS - 1][0] + c], br = (float)a.in[off[TAPS - 1][TAPS - 1] + c];
            const float top = tl + (tr - tl) * wx[TAPS - 1];
            const float bottom = bl + (br - bl) * wx[TAPS - 1];
            r = top + (bottom - top) * wy[TAPS - 1];
          }
          v[c] = (r / 255.0f - a.mean[c]) / a.std[c];
        }
      }
    }
    store_pixel<F32>(a.out, id, v, a.c_out, a.vec);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// antialiased launch: one workgroup per tile of output rows x output columns of one image (resize_aa.hip resize_aa_kernel)
// ---------------------------------------------------------------------------------------------------------------------
template <class Rec>
struct BatchAAArgs {
  const uint8_t* in;
  const Rec* recs;
  void* out;
  const int32_t* start;
  const int32_t* count;
  const float* w;
  int64_t in_bytes, pos_cap, w_cap;   // bytes of the pixel arena; entries of start and of count; floats of w
  int64_t max_tiles;                  // B * HP * tiles_x: what the batch has with one-row tiles
  int B, c_in, H, W, c_out, pad_t, pad_l, HP, WP;
  int taps_cap, lds_floats, tiles_x;
  int vec;
  float mean[TFIMM_PREPROCESS_MAX_CHANNELS];
  float std[TFIMM_PREPROCESS_MAX_CHANNELS];
};

template <bool F32, class Rec>
__global__ void __launch_bounds__(kThreads) resize_batch_aa_kernel(BatchAAArgs<Rec> a) {
  constexpr int MAXC = TFIMM_PREPROCESS_MAX_CHANNELS;
  extern __shared__ float rows_lds[];   // [tile rows][ncols][c_in]: the vertical sums
  const int tid = threadIdx.x;
  const int64_t last = a.in_bytes - 1;
  const int64_t n_tiles = clampl((int64_t)a.recs[a.B - 1].tile0 + a.recs[a.B - 1].n_tiles, 0, a.max_tiles);
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    // the image of this tile: the last record whose first tile is <= tile.  Whatever the records hold, b is in [0, B)
    int lo = 0, hi = a.B - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((int64_t)a.recs[mid].tile0 <= tile) lo = mid;
      else hi = mid - 1;
    }
    const int b = lo;
    const Rec* r = a.recs + b;
    const int Hs = clampi(r->Hs, 1, kMaxSide), Ws = clampi(r->Ws, 1, kMaxSide);
    const int64_t pitch = row_pitch(r, Ws, a.c_in);
    const int64_t base = clampl(r->in_offset, 0, last);
    const int y_taps = clampi(r->y_taps, 1, (int)min((int64_t)a.taps_cap, a.w_cap / a.H));
    const int x_taps = clampi(r->x_taps, 1, (int)min((int64_t)a.taps_cap, a.w_cap / a.W));
    const int32_t* y_start = a.start + clampl(r->y_tab, 0, a.pos_cap - a.H);
    const int32_t* y_count = a.count + clampl(r->y_tab, 0, a.pos_cap - a.H);
    const int32_t* x_start = a.start + clampl(r->x_tab, 0, a.pos_cap - a.W);
    const int32_t* x_count = a.count + clampl(r->x_tab, 0, a.pos_cap - a.W);
    const float* y_w = a.w + clampl(r->y_w, 0, a.w_cap - (int64_t)a.H * y_taps);
    const float* x_w = a.w + clampl(r->x_w, 0, a.w_cap - (int64_t)a.W * x_taps);
    const int tile_rows = clampi(r->tile_rows, 1, kTileRows);
    const int cols_max = clampi(r->cols_max, 1, a.lds_floats / (tile_rows * a.c_in));
    const int64_t local = max(tile - (int64_t)r->tile0, (int64_t)0);
    const int tx = (int)(local % a.tiles_x);
    const int ty = (int)min(local / a.tiles_x, (int64_t)a.HP);        // ty * tile_rows >= HP: a tile outside, nothing stored
    const int yp0 = ty * tile_rows, xp0 = tx * kTileCols;             // the tile in the padded output
    // its part inside the image: output rows [y0, y1), columns [x0, x1)
    const int y0 = max(yp0 - a.pad_t, 0), y1 = min(yp0 + tile_rows - a.pad_t, a.H);
    const int x0 = max(xp0 - a.pad_l, 0), x1 = min(xp0 + kTileCols - a.pad_l, a.W);
    int c_lo = 0, ncols = 0;
    if (y0 < y1 && x0 < x1) {
      // spans start and end in ascending order along an axis: the tile's x-spans cover [start of the first, end of the last]
      c_lo = clampi(x_start[x0], 0, Ws - 1);
      const int lastc = clampi(x_start[x1 - 1], 0, Ws - 1) + clampi(x_count[x1 - 1], 1, x_taps) - 1;
      ncols = min(clampi(lastc, c_lo, Ws - 1) - c_lo + 1, cols_max);
      // ---- phase 1: vertical sums of ncols * c_in consecutive source bytes per output row
      const int nbytes = ncols * a.c_in;
      const int items = (y1 - y0) * nbytes;
      const int64_t first = base + (int64_t)c_lo * a.c_in;
      for (int i = tid; i < items; i += kThreads) {
        const int rr = i / nbytes, j = i - rr * nbytes;
        const int y = y0 + rr;
        const int ys = clampi(y_start[y], 0, Hs - 1);
        const int cnt = clampi(y_count[y], 0, y_taps);
        const float* w = y_w + (int64_t)y * y_taps;
        float s = 0.f;
        for (int t = 0; t < cnt; ++t) {
          const int iy = min(ys + t, Hs - 1);
          const int64_t off = min(first + ((int64_t)iy * pitch + j), last);
          s = s + w[t] * (float)a.in[off];
        }
        rows_lds[i] = s;
      }
    }
    __syncthreads();
    // ---- phase 2: horizontal sums out of LDS, normalise, store; pixels outside the image are the zero border
    const int n_pix = tile_rows * kTileCols;
    for (int p = tid; p < n_pix; p += kThreads) {
      const int pr = p / kTileCols, pc = p - pr * kTileCols;
      const int yp = yp0 + pr, xp = xp0 + pc;
      if (yp >= a.HP || xp >= a.WP) continue;
      const int y = yp - a.pad_t, x = xp - a.pad_l;
      float v[MAXC];
#pragma unroll
      for (int c = 0; c < MAXC; ++c) v[c] = 0.f;
      if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W) {
        const int xs = clampi(x_start[x], 0, Ws - 1);
        const int cnt = clampi(x_count[x], 0, x_taps);
        const float* w = x_w + (int64_t)x * x_taps;
        const float* row = rows_lds + (y - y0) * ncols * a.c_in;
        for (int t = 0; t < cnt; ++t) {
          const int col = clampi(min(xs + t, Ws - 1) - c_lo, 0, ncols - 1);
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
      store_pixel<F32>(a.out, ((int64_t)b * a.HP + yp) * a.WP + xp, v, a.c_out, a.vec);
    }
    __syncthreads();   // the next tile's phase 1 overwrites the buffer
  }
}

// the checks both descriptors share; fills mean / std
inline int check_common(const char* who, const void* in, const void* recs, const void* out, const float* mean_host,
                        const float* std_host, int64_t in_bytes, int B, int c_in, int H, int W, int c_out, int pad_t, int pad_b,
                        int pad_l, int pad_r, float* mean, float* std) {
  if (!in || !recs || !out || !mean_host || !std_host) TFIMM_FAIL(TFIMM_EINVAL, "%s: null pointer", who);
  if (B <= 0 || c_in <= 0 || H <= 0 || W <= 0 || c_out <= 0 || in_bytes <= 0)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: sizes must be positive (B=%d c_in=%d H=%d W=%d c_out=%d in_bytes=%lld)", who, B, c_in, H, W,
               c_out, (long long)in_bytes);
  if (c_in > TFIMM_PREPROCESS_MAX_CHANNELS || c_out < c_in)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: c_in=%d must be <= %d and <= c_out=%d", who, c_in, TFIMM_PREPROCESS_MAX_CHANNELS, c_out);
  if (in_bytes < c_in || in_bytes > ((int64_t)1 << 56))
    TFIMM_FAIL(TFIMM_EINVAL, "%s: in_bytes=%lld holds no pixel of %d channels (or is absurd)", who, (long long)in_bytes, c_in);
  if (pad_t < 0 || pad_b < 0 || pad_l < 0 || pad_r < 0) TFIMM_FAIL(TFIMM_EINVAL, "%s: negative pad", who);
  const bool padded = (pad_t | pad_b | pad_l | pad_r) != 0;
  if (padded && c_out != 4)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: the zero-bordered layout has 4 stored channels (c_in <= 4), got c_out=%d", who, c_out);
  if ((int64_t)B * ((int64_t)H + W) * 4 > INT_MAX)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: B * (H + W) = %lld: table offsets are 32-bit", who, (long long)B * ((int64_t)H + W));
  for (int c = 0; c < TFIMM_PREPROCESS_MAX_CHANNELS; ++c) {
    mean[c] = c < c_in ? mean_host[c] : 0.f;
    std[c] = c < c_in ? std_host[c] : 1.f;
    if (!(std[c] != 0.f)) TFIMM_FAIL(TFIMM_EINVAL, "%s: std[%d] == 0", who, c);
  }
  return 0;
}

inline int vec_of(bool f32, int c_out, const void* out) {
  if (!f32 && c_out == 4 && ((uintptr_t)out & 7) == 0) return 1;
  if (!f32 && c_out == 8 && ((uintptr_t)out & 15) == 0) return 2;
  return 0;
}

// Desc: tfimm_resize_batch_desc or tfimm_resize_region_desc -- the same fields, `recs` of the record type Rec
template <class Rec, class Desc>
int resize_batch_launch(const Desc* d, void* stream, bool f32, const char* who) {
  if (!d) TFIMM_FAIL(TFIMM_EINVAL, "%s: null descriptor", who);
  if (!d->idx || !d->w) TFIMM_FAIL(TFIMM_EINVAL, "%s: null pointer", who);
  BatchArgs<Rec> a;
  const int rc = check_common(who, d->in, d->recs, d->out, d->mean_host, d->std_host, d->in_bytes, d->B, d->c_in, d->H, d->W,
                              d->c_out, d->pad_t, d->pad_b, d->pad_l, d->pad_r, a.mean, a.std);
  if (rc != 0) return rc;
  if (d->taps != 2 && d->taps != 4) TFIMM_FAIL(TFIMM_EINVAL, "%s: taps=%d, must be 2 (bilinear) or 4 (bicubic)", who, d->taps);
  a.in = (const uint8_t*)d->in;
  a.recs = d->recs;
  a.out = d->out;
  a.idx = d->idx; a.w = d->w;
  a.in_bytes = d->in_bytes;
  a.tab_cap = (int64_t)d->B * (d->H + d->W) * d->taps;
  a.B = d->B; a.c_in = d->c_in; a.H = d->H; a.W = d->W; a.c_out = d->c_out;
  a.pad_t = d->pad_t; a.pad_l = d->pad_l;
  a.HP = d->H + d->pad_t + d->pad_b;
  a.WP = d->W + d->pad_l + d->pad_r;
  a.vec = vec_of(f32, d->c_out, d->out);
  const int64_t total = (int64_t)a.B * a.HP * a.WP;
  int64_t blocks = (total + 255) / 256;
  if (blocks > kResizeMaxBlocks) blocks = kResizeMaxBlocks;
  const dim3 grid((unsigned)blocks), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (d->taps == 4) {
    if (f32) TFIMM_LAUNCH((resize_batch_kernel<4, true, Rec>), grid, block, 0, st, a);
    else TFIMM_LAUNCH((resize_batch_kernel<4, false, Rec>), grid, block, 0, st, a);
  } else {
    if (f32) TFIMM_LAUNCH((resize_batch_kernel<2, true, Rec>), grid, block, 0, st, a);
    else TFIMM_LAUNCH((resize_batch_kernel<2, false, Rec>), grid, block, 0, st, a);
  }
  return 0;
}

// Desc: tfimm_resize_batch_aa_desc or tfimm_resize_region_aa_desc
template <class Rec, class Desc>
int resize_batch_aa_launch(const Desc* d, void* stream, bool f32, const char* who) {
  if (!d) TFIMM_FAIL(TFIMM_EINVAL, "%s: null descriptor", who);
  if (!d->start || !d->count || !d->w) TFIMM_FAIL(TFIMM_EINVAL, "%s: null pointer", who);
  BatchAAArgs<Rec> a;
  const int rc = check_common(who, d->in, d->recs, d->out, d->mean_host, d->std_host, d->in_bytes, d->B, d->c_in, d->H, d->W,
                              d->c_out, d->pad_t, d->pad_b, d->pad_l, d->pad_r, a.mean, a.std);
  if (rc != 0) return rc;
  if (d->taps_cap <= 0 || d->taps_cap > TFIMM_RESIZE_AA_MAX_TAPS)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: taps_cap=%d, must be in [1, TFIMM_RESIZE_AA_MAX_TAPS = %d]", who, d->taps_cap,
               TFIMM_RESIZE_AA_MAX_TAPS);
  if (d->w_floats < (d->H > d->W ? d->H : d->W) || d->w_floats > INT_MAX)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: w_floats=%lld, must hold one weight per output row / column and fit 32-bit offsets", who,
               (long long)d->w_floats);
  const int lds_bytes = d->lds_bytes == 0 ? kLdsFloats * 4 : d->lds_bytes;
  if (lds_bytes < 4 * kTileRows * TFIMM_PREPROCESS_MAX_CHANNELS || lds_bytes > kLdsFloats * 4 || lds_bytes % 4)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: lds_bytes=%d, must be 0 or a multiple of 4 in [%d, %d]", who, d->lds_bytes,
               4 * kTileRows * TFIMM_PREPROCESS_MAX_CHANNELS, kLdsFloats * 4);
  a.in = (const uint8_t*)d->in;
  a.recs = d->recs;
  a.out = d->out;
  a.start = d->start; a.count = d->count; a.w = d->w;
  a.in_bytes = d->in_bytes;
  a.pos_cap = (int64_t)d->B * (d->H + d->W);
  a.w_cap = d->w_floats;
  a.B = d->B; a.c_in = d->c_in; a.H = d->H; a.W = d->W; a.c_out = d->c_out;
  a.pad_t = d->pad_t; a.pad_l = d->pad_l;
  a.HP = d->H + d->pad_t + d->pad_b;
  a.WP = d->W + d->pad_l + d->pad_r;
  a.taps_cap = d->taps_cap;
  a.lds_floats = lds_bytes / 4;
  a.tiles_x = (a.WP + kTileCols - 1) / kTileCols;
  a.max_tiles = (int64_t)a.B * a.HP * a.tiles_x;
  if (a.max_tiles > INT_MAX) TFIMM_FAIL(TFIMM_EINVAL, "%s: %lld tiles: tile indices are 32-bit", who, (long long)a.max_tiles);
  a.vec = vec_of(f32, d->c_out, d->out);
  // the grid: the tiles the batch has when every image takes the tallest tile -- no image has fewer -- capped; a function of
  // the descriptor's scalars alone.  The workgroups read the real count from the records and stride over it.
  const int rows = a.HP < kTileRows ? a.HP : kTileRows;
  int64_t blocks = (int64_t)a.B * ((a.HP + rows - 1) / rows) * a.tiles_x;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  const dim3 grid((unsigned)blocks), block(kThreads);
  hipStream_t st = (hipStream_t)stream;
  if (f32) TFIMM_LAUNCH((resize_batch_aa_kernel<true, Rec>), grid, block, (size_t)lds_bytes, st, a);
  else TFIMM_LAUNCH((resize_batch_aa_kernel<false, Rec>), grid, block, (size_t)lds_bytes, st, a);
  return 0;
}

}  // namespace

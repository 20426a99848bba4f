// Resize + centre crop + normalise of a uint8 batch whose images each have a SIZE OF THEIR OWN, in ONE launch: the two
// launches of resize.hip and resize_aa.hip behind one more indirection.  Reference call sites: include/tfimm_hip.h;
// DESIGN.md 3.16.
//
// For image b both kernels compute exactly what the uniform launches compute for that image alone at B = 1: the per-pixel
// body of resize.hip and the per-tile body of resize_aa.hip are restated operation by operation (same tables, built by
// the same host functions; every product and every sum a separate float32 operation in the same order; the same three
// operations of the normalisation; one rounding to bf16) in resize_rec_kernels.h, which resize_regions.hip instantiates for
// boxes inside larger frames.  This file is built with -ffp-contract=off (csrc/Makefile) and the header carries the contract
// pragma: nothing may contract to an FMA.
//
// What differs is where the per-image quantities come from.  The pixels of all images are packed back to back in one byte
// arena, the tables of all images in table arenas, and a device array of records (tfimm_resize_batch_rec) says for every
// image where its pixels and tables start, how large it is and -- antialiased -- its span pitches and its tile shape.  The
// launch arguments, the grid and the LDS size depend on the output geometry and the arena capacities only, so a recording of
// the launch stays valid whatever the buffers hold later.
//
// Nothing read from device memory is trusted: sizes are clamped to [1, 2^24], pitches to [1, taps_cap], table offsets into
// their arenas, table indices into their image, tile shapes into the LDS allocation and every source byte offset into
// [0, in_bytes).  All global offsets are 64-bit.  A stale or bad record gives wrong pixels, never an access out of bounds.
#include "resize_rec_kernels.h"   // the device bodies and the launch code, shared with resize_regions.hip

namespace {
using Rec = tfimm_resize_batch_rec;
}  // namespace

extern "C" int tfimm_hip_resize_batch_tables(int B, const int32_t* src_hw, const int32_t* geometry, int H, int W, int c_in,
                                             const int32_t* pad, int method, int antialias, tfimm_resize_batch_sizes* sizes,
                                             tfimm_resize_batch_rec* recs, int32_t* tab_a, int32_t* tab_b, float* w) {
  const char* who = "resize_batch_tables";
  if (!src_hw || !geometry || !sizes) TFIMM_FAIL(TFIMM_EINVAL, "%s: null pointer", who);
  if (B <= 0 || H <= 0 || W <= 0 || c_in <= 0 || c_in > TFIMM_PREPROCESS_MAX_CHANNELS)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: bad sizes (B=%d H=%d W=%d c_in=%d)", who, B, H, W, c_in);
  if (method != 0 && method != 1) TFIMM_FAIL(TFIMM_EINVAL, "%s: method=%d, must be 0 (bilinear) or 1 (bicubic)", who, method);
  if (pad && (pad[0] < 0 || pad[1] < 0 || pad[2] < 0 || pad[3] < 0)) TFIMM_FAIL(TFIMM_EINVAL, "%s: negative pad", who);
  if (recs && (!tab_a || !w || (antialias && !tab_b))) TFIMM_FAIL(TFIMM_EINVAL, "%s: null table pointer", who);
  const int HP = H + (pad ? pad[0] + pad[1] : 0), WP = W + (pad ? pad[2] + pad[3] : 0);
  const int tiles_x = (WP + TFIMM_RESIZE_AA_TILE_COLS - 1) / TFIMM_RESIZE_AA_TILE_COLS;
  const int taps = method == 1 ? 4 : 2;
  const int64_t per_image = (int64_t)H + W;
  tfimm_resize_batch_sizes s = {};
  s.bad_image = -1;
  s.tab_elems = antialias ? B * per_image : B * per_image * taps;
  if (s.tab_elems > INT_MAX) TFIMM_FAIL(TFIMM_EINVAL, "%s: %lld table entries: offsets are 32-bit", who, (long long)s.tab_elems);
  s.max_taps = antialias ? 0 : taps;
  // pass 1: sizes, and the records into a local array; pass 2 below fills the tables
  int64_t in_off = 0, w_off = 0, tile0 = 0;
  for (int b = 0; b < B; ++b) {
    const int Hs = src_hw[2 * b], Ws = src_hw[2 * b + 1];
    const int Rh = geometry[4 * b], Rw = geometry[4 * b + 1];
    if (Hs <= 0 || Ws <= 0 || Hs > kMaxSide || Ws > kMaxSide)
      TFIMM_FAIL(TFIMM_EINVAL, "%s: image %d has size %d x %d (sides must be in [1, 2^24])", who, b, Hs, Ws);
    tfimm_resize_batch_rec r = {};
    r.in_offset = in_off;
    r.Hs = Hs; r.Ws = Ws;
    in_off += (int64_t)Hs * Ws * c_in;
    if (!antialias) {
      r.y_tab = r.y_w = (int32_t)(b * per_image * taps);
      r.x_tab = r.x_w = r.y_tab + H * taps;
      r.y_taps = r.x_taps = taps;
      w_off += per_image * taps;
    } else {
      const int Ty = tfimm_hip_resize_span_taps(Hs, Rh, method), Tx = tfimm_hip_resize_span_taps(Ws, Rw, method);
      if (Ty <= 0 || Tx <= 0) return TFIMM_EINVAL;                     // (the message is resize_span_taps's)
      if ((Ty > TFIMM_RESIZE_AA_MAX_TAPS || Tx > TFIMM_RESIZE_AA_MAX_TAPS) && s.bad_image < 0) s.bad_image = b;
      r.y_tab = (int32_t)(b * per_image);
      r.x_tab = r.y_tab + H;
      r.y_taps = Ty; r.x_taps = Tx;
      r.y_w = (int32_t)w_off;
      r.x_w = (int32_t)(w_off + (int64_t)H * Ty);
      w_off += (int64_t)H * Ty + (int64_t)W * Tx;
      if (w_off > INT_MAX) TFIMM_FAIL(TFIMM_EINVAL, "%s: more than 2^31 weights at image %d: offsets are 32-bit", who, b);
      if (s.bad_image < 0) {
        int cols_max = 0;
        r.tile_rows = tfimm_resize::tile_rows(Ws, W, Tx, c_in, HP, &cols_max);
        if (r.tile_rows < 1) TFIMM_FAIL(TFIMM_EINVAL, "%s: image %d: a tile row of %d columns x %d channels exceeds the LDS budget", who, b, cols_max, c_in);
        r.cols_max = cols_max;
        r.tile0 = (int32_t)tile0;
        r.n_tiles = ((HP + r.tile_rows - 1) / r.tile_rows) * tiles_x;
        tile0 += r.n_tiles;
        if (tile0 > INT_MAX) TFIMM_FAIL(TFIMM_EINVAL, "%s: more than 2^31 tiles at image %d", who, b);
        if (r.tile_rows * cols_max * c_in > s.lds_floats) s.lds_floats = r.tile_rows * cols_max * c_in;
      }
      if (Ty > s.max_taps) s.max_taps = Ty;
      if (Tx > s.max_taps) s.max_taps = Tx;
    }
    if (recs && s.bad_image < 0) recs[b] = r;
  }
  s.in_bytes = in_off;
  s.w_floats = w_off;
  s.n_tiles = tile0;
  *sizes = s;
  if (s.bad_image >= 0)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: image %d (%d x %d) needs more than TFIMM_RESIZE_AA_MAX_TAPS = %d taps per output pixel", who,
               s.bad_image, src_hw[2 * s.bad_image], src_hw[2 * s.bad_image + 1], TFIMM_RESIZE_AA_MAX_TAPS);
  if (!recs) return 0;
  for (int b = 0; b < B; ++b) {
    const tfimm_resize_batch_rec& r = recs[b];
    const int32_t* g = geometry + 4 * b;
    int rc;
    if (!antialias) {
      rc = tfimm_hip_resize_taps(r.Hs, g[0], g[2], H, method, tab_a + r.y_tab, w + r.y_w);
      if (rc == 0) rc = tfimm_hip_resize_taps(r.Ws, g[1], g[3], W, method, tab_a + r.x_tab, w + r.x_w);
    } else {
      rc = tfimm_hip_resize_spans(r.Hs, g[0], g[2], H, method, tab_a + r.y_tab, tab_b + r.y_tab, w + r.y_w);
      if (rc == 0) rc = tfimm_hip_resize_spans(r.Ws, g[1], g[3], W, method, tab_a + r.x_tab, tab_b + r.x_tab, w + r.x_w);
    }
    if (rc != 0) return rc;                                            // (a bad crop window: the message is the rule's)
  }
  return 0;
}

extern "C" int tfimm_hip_preprocess_resize_batch(const tfimm_resize_batch_desc* d, void* stream) {
  return resize_batch_launch<Rec>(d, stream, false, "preprocess_resize_batch");
}

extern "C" int tfimm_hip_ref_preprocess_resize_batch(const tfimm_resize_batch_desc* d, void* stream) {
  return resize_batch_launch<Rec>(d, stream, true, "ref_preprocess_resize_batch");
}

extern "C" int tfimm_hip_preprocess_resize_batch_aa(const tfimm_resize_batch_aa_desc* d, void* stream) {
  return resize_batch_aa_launch<Rec>(d, stream, false, "preprocess_resize_batch_aa");
}

extern "C" int tfimm_hip_ref_preprocess_resize_batch_aa(const tfimm_resize_batch_aa_desc* d, void* stream) {
  return resize_batch_aa_launch<Rec>(d, stream, true, "ref_preprocess_resize_batch_aa");
}

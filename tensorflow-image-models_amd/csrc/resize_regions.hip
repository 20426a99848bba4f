// Resize + centre crop + normalise of BOXES inside larger uint8 frames, in ONE launch: the two launches of resize_batch.hip
// with one more number per record, the bytes between two source rows.  Reference call sites: include/tfimm_hip.h;
// DESIGN.md 3.22.
//
// Box n covers rows [y0, y1) and columns [x0, x1) of its frame and is an image of its own: both kernels compute, bit for bit,
// what the launches of resize_batch.hip compute for the slice packed on its own.  The device code IS that of
// resize_batch.hip -- the per-pixel body and the per-tile body of resize_rec_kernels.h, instantiated for
// tfimm_resize_region_rec: the tables, every float32 operation and its order, the normalisation and the one rounding to bf16
// are the same text; only the address of a source row differs, in_offset + iy * row_pitch with the pitch of the FRAME in
// place of the width of the image.  Table indices are clamped to the box (Hs, Ws of the record), so no pixel outside it
// contributes.  Every frame lies once in the arena, however many boxes name it.
//
// This file is built with -ffp-contract=off (csrc/Makefile) and the header carries the contract pragma: nothing may contract
// to an FMA.  Nothing read from device memory is trusted -- the clamps of resize_rec_kernels.h, the row pitch among them.
#include "resize_rec_kernels.h"

#include <vector>

#pragma clang fp contract(off)

namespace {
using Rec = tfimm_resize_region_rec;
}  // namespace

extern "C" int tfimm_hip_resize_region_tables(int F, const int32_t* frame_hw, int N, const int32_t* boxes,
                                              const int32_t* box_frame, const int32_t* geometry, int H, int W, int c_in,
                                              const int32_t* pad, int method, int antialias, tfimm_resize_batch_sizes* sizes,
                                              tfimm_resize_region_rec* recs, int32_t* tab_a, int32_t* tab_b, float* w) {
  const char* who = "resize_region_tables";
  if (!frame_hw || !boxes || !box_frame || !geometry || !sizes) TFIMM_FAIL(TFIMM_EINVAL, "%s: null pointer", who);
  if (F <= 0 || N <= 0 || c_in <= 0 || c_in > TFIMM_PREPROCESS_MAX_CHANNELS)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: bad sizes (F=%d N=%d c_in=%d)", who, F, N, c_in);
  // the frames once each, back to back in list order
  std::vector<int64_t> frame_off((size_t)F);
  int64_t in_bytes = 0;
  for (int f = 0; f < F; ++f) {
    const int Hf = frame_hw[2 * f], Wf = frame_hw[2 * f + 1];
    if (Hf <= 0 || Wf <= 0 || Hf > kMaxSide || Wf > kMaxSide)
      TFIMM_FAIL(TFIMM_EINVAL, "%s: frame %d has size %d x %d (sides must be in [1, 2^24])", who, f, Hf, Wf);
    frame_off[f] = in_bytes;
    in_bytes += (int64_t)Hf * Wf * c_in;
    if (in_bytes > ((int64_t)1 << 56)) TFIMM_FAIL(TFIMM_EINVAL, "%s: the frames exceed 2^56 bytes at frame %d", who, f);
  }
  // every box an image of its own size
  std::vector<int32_t> box_hw((size_t)N * 2);
  for (int n = 0; n < N; ++n) {
    const int32_t* b = boxes + 4 * n;
    const int f = box_frame[n];
    if (f < 0 || f >= F) TFIMM_FAIL(TFIMM_EINVAL, "%s: box %d names frame %d of %d", who, n, f, F);
    if (b[2] <= b[0] || b[3] <= b[1])
      TFIMM_FAIL(TFIMM_EINVAL, "%s: box %d (%d, %d, %d, %d) is empty", who, n, b[0], b[1], b[2], b[3]);
    if (b[0] < 0 || b[1] < 0 || b[2] > frame_hw[2 * f] || b[3] > frame_hw[2 * f + 1])
      TFIMM_FAIL(TFIMM_EINVAL, "%s: box %d (%d, %d, %d, %d) lies outside its frame %d (%d x %d)", who, n, b[0], b[1], b[2], b[3],
                 f, frame_hw[2 * f], frame_hw[2 * f + 1]);
    box_hw[2 * n] = b[2] - b[0];
    box_hw[2 * n + 1] = b[3] - b[1];
  }
  // records and tables of those images: the one place where they are built
  std::vector<tfimm_resize_batch_rec> packed(recs ? (size_t)N : 0);
  tfimm_resize_batch_sizes s = {};
  s.bad_image = -1;
  const int rc = tfimm_hip_resize_batch_tables(N, box_hw.data(), geometry, H, W, c_in, pad, method, antialias, &s,
                                               recs ? packed.data() : nullptr, tab_a, tab_b, w);
  s.in_bytes = in_bytes;
  if (rc != 0) {
    if (s.bad_image < 0) return rc;                                    // (the message is resize_batch_tables's)
    *sizes = s;
    TFIMM_FAIL(TFIMM_EINVAL, "%s: box %d (%d x %d) needs more than TFIMM_RESIZE_AA_MAX_TAPS = %d taps per output pixel", who,
               s.bad_image, box_hw[2 * s.bad_image], box_hw[2 * s.bad_image + 1], TFIMM_RESIZE_AA_MAX_TAPS);
  }
  *sizes = s;
  if (!recs) return 0;
  for (int n = 0; n < N; ++n) {
    const tfimm_resize_batch_rec& p = packed[n];
    const int f = box_frame[n];
    const int64_t Wf = frame_hw[2 * f + 1];
    tfimm_resize_region_rec r = {};
    r.in_offset = frame_off[f] + ((int64_t)boxes[4 * n] * Wf + boxes[4 * n + 1]) * c_in;
    r.row_pitch = Wf * c_in;
    r.Hs = p.Hs; r.Ws = p.Ws;
    r.y_tab = p.y_tab; r.x_tab = p.x_tab;
    r.y_w = p.y_w; r.x_w = p.x_w;
    r.y_taps = p.y_taps; r.x_taps = p.x_taps;
    r.tile_rows = p.tile_rows; r.cols_max = p.cols_max;
    r.tile0 = p.tile0; r.n_tiles = p.n_tiles;
    recs[n] = r;
  }
  return 0;
}

extern "C" int tfimm_hip_preprocess_regions(const tfimm_resize_region_desc* d, void* stream) {
  return resize_batch_launch<Rec>(d, stream, false, "preprocess_regions");
}

extern "C" int tfimm_hip_ref_preprocess_regions(const tfimm_resize_region_desc* d, void* stream) {
  return resize_batch_launch<Rec>(d, stream, true, "ref_preprocess_regions");
}

extern "C" int tfimm_hip_preprocess_regions_aa(const tfimm_resize_region_aa_desc* d, void* stream) {
  return resize_batch_aa_launch<Rec>(d, stream, false, "preprocess_regions_aa");
}

extern "C" int tfimm_hip_ref_preprocess_regions_aa(const tfimm_resize_region_aa_desc* d, void* stream) {
  return resize_batch_aa_launch<Rec>(d, stream, true, "ref_preprocess_regions_aa");
}

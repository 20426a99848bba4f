// The tile rule of the antialiased resize launches (resize_aa.hip, resize_batch.hip): how many source columns a tile of
// output columns can cover and how many output rows of vertical sums fit the LDS budget.  Host code only; written once so
// that the uniform launch and the records of a mixed-size batch cannot drift apart.
#pragma once

#include <cmath>

#include "../../include/tfimm_hip.h"

namespace tfimm_resize {

// LDS budget of a workgroup: 64 KiB of float32, so two workgroups share a CU's 160 KiB with 32 KiB to spare
constexpr int kLdsFloats = 64 * 1024 / 4;

// Source columns that the x-spans of `n_cols` consecutive output columns can cover.  Consecutive span centres lie inv =
// Ws / Rw apart and a span is at most x_taps long, so the range is (n_cols - 1) * inv + x_taps, plus 2 for the float32
// rounding of the centres.  The descriptor does not carry Rw; inv <= Ws / W (the crop window is no wider than the resized
// image) and inv <= (x_taps - 1) / 2 (x_taps >= 2 * radius * max(inv, 1) + 1 with radius >= 1, unless Ws caps it -- and then
// Ws caps the range too) bound it.
inline int span_cols(int n_cols, int Ws, int W, int x_taps) {
  const double inv = fmin((double)Ws / (double)W, fmax((double)(x_taps - 1) * 0.5, 1.0));
  const double cols = ceil((double)(n_cols - 1) * inv) + (double)x_taps + 2.0;
  return cols < (double)Ws ? (int)cols : Ws;
}

// The tile of an image: TFIMM_RESIZE_AA_TILE_COLS output columns, and as many output rows (TFIMM_RESIZE_AA_TILE_ROWS at
// most) as the LDS budget holds of their vertical sums.  At the limits of the domain (x_taps = 64, c_in = 8) one row is
// 1043 x 8 floats = 33 KiB: always >= 1 row.  HP: rows of the (padded) output.  Returns the rows of a tile, 0 when not even
// one fits; *cols_max: the capacity of an LDS row in source columns.
inline int tile_rows(int Ws, int W, int x_taps, int c_in, int HP, int* cols_max) {
  *cols_max = span_cols(TFIMM_RESIZE_AA_TILE_COLS, Ws, W, x_taps);
  int rows = kLdsFloats / (*cols_max * c_in);
  if (rows > TFIMM_RESIZE_AA_TILE_ROWS) rows = TFIMM_RESIZE_AA_TILE_ROWS;
  if (rows > HP) rows = HP;
  return rows;
}

}  // namespace tfimm_resize

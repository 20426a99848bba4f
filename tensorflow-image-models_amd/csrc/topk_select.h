// The selection shared by tfimm_hip_topk (topk.hip) and the second pass of tfimm_hip_embed_search (embed.hip): float32 values
// as ORDER-PRESERVING 32-bit KEYS in LDS, and one selection round of a workgroup of 256 threads over them.
//
//     key(x) = 0xffffffff                     x is a NaN (any sign, any payload): above +inf
//              bits(x) | 0x80000000           x >= +0.0, and x == -0.0 (the sign of zero is canonicalised first)
//              ~bits(x)                       x < 0
//
// so that float order is unsigned order, -inf has the smallest key (0x007fffff) and 0 is free to mark a RETIRED (or empty)
// position.  The map is invertible except for zeros and NaNs.
//
// A round: every thread scans its positions tid, tid + 256, ... in ascending order for the largest key (a strict comparison:
// of equal keys the lowest position stays), the wave reduces the (key, position) pairs by cross-lane moves (larger key, then
// lower position: a total order, so the butterfly leaves the same pair in every lane), the four waves reduce through LDS in a
// fixed tree.  Every thread leaves with the same winner; the caller writes it out, retires it (keys[pos] = kRetired) and
// places the __syncthreads() in front of the next round.
#pragma once
#include "common.h"

#include <climits>

namespace topk_sel {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kKeyNaN = 0xffffffffu;    // every NaN
constexpr uint32_t kKeyZero = 0x80000000u;   // +0.0 and -0.0
constexpr uint32_t kRetired = 0u;            // below key(-inf) = 0x007fffff

__device__ __forceinline__ uint32_t key_of(uint32_t b) {
  if ((b & 0x7fffffffu) > 0x7f800000u) return kKeyNaN;
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// the float a key stands for; +0.0 for both zeros, one quiet NaN for every NaN
__device__ __forceinline__ uint32_t bits_of(uint32_t key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }

// (key, position) order of the selection: larger key first, of equal keys the lower position
__device__ __forceinline__ bool beats(uint32_t ka, int ia, uint32_t kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

// One round over keys[0, N) (LDS).  w_key / w_idx: kWaves entries of LDS each.  Contains one __syncthreads(); the caller's
// barrier behind the retirement also keeps w_key / w_idx from being rewritten before everyone has read them.
__device__ __forceinline__ void select_round(const uint32_t* keys, int N, int tid, uint32_t* w_key, int* w_idx, uint32_t& k0, int& i0) {
  const int lane = tid & 63, wave = tid >> 6;
  // ---- this thread's best: ascending positions, strict comparison
  uint32_t bk = kRetired;
  int bi = INT_MAX;
  for (int c = tid; c < N; c += kThreads) {
    const uint32_t q = keys[c];
    if (q > bk) { bk = q; bi = c; }
  }
  // ---- the wave's best in every lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t ok = __shfl_xor(bk, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (beats(ok, oi, bk, bi)) { bk = ok; bi = oi; }
  }
  if (lane == 0) { w_key[wave] = bk; w_idx[wave] = bi; }
  __syncthreads();
  // ---- the workgroup's best in every thread: (w0, w1), (w2, w3), then the two
  k0 = w_key[0];
  i0 = w_idx[0];
  uint32_t k1 = w_key[2];
  int i1 = w_idx[2];
  if (beats(w_key[1], w_idx[1], k0, i0)) { k0 = w_key[1]; i0 = w_idx[1]; }
  if (beats(w_key[3], w_idx[3], k1, i1)) { k1 = w_key[3]; i1 = w_idx[3]; }
  if (beats(k1, i1, k0, i0)) { k0 = k1; i0 = i1; }
}

}  // namespace topk_sel

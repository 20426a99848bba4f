// The two passes over a row of logits shared by tfimm_hip_topk (topk.hip) and tfimm_hip_score (score.hip): the row from global
// memory into LDS as the keys of topk_select.h, and sum_i exp(x_i - m) over that copy.  Both kernels run these instructions
// in this order, so the sum -- and every probability formed from it -- has the same bits in both.
//
// Loader: the row is read once, with 16-byte loads between a scalar head and a scalar tail chosen from the row's own address
// (no alignment is required of the base or of ld).  The stores behind a 16-byte load hit every fourth LDS bank (4-way on
// ds_write_b32: twice its conflict-free time, once per row).
//
// Sum: per-thread partials over the columns tid, tid + 256, ... in ascending order, the wave butterfly, the four waves through
// LDS in the fixed tree (w0 + w1) + (w2 + w3): float addition commutes exactly, so every lane holds the same bits.  The pass
// hands every (key, column) it reads to `visit`, so that a kernel with more to learn from the row (score.hip: the label's
// rank) reads LDS once; topk.hip passes a visitor that does nothing.
#pragma once
#include "topk_select.h"

namespace topk_sel {

// row[0, N) -> keys[0, N) (LDS).  The caller places the __syncthreads() behind it.
__device__ __forceinline__ void load_row_keys(const uint32_t* row, int N, int tid, uint32_t* keys) {
  const int head = min(N, (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2));
  const int nvec = (N - head) >> 2;
  for (int c = tid; c < head; c += kThreads) keys[c] = key_of(row[c]);
  const uint4* body = reinterpret_cast<const uint4*>(row + head);
  for (int v = tid; v < nvec; v += kThreads) {
    const uint4 u = body[v];
    uint32_t* dst = keys + head + 4 * v;
    dst[0] = key_of(u.x); dst[1] = key_of(u.y); dst[2] = key_of(u.z); dst[3] = key_of(u.w);
  }
  for (int c = head + 4 * nvec + tid; c < N; c += kThreads) keys[c] = key_of(row[c]);
}

// this thread's part of sum_i exp(x_i - m): its columns in ascending order; visit(key, column) for each of them
template <class Visit>
__device__ __forceinline__ float sum_exp_partial(const uint32_t* keys, int N, int tid, float m, Visit visit) {
  float s = 0.f;
  for (int c = tid; c < N; c += kThreads) {
    const uint32_t q = keys[c];
    s += expf(__uint_as_float(bits_of(q)) - m);
    visit(q, c);
  }
  return s;
}

// the workgroup's sum of the partials in every thread.  w_sum: kWaves floats of LDS.  Contains one __syncthreads().
__device__ __forceinline__ float block_sum(float s, int tid, float* w_sum) {
  s = wave_sum(s);
  if ((tid & 63) == 0) w_sum[tid >> 6] = s;
  __syncthreads();
  return (w_sum[0] + w_sum[1]) + (w_sum[2] + w_sum[3]);
}

}  // namespace topk_sel

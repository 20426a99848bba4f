// tfimm_hip_topk: the k largest logits of every row, their columns and their softmax probabilities (include/tfimm_hip.h;
// DESIGN.md 3.17; the CPU restatement of the rule is tests/topk_ref.py).  Replaces tf.nn.softmax + tf.math.top_k behind
// `model(x)`.
//
// One workgroup of 256 threads (4 waves) per row.  The row is read from global memory once, with 16-byte loads between a
// scalar head and a scalar tail chosen from the row's own address, and kept in LDS as ORDER-PRESERVING 32-bit KEYS:
//
//     key(x) = 0xffffffff                     x is a NaN (any sign, any payload): above +inf
//              bits(x) | 0x80000000           x >= +0.0, and x == -0.0 (the sign of zero is canonicalised first)
//              ~bits(x)                       x < 0
//
// so that float order is unsigned order, -inf has the smallest key (0x007fffff) and 0 is free to mark a RETIRED column.  The
// map is invertible except for zeros and NaNs; `values` is bit-exact all the same: the winner of a round whose key is one of
// those two re-reads its 4 bytes from the row (every other column of every row is read exactly once).
//
// Then k selection rounds.  Every thread scans its columns tid, tid + 256, ... in ascending order for the largest key (a
// strict comparison: of equal keys the lowest column stays), the wave reduces the (key, column) pairs by cross-lane moves
// (larger key, then lower column: a total order, so the butterfly leaves the same pair in every lane), the four waves
// reduce through LDS in a fixed tree, thread 0 writes the winner out and retires it in LDS.  Row maximum = the winner of
// round 0; sum of exp(x - max) = one more pass over the LDS copy before that winner is retired, per-thread partials in
// ascending column order, the same butterfly, the same tree ((w0 + w1) + (w2 + w3)): float addition commutes exactly, so every
// lane holds the same bits.  No atomics, no global scratch; rows never mix: bit-reproducible and independent of B.
//
// LDS traffic: the scans read lds[tid + 256 i] (consecutive lanes, consecutive banks: conflict-free); the stores behind a
// 16-byte load hit every fourth bank (4-way on ds_write_b32: twice its conflict-free time, once per row).
#include "topk_row.h"

namespace {

using namespace topk_sel;   // key_of / bits_of / beats / select_round: shared with embed.hip; the row passes with score.hip

struct TopkArgs {
  const uint32_t* logits;   // float32 bits
  uint32_t* values;
  int32_t* indices;
  float* probs;
  int64_t ld;
  int N, k;
};

__global__ void __launch_bounds__(kThreads) topk_kernel(TopkArgs a) {
  extern __shared__ uint32_t keys[];   // [N]
  __shared__ uint32_t w_key[kWaves];
  __shared__ int w_idx[kWaves];
  __shared__ float w_sum[kWaves];
  const int tid = threadIdx.x;
  const int N = a.N;
  const uint32_t* row = a.logits + (int64_t)blockIdx.x * a.ld;

  // ---- the row -> keys in LDS: scalar head up to the first 16-byte boundary, 16-byte body, scalar tail (topk_row.h)
  load_row_keys(row, N, tid, keys);
  __syncthreads();

  float m = 0.f, sum = 1.f;
  for (int j = 0; j < a.k; ++j) {
    // ---- the workgroup's best (key, column) in every thread (topk_select.h)
    uint32_t k0;
    int i0;
    select_round(keys, N, tid, w_key, w_idx, k0, i0);

    if (j == 0 && a.probs != nullptr) {
      // ---- row maximum = this winner; sum of exp(x - max) over the LDS copy, nothing retired yet
      m = __uint_as_float(bits_of(k0));
      sum = block_sum(sum_exp_partial(keys, N, tid, m, [](uint32_t, int) {}), tid, w_sum);
    }

    if (tid == 0 && i0 < N) {       // (k <= N: a round always has a winner; the test keeps a broken invariant inside the row)
      // a zero or a NaN lost its sign / payload in the key: its bits come from the row
      const uint32_t vb = (k0 == kKeyNaN || k0 == kKeyZero) ? row[i0] : bits_of(k0);
      const int64_t o = (int64_t)blockIdx.x * a.k + j;
      a.values[o] = vb;
      a.indices[o] = i0;
      if (a.probs != nullptr) a.probs[o] = expf(__uint_as_float(vb) - m) / sum;
      keys[i0] = kRetired;
    }
    __syncthreads();                // the retired key before the next scan; w_key / w_idx read by everyone before they are rewritten
  }
}

}  // namespace

extern "C" int tfimm_hip_topk(const float* logits, int64_t ld, int B, int N, int k, float* values, int32_t* indices,
                              float* probs, void* stream) {
  if (!logits) TFIMM_FAIL(TFIMM_EINVAL, "topk: logits is null");
  if (!values) TFIMM_FAIL(TFIMM_EINVAL, "topk: values is null");
  if (!indices) TFIMM_FAIL(TFIMM_EINVAL, "topk: indices is null");
  if (((uintptr_t)logits | (uintptr_t)values | (uintptr_t)indices | (uintptr_t)probs) & 3)
    TFIMM_FAIL(TFIMM_EINVAL, "topk: logits, values, indices and probs hold 4-byte elements and must be 4-byte aligned");
  if (N < 1 || N > TFIMM_TOPK_MAX_N) TFIMM_FAIL(TFIMM_EINVAL, "topk: N=%d, must be in [1, TFIMM_TOPK_MAX_N = %d]", N, TFIMM_TOPK_MAX_N);
  if (k < 1 || k > N || k > TFIMM_TOPK_MAX_K)
    TFIMM_FAIL(TFIMM_EINVAL, "topk: k=%d, must be in [1, min(N = %d, TFIMM_TOPK_MAX_K = %d)]", k, N, TFIMM_TOPK_MAX_K);
  if (ld < N) TFIMM_FAIL(TFIMM_EINVAL, "topk: ld=%lld is smaller than N=%d", (long long)ld, N);
  if (B < 0) TFIMM_FAIL(TFIMM_EINVAL, "topk: B=%d is negative", B);
  if (B == 0) return 0;
  static tfimm_once_t ready;
  if (ready.need()) {
    TFIMM_HIP_CHECK(hipFuncSetAttribute((const void*)topk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TFIMM_TOPK_MAX_N * 4));
    ready.mark();
  }
  TopkArgs a;
  a.logits = reinterpret_cast<const uint32_t*>(logits);
  a.values = reinterpret_cast<uint32_t*>(values);
  a.indices = indices;
  a.probs = probs;
  a.ld = ld;
  a.N = N;
  a.k = k;
  const size_t lds_bytes = (size_t)((N + 3) / 4 * 4) * 4;
  TFIMM_LAUNCH(topk_kernel, dim3((unsigned)B), dim3(kThreads), lds_bytes, (hipStream_t)stream, a);
  return 0;
}

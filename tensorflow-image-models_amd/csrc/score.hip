// tfimm_hip_score: a labelled batch of logits scored on the device -- per row the cross-entropy loss, the true class's rank,
// the predicted class and the true class's probability -- and the integer accumulators of a meter updated by the same launch
// (include/tfimm_hip.h; the CPU restatement of the rule is tests/score_ref.py).  Replaces, in a caller of the
// reference's validation loop: the logits copied to the host, tf.nn.sparse_softmax_cross_entropy_with_logits and tf.argmax.
//
// One workgroup of 256 threads (4 waves) per row, the shape of topk.hip: the row is read from global memory once into LDS as
// order-preserving keys (topk_row.h: the loader and the sum are that kernel's, instruction for instruction), then
//
//   1. one selection round (topk_select.h): the first maximum = pred, its value = m;
//   2. one pass over the LDS copy: sum_i exp(x_i - m) as in topk.hip, and in the same pass the number of columns that BEAT
//      the label's column y (larger key, or equal key and lower column) -- integer per-thread partials, the wave butterfly,
//      the four waves through LDS in the fixed tree.  That count is the position column y has in tfimm_hip_topk's answer;
//   3. thread 0: prob = expf(x_y - m) / sum (topk.hip's expression), loss = logf(sum) - (x_y - m), the four outputs, and
//      the meter: 64- / 32-bit integer atomicAdd only, so the accumulators do not depend on the order in which rows arrive.
//
// x_y comes from the key: both zeros read as +0.0, which changes neither x_y - m (m is a key's value too) nor expf of it.  A
// label outside [0, N) reads no column at all: its row is counted as ignored (-1) or invalid (anything else).
#include "topk_row.h"

namespace {

using namespace topk_sel;

struct ScoreArgs {
  const uint32_t* logits;   // float32 bits
  const int32_t* labels;
  float* loss;
  int32_t* rank;
  int32_t* pred;
  float* prob;
  unsigned long long* state;       // TFIMM_SCORE_STATE_WORDS, or null
  unsigned long long* per_class;   // [2][N], or null
  uint32_t* confusion;             // [N][N], or null
  int64_t ld;
  int N;
};

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(kThreads) score_kernel(ScoreArgs a) {
  extern __shared__ uint32_t keys[];   // [N]
  __shared__ uint32_t w_key[kWaves];
  __shared__ int w_idx[kWaves];
  __shared__ float w_sum[kWaves];
  __shared__ int w_cnt[kWaves];
  const int tid = threadIdx.x;
  const int N = a.N;
  const int64_t b = blockIdx.x;
  const uint32_t* row = a.logits + b * a.ld;

  load_row_keys(row, N, tid, keys);
  __syncthreads();

  // ---- pred and the row maximum: the winner of one round
  uint32_t k0;
  int i0;
  select_round(keys, N, tid, w_key, w_idx, k0, i0);
  const float m = __uint_as_float(bits_of(k0));

  // ---- the label's key: only a label inside the row is ever used as a column
  const int y = a.labels[b];
  const bool scored = y >= 0 && y < N;
  const uint32_t ky = scored ? keys[y] : kKeyNaN;

  // ---- one pass: the sum of topk.hip, and how many columns beat column y
  int cnt = 0;
  const float part = sum_exp_partial(keys, N, tid, m, [&](uint32_t q, int c) { cnt += beats(q, c, ky, y) ? 1 : 0; });
  cnt = wave_sum_int(cnt);
  if ((tid & 63) == 0) w_cnt[tid >> 6] = cnt;
  const float sum = block_sum(part, tid, w_sum);   // its barrier also publishes w_cnt

  if (tid != 0) return;
  float loss = 0.f, prob = 0.f;
  int rank = y == TFIMM_SCORE_IGNORE ? -1 : -2;
  if (scored) {
    rank = (w_cnt[0] + w_cnt[1]) + (w_cnt[2] + w_cnt[3]);
    const float d = __uint_as_float(bits_of(ky)) - m;
    prob = expf(d) / sum;
    loss = logf(sum) - d;
  }
  a.loss[b] = loss;
  a.rank[b] = rank;
  a.pred[b] = i0;
  a.prob[b] = prob;

  if (a.state != nullptr) {
    if (!scored) {
      atomicAdd(a.state + (y == TFIMM_SCORE_IGNORE ? TFIMM_SCORE_IGNORED : TFIMM_SCORE_INVALID), 1ull);
    } else {
      atomicAdd(a.state + TFIMM_SCORE_SCORED, 1ull);
      if (loss < 1024.0f)   // false for a NaN
        atomicAdd(a.state + TFIMM_SCORE_LOSS_Q, (unsigned long long)__double2ll_rn((double)loss * 4294967296.0));
      else
        atomicAdd(a.state + TFIMM_SCORE_LOSS_EXCLUDED, 1ull);
      atomicAdd(a.state + TFIMM_SCORE_RANK_HIST + min(rank, TFIMM_SCORE_RANK_BINS - 1), 1ull);
    }
  }
  if (scored && a.per_class != nullptr) {
    atomicAdd(a.per_class + y, 1ull);
    if (rank == 0) atomicAdd(a.per_class + N + y, 1ull);
  }
  if (scored && a.confusion != nullptr && i0 < N)   // (N >= 1: a round always has a winner)
    atomicAdd(a.confusion + (int64_t)y * N + i0, 1u);
}

}  // namespace

extern "C" int tfimm_hip_score(const float* logits, int64_t ld, int B, int N, const int32_t* labels, float* loss, int32_t* rank,
                               int32_t* pred, float* prob, int64_t* state, int64_t* per_class, uint32_t* confusion, void* stream) {
  if (!logits) TFIMM_FAIL(TFIMM_EINVAL, "score: logits is null");
  if (!labels) TFIMM_FAIL(TFIMM_EINVAL, "score: labels is null");
  if (!loss) TFIMM_FAIL(TFIMM_EINVAL, "score: loss is null");
  if (!rank) TFIMM_FAIL(TFIMM_EINVAL, "score: rank is null");
  if (!pred) TFIMM_FAIL(TFIMM_EINVAL, "score: pred is null");
  if (!prob) TFIMM_FAIL(TFIMM_EINVAL, "score: prob is null");
  if (((uintptr_t)logits | (uintptr_t)labels | (uintptr_t)loss | (uintptr_t)rank | (uintptr_t)pred | (uintptr_t)prob |
       (uintptr_t)confusion) & 3)
    TFIMM_FAIL(TFIMM_EINVAL, "score: logits, labels, loss, rank, pred, prob and confusion hold 4-byte elements and must be 4-byte aligned");
  if (((uintptr_t)state | (uintptr_t)per_class) & 7)
    TFIMM_FAIL(TFIMM_EINVAL, "score: state and per_class hold 8-byte elements and must be 8-byte aligned");
  if (N < 1 || N > TFIMM_SCORE_MAX_N) TFIMM_FAIL(TFIMM_EINVAL, "score: N=%d, must be in [1, TFIMM_SCORE_MAX_N = %d]", N, TFIMM_SCORE_MAX_N);
  if (ld < N) TFIMM_FAIL(TFIMM_EINVAL, "score: ld=%lld is smaller than N=%d", (long long)ld, N);
  if (B < 0) TFIMM_FAIL(TFIMM_EINVAL, "score: B=%d is negative", B);
  if (confusion && N > TFIMM_SCORE_MAX_CONFUSION_N)
    TFIMM_FAIL(TFIMM_EINVAL, "score: confusion with N=%d, more than TFIMM_SCORE_MAX_CONFUSION_N = %d", N, TFIMM_SCORE_MAX_CONFUSION_N);
  if (B == 0) return 0;
  static tfimm_once_t ready;
  if (ready.need()) {
    TFIMM_HIP_CHECK(hipFuncSetAttribute((const void*)score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TFIMM_SCORE_MAX_N * 4));
    ready.mark();
  }
  ScoreArgs a;
  a.logits = reinterpret_cast<const uint32_t*>(logits);
  a.labels = labels;
  a.loss = loss;
  a.rank = rank;
  a.pred = pred;
  a.prob = prob;
  a.state = reinterpret_cast<unsigned long long*>(state);
  a.per_class = reinterpret_cast<unsigned long long*>(per_class);
  a.confusion = confusion;
  a.ld = ld;
  a.N = N;
  const size_t lds_bytes = (size_t)((N + 3) / 4 * 4) * 4;
  TFIMM_LAUNCH(score_kernel, dim3((unsigned)B), dim3(kThreads), lds_bytes, (hipStream_t)stream, a);
  return 0;
}

// tfimm_hip_matches_merge (include/tfimm_hip.h): the k best of up to eight sets of matches per query, on the
// device -- the join of the searches of two galleries, of two shards, or of a GalleryIndex and the rows added behind it.
// tests/live_ref.py::merge restates the rule on the CPU.
//
//   A candidate is an entry of a set whose index is not negative; its row is index + base of its set, its key
//   topk_sel::key_of(bits(score)).  The result is the k best candidates under (key descending, row ascending), scores written as
//   bits_of(key), the slots behind the last candidate as (-1, -inf).
//
//   The sets are SORTED -- every search here leaves its rows so: valid entries first, in that order, -1 behind them -- so no
//   selection is needed: the place of a candidate in the result is the number of candidates that beat it, which is its own
//   position in its set plus, for every other set, the number of entries there that beat it: a binary search.  Only the first
//   min(k_s, k) entries of a set can reach the result (a later one is beaten by k of its own set).
//
//   One wave per query, four queries per workgroup of 256 threads, a grid-stride loop over the queries in steps of four (every
//   wave runs the same number of steps, so the two barriers of a step are met by all).  A wave holds its query's entries in LDS
//   as the 64-bit words of embed_buffer.h, key << 32 | ~row (larger is better, distinct rows make distinct words, 0 -- below
//   every real word -- for an entry that is no candidate): total = sum_s min(k_s, k) words, at most 2048, 8 * total bytes per
//   wave and at most 64 KiB per workgroup.  Lane l owns entries l, l + 64, ... of every set; it finds their places with
//   sum_t ceil(log2(m_t + 1)) LDS reads each and writes those below k.  The number of candidates n is the sum of the sets'
//   valid prefixes (the same search, for the word 0); lanes write (-1, -inf) to slots n .. k - 1.  Under the preconditions the
//   places are a permutation of 0 .. n - 1: every output slot is written exactly once, by one lane.  Without them places may
//   collide or leave holes -- the result is unspecified --, and still every store goes to [b][0 .. k).
//
// The result is a function of the candidate set alone: no atomics, no dependence on B or on which queries share a workgroup.
#include "embed_check.h"
#include "topk_select.h"

namespace {

using namespace topk_sel;
using namespace embed_check;

constexpr const char* kFn = "matches_merge";
constexpr int kMaxBlocks = 8192;             // the grid-stride loop takes the rest: B is no grid dimension

struct MergeArgs {
  tfimm_match_set set[TFIMM_MERGE_MAX_SETS];
  int m[TFIMM_MERGE_MAX_SETS];               // min(k_s, k): the entries of set s that are looked at
  int off[TFIMM_MERGE_MAX_SETS];             // where they start among a wave's words
  uint32_t* scores;                          // float32 bits
  int32_t* indices;
  int64_t ld_out;
  int S, B, k, total;
};

// how many of the descending words a[0 .. m) are above x
__device__ __forceinline__ int count_above(const uint64_t* a, int m, uint64_t x) {
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] > x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kThreads) matches_merge_kernel(MergeArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint64_t words[];          // [kWaves][total]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int S = a.S, k = a.k;
  uint64_t* w = words + (size_t)wave * a.total;

  for (int64_t first = (int64_t)blockIdx.x * kWaves; first < a.B; first += (int64_t)gridDim.x * kWaves) {
    const int64_t b = first + wave;
    const bool have = b < a.B;
    if (have)
      for (int s = 0; s < S; ++s) {
        const int32_t* idx = a.set[s].indices + b * a.set[s].ld;
        const uint32_t* sc = reinterpret_cast<const uint32_t*>(a.set[s].scores) + b * a.set[s].ld;
        const uint32_t base = (uint32_t)a.set[s].base;
        for (int j = lane; j < a.m[s]; j += 64) {
          const int32_t i = idx[j];
          w[a.off[s] + j] = i >= 0 ? ((uint64_t)key_of(sc[j]) << 32) | (uint32_t)~((uint32_t)i + base) : 0ull;
        }
      }
    __syncthreads();
    if (have) {
      uint32_t* out_sc = a.scores + b * a.ld_out;
      int32_t* out_idx = a.indices + b * a.ld_out;
      int n = 0;                                                             // the candidates: the sets' valid prefixes
      for (int s = 0; s < S; ++s) n += count_above(w + a.off[s], a.m[s], 0ull);
      for (int j = n + lane; j < k; j += 64) {
        out_sc[j] = 0xff800000u;                                             // -inf
        out_idx[j] = -1;
      }
      for (int s = 0; s < S; ++s)
        for (int j = lane; j < a.m[s]; j += 64) {
          const uint64_t x = w[a.off[s] + j];
          if (x == 0ull) continue;
          int place = j;
          for (int t = 0; t < S; ++t)
            if (t != s) place += count_above(w + a.off[t], a.m[t], x);
          if (place < k) {
            out_sc[place] = bits_of((uint32_t)(x >> 32));
            out_idx[place] = (int32_t)~(uint32_t)x;
          }
        }
    }
    __syncthreads();                                                         // the next step overwrites the words
  }
}

}  // namespace

extern "C" int tfimm_hip_matches_merge(const tfimm_match_set* sets, int S, int B, int k, float* scores, int32_t* indices,
                                       int64_t ld_out, void* stream) {
  TFIMM_EMBED_TRY(check_pointers(kFn, {{"sets", sets, 4}, {"scores", scores, 4}, {"indices", indices, 4}},
                                 "must be 4-byte aligned"));
  if (S < 1 || S > TFIMM_MERGE_MAX_SETS)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: S=%d, must be in [1, TFIMM_MERGE_MAX_SETS = %d]", kFn, S, TFIMM_MERGE_MAX_SETS);
  for (int s = 0; s < S; ++s) {
    if (!sets[s].scores) TFIMM_FAIL(TFIMM_EINVAL, "%s: sets[%d].scores is null", kFn, s);
    if (!sets[s].indices) TFIMM_FAIL(TFIMM_EINVAL, "%s: sets[%d].indices is null", kFn, s);
  }
  for (int s = 0; s < S; ++s)
    if (((uintptr_t)sets[s].scores | (uintptr_t)sets[s].indices) & 3)
      TFIMM_FAIL(TFIMM_EINVAL, "%s: sets[%d].scores and sets[%d].indices hold 4-byte elements and must be 4-byte aligned", kFn, s, s);
  if (k < 1 || k > TFIMM_EMBED_WIDE_MAX_K)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: k=%d, must be in [1, TFIMM_EMBED_WIDE_MAX_K = %d]", kFn, k, TFIMM_EMBED_WIDE_MAX_K);
  for (int s = 0; s < S; ++s) {
    if (sets[s].k < 1 || sets[s].k > TFIMM_EMBED_WIDE_MAX_K)
      TFIMM_FAIL(TFIMM_EINVAL, "%s: sets[%d].k=%d, must be in [1, TFIMM_EMBED_WIDE_MAX_K = %d]", kFn, s, sets[s].k,
                 TFIMM_EMBED_WIDE_MAX_K);
    if (sets[s].ld < sets[s].k)
      TFIMM_FAIL(TFIMM_EINVAL, "%s: sets[%d].ld=%lld is smaller than sets[%d].k=%d", kFn, s, (long long)sets[s].ld, s, sets[s].k);
    if (sets[s].base < 0) TFIMM_FAIL(TFIMM_EINVAL, "%s: sets[%d].base=%d, must not be negative", kFn, s, sets[s].base);
  }
  if (ld_out < k) TFIMM_FAIL(TFIMM_EINVAL, "%s: ld_out=%lld is smaller than k=%d", kFn, (long long)ld_out, k);
  TFIMM_EMBED_TRY(check_B(kFn, B));
  if (B == 0) return 0;

  MergeArgs a = {};
  int total = 0;
  for (int s = 0; s < S; ++s) {
    a.set[s] = sets[s];
    a.m[s] = sets[s].k < k ? sets[s].k : k;
    a.off[s] = total;
    total += a.m[s];
  }
  a.scores = reinterpret_cast<uint32_t*>(scores);
  a.indices = indices;
  a.ld_out = ld_out;
  a.S = S;
  a.B = B;
  a.k = k;
  a.total = total;
  const int64_t blocks = cdiv64(B, kWaves);
  TFIMM_LAUNCH(matches_merge_kernel, dim3((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), dim3(kThreads),
               (size_t)kWaves * total * sizeof(uint64_t), (hipStream_t)stream, a);
  return 0;
}

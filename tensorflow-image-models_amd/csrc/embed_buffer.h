// The selection machinery shared by tfimm_hip_embed_search_wide (embed_wide.hip) and the fp8 scan of
// tfimm_hip_embed_search_coarse (embed_coarse.hip): the BUFFER of (key, row) pairs with its threshold, the
// prune that keeps its k best, the second pass that merges the chunks of a query, and the choice of the chunk.
//
//   A BUFFER is an unsorted set of up to `cap` (key, row) pairs in LDS with a count and a THRESHOLD: the k-th best pair it
//   held at its last prune, or "empty" (key 0, row INT_MAX: every real pair beats it).  A candidate that beats the threshold
//   under the total order (key descending, row ascending) takes the next slot -- an integer LDS atomic on the count -- so the
//   cost of accepting it is one atomic and two stores, whatever k is.  Slot order depends on the order of arrival; nothing
//   else does: prune_to_k reduces a buffer to the k best pairs of its CONTENT under the total order, a set that no order of
//   arrival changes, and raises the threshold to the k-th of them.  Every pair dropped -- by a prune or at the threshold --
//   is beaten by k pairs seen before it, so it is not among the k best of the whole: after any sequence of appends and prunes
//   the buffer holds the k best of everything seen so far, or everything seen if that is less.
//
//   prune_to_k, one wave per buffer: lane l takes pairs l, l + 64, ... into registers as 64-bit words (key << 32 | ~row: larger
//   is better, and distinct rows make distinct words), finds the k-th largest word T by a bitwise search from the top -- is
//   the count of words >= T | bit at least k? a comparison, a ballot and a population count per register; bits on which all
//   words agree are T's without a step --, and writes the words >= T back to slots 0 .. k-1 in lane order.  At most 64 steps
//   whatever the content; no float atomics, no spinning, no scratch.
//
//   select_pass2, one workgroup per query: the chunks * k pairs stream through one buffer in steps of 2048 (eight per thread,
//   all loads of a step in flight together), pruned by wave 0 whenever the count exceeds its cap - 2048.  No limit on the
//   number of candidates, so none on the number of chunks.  Then the k survivors are ordered by rank: survivor t goes to the
//   position given by the number of survivors that beat it -- a function of the set alone.
#pragma once
#include "embed_score.h"
#include "topk_select.h"

namespace embed_buffer {

using namespace topk_sel;
using namespace embed_score;

constexpr int kStepRows = kWaves * kRowTile;              // gallery rows per step of pass 1: what a buffer can gain in one
constexpr int kMaxCap = 512;                              // pairs per buffer of pass 1: eight per lane of the pruning wave
constexpr int kPass2Loads = 8;                            // pairs per thread and step of pass 2
constexpr int kPass2Step = kThreads * kPass2Loads;        // 2048
constexpr int kPass2Cap = TFIMM_EMBED_WIDE_MAX_K + kPass2Step;   // 2304 pairs: 18 KiB
static_assert(TFIMM_EMBED_WIDE_MAX_K + 2 * kStepRows <= kMaxCap, "cap = k + 256 fits the pruning wave's registers");
static_assert(kMaxCap % 64 == 0 && kPass2Cap % 64 == 0, "a whole number of pairs per lane");
static_assert(TFIMM_EMBED_WIDE_MAX_K <= kThreads, "pass 2 ranks one survivor per thread");

struct Buffer {
  uint32_t* key;   // [cap]
  int* idx;        // [cap]
  int* meta;       // count, threshold key, threshold row
  int cap;
  int rot;         // slot s lives at (s + rot) mod cap: the buffers of a tile start on different banks
};

__device__ __forceinline__ int slot_at(const Buffer& b, int s) {
  s += b.rot;
  return s >= b.cap ? s - b.cap : s;
}

// one more pair; returns the count behind it.  The caller keeps count <= cap (the bound check keeps a broken invariant inside
// the buffer).
__device__ __forceinline__ int buffer_append(const Buffer& b, uint32_t key, int row) {
  const int s = atomicAdd(b.meta, 1);
  if (s < b.cap) {
    const int p = slot_at(b, s);
    b.key[p] = key;
    b.idx[p] = row;
  }
  return s + 1;
}

// a value that every lane holds, where the compiler can see it: in scalar registers
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// One wave: the buffer keeps the k best of its pairs (all of them if there are no more than k; the threshold then stays) and
// its threshold becomes the k-th.  kPerLane * 64 >= cap.  LDS operations of one wave are in program order; the caller's
// barriers separate the prune from the appends of other waves.
template <int kPerLane>
__device__ __forceinline__ void prune_to_k(const Buffer& b, int k, int lane) {
  const int n = min(b.meta[0], b.cap);
  if (n <= k) return;
  uint64_t c[kPerLane];
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int e = j * 64 + lane;
    c[j] = 0;                                         // below every pair: a real key is at least 0x007fffff
    if (e < n) {
      const int p = slot_at(b, e);
      c[j] = ((uint64_t)b.key[p] << 32) | (uint32_t)~b.idx[p];
    }
  }
  // a bit on which all words agree is the k-th largest word's too (it is one of them): only the others are searched.  A word
  // has every common one, so below a searched bit it is never smaller than t: the comparison sees the bits above alone.
  uint64_t every = ~0ull, any = 0;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j)
    if (j * 64 + lane < n) {
      every &= c[j];
      any |= c[j];
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    every &= __shfl_xor(every, o, 64);
    any |= __shfl_xor(any, o, 64);
  }
  uint64_t t = uniform64(every);                      // becomes the largest word with at least k words >= it: the k-th largest
  uint64_t open = uniform64(any) ^ t;
  while (open) {                                      // at most 64 steps, from the highest bit down
    const int bit = 63 - __clzll(open);
    open ^= 1ull << bit;
    const uint64_t cand = t | (1ull << bit);
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j)
      if (j * 64 < n) cnt += __popcll(__ballot(c[j] >= cand));
    if (cnt >= k) t = cand;
  }
  int kept = 0;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    if (j * 64 < n) {
      const bool keep = c[j] >= t;
      const uint64_t mask = __ballot(keep);
      if (keep) {
        const int p = slot_at(b, kept + __popcll(mask & ((1ull << lane) - 1ull)));     // < k: exactly k words are >= t
        b.key[p] = (uint32_t)(c[j] >> 32);
        b.idx[p] = (int)~(uint32_t)c[j];
      }
      kept += __popcll(mask);
    }
  }
  if (lane == 0) {
    b.meta[0] = kept;
    b.meta[1] = (int)(uint32_t)(t >> 32);
    b.meta[2] = (int)~(uint32_t)t;
  }
}

struct SelectArgs {
  const uint32_t* ws_key;
  const int32_t* ws_idx;
  uint32_t* scores;    // float32 bits
  int32_t* indices;
  int64_t cand;        // chunks * k
  int k;
};

// the body of a second pass: a workgroup of kThreads, query blockIdx.x
__device__ __forceinline__ void select_pass2(const SelectArgs& a) {
  __shared__ uint32_t buf_key[kPass2Cap];
  __shared__ int buf_idx[kPass2Cap];
  __shared__ int meta[3];
  __shared__ int flags[3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = a.k;
  const Buffer b = {buf_key, buf_idx, meta, kPass2Cap, 0};
  if (tid == 0) {
    meta[0] = 0;
    meta[1] = (int)kRetired;
    meta[2] = INT_MAX;
    flags[0] = flags[1] = flags[2] = 0;
  }
  __syncthreads();
  const uint32_t* src_key = a.ws_key + (int64_t)blockIdx.x * a.cand;
  const int32_t* src_idx = a.ws_idx + (int64_t)blockIdx.x * a.cand;

  int f = 0;
  for (int64_t base = 0; base < a.cand; base += kPass2Step) {
    const int fn = f == 2 ? 0 : f + 1;
    if (tid == 0) flags[fn] = 0;
    uint32_t ck[kPass2Loads];
    int ci[kPass2Loads];
#pragma unroll
    for (int u = 0; u < kPass2Loads; ++u) {
      const int64_t c = base + u * kThreads + tid;
      ck[u] = c < a.cand ? src_key[c] : kRetired;       // an empty entry beats no threshold
      ci[u] = c < a.cand ? src_idx[c] : INT_MAX;
    }
    const uint32_t tk = (uint32_t)meta[1];
    const int ti = meta[2];
    int top = 0;
#pragma unroll
    for (int u = 0; u < kPass2Loads; ++u)
      if (beats(ck[u], ci[u], tk, ti)) top = buffer_append(b, ck[u], ci[u]);
    if (top > kPass2Cap - kPass2Step) flags[f] = 1;
    __syncthreads();
    if (flags[f]) {
      if (wave == 0) prune_to_k<kPass2Cap / 64>(b, k, lane);
      __syncthreads();
    }
    f = fn;
  }
  if (wave == 0) prune_to_k<kPass2Cap / 64>(b, k, lane);
  __syncthreads();

  // ---- the survivors by rank (k <= N: there are k of them; the test keeps a broken invariant inside the outputs)
  const int n = min(meta[0], k);
  if (tid < n) {
    const uint32_t mk = buf_key[tid];
    const int mi = buf_idx[tid];
    int pos = 0;
    for (int j = 0; j < n; ++j) pos += beats(buf_key[j], buf_idx[j], mk, mi) ? 1 : 0;
    const int64_t o = (int64_t)blockIdx.x * k + pos;
    a.scores[o] = bits_of(mk);
    a.indices[o] = mi;
  }
}

// pairs per buffer of pass 1 when `tile` bytes of LDS hold the query tile.  k + 128 pairs are the least.  The loop is bound by
// the gallery reads in flight, so the workgroups per CU that the least would allow come first; within their share of LDS room
// for two steps above k, so that a prune is due every other step at the earliest.
inline int choose_cap(int tile, int k) {
  const int per_cu = kLdsBudget / (tile + kQTile * 8 * (k + kStepRows));
  const int want = k + 2 * kStepRows, fit = (kLdsBudget / per_cu - tile) / (kQTile * 8);
  return want < fit ? want : fit;
}

// rows per workgroup of pass 1 when the caller leaves the choice: enough chunks to fill the chip several times over (256 CUs,
// a few workgroups each) however few query tiles there are, but at least 4 k rows (a chunk that is not several times k filters
// nothing; `least_factor` times k for a caller that wants fewer pairs in its second pass), in whole steps of 128
inline int choose_chunk(int B, int N, int k, int least_factor = 4) {
  const int64_t qtiles = B > kQTile ? (B + kQTile - 1) / kQTile : 1;
  int64_t want = 2048 / qtiles;
  if (want < 64) want = 64;
  int64_t chunk = cdiv64(cdiv64(N, want), kStepRows) * kStepRows;
  const int64_t least = cdiv64(least_factor * (int64_t)k, kStepRows) * kStepRows;
  return (int)(chunk < least ? least : chunk);
}

}  // namespace embed_buffer

// The selection machinery shared by the buffered gallery searches -- tfimm_hip_embed_search_wide (embed_wide.hip), the
// fp8 scan of tfimm_hip_embed_search_coarse (embed_coarse.hip; 3.27), tfimm_hip_embed_search_lists (embed_lists.hip; 3.28) and
// tfimm_hip_embed_search_lists_grouped (embed_lists_grouped.hip; 3.29): the BUFFER of (key, row) pairs with its threshold, the prune
// that keeps its k best, the STEP LOOP of a first pass over a tile of 32 buffers, the second pass that merges the chunks of a
// query, and the choice of the chunk.
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
//   StepFlags: a loop that appends in steps prunes when some count could overflow in the next step.  That test is a flag in LDS,
//   raised by the thread whose atomic returned such a count and read by every thread behind the step's barrier; the flags of
//   three consecutive steps are three different words (one is written, one read and one cleared at any time), so one barrier
//   per step is enough and every thread takes the same branch.  The rotation is written here once.
//
//   BufferTile and buffered_steps, the first pass of a tile of up to 32 queries (256 threads): every query owns one buffer, shared
//   by the four waves; count, threshold and a flag live in the 16 bytes behind its row of the query tile, which no score loop
//   reads.  A STEP is one 32-row tile per wave (128 positions): the caller's `score(base)` yields the wave's 32 x 32 scores
//   (query on the lane, 16 rows in the registers: embed_score.h), and a lane that holds a query appends those that beat its
//   threshold.  A step adds at most 128 pairs to a buffer, so all buffers are pruned -- by the waves in turn -- whenever a count
//   exceeds cap - 128 at the end of a step.  Every wave runs the same number of steps; a wave whose tile lies past the end
//   computes and appends nothing.  After the last step one more prune; emit_pairs then writes k pairs per query, unsorted,
//   empty entries as key 0, row INT_MAX.  What differs between the three users -- where the scores come from, which lanes hold
//   a query, where the pairs go and whether a position is a row or stands for one -- is their set-up and their two callables.
//
//   select_pass2, one workgroup per query: the chunks * k pairs stream through one buffer in steps of 2048 (eight per thread,
//   all loads of a step in flight together), pruned by wave 0 whenever the count exceeds its cap - 2048.  No limit on the
//   number of candidates, so none on the number of chunks.  Then the k survivors are ordered by rank: survivor t goes to the
//   position given by the number of survivors that beat it -- a function of the set alone.
#pragma once
#include "embed_check.h"
#include "embed_score.h"
#include "topk_select.h"

namespace embed_buffer {

using namespace topk_sel;
using namespace embed_score;
using namespace embed_check;

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

// the wave of this thread within its workgroup, where the compiler can see that all its lanes agree: in a scalar register.
// Loops and branches on threadIdx.x >> 6 are compiled as divergent ones -- vector addresses, an exec mask around every
// iteration --, and the prunes and the emit are loops over "the buffers of my wave".
__device__ __forceinline__ int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

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

// the flags of the steps of an appending loop (above): step s uses word[(s mod 3) * stride]; the caller clears them before
// the loop's first barrier.  Every thread calls open and close in every step.
template <typename T>
struct StepFlags {
  T* word;
  int stride;
  int f;       // this step's: s mod 3
  __device__ __forceinline__ int next() const { return f == 2 ? 0 : f + 1; }
  // the next step's flag goes down: it was last read behind the barrier before last
  __device__ __forceinline__ void open(int tid) const {
    if (tid == 0) word[next() * stride] = 0;
  }
  // the next step could overflow a buffer
  __device__ __forceinline__ void raise() const { word[f * stride] = 1; }
  // the step's one barrier; true when a prune is due (one value for all threads).  The caller prunes and places a barrier.
  __device__ __forceinline__ bool close() {
    __syncthreads();
    const bool due = word[f * stride] != 0;
    f = next();
    return due;
  }
};

// kQTile buffers of `cap` pairs behind a query tile of kQTile rows of `pitch` bytes, `values` of them the query's (2 E: bf16, E:
// fp8 codes); the four words behind the values of row qi: count, threshold key, threshold row, and (rows 0 .. 2) a step's flag.
// LDS is 32 pitch + 32 * 8 * cap bytes.
struct BufferTile {
  unsigned char* smem;
  int pitch, values, cap;
  uint32_t* key;   // [32][cap]
  int* idx;        // [32][cap]
  __device__ __forceinline__ BufferTile(unsigned char* smem_, int pitch_, int values_, int cap_)
      : smem(smem_), pitch(pitch_), values(values_), cap(cap_),
        key(reinterpret_cast<uint32_t*>(smem_ + (size_t)kQTile * pitch_)), idx(reinterpret_cast<int*>(key + kQTile * cap_)) {}
  __device__ __forceinline__ int* meta(int qi) const { return reinterpret_cast<int*>(smem + (size_t)qi * pitch + values); }
  __device__ __forceinline__ Buffer buffer(int qi) const { return Buffer{key + qi * cap, idx + qi * cap, meta(qi), cap, qi}; }
  __device__ __forceinline__ StepFlags<int> flags() const { return StepFlags<int>{meta(0) + 3, pitch / 4, 0}; }
  // every buffer empty, every flag down; the caller places the barrier
  __device__ __forceinline__ void clear(int tid) const {
    if (tid < kQTile) {
      int* m = meta(tid);
      m[0] = 0;
      m[1] = (int)kRetired;
      m[2] = INT_MAX;
      m[3] = 0;
    }
  }
  // the waves in turn: the buffers of lanes 0 .. occ - 1 down to their k best
  __device__ __forceinline__ void prune(int occ, int k, int lane, int wave) const {
    for (int qi = wave; qi < occ; qi += kWaves) prune_to_k<kMaxCap / 64>(buffer(qi), k, lane);
  }
};

// The step loop of a first pass (above) over positions [begin, end), the same in every thread of a workgroup of kThreads; lanes
// 0 .. occ - 1 of the tile hold a query.  score(base) -> f32x16: the scores of positions base .. base + 31 (base < end) against
// the tile, register i of lane (r, h) being position base + (i & 3) + 8 (i >> 2) + 4 h for query r; each wave calls it once per
// step with its own base, in ascending order.  Ends behind the last prune and its barrier.
template <typename Score>
__device__ __forceinline__ void buffered_steps(const BufferTile& t, int64_t begin, int64_t end, int occ, int k, Score&& score) {
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
  const int r = lane & 31, h = lane >> 5;
  const Buffer mine = t.buffer(r);
  StepFlags<int> flags = t.flags();
  const int steps = (int)((end - begin + kStepRows - 1) / kStepRows);
  for (int s = 0; s < steps; ++s) {
    flags.open(tid);
    const int64_t base = begin + (int64_t)s * kStepRows + wave * kRowTile;
    if (base < end) {
      const f32x16 acc = score(base);
      if (r < occ) {
        const uint32_t tk = (uint32_t)mine.meta[1];
        const int ti = mine.meta[2];
        int top = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int64_t pos = base + (i & 3) + 8 * (i >> 2) + 4 * h;
          const uint32_t key = key_of(__float_as_uint(acc[i]));
          if (pos < end && beats(key, (int)pos, tk, ti)) top = buffer_append(mine, key, (int)pos);
        }
        if (top > t.cap - kStepRows) flags.raise();
      }
    }
    if (flags.close()) {
      t.prune(occ, k, lane, wave);
      __syncthreads();
    }
  }
  t.prune(occ, k, lane, wave);
  __syncthreads();
}

// behind buffered_steps: the k pairs of every lane qi < occ to ws_key / ws_idx [out(qi) .. + k), a wave per lane; out(qi) < 0:
// nothing is written for it.  Unsorted; an empty entry (fewer than k positions seen): key 0, row INT_MAX.  With `ids` a pair's
// position pos stands for row ids[pos] (pos in [0, N)), without it is the row.
template <typename Out>
__device__ __forceinline__ void emit_pairs(const BufferTile& t, int occ, int k, uint32_t* ws_key, int32_t* ws_idx, Out&& out,
                                           const int32_t* ids = nullptr, int N = 0) {
  const int lane = threadIdx.x & 63, wave = wave_index();
  for (int qi = wave; qi < occ; qi += kWaves) {
    const int64_t o = out(qi);
    if (o < 0) continue;
    const Buffer b = t.buffer(qi);
    const int n = min(b.meta[0], k);
    for (int j = lane; j < k; j += 64) {
      uint32_t key = kRetired;
      int row = INT_MAX;
      if (j < n) {
        const int at = slot_at(b, j);
        key = b.key[at];
        row = b.idx[at];
        if (ids) row = row >= 0 && row < N ? ids[row] : INT_MAX;   // (always inside: the test keeps a broken invariant from reading)
      }
      ws_key[o + j] = key;
      ws_idx[o + j] = row;
    }
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
  __shared__ int flag_words[3];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
  const int k = a.k;
  const Buffer b = {buf_key, buf_idx, meta, kPass2Cap, 0};
  if (tid == 0) {
    meta[0] = 0;
    meta[1] = (int)kRetired;
    meta[2] = INT_MAX;
    flag_words[0] = flag_words[1] = flag_words[2] = 0;
  }
  __syncthreads();
  const uint32_t* src_key = a.ws_key + (int64_t)blockIdx.x * a.cand;
  const int32_t* src_idx = a.ws_idx + (int64_t)blockIdx.x * a.cand;

  StepFlags<int> flags = {flag_words, 1, 0};
  for (int64_t base = 0; base < a.cand; base += kPass2Step) {
    flags.open(tid);
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
    if (top > kPass2Cap - kPass2Step) flags.raise();
    if (flags.close()) {
      if (wave == 0) prune_to_k<kPass2Cap / 64>(b, k, lane);
      __syncthreads();
    }
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

// the most pairs per query a first pass can keep when `tile` bytes of LDS hold the query tile: tile + 32 * 8 * cap <= 160 KiB with
// cap = k + 128 at the least; `most` is what the second pass holds
inline int fit_max_k(int tile, int most) {
  const int m = (kLdsBudget - tile) / (kQTile * 8) - kStepRows;
  return m > most ? most : m;
}

// tfimm_hip_embed_search_wide_max_k: next to a bf16 query tile, 32 (2 E + 16) bytes
inline int tile_max_k(int E) { return e_ok(E) ? fit_max_k(kQTile * query_pitch(E), TFIMM_EMBED_WIDE_MAX_K) : 0; }

inline int check_tile_fit(const char* fn, int E, int k) {
  if (k > tile_max_k(E))
    TFIMM_FAIL(TFIMM_EINVAL,
               "%s: E=%d with k=%d: 32 buffers of k + %d pairs do not fit %d KiB of LDS next to the query tile; "
               "tfimm_hip_embed_search_wide_max_k(%d) = %d",
               fn, E, k, kStepRows, kLdsBudget / 1024, E, tile_max_k(E));
  return 0;
}

inline int check_chunk(const char* fn, int chunk) {
  if (chunk < 0 || chunk % kRowTile != 0) TFIMM_FAIL(TFIMM_EINVAL, "%s: chunk=%d, must be 0 or a positive multiple of 32", fn, chunk);
  return 0;
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

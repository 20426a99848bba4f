// The rules of the searches over INVERTED LISTS, shared by tfimm_hip_embed_search_lists (embed_lists.hip) and
// tfimm_hip_embed_search_lists_grouped (embed_lists_grouped.hip; 3.29).  The two leave the same set of k pairs at the same
// workspace address for every (query, probe slot, part) because each of these is written here once and called from both:
//
//   LIVE PAIR   (query, probe slot) is live when its list l = probes[slot] is in [0, L), no earlier slot of the query names l (a
//               repeated list counts once: select_pass2 ranks a pair by the number of pairs that beat it, which takes distinct
//               pairs), and the list is not empty, its offsets clamped to [0, N].
//   CUT         part p of a list [lo, hi) is positions [lo + p per, lo + (p + 1) per) within the list, per = ceil((hi - lo) / parts);
//               a part behind the last row is empty.
//   EMPTY       whoever owns a (query, slot, part) that scores nothing writes its k workspace entries as key 0, row INT_MAX.
//
// tests/index_ref.py restates them on the CPU.
#pragma once
#include "embed_buffer.h"

namespace embed_lists {

using namespace embed_buffer;

constexpr int kMaxParts = 64;
constexpr int kMaxB = 65535;                              // queries of a call: a grid dimension of embed_lists_pass1
static_assert(TFIMM_EMBED_LISTS_MAX_PROBE * kMaxParts <= 65535, "nprobe * parts is a grid dimension");
static_assert((int64_t)kMaxB * TFIMM_EMBED_LISTS_MAX_PROBE < (1ll << 31), "a pair number is an int");

// the arguments both entry points pass to their kernels
struct ListsArgs {
  const float* q;
  const uint16_t* g;         // rows in list order
  const int32_t* ids;        // [N]
  const int32_t* offsets;    // [L + 1]
  const int32_t* probes;     // [B][ld_p]
  uint32_t* ws_key;          // [B][nprobe * parts][k]
  int32_t* ws_idx;           // [B][nprobe * parts][k]
  uint32_t* scores;          // float32 bits [B][k]
  int32_t* indices;          // [B][k]
  int64_t ld_q, ld_g, ld_p;
  int N, E, L, nprobe, k, parts, cap;
};

__device__ __forceinline__ int clamp_pos(int v, int N) { return v < 0 ? 0 : (v > N ? N : v); }

// probes: the nprobe lists of one query
__device__ __forceinline__ bool live_pair(const ListsArgs& a, const int32_t* probes, int slot) {
  const int l = probes[slot];
  bool live = l >= 0 && l < a.L;
  for (int e = 0; e < slot && live; ++e) live = probes[e] != l;
  return live && clamp_pos(a.offsets[l + 1], a.N) > clamp_pos(a.offsets[l], a.N);
}

// positions [begin, end) of the list order; begin = end = 0 for an empty list, end <= begin for a part behind the last row
struct Cut {
  int64_t begin, end;
};
__device__ __forceinline__ Cut list_cut(const ListsArgs& a, int l, int part) {
  const int lo = clamp_pos(a.offsets[l], a.N), hi = clamp_pos(a.offsets[l + 1], a.N);
  Cut c = {0, 0};
  if (hi > lo) {
    const int64_t per = ((int64_t)(hi - lo) + a.parts - 1) / a.parts;
    c.begin = min((int64_t)lo + part * per, (int64_t)hi);
    c.end = min(c.begin + per, (int64_t)hi);
  }
  return c;
}

// n empty entries from `out` on, by the threads t = 0 .. threads - 1
__device__ __forceinline__ void empty_entries(const ListsArgs& a, int64_t out, int n, int t, int threads) {
  for (int j = t; j < n; j += threads) {
    a.ws_key[out + j] = kRetired;
    a.ws_idx[out + j] = INT_MAX;
  }
}

// ---- host: validates the shape of a call and resolves parts = 0; returns 0 or TFIMM_EINVAL with the message set.  `b_note`
// ends the text about B.  What else an entry point asks it checks behind this.
inline int resolve_lists(const char* fn, int B, int N, int E, int L, int nprobe, int k, int* parts, const char* b_note) {
  TFIMM_EMBED_TRY(check_E(fn, E));
  TFIMM_EMBED_TRY(check_N(fn, N));
  if (L < 1 || L > TFIMM_CLUSTER_MAX_C) TFIMM_FAIL(TFIMM_EINVAL, "%s: L=%d, must be in [1, TFIMM_CLUSTER_MAX_C = %d]", fn, L, TFIMM_CLUSTER_MAX_C);
  if (nprobe < 1 || nprobe > TFIMM_EMBED_LISTS_MAX_PROBE)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: nprobe=%d, must be in [1, TFIMM_EMBED_LISTS_MAX_PROBE = %d]", fn, nprobe, TFIMM_EMBED_LISTS_MAX_PROBE);
  if (k < 1 || k > TFIMM_EMBED_WIDE_MAX_K)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: k=%d, must be in [1, TFIMM_EMBED_WIDE_MAX_K = %d]", fn, k, TFIMM_EMBED_WIDE_MAX_K);
  if (*parts < 0 || *parts > kMaxParts)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: parts=%d, must be 0 (the library chooses) or in [1, %d]", fn, *parts, kMaxParts);
  if (*parts == 0) *parts = 1;
  if (B < 0 || B > kMaxB) TFIMM_FAIL(TFIMM_EINVAL, "%s: B=%d, must be in [0, %d]%s", fn, B, kMaxB, b_note);
  return 0;                                              // nprobe * parts, the other grid dimension, is at most 16384
}

// the pointer arguments both entry points take, in argument order
inline int check_lists_pointers(const char* fn, const float* q, const void* g, const int32_t* ids, const int32_t* offsets,
                                const int32_t* probes, const float* scores, const int32_t* indices, const void* workspace) {
  return check_pointers(fn, {{"q", q, 4}, {"g", g, 16}, {"ids", ids, 4}, {"offsets", offsets, 4}, {"probes", probes, 4},
                             {"scores", scores, 4}, {"indices", indices, 4}, {"workspace", workspace, 4}});
}

}  // namespace embed_lists

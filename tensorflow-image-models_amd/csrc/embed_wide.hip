// tfimm_hip_embed_search_wide (include/tfimm_hip.h): the gallery search of embed.hip for up to 256 neighbours
// per query, with a selection whose cost per accepted candidate does not grow with k.  Same rule (tests/embed_ref.py), same
// scores -- the query tile and the MFMA loop are embed_score.h, shared with embed.hip --, same keys (topk_select.h).
//
//   The buffers of (key, row) pairs, their prune, the step loop of the first pass and the second pass are embed_buffer.h, shared
//   with embed_coarse.hip, embed_lists.hip and embed_lists_grouped.hip; the argument checks are embed_check.h.
//
//   Pass 1, grid (gallery chunks, query tiles of 32), 256 threads: the query tile of embed_score.h, a BufferTile behind it, and
//   buffered_steps over the chunk's rows with score_tile as the score of a step; every query of the tile owns one buffer, and a
//   position is a gallery row.  Then k pairs per query go to the workspace [query][chunk][k], unsorted, empty entries (a chunk
//   of fewer than k rows) as key 0, row INT_MAX.  LDS is 32 (2 E + 16) + 32 * 8 * cap bytes exactly.
//
//   Pass 2, one workgroup per query: select_pass2 of embed_buffer.h over the chunks * k pairs.
//
// The result is therefore a function of the scores alone: bit-reproducible, independent of B, of chunk and of the order in
// which the waves arrive, and bit-equal to tfimm_hip_embed_search wherever both apply.
#include "embed_buffer.h"

namespace {

using namespace embed_buffer;

struct WideArgs {
  const float* q;
  const uint16_t* g;
  uint32_t* ws_key;    // [B][chunks][k]
  int32_t* ws_idx;     // [B][chunks][k]
  int64_t ld_q, ld_g;
  int B, N, E, k, chunk, chunks, cap;
};

__global__ void __launch_bounds__(kThreads) embed_wide_pass1(WideArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int E = a.E, k = a.k;
  const BufferTile t(smem, query_pitch(E), 2 * E, a.cap);
  const int q0 = blockIdx.y * kQTile;
  const int occ = min(kQTile, a.B - q0);                // lanes 0 .. occ - 1 hold a query

  load_query_tile(smem, a.q, a.ld_q, q0, a.B, E, tid, kThreads);
  t.clear(tid);
  __syncthreads();

  const int64_t row_begin = (int64_t)blockIdx.x * a.chunk;
  const int64_t row_end = min(row_begin + (int64_t)a.chunk, (int64_t)a.N);
  const int r = lane & 31, h = lane >> 5;
  const int groups = E / 64, tail = (E % 64) / 16;
  const unsigned char* qrow = smem + (size_t)r * t.pitch;
  buffered_steps(t, row_begin, row_end, occ, k, [&](int64_t base) {
    // a row past the gallery reads the last row instead (its scores are never looked at)
    const int64_t grow = min(base + r, (int64_t)a.N - 1);
    return score_tile(a.g + grow * a.ld_g, qrow, h, groups, tail);
  });
  emit_pairs(t, occ, k, a.ws_key, a.ws_idx, [&](int qi) { return ((int64_t)(q0 + qi) * a.chunks + blockIdx.x) * k; });
}

__global__ void __launch_bounds__(kThreads) embed_wide_pass2(SelectArgs a) { select_pass2(a); }

constexpr const char* kFn = "embed_search_wide";

// validates (B, N, E, k, chunk) and resolves chunk = 0; returns 0 or TFIMM_EINVAL with the message set
int resolve(int B, int N, int E, int k, int* chunk, int64_t* chunks) {
  TFIMM_EMBED_TRY(check_E(kFn, E));
  TFIMM_EMBED_TRY(check_N(kFn, N));
  if (k < 1 || k > N || k > TFIMM_EMBED_WIDE_MAX_K)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: k=%d, must be in [1, min(N = %d, TFIMM_EMBED_WIDE_MAX_K = %d)]", kFn, k, N, TFIMM_EMBED_WIDE_MAX_K);
  TFIMM_EMBED_TRY(check_chunk(kFn, *chunk));
  TFIMM_EMBED_TRY(check_B(kFn, B));
  TFIMM_EMBED_TRY(check_tile_fit(kFn, E, k));
  if (*chunk == 0) *chunk = choose_chunk(B, N, k);
  *chunks = cdiv64(N, *chunk);
  return 0;
}

// [B][chunks][k] keys and rows
int64_t workspace_need(int B, int64_t chunks, int k) { return (int64_t)(B > 0 ? B : 1) * chunks * k * 8; }

}  // namespace

extern "C" int tfimm_hip_embed_search_wide_max_k(int E) { return tile_max_k(E); }

extern "C" int64_t tfimm_hip_embed_search_wide_workspace(int B, int N, int E, int k, int chunk) {
  int64_t chunks = 0;
  TFIMM_EMBED_TRY(resolve(B, N, E, k, &chunk, &chunks));
  return workspace_need(B, chunks, k);
}

extern "C" int tfimm_hip_embed_search_wide(const float* q, int64_t ld_q, int B, const void* g, int64_t ld_g, int N, int E, int k,
                                           int chunk, float* scores, int32_t* indices, void* workspace, int64_t workspace_bytes,
                                           void* stream) {
  TFIMM_EMBED_TRY(check_pointers(kFn, {{"q", q, 4}, {"g", g, 16}, {"scores", scores, 4}, {"indices", indices, 4}, {"workspace", workspace, 4}}));
  int64_t chunks = 0;
  TFIMM_EMBED_TRY(resolve(B, N, E, k, &chunk, &chunks));
  TFIMM_EMBED_TRY(check_ld_q(kFn, ld_q, E));
  TFIMM_EMBED_TRY(check_ld_g(kFn, ld_g, E));
  TFIMM_EMBED_TRY(check_workspace(kFn, workspace_bytes, workspace_need(B, chunks, k)));
  if (B == 0) return 0;

  static tfimm_once_t ready;
  if (ready.need()) {
    TFIMM_HIP_CHECK(hipFuncSetAttribute((const void*)embed_wide_pass1, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
    ready.mark();
  }
  WideArgs a;
  a.q = q;
  a.g = reinterpret_cast<const uint16_t*>(g);
  a.ws_key = reinterpret_cast<uint32_t*>(workspace);
  a.ws_idx = reinterpret_cast<int32_t*>(a.ws_key + (int64_t)B * chunks * k);
  a.ld_q = ld_q;
  a.ld_g = ld_g;
  a.B = B;
  a.N = N;
  a.E = E;
  a.k = k;
  a.chunk = chunk;
  a.chunks = (int)chunks;
  a.cap = choose_cap(kQTile * query_pitch(E), k);
  const int qtiles = (B + kQTile - 1) / kQTile;
  TFIMM_LAUNCH(embed_wide_pass1, dim3((unsigned)chunks, (unsigned)qtiles), dim3(kThreads),
               (size_t)(kQTile * query_pitch(E) + kQTile * 8 * a.cap), (hipStream_t)stream, a);
  SelectArgs s;
  s.ws_key = a.ws_key;
  s.ws_idx = a.ws_idx;
  s.scores = reinterpret_cast<uint32_t*>(scores);
  s.indices = indices;
  s.cand = chunks * k;
  s.k = k;
  TFIMM_LAUNCH(embed_wide_pass2, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, s);
  return 0;
}

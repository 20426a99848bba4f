// tfimm_hip_embed_search_wide (include/tfimm_hip.h): the gallery search of embed.hip for up to 256 neighbours
// per query, with a selection whose cost per accepted candidate does not grow with k.  Same rule (tests/embed_ref.py), same
// scores -- the query tile and the MFMA loop are embed_score.h, shared with embed.hip --, same keys (topk_select.h).
//
//   The buffers of (key, row) pairs, their prune and the second pass are embed_buffer.h, shared with embed_coarse.hip.
//
//   Pass 1, grid (gallery chunks, query tiles of 32), 256 threads; every query of the tile owns one buffer, shared by the four
//   waves.  A STEP is one 32-row tile per wave (128 rows): after its MFMAs a lane appends those of its 16 scores that beat the
//   query's threshold.  A step adds at most 128 pairs to a buffer, so the workgroup prunes every buffer whenever some count
//   exceeds cap - 128 at the end of a step.  That test is a flag in LDS raised by the lane whose atomic returned such a count
//   and read by every thread behind the step's barrier; the flags of three consecutive steps are three different words (one is
//   written, one read and one cleared at any time), so one barrier per step is enough and every thread takes the same
//   branch.  Every wave runs the same number of steps; a wave whose rows lie past the chunk computes and appends nothing.
//   After the last step one more prune, then k pairs go to the workspace [query][chunk][k], unsorted, empty entries (a chunk
//   of fewer than k rows) as key 0, row INT_MAX.  The count, the threshold and the flags live in the 16 bytes behind every
//   query row of the tile, which the score loop never reads: LDS is 32 (2 E + 16) + 32 * 8 * cap bytes exactly.
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

// the four words behind query row qi of the tile: count, threshold key, threshold row, and (rows 0 .. 2) a step's flag
__device__ __forceinline__ int* tile_meta(unsigned char* smem, int pitch, int E, int qi) {
  return reinterpret_cast<int*>(smem + (size_t)qi * pitch + 2 * E);
}

__global__ void __launch_bounds__(kThreads) embed_wide_pass1(WideArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E = a.E, k = a.k, cap = a.cap;
  const int pitch = query_pitch(E);
  uint32_t* buf_key = reinterpret_cast<uint32_t*>(smem + (size_t)kQTile * pitch);   // [32][cap]
  int* buf_idx = reinterpret_cast<int*>(buf_key + kQTile * cap);                   // [32][cap]
  const int q0 = blockIdx.y * kQTile;

  load_query_tile(smem, a.q, a.ld_q, q0, a.B, E, tid, kThreads);
  if (tid < kQTile) {
    int* m = tile_meta(smem, pitch, E, tid);
    m[0] = 0;
    m[1] = (int)kRetired;
    m[2] = INT_MAX;
    m[3] = 0;
  }
  __syncthreads();

  const int64_t row_begin = (int64_t)blockIdx.x * a.chunk;
  const int64_t row_end = min(row_begin + (int64_t)a.chunk, (int64_t)a.N);
  const int r = lane & 31, h = lane >> 5;
  const bool q_valid = q0 + r < a.B;
  const int groups = E / 64, tail = (E % 64) / 16;
  const unsigned char* qrow = smem + (size_t)r * pitch;
  const Buffer mine = {buf_key + r * cap, buf_idx + r * cap, tile_meta(smem, pitch, E, r), cap, r};
  const int steps = (int)((row_end - row_begin + kStepRows - 1) / kStepRows);

  int f = 0;                                           // this step's flag: step mod 3
  for (int s = 0; s < steps; ++s) {
    int* flag = tile_meta(smem, pitch, E, f) + 3;
    const int fn = f == 2 ? 0 : f + 1;
    if (tid == 0) tile_meta(smem, pitch, E, fn)[3] = 0;          // the next step's: last read behind the barrier before last
    const int64_t base = row_begin + (int64_t)s * kStepRows + wave * kRowTile;
    if (base < row_end) {
      // a row past the gallery reads the last row instead (its scores are never looked at)
      const int64_t grow = min(base + r, (int64_t)a.N - 1);
      const f32x16 acc = score_tile(a.g + grow * a.ld_g, qrow, h, groups, tail);
      // ---- lane (r, h): query q0 + r, gallery rows base + (i & 3) + 8 (i >> 2) + 4 h
      if (q_valid) {
        const uint32_t tk = (uint32_t)mine.meta[1];
        const int ti = mine.meta[2];
        int top = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int64_t row = base + (i & 3) + 8 * (i >> 2) + 4 * h;
          const uint32_t key = key_of(__float_as_uint(acc[i]));
          if (row < row_end && beats(key, (int)row, tk, ti)) top = buffer_append(mine, key, (int)row);
        }
        if (top > cap - kStepRows) *flag = 1;          // the next step could overflow this buffer
      }
    }
    __syncthreads();
    if (*flag) {                                       // written before the barrier, cleared two steps on: one value for all
      for (int qi = wave; qi < kQTile; qi += kWaves) {
        const Buffer b = {buf_key + qi * cap, buf_idx + qi * cap, tile_meta(smem, pitch, E, qi), cap, qi};
        prune_to_k<kMaxCap / 64>(b, k, lane);
      }
      __syncthreads();
    }
    f = fn;
  }
  for (int qi = wave; qi < kQTile; qi += kWaves) {
    const Buffer b = {buf_key + qi * cap, buf_idx + qi * cap, tile_meta(smem, pitch, E, qi), cap, qi};
    prune_to_k<kMaxCap / 64>(b, k, lane);
  }
  __syncthreads();

  // ---- k pairs per query, unsorted; an empty entry (a chunk of fewer than k rows): key 0, row INT_MAX
  for (int i = tid; i < kQTile * k; i += kThreads) {
    const int qi = i / k, j = i - qi * k;
    if (q0 + qi >= a.B) continue;
    const Buffer b = {buf_key + qi * cap, buf_idx + qi * cap, tile_meta(smem, pitch, E, qi), cap, qi};
    const int n = min(b.meta[0], k);
    const int p = slot_at(b, j);
    const int64_t out = ((int64_t)(q0 + qi) * a.chunks + blockIdx.x) * k + j;
    a.ws_key[out] = j < n ? b.key[p] : kRetired;
    a.ws_idx[out] = j < n ? b.idx[p] : INT_MAX;
  }
}

__global__ void __launch_bounds__(kThreads) embed_wide_pass2(SelectArgs a) { select_pass2(a); }

// pairs per buffer that fit LDS next to the query tile: 32 (2 E + 16) + 32 * 8 * cap <= 160 KiB
int cap_fit(int E) { return (kLdsBudget - kQTile * query_pitch(E)) / (kQTile * 8); }

int wide_max_k(int E) {
  if (E < TFIMM_EMBED_MIN_E || E > TFIMM_EMBED_MAX_E || E % 16 != 0) return 0;
  const int m = cap_fit(E) - kStepRows;
  return m > TFIMM_EMBED_WIDE_MAX_K ? TFIMM_EMBED_WIDE_MAX_K : m;
}

// validates (B, N, E, k, chunk) and resolves chunk = 0; returns what is wrong or nullptr
const char* resolve(int B, int N, int E, int k, int* chunk, int64_t* chunks) {
  if (E < TFIMM_EMBED_MIN_E || E > TFIMM_EMBED_MAX_E || E % 16 != 0) return "E";
  if (N < 1) return "N";
  if (k < 1 || k > N || k > TFIMM_EMBED_WIDE_MAX_K) return "k";
  if (*chunk < 0 || *chunk % kRowTile != 0) return "chunk";
  if (B < 0 || B > TFIMM_EMBED_MAX_B) return "B";
  if (k > wide_max_k(E)) return "fit";
  if (*chunk == 0) *chunk = choose_chunk(B, N, k);
  *chunks = cdiv64(N, *chunk);
  return nullptr;
}

int wide_fail(const char* what, int B, int N, int E, int k, int chunk) {
  if (what[0] == 'E')
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_wide: E=%d, must be a multiple of 16 in [%d, TFIMM_EMBED_MAX_E = %d]", E, TFIMM_EMBED_MIN_E,
               TFIMM_EMBED_MAX_E);
  if (what[0] == 'N') TFIMM_FAIL(TFIMM_EINVAL, "embed_search_wide: N=%d, must be in [1, 2^31)", N);
  if (what[0] == 'k')
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_wide: k=%d, must be in [1, min(N = %d, TFIMM_EMBED_WIDE_MAX_K = %d)]", k, N,
               TFIMM_EMBED_WIDE_MAX_K);
  if (what[0] == 'B') TFIMM_FAIL(TFIMM_EINVAL, "embed_search_wide: B=%d, must be in [0, TFIMM_EMBED_MAX_B = %d]", B, TFIMM_EMBED_MAX_B);
  if (what[0] == 'f')
    TFIMM_FAIL(TFIMM_EINVAL,
               "embed_search_wide: E=%d with k=%d: 32 buffers of k + %d pairs do not fit %d KiB of LDS next to the query tile; "
               "tfimm_hip_embed_search_wide_max_k(%d) = %d",
               E, k, kStepRows, kLdsBudget / 1024, E, wide_max_k(E));
  TFIMM_FAIL(TFIMM_EINVAL, "embed_search_wide: chunk=%d, must be 0 or a positive multiple of 32", chunk);
}

}  // namespace

extern "C" int tfimm_hip_embed_search_wide_max_k(int E) { return wide_max_k(E); }

extern "C" int64_t tfimm_hip_embed_search_wide_workspace(int B, int N, int E, int k, int chunk) {
  int64_t chunks = 0;
  const char* bad = resolve(B, N, E, k, &chunk, &chunks);
  if (bad) return wide_fail(bad, B, N, E, k, chunk);
  return (int64_t)(B > 0 ? B : 1) * chunks * k * 8;
}

extern "C" int tfimm_hip_embed_search_wide(const float* q, int64_t ld_q, int B, const void* g, int64_t ld_g, int N, int E, int k,
                                           int chunk, float* scores, int32_t* indices, void* workspace, int64_t workspace_bytes,
                                           void* stream) {
  if (!q) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_wide: q is null");
  if (!g) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_wide: g is null");
  if (!scores) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_wide: scores is null");
  if (!indices) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_wide: indices is null");
  if (!workspace) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_wide: workspace is null");
  if ((uintptr_t)g & 15) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_wide: g must be 16-byte aligned");
  if (((uintptr_t)q | (uintptr_t)scores | (uintptr_t)indices | (uintptr_t)workspace) & 3)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_wide: q, scores, indices and workspace hold 4-byte elements and must be 4-byte aligned");
  int64_t chunks = 0;
  const char* bad = resolve(B, N, E, k, &chunk, &chunks);
  if (bad) return wide_fail(bad, B, N, E, k, chunk);
  if (ld_q < E) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_wide: ld_q=%lld is smaller than E=%d", (long long)ld_q, E);
  if (ld_g < E || ld_g % 8 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_wide: ld_g=%lld, must be a multiple of 8 elements and at least E=%d", (long long)ld_g, E);
  const int64_t need = (int64_t)(B > 0 ? B : 1) * chunks * k * 8;
  if (workspace_bytes < need)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_wide: workspace_bytes=%lld, tfimm_hip_embed_search_wide_workspace asks for %lld",
               (long long)workspace_bytes, (long long)need);
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

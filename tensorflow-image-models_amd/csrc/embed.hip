// The embedding end (include/tfimm_hip.h; the CPU restatement of both rules is tests/embed_ref.py).
//
// tfimm_hip_l2_normalize: y = x * (1 / sqrt(max(sum(x^2), 1e-12))) per row (tf.math.l2_normalize), float32 on both sides.
// One wave per row, four rows per workgroup.  Lane l sums the squares of columns l, l + 64, ... in ascending order, the 64
// partial sums go through the fixed six-step butterfly (float addition commutes exactly: every lane holds the same bits), the
// square root and the division are the correctly rounded ones.  Rows never mix: bit-reproducible and independent of B.
//
// tfimm_hip_embed_search: for B float32 queries the k gallery rows (bf16, [N][ld_g]) with the largest inner products, in two
// launches and without the B x N score matrix.
//
//   Pass 1, grid (gallery chunks, query tiles of 32), 256 threads.  The query tile is rounded to bf16 once and kept in LDS
//   (row pitch 2 E + 16 bytes: pitch / 16 is odd, so the 16 lanes of a ds_read_b128 pass fall on 16 distinct 16-byte bank
//   groups).  Every wave walks 32-row gallery tiles of its chunk; the tile is the A operand of v_mfma_f32_32x32x16_bf16 and
//   comes straight from global memory: lane (r, h) holds A[row r][k = 8h .. 8h+7], 16 contiguous bytes of gallery row r.  k is
//   permuted identically on both operands so that within 64 columns lane (r, h) owns columns 32h .. 32h+31: it reads 64
//   contiguous bytes of its row per four MFMA steps (the < 64 columns behind the last full group use the plain map).  The
//   32 x 32 float32 tile has the query on the lane (column = lane & 31) and 16 gallery rows in the registers.  (The query
//   tile and this loop are embed_score.h, shared with the other gallery searches; the argument checks are embed_check.h.)
//   Every (wave, query) owns a list of k (key, row) pairs in LDS, ordered by (key descending, row ascending) -- the keys of
//   topk_select.h, 0 = empty.  A lane compares its 16 scores with the list's last entry and inserts the few that beat it; the
//   two lanes of a query (h = 0, 1) take turns, so a list has one writer at a time.  The list is the k best of what the wave
//   has seen under a total order, whatever the order of insertion.  At the end of the chunk thread q merges the waves' lists
//   of query q and writes k (key, row) pairs to the workspace: [query][chunk][k].
//
//   Pass 2, one workgroup per query: chunks * k candidate keys into LDS, k selection rounds of topk_select.h.  Chunks are in
//   ascending gallery order and every list has equal keys in ascending row order, so among equal keys candidate position
//   is gallery order: the rounds' tie rule (lower position) is the search's (lower index).
//
// No atomics, no scratch memory, every reduction in a fixed order; a score is a function of its query and its gallery row
// alone (the k loop does not depend on B, chunk or the tile's other queries), and the selection is by a total order: results
// are bit-reproducible and independent of B and chunk.
#include "embed_check.h"
#include "embed_score.h"
#include "topk_select.h"

namespace {

using namespace topk_sel;
using namespace embed_score;
using namespace embed_check;

// ------------------------------------------------------------------------------------------------------------------------
// l2_normalize
// ------------------------------------------------------------------------------------------------------------------------
constexpr int kNormRows = 4;   // rows (= waves) per workgroup

__global__ void __launch_bounds__(64 * kNormRows) l2_normalize_kernel(const float* x, int64_t ld_x, float* y,
                                                                       int64_t ld_y, int B, int E) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kNormRows + (threadIdx.x >> 6);
  if (row >= B) return;
  const float* xr = x + row * ld_x;
  float* yr = y + row * ld_y;
  float s = 0.f;
  for (int c = lane; c < E; c += 64) {
    const float v = xr[c];
    s = __fmaf_rn(v, v, s);
  }
  s = wave_sum(s);
  const float inv = __fdiv_rn(1.0f, __fsqrt_rn(fmaxf(s, 1e-12f)));
  for (int c = lane; c < E; c += 64) yr[c] = xr[c] * inv;
}

// ------------------------------------------------------------------------------------------------------------------------
// embed_search
// ------------------------------------------------------------------------------------------------------------------------
static_assert(TFIMM_EMBED_MAX_B == 65535 * kQTile, "query tiles are grid.y");
constexpr int kPass2MaxCand = 16384;            // candidate keys pass 2 holds in LDS (64 KiB)

struct SearchArgs {
  const float* q;
  const uint16_t* g;
  uint32_t* ws_key;    // [B][chunks][k]
  int32_t* ws_idx;     // [B][chunks][k]
  int64_t ld_q, ld_g;
  int B, N, E, k, chunk, chunks, list_waves;
};

__device__ __forceinline__ void list_insert(uint32_t* lk, int* li, int k, uint32_t key, int row) {
  int j = k - 1;
  while (j > 0) {
    const uint32_t pk = lk[j - 1];
    const int pi = li[j - 1];
    if (!beats(key, row, pk, pi)) break;
    lk[j] = pk;
    li[j] = pi;
    --j;
  }
  lk[j] = key;
  li[j] = row;
}

__global__ void __launch_bounds__(kThreads) embed_search_pass1(SearchArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E = a.E, k = a.k;
  const int pitch = query_pitch(E);                               // bytes per query row in LDS
  uint32_t* list_key = reinterpret_cast<uint32_t*>(smem + (size_t)kQTile * pitch);   // [list_waves][32][k]
  int* list_idx = reinterpret_cast<int*>(list_key + a.list_waves * kQTile * k);
  const int q0 = blockIdx.y * kQTile;

  // ---- the query tile -> bf16 in LDS (queries past B: zeros), the lists -> empty
  load_query_tile(smem, a.q, a.ld_q, q0, a.B, E, tid, kThreads);
  for (int i = tid; i < a.list_waves * kQTile * k; i += kThreads) {
    list_key[i] = kRetired;
    list_idx[i] = INT_MAX;
  }
  __syncthreads();

  const int64_t row_begin = (int64_t)blockIdx.x * a.chunk;
  const int64_t row_end = min(row_begin + (int64_t)a.chunk, (int64_t)a.N);
  const int r = lane & 31, h = lane >> 5;
  const bool q_valid = q0 + r < a.B;
  const int groups = E / 64, tail = (E % 64) / 16;

  if (wave < a.list_waves) {
    uint32_t* lk = list_key + (wave * kQTile + r) * k;
    int* li = list_idx + (wave * kQTile + r) * k;
    const unsigned char* qrow = smem + (size_t)r * pitch;
    for (int64_t base = row_begin + (int64_t)wave * kRowTile; base < row_end; base += (int64_t)a.list_waves * kRowTile) {
      // a row past the gallery reads the last row instead (its scores are never looked at)
      const int64_t grow = min(base + r, (int64_t)a.N - 1);
      const uint16_t* ga = a.g + grow * a.ld_g;
      const f32x16 acc = score_tile(ga, qrow, h, groups, tail);
      // ---- lane (r, h): query q0 + r, gallery rows base + (i & 3) + 8 (i >> 2) + 4 h.  h = 0 inserts, then h = 1.
#pragma unroll
      for (int phase = 0; phase < 2; ++phase) {
        if (h == phase && q_valid) {
          uint32_t tk = lk[k - 1];
          int ti = li[k - 1];
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int64_t row = base + (i & 3) + 8 * (i >> 2) + 4 * h;
            const uint32_t key = key_of(__float_as_uint(acc[i]));
            if (row < row_end && beats(key, (int)row, tk, ti)) {
              list_insert(lk, li, k, key, (int)row);
              tk = lk[k - 1];
              ti = li[k - 1];
            }
          }
        }
        // the other half-wave reads what this one wrote: same wave, LDS operations in program order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    }
  }
  __syncthreads();

  // ---- thread q: merge the waves' lists of query q (each ordered; heads compared under the same total order)
  if (tid < kQTile && q0 + tid < a.B) {
    int pos[kWaves] = {0, 0, 0, 0};
    const int64_t out = ((int64_t)(q0 + tid) * a.chunks + blockIdx.x) * k;
    for (int j = 0; j < k; ++j) {
      uint32_t bk = kRetired;
      int bi = INT_MAX, bw = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        if (w < a.list_waves && pos[w] < k) {
          const uint32_t ck = list_key[(w * kQTile + tid) * k + pos[w]];
          const int ci = list_idx[(w * kQTile + tid) * k + pos[w]];
          if (beats(ck, ci, bk, bi)) { bk = ck; bi = ci; bw = w; }
        }
      }
#pragma unroll
      for (int w = 0; w < kWaves; ++w) pos[w] += (w == bw) ? 1 : 0;
      a.ws_key[out + j] = bk;      // an empty entry (a chunk of fewer than k rows): key 0, row INT_MAX
      a.ws_idx[out + j] = bi;
    }
  }
}

struct SelectArgs {
  const uint32_t* ws_key;
  const int32_t* ws_idx;
  uint32_t* scores;    // float32 bits
  int32_t* indices;
  int cand, k;         // cand = chunks * k
};

__global__ void __launch_bounds__(kThreads) embed_search_pass2(SelectArgs a) {
  extern __shared__ uint32_t keys[];   // [cand]
  __shared__ uint32_t w_key[kWaves];
  __shared__ int w_idx[kWaves];
  const int tid = threadIdx.x;
  const uint32_t* src = a.ws_key + (int64_t)blockIdx.x * a.cand;
  for (int c = tid; c < a.cand; c += kThreads) keys[c] = src[c];
  __syncthreads();
  for (int j = 0; j < a.k; ++j) {
    uint32_t k0;
    int p0;
    select_round(keys, a.cand, tid, w_key, w_idx, k0, p0);
    if (tid == 0 && p0 < a.cand) {     // (k <= N: a round always has a winner; the test keeps a broken invariant inside the list)
      const int64_t o = (int64_t)blockIdx.x * a.k + j;
      a.scores[o] = bits_of(k0);
      a.indices[o] = a.ws_idx[(int64_t)blockIdx.x * a.cand + p0];
      keys[p0] = kRetired;
    }
    __syncthreads();
  }
}

// rows per workgroup of pass 1 when the caller leaves the choice: enough chunks to fill the chip several times over (256 CUs,
// a few workgroups each) however few query tiles there are, at least 128 rows (one tile per wave), within what pass 2 holds
int choose_chunk(int B, int N, int k) {
  const int64_t qtiles = B > kQTile ? (B + kQTile - 1) / kQTile : 1;
  int64_t want = 2048 / qtiles;
  if (want < 64) want = 64;
  if (want > kPass2MaxCand / k) want = kPass2MaxCand / k;
  int64_t chunk = cdiv64(cdiv64(N, want), 128) * 128;
  if (chunk < 128) chunk = 128;
  return (int)chunk;
}

int pass1_lds_bytes(int E, int k, int list_waves) { return kQTile * query_pitch(E) + list_waves * kQTile * k * 8; }

constexpr const char* kFn = "embed_search";

// a chunk of the wrong form, or one that leaves pass 2 more candidates than it holds
int chunk_fail(int chunk, int N, int k) {
  TFIMM_FAIL(TFIMM_EINVAL, "%s: chunk=%d, must be 0 or a positive multiple of 32 with ceil(N / chunk) * k <= %d (N=%d, k=%d)", kFn, chunk,
             kPass2MaxCand, N, k);
}

// validates (B, N, E, k, chunk) and resolves chunk = 0; returns 0 or TFIMM_EINVAL with the message set
int resolve_chunk(int B, int N, int E, int k, int* chunk, int64_t* chunks) {
  TFIMM_EMBED_TRY(check_E(kFn, E));
  TFIMM_EMBED_TRY(check_N(kFn, N));
  if (k < 1 || k > N || k > TFIMM_EMBED_MAX_K)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: k=%d, must be in [1, min(N = %d, TFIMM_EMBED_MAX_K = %d)]", kFn, k, N, TFIMM_EMBED_MAX_K);
  if (*chunk < 0 || *chunk % kRowTile != 0) return chunk_fail(*chunk, N, k);
  TFIMM_EMBED_TRY(check_B(kFn, B));
  if (*chunk == 0) *chunk = choose_chunk(B, N, k);
  *chunks = cdiv64(N, *chunk);
  if (*chunks * k > kPass2MaxCand) return chunk_fail(*chunk, N, k);
  return 0;
}

// [B][chunks][k] keys and rows
int64_t workspace_need(int B, int64_t chunks, int k) { return (int64_t)(B > 0 ? B : 1) * chunks * k * 8; }

}  // namespace

extern "C" int tfimm_hip_l2_normalize(const float* x, int64_t ld_x, int B, int E, float* y, int64_t ld_y, void* stream) {
  if (!x) TFIMM_FAIL(TFIMM_EINVAL, "l2_normalize: x is null");
  if (!y) TFIMM_FAIL(TFIMM_EINVAL, "l2_normalize: y is null");
  if (((uintptr_t)x | (uintptr_t)y) & 3) TFIMM_FAIL(TFIMM_EINVAL, "l2_normalize: x and y hold float32 and must be 4-byte aligned");
  if (E < 1) TFIMM_FAIL(TFIMM_EINVAL, "l2_normalize: E=%d, must be at least 1", E);
  if (ld_x < E) TFIMM_FAIL(TFIMM_EINVAL, "l2_normalize: ld_x=%lld is smaller than E=%d", (long long)ld_x, E);
  if (ld_y < E) TFIMM_FAIL(TFIMM_EINVAL, "l2_normalize: ld_y=%lld is smaller than E=%d", (long long)ld_y, E);
  if (B < 0) TFIMM_FAIL(TFIMM_EINVAL, "l2_normalize: B=%d is negative", B);
  if (B == 0) return 0;
  TFIMM_LAUNCH(l2_normalize_kernel, dim3((unsigned)((B + kNormRows - 1) / kNormRows)), dim3(64 * kNormRows), 0, (hipStream_t)stream, x, ld_x,
               y, ld_y, B, E);
  return 0;
}

extern "C" int64_t tfimm_hip_embed_search_workspace(int B, int N, int E, int k, int chunk) {
  int64_t chunks = 0;
  TFIMM_EMBED_TRY(resolve_chunk(B, N, E, k, &chunk, &chunks));
  return workspace_need(B, chunks, k);
}

extern "C" int tfimm_hip_embed_search(const float* q, int64_t ld_q, int B, const void* g, int64_t ld_g, int N, int E, int k, int chunk,
                                      float* scores, int32_t* indices, void* workspace, int64_t workspace_bytes, void* stream) {
  TFIMM_EMBED_TRY(check_pointers(kFn, {{"q", q, 4}, {"g", g, 16}, {"scores", scores, 4}, {"indices", indices, 4}, {"workspace", workspace, 4}}));
  int64_t chunks = 0;
  TFIMM_EMBED_TRY(resolve_chunk(B, N, E, k, &chunk, &chunks));
  TFIMM_EMBED_TRY(check_ld_q(kFn, ld_q, E));
  TFIMM_EMBED_TRY(check_ld_g(kFn, ld_g, E));
  TFIMM_EMBED_TRY(check_workspace(kFn, workspace_bytes, workspace_need(B, chunks, k)));
  if (B == 0) return 0;

  // as many list-keeping waves as LDS allows next to the query tile: 4, else 2, else 1 (E = 2048 with k > 32 only)
  int list_waves = kWaves;
  while (list_waves > 1 && pass1_lds_bytes(E, k, list_waves) > kLdsBudget) list_waves >>= 1;
  static tfimm_once_t ready;
  if (ready.need()) {
    TFIMM_HIP_CHECK(hipFuncSetAttribute((const void*)embed_search_pass1, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
    TFIMM_HIP_CHECK(hipFuncSetAttribute((const void*)embed_search_pass2, hipFuncAttributeMaxDynamicSharedMemorySize, kPass2MaxCand * 4));
    ready.mark();
  }
  SearchArgs a;
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
  a.list_waves = list_waves;
  const int qtiles = (B + kQTile - 1) / kQTile;
  TFIMM_LAUNCH(embed_search_pass1, dim3((unsigned)chunks, (unsigned)qtiles), dim3(kThreads), (size_t)pass1_lds_bytes(E, k, list_waves),
               (hipStream_t)stream, a);
  SelectArgs s;
  s.ws_key = a.ws_key;
  s.ws_idx = a.ws_idx;
  s.scores = reinterpret_cast<uint32_t*>(scores);
  s.indices = indices;
  s.cand = (int)(chunks * k);
  s.k = k;
  TFIMM_LAUNCH(embed_search_pass2, dim3((unsigned)B), dim3(kThreads), (size_t)((s.cand + 3) / 4 * 4) * 4, (hipStream_t)stream, s);
  return 0;
}

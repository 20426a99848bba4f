// tfimm_hip_embed_search_lists (include/tfimm_hip.h): the gallery search over INVERTED LISTS.  The gallery rows
// stand in list order (list l is positions offsets[l] : offsets[l + 1], ids[pos] the original row of a position, ascending
// inside a list), every query names nprobe lists, and only their rows are scored -- by the loop of the exact searches
// (embed_score.h), so a returned score has the bits tfimm_hip_embed_search gives for that row.  tests/index_ref.py restates the
// rule on the CPU.
//
//   Pass 1, grid (nprobe * parts, B), 256 threads: one workgroup owns one (query, probe slot, part of the list).  The query
//   lives in LDS as bf16 once, 2 E bytes; every wave walks 32-row tiles of the part through score_tile with all 32 columns of
//   the B operand that one query (every lane reads the same LDS row, as embed_coarse_rerank does), so each of a tile's 32
//   scores arrives in 32 lanes.  Lane (r, h) with r < 16 takes register r -- tile row (r & 3) + 8 (r >> 2) + 4 h -- by a
//   compile-time chain of selects: the threshold test and the append are one step on 32 lanes, not sixteen on two.  The
//   workgroup keeps ONE buffer of cap = k + 256 pairs (embed_buffer.h) keyed by (score key, POSITION); the step structure is
//   embed_wide_pass1's: a step is one tile per wave (128 rows), one barrier per step, the flags of three consecutive steps
//   are three different bytes, wave 0 prunes when a count exceeds cap - 128.  Inside a list order by position is order by
//   original row, so the k best pairs of the part under (key, position) are its k best under the rule's (key, row); they go
//   to workspace[b][slot * parts + part][k] with ids[pos] in place of the position, empty entries as key 0, row INT_MAX.  A
//   slot that names no list (outside [0, L)), a slot whose list an earlier slot of the query names already (a repeated list
//   counts once: pass 2 ranks distinct pairs) and an empty part write k empty entries.  The workgroups of slot 0, part 0 also
//   write the query's k outputs as "none" (-1, -inf): pass 2 writes the survivors only.
//   LDS is 2 E + 16 + 8 cap bytes -- at most 8208 at E = 2048, k = 256 --: count, threshold and the three flags in the 16 bytes
//   behind the query.  Many workgroups per CU, where the full scans have one or two.
//
//   Pass 2, one workgroup per query: select_pass2 of embed_buffer.h over the nprobe * parts * k pairs, unchanged.
//
// The result is a function of the scores and the lists alone: independent of B, of parts and of the order in which waves arrive.
#include "embed_buffer.h"

namespace {

using namespace embed_buffer;

constexpr int kMaxParts = 64;
constexpr int kCapExtra = 2 * kStepRows;     // cap = k + 256: a prune every other step at the earliest
static_assert(TFIMM_EMBED_WIDE_MAX_K + kCapExtra <= kMaxCap, "the pruning wave holds the whole buffer in registers");
static_assert(TFIMM_EMBED_LISTS_MAX_PROBE * kMaxParts <= 65535, "nprobe * parts is a grid dimension");

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

__global__ void __launch_bounds__(kThreads, 4) embed_lists_pass1(ListsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E = a.E, k = a.k, cap = a.cap;
  int* meta = reinterpret_cast<int*>(smem + 2 * E);                       // count, threshold key, threshold position, flags
  unsigned char* flags = reinterpret_cast<unsigned char*>(meta + 3);     // three bytes: step mod 3
  uint32_t* buf_key = reinterpret_cast<uint32_t*>(smem + 2 * E + 16);     // [cap]
  int* buf_idx = reinterpret_cast<int*>(buf_key + cap);                   // [cap]
  const int b = blockIdx.y;
  const int slot = blockIdx.x / a.parts, part = blockIdx.x - slot * a.parts;
  const int64_t out = ((int64_t)b * gridDim.x + blockIdx.x) * k;

  if (blockIdx.x == 0)                                   // what pass 2 leaves alone: the slots behind the survivors
    for (int j = tid; j < k; j += kThreads) {
      a.scores[(int64_t)b * k + j] = 0xff800000u;        // -inf
      a.indices[(int64_t)b * k + j] = -1;
    }

  // ---- this workgroup's rows: positions [begin, end) of the list order; the same values in every thread
  const int32_t* mine_probes = a.probes + (int64_t)b * a.ld_p;
  const int l = mine_probes[slot];
  // a list that an earlier slot of this query names already counts ONCE: this slot is "no list".  select_pass2 ranks a pair by
  // the number of pairs that beat it, which takes distinct (key, row) pairs; two copies of a list would hand it equal ones.
  bool first = true;
  for (int s = 0; s < slot; ++s) first = first && mine_probes[s] != l;      // uniform: scalar loads, at most 255
  int64_t begin = 0, end = 0;
  if (first && l >= 0 && l < a.L) {
    const int lo = clamp_pos(a.offsets[l], a.N), hi = clamp_pos(a.offsets[l + 1], a.N);
    if (hi > lo) {
      const int64_t per = ((int64_t)(hi - lo) + a.parts - 1) / a.parts;
      begin = min((int64_t)lo + part * per, (int64_t)hi);
      end = min(begin + per, (int64_t)hi);
    }
  }
  if (end <= begin) {                                    // no list, a repeated or an empty list, or a part behind the last row
    for (int j = tid; j < k; j += kThreads) {
      a.ws_key[out + j] = kRetired;
      a.ws_idx[out + j] = INT_MAX;
    }
    return;
  }

  const float* src = a.q + (int64_t)b * a.ld_q;
  for (int i = tid; i < E / 2; i += kThreads)
    reinterpret_cast<uint32_t*>(smem)[i] = bf16_rne(__float_as_uint(src[2 * i])) | (bf16_rne(__float_as_uint(src[2 * i + 1])) << 16);
  if (tid == 0) {
    meta[0] = 0;
    meta[1] = (int)kRetired;
    meta[2] = INT_MAX;
    meta[3] = 0;
  }
  __syncthreads();

  const int r = lane & 31, h = lane >> 5;
  const int groups = E / 64, tail = (E % 64) / 16;
  const Buffer buf = {buf_key, buf_idx, meta, cap, 0};
  const int steps = (int)((end - begin + kStepRows - 1) / kStepRows);
  const int mine = (r & 3) + 8 * ((r & 15) >> 2) + 4 * h;       // the tile row whose score this lane takes (r < 16)

  int f = 0;                                             // this step's flag: step mod 3
  for (int s = 0; s < steps; ++s) {
    const int fn = f == 2 ? 0 : f + 1;
    if (tid == 0) flags[fn] = 0;                         // the next step's: last read behind the barrier before last
    const int64_t base = begin + (int64_t)s * kStepRows + wave * kRowTile;
    if (base < end) {
      // a tile row past the part reads the gallery's last row instead (its scores are never looked at)
      const int64_t grow = min(base + r, (int64_t)a.N - 1);
      const f32x16 acc = score_tile(a.g + grow * a.ld_g, smem, h, groups, tail);
      float v = acc[0];
#pragma unroll
      for (int i = 1; i < 16; ++i) v = (r & 15) == i ? acc[i] : v;
      const int64_t pos = base + mine;
      if (r < 16 && pos < end) {
        const uint32_t key = key_of(__float_as_uint(v));
        if (beats(key, (int)pos, (uint32_t)meta[1], meta[2]) && buffer_append(buf, key, (int)pos) > cap - kStepRows)
          flags[f] = 1;                                  // the next step could overflow the buffer
      }
    }
    __syncthreads();
    if (flags[f]) {                                      // written before the barrier, cleared two steps on: one value for all
      if (wave == 0) prune_to_k<kMaxCap / 64>(buf, k, lane);
      __syncthreads();
    }
    f = fn;
  }
  if (wave == 0) prune_to_k<kMaxCap / 64>(buf, k, lane);
  __syncthreads();

  // ---- k pairs, unsorted, the original row in place of the position; an empty entry (fewer than k rows): key 0, row INT_MAX
  const int n = min(meta[0], k);
  for (int j = tid; j < k; j += kThreads) {
    uint32_t key = kRetired;
    int id = INT_MAX;
    if (j < n) {
      const int pos = buf_idx[j];
      key = buf_key[j];
      id = pos >= 0 && pos < a.N ? a.ids[pos] : INT_MAX;   // (always inside: the test keeps a broken invariant from reading)
    }
    a.ws_key[out + j] = key;
    a.ws_idx[out + j] = id;
  }
}

__global__ void __launch_bounds__(kThreads) embed_lists_pass2(SelectArgs a) { select_pass2(a); }

// validates the shape of a call and resolves parts = 0; returns 0 or TFIMM_EINVAL with the message set
int resolve(int B, int N, int E, int L, int nprobe, int k, int* parts) {
  if (E < TFIMM_EMBED_MIN_E || E > TFIMM_EMBED_MAX_E || E % 16 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: E=%d, must be a multiple of 16 in [%d, TFIMM_EMBED_MAX_E = %d]", E, TFIMM_EMBED_MIN_E,
               TFIMM_EMBED_MAX_E);
  if (N < 1) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: N=%d, must be in [1, 2^31)", N);
  if (L < 1 || L > TFIMM_CLUSTER_MAX_C)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: L=%d, must be in [1, TFIMM_CLUSTER_MAX_C = %d]", L, TFIMM_CLUSTER_MAX_C);
  if (nprobe < 1 || nprobe > TFIMM_EMBED_LISTS_MAX_PROBE)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: nprobe=%d, must be in [1, TFIMM_EMBED_LISTS_MAX_PROBE = %d]", nprobe,
               TFIMM_EMBED_LISTS_MAX_PROBE);
  if (k < 1 || k > TFIMM_EMBED_WIDE_MAX_K)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: k=%d, must be in [1, TFIMM_EMBED_WIDE_MAX_K = %d]", k, TFIMM_EMBED_WIDE_MAX_K);
  if (*parts < 0 || *parts > kMaxParts)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: parts=%d, must be 0 (the library chooses) or in [1, %d]", *parts, kMaxParts);
  if (*parts == 0) *parts = 1;
  if (B < 0 || B > 65535) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: B=%d, must be in [0, 65535] (a grid dimension)", B);
  return 0;                                              // nprobe * parts, the other grid dimension, is at most 16384
}

// [B][nprobe * parts][k] keys and rows
int64_t workspace_need(int B, int nprobe, int k, int parts) { return (int64_t)(B > 0 ? B : 1) * nprobe * parts * k * 8; }

}  // namespace

extern "C" int64_t tfimm_hip_embed_search_lists_workspace(int B, int N, int E, int L, int nprobe, int k, int parts) {
  const int rc = resolve(B, N, E, L, nprobe, k, &parts);
  if (rc) return rc;
  return workspace_need(B, nprobe, k, parts);
}

extern "C" int tfimm_hip_embed_search_lists(const float* q, int64_t ld_q, int B, const void* g, int64_t ld_g, int N, int E,
                                            const int32_t* ids, const int32_t* offsets, int L, const int32_t* probes, int64_t ld_p,
                                            int nprobe, int k, int parts, float* scores, int32_t* indices, void* workspace,
                                            int64_t workspace_bytes, void* stream) {
  if (!q) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: q is null");
  if (!g) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: g is null");
  if (!ids) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: ids is null");
  if (!offsets) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: offsets is null");
  if (!probes) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: probes is null");
  if (!scores) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: scores is null");
  if (!indices) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: indices is null");
  if (!workspace) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: workspace is null");
  if ((uintptr_t)g & 15) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: g must be 16-byte aligned");
  if (((uintptr_t)q | (uintptr_t)ids | (uintptr_t)offsets | (uintptr_t)probes | (uintptr_t)scores | (uintptr_t)indices |
       (uintptr_t)workspace) & 3)
    TFIMM_FAIL(TFIMM_EINVAL,
               "embed_search_lists: q, ids, offsets, probes, scores, indices and workspace hold 4-byte elements and must be 4-byte aligned");
  const int rc = resolve(B, N, E, L, nprobe, k, &parts);
  if (rc) return rc;
  if (ld_q < E) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: ld_q=%lld is smaller than E=%d", (long long)ld_q, E);
  if (ld_g < E || ld_g % 8 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: ld_g=%lld, must be a multiple of 8 elements and at least E=%d", (long long)ld_g, E);
  if (ld_p < nprobe) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: ld_p=%lld is smaller than nprobe=%d", (long long)ld_p, nprobe);
  const int64_t need = workspace_need(B, nprobe, k, parts);
  if (workspace_bytes < need)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists: workspace_bytes=%lld, tfimm_hip_embed_search_lists_workspace asks for %lld",
               (long long)workspace_bytes, (long long)need);
  if (B == 0) return 0;

  const int64_t pairs = (int64_t)nprobe * parts * k;      // per query
  ListsArgs a;
  a.q = q;
  a.g = reinterpret_cast<const uint16_t*>(g);
  a.ids = ids;
  a.offsets = offsets;
  a.probes = probes;
  a.ws_key = reinterpret_cast<uint32_t*>(workspace);
  a.ws_idx = reinterpret_cast<int32_t*>(a.ws_key + (int64_t)B * pairs);
  a.scores = reinterpret_cast<uint32_t*>(scores);
  a.indices = indices;
  a.ld_q = ld_q;
  a.ld_g = ld_g;
  a.ld_p = ld_p;
  a.N = N;
  a.E = E;
  a.L = L;
  a.nprobe = nprobe;
  a.k = k;
  a.parts = parts;
  a.cap = k + kCapExtra;
  TFIMM_LAUNCH(embed_lists_pass1, dim3((unsigned)(nprobe * parts), (unsigned)B), dim3(kThreads), (size_t)(2 * E + 16 + 8 * a.cap),
               (hipStream_t)stream, a);
  SelectArgs s;
  s.ws_key = a.ws_key;
  s.ws_idx = a.ws_idx;
  s.scores = a.scores;
  s.indices = indices;
  s.cand = pairs;
  s.k = k;
  TFIMM_LAUNCH(embed_lists_pass2, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, s);
  return 0;
}

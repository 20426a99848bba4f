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
//   that of buffered_steps with its own append, the single buffer being another shape than a tile of 32: a step is one tile
//   per wave (128 rows), one barrier per step, the flags of three consecutive steps (StepFlags) are three different bytes,
//   wave 0 prunes when a count exceeds cap - 128.  Inside a list order by position is order by
//   original row, so the k best pairs of the part under (key, position) are its k best under the rule's (key, row); they go
//   to workspace[b][slot * parts + part][k] with ids[pos] in place of the position, empty entries as key 0, row INT_MAX.  A
//   slot that is no LIVE PAIR and an empty part write k empty entries: that rule, the CUT of a list into parts and the
//   arguments are embed_lists.h, shared with embed_lists_grouped.hip.  The workgroups of slot 0, part 0 also
//   write the query's k outputs as "none" (-1, -inf): pass 2 writes the survivors only.
//   LDS is 2 E + 16 + 8 cap bytes -- at most 8208 at E = 2048, k = 256 --: count, threshold and the three flags in the 16 bytes
//   behind the query.  Many workgroups per CU, where the full scans have one or two.
//
//   Pass 2, one workgroup per query: select_pass2 of embed_buffer.h over the nprobe * parts * k pairs, unchanged.
//
// The result is a function of the scores and the lists alone: independent of B, of parts and of the order in which waves arrive.
#include "embed_lists.h"

namespace {

using namespace embed_lists;

constexpr const char* kFn = "embed_search_lists";
constexpr int kCapExtra = 2 * kStepRows;     // cap = k + 256: a prune every other step at the earliest
static_assert(TFIMM_EMBED_WIDE_MAX_K + kCapExtra <= kMaxCap, "the pruning wave holds the whole buffer in registers");

__global__ void __launch_bounds__(kThreads, 4) embed_lists_pass1(ListsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
  const int E = a.E, k = a.k, cap = a.cap;
  int* meta = reinterpret_cast<int*>(smem + 2 * E);                       // count, threshold key, threshold position, flags
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

  // ---- this workgroup's rows: positions [begin, end) of the list order; the same values in every thread (scalar loads, at
  // most 255 earlier slots)
  const int32_t* probes = a.probes + (int64_t)b * a.ld_p;
  Cut cut = {0, 0};
  if (live_pair(a, probes, slot)) cut = list_cut(a, probes[slot], part);
  const int64_t begin = cut.begin, end = cut.end;
  if (end <= begin) {                                    // not a live pair, or a part behind the last row
    empty_entries(a, out, k, tid, kThreads);
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
  StepFlags<unsigned char> flags = {reinterpret_cast<unsigned char*>(meta + 3), 1, 0};      // three bytes of one word
  const int steps = (int)((end - begin + kStepRows - 1) / kStepRows);
  const int mine = (r & 3) + 8 * ((r & 15) >> 2) + 4 * h;       // the tile row whose score this lane takes (r < 16)

  for (int s = 0; s < steps; ++s) {
    flags.open(tid);
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
          flags.raise();                                 // the next step could overflow the buffer
      }
    }
    if (flags.close()) {
      if (wave == 0) prune_to_k<kMaxCap / 64>(buf, k, lane);
      __syncthreads();
    }
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

int resolve(int B, int N, int E, int L, int nprobe, int k, int* parts) {
  return resolve_lists(kFn, B, N, E, L, nprobe, k, parts, " (a grid dimension)");
}

// [B][nprobe * parts][k] keys and rows
int64_t workspace_need(int B, int nprobe, int k, int parts) { return (int64_t)(B > 0 ? B : 1) * nprobe * parts * k * 8; }

}  // namespace

extern "C" int64_t tfimm_hip_embed_search_lists_workspace(int B, int N, int E, int L, int nprobe, int k, int parts) {
  TFIMM_EMBED_TRY(resolve(B, N, E, L, nprobe, k, &parts));
  return workspace_need(B, nprobe, k, parts);
}

extern "C" int tfimm_hip_embed_search_lists(const float* q, int64_t ld_q, int B, const void* g, int64_t ld_g, int N, int E,
                                            const int32_t* ids, const int32_t* offsets, int L, const int32_t* probes, int64_t ld_p,
                                            int nprobe, int k, int parts, float* scores, int32_t* indices, void* workspace,
                                            int64_t workspace_bytes, void* stream) {
  TFIMM_EMBED_TRY(check_lists_pointers(kFn, q, g, ids, offsets, probes, scores, indices, workspace));
  TFIMM_EMBED_TRY(resolve(B, N, E, L, nprobe, k, &parts));
  TFIMM_EMBED_TRY(check_ld_q(kFn, ld_q, E));
  TFIMM_EMBED_TRY(check_ld_g(kFn, ld_g, E));
  TFIMM_EMBED_TRY(check_ld_p(kFn, ld_p, nprobe));
  TFIMM_EMBED_TRY(check_workspace(kFn, workspace_bytes, workspace_need(B, nprobe, k, parts)));
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

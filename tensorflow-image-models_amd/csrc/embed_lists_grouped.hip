// tfimm_hip_embed_search_lists_grouped (include/tfimm_hip.h): tfimm_hip_embed_search_lists with every probed list
// scored ONCE for up to 32 of the queries that name it.  Same arguments, same rule (tests/index_ref.py), same bits: the first pass
// leaves, at the address the single-query kernel would write, the same SET of k pairs for every (query, probe slot, part) -- the
// cuts of a list are the same, a score is a function of its query and its row alone (embed_score.h), and a buffer's content after
// a prune is a function of what it has seen (embed_buffer.h) -- and the second pass is the same select_pass2.  Only the work per
// byte read changes: embed_lists_pass1 fills all 32 columns of the MFMA's B operand with one query, this kernel with 32.
//
//   A PAIR is (query b, probe slot s), p = b * nprobe + s, P = B * nprobe of them.  It is LIVE by the rule of embed_lists.h, which
//   also holds the cut of a list into parts and the empty entries: one text for both searches over lists.
//
//   Grouping, four small launches over tables in the workspace:
//     grouped_fill   count[0 : L] = 0, and every query's k outputs "none" (-1, -inf): pass 2 writes the survivors only.
//     grouped_rank   one thread per pair: rank[p] = atomicAdd(count + l, 1) for a live pair, -1 otherwise.
//     grouped_scan   one workgroup: first[l] = the tiles of the lists before l, a list having ceil(count[l] / 32); first[L], the
//                    total.
//     grouped_place  32 threads per pair: a live pair is member rank % 32 of tile first[l] + rank / 32 (the member of lane 0 also
//                    writes the tile's list); any other pair writes its k * parts workspace entries as empty (key 0, row INT_MAX).
//   Lane j of a tile is occupied exactly when (tile - first[l]) * 32 + j < count[l], so `members` is never filled.  The ranks
//   come from integer atomics and differ from run to run; they decide which tile and lane a query sits in and nothing else.
//
//   Pass 1, grid (T_max, parts), 256 threads: the number of tiles is on the device only, so the launch takes the bound
//   T_max = min(P / 32 + min(L, P), min(L, P) * ceil(B / 32)) -- a list counts once per query and the counts sum to at most P --
//   and a workgroup whose tile is not below first[L] returns at once.  A workgroup owns one (tile, part): it gathers its up to
//   32 queries through `members` into the query tile of embed_score.h (an unoccupied lane: zeros, and it never appends), takes
//   cut `part` of the tile's list, and runs buffered_steps of embed_buffer.h over those positions with score_tile as the score
//   of a step: one buffer per query keyed by (score key, POSITION), cap = choose_cap(...).  Then emit_pairs: each occupied
//   lane's k pairs go to workspace[b][s * parts + part][k], ids[pos] in place of the position; a workgroup whose cut is empty writes k empty entries
//   for each member.  Every (query, slot, part) is written by exactly one workgroup or by grouped_place, in every call.
//   LDS is 32 (2 E + 16) + 32 * 8 * cap bytes, as in embed_wide.hip: hence k <= tfimm_hip_embed_search_wide_max_k(E).
//
//   Pass 2, one workgroup per query: select_pass2 of embed_buffer.h over the nprobe * parts * k pairs, unchanged.
#include "embed_lists.h"

namespace {

using namespace embed_lists;

constexpr const char* kFn = "embed_search_lists_grouped";
constexpr int kPlaceThreads = 32;                         // threads per pair of grouped_place

struct GroupArgs : ListsArgs {
  int32_t* count;            // [L]         live pairs per list
  int32_t* first;            // [L + 1]     first tile per list; [L]: the number of tiles
  int32_t* rank;             // [P]         of a live pair among those of its list, -1: not live
  int32_t* tile_list;        // [T_max]
  int32_t* members;          // [T_max][32] pair numbers
  int B, P, tmax;
};

__global__ void __launch_bounds__(kThreads) grouped_fill(GroupArgs a) {
  const int64_t step = (int64_t)gridDim.x * kThreads, outs = (int64_t)a.B * a.k;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < outs; i += step) {
    a.scores[i] = 0xff800000u;                           // -inf
    a.indices[i] = -1;
  }
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.L; i += step) a.count[i] = 0;
}

__global__ void __launch_bounds__(kThreads) grouped_rank(GroupArgs a) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= a.P) return;
  const int b = p / a.nprobe, s = p - b * a.nprobe;
  const int32_t* probes = a.probes + (int64_t)b * a.ld_p;
  a.rank[p] = live_pair(a, probes, s) ? atomicAdd(a.count + probes[s], 1) : -1;
}

// one workgroup: the exclusive scan of ceil(count / 32) over the lists, thread t taking a run of ceil(L / 256) lists
__global__ void __launch_bounds__(kThreads) grouped_scan(GroupArgs a) {
  __shared__ int sum[kThreads];
  const int tid = threadIdx.x;
  const int run = (a.L + kThreads - 1) / kThreads;
  const int lo = min(tid * run, a.L), hi = min(lo + run, a.L);
  int mine = 0;
  for (int l = lo; l < hi; ++l) mine += (a.count[l] + kQTile - 1) / kQTile;
  sum[tid] = mine;
  __syncthreads();
  for (int o = 1; o < kThreads; o <<= 1) {
    const int v = tid >= o ? sum[tid - o] : 0;
    __syncthreads();
    sum[tid] += v;
    __syncthreads();
  }
  int at = sum[tid] - mine;
  for (int l = lo; l < hi; ++l) {
    a.first[l] = at;
    at += (a.count[l] + kQTile - 1) / kQTile;
  }
  if (tid == kThreads - 1) a.first[a.L] = sum[tid];
}

__global__ void __launch_bounds__(kThreads) grouped_place(GroupArgs a) {
  const int p = blockIdx.x * (kThreads / kPlaceThreads) + threadIdx.x / kPlaceThreads;
  const int t = threadIdx.x % kPlaceThreads;
  if (p >= a.P) return;
  const int rank = a.rank[p];
  if (rank >= 0) {
    if (t == 0) {
      const int b = p / a.nprobe;
      const int l = a.probes[(int64_t)b * a.ld_p + (p - b * a.nprobe)];
      const int tile = a.first[l] + rank / kQTile;
      if (tile >= 0 && tile < a.tmax) {                  // (always: the test keeps a broken invariant inside the tables)
        a.members[(int64_t)tile * kQTile + rank % kQTile] = p;
        if (rank % kQTile == 0) a.tile_list[tile] = l;
      }
    }
    return;
  }
  empty_entries(a, (int64_t)p * a.parts * a.k, a.parts * a.k, t, kPlaceThreads);
}

__global__ void __launch_bounds__(kThreads) embed_lists_grouped_pass1(GroupArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
  const int E = a.E, k = a.k;
  const int tile = blockIdx.x, part = blockIdx.y;
  if (tile >= a.first[a.L]) return;                      // the grid is the bound T_max
  const int l = a.tile_list[tile];
  if (l < 0 || l >= a.L) return;                         // (never: the test keeps a broken invariant from reading)
  const int occ = max(0, min(kQTile, a.count[l] - (tile - a.first[l]) * kQTile));      // lanes 0 .. occ - 1 hold a query
  const int32_t* members = a.members + (int64_t)tile * kQTile;
  // where member qi's pairs of this part go; a pair number outside the table (never) writes nothing
  const auto out = [&](int qi) {
    const int p = members[qi];
    return p < 0 || p >= a.P ? (int64_t)-1 : ((int64_t)p * a.parts + part) * k;
  };

  // ---- this workgroup's rows: positions [begin, end) of the list order; the same in every thread
  const Cut cut = list_cut(a, l, part);
  if (cut.end <= cut.begin) {                            // a part behind the list's last row: k empty entries per member
    for (int qi = wave; qi < occ; qi += kWaves)
      if (out(qi) >= 0) empty_entries(a, out(qi), k, lane, 64);
    return;
  }

  // ---- the query tile, gathered: a wave takes a row at a time (its query is a scalar), the lanes two values each
  const BufferTile t(smem, query_pitch(E), 2 * E, a.cap);
  for (int qi = wave; qi < kQTile; qi += kWaves) {
    const int p = qi < occ ? members[qi] : -1;
    const float* src = p >= 0 && p < a.P ? a.q + (int64_t)(p / a.nprobe) * a.ld_q : nullptr;
    uint32_t* dst = reinterpret_cast<uint32_t*>(smem + (size_t)qi * t.pitch);
    for (int i = lane; i < E / 2; i += 64)
      dst[i] = src ? bf16_rne(__float_as_uint(src[2 * i])) | (bf16_rne(__float_as_uint(src[2 * i + 1])) << 16) : 0u;
  }
  t.clear(tid);
  __syncthreads();

  const int r = lane & 31, h = lane >> 5;
  const int groups = E / 64, tail = (E % 64) / 16;
  const unsigned char* qrow = smem + (size_t)r * t.pitch;
  buffered_steps(t, cut.begin, cut.end, occ, k, [&](int64_t base) {
    // a tile row past the cut reads row min(.., N - 1) instead (its scores are never looked at)
    const int64_t grow = min(base + r, (int64_t)a.N - 1);
    return score_tile(a.g + grow * a.ld_g, qrow, h, groups, tail);
  });
  emit_pairs(t, occ, k, a.ws_key, a.ws_idx, out, a.ids, a.N);      // the original row in place of the position
}

__global__ void __launch_bounds__(kThreads) embed_lists_grouped_pass2(SelectArgs a) { select_pass2(a); }

// the bound on the tiles of a call: a list counts once per query, and the counts sum to at most P
int64_t tiles_bound(int B, int L, int nprobe) {
  const int64_t P = (int64_t)B * nprobe, lists = L < P ? L : P;
  const int64_t by_pairs = P / kQTile + lists, by_lists = lists * ((B + kQTile - 1) / kQTile);
  return by_pairs < by_lists ? by_pairs : by_lists;
}

// the shape of a call as embed_search_lists takes it, and the buffers of a query tile in LDS
int resolve(int B, int N, int E, int L, int nprobe, int k, int* parts) {
  TFIMM_EMBED_TRY(resolve_lists(kFn, B, N, E, L, nprobe, k, parts, ""));
  return check_tile_fit(kFn, E, k);
}

// the pair arrays of tfimm_hip_embed_search_lists, then count [L], first [L + 1], rank [P], tile_list [T], members [T][32]
int64_t workspace_need(int B, int L, int nprobe, int k, int parts) {
  const int b = B > 0 ? B : 1;
  return (int64_t)b * nprobe * parts * k * 8 + 4 * ((int64_t)L + (L + 1) + (int64_t)b * nprobe + (1 + kQTile) * tiles_bound(b, L, nprobe));
}

}  // namespace

extern "C" int64_t tfimm_hip_embed_search_lists_grouped_tiles(int B, int L, int nprobe) {
  if (B < 0 || B > kMaxB) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped_tiles: B=%d, must be in [0, %d]", B, kMaxB);
  if (L < 1 || L > TFIMM_CLUSTER_MAX_C)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped_tiles: L=%d, must be in [1, TFIMM_CLUSTER_MAX_C = %d]", L, TFIMM_CLUSTER_MAX_C);
  if (nprobe < 1 || nprobe > TFIMM_EMBED_LISTS_MAX_PROBE)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped_tiles: nprobe=%d, must be in [1, TFIMM_EMBED_LISTS_MAX_PROBE = %d]", nprobe,
               TFIMM_EMBED_LISTS_MAX_PROBE);
  return tiles_bound(B, L, nprobe);
}

extern "C" int64_t tfimm_hip_embed_search_lists_grouped_workspace(int B, int N, int E, int L, int nprobe, int k, int parts) {
  TFIMM_EMBED_TRY(resolve(B, N, E, L, nprobe, k, &parts));
  return workspace_need(B, L, nprobe, k, parts);
}

extern "C" int tfimm_hip_embed_search_lists_grouped(const float* q, int64_t ld_q, int B, const void* g, int64_t ld_g, int N, int E,
                                                    const int32_t* ids, const int32_t* offsets, int L, const int32_t* probes,
                                                    int64_t ld_p, int nprobe, int k, int parts, float* scores, int32_t* indices,
                                                    void* workspace, int64_t workspace_bytes, void* stream) {
  TFIMM_EMBED_TRY(check_lists_pointers(kFn, q, g, ids, offsets, probes, scores, indices, workspace));
  TFIMM_EMBED_TRY(resolve(B, N, E, L, nprobe, k, &parts));
  TFIMM_EMBED_TRY(check_ld_q(kFn, ld_q, E));
  TFIMM_EMBED_TRY(check_ld_g(kFn, ld_g, E));
  TFIMM_EMBED_TRY(check_ld_p(kFn, ld_p, nprobe));
  TFIMM_EMBED_TRY(check_workspace(kFn, workspace_bytes, workspace_need(B, L, nprobe, k, parts)));
  if (B == 0) return 0;

  static tfimm_once_t ready;
  if (ready.need()) {
    TFIMM_HIP_CHECK(hipFuncSetAttribute((const void*)embed_lists_grouped_pass1, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
    ready.mark();
  }
  const int64_t pairs = (int64_t)nprobe * parts * k;      // per query
  const int64_t tmax = tiles_bound(B, L, nprobe);         // >= 1
  GroupArgs a;
  a.q = q;
  a.g = reinterpret_cast<const uint16_t*>(g);
  a.ids = ids;
  a.offsets = offsets;
  a.probes = probes;
  a.ws_key = reinterpret_cast<uint32_t*>(workspace);
  a.ws_idx = reinterpret_cast<int32_t*>(a.ws_key + (int64_t)B * pairs);
  a.count = a.ws_idx + (int64_t)B * pairs;
  a.first = a.count + L;
  a.rank = a.first + L + 1;
  a.tile_list = a.rank + (int64_t)B * nprobe;
  a.members = a.tile_list + tmax;
  a.scores = reinterpret_cast<uint32_t*>(scores);
  a.indices = indices;
  a.ld_q = ld_q;
  a.ld_g = ld_g;
  a.ld_p = ld_p;
  a.B = B;
  a.N = N;
  a.E = E;
  a.L = L;
  a.nprobe = nprobe;
  a.k = k;
  a.parts = parts;
  a.cap = choose_cap(kQTile * query_pitch(E), k);
  a.P = B * nprobe;
  a.tmax = (int)tmax;
  hipStream_t st = (hipStream_t)stream;
  const int64_t fill = cdiv64((int64_t)B * k > L ? (int64_t)B * k : L, kThreads);
  TFIMM_LAUNCH(grouped_fill, dim3((unsigned)(fill < 4096 ? fill : 4096)), dim3(kThreads), 0, st, a);
  TFIMM_LAUNCH(grouped_rank, dim3((unsigned)cdiv64(a.P, kThreads)), dim3(kThreads), 0, st, a);
  TFIMM_LAUNCH(grouped_scan, dim3(1), dim3(kThreads), 0, st, a);
  TFIMM_LAUNCH(grouped_place, dim3((unsigned)cdiv64(a.P, kThreads / kPlaceThreads)), dim3(kThreads), 0, st, a);
  TFIMM_LAUNCH(embed_lists_grouped_pass1, dim3((unsigned)tmax, (unsigned)parts), dim3(kThreads),
               (size_t)(kQTile * query_pitch(E) + kQTile * 8 * a.cap), st, a);
  SelectArgs s;
  s.ws_key = a.ws_key;
  s.ws_idx = a.ws_idx;
  s.scores = a.scores;
  s.indices = indices;
  s.cand = pairs;
  s.k = k;
  TFIMM_LAUNCH(embed_lists_grouped_pass2, dim3((unsigned)B), dim3(kThreads), 0, st, s);
  return 0;
}

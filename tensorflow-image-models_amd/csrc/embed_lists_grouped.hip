// tfimm_hip_embed_search_lists_grouped (include/tfimm_hip.h): tfimm_hip_embed_search_lists with every probed list
// scored ONCE for up to 32 of the queries that name it.  Same arguments, same rule (tests/index_ref.py), same bits: the first pass
// leaves, at the address the single-query kernel would write, the same SET of k pairs for every (query, probe slot, part) -- the
// cuts of a list are the same, a score is a function of its query and its row alone (embed_score.h), and a buffer's content after
// a prune is a function of what it has seen (embed_buffer.h) -- and the second pass is the same select_pass2.  Only the work per
// byte read changes: embed_lists_pass1 fills all 32 columns of the MFMA's B operand with one query, this kernel with 32.
//
//   A PAIR is (query b, probe slot s), p = b * nprobe + s, P = B * nprobe of them.  It is LIVE when its list l = probes[b][s] is in
//   [0, L), no earlier slot of the query names l, and the list is not empty (offsets clamped to [0, N]).
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
//   cut `part` of the tile's list by embed_lists_pass1's formula, and runs embed_wide_pass1's step loop over those rows: four
//   waves, one score_tile per wave and step with the query on the lane, one buffer per query keyed by (score key, POSITION),
//   the three rotating flags, prune_to_k by the waves in turn, cap = choose_cap(...).  Then each occupied lane's k pairs go to
//   workspace[b][s * parts + part][k], ids[pos] in place of the position; a workgroup whose cut is empty writes k empty entries
//   for each member.  Every (query, slot, part) is written by exactly one workgroup or by grouped_place, in every call.
//   LDS is 32 (2 E + 16) + 32 * 8 * cap bytes, as in embed_wide.hip: hence k <= tfimm_hip_embed_search_wide_max_k(E).
//
//   Pass 2, one workgroup per query: select_pass2 of embed_buffer.h over the nprobe * parts * k pairs, unchanged.
#include "embed_buffer.h"

namespace {

using namespace embed_buffer;

constexpr int kMaxParts = 64;
constexpr int kMaxB = 65535;
constexpr int kPlaceThreads = 32;                         // threads per pair of grouped_place
static_assert((int64_t)kMaxB * TFIMM_EMBED_LISTS_MAX_PROBE < (1ll << 31), "a pair number is an int");

struct GroupArgs {
  const float* q;
  const uint16_t* g;         // rows in list order
  const int32_t* ids;        // [N]
  const int32_t* offsets;    // [L + 1]
  const int32_t* probes;     // [B][ld_p]
  uint32_t* ws_key;          // [B][nprobe * parts][k]
  int32_t* ws_idx;           // [B][nprobe * parts][k]
  int32_t* count;            // [L]         live pairs per list
  int32_t* first;            // [L + 1]     first tile per list; [L]: the number of tiles
  int32_t* rank;             // [P]         of a live pair among those of its list, -1: not live
  int32_t* tile_list;        // [T_max]
  int32_t* members;          // [T_max][32] pair numbers
  uint32_t* scores;          // float32 bits [B][k]
  int32_t* indices;          // [B][k]
  int64_t ld_q, ld_g, ld_p;
  int B, N, E, L, nprobe, k, parts, cap, P, tmax;
};

__device__ __forceinline__ int clamp_pos(int v, int N) { return v < 0 ? 0 : (v > N ? N : v); }

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
  const int32_t* mine = a.probes + (int64_t)b * a.ld_p;
  const int l = mine[s];
  bool live = l >= 0 && l < a.L;
  for (int e = 0; e < s && live; ++e) live = mine[e] != l;                 // a repeated list counts once
  if (live) live = clamp_pos(a.offsets[l + 1], a.N) > clamp_pos(a.offsets[l], a.N);
  a.rank[p] = live ? atomicAdd(a.count + l, 1) : -1;
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
  const int64_t out = (int64_t)p * a.parts * a.k;
  for (int j = t; j < a.parts * a.k; j += kPlaceThreads) {
    a.ws_key[out + j] = kRetired;
    a.ws_idx[out + j] = INT_MAX;
  }
}

// the four words behind query row qi of the tile: count, threshold key, threshold row, and (rows 0 .. 2) a step's flag
__device__ __forceinline__ int* tile_meta(unsigned char* smem, int pitch, int E, int qi) {
  return reinterpret_cast<int*>(smem + (size_t)qi * pitch + 2 * E);
}

__global__ void __launch_bounds__(kThreads) embed_lists_grouped_pass1(GroupArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E = a.E, k = a.k, cap = a.cap;
  const int tile = blockIdx.x, part = blockIdx.y;
  if (tile >= a.first[a.L]) return;                      // the grid is the bound T_max
  const int l = a.tile_list[tile];
  if (l < 0 || l >= a.L) return;                         // (never: the test keeps a broken invariant from reading)
  const int occ = max(0, min(kQTile, a.count[l] - (tile - a.first[l]) * kQTile));      // lanes 0 .. occ - 1 hold a query
  const int32_t* members = a.members + (int64_t)tile * kQTile;

  // ---- this workgroup's rows: positions [begin, end) of the list order, embed_lists_pass1's cut; the same in every thread
  const int lo = clamp_pos(a.offsets[l], a.N), hi = clamp_pos(a.offsets[l + 1], a.N);
  int64_t begin = 0, end = 0;
  if (hi > lo) {
    const int64_t per = ((int64_t)(hi - lo) + a.parts - 1) / a.parts;
    begin = min((int64_t)lo + part * per, (int64_t)hi);
    end = min(begin + per, (int64_t)hi);
  }
  if (end <= begin) {                                    // a part behind the list's last row: k empty entries per member
    for (int qi = wave; qi < occ; qi += kWaves) {
      const int p = members[qi];
      if (p < 0 || p >= a.P) continue;
      const int64_t out = ((int64_t)p * a.parts + part) * k;
      for (int j = lane; j < k; j += 64) {
        a.ws_key[out + j] = kRetired;
        a.ws_idx[out + j] = INT_MAX;
      }
    }
    return;
  }

  // ---- the query tile, gathered: a wave takes a row at a time (its query is a scalar), the lanes two values each
  const int pitch = query_pitch(E);
  uint32_t* buf_key = reinterpret_cast<uint32_t*>(smem + (size_t)kQTile * pitch);   // [32][cap]
  int* buf_idx = reinterpret_cast<int*>(buf_key + kQTile * cap);                   // [32][cap]
  for (int qi = wave; qi < kQTile; qi += kWaves) {
    const int p = qi < occ ? members[qi] : -1;
    const float* src = p >= 0 && p < a.P ? a.q + (int64_t)(p / a.nprobe) * a.ld_q : nullptr;
    uint32_t* dst = reinterpret_cast<uint32_t*>(smem + (size_t)qi * pitch);
    for (int i = lane; i < E / 2; i += 64)
      dst[i] = src ? bf16_rne(__float_as_uint(src[2 * i])) | (bf16_rne(__float_as_uint(src[2 * i + 1])) << 16) : 0u;
  }
  if (tid < kQTile) {
    int* m = tile_meta(smem, pitch, E, tid);
    m[0] = 0;
    m[1] = (int)kRetired;
    m[2] = INT_MAX;
    m[3] = 0;
  }
  __syncthreads();

  const int r = lane & 31, h = lane >> 5;
  const bool q_valid = r < occ;
  const int groups = E / 64, tail = (E % 64) / 16;
  const unsigned char* qrow = smem + (size_t)r * pitch;
  const Buffer mine = {buf_key + r * cap, buf_idx + r * cap, tile_meta(smem, pitch, E, r), cap, r};
  const int steps = (int)((end - begin + kStepRows - 1) / kStepRows);

  int f = 0;                                             // this step's flag: step mod 3
  for (int s = 0; s < steps; ++s) {
    int* flag = tile_meta(smem, pitch, E, f) + 3;
    const int fn = f == 2 ? 0 : f + 1;
    if (tid == 0) tile_meta(smem, pitch, E, fn)[3] = 0;  // the next step's: last read behind the barrier before last
    const int64_t base = begin + (int64_t)s * kStepRows + wave * kRowTile;
    if (base < end) {
      // a tile row past the cut reads row min(.., N - 1) instead (its scores are never looked at)
      const int64_t grow = min(base + r, (int64_t)a.N - 1);
      const f32x16 acc = score_tile(a.g + grow * a.ld_g, qrow, h, groups, tail);
      // ---- lane (r, h): member r, positions base + (i & 3) + 8 (i >> 2) + 4 h
      if (q_valid) {
        const uint32_t tk = (uint32_t)mine.meta[1];
        const int ti = mine.meta[2];
        int top = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int64_t pos = base + (i & 3) + 8 * (i >> 2) + 4 * h;
          const uint32_t key = key_of(__float_as_uint(acc[i]));
          if (pos < end && beats(key, (int)pos, tk, ti)) top = buffer_append(mine, key, (int)pos);
        }
        if (top > cap - kStepRows) *flag = 1;            // the next step could overflow this buffer
      }
    }
    __syncthreads();
    if (*flag) {                                         // written before the barrier, cleared two steps on: one value for all
      for (int qi = wave; qi < occ; qi += kWaves) {
        const Buffer b = {buf_key + qi * cap, buf_idx + qi * cap, tile_meta(smem, pitch, E, qi), cap, qi};
        prune_to_k<kMaxCap / 64>(b, k, lane);
      }
      __syncthreads();
    }
    f = fn;
  }
  for (int qi = wave; qi < occ; qi += kWaves) {
    const Buffer b = {buf_key + qi * cap, buf_idx + qi * cap, tile_meta(smem, pitch, E, qi), cap, qi};
    prune_to_k<kMaxCap / 64>(b, k, lane);
  }
  __syncthreads();

  // ---- k pairs per member, unsorted, the original row in place of the position; an empty entry: key 0, row INT_MAX
  for (int qi = wave; qi < occ; qi += kWaves) {
    const int p = members[qi];
    if (p < 0 || p >= a.P) continue;
    const Buffer b = {buf_key + qi * cap, buf_idx + qi * cap, tile_meta(smem, pitch, E, qi), cap, qi};
    const int n = min(b.meta[0], k);
    const int64_t out = ((int64_t)p * a.parts + part) * k;
    for (int j = lane; j < k; j += 64) {
      uint32_t key = kRetired;
      int id = INT_MAX;
      if (j < n) {
        const int at = slot_at(b, j);
        const int pos = b.idx[at];
        key = b.key[at];
        id = pos >= 0 && pos < a.N ? a.ids[pos] : INT_MAX;   // (always inside: the test keeps a broken invariant from reading)
      }
      a.ws_key[out + j] = key;
      a.ws_idx[out + j] = id;
    }
  }
}

__global__ void __launch_bounds__(kThreads) embed_lists_grouped_pass2(SelectArgs a) { select_pass2(a); }

// the bound on the tiles of a call: a list counts once per query, and the counts sum to at most P
int64_t tiles_bound(int B, int L, int nprobe) {
  const int64_t P = (int64_t)B * nprobe, lists = L < P ? L : P;
  const int64_t by_pairs = P / kQTile + lists, by_lists = lists * ((B + kQTile - 1) / kQTile);
  return by_pairs < by_lists ? by_pairs : by_lists;
}

// validates the shape of a call and resolves parts = 0; returns 0 or TFIMM_EINVAL with the message set
int resolve(int B, int N, int E, int L, int nprobe, int k, int* parts) {
  if (E < TFIMM_EMBED_MIN_E || E > TFIMM_EMBED_MAX_E || E % 16 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: E=%d, must be a multiple of 16 in [%d, TFIMM_EMBED_MAX_E = %d]", E,
               TFIMM_EMBED_MIN_E, TFIMM_EMBED_MAX_E);
  if (N < 1) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: N=%d, must be in [1, 2^31)", N);
  if (L < 1 || L > TFIMM_CLUSTER_MAX_C)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: L=%d, must be in [1, TFIMM_CLUSTER_MAX_C = %d]", L, TFIMM_CLUSTER_MAX_C);
  if (nprobe < 1 || nprobe > TFIMM_EMBED_LISTS_MAX_PROBE)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: nprobe=%d, must be in [1, TFIMM_EMBED_LISTS_MAX_PROBE = %d]", nprobe,
               TFIMM_EMBED_LISTS_MAX_PROBE);
  if (k < 1 || k > TFIMM_EMBED_WIDE_MAX_K)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: k=%d, must be in [1, TFIMM_EMBED_WIDE_MAX_K = %d]", k, TFIMM_EMBED_WIDE_MAX_K);
  if (*parts < 0 || *parts > kMaxParts)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: parts=%d, must be 0 (the library chooses) or in [1, %d]", *parts, kMaxParts);
  if (*parts == 0) *parts = 1;
  if (B < 0 || B > kMaxB) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: B=%d, must be in [0, %d]", B, kMaxB);
  const int most = tfimm_hip_embed_search_wide_max_k(E);
  if (k > most)
    TFIMM_FAIL(TFIMM_EINVAL,
               "embed_search_lists_grouped: E=%d with k=%d: 32 buffers of k + %d pairs do not fit %d KiB of LDS next to the query "
               "tile; tfimm_hip_embed_search_wide_max_k(%d) = %d",
               E, k, kStepRows, kLdsBudget / 1024, E, most);
  return 0;
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
  const int rc = resolve(B, N, E, L, nprobe, k, &parts);
  if (rc) return rc;
  return workspace_need(B, L, nprobe, k, parts);
}

extern "C" int tfimm_hip_embed_search_lists_grouped(const float* q, int64_t ld_q, int B, const void* g, int64_t ld_g, int N, int E,
                                                    const int32_t* ids, const int32_t* offsets, int L, const int32_t* probes,
                                                    int64_t ld_p, int nprobe, int k, int parts, float* scores, int32_t* indices,
                                                    void* workspace, int64_t workspace_bytes, void* stream) {
  if (!q) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: q is null");
  if (!g) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: g is null");
  if (!ids) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: ids is null");
  if (!offsets) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: offsets is null");
  if (!probes) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: probes is null");
  if (!scores) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: scores is null");
  if (!indices) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: indices is null");
  if (!workspace) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: workspace is null");
  if ((uintptr_t)g & 15) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: g must be 16-byte aligned");
  if (((uintptr_t)q | (uintptr_t)ids | (uintptr_t)offsets | (uintptr_t)probes | (uintptr_t)scores | (uintptr_t)indices |
       (uintptr_t)workspace) & 3)
    TFIMM_FAIL(TFIMM_EINVAL,
               "embed_search_lists_grouped: q, ids, offsets, probes, scores, indices and workspace hold 4-byte elements and must be "
               "4-byte aligned");
  const int rc = resolve(B, N, E, L, nprobe, k, &parts);
  if (rc) return rc;
  if (ld_q < E) TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: ld_q=%lld is smaller than E=%d", (long long)ld_q, E);
  if (ld_g < E || ld_g % 8 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: ld_g=%lld, must be a multiple of 8 elements and at least E=%d", (long long)ld_g,
               E);
  if (ld_p < nprobe)
    TFIMM_FAIL(TFIMM_EINVAL, "embed_search_lists_grouped: ld_p=%lld is smaller than nprobe=%d", (long long)ld_p, nprobe);
  const int64_t need = workspace_need(B, L, nprobe, k, parts);
  if (workspace_bytes < need)
    TFIMM_FAIL(TFIMM_EINVAL,
               "embed_search_lists_grouped: workspace_bytes=%lld, tfimm_hip_embed_search_lists_grouped_workspace asks for %lld",
               (long long)workspace_bytes, (long long)need);
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

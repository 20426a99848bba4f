// The cluster end (include/tfimm_hip.h; the CPU restatement of both rules is tests/cluster_ref.py).
//
// tfimm_hip_cluster_assign: for every row of a bf16 gallery [N][ld_g] the centroid (bf16, [C][ld_c]) with the largest inner
// product and that score, in one launch and without the N x C score matrix: a GEMM with an argmax epilogue.
//
//   One workgroup of 256 threads owns 128 gallery rows, 32 per wave, and walks the centroids in tiles of 128.  Per tile it
//   walks E in chunks of 64 columns: the chunk of both operands goes global -> registers -> LDS (128 rows x 128 bytes each,
//   row pitch 144 bytes: pitch / 16 is odd, so the 16 lanes of a ds_read_b128 group fall on 16 distinct 16-byte bank groups);
//   the next chunk's global loads are issued before the MFMAs of this one.  Columns >= E of the last chunk are zeros in LDS
//   and never read from memory: a product of zeros adds +0.0, which leaves every accumulator as it is.
//   The centroids are the A operand of v_mfma_f32_32x32x16_bf16 and the gallery rows the B operand, so the 32 x 32 float32
//   tile has the gallery row on the lane (column = lane & 31) and 16 centroids in the registers: a wave holds 4 such tiles
//   (128 centroids x its 32 rows), reads 1 B and 4 A fragments per 4 MFMAs, and the running best (score, index) of a row
//   lives in the registers of its two lanes (h = lane >> 5) across all centroid tiles.  k is permuted identically on both
//   operands (lane (r, h) owns columns 32h .. 32h+31 of a chunk: 64 contiguous bytes), as in embed.hip.
//   A lane meets its centroids in ascending order, so "strictly larger replaces" keeps the lowest index among equal scores
//   (-0.0 == +0.0); the two lanes of a row are merged by (score, then lower index) and lane h = 0 writes the row's 8 bytes.
//   A score is a function of its row, its centroid and E alone (the chunk loop and the MFMA steps do not depend on N, C or the
//   tile), and the choice is by a total order: bit-reproducible and independent of N, C, the tiling and the other rows.
//
// tfimm_hip_segment_mean: per segment of a CSR list of gallery rows the float32 mean of the rows, by RUNS of
// TFIMM_SEGMENT_RUN entries counted from the segment's own begin (the rule is in the header).  Two launches:
//   partial sums: one thread per (run slot, 8 columns).  Segment c owns the slots [begin / R + c, ...): for ascending offsets
//     the slot ranges of different segments are disjoint and there are at most M / R + C of them -- the work is split by
//     runs, whatever the segments' lengths, and no prefix sum is needed.  A thread finds its slot's segment by bisection over
//     the offsets (at most 31 clamped reads: garbage cannot leave the arrays), adds the run's valid rows in list order and
//     writes 8 sums to the workspace, plus the run's count of valid entries.
//   combine: one thread per (segment, 4 columns) adds the segment's partial sums in ascending run order, divides by the count
//     (one correctly rounded division) and writes mean and counts; an empty segment gives +0.0 and 0.
// No atomics, no scratch memory, every sum in a fixed order that depends on the segment's own entries alone.
#include <limits.h>

#include "common.h"

// sums are sequences of single float32 additions
#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------------------------------------------------------------
// cluster_assign
// ------------------------------------------------------------------------------------------------------------------------
constexpr int kThreads = 256;
constexpr int kRowTile = 128;                 // gallery rows per workgroup: 32 per wave, the N dimension of the MFMA
constexpr int kCenTile = 128;                 // centroids per LDS tile: 4 MFMA tiles of 32
constexpr int kChunk = 64;                    // columns per staged chunk
constexpr int kPitch = 2 * kChunk + 16;       // bytes per staged row
constexpr int kPieces = kRowTile * (kChunk / 8) / kThreads;   // 16-byte pieces per thread, chunk and operand: 4
static_assert(kRowTile == kCenTile && kPieces == 4, "both operands are staged by the same thread map");

struct AssignArgs {
  const uint16_t* g;
  const uint16_t* c;
  int32_t* assign;
  float* score;
  int64_t ld_g, ld_c;
  int N, C, E;
};

template <bool kMask>
__device__ __forceinline__ void take_best(const f32x16 (&acc)[4], int c0, int h, int C, float& best, int& bidx) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = c0 + t * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
      const float s = acc[t][i];
      if ((!kMask || j < C) && s > best) {
        best = s;
        bidx = j;
      }
    }
  }
}

__global__ void __launch_bounds__(kThreads) cluster_assign_kernel(AssignArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kRowTile * kPitch];
  unsigned char* const lg = smem;                         // [128 gallery rows][kPitch]
  unsigned char* const lc = smem + kRowTile * kPitch;     // [128 centroids][kPitch]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int E = a.E, C = a.C;
  const int64_t row0 = (int64_t)blockIdx.x * kRowTile;
  const int chunks = (E + kChunk - 1) / kChunk;

  // staging: piece j of this thread is row srow + 32 j, columns 8 sc8 .. 8 sc8 + 7 of the chunk.  A row past the gallery (a
  // centroid past C) reads the last one instead: its scores are never looked at
  const int srow = tid >> 3, sc8 = tid & 7;
  const uint16_t* gp[kPieces];
#pragma unroll
  for (int j = 0; j < kPieces; ++j) {
    const int64_t grow = min(row0 + srow + 32 * j, (int64_t)a.N - 1);
    gp[j] = a.g + grow * a.ld_g + sc8 * 8;
  }
  const int st_off = srow * kPitch + sc8 * 16;

  float best = -INFINITY;
  int bidx = INT_MAX;
  const uint4 zero = {0u, 0u, 0u, 0u};

  for (int c0 = 0; c0 < C; c0 += kCenTile) {
    const uint16_t* cp[kPieces];
#pragma unroll
    for (int j = 0; j < kPieces; ++j) {
      const int crow = min(c0 + srow + 32 * j, C - 1);
      cp[j] = a.c + (int64_t)crow * a.ld_c + sc8 * 8;
    }
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

    uint4 rg[kPieces], rc[kPieces];
#pragma unroll
    for (int j = 0; j < kPieces; ++j) rg[j] = rc[j] = zero;
    if (sc8 * 8 < E) {
#pragma unroll
      for (int j = 0; j < kPieces; ++j) {
        rg[j] = *reinterpret_cast<const uint4*>(gp[j]);
        rc[j] = *reinterpret_cast<const uint4*>(cp[j]);
      }
    }
    for (int kc = 0; kc < chunks; ++kc) {
      __syncthreads();      // every wave has read the chunk before
#pragma unroll
      for (int j = 0; j < kPieces; ++j) {
        *reinterpret_cast<uint4*>(lg + st_off + 32 * j * kPitch) = rg[j];
        *reinterpret_cast<uint4*>(lc + st_off + 32 * j * kPitch) = rc[j];
      }
      __syncthreads();
      if (kc + 1 < chunks) {      // the next chunk's loads fly while this one is multiplied
        const int col = (kc + 1) * kChunk;
#pragma unroll
        for (int j = 0; j < kPieces; ++j) rg[j] = rc[j] = zero;
        if (col + sc8 * 8 < E) {
#pragma unroll
          for (int j = 0; j < kPieces; ++j) {
            rg[j] = *reinterpret_cast<const uint4*>(gp[j] + col);
            rc[j] = *reinterpret_cast<const uint4*>(cp[j] + col);
          }
        }
      }
      const uint4* bp = reinterpret_cast<const uint4*>(lg + (wave * 32 + r) * kPitch + h * 64);
      const uint4 b0 = bp[0], b1 = bp[1], b2 = bp[2], b3 = bp[3];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const uint4* ap = reinterpret_cast<const uint4*>(lc + (t * 32 + r) * kPitch + h * 64);
        const uint4 a0 = ap[0], a1 = ap[1], a2 = ap[2], a3 = ap[3];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a0), __builtin_bit_cast(bf16x8, b0), acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a1), __builtin_bit_cast(bf16x8, b1), acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a2), __builtin_bit_cast(bf16x8, b2), acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a3), __builtin_bit_cast(bf16x8, b3), acc[t], 0, 0, 0);
      }
    }
    // ---- lane (r, h): gallery row row0 + 32 wave + r, centroids c0 + 32 t + (i & 3) + 8 (i >> 2) + 4 h, ascending in (t, i)
    if (c0 + kCenTile <= C)
      take_best<false>(acc, c0, h, C, best, bidx);
    else
      take_best<true>(acc, c0, h, C, best, bidx);
  }

  // ---- the two lanes of a row: the larger score, of equal scores the lower centroid
  const float ob = __shfl_xor(best, 32, 64);
  const int oi = __shfl_xor(bidx, 32, 64);
  if (ob > best || (ob == best && oi < bidx)) {
    best = ob;
    bidx = oi;
  }
  const int64_t n = row0 + wave * 32 + r;
  if (h == 0 && n < a.N) {
    a.assign[n] = bidx == INT_MAX ? 0 : bidx;      // (only when no score compares: the rule is for finite inputs)
    a.score[n] = best;
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// segment_mean
// ------------------------------------------------------------------------------------------------------------------------
constexpr int kRun = TFIMM_SEGMENT_RUN;
constexpr int kMaxBlocks = 1 << 20;           // both kernels stride over their items

struct SegArgs {
  const uint16_t* g;
  const int32_t* rows;
  const int32_t* offsets;
  float* mean;
  int32_t* counts;
  float* part;          // workspace: [slots][E] partial sums
  int32_t* pcount;      //            [slots] valid entries per run
  int64_t ld_g, ld_m, slots;
  int N, E, M, C;
};

// segment c as [s, e) inside [0, M]; an end below its begin: empty
__device__ __forceinline__ void seg_bounds(const SegArgs& a, int c, int& s, int& e) {
  s = min(max(a.offsets[c], 0), a.M);
  e = min(max(a.offsets[c + 1], 0), a.M);
  if (e < s) e = s;
}
__device__ __forceinline__ int64_t seg_base(const SegArgs& a, int c) {
  return (int64_t)(min(max(a.offsets[c], 0), a.M) / kRun) + c;
}

__global__ void __launch_bounds__(kThreads) segment_partial_kernel(SegArgs a) {
  const int tps = a.E / 8;                    // threads per slot
  const int64_t items = a.slots * tps;
  for (int64_t it = (int64_t)blockIdx.x * kThreads + threadIdx.x; it < items; it += (int64_t)gridDim.x * kThreads) {
    const int64_t t = it / tps;
    const int cg = (int)(it - t * tps);
    // the last segment whose first slot is not behind t
    int lo = 0, hi = a.C;
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      if (seg_base(a, mid) <= t)
        lo = mid;
      else
        hi = mid;
    }
    int s, e;
    seg_bounds(a, lo, s, e);
    const int64_t run = t - ((int64_t)(s / kRun) + lo);
    if (run < 0 || run * kRun >= (int64_t)(e - s)) continue;      // a slot no run owns
    const int64_t p0 = s + run * kRun;
    const int64_t p1 = min(p0 + kRun, (int64_t)e);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    for (int64_t p = p0; p < p1; p += 8) {
      int idx[8];
      uint4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) idx[u] = p + u < p1 ? a.rows[p + u] : -1;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool ok = idx[u] >= 0 && idx[u] < a.N;      // no gallery row is read for an entry outside [0, N)
        v[u] = uint4{0u, 0u, 0u, 0u};
        if (ok) v[u] = *reinterpret_cast<const uint4*>(a.g + (int64_t)idx[u] * a.ld_g + cg * 8);
        cnt += ok ? 1 : 0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {     // list order; the +0.0 of a skipped entry leaves a sum that began at +0.0 as it is
        float f[8];
        unpack8(v[u], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += f[j];
      }
    }
    float4* out = reinterpret_cast<float4*>(a.part + t * a.E + cg * 8);
    out[0] = float4{acc[0], acc[1], acc[2], acc[3]};
    out[1] = float4{acc[4], acc[5], acc[6], acc[7]};
    if (cg == 0) a.pcount[t] = cnt;
  }
}

__global__ void __launch_bounds__(kThreads) segment_combine_kernel(SegArgs a) {
  const int tps = a.E / 4;                    // threads per segment
  const int64_t items = (int64_t)a.C * tps;
  for (int64_t it = (int64_t)blockIdx.x * kThreads + threadIdx.x; it < items; it += (int64_t)gridDim.x * kThreads) {
    const int c = (int)(it / tps);
    const int cg = (int)(it - (int64_t)c * tps);
    int s, e;
    seg_bounds(a, c, s, e);
    const int64_t runs = ((int64_t)(e - s) + kRun - 1) / kRun;
    const int64_t base = (int64_t)(s / kRun) + c;
    const float4* part = reinterpret_cast<const float4*>(a.part + base * a.E + cg * 4);
    const int64_t step = a.E / 4;             // float4 per slot
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    int64_t run = 0;
    for (; run + 16 <= runs; run += 16) {     // 16 partial sums in flight, added in ascending run order
      float4 v[16];
      int n[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        v[u] = part[(run + u) * step];
        n[u] = a.pcount[base + run + u];
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        sum[0] += v[u].x; sum[1] += v[u].y; sum[2] += v[u].z; sum[3] += v[u].w;
        cnt += n[u];
      }
    }
    for (; run < runs; ++run) {
      const float4 v = part[run * step];
      sum[0] += v.x; sum[1] += v.y; sum[2] += v.z; sum[3] += v.w;
      cnt += a.pcount[base + run];
    }
    float* out = a.mean + (int64_t)c * a.ld_m + cg * 4;
    const float d = (float)cnt;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = cnt > 0 ? __fdiv_rn(sum[j], d) : 0.f;
    if (cg == 0) a.counts[c] = cnt;
  }
}

bool bad_e(int E) { return E < TFIMM_EMBED_MIN_E || E > TFIMM_EMBED_MAX_E || E % 16 != 0; }

int64_t segment_slots(int M, int C) { return (int64_t)(M / kRun) + C; }
int64_t segment_bytes(int M, int C, int E) {
  const int64_t slots = segment_slots(M, C);
  return (slots * E * 4 + slots * 4 + 15) / 16 * 16;
}

// what tfimm_hip_segment_mean and its workspace query refuse alike
int check_segment_shape(const char* who, int M, int C, int E) {
  if (bad_e(E))
    TFIMM_FAIL(TFIMM_EINVAL, "%s: E=%d, must be a multiple of 16 in [%d, TFIMM_EMBED_MAX_E = %d]", who, E, TFIMM_EMBED_MIN_E, TFIMM_EMBED_MAX_E);
  if (C < 1) TFIMM_FAIL(TFIMM_EINVAL, "%s: C=%d, must be in [1, 2^31)", who, C);
  if (M < 0) TFIMM_FAIL(TFIMM_EINVAL, "%s: M=%d, must be in [0, 2^31)", who, M);
  return 0;
}

unsigned blocks_for(int64_t items) {
  const int64_t b = cdiv64(items, kThreads);
  return (unsigned)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

}  // namespace

extern "C" int tfimm_hip_cluster_assign(const void* g, int64_t ld_g, int N, const void* c, int64_t ld_c, int C, int E, int32_t* assign,
                                        float* score, void* stream) {
  if (!g) TFIMM_FAIL(TFIMM_EINVAL, "cluster_assign: g is null");
  if (!c) TFIMM_FAIL(TFIMM_EINVAL, "cluster_assign: c is null");
  if (!assign) TFIMM_FAIL(TFIMM_EINVAL, "cluster_assign: assign is null");
  if (!score) TFIMM_FAIL(TFIMM_EINVAL, "cluster_assign: score is null");
  if (((uintptr_t)g | (uintptr_t)c) & 15) TFIMM_FAIL(TFIMM_EINVAL, "cluster_assign: g and c must be 16-byte aligned");
  if (((uintptr_t)assign | (uintptr_t)score) & 3)
    TFIMM_FAIL(TFIMM_EINVAL, "cluster_assign: assign and score hold 4-byte elements and must be 4-byte aligned");
  if (bad_e(E))
    TFIMM_FAIL(TFIMM_EINVAL, "cluster_assign: E=%d, must be a multiple of 16 in [%d, TFIMM_EMBED_MAX_E = %d]", E, TFIMM_EMBED_MIN_E,
               TFIMM_EMBED_MAX_E);
  if (C < 1 || C > TFIMM_CLUSTER_MAX_C)
    TFIMM_FAIL(TFIMM_EINVAL, "cluster_assign: C=%d, must be in [1, TFIMM_CLUSTER_MAX_C = %d]", C, TFIMM_CLUSTER_MAX_C);
  if (N < 0) TFIMM_FAIL(TFIMM_EINVAL, "cluster_assign: N=%d, must be in [0, 2^31)", N);
  if (ld_g < E || ld_g % 8 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "cluster_assign: ld_g=%lld, must be a multiple of 8 elements and at least E=%d", (long long)ld_g, E);
  if (ld_c < E || ld_c % 8 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "cluster_assign: ld_c=%lld, must be a multiple of 8 elements and at least E=%d", (long long)ld_c, E);
  if (N == 0) return 0;
  AssignArgs a;
  a.g = reinterpret_cast<const uint16_t*>(g);
  a.c = reinterpret_cast<const uint16_t*>(c);
  a.assign = assign;
  a.score = score;
  a.ld_g = ld_g;
  a.ld_c = ld_c;
  a.N = N;
  a.C = C;
  a.E = E;
  TFIMM_LAUNCH(cluster_assign_kernel, dim3((unsigned)cdiv64(N, kRowTile)), dim3(kThreads), 0, (hipStream_t)stream, a);
  return 0;
}

extern "C" int64_t tfimm_hip_segment_mean_workspace(int M, int C, int E) {
  if (int rc = check_segment_shape("segment_mean_workspace", M, C, E)) return rc;
  return segment_bytes(M, C, E);
}

extern "C" int tfimm_hip_segment_mean(const void* g, int64_t ld_g, int N, int E, const int32_t* rows, int M, const int32_t* offsets,
                                      int C, float* mean, int64_t ld_m, int32_t* counts, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
  if (!g) TFIMM_FAIL(TFIMM_EINVAL, "segment_mean: g is null");
  if (!rows && M != 0) TFIMM_FAIL(TFIMM_EINVAL, "segment_mean: rows is null");
  if (!offsets) TFIMM_FAIL(TFIMM_EINVAL, "segment_mean: offsets is null");
  if (!mean) TFIMM_FAIL(TFIMM_EINVAL, "segment_mean: mean is null");
  if (!counts) TFIMM_FAIL(TFIMM_EINVAL, "segment_mean: counts is null");
  if (!workspace) TFIMM_FAIL(TFIMM_EINVAL, "segment_mean: workspace is null");
  if (((uintptr_t)g | (uintptr_t)workspace) & 15) TFIMM_FAIL(TFIMM_EINVAL, "segment_mean: g and workspace must be 16-byte aligned");
  if (((uintptr_t)rows | (uintptr_t)offsets | (uintptr_t)mean | (uintptr_t)counts) & 3)
    TFIMM_FAIL(TFIMM_EINVAL, "segment_mean: rows, offsets, mean and counts hold 4-byte elements and must be 4-byte aligned");
  if (int rc = check_segment_shape("segment_mean", M, C, E)) return rc;
  if (N < 0) TFIMM_FAIL(TFIMM_EINVAL, "segment_mean: N=%d, must be in [0, 2^31)", N);
  if (ld_g < E || ld_g % 8 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "segment_mean: ld_g=%lld, must be a multiple of 8 elements and at least E=%d", (long long)ld_g, E);
  if (ld_m < E) TFIMM_FAIL(TFIMM_EINVAL, "segment_mean: ld_m=%lld is smaller than E=%d", (long long)ld_m, E);
  const int64_t need = segment_bytes(M, C, E);
  if (workspace_bytes < need)
    TFIMM_FAIL(TFIMM_EINVAL, "segment_mean: workspace_bytes=%lld, tfimm_hip_segment_mean_workspace asks for %lld", (long long)workspace_bytes,
               (long long)need);
  SegArgs a;
  a.g = reinterpret_cast<const uint16_t*>(g);
  a.rows = rows;
  a.offsets = offsets;
  a.mean = mean;
  a.counts = counts;
  a.slots = segment_slots(M, C);
  a.part = reinterpret_cast<float*>(workspace);
  a.pcount = reinterpret_cast<int32_t*>(a.part + a.slots * E);
  a.ld_g = ld_g;
  a.ld_m = ld_m;
  a.N = N;
  a.E = E;
  a.M = M;
  a.C = C;
  TFIMM_LAUNCH(segment_partial_kernel, dim3(blocks_for(a.slots * (E / 8))), dim3(kThreads), 0, (hipStream_t)stream, a);
  TFIMM_LAUNCH(segment_combine_kernel, dim3(blocks_for((int64_t)C * (E / 4))), dim3(kThreads), 0, (hipStream_t)stream, a);
  return 0;
}

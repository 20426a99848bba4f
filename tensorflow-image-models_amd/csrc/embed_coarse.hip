// tfimm_hip_embed_quantize_rows / tfimm_hip_embed_search_coarse (include/tfimm_hip.h): a coarse-to-fine gallery
// search.  Every gallery row is still visited, but as one fp8 byte per element; the scan keeps `candidates` rows per query,
// and only those are scored in bf16 -- by the loop of the exact searches (embed_score.h), so a returned score has the bits
// tfimm_hip_embed_search gives for that row, and where the candidates contain the true top k the whole result is bit-equal.
// tests/coarse_ref.py restates the rule on the CPU.
//
//   ROW QUANTISATION.  For a bf16 row g of E values: a = max |g_e|; e = 0 if a == 0, else ceil(log2(a / 448)) clamped to
//   [-126, 126] (the scale 2^-e and the factor 2^e are then normal float32 numbers; a finite bf16 row asks for at most 121, and
//   only rows whose amax is below 2^-118 meet the lower clamp: their codes are smaller than they could be, nothing else);
//   code_e = e4m3fn_rne(g_e * 2^-e) (OCP e4m3fn, the encoder of mx.hip).  The scale is a power of two, so scaling is exact, and
//   |g_e * 2^-e| <= 448: nothing saturates.  One int8 exponent and E code bytes per row.  From the bits of a: with x the
//   exponent field and m the 7 mantissa bits, e = x - 135 + (m > 0x60): 448 = 1.75 * 2^8, and 1.75 is m = 0x60.
//   A NON-FINITE entry becomes the NaN code (0x7f with its sign), its row's exponent is 120 or 121, and its row's key is a NaN,
//   which orders above every number (topk_select.h) as it does in the exact searches: such a row is a candidate of every query
//   (as long as there are no more than `candidates` of them) and is then scored exactly.  Nothing faults or hangs.
//
//   COARSE KEY of (query, row).  The query is rounded to bf16 exactly as load_query_tile does and quantised by the same rule
//   with its own exponent; acc is the float32 MFMA sum of the code products from a zero accumulator
//   (v_mfma_f32_32x32x16_fp8_fp8, same shape, operand map and C/D layout as the bf16 instruction of embed_score.h; lane (r, h)
//   holds 8 contiguous bytes); key = acc * 2^(e_row).  The query's exponent is a positive constant per query and is not applied.
//
//   Pass 1 is the grid and the buffer selection of embed_wide.hip -- BufferTile, buffered_steps and emit_pairs of embed_buffer.h
//   -- with k = candidates; what is its own is the score of a step: the query tile lives in LDS as fp8, row pitch E + 16 bytes,
//   count / threshold / flags in the 16 bytes behind a row; within 64 columns lane (r, h) owns bytes 32h .. 32h+31 of its row:
//   two 16-byte loads for four MFMAs, the same permutation on both operands (the < 64 columns behind the last full group use
//   the plain map, 8 bytes per lane).  The loads of the next 64 columns -- of the next tile behind the last group of this one,
//   across the step's barrier and the selection -- are issued before the MFMAs of the current ones; the registers that hold
//   them live in the kernel and the score callable works on them.  The 16 row exponents of a lane's registers are four
//   aligned 4-byte loads, applied inside the callable: the loop sees final keys.  LDS is 32 (E + 16) + 32 * 8 * cap bytes.
//   Pass 2 is select_pass2: chunks * candidates pairs -> the `candidates` best rows per query.
//   Pass 3, one workgroup per query: the query rounded to bf16 in LDS; its candidates 32 at a time through score_tile, lane r's
//   row pointer being candidate r and every column of the B operand the one query (all lanes read the same LDS row), so the
//   bits are those of the exact searches; then the k best by counting: candidate t goes to the position given by the number
//   of candidates that beat it under (score descending, row ascending).  An empty slot (none can arise: candidates <= N)
//   would hold key 0 and never reach the output.
//
// The result is a function of the keys and scores alone: independent of B, of chunk and of the order in which waves arrive.
#include "embed_buffer.h"

namespace {

using namespace embed_buffer;

constexpr int kExpMin = -126, kExpMax = 126;
static_assert(TFIMM_EMBED_COARSE_MAX_CANDIDATES <= TFIMM_EMBED_WIDE_MAX_K, "select_pass2 and the buffers hold that many");

__host__ __device__ constexpr int code_pitch(int E) { return E + 16; }      // bytes per fp8 query row in LDS

// float32 -> OCP e4m3fn, round to nearest even (mx.hip's mx_e4m3); what is not <= 448 in magnitude -- only a non-finite
// entry, after the row's scale -- becomes the NaN code
__device__ __forceinline__ uint32_t e4m3(float v) {
  const uint32_t sign = (__float_as_uint(v) >> 24) & 0x80u;
  const float a = fabsf(v);
  const uint32_t sub = (uint32_t)rintf(a * 512.f);
  uint32_t au = __float_as_uint(a);
  au += 0x7ffffu + ((au >> 20) & 1u);
  const uint32_t nrm = (au >> 20) - (120u << 3);
  if (!(a <= 448.f)) return sign | 0x7fu;
  return sign | (a < 0.015625f ? sub : nrm);
}

// the exponent of a row from the bf16 bits of its largest magnitude
__device__ __forceinline__ int exp_of(uint32_t abits) {
  if (abits == 0) return 0;
  const int e = (int)(abits >> 7) - 135 + ((abits & 0x7fu) > 0x60u ? 1 : 0);
  return e < kExpMin ? kExpMin : (e > kExpMax ? kExpMax : e);
}
__device__ __forceinline__ float pow2(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }      // e in [-126, 127]

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}

// ---- the quantiser: one wave per row, the row held in registers (E <= 2048: four 16-byte loads per lane) -----------------------
__global__ void __launch_bounds__(kThreads) embed_quantize_rows(const uint16_t* __restrict__ g, int64_t ld_g, int N, int E,
                                                                unsigned char* __restrict__ codes, int64_t ld_c,
                                                                signed char* __restrict__ exps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (row >= N) return;                                  // wave-uniform
  const int nch = E / 8;
  const uint4* src = reinterpret_cast<const uint4*>(g + row * ld_g);
  uint4 v[TFIMM_EMBED_MAX_E / 512];
  uint32_t amax = 0;
#pragma unroll
  for (int j = 0; j < TFIMM_EMBED_MAX_E / 512; ++j) {
    const int c = j * 64 + lane;
    v[j] = make_uint4(0u, 0u, 0u, 0u);
    if (c < nch) v[j] = src[c];
    const uint32_t w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
    for (int i = 0; i < 4; ++i) amax = max(amax, max(w[i] & 0x7fffu, (w[i] >> 16) & 0x7fffu));
  }
  const int e = exp_of(wave_max(amax));
  const float scale = pow2(-e);
#pragma unroll
  for (int j = 0; j < TFIMM_EMBED_MAX_E / 512; ++j) {
    const int c = j * 64 + lane;
    if (c < nch) {
      const uint32_t w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
      uint32_t o[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        o[i] = e4m3(__uint_as_float(w[2 * i] << 16) * scale) | (e4m3(__uint_as_float(w[2 * i] & 0xffff0000u) * scale) << 8) |
               (e4m3(__uint_as_float(w[2 * i + 1] << 16) * scale) << 16) | (e4m3(__uint_as_float(w[2 * i + 1] & 0xffff0000u) * scale) << 24);
      *reinterpret_cast<uint2*>(codes + row * ld_c + 8 * c) = make_uint2(o[0], o[1]);
    }
  }
  if (lane == 0) exps[row] = (signed char)e;
}

// ---- pass 1 ------------------------------------------------------------------------------------------------------------------------
struct CoarseArgs {
  const float* q;
  const unsigned char* codes;
  const signed char* exps;
  uint32_t* ws_key;    // [B][chunks][c]
  int32_t* ws_idx;     // [B][chunks][c]
  int64_t ld_q, ld_c;
  int B, N, E, c, chunk, chunks, cap;
};

// queries q0 .. q0 + 31 -> bf16 -> fp8 codes in smem (queries past B: zeros), a wave per query; the caller places the barrier
__device__ __forceinline__ void load_query_codes(unsigned char* smem, const float* q, int64_t ld_q, int q0, int B, int E, int lane,
                                                 int wave) {
  const int pitch = code_pitch(E);
  for (int qi = wave; qi < kQTile; qi += kWaves) {
    uint32_t* dst = reinterpret_cast<uint32_t*>(smem + (size_t)qi * pitch);
    if (q0 + qi >= B) {
      for (int w = lane; w < E / 4; w += 64) dst[w] = 0u;
      continue;
    }
    const float* src = q + (int64_t)(q0 + qi) * ld_q;
    uint32_t amax = 0;
    for (int c = lane; c < E; c += 64) amax = max(amax, bf16_rne(__float_as_uint(src[c])) & 0x7fffu);
    const float scale = pow2(-exp_of(wave_max(amax)));
    for (int w = lane; w < E / 4; w += 64) {
      uint32_t o = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) o |= e4m3(__uint_as_float(bf16_rne(__float_as_uint(src[4 * w + i])) << 16) * scale) << (8 * i);
      dst[w] = o;
    }
  }
}

__device__ __forceinline__ long lo64(const uint4& v) { return (long)(((uint64_t)v.y << 32) | v.x); }
__device__ __forceinline__ long hi64(const uint4& v) { return (long)(((uint64_t)v.w << 32) | v.z); }

// the fp8 sums of the code row at ca (this lane's row of the tile) and its 31 neighbours against the query tile.  c0 / c1: the
// lane's 32 bytes of the first 64 columns, loaded by the caller (groups > 0); on return those of the row at next (the caller
// passes ca again behind the last tile: one load that nobody uses, and no branch around a load).
__device__ __forceinline__ f32x16 coarse_tile(const unsigned char* ca, const unsigned char* next, const unsigned char* qrow, int h,
                                              int groups, int tail, uint4& c0, uint4& c1) {
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int gi = 0; gi < groups; ++gi) {
    const uint4* np = reinterpret_cast<const uint4*>((gi + 1 < groups ? ca + (gi + 1) * 64 : next) + h * 32);
    const uint4 n0 = np[0], n1 = np[1];
    const uint4* bp = reinterpret_cast<const uint4*>(qrow + gi * 64 + h * 32);
    const uint4 b0 = bp[0], b1 = bp[1];
    acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(lo64(c0), lo64(b0), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(hi64(c0), hi64(b0), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(lo64(c1), lo64(b1), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(hi64(c1), hi64(b1), acc, 0, 0, 0);
    c0 = n0;
    c1 = n1;
  }
  for (int t = 0; t < tail; ++t) {
    const int c = groups * 64 + t * 16 + h * 8;
    const uint2 av = *reinterpret_cast<const uint2*>(ca + c);
    const uint2 bv = *reinterpret_cast<const uint2*>(qrow + c);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8((long)(((uint64_t)av.y << 32) | av.x), (long)(((uint64_t)bv.y << 32) | bv.x), acc,
                                                     0, 0, 0);
  }
  return acc;
}

// A HELD tile (E <= 512: at most G groups of 64 columns): the lane's bytes of all groups of a tile in registers, 2 G uint4, so
// that every load of the NEXT tile is in flight before the first MFMA of the current one.
template <int G>
__device__ __forceinline__ void load_held(uint4 (&t)[2 * G], const unsigned char* ca, int h, int groups) {
#pragma unroll
  for (int gi = 0; gi < G; ++gi)
    if (gi < groups) {
      const uint4* p = reinterpret_cast<const uint4*>(ca + gi * 64 + h * 32);
      t[2 * gi] = p[0];
      t[2 * gi + 1] = p[1];
    }
}

template <int G>
__device__ __forceinline__ f32x16 held_tile(const uint4 (&t)[2 * G], const unsigned char* ca, const unsigned char* qrow, int h, int groups,
                                            int tail) {
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int gi = 0; gi < G; ++gi)
    if (gi < groups) {
      const uint4* bp = reinterpret_cast<const uint4*>(qrow + gi * 64 + h * 32);
      const uint4 b0 = bp[0], b1 = bp[1];
      acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(lo64(t[2 * gi]), lo64(b0), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(hi64(t[2 * gi]), hi64(b0), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(lo64(t[2 * gi + 1]), lo64(b1), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(hi64(t[2 * gi + 1]), hi64(b1), acc, 0, 0, 0);
    }
  for (int u = 0; u < tail; ++u) {
    const int c = groups * 64 + u * 16 + h * 8;
    const uint2 av = *reinterpret_cast<const uint2*>(ca + c);
    const uint2 bv = *reinterpret_cast<const uint2*>(qrow + c);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8((long)(((uint64_t)av.y << 32) | av.x), (long)(((uint64_t)bv.y << 32) | bv.x), acc,
                                                     0, 0, 0);
  }
  return acc;
}

// G = 0: the streaming tile (any E).  G = 2, 4, 8: held tiles of at most G groups.  Waves per SIMD asked of the compiler: what
// LDS allows anyway at that width -- 3 (at most 168 registers), or 2 where two tiles of eight groups are held.
template <int G>
__global__ void __launch_bounds__(kThreads, G == 8 ? 2 : 3) embed_coarse_pass1(CoarseArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
  const int E = a.E, k = a.c;
  const BufferTile t(smem, code_pitch(E), E, a.cap);
  const int q0 = blockIdx.y * kQTile;
  const int occ = min(kQTile, a.B - q0);                // lanes 0 .. occ - 1 hold a query

  load_query_codes(smem, a.q, a.ld_q, q0, a.B, E, lane, wave);
  t.clear(tid);
  __syncthreads();

  const int64_t row_begin = (int64_t)blockIdx.x * a.chunk;
  const int64_t row_end = min(row_begin + (int64_t)a.chunk, (int64_t)a.N);
  const int r = lane & 31, h = lane >> 5;
  const int groups = E / 64, tail = (E % 64) / 16;
  const unsigned char* qrow = smem + (size_t)r * t.pitch;

  // the wave's first tile, loaded ahead of the loop.  A row past the gallery reads the last row instead (its sums are never
  // looked at).
  const int64_t first = row_begin + wave * kRowTile;
  constexpr int kHeld = G > 0 ? 2 * G : 2;
  uint4 cur[kHeld];
#pragma unroll
  for (int i = 0; i < kHeld; ++i) cur[i] = make_uint4(0u, 0u, 0u, 0u);
  if (first < row_end && groups > 0) {
    const unsigned char* ca = a.codes + min(first + r, (int64_t)a.N - 1) * a.ld_c;
    if constexpr (G > 0) {
      load_held<G>(cur, ca, h, groups);
    } else {
      cur[0] = reinterpret_cast<const uint4*>(ca + h * 32)[0];
      cur[1] = reinterpret_cast<const uint4*>(ca + h * 32)[1];
    }
  }

  // the coarse keys of a step: the code sums of the tile in `cur` -- while the loads of the wave's next tile, which outlive the
  // step's barrier and the selection, are in flight -- times 2^(e_row)
  buffered_steps(t, row_begin, row_end, occ, k, [&](int64_t base) {
    const unsigned char* ca = a.codes + min(base + r, (int64_t)a.N - 1) * a.ld_c;
    const int64_t nbase = base + kStepRows;
    const unsigned char* next = nbase < row_end ? a.codes + min(nbase + r, (int64_t)a.N - 1) * a.ld_c : ca;
    // the exponents of rows base + 8 j + 4 h .. + 3: one aligned word each (base is a multiple of 32); bytes past N are not read
    uint32_t ew[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t at = base + 8 * j + 4 * h;
      ew[j] = 0;
      if (at + 3 < a.N) {
        ew[j] = *reinterpret_cast<const uint32_t*>(a.exps + at);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (at + u < a.N) ew[j] |= (uint32_t)(unsigned char)a.exps[at + u] << (8 * u);
      }
    }
    f32x16 acc;
    if constexpr (G > 0) {
      uint4 nxt[kHeld];
#pragma unroll
      for (int i = 0; i < kHeld; ++i) nxt[i] = cur[i];
      if (nbase < row_end) load_held<G>(nxt, next, h, groups);
      acc = held_tile<G>(cur, ca, qrow, h, groups, tail);
#pragma unroll
      for (int i = 0; i < kHeld; ++i) cur[i] = nxt[i];
    } else {
      acc = coarse_tile(ca, next, qrow, h, groups, tail, cur[0], cur[1]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      int e = (int)(signed char)(ew[i >> 2] >> (8 * (i & 3)));
      e = e < kExpMin ? kExpMin : (e > kExpMax ? kExpMax : e);        // whatever the bytes are, a float32 factor
      acc[i] *= pow2(e);
    }
    return acc;
  });
  emit_pairs(t, occ, k, a.ws_key, a.ws_idx, [&](int qi) { return ((int64_t)(q0 + qi) * a.chunks + blockIdx.x) * k; });
}

__global__ void __launch_bounds__(kThreads) embed_coarse_pass2(SelectArgs a) { select_pass2(a); }

// ---- pass 3: the rerank --------------------------------------------------------------------------------------------------------------
struct RerankArgs {
  const float* q;
  const uint16_t* g;
  const int32_t* cand;   // [B][c]
  uint32_t* scores;      // float32 bits [B][k]
  int32_t* indices;      // [B][k]
  int64_t ld_q, ld_g;
  int N, E, c, k;
};

__global__ void __launch_bounds__(kThreads) embed_coarse_rerank(RerankArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];          // the query as bf16: 2 E bytes
  __shared__ uint32_t ck[TFIMM_EMBED_COARSE_MAX_CANDIDATES];
  __shared__ int ci[TFIMM_EMBED_COARSE_MAX_CANDIDATES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int E = a.E, c = a.c;
  const float* src = a.q + (int64_t)blockIdx.x * a.ld_q;
  for (int i = tid; i < E / 2; i += kThreads)
    reinterpret_cast<uint32_t*>(smem)[i] = bf16_rne(__float_as_uint(src[2 * i])) | (bf16_rne(__float_as_uint(src[2 * i + 1])) << 16);
  if (tid < c) {
    const int row = a.cand[(int64_t)blockIdx.x * c + tid];
    ci[tid] = row >= 0 && row < a.N ? row : INT_MAX;     // an empty slot: never scored, never ranked
    ck[tid] = kRetired;
  }
  __syncthreads();

  const int r = lane & 31, h = lane >> 5;
  const int groups = E / 64, tail = (E % 64) / 16;
  for (int t0 = wave * kRowTile; t0 < c; t0 += kWaves * kRowTile) {
    const int row = t0 + r < c ? ci[t0 + r] : INT_MAX;
    const f32x16 acc = score_tile(a.g + (int64_t)(row == INT_MAX ? 0 : row) * a.ld_g, smem, h, groups, tail);
    // every column is the one query: lanes (0, h) write their 16 rows
    if (r == 0) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int t = t0 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (t < c && ci[t] != INT_MAX) ck[t] = key_of(__float_as_uint(acc[i]));
      }
    }
  }
  __syncthreads();

  if (tid < c && ci[tid] != INT_MAX) {
    const uint32_t mk = ck[tid];
    const int mi = ci[tid];
    int pos = 0;
    for (int j = 0; j < c; ++j) pos += beats(ck[j], ci[j], mk, mi) ? 1 : 0;
    if (pos < a.k) {
      const int64_t o = (int64_t)blockIdx.x * a.k + pos;
      a.scores[o] = bits_of(mk);
      a.indices[o] = mi;
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
constexpr const char* kFn = "embed_search_coarse";

// what the LDS next to an fp8 query tile holds: 32 (E + 16) + 32 * 8 * cap <= 160 KiB with cap >= candidates + 128
int max_candidates(int E) { return e_ok(E) ? fit_max_k(kQTile * code_pitch(E), TFIMM_EMBED_COARSE_MAX_CANDIDATES) : 0; }

// validates (B, N, E, k, candidates, chunk) and resolves chunk = 0; returns 0 or TFIMM_EINVAL with the message set
int resolve(int B, int N, int E, int k, int c, int* chunk, int64_t* chunks) {
  TFIMM_EMBED_TRY(check_E(kFn, E));
  TFIMM_EMBED_TRY(check_N(kFn, N));
  if (c < 1 || c > N || c > max_candidates(E))
    TFIMM_FAIL(TFIMM_EINVAL, "%s: candidates=%d, must be in [1, min(N = %d, tfimm_hip_embed_search_coarse_max_candidates(%d) = %d)]", kFn, c,
               N, E, max_candidates(E));
  if (k < 1 || k > c) TFIMM_FAIL(TFIMM_EINVAL, "%s: k=%d, must be in [1, candidates = %d]", kFn, k, c);
  TFIMM_EMBED_TRY(check_chunk(kFn, *chunk));
  TFIMM_EMBED_TRY(check_B(kFn, B));
  // every chunk hands `candidates` pairs to pass 2, which one workgroup per query reads: at least 16 times as many rows
  if (*chunk == 0) *chunk = choose_chunk(B, N, c, 16);
  *chunks = cdiv64(N, *chunk);
  return 0;
}

// [B][chunks][c] keys and rows of pass 1, [B][c] keys and rows of pass 2
int64_t workspace_need(int B, int64_t chunks, int c) { return (int64_t)(B > 0 ? B : 1) * (chunks + 1) * c * 8; }

}  // namespace

extern "C" int tfimm_hip_embed_quantize_rows(const void* g, int64_t ld_g, int N, int E, void* codes, int64_t ld_c, int8_t* exps,
                                             void* stream) {
  constexpr const char* fn = "embed_quantize_rows";
  TFIMM_EMBED_TRY(check_pointers(fn, {{"g", g, 16}, {"codes", codes, 16}, {"exps", exps, 1}}));
  TFIMM_EMBED_TRY(check_E(fn, E));
  if (N < 0) TFIMM_FAIL(TFIMM_EINVAL, "%s: N=%d, must be in [0, 2^31)", fn, N);
  TFIMM_EMBED_TRY(check_ld_g(fn, ld_g, E));
  TFIMM_EMBED_TRY(check_ld_c(fn, ld_c, E));
  if (N == 0) return 0;
  TFIMM_LAUNCH(embed_quantize_rows, dim3((unsigned)cdiv64(N, kWaves)), dim3(kThreads), 0, (hipStream_t)stream,
               reinterpret_cast<const uint16_t*>(g), ld_g, N, E, reinterpret_cast<unsigned char*>(codes), ld_c,
               reinterpret_cast<signed char*>(exps));
  return 0;
}

extern "C" int tfimm_hip_embed_search_coarse_max_candidates(int E) { return max_candidates(E); }

extern "C" int64_t tfimm_hip_embed_search_coarse_workspace(int B, int N, int E, int k, int candidates, int chunk) {
  int64_t chunks = 0;
  TFIMM_EMBED_TRY(resolve(B, N, E, k, candidates, &chunk, &chunks));
  return workspace_need(B, chunks, candidates);
}

extern "C" int tfimm_hip_embed_search_coarse(const float* q, int64_t ld_q, int B, const void* g, int64_t ld_g, const void* codes,
                                             int64_t ld_c, const int8_t* exps, int N, int E, int k, int candidates, int chunk,
                                             float* scores, int32_t* indices, void* workspace, int64_t workspace_bytes, void* stream) {
  TFIMM_EMBED_TRY(check_pointers(kFn,
                                 {{"q", q, 4}, {"g", g, 16}, {"codes", codes, 16}, {"exps", exps, 4}, {"scores", scores, 4},
                                  {"indices", indices, 4}, {"workspace", workspace, 4}},
                                 "must be 4-byte aligned"));
  int64_t chunks = 0;
  TFIMM_EMBED_TRY(resolve(B, N, E, k, candidates, &chunk, &chunks));
  TFIMM_EMBED_TRY(check_ld_q(kFn, ld_q, E));
  TFIMM_EMBED_TRY(check_ld_g(kFn, ld_g, E));
  TFIMM_EMBED_TRY(check_ld_c(kFn, ld_c, E));
  TFIMM_EMBED_TRY(check_workspace(kFn, workspace_bytes, workspace_need(B, chunks, candidates)));
  if (B == 0) return 0;

  static tfimm_once_t ready;
  if (ready.need()) {
    TFIMM_HIP_CHECK(hipFuncSetAttribute((const void*)embed_coarse_pass1<0>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
    TFIMM_HIP_CHECK(hipFuncSetAttribute((const void*)embed_coarse_pass1<2>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
    TFIMM_HIP_CHECK(hipFuncSetAttribute((const void*)embed_coarse_pass1<4>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
    TFIMM_HIP_CHECK(hipFuncSetAttribute((const void*)embed_coarse_pass1<8>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
    ready.mark();
  }
  const int c = candidates;
  CoarseArgs a;
  a.q = q;
  a.codes = reinterpret_cast<const unsigned char*>(codes);
  a.exps = reinterpret_cast<const signed char*>(exps);
  a.ws_key = reinterpret_cast<uint32_t*>(workspace);
  a.ws_idx = reinterpret_cast<int32_t*>(a.ws_key + (int64_t)B * chunks * c);
  a.ld_q = ld_q;
  a.ld_c = ld_c;
  a.B = B;
  a.N = N;
  a.E = E;
  a.c = c;
  a.chunk = chunk;
  a.chunks = (int)chunks;
  const int tile = kQTile * code_pitch(E);
  a.cap = choose_cap(tile, c);
  const int qtiles = (B + kQTile - 1) / kQTile;
  const dim3 grid((unsigned)chunks, (unsigned)qtiles);
  const size_t lds = (size_t)(tile + kQTile * 8 * a.cap);
  const int groups = E / 64;                            // held tiles up to E = 512 + a tail; wider rows and E < 64 stream
  if (groups == 0 || groups > 8) {
    TFIMM_LAUNCH(embed_coarse_pass1<0>, grid, dim3(kThreads), lds, (hipStream_t)stream, a);
  } else if (groups <= 2) {
    TFIMM_LAUNCH(embed_coarse_pass1<2>, grid, dim3(kThreads), lds, (hipStream_t)stream, a);
  } else if (groups <= 4) {
    TFIMM_LAUNCH(embed_coarse_pass1<4>, grid, dim3(kThreads), lds, (hipStream_t)stream, a);
  } else {
    TFIMM_LAUNCH(embed_coarse_pass1<8>, grid, dim3(kThreads), lds, (hipStream_t)stream, a);
  }
  SelectArgs s;
  s.ws_key = a.ws_key;
  s.ws_idx = a.ws_idx;
  s.scores = reinterpret_cast<uint32_t*>(a.ws_idx + (int64_t)B * chunks * c);       // the coarse keys as floats: [B][c], not used again
  s.indices = reinterpret_cast<int32_t*>(s.scores + (int64_t)B * c);               // the candidates: [B][c]
  s.cand = chunks * c;
  s.k = c;
  TFIMM_LAUNCH(embed_coarse_pass2, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, s);
  RerankArgs t;
  t.q = q;
  t.g = reinterpret_cast<const uint16_t*>(g);
  t.cand = s.indices;
  t.scores = reinterpret_cast<uint32_t*>(scores);
  t.indices = indices;
  t.ld_q = ld_q;
  t.ld_g = ld_g;
  t.N = N;
  t.E = E;
  t.c = c;
  t.k = k;
  TFIMM_LAUNCH(embed_coarse_rerank, dim3((unsigned)B), dim3(kThreads), (size_t)(2 * E), (hipStream_t)stream, t);
  return 0;
}

// The score loop shared by the five gallery searches: the query tile rounded to bf16 in LDS, and one 32 x 32 tile of float32
// scores of 32 gallery rows against it.  Its users: the first passes of tfimm_hip_embed_search (embed.hip),
// tfimm_hip_embed_search_wide (embed_wide.hip), tfimm_hip_embed_search_lists (embed_lists.hip, one query in all 32 columns) and
// tfimm_hip_embed_search_lists_grouped (embed_lists_grouped.hip, the tile gathered through its members), and the rerank of
// tfimm_hip_embed_search_coarse (embed_coarse.hip), whose fp8 scan keeps the tile's shape and lane map.
//
// The query tile: 32 rows of E bf16 values, row pitch 2 E + 16 bytes (pitch / 16 is odd, so the 16 lanes of a ds_read_b128
// pass fall on 16 distinct 16-byte bank groups).  The 16 bytes behind a row's values are never read by the score loop.
//
// A tile: the 32 gallery rows are the A operand of v_mfma_f32_32x32x16_bf16 and come straight from global memory: lane (r, h)
// holds A[row r][k = 8h .. 8h+7], 16 contiguous bytes of gallery row r.  k is permuted identically on both operands so that
// within 64 columns lane (r, h) owns columns 32h .. 32h+31: it reads 64 contiguous bytes of its row per four MFMA steps (the
// < 64 columns behind the last full group use the plain map).  The MFMA steps run in ascending column order from a zero
// accumulator, so a score is a function of its query and its gallery row alone -- the same bits from every entry point.  The
// result has the query on the lane (column = lane & 31) and 16 gallery rows in the registers: register i of lane (r, h) is
// gallery row (i & 3) + 8 (i >> 2) + 4 h of the tile.
#pragma once
#include "common.h"

namespace embed_score {

constexpr int kQTile = 32;                      // queries per workgroup: the N dimension of the MFMA
constexpr int kRowTile = 32;                    // gallery rows per MFMA tile
constexpr int kLdsBudget = 160 * 1024;          // gfx950: LDS per workgroup

__host__ __device__ constexpr int query_pitch(int E) { return 2 * E + 16; }   // bytes per query row in LDS

// float32 -> bf16 bits, round to nearest even; a NaN stays a (quiet) NaN
__device__ __forceinline__ uint32_t bf16_rne(uint32_t b) {
  if ((b & 0x7fffffffu) > 0x7f800000u) return (b >> 16) | 0x40u;
  return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
}

// queries q0 .. q0 + 31 -> bf16 in smem (queries past B: zeros); the caller places the __syncthreads()
__device__ __forceinline__ void load_query_tile(unsigned char* smem, const float* q, int64_t ld_q, int q0, int B, int E, int tid,
                                                int threads) {
  const int pitch = query_pitch(E);
  for (int i = tid; i < kQTile * (E / 2); i += threads) {
    const int qi = i / (E / 2), c = (i - qi * (E / 2)) * 2;
    uint32_t lo = 0, hi = 0;
    if (q0 + qi < B) {
      const float* src = q + (int64_t)(q0 + qi) * ld_q + c;
      lo = bf16_rne(__float_as_uint(src[0]));
      hi = bf16_rne(__float_as_uint(src[1]));
    }
    *reinterpret_cast<uint32_t*>(smem + (size_t)qi * pitch + 2 * c) = lo | (hi << 16);
  }
}

// the scores of the gallery row at ga (this lane's row of the tile) and its 31 neighbours against the query tile: qrow is the
// LDS row of query lane & 31, h = lane >> 5, groups = E / 64, tail = (E % 64) / 16
__device__ __forceinline__ f32x16 score_tile(const uint16_t* ga, const unsigned char* qrow, int h, int groups, int tail) {
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int gi = 0; gi < groups; ++gi) {
    const uint4* ap = reinterpret_cast<const uint4*>(ga + gi * 64 + h * 32);
    const uint4* bp = reinterpret_cast<const uint4*>(qrow + 2 * (gi * 64 + h * 32));
    const uint4 a0 = ap[0], a1 = ap[1], a2 = ap[2], a3 = ap[3];
    const uint4 b0 = bp[0], b1 = bp[1], b2 = bp[2], b3 = bp[3];
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a0), __builtin_bit_cast(bf16x8, b0), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a1), __builtin_bit_cast(bf16x8, b1), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a2), __builtin_bit_cast(bf16x8, b2), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a3), __builtin_bit_cast(bf16x8, b3), acc, 0, 0, 0);
  }
  for (int t = 0; t < tail; ++t) {
    const int c = groups * 64 + t * 16 + h * 8;
    const uint4 av = *reinterpret_cast<const uint4*>(ga + c);
    const uint4 bv = *reinterpret_cast<const uint4*>(qrow + 2 * c);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), acc, 0, 0, 0);
  }
  return acc;
}

}  // namespace embed_score

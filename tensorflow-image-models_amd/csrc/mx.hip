// MXFP8 (OCP microscaling, e4m3fn elements in blocks of 32 with one E8M0 scale) for the Dense layers of the transformer
// families: the fp8 precision mode of tfimm/engine/precision.py.
//
//   tfimm_hip_quantize_mx  bf16 rows -> MXFP8 rows, optionally through a LayerNormalization first (one pass instead of
//                          row_stats + the LN fold of the bf16 path).  One wave per row, 8 elements per lane per 512-element
//                          piece, the 32-element block's amax over 4 neighbouring lanes.
//   tfimm_hip_gemm_mx      out = epilogue( deq(A) . deq(W)^T ) on v_mfma_scale_f32_32x32x64_f8f6f4: 256 x 256 x 128 tiles,
//                          8 waves of 128 x 64, both operands and both scale arrays global -> LDS by LDS-DMA (one load kind
//                          in the k-loop, so nothing drains the pipeline early), 2-stage ring, one barrier per K-tile -- the
//                          loop of csrc/gemm_dma_kernel.h.  Epilogue in registers (bias, act, bf16 residual, act after the
//                          residual as tfimm_hip_gemm), stored as bf16, fp32 or MXFP8 (the 32-column block of a row lies in
//                          one lane pair: lane l and l ^ 32 hold its 2 x 16 values).
//
// Scale rule (tfimm/engine/pack.py mx_quantize, the host reference every test shares): the block scale is the smallest power
// of two s = 2^k with amax / s <= 448 (k >= -127; an all-zero block gets 2^-127, E8M0 byte 0), the elements are x / s rounded
// to nearest-even in e4m3fn.  |x / s| <= 448 by construction, so nothing saturates; a zero result keeps the sign of x.
#include "common.h"

#include <algorithm>

namespace {

typedef __attribute__((address_space(3))) void* mx_lds_ptr_t;
typedef __attribute__((ext_vector_type(8))) int i32x8;

// k of the block scale 2^k: amax = 1.m * 2^e  ->  k = e - 8, one more when 1.m > 1.75 (448 = 1.75 * 2^8); clamped to the
// smallest E8M0 value (zero and tiny blocks)
__device__ __forceinline__ int mx_scale_exp(float amax) {
  const uint32_t u = __float_as_uint(amax);
  const int k = (int)(u >> 23) - 135 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
  return k < -127 ? -127 : k;
}
// 2^-k as a float (-k in [-120, 127]: a normal number)
__device__ __forceinline__ float mx_inv_scale(int k) { return __uint_as_float((uint32_t)(127 - k) << 23); }

// fp32 (|v| <= 448) -> e4m3fn, round to nearest even; subnormals (steps of 2^-9) by rint of the scaled magnitude, whose codes
// continue into the normal range (8 = 2^-6), normals by rounding the fp32 mantissa to 3 bits and re-biasing the exponent
__device__ __forceinline__ uint32_t mx_e4m3(float v) {
  const uint32_t sign = (__float_as_uint(v) >> 24) & 0x80u;
  const float a = fabsf(v);
  const uint32_t sub = (uint32_t)rintf(a * 512.f);
  uint32_t au = __float_as_uint(a);
  au += 0x7ffffu + ((au >> 20) & 1u);
  const uint32_t nrm = (au >> 20) - (120u << 3);
  return sign | (a < 0.015625f ? sub : nrm);
}
__device__ __forceinline__ uint32_t mx_pack4(const float* v, float inv) {
  return mx_e4m3(v[0] * inv) | (mx_e4m3(v[1] * inv) << 8) | (mx_e4m3(v[2] * inv) << 16) | (mx_e4m3(v[3] * inv) << 24);
}

// ---- quantize ------------------------------------------------------------------------------------------------------------
template <int NCH, bool LN>
__global__ void __launch_bounds__(256) quantize_mx_kernel(const bf16_t* __restrict__ x, int64_t rows, int C, int64_t xs,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float eps, uint8_t* __restrict__ q, uint8_t* __restrict__ qs,
                                                         int ldq) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;   // wave-uniform
  const int nchunks = C >> 3;
  float v[NCH][8];
  const bf16_t* xr = x + r * xs;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + 64 * i;
    uint4 u = make_uint4(0u, 0u, 0u, 0u);
    if (c < nchunks) u = reinterpret_cast<const uint4*>(xr)[c];
    unpack8(u, v[i]);
  }
  if (LN) {
    // two-pass fp32 statistics (mean, then the mean square deviation; rsqrt).  Both are divided by C, not multiplied by a
    // rounded 1 / C: the mean of a constant row is then its value exactly (C * x is exact in fp32), so y == beta
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += v[i][e];
    const float mean = wave_sum(sum) / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      if (lane + 64 * i < nchunks) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float t = v[i][e] - mean;
          sq += t * t;
        }
      }
    const float rstd = rsqrtf(wave_sum(sq) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + 64 * i;
      if (c < nchunks) {
        const float4 g0 = reinterpret_cast<const float4*>(gamma)[2 * c], g1 = reinterpret_cast<const float4*>(gamma)[2 * c + 1];
        const float4 b0 = reinterpret_cast<const float4*>(beta)[2 * c], b1 = reinterpret_cast<const float4*>(beta)[2 * c + 1];
        const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) v[i][e] = fmaf((v[i][e] - mean) * rstd, g[e], b[e]);
      }
    }
  }
  uint8_t* qr = q + r * (int64_t)ldq;
  uint8_t* sr = qs + r * (int64_t)(ldq >> 5);
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = lane + 64 * i;
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(v[i][e]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));   // the 4 lanes of a 32-element block (C % 32 == 0: all in or all out)
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    const int k = mx_scale_exp(amax);
    const float inv = mx_inv_scale(k);
    if (c < nchunks) {
      *reinterpret_cast<uint2*>(qr + c * 8) = make_uint2(mx_pack4(&v[i][0], inv), mx_pack4(&v[i][4], inv));
      if ((lane & 3) == 0) sr[c >> 2] = (uint8_t)(k + 127);
    }
  }
  // zero elements (and 2^-127 scales) up to the padded row length: the K tail of the consumer GEMM
  for (int c = nchunks + lane; c < (ldq >> 3); c += 64) {
    *reinterpret_cast<uint2*>(qr + c * 8) = make_uint2(0u, 0u);
    if ((c & 3) == 0) sr[c >> 2] = 0;
  }
}

// ---- GEMM ----------------------------------------------------------------------------------------------------------------
constexpr int MX_BM = 256, MX_BN = 256, MX_BK = 128;      // BK in elements = bytes per row of a stage
constexpr int MX_WAVES_M = 2, MX_WAVES_N = 4, MX_NW = 8;
constexpr int MX_WTM = MX_BM / MX_WAVES_M, MX_WTN = MX_BN / MX_WAVES_N;   // 128 x 64 per wave
constexpr int MX_TM = MX_WTM / 32, MX_TN = MX_WTN / 32;
constexpr int MX_A_BYTES = MX_BM * MX_BK, MX_B_BYTES = MX_BN * MX_BK;
constexpr int MX_AS_OFF = MX_A_BYTES + MX_B_BYTES, MX_BS_OFF = MX_AS_OFF + MX_BM * 4;
constexpr int MX_STAGE = MX_BS_OFF + MX_BN * 4;
constexpr int MX_A_INSTR = MX_BM / 8 / MX_NW, MX_B_INSTR = MX_BN / 8 / MX_NW;   // 1-KiB data pieces per wave per K-tile
static_assert(MX_BM / 64 + MX_BN / 64 == MX_NW, "one 256-byte scale piece per wave per K-tile");

struct MxArgs {
  const uint8_t* a;
  const uint8_t* as;
  const uint8_t* w;
  const uint8_t* ws;
  const float* bias;
  const bf16_t* res;
  void* out;
  uint8_t* os;
  int M, N, K, lda, ldw, ldr, ldc, out_fmt, act, act_after_res, tiles_n;
};

// ---- epilogue of one 32 x 32 accumulator tile: the lane holds row m and columns nb + q * 8 + 4 h + (0..3), q = 0..3
__device__ __forceinline__ void mx_epilogue(const MxArgs& p, const f32x16 acc, int m, int nb, int fhi, const ActParams& ap) {
  const bool mok = m < p.M;
  float v[16];
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    const int n = nb + qd * 8 + fhi * 4;
    float* vv = v + qd * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) vv[e] = acc[qd * 4 + e];
    if (p.bias) {
      const float4 b = *reinterpret_cast<const float4*>(p.bias + n);
      vv[0] += b.x; vv[1] += b.y; vv[2] += b.z; vv[3] += b.w;
    }
    if (!p.act_after_res)
#pragma unroll
      for (int e = 0; e < 4; ++e) vv[e] = act1(vv[e], ap);
    if (p.res && mok) {
      const uint2 r = *reinterpret_cast<const uint2*>(p.res + (size_t)m * p.ldr + n);
      vv[0] += bf2f(r.x & 0xffffu); vv[1] += bf2f(r.x >> 16); vv[2] += bf2f(r.y & 0xffffu); vv[3] += bf2f(r.y >> 16);
    }
    if (p.act_after_res)
#pragma unroll
      for (int e = 0; e < 4; ++e) vv[e] = act1(vv[e], ap);
  }
  if (p.out_fmt == 2) {
    // the row's 32-column block: 16 values here, 16 in lane ^ 32
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fabsf(v[e]));
    amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
    const int k = mx_scale_exp(amax);
    const float inv = mx_inv_scale(k);
    if (mok) {
      uint8_t* o = reinterpret_cast<uint8_t*>(p.out) + (size_t)m * p.ldc + nb + fhi * 4;
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) *reinterpret_cast<uint32_t*>(o + qd * 8) = mx_pack4(v + qd * 4, inv);
      if (fhi == 0) p.os[(size_t)m * (p.ldc >> 5) + (nb >> 5)] = (uint8_t)(k + 127);
    }
  } else if (mok) {
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int n = nb + qd * 8 + fhi * 4;
      const float* vv = v + qd * 4;
      if (p.out_fmt == 1) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.out) + (size_t)m * p.ldc + n) = make_float4(vv[0], vv[1], vv[2], vv[3]);
      } else {
        *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(p.out) + (size_t)m * p.ldc + n) =
            make_uint2(pack_bf2(vv[0], vv[1]), pack_bf2(vv[2], vv[3]));
      }
    }
  }
}

__global__ void __launch_bounds__(MX_NW * 64) gemm_mx_kernel(const MxArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / MX_WAVES_N, wn = wave % MX_WAVES_N;

  int tile;
  {   // consecutive tiles on one XCD (blocks go round-robin over the 8 XCDs)
    const int nb = gridDim.x, bid = blockIdx.x;
    const int q = nb >> 3, r = nb & 7, xcd = bid & 7, i = bid >> 3;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + i;
  }
  const int mt = tile / p.tiles_n, nt = tile - mt * p.tiles_n;
  const int m0 = mt * MX_BM, n0 = nt * MX_BN;

  // ---- per-lane DMA sources: lane fills physical 16-byte slot (lane & 7) of row (lane >> 3) of an 8-row piece; the row's
  // chunk c lives in slot c ^ (row & 7), so the ds_read_b128 fragment reads below are conflict free.  Rows past M / N
  // re-read the last row (their results are never stored); K is padded with zero elements to the row length.
  const int lrow = lane >> 3, lslot = lane & 7;
  const uint8_t* a_src[MX_A_INSTR];
  const uint8_t* b_src[MX_B_INSTR];
#pragma unroll
  for (int j = 0; j < MX_A_INSTR; ++j) {
    const int r = (wave * MX_A_INSTR + j) * 8 + lrow;
    const int m = min(m0 + r, p.M - 1);
    a_src[j] = p.a + (size_t)m * p.lda + ((lslot ^ (r & 7)) << 4);
  }
#pragma unroll
  for (int j = 0; j < MX_B_INSTR; ++j) {
    const int r = (wave * MX_B_INSTR + j) * 8 + lrow;
    const int n = min(n0 + r, p.N - 1);
    b_src[j] = p.w + (size_t)n * p.ldw + ((lslot ^ (r & 7)) << 4);
  }
  // scales: wave w < BM / 64 fetches the A-scale dwords of rows 64 w .. 64 w + 63, the others those of B
  const bool s_is_a = wave < MX_BM / 64;
  const int s_piece = s_is_a ? wave : wave - MX_BM / 64;
  const uint8_t* s_src;
  {
    const int r = s_piece * 64 + lane;
    s_src = s_is_a ? p.as + (size_t)min(m0 + r, p.M - 1) * (p.lda >> 5) : p.ws + (size_t)min(n0 + r, p.N - 1) * (p.ldw >> 5);
  }
  const int s_dst = (s_is_a ? MX_AS_OFF : MX_BS_OFF) + s_piece * 256;

  auto issue = [&](int kt, int stage) __attribute__((always_inline)) {
    char* st = smem + stage * MX_STAGE;
    const int kb = kt * MX_BK;
#pragma unroll
    for (int j = 0; j < MX_A_INSTR; ++j)
      __builtin_amdgcn_global_load_lds((const void*)(a_src[j] + kb), (mx_lds_ptr_t)(st + (wave * MX_A_INSTR + j) * 1024), 16, 0, 0);
#pragma unroll
    for (int j = 0; j < MX_B_INSTR; ++j)
      __builtin_amdgcn_global_load_lds((const void*)(b_src[j] + kb), (mx_lds_ptr_t)(st + MX_A_BYTES + (wave * MX_B_INSTR + j) * 1024),
                                       16, 0, 0);
    __builtin_amdgcn_global_load_lds((const void*)(s_src + kt * 4), (mx_lds_ptr_t)(st + s_dst), 4, 0, 0);
  };

  f32x16 acc[MX_TM][MX_TN];
#pragma unroll
  for (int i = 0; i < MX_TM; ++i)
#pragma unroll
    for (int j = 0; j < MX_TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int nk = (p.K + MX_BK - 1) / MX_BK;
  const int frow = lane & 31;
  const int fhi = lane >> 5;

  issue(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of tile kt have landed
    tfimm_lds_reuse_barrier();                         // ... everyone's; and stage cur ^ 1 is free again
    asm volatile("" ::: "memory");
    if (kt + 1 < nk) issue(kt + 1, cur ^ 1);

    const char* st = smem + cur * MX_STAGE;
    const uint4* sA = reinterpret_cast<const uint4*>(st);
    const uint4* sB = reinterpret_cast<const uint4*>(st + MX_A_BYTES);
    const uint32_t* sAs = reinterpret_cast<const uint32_t*>(st + MX_AS_OFF);
    const uint32_t* sBs = reinterpret_cast<const uint32_t*>(st + MX_BS_OFF);
    uint32_t xs_w[MX_TM], ws_w[MX_TN];
#pragma unroll
    for (int i = 0; i < MX_TM; ++i) xs_w[i] = sAs[wm * MX_WTM + i * 32 + frow];
#pragma unroll
    for (int j = 0; j < MX_TN; ++j) ws_w[j] = sBs[wn * MX_WTN + j * 32 + frow];
#pragma unroll
    for (int s = 0; s < MX_BK / 64; ++s) {
      // operand lane map of the scaled instruction (measured with exact integer data and per-block scales): lane (row r,
      // half h) holds k = 16 h .. 16 h + 15 in bytes 0..15 and k = 32 + 16 h .. 32 + 16 h + 15 in bytes 16..31 of the
      // 64-deep step, while its scale byte covers the 32-block h (k = 32 h .. 32 h + 31) of BOTH halves -- so byte j of
      // half h is a different k than the scale layout suggests.  16-byte chunks 4 s + h and 4 s + 2 + h of the row.
      const int c0 = 4 * s + fhi;
      i32x8 fx[MX_TM], fw[MX_TN];
      int sx[MX_TM], sw[MX_TN];
#pragma unroll
      for (int i = 0; i < MX_TM; ++i) {
        const int row = wm * MX_WTM + i * 32 + frow;
        const uint4 lo = sA[row * 8 + (c0 ^ (row & 7))], hi = sA[row * 8 + ((c0 + 2) ^ (row & 7))];
        fx[i] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
        sx[i] = (int)((xs_w[i] >> (8 * (2 * s + fhi))) & 0xffu);
      }
#pragma unroll
      for (int j = 0; j < MX_TN; ++j) {
        const int row = wn * MX_WTN + j * 32 + frow;
        const uint4 lo = sB[row * 8 + (c0 ^ (row & 7))], hi = sB[row * 8 + ((c0 + 2) ^ (row & 7))];
        fw[j] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
        sw[j] = (int)((ws_w[j] >> (8 * (2 * s + fhi))) & 0xffu);
      }
      // the weight tile is the instruction's A operand: D[n][m], so a lane ends up with ONE output row m (its column)
#pragma unroll
      for (int i = 0; i < MX_TM; ++i)
#pragma unroll
        for (int j = 0; j < MX_TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[j], fx[i], acc[i][j], 0, 0, 0, sw[j], 0, sx[i]);
    }
  }

  // ---- epilogue in registers
  const ActParams ap = make_act(p.act);
#pragma clang loop unroll(full)
  for (int i = 0; i < MX_TM; ++i) {
    const int m = m0 + wm * MX_WTM + i * 32 + frow;
#pragma clang loop unroll(full)
    for (int j = 0; j < MX_TN; ++j) {
      const int nb = n0 + wn * MX_WTN + j * 32;     // N % 32 == 0: a 32-column block is all in or all out
      if (nb < p.N) mx_epilogue(p, acc[i][j], m, nb, fhi, ap);   // wave-uniform
    }
  }
}

inline bool mis(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" int tfimm_hip_quantize_mx(const void* x, int64_t rows, int C, int64_t x_stride, const float* gamma, const float* beta,
                                     float eps, void* q, void* q_scale, int ldq, void* stream) {
  if (!x || !q || !q_scale) TFIMM_FAIL(TFIMM_EINVAL, "quantize_mx: null pointer");
  if (rows <= 0 || C <= 0 || (C & 31) || x_stride < C || (x_stride & 7) || ldq < C || (ldq & 31))
    TFIMM_FAIL(TFIMM_EINVAL, "quantize_mx: bad shape (C %% 32 == 0, x_stride >= C, x_stride %% 8 == 0, ldq >= C, ldq %% 32 == 0)");
  if ((gamma == nullptr) != (beta == nullptr)) TFIMM_FAIL(TFIMM_EINVAL, "quantize_mx: gamma and beta go together");
  if (gamma && !(eps >= 0.f)) TFIMM_FAIL(TFIMM_EINVAL, "quantize_mx: eps < 0");
  if (mis(x, 16) || mis(q, 8) || (gamma && (mis(gamma, 16) || mis(beta, 16))))
    TFIMM_FAIL(TFIMM_EINVAL, "quantize_mx: x / gamma / beta must be 16-byte aligned, q 8-byte aligned");
  if (C > 4096) TFIMM_FAIL(TFIMM_EUNSUP, "quantize_mx: rows of at most 4096 channels");
  if (rows > ((int64_t)INT32_MAX) * 4) TFIMM_FAIL(TFIMM_EUNSUP, "quantize_mx: too many rows");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((rows + 3) / 4));
  const bf16_t* xb = (const bf16_t*)x;
  uint8_t* qb = (uint8_t*)q;
  uint8_t* sb = (uint8_t*)q_scale;
  const int nch = (C + 511) / 512;
#define TFIMM_MXQ(N)                                                                                                      \
  if (gamma) TFIMM_LAUNCH((quantize_mx_kernel<N, true>), grid, dim3(256), 0, st, xb, rows, C, x_stride, gamma, beta, eps, qb, sb, ldq); \
  else TFIMM_LAUNCH((quantize_mx_kernel<N, false>), grid, dim3(256), 0, st, xb, rows, C, x_stride, gamma, beta, eps, qb, sb, ldq)
  if (nch == 1) { TFIMM_MXQ(1); }
  else if (nch == 2) { TFIMM_MXQ(2); }
  else if (nch <= 4) { TFIMM_MXQ(4); }
  else { TFIMM_MXQ(8); }
#undef TFIMM_MXQ
  return 0;
}

extern "C" int tfimm_hip_gemm_mx(const tfimm_gemm_mx_desc* d, void* stream) {
  if (!d) TFIMM_FAIL(TFIMM_EINVAL, "gemm_mx: null descriptor");
  if (!d->a || !d->a_scale || !d->w || !d->w_scale || !d->out) TFIMM_FAIL(TFIMM_EINVAL, "gemm_mx: null operand");
  if (d->M <= 0 || d->N <= 0 || d->K <= 0 || (d->K & 31) || (d->N & 31))
    TFIMM_FAIL(TFIMM_EINVAL, "gemm_mx: bad shape M=%d N=%d K=%d (K and N multiples of 32)", d->M, d->N, d->K);
  const int kp = (d->K + MX_BK - 1) / MX_BK * MX_BK;
  if ((d->lda & 127) || (d->ldw & 127) || d->lda < kp || d->ldw < kp)
    TFIMM_FAIL(TFIMM_EINVAL, "gemm_mx: lda / ldw must be multiples of 128 and >= K rounded up to 128 (%d)", kp);
  if (d->out_fmt < 0 || d->out_fmt > 2 || d->act < TFIMM_ACT_NONE || d->act > TFIMM_ACT_TANH)
    TFIMM_FAIL(TFIMM_EINVAL, "gemm_mx: bad out_fmt / act");
  if (d->out_fmt == 2 ? (!d->out_scale || d->ldc != d->N || (d->N & 127)) : (d->ldc < d->N || (d->ldc & 3)))
    TFIMM_FAIL(TFIMM_EINVAL, "gemm_mx: bad ldc (MXFP8 output: ldc == N, N %% 128 == 0, out_scale set; otherwise ldc >= N, ldc %% 4 == 0)");
  if (d->residual && (d->ldr < d->N || (d->ldr & 3) || mis(d->residual, 8)))
    TFIMM_FAIL(TFIMM_EINVAL, "gemm_mx: residual needs ldr >= N, ldr %% 4 == 0, 8-byte alignment");
  if (mis(d->a, 16) || mis(d->w, 16) || mis(d->a_scale, 4) || mis(d->w_scale, 4) || (d->bias && mis(d->bias, 16)) ||
      mis(d->out, d->out_fmt == 1 ? 16 : d->out_fmt == 0 ? 8 : 4))
    TFIMM_FAIL(TFIMM_EINVAL, "gemm_mx: misaligned pointer");
  MxArgs p;
  p.a = (const uint8_t*)d->a; p.as = (const uint8_t*)d->a_scale;
  p.w = (const uint8_t*)d->w; p.ws = (const uint8_t*)d->w_scale;
  p.bias = d->bias; p.res = (const bf16_t*)d->residual;
  p.out = d->out; p.os = (uint8_t*)d->out_scale;
  p.M = d->M; p.N = d->N; p.K = d->K;
  p.lda = d->lda; p.ldw = d->ldw; p.ldr = d->ldr; p.ldc = d->ldc;
  p.out_fmt = d->out_fmt; p.act = d->act; p.act_after_res = d->act_after_res ? 1 : 0;
  const int64_t tiles_m = (d->M + MX_BM - 1) / MX_BM;
  p.tiles_n = (d->N + MX_BN - 1) / MX_BN;
  if (tiles_m * p.tiles_n > INT32_MAX) TFIMM_FAIL(TFIMM_EUNSUP, "gemm_mx: too many tiles");
  static tfimm_once_t once;
  if (once.need()) {
    TFIMM_HIP_CHECK(hipFuncSetAttribute((const void*)gemm_mx_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * MX_STAGE));
    once.mark();
  }
  TFIMM_LAUNCH(gemm_mx_kernel, dim3((unsigned)(tiles_m * p.tiles_n)), dim3(MX_NW * 64), 2 * MX_STAGE, (hipStream_t)stream, p);
  return 0;
}

// tfimm_hip_lora_delta: the low-rank term of a LoRA Dense layer in ONE launch (gfx950),
//
//     t   = bf16( x[M][K] . A[K][R] )                      fp32 accumulation, one rounding
//     out = bf16( residual[M][N] + t[M][R] . B'[R][N] )    fp32 accumulation
//
// (LoRADense.call, reference architectures/lora/layers.py:93-100: x2 = (x A) B; scaling and a LayerScale behind the layer are
// folded into B' by the host.)  The result is the `residual` operand of the layer's full-rank tfimm_hip_gemm launch, so the
// adapter weights never touch the layer's packed kernel and can be swapped without re-packing it.
//
// Both products run on the matrix unit (mfma_f32_16x16x32_bf16) and t never leaves the registers:
//   * a wave owns 32 rows of x (two 16-row tiles), a workgroup of 4 waves 128 rows; waves do not communicate (no LDS, no
//     barrier), so a row's result cannot depend on M or on its neighbours.
//   * product 1 is computed TRANSPOSED, T^T = A^T . x^T per 16-rank tile: the A operand is a row segment of a[rank][k], the B
//     operand a row segment of x[m][k] -- both plain 16-byte loads.  The accumulator of a tile then holds, in lane (c, g) =
//     (lane & 15, lane >> 4), the ranks 4 g .. 4 g + 3 of row m = c.
//   * product 2 is out^T = B'^T . T^T, which sums over the rank: T^T is its B operand, whose lane (c, g) must hold 8 values of
//     the summation index for column c.  Two rank tiles make one 32-deep step: elements 0-3 of the fragment are the four
//     accumulators of the even tile (ranks 4 g + j), elements 4-7 those of the odd tile (ranks 16 + 4 g + j), rounded to bf16
//     once.  The summation order inside a step is free as long as both operands agree, so the A operand b[n][rank] is fetched
//     in the same order: two 8-byte loads per step.  An odd tile that does not exist (Rp = 16, 48) is zero on both sides.
//   * the result tile holds, in lane (c, g), out[m = c][n0 + 4 g .. + 3]: the residual is read and the output written as
//     8-byte pieces, four consecutive 16-column tiles (one 128-byte line per row) per trip.
// Traffic: x and residual are read once and out is written once; a and b (at most 2 * 64 * 8192 * 2 bytes, L2 resident) are
// re-read by every wave -- a: Rp / 32 times the bytes of x.
#include "common.h"

namespace {

constexpr int kLoraWaves = 4;                      // waves per workgroup
constexpr int kLoraMT = 2;                         // 16-row tiles per wave
constexpr int kLoraRows = kLoraWaves * kLoraMT * 16;   // rows per workgroup
constexpr int kLoraNT = 4;                         // 16-column output tiles per trip

typedef __attribute__((ext_vector_type(4))) unsigned int lora_u32x4;

struct LoraArgs {
  const bf16_t* x;
  const bf16_t* a;
  const bf16_t* b;
  const bf16_t* residual;
  bf16_t* out;
  int64_t M, lda, lda_a, ldr, ldc;
  int K, N, Rp;
};

__device__ __forceinline__ bf16x8 lora_load8(const bf16_t* p, bool ok) {
  lora_u32x4 v = {0u, 0u, 0u, 0u};
  if (ok) v = *reinterpret_cast<const lora_u32x4*>(p);
  return __builtin_bit_cast(bf16x8, v);
}

template <int RT>   // rank tiles of 16: Rp = 16 RT
__global__ void __launch_bounds__(kLoraWaves * 64) lora_delta_kernel(const LoraArgs p) {
  constexpr int S = (RT + 1) / 2;                  // 32-deep steps of product 2
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int64_t m_base = (int64_t)blockIdx.x * kLoraRows + wave * (kLoraMT * 16);
  if (m_base >= p.M) return;                       // (no barrier anywhere in this kernel)

  // ---- product 1: tacc[mt][rt] = T^T of (16 ranks of tile rt) x (16 rows of tile mt) ----------------------------------
  f32x4 tacc[kLoraMT][RT];
  const bf16_t* xrow[kLoraMT];
  bool xok[kLoraMT];
#pragma unroll
  for (int mt = 0; mt < kLoraMT; ++mt) {
    const int64_t m = m_base + mt * 16 + c;
    xok[mt] = m < p.M;
    xrow[mt] = p.x + (xok[mt] ? m : 0) * p.lda + 8 * g;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) tacc[mt][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const bf16_t* arow = p.a + (int64_t)c * p.lda_a + 8 * g;
  for (int k0 = 0; k0 < p.K; k0 += 32) {
    const bool kin = k0 + 8 * g < p.K;             // K is a multiple of 8: a lane's 8 values are all inside or all outside
    bf16x8 xf[kLoraMT], af[RT];
#pragma unroll
    for (int mt = 0; mt < kLoraMT; ++mt) xf[mt] = lora_load8(xrow[mt] + k0, kin && xok[mt]);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) af[rt] = lora_load8(arow + (int64_t)rt * 16 * p.lda_a + k0, kin);
#pragma unroll
    for (int mt = 0; mt < kLoraMT; ++mt)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
        tacc[mt][rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[rt], xf[mt], tacc[mt][rt], 0, 0, 0);
  }

  // ---- t rounded to bf16 once, as the B operand of product 2 ----------------------------------------------------------
  bf16x8 tb[kLoraMT][S];
#pragma unroll
  for (int mt = 0; mt < kLoraMT; ++mt)
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const f32x4 lo = tacc[mt][2 * s];
      lora_u32x4 v;
      v.x = pack_bf2(lo[0], lo[1]);
      v.y = pack_bf2(lo[2], lo[3]);
      if (2 * s + 1 < RT) {
        const f32x4 hi = tacc[mt][(2 * s + 1 < RT) ? 2 * s + 1 : 0];
        v.z = pack_bf2(hi[0], hi[1]);
        v.w = pack_bf2(hi[2], hi[3]);
      } else {
        v.z = 0u;
        v.w = 0u;
      }
      tb[mt][s] = __builtin_bit_cast(bf16x8, v);
    }

  // ---- product 2 and the epilogue, 64 output columns per trip ----------------------------------------------------------
  int64_t orow[kLoraMT];
#pragma unroll
  for (int mt = 0; mt < kLoraMT; ++mt) orow[mt] = xok[mt] ? m_base + mt * 16 + c : 0;
  const bool has_res = p.residual != nullptr;
  for (int n0 = 0; n0 < p.N; n0 += 16 * kLoraNT) {
    f32x4 acc[kLoraNT][kLoraMT];
    uint2 res[kLoraNT][kLoraMT];
#pragma unroll
    for (int nt = 0; nt < kLoraNT; ++nt) {
      const int nc = n0 + nt * 16 + 4 * g;         // this lane's 4 output columns (N % 8 == 0: all inside or all outside)
#pragma unroll
      for (int mt = 0; mt < kLoraMT; ++mt) {
        res[nt][mt] = uint2{0u, 0u};
        if (has_res && nc < p.N && xok[mt]) res[nt][mt] = *reinterpret_cast<const uint2*>(p.residual + orow[mt] * p.ldr + nc);
        acc[nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int nt = 0; nt < kLoraNT; ++nt) {
      const int n = n0 + nt * 16 + c;              // the row of b this lane feeds to the A operand
      const bool nok = n < p.N;
      const bf16_t* brow = p.b + (int64_t)(nok ? n : 0) * p.Rp + 4 * g;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        lora_u32x4 v = {0u, 0u, 0u, 0u};
        if (nok) {
          const uint2 lo = *reinterpret_cast<const uint2*>(brow + 32 * s);
          v.x = lo.x;
          v.y = lo.y;
          if (2 * s + 1 < RT) {
            const uint2 hi = *reinterpret_cast<const uint2*>(brow + 32 * s + 16);
            v.z = hi.x;
            v.w = hi.y;
          }
        }
        const bf16x8 bf = __builtin_bit_cast(bf16x8, v);
#pragma unroll
        for (int mt = 0; mt < kLoraMT; ++mt)
          acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, tb[mt][s], acc[nt][mt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int nt = 0; nt < kLoraNT; ++nt) {
      const int nc = n0 + nt * 16 + 4 * g;
#pragma unroll
      for (int mt = 0; mt < kLoraMT; ++mt) {
        if (nc >= p.N || !xok[mt]) continue;
        const uint2 r = res[nt][mt];
        const f32x4 v = acc[nt][mt];
        uint2 o;
        o.x = pack_bf2(v[0] + bf2f(r.x & 0xffffu), v[1] + bf2f(r.x >> 16));
        o.y = pack_bf2(v[2] + bf2f(r.y & 0xffffu), v[3] + bf2f(r.y >> 16));
        *reinterpret_cast<uint2*>(p.out + orow[mt] * p.ldc + nc) = o;
      }
    }
  }
}

bool lora_overlap(const void* p0, int64_t n0, const void* p1, int64_t n1) {
  const uintptr_t a0 = (uintptr_t)p0, a1 = (uintptr_t)p1;
  return a0 < a1 + (uintptr_t)n1 && a1 < a0 + (uintptr_t)n0;
}

}  // namespace

// The descriptor checks of tfimm_hip_lora_delta and of its float32 twin (ref32.hip); ``elem``: bytes per element, ``align``: what
// every pointer must be aligned to.  0, or the error code with the message set.
int tfimm_lora_validate(const tfimm_lora_desc* dp, int elem, int align, const char* who) {
  if (!dp) TFIMM_FAIL(TFIMM_EINVAL, "%s: null descriptor", who);
  const tfimm_lora_desc& d = *dp;
  if (!d.x || !d.a || !d.b || !d.out) TFIMM_FAIL(TFIMM_EINVAL, "%s: x, a, b and out must not be null", who);
  if (d.M < 0) TFIMM_FAIL(TFIMM_EINVAL, "%s: M=%lld is negative", who, (long long)d.M);
  if (d.K < 8 || d.K % 8 || d.K > TFIMM_LORA_MAX_DIM)
    TFIMM_FAIL(TFIMM_EUNSUP, "%s: K=%d, must be a multiple of 8 in [8, %d]", who, d.K, TFIMM_LORA_MAX_DIM);
  if (d.N < 8 || d.N % 8 || d.N > TFIMM_LORA_MAX_DIM)
    TFIMM_FAIL(TFIMM_EUNSUP, "%s: N=%d, must be a multiple of 8 in [8, %d]", who, d.N, TFIMM_LORA_MAX_DIM);
  if (d.Rp < 16 || d.Rp % 16 || d.Rp > TFIMM_LORA_MAX_RP)
    TFIMM_FAIL(TFIMM_EUNSUP, "%s: Rp=%d, must be a multiple of 16 in [16, %d]", who, d.Rp, TFIMM_LORA_MAX_RP);
  if (d.lda < d.K || d.lda % 8) TFIMM_FAIL(TFIMM_EINVAL, "%s: lda=%d, must be a multiple of 8 and at least K=%d", who, d.lda, d.K);
  if (d.lda_a < d.K || d.lda_a % 8)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: lda_a=%d, must be a multiple of 8 and at least K=%d", who, d.lda_a, d.K);
  if (d.ldc < d.N || d.ldc % 8) TFIMM_FAIL(TFIMM_EINVAL, "%s: ldc=%d, must be a multiple of 8 and at least N=%d", who, d.ldc, d.N);
  if (d.residual && (d.ldr < d.N || d.ldr % 8))
    TFIMM_FAIL(TFIMM_EINVAL, "%s: ldr=%d, must be a multiple of 8 and at least N=%d", who, d.ldr, d.N);
  const uintptr_t ptrs = (uintptr_t)d.x | (uintptr_t)d.a | (uintptr_t)d.b | (uintptr_t)d.residual | (uintptr_t)d.out;
  if (ptrs & (uintptr_t)(align - 1)) TFIMM_FAIL(TFIMM_EINVAL, "%s: x, a, b, residual and out must be %d-byte aligned", who, align);
  if (d.M > 0) {
    const int64_t e = elem;
    const int64_t out_bytes = ((d.M - 1) * d.ldc + d.N) * e;
    if (lora_overlap(d.out, out_bytes, d.x, ((d.M - 1) * d.lda + d.K) * e)) TFIMM_FAIL(TFIMM_EINVAL, "%s: out overlaps x", who);
    if (lora_overlap(d.out, out_bytes, d.a, ((int64_t)(d.Rp - 1) * d.lda_a + d.K) * e))
      TFIMM_FAIL(TFIMM_EINVAL, "%s: out overlaps a", who);
    if (lora_overlap(d.out, out_bytes, d.b, (int64_t)d.N * d.Rp * e)) TFIMM_FAIL(TFIMM_EINVAL, "%s: out overlaps b", who);
    if (d.residual && lora_overlap(d.out, out_bytes, d.residual, ((d.M - 1) * d.ldr + d.N) * e))
      TFIMM_FAIL(TFIMM_EINVAL, "%s: out overlaps residual", who);
    if ((d.M + kLoraRows - 1) / kLoraRows > 0x7fffffffll) TFIMM_FAIL(TFIMM_EUNSUP, "%s: M=%lld exceeds the grid", who, (long long)d.M);
  }
  return 0;
}

extern "C" int tfimm_hip_lora_delta(const tfimm_lora_desc* dp, void* stream) {
  const int rc = tfimm_lora_validate(dp, 2, 16, "lora_delta");
  if (rc) return rc;
  const tfimm_lora_desc& d = *dp;
  if (d.M == 0) return 0;
  LoraArgs p;
  p.x = (const bf16_t*)d.x; p.a = (const bf16_t*)d.a; p.b = (const bf16_t*)d.b; p.residual = (const bf16_t*)d.residual;
  p.out = (bf16_t*)d.out;
  p.M = d.M; p.lda = d.lda; p.lda_a = d.lda_a; p.ldr = d.ldr; p.ldc = d.ldc;
  p.K = d.K; p.N = d.N; p.Rp = d.Rp;
  const dim3 grid((unsigned)((d.M + kLoraRows - 1) / kLoraRows)), block(kLoraWaves * 64);
  switch (d.Rp / 16) {
    case 1: TFIMM_LAUNCH(lora_delta_kernel<1>, grid, block, 0, (hipStream_t)stream, p); break;
    case 2: TFIMM_LAUNCH(lora_delta_kernel<2>, grid, block, 0, (hipStream_t)stream, p); break;
    case 3: TFIMM_LAUNCH(lora_delta_kernel<3>, grid, block, 0, (hipStream_t)stream, p); break;
    default: TFIMM_LAUNCH(lora_delta_kernel<4>, grid, block, 0, (hipStream_t)stream, p); break;
  }
  return 0;
}

// The distillation gradient (include/tfimm_hip.h; the CPU restatement of the rule is tests/distill_ref.py):
// per row the squared distance between the L2-normalised student and teacher embeddings, its gradient with respect to the
// student as the bf16 rows tfimm_hip_head_update reads, and the cosine -- the loss of the reference's DistillationProblem
// behind the student's head, between tfimm_hip_gemm and tfimm_hip_head_update.
//
// One wave per row, four rows per workgroup (the mapping of l2_normalize in embed.hip).  Lane l owns the 4-column pieces
// l, l + 64, ... of its row: 16-byte loads of s and t, one 8-byte store of the four bf16 gradients.  Two passes over the row:
//   1. sum s^2, sum t^2, sum s t: the lane adds its even and its odd columns in ascending order with one fma per term, adds
//      the two, and the 64 partial sums go through the fixed six-step butterfly of wave_sum (float addition commutes
//      exactly: every lane holds the same bits).
//      inv_s, inv_t by tfimm_hip_l2_normalize's expression (IEEE square root and division), c = (sum s t) * inv_s * inv_t.
//   2. the row is read again -- it was read a moment ago by the same wave: at most 32 KiB, an L2 hit -- and u, v, the
//      gradient and the terms of the loss are formed per element; the loss goes through the same per-lane order and butterfly.
// The loss is summed from (u - v)^2 and not taken from 2 - 2 c: a row with s == t has u == v bit for bit and a loss of
// exactly zero.  The piece that straddles E is read and written element by element, columns >= E are never touched.
// FMA contraction is off for the whole file (the pragma below): every fma is written out, so u - v stays the difference
// of the two ROUNDED products.
// Rows never mix, no LDS, no barrier, no atomics: bit-reproducible, and a row's four outputs depend neither on B nor on the
// workgroup that holds it.  (The vector loads need 16-byte aligned rows; rows that are not read the same pieces element by
// element, in the same order: the bits do not depend on the alignment either.)
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kRows = 4;   // rows (= waves) per workgroup

struct DistillArgs {
  const float* s;
  const float* t;
  const int32_t* valid;
  uint16_t* grad;
  float* loss;
  float* cosine;
  int64_t ld_s, ld_t, ldg;
  int B, E, normalize;
};

typedef tfimm_f32x2 f2;

__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

// columns [0, n) of the piece at p as the pairs (0, 1) and (2, 3), zeros behind column n (a zero adds nothing to any sum)
template <bool kVec>
__device__ __forceinline__ void load_piece(const float* p, int n, f2& lo, f2& hi) {
  if (n == 4) {
    if (kVec) {
      const float4 q = *reinterpret_cast<const float4*>(p);
      lo = f2{q.x, q.y};
      hi = f2{q.z, q.w};
    } else {
      lo = f2{p[0], p[1]};
      hi = f2{p[2], p[3]};
    }
  } else {
    lo = f2{p[0], n > 1 ? p[1] : 0.f};
    hi = f2{n > 2 ? p[2] : 0.f, 0.f};
  }
}

template <bool kVec>
__global__ void __launch_bounds__(64 * kRows) distill_grad_kernel(DistillArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kRows + (threadIdx.x >> 6);
  if (row >= a.B) return;
  const int E = a.E;
  uint16_t* gr = a.grad + row * a.ldg;

  // ---- a row that is not trained on: +0.0 everywhere, s and t are not read
  const int ok = a.valid[row];
  if (ok < 0 || ok >= E) {
    for (int c = 4 * lane; c < E; c += 256) {
      if (c + 4 <= E) {
        *reinterpret_cast<uint2*>(gr + c) = make_uint2(0u, 0u);
      } else {
        for (int i = 0; c + i < E; ++i) gr[c + i] = 0;
      }
    }
    if (lane == 0) {
      a.loss[row] = 0.f;
      a.cosine[row] = 0.f;
    }
    return;
  }

  const float* sr = a.s + row * a.ld_s;
  const float* tr = a.t + row * a.ld_t;

  // ---- pass 1: the three sums.  Everything per element is written on PAIRS of neighbouring columns -- the halves of an
  // accumulator pair hold the lane's even and odd columns, added once at the end: written with scalars, the vectoriser paired
  // registers of different origin and bridged them with operand selects (v_pk_fma_f32 ... op_sel), which tools/isa_lint.py
  // rules out on gfx950
  const f2 zero = {0.f, 0.f};
  f2 ss2 = zero, tt2 = zero, st2 = zero;
#pragma unroll 2
  for (int c = 4 * lane; c < E; c += 256) {
    f2 x0, x1, y0, y1;
    load_piece<kVec>(sr + c, min(4, E - c), x0, x1);
    load_piece<kVec>(tr + c, min(4, E - c), y0, y1);
    ss2 = fma2(x1, x1, fma2(x0, x0, ss2));
    tt2 = fma2(y1, y1, fma2(y0, y0, tt2));
    st2 = fma2(x1, y1, fma2(x0, y0, st2));
  }
  const float ss = wave_sum(ss2.x + ss2.y);
  const float tt = wave_sum(tt2.x + tt2.y);
  const float st = wave_sum(st2.x + st2.y);
  const float inv_s = __fdiv_rn(1.0f, __fsqrt_rn(fmaxf(ss, 1e-12f)));
  const float inv_t = __fdiv_rn(1.0f, __fsqrt_rn(fmaxf(tt, 1e-12f)));
  const float c_st = (st * inv_s) * inv_t;

  // ---- pass 2: gradient and loss.  normalize == 0 is the same expression with both scales 1 (u = s, v = t exactly) and
  // k = 1; so is a row under the clamp, whose inv_s is a constant: d/ds (u - v)^2 = 2 inv_s (u - v)
  const bool norm = a.normalize != 0;
  const float ks = norm ? inv_s : 1.0f, kt = norm ? inv_t : 1.0f;
  const float k = (norm && ss >= 1e-12f) ? c_st : 1.0f;
  const float two = 2.0f * ks;
  const f2 ks2 = {ks, ks}, kt2 = {kt, kt}, k2 = {k, k}, two2 = {two, two};
  f2 loss2 = zero;
#pragma unroll 2
  for (int c = 4 * lane; c < E; c += 256) {
    const int n = min(4, E - c);
    f2 x0, x1, y0, y1;
    load_piece<kVec>(sr + c, n, x0, x1);
    load_piece<kVec>(tr + c, n, y0, y1);
    const f2 u0 = x0 * ks2, u1 = x1 * ks2, v0 = y0 * kt2, v1 = y1 * kt2;
    const f2 d0 = u0 - v0, d1 = u1 - v1;
    loss2 = fma2(d1, d1, fma2(d0, d0, loss2));
    const f2 g0 = two2 * fma2(k2, u0, -v0), g1 = two2 * fma2(k2, u1, -v1);
    if (n == 4) {
      *reinterpret_cast<uint2*>(gr + c) = make_uint2(pack_bf2(g0.x, g0.y), pack_bf2(g1.x, g1.y));
    } else {
      gr[c] = (uint16_t)f2bf(g0.x);
      if (n > 1) gr[c + 1] = (uint16_t)f2bf(g0.y);
      if (n > 2) gr[c + 2] = (uint16_t)f2bf(g1.x);
    }
  }
  float loss = loss2.x + loss2.y;
  loss = wave_sum(loss);
  if (lane == 0) {
    a.loss[row] = loss;
    a.cosine[row] = c_st;
  }
}

}  // namespace

extern "C" int tfimm_hip_distill_grad(const float* s, int64_t ld_s, const float* t, int64_t ld_t, int B, int E, const int32_t* valid,
                                      int normalize, void* grad, int64_t ldg, float* loss, float* cosine, void* stream) {
  if (!s) TFIMM_FAIL(TFIMM_EINVAL, "distill_grad: s is null");
  if (!t) TFIMM_FAIL(TFIMM_EINVAL, "distill_grad: t is null");
  if (!valid) TFIMM_FAIL(TFIMM_EINVAL, "distill_grad: valid is null");
  if (!grad) TFIMM_FAIL(TFIMM_EINVAL, "distill_grad: grad is null");
  if (!loss) TFIMM_FAIL(TFIMM_EINVAL, "distill_grad: loss is null");
  if (!cosine) TFIMM_FAIL(TFIMM_EINVAL, "distill_grad: cosine is null");
  if (((uintptr_t)s | (uintptr_t)t | (uintptr_t)valid | (uintptr_t)loss | (uintptr_t)cosine) & 3)
    TFIMM_FAIL(TFIMM_EINVAL, "distill_grad: s, t, valid, loss and cosine hold 4-byte elements and must be 4-byte aligned");
  if ((uintptr_t)grad & 15) TFIMM_FAIL(TFIMM_EINVAL, "distill_grad: grad must be 16-byte aligned");
  if (E < 1 || E > TFIMM_DISTILL_MAX_E)
    TFIMM_FAIL(TFIMM_EINVAL, "distill_grad: E=%d, must be in [1, TFIMM_DISTILL_MAX_E = %d]", E, TFIMM_DISTILL_MAX_E);
  if (ld_s < E) TFIMM_FAIL(TFIMM_EINVAL, "distill_grad: ld_s=%lld is smaller than E=%d", (long long)ld_s, E);
  if (ld_t < E) TFIMM_FAIL(TFIMM_EINVAL, "distill_grad: ld_t=%lld is smaller than E=%d", (long long)ld_t, E);
  if (ldg < E || ldg % 8 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "distill_grad: ldg=%lld, must be a multiple of 8 elements and at least E=%d", (long long)ldg, E);
  if (B < 0) TFIMM_FAIL(TFIMM_EINVAL, "distill_grad: B=%d is negative", B);
  if (normalize != 0 && normalize != 1) TFIMM_FAIL(TFIMM_EINVAL, "distill_grad: normalize=%d, must be 0 or 1", normalize);
  if (B == 0) return 0;

  DistillArgs a;
  a.s = s;
  a.t = t;
  a.valid = valid;
  a.grad = reinterpret_cast<uint16_t*>(grad);
  a.loss = loss;
  a.cosine = cosine;
  a.ld_s = ld_s;
  a.ld_t = ld_t;
  a.ldg = ldg;
  a.B = B;
  a.E = E;
  a.normalize = normalize;
  const dim3 grid((unsigned)(((int64_t)B + kRows - 1) / kRows));
  const bool vec = (((uintptr_t)s | (uintptr_t)t) & 15) == 0 && ld_s % 4 == 0 && ld_t % 4 == 0;
  if (vec)
    TFIMM_LAUNCH(distill_grad_kernel<true>, grid, dim3(64 * kRows), 0, (hipStream_t)stream, a);
  else
    TFIMM_LAUNCH(distill_grad_kernel<false>, grid, dim3(64 * kRows), 0, (hipStream_t)stream, a);
  return 0;
}

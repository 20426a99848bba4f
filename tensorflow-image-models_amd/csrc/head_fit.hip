// The head fit (include/tfimm_hip.h; the CPU restatement of both rules is tests/head_fit_ref.py): one
// optimizer step of a classifier head on frozen features, behind the logits product of tfimm_hip_gemm.
//
// tfimm_hip_softmax_grad: the kernel of score.hip with the gradient row in place of the rank.  One workgroup of 256 threads
// per row, the row read from global memory once into LDS as the keys of topk_select.h; one selection round (pred, the
// maximum m), the sum of topk_row.h, then one more pass over the LDS copy: grad[c] = bf16_rne(expf(x_c - m) / sum - [c == y]),
// two columns per thread and one 4-byte store.  loss and pred are formed by score.hip's expressions from the same loader,
// round and sum, so they carry its bits.
//
// tfimm_hip_head_update: acc[c][d] = sum_b g[b][c] f[b][d] and the optimizer step on w[c][d] in one launch.
//   Grid (ceil(D / 128), ceil(C / 32)), 256 threads: a workgroup owns a 32-class x 128-column tile of w (s1, s2, w16, grad_out)
//   and nobody else touches it; wave v owns columns 32 v .. 32 v + 31.  The batch is walked in chunks of 128 rows: the g chunk
//   [128 b][32 c] and the f chunk [128 b][128 d] go through registers (the next chunk's global loads are issued before this
//   chunk's MFMAs) into LDS, row-major with 64-byte rows -- g as one image, f as one [128 b][32 d] image per wave (40 KB).
//   (A long batch of few classes is a serial walk of few workgroups: the larger the chunk, the fewer waits for memory.)
//   Both operands of v_mfma_f32_32x32x16_bf16 are reduced over their ROW index here (A[c][k = b] = g[b][c], B[k = b][d] =
//   f[b][d]), so both come out of LDS through ds_read_b64_tr_b16: a 16-lane group fetches a 4-row x 16-column block as
//   8-byte pieces (lane 4 q + p: row q, columns 4 p .. 4 p + 3) and lane i receives column i of the 4 rows.  Lane (r, h)
//   of the MFMA wants k = 8 h .. 8 h + 7 at column r: two reads, rows 8 h + 4 t .. + 3 (t = 0, 1), group (l >> 4) & 1 picks
//   columns 0..15 or 16..31.  With 64-byte rows the four rows of a block lie on four distinct quarters of the 64 banks and
//   the two groups of a 32-lane half on the two halves of a quarter: conflict-free without a swizzle.  A and B use the same
//   map, so every k meets its partner.  Rows >= B and columns >= C / >= D are written to LDS as zeros and never read from
//   global memory (the g chunk that straddles C is read element by element).
//   The accumulator has d on the lane (column = lane & 31) and 16 classes in the registers (row = (i & 3) + 8 (i >> 2) +
//   4 (lane >> 5)): the float32 reads and writes of w / s1 / s2 / grad_out are 128 contiguous bytes per half-wave.
//   n (labels in [0, C)) is counted by every workgroup for itself with integer adds; the bias column sum is formed by the
//   workgroups with blockIdx.x == 0 from the LDS image: thread (c, p) adds rows 16 p .. 16 p + 15 of every chunk of class c in
//   ascending order, the eight partial sums of a class are added in a fixed tree.
//   Behind acc every operation is a separate correctly rounded float32 operation: the helpers below are compiled with
//   contraction off (the __f*_rn intrinsics are plain operators in this toolchain and would fuse), division and square
//   root are the IEEE ones.
#include "topk_row.h"

namespace {

using namespace topk_sel;

// ------------------------------------------------------------------------------------------------------------------------
// softmax_grad
// ------------------------------------------------------------------------------------------------------------------------
struct SoftmaxGradArgs {
  const uint32_t* logits;   // float32 bits
  const int32_t* labels;
  uint16_t* grad;
  float* loss;
  int32_t* pred;
  int64_t ld, ldg;
  int N;
};

__global__ void __launch_bounds__(kThreads) softmax_grad_kernel(SoftmaxGradArgs a) {
  extern __shared__ uint32_t keys[];   // [N]
  __shared__ uint32_t w_key[kWaves];
  __shared__ int w_idx[kWaves];
  __shared__ float w_sum[kWaves];
  const int tid = threadIdx.x;
  const int N = a.N;
  const int64_t b = blockIdx.x;
  const uint32_t* row = a.logits + b * a.ld;

  load_row_keys(row, N, tid, keys);
  __syncthreads();

  uint32_t k0;
  int i0;
  select_round(keys, N, tid, w_key, w_idx, k0, i0);
  const float m = __uint_as_float(bits_of(k0));

  const int y = a.labels[b];
  const bool scored = y >= 0 && y < N;
  const uint32_t ky = scored ? keys[y] : kKeyNaN;

  const float part = sum_exp_partial(keys, N, tid, m, [](uint32_t, int) {});
  const float sum = block_sum(part, tid, w_sum);

  // ---- the gradient row: columns 2 i and 2 i + 1 in thread i, i + 256, ...
  uint16_t* grow = a.grad + b * a.ldg;
  for (int c = 2 * tid; c < N; c += 2 * kThreads) {
    uint32_t lo = 0, hi = 0;
    if (scored) {
      const float p0 = expf(__uint_as_float(bits_of(keys[c])) - m) / sum;
      lo = f2bf(p0 - (c == y ? 1.0f : 0.0f));
      if (c + 1 < N) {
        const float p1 = expf(__uint_as_float(bits_of(keys[c + 1])) - m) / sum;
        hi = f2bf(p1 - (c + 1 == y ? 1.0f : 0.0f));
      }
    }
    if (c + 1 < N)
      *reinterpret_cast<uint32_t*>(grow + c) = lo | (hi << 16);
    else
      grow[c] = (uint16_t)lo;
  }

  if (tid != 0) return;
  float loss = 0.f;
  if (scored) {
    const float d = __uint_as_float(bits_of(ky)) - m;
    loss = logf(sum) - d;
  }
  a.loss[b] = loss;
  a.pred[b] = i0;
}

// ------------------------------------------------------------------------------------------------------------------------
// head_update
// ------------------------------------------------------------------------------------------------------------------------
constexpr int kTileC = 32;     // classes per workgroup: the M dimension of the MFMA
constexpr int kTileD = 128;    // columns per workgroup: 32 per wave
constexpr int kChunkB = 128;   // batch rows per LDS stage: eight MFMA k-steps
constexpr int kFPieces = kChunkB * 16 / 256;   // 16-byte pieces of the f chunk per thread
constexpr int kGPieces = kChunkB * 4 / 256;    // ... of the g chunk
constexpr int kImage = kChunkB * 64;   // bytes of one [128 b][32 columns] bf16 image
static_assert(TFIMM_HEAD_MAX_C <= 65535 * kTileC, "class tiles are grid.y");

struct HeadArgs {
  const uint16_t* f;
  const uint16_t* g;
  const int32_t* labels;
  float* w;
  uint16_t* w16;
  float* s1;
  float* s2;
  float* bias;
  float* bias_s1;
  float* bias_s2;
  float* grad_out;
  float* bias_grad_out;
  int64_t ldf, ldg, ldw, ldw16;
  int B, D, C, opt;
  float lr, mom, omb2, eps, wd2;
};

// one float32 operation each, never fused with a neighbour
#pragma clang fp contract(off)
__device__ __forceinline__ float mul_rn(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ float add_rn(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}
__device__ __forceinline__ float sub_rn(float x, float y) {
#pragma clang fp contract(off)
  return x - y;
}
__device__ __forceinline__ float div_rn(float x, float y) {
#pragma clang fp contract(off)
  return x / y;
}
__device__ __forceinline__ float sqrt_rn(float x) { return __builtin_sqrtf(x); }

struct Step {
  float w, s1, s2, gd;
};

// gd -> the new (w, s1, s2) of one element
__device__ __forceinline__ void head_step(const HeadArgs& a, float acc, float inv_n, Step& e) {
#pragma clang fp contract(off)
  e.gd = mul_rn(acc, inv_n);
  const float gr = add_rn(e.gd, mul_rn(a.wd2, e.w));
  if (a.opt == TFIMM_HEAD_SGD) {
    e.s1 = sub_rn(mul_rn(a.mom, e.s1), mul_rn(a.lr, gr));
    e.w = add_rn(e.w, e.s1);
  } else {
    e.s1 = add_rn(e.s1, mul_rn(sub_rn(gr, e.s1), a.mom));
    e.s2 = add_rn(e.s2, mul_rn(sub_rn(mul_rn(gr, gr), e.s2), a.omb2));
    e.w = sub_rn(e.w, div_rn(mul_rn(e.s1, a.lr), add_rn(sqrt_rn(e.s2), a.eps)));
  }
}

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

// the fragment of k-step s out of a [128 rows][32 columns] image: rows 16 s + 8 h .. + 7 at column r
__device__ __forceinline__ bf16x8 tr_fragment(const unsigned char* lane_base, int s) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(lane_base + (16 * s) * 64));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(lane_base + (16 * s + 4) * 64));
  const s16x8 cat = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, cat);
}

__global__ void __launch_bounds__(256) head_update_kernel(HeadArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char gs[kImage];         // [128 b][32 c]
  __shared__ __attribute__((aligned(16))) unsigned char fs[4 * kImage];     // [wave][128 b][32 d]
  __shared__ int w_cnt[4];
  __shared__ float accb_s[8][kTileC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d0 = blockIdx.x * kTileD, c0 = blockIdx.y * kTileC;
  const int B = a.B, C = a.C, D = a.D;

  // ---- n: labels inside [0, C), counted with integer adds
  int cnt = 0;
  for (int b = tid; b < B; b += 256) {
    const int y = a.labels[b];
    cnt += (y >= 0 && y < C) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) w_cnt[wave] = cnt;

  // ---- this thread's pieces of a chunk: eight 16-byte pieces of f (rows f_row + 16 u), two of g (rows g_row + 64 u)
  const int f_row = tid >> 4, f_ch = tid & 15;        // columns d0 + 8 f_ch .. + 7
  const bool f_col_ok = d0 + 8 * f_ch < D;            // D % 8 == 0: a piece is inside or outside as a whole
  const int g_row = tid >> 2, g_ch = tid & 3;         // columns c0 + 8 g_ch .. + 7
  const int g_cols = min(8, C - (c0 + 8 * g_ch));     // <= 0: outside
  const int f_lds = (f_ch >> 2) * kImage + (f_ch & 3) * 16;

  uint4 fr[kFPieces], gr[kGPieces];
  auto fetch = [&](int b0) {
#pragma unroll
    for (int u = 0; u < kFPieces; ++u) {
      fr[u] = make_uint4(0u, 0u, 0u, 0u);
      const int b = b0 + f_row + 16 * u;
      if (f_col_ok && b < B) fr[u] = *reinterpret_cast<const uint4*>(a.f + (int64_t)b * a.ldf + d0 + 8 * f_ch);
    }
#pragma unroll
    for (int u = 0; u < kGPieces; ++u) {
      gr[u] = make_uint4(0u, 0u, 0u, 0u);
      const int b = b0 + g_row + 64 * u;
      if (b < B && g_cols > 0) {
        const uint16_t* src = a.g + (int64_t)b * a.ldg + c0 + 8 * g_ch;
        if (g_cols == 8) {
          gr[u] = *reinterpret_cast<const uint4*>(src);
        } else {   // the piece that straddles C: its valid elements only
          uint32_t e[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) e[j] = j < g_cols ? (uint32_t)src[j] : 0u;
          gr[u].x = e[0] | (e[1] << 16);
          gr[u].y = e[2] | (e[3] << 16);
          gr[u].z = e[4] | (e[5] << 16);
          gr[u].w = e[6] | (e[7] << 16);
        }
      }
    }
  };

  // ---- the lane's address inside an image for the transposed reads
  const int i15 = lane & 15, grp = lane >> 4;
  const int tr_off = (8 * (grp >> 1) + (i15 >> 2)) * 64 + (16 * (grp & 1) + 4 * (i15 & 3)) * 2;
  const unsigned char* g_base = gs + tr_off;
  const unsigned char* f_base = fs + wave * kImage + tr_off;

  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float accb = 0.f;                                   // class tid & 31, rows 16 (tid >> 5) .. + 15 of every chunk
  const bool bias_block = blockIdx.x == 0;

  fetch(0);
  for (int b0 = 0; b0 < B; b0 += kChunkB) {
#pragma unroll
    for (int u = 0; u < kFPieces; ++u) *reinterpret_cast<uint4*>(fs + f_lds + (f_row + 16 * u) * 64) = fr[u];
#pragma unroll
    for (int u = 0; u < kGPieces; ++u) *reinterpret_cast<uint4*>(gs + (g_row + 64 * u) * 64 + g_ch * 16) = gr[u];
    __syncthreads();
    if (b0 + kChunkB < B) fetch(b0 + kChunkB);
    if (bias_block) {
      const uint16_t* col = reinterpret_cast<const uint16_t*>(gs) + (tid >> 5) * 16 * 32 + (tid & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) accb += bf2f(col[r * 32]);
    }
#pragma unroll
    for (int s = 0; s < kChunkB / 16; ++s) {
      const bf16x8 af = tr_fragment(g_base, s);
      const bf16x8 bf = tr_fragment(f_base, s);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
    }
    tfimm_lds_reuse_barrier();
  }

  const int n = (w_cnt[0] + w_cnt[1]) + (w_cnt[2] + w_cnt[3]);
  const float inv_n = div_rn(1.0f, (float)max(n, 1));
  const bool adam = a.opt == TFIMM_HEAD_ADAM;

  // ---- the tile of w: lane = column, registers = classes
  const int d = d0 + wave * 32 + (lane & 31);
  if (d < D) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = c0 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
      if (c < C) {
        const int64_t o = (int64_t)c * a.ldw + d;
        Step e;
        e.w = a.w[o];
        e.s1 = a.s1[o];
        e.s2 = adam ? a.s2[o] : 0.f;
        head_step(a, acc[i], inv_n, e);
        a.w[o] = e.w;
        a.s1[o] = e.s1;
        if (adam) a.s2[o] = e.s2;
        a.w16[(int64_t)c * a.ldw16 + d] = (uint16_t)f2bf(e.w);
        if (a.grad_out) a.grad_out[o] = e.gd;
      }
    }
  }

  // ---- the bias: the eight partial sums of class c in ascending order, thread c of the first column tile
  if (!bias_block) return;
  accb_s[tid >> 5][tid & 31] = accb;
  __syncthreads();
  if (tid < kTileC && c0 + tid < C) {
    const int c = c0 + tid;
    accb = ((accb_s[0][tid] + accb_s[1][tid]) + (accb_s[2][tid] + accb_s[3][tid])) +
           ((accb_s[4][tid] + accb_s[5][tid]) + (accb_s[6][tid] + accb_s[7][tid]));
    Step e;
    e.w = a.bias[c];
    e.s1 = a.bias_s1[c];
    e.s2 = adam ? a.bias_s2[c] : 0.f;
    head_step(a, accb, inv_n, e);
    a.bias[c] = e.w;
    a.bias_s1[c] = e.s1;
    if (adam) a.bias_s2[c] = e.s2;
    if (a.bias_grad_out) a.bias_grad_out[c] = e.gd;
  }
}

struct Region {
  const char* name;
  uintptr_t lo, hi;   // [lo, hi) bytes; lo == 0: absent
  bool out;
};

Region region(const char* name, const void* p, int64_t rows, int64_t ld, int64_t cols, int elem, bool out) {
  Region r;
  r.name = name;
  r.lo = (uintptr_t)p;
  r.hi = p && rows > 0 ? r.lo + (uintptr_t)(((rows - 1) * ld + cols) * elem) : r.lo;
  r.out = out;
  return r;
}

}  // namespace

extern "C" int tfimm_hip_softmax_grad(const float* logits, int64_t ld, int B, int N, const int32_t* labels, void* grad, int64_t ldg,
                                      float* loss, int32_t* pred, void* stream) {
  if (!logits) TFIMM_FAIL(TFIMM_EINVAL, "softmax_grad: logits is null");
  if (!labels) TFIMM_FAIL(TFIMM_EINVAL, "softmax_grad: labels is null");
  if (!grad) TFIMM_FAIL(TFIMM_EINVAL, "softmax_grad: grad is null");
  if (!loss) TFIMM_FAIL(TFIMM_EINVAL, "softmax_grad: loss is null");
  if (!pred) TFIMM_FAIL(TFIMM_EINVAL, "softmax_grad: pred is null");
  if (((uintptr_t)logits | (uintptr_t)labels | (uintptr_t)loss | (uintptr_t)pred) & 3)
    TFIMM_FAIL(TFIMM_EINVAL, "softmax_grad: logits, labels, loss and pred hold 4-byte elements and must be 4-byte aligned");
  if ((uintptr_t)grad & 15) TFIMM_FAIL(TFIMM_EINVAL, "softmax_grad: grad must be 16-byte aligned");
  if (N < 1 || N > TFIMM_SCORE_MAX_N)
    TFIMM_FAIL(TFIMM_EINVAL, "softmax_grad: N=%d, must be in [1, TFIMM_SCORE_MAX_N = %d]", N, TFIMM_SCORE_MAX_N);
  if (ld < N) TFIMM_FAIL(TFIMM_EINVAL, "softmax_grad: ld=%lld is smaller than N=%d", (long long)ld, N);
  if (ldg < N || ldg % 8 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "softmax_grad: ldg=%lld, must be a multiple of 8 elements and at least N=%d", (long long)ldg, N);
  if (B < 0) TFIMM_FAIL(TFIMM_EINVAL, "softmax_grad: B=%d is negative", B);
  if (B == 0) return 0;
  static tfimm_once_t ready;
  if (ready.need()) {
    TFIMM_HIP_CHECK(hipFuncSetAttribute((const void*)softmax_grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TFIMM_SCORE_MAX_N * 4));
    ready.mark();
  }
  SoftmaxGradArgs a;
  a.logits = reinterpret_cast<const uint32_t*>(logits);
  a.labels = labels;
  a.grad = reinterpret_cast<uint16_t*>(grad);
  a.loss = loss;
  a.pred = pred;
  a.ld = ld;
  a.ldg = ldg;
  a.N = N;
  const size_t lds_bytes = (size_t)((N + 3) / 4 * 4) * 4;
  TFIMM_LAUNCH(softmax_grad_kernel, dim3((unsigned)B), dim3(kThreads), lds_bytes, (hipStream_t)stream, a);
  return 0;
}

extern "C" int tfimm_hip_head_update(const tfimm_head_update_desc* d, void* stream) {
  if (!d) TFIMM_FAIL(TFIMM_EINVAL, "head_update: descriptor is null");
  if (!d->f) TFIMM_FAIL(TFIMM_EINVAL, "head_update: f is null");
  if (!d->g) TFIMM_FAIL(TFIMM_EINVAL, "head_update: g is null");
  if (!d->labels) TFIMM_FAIL(TFIMM_EINVAL, "head_update: labels is null");
  if (!d->w) TFIMM_FAIL(TFIMM_EINVAL, "head_update: w is null");
  if (!d->w16) TFIMM_FAIL(TFIMM_EINVAL, "head_update: w16 is null");
  if (!d->s1) TFIMM_FAIL(TFIMM_EINVAL, "head_update: s1 is null");
  if (!d->bias) TFIMM_FAIL(TFIMM_EINVAL, "head_update: bias is null");
  if (!d->bias_s1) TFIMM_FAIL(TFIMM_EINVAL, "head_update: bias_s1 is null");
  if (d->opt != TFIMM_HEAD_SGD && d->opt != TFIMM_HEAD_ADAM)
    TFIMM_FAIL(TFIMM_EINVAL, "head_update: opt=%d, must be TFIMM_HEAD_SGD (0) or TFIMM_HEAD_ADAM (1)", d->opt);
  const bool adam = d->opt == TFIMM_HEAD_ADAM;
  if (adam && !d->s2) TFIMM_FAIL(TFIMM_EINVAL, "head_update: s2 is null (adam keeps two slots)");
  if (adam && !d->bias_s2) TFIMM_FAIL(TFIMM_EINVAL, "head_update: bias_s2 is null (adam keeps two slots)");
  if (d->B < 0) TFIMM_FAIL(TFIMM_EINVAL, "head_update: B=%d is negative", d->B);
  if (d->B > TFIMM_HEAD_MAX_B) TFIMM_FAIL(TFIMM_EUNSUP, "head_update: B=%d, more than TFIMM_HEAD_MAX_B = %d", d->B, TFIMM_HEAD_MAX_B);
  if (d->D % 8 != 0 || d->D < 8 || d->D > TFIMM_HEAD_MAX_D)
    TFIMM_FAIL(TFIMM_EUNSUP, "head_update: D=%d, must be a multiple of 8 in [8, TFIMM_HEAD_MAX_D = %d]", d->D, TFIMM_HEAD_MAX_D);
  if (d->C < 1 || d->C > TFIMM_HEAD_MAX_C)
    TFIMM_FAIL(TFIMM_EUNSUP, "head_update: C=%d, must be in [1, TFIMM_HEAD_MAX_C = %d]", d->C, TFIMM_HEAD_MAX_C);
  if (d->ldf < d->D || d->ldf % 8 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "head_update: ldf=%d, must be a multiple of 8 elements and at least D=%d", d->ldf, d->D);
  if (d->ldg < d->C || d->ldg % 8 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "head_update: ldg=%d, must be a multiple of 8 elements and at least C=%d", d->ldg, d->C);
  if (d->ldw16 < d->D || d->ldw16 % 8 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "head_update: ldw16=%d, must be a multiple of 8 elements and at least D=%d", d->ldw16, d->D);
  if (d->ldw < d->D || d->ldw % 4 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "head_update: ldw=%d, must be a multiple of 4 elements and at least D=%d", d->ldw, d->D);
  if (((uintptr_t)d->f | (uintptr_t)d->g | (uintptr_t)d->w | (uintptr_t)d->w16 | (uintptr_t)d->s1 | (uintptr_t)d->s2 |
       (uintptr_t)d->grad_out) & 15)
    TFIMM_FAIL(TFIMM_EINVAL, "head_update: f, g, w, w16, s1, s2 and grad_out must be 16-byte aligned");
  if (((uintptr_t)d->labels | (uintptr_t)d->bias | (uintptr_t)d->bias_s1 | (uintptr_t)d->bias_s2 | (uintptr_t)d->bias_grad_out) & 3)
    TFIMM_FAIL(TFIMM_EINVAL, "head_update: labels, bias, bias_s1, bias_s2 and bias_grad_out hold 4-byte elements and must be 4-byte aligned");
  if (d->B == 0) return 0;

  const int64_t B = d->B, C = d->C, D = d->D;
  const Region rs[] = {
      region("f", d->f, B, d->ldf, D, 2, false),
      region("g", d->g, B, d->ldg, C, 2, false),
      region("labels", d->labels, 1, B, B, 4, false),
      region("w", d->w, C, d->ldw, D, 4, true),
      region("w16", d->w16, C, d->ldw16, D, 2, true),
      region("s1", d->s1, C, d->ldw, D, 4, true),
      region("s2", adam ? d->s2 : nullptr, C, d->ldw, D, 4, true),
      region("bias", d->bias, 1, C, C, 4, true),
      region("bias_s1", d->bias_s1, 1, C, C, 4, true),
      region("bias_s2", adam ? d->bias_s2 : nullptr, 1, C, C, 4, true),
      region("grad_out", d->grad_out, C, d->ldw, D, 4, true),
      region("bias_grad_out", d->bias_grad_out, 1, C, C, 4, true),
  };
  constexpr int kRegions = sizeof(rs) / sizeof(rs[0]);
  for (int i = 0; i < kRegions; ++i)
    for (int j = i + 1; j < kRegions; ++j)
      if ((rs[i].out || rs[j].out) && rs[i].lo && rs[j].lo && rs[i].lo < rs[j].hi && rs[j].lo < rs[i].hi)
        TFIMM_FAIL(TFIMM_EINVAL, "head_update: %s overlaps %s", rs[j].out ? rs[j].name : rs[i].name, rs[j].out ? rs[i].name : rs[j].name);

  HeadArgs a;
  a.f = reinterpret_cast<const uint16_t*>(d->f);
  a.g = reinterpret_cast<const uint16_t*>(d->g);
  a.labels = d->labels;
  a.w = d->w;
  a.w16 = reinterpret_cast<uint16_t*>(d->w16);
  a.s1 = d->s1;
  a.s2 = d->s2;
  a.bias = d->bias;
  a.bias_s1 = d->bias_s1;
  a.bias_s2 = d->bias_s2;
  a.grad_out = d->grad_out;
  a.bias_grad_out = d->bias_grad_out;
  a.ldf = d->ldf;
  a.ldg = d->ldg;
  a.ldw = d->ldw;
  a.ldw16 = d->ldw16;
  a.B = d->B;
  a.D = d->D;
  a.C = d->C;
  a.opt = d->opt;
  a.lr = d->lr;
  a.mom = d->mom_or_one_minus_b1;
  a.omb2 = d->one_minus_b2;
  a.eps = d->eps;
  a.wd2 = d->wd2;
  const dim3 grid((unsigned)((d->D + kTileD - 1) / kTileD), (unsigned)((d->C + kTileC - 1) / kTileC));
  TFIMM_LAUNCH(head_update_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  return 0;
}

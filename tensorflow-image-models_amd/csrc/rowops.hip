// Bandwidth-bound row/pixel kernels of the tfimm forward path: input cast, LayerNorm,
// pooling, token-row broadcast, depthwise conv (+SE squeeze), SE gate, channel scaling,
// Swin patch-merge + LN.  All NHWC / (rows, channels) bf16 with 16-byte vector access
// whenever the channel count allows it.  Reference call sites: include/tfimm_hip.h.
#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include <cstdarg>
#include <cstdio>

// ---------------------------------------------------------------------------------------
// error string + misc C ABI
// ---------------------------------------------------------------------------------------
static thread_local char g_err[512] = "ok";
void tfimm_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* tfimm_hip_last_error(void) { return g_err; }
extern "C" int tfimm_hip_abi_version(void) { return TFIMM_HIP_ABI_VERSION; }
extern "C" int tfimm_hip_device_info(int device, char* name, int len) {
  hipDeviceProp_t prop;
  // a positive return is a CU count: a failure comes back as the NEGATED hipError_t (TFIMM_HIP_CHECK would return it as it is)
  const hipError_t e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) TFIMM_FAIL(-(int)e, "hipGetDeviceProperties(device %d) failed: %s", device, hipGetErrorString(e));
  if (name && len > 0) snprintf(name, (size_t)len, "%s", prop.gcnArchName);
  return prop.multiProcessorCount;
}

namespace {

constexpr int kMaxBlocks = 256 * 16;  // grid-stride cap: 16 blocks per CU

inline unsigned grid_for(int64_t work_items, int per_block) {
  int64_t b = cdiv64(work_items, per_block);
  if (b < 1) b = 1;
  if (b > kMaxBlocks) b = kMaxBlocks;
  return (unsigned)b;
}

// ---------------------------------------------------------------------------------------
// cast_input
// ---------------------------------------------------------------------------------------
template <bool IN_BF16>
__global__ void cast_input_kernel(const void* in, bf16_t* out, int64_t n_pixels, int c_in, int c_out) {
  for (int64_t px = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; px < n_pixels;
       px += (int64_t)gridDim.x * blockDim.x) {
    bf16_t* o = out + px * c_out;
    for (int c = 0; c < c_out; ++c) {
      uint32_t v = 0u;
      if (c < c_in) {
        if (IN_BF16) v = reinterpret_cast<const bf16_t*>(in)[px * c_in + c];
        else v = f2bf(reinterpret_cast<const float*>(in)[px * c_in + c]);
      }
      o[c] = (bf16_t)v;
    }
  }
}

// RGB fast path: 3 -> 4 channels, one 8-byte store per pixel
template <bool IN_BF16>
__global__ void cast_rgb4_kernel(const void* in, uint2* out, int64_t n_pixels) {
  for (int64_t px = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; px < n_pixels;
       px += (int64_t)gridDim.x * blockDim.x) {
    uint32_t r, g, b;
    if (IN_BF16) {
      const bf16_t* p = reinterpret_cast<const bf16_t*>(in) + px * 3;
      r = p[0]; g = p[1]; b = p[2];
    } else {
      const float* p = reinterpret_cast<const float*>(in) + px * 3;
      r = f2bf(p[0]); g = f2bf(p[1]); b = f2bf(p[2]);
    }
    out[px] = make_uint2(r | (g << 16), b);
  }
}

// bf16 RGB, FOUR pixels per thread: 24 contiguous input bytes as three 8-byte loads, 32 output bytes (the one-pixel kernels
// issue three 2-byte loads per pixel and reach 2.3 - 2.9 TB/s on a copy that is pure HBM traffic)
__device__ __forceinline__ void rgb4_quad(const uint2* src, uint2* o) {
  const uint2 a = src[0], b = src[1], c = src[2];          // r0 g0 | b0 r1,  g1 b1 | r2 g2,  b2 r3 | g3 b3
  o[0] = make_uint2(a.x, a.y & 0xffffu);
  o[1] = make_uint2((a.y >> 16) | (b.x << 16), b.x >> 16);
  o[2] = make_uint2(b.y, c.x & 0xffffu);
  o[3] = make_uint2((c.x >> 16) | (c.y << 16), c.y >> 16);
}
__global__ void cast_rgb4_quad_kernel(const uint2* in, uint4* out, int64_t n_quads) {
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_quads; q += (int64_t)gridDim.x * blockDim.x) {
    uint2 o[4];
    rgb4_quad(in + q * 3, o);
    out[q * 2] = make_uint4(o[0].x, o[0].y, o[1].x, o[1].y);
    out[q * 2 + 1] = make_uint4(o[2].x, o[2].y, o[3].x, o[3].y);
  }
}
// the same into a zero-bordered image: one thread per quad of INTERIOR pixels (W % 4 == 0), the border by the threads behind
__global__ void cast_pad4_quad_kernel(const uint2* in, uint2* out, int B, int H, int W, int pad_t, int pad_l, int HP, int WP) {
  const int wq = W >> 2;
  const int64_t n_quads = (int64_t)B * H * wq;
  const int64_t n_border = (int64_t)B * ((int64_t)HP * WP - (int64_t)H * W);
  const int border_row = WP - W;                            // border pixels of an interior row
  const int64_t per_image = (int64_t)HP * WP - (int64_t)H * W;
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < n_quads + n_border; id += (int64_t)gridDim.x * blockDim.x) {
    if (id < n_quads) {
      const int xq = (int)(id % wq);
      const int64_t t = id / wq;
      const int y = (int)(t % H);
      const int b = (int)(t / H);
      uint2 o[4];
      rgb4_quad(in + id * 3, o);
      uint2* dst = out + ((int64_t)b * HP + (y + pad_t)) * WP + pad_l + xq * 4;
      dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2]; dst[3] = o[3];
    } else {
      int64_t r = id - n_quads;
      const int b = (int)(r / per_image);
      r -= (int64_t)b * per_image;
      // border pixels of an image in order: pad_t full rows, then per interior row its left and right margins, then the rest
      int yp, xp;
      const int64_t top = (int64_t)pad_t * WP;
      const int64_t mid = (int64_t)H * border_row;
      if (r < top) {
        yp = (int)(r / WP); xp = (int)(r % WP);
      } else if (r < top + mid) {
        const int64_t m = r - top;
        const int row = (int)(m / border_row), k = (int)(m % border_row);
        yp = pad_t + row;
        xp = k < pad_l ? k : k + W;
      } else {
        const int64_t m = r - top - mid;
        yp = pad_t + H + (int)(m / WP); xp = (int)(m % WP);
      }
      out[((int64_t)b * HP + yp) * WP + xp] = make_uint2(0u, 0u);
    }
  }
}

// image -> zero-bordered 4-channel bf16 image (one thread per OUTPUT pixel)
template <bool IN_BF16>
__global__ void cast_pad4_kernel(const void* in, uint2* out, int B, int H, int W, int c_in, int pad_t, int pad_l,
                                 int HP, int WP) {
  const int64_t total = (int64_t)B * HP * WP;
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (int64_t)gridDim.x * blockDim.x) {
    const int xp = (int)(id % WP);
    const int64_t t = id / WP;
    const int yp = (int)(t % HP);
    const int b = (int)(t / HP);
    const int y = yp - pad_t, x = xp - pad_l;
    uint32_t c[4] = {0u, 0u, 0u, 0u};
    if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
      const int64_t px = ((int64_t)b * H + y) * W + x;
      for (int e = 0; e < c_in; ++e) {
        if (IN_BF16) c[e] = reinterpret_cast<const bf16_t*>(in)[px * c_in + e];
        else c[e] = f2bf(reinterpret_cast<const float*>(in)[px * c_in + e]);
      }
    }
    out[id] = make_uint2(c[0] | (c[1] << 16), c[2] | (c[3] << 16));
  }
}

// ---------------------------------------------------------------------------------------
// preprocess_input: uint8 image -> (v / 255 - mean[c]) / std[c] -> bf16, in the layouts of the cast kernels above.
// The three fp32 operations are the reference's (factory.py:165-167), each correctly rounded, so the result equals
// preprocessing on the host in float32 followed by cast_input, bit for bit.
// ---------------------------------------------------------------------------------------
struct NormParams {
  float mean[TFIMM_PREPROCESS_MAX_CHANNELS];
  float std[TFIMM_PREPROCESS_MAX_CHANNELS];
};

__device__ __forceinline__ uint32_t norm_u8(uint32_t v, float mean, float std) {
  return f2bf(((float)v / 255.0f - mean) / std);
}

__global__ void preprocess_kernel(const uint8_t* in, bf16_t* out, int64_t n_pixels, int c_in, int c_out, NormParams np) {
  for (int64_t px = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; px < n_pixels;
       px += (int64_t)gridDim.x * blockDim.x) {
    bf16_t* o = out + px * c_out;
    for (int c = 0; c < c_out; ++c) o[c] = (bf16_t)(c < c_in ? norm_u8(in[px * c_in + c], np.mean[c], np.std[c]) : 0u);
  }
}

// The two image kernels below look the 256 possible results per channel up in LDS (each block evaluates the formula
// once per (channel, value), 256 threads): six correctly rounded divisions per pixel would make them ALU-bound.
__device__ __forceinline__ void build_norm_lut(uint16_t (*lut)[256], int c_in, const NormParams& np) {
  for (int c = 0; c < 4; ++c)
    for (int v = threadIdx.x; v < 256; v += blockDim.x)
      lut[c][v] = c < c_in ? (uint16_t)norm_u8((uint32_t)v, np.mean[c], np.std[c]) : (uint16_t)0;
  __syncthreads();
}

// RGB fast path: a thread converts 4 pixels = 12 input bytes (three aligned dwords) -> 32 output bytes
__global__ void preprocess_rgb4_kernel(const uint8_t* in, uint2* out, int64_t n_pixels, NormParams np) {
  __shared__ uint16_t lut[4][256];
  build_norm_lut(lut, 3, np);
  const int64_t groups = n_pixels >> 2;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(in) + g * 3;
    const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
    const uint32_t by[12] = {w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u, w0 >> 24, w1 & 255u, (w1 >> 8) & 255u,
                             (w1 >> 16) & 255u, w1 >> 24, w2 & 255u, (w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24};
    uint2 o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t r = lut[0][by[3 * k]], gch = lut[1][by[3 * k + 1]], b = lut[2][by[3 * k + 2]];
      o[k] = make_uint2(r | (gch << 16), b);
    }
    uint4* q = reinterpret_cast<uint4*>(out + g * 4);
    q[0] = make_uint4(o[0].x, o[0].y, o[1].x, o[1].y);
    q[1] = make_uint4(o[2].x, o[2].y, o[3].x, o[3].y);
  }
  // the last n_pixels % 4 pixels
  const int64_t px = (groups << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (px < n_pixels) {
    const uint8_t* p = in + px * 3;
    out[px] = make_uint2((uint32_t)lut[0][p[0]] | ((uint32_t)lut[1][p[1]] << 16), (uint32_t)lut[2][p[2]]);
  }
}

// uint8 image -> zero-bordered 4-channel bf16 image (one thread per OUTPUT pixel); the border stays 0: the
// reference pads the preprocessed image
__global__ void preprocess_pad4_kernel(const uint8_t* in, uint2* out, int B, int H, int W, int c_in, int pad_t, int pad_l,
                                       int HP, int WP, NormParams np) {
  __shared__ uint16_t lut[4][256];
  build_norm_lut(lut, c_in, np);
  const int64_t total = (int64_t)B * HP * WP;
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (int64_t)gridDim.x * blockDim.x) {
    const int xp = (int)(id % WP);
    const int64_t t = id / WP;
    const int yp = (int)(t % HP);
    const int b = (int)(t / HP);
    const int y = yp - pad_t, x = xp - pad_l;
    uint32_t c[4] = {0u, 0u, 0u, 0u};
    if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
      const int64_t px = ((int64_t)b * H + y) * W + x;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < c_in) c[e] = lut[e][in[px * c_in + e]];
    }
    out[id] = make_uint2(c[0] | (c[1] << 16), c[2] | (c[3] << 16));
  }
}

// ---------------------------------------------------------------------------------------
// layernorm: one wave per row, row cached in registers (vector path) or re-read (generic)
// ---------------------------------------------------------------------------------------
template <int NCH>  // 16-byte chunks per lane: supports d <= NCH * 512
__global__ void __launch_bounds__(256) layernorm_vec_kernel(const bf16_t* x, bf16_t* y, const float* gamma,
                                                            const float* beta, int64_t rows, int d,
                                                            int64_t xs, int64_t ys, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const int nchunks = d >> 3;
  const float inv_d = 1.f / (float)d;
  for (int64_t r = wave0; r < rows; r += nwaves) {
    const uint4* xr = reinterpret_cast<const uint4*>(x + r * xs);
    float v[NCH][8];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + i * 64;
      if (c < nchunks) {
        const uint4 u = xr[c];
        unpack8(u, v[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += v[i][e];
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
      }
    }
    const float mean = wave_sum(sum) * inv_d;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + i * 64;
      if (c < nchunks) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float t = v[i][e] - mean;
          sq += t * t;
        }
      }
    }
    const float var = wave_sum(sq) * inv_d;
    const float rstd = rsqrtf(var + eps);
    uint4* yr = reinterpret_cast<uint4*>(y + r * ys);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = lane + i * 64;
      if (c < nchunks) {
        const float4 g0 = reinterpret_cast<const float4*>(gamma)[2 * c];
        const float4 g1 = reinterpret_cast<const float4*>(gamma)[2 * c + 1];
        const float4 b0 = reinterpret_cast<const float4*>(beta)[2 * c];
        const float4 b1 = reinterpret_cast<const float4*>(beta)[2 * c + 1];
        const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (v[i][e] - mean) * rstd * gg[e] + bb[e];
        yr[c] = pack8(o);
      }
    }
  }
}

// Narrow rows (d <= 256, i.e. <= 32 chunks of 16 bytes): a wave normalises 64 / LPR rows at once, LPR = 8, 16 or
// 32 lanes per row, statistics by LPR-wide butterfly reductions.  (With one row per wave a 128-channel row keeps
// 16 of 64 lanes busy: Swin-B's 56x56x128 LayerNorms ran at 1.9 TB/s.)
template <int LPR>
__global__ void __launch_bounds__(256) layernorm_narrow_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, int64_t rows, int d,
                                                               int64_t xs, int64_t ys, float eps) {
  constexpr int RPW = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int sub = lane / LPR, c = lane % LPR;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const int nchunks = d >> 3;
  const float inv_d = 1.f / (float)d;
  const bool cok = c < nchunks;
  float gg[8], bb[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { gg[e] = 0.f; bb[e] = 0.f; }
  if (cok) {
    const float4 g0 = reinterpret_cast<const float4*>(gamma)[2 * c], g1 = reinterpret_cast<const float4*>(gamma)[2 * c + 1];
    const float4 b0 = reinterpret_cast<const float4*>(beta)[2 * c], b1 = reinterpret_cast<const float4*>(beta)[2 * c + 1];
    gg[0] = g0.x; gg[1] = g0.y; gg[2] = g0.z; gg[3] = g0.w; gg[4] = g1.x; gg[5] = g1.y; gg[6] = g1.z; gg[7] = g1.w;
    bb[0] = b0.x; bb[1] = b0.y; bb[2] = b0.z; bb[3] = b0.w; bb[4] = b1.x; bb[5] = b1.y; bb[6] = b1.z; bb[7] = b1.w;
  }
  auto group_sum = [&](float v) -> float {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  };
  for (int64_t r0 = wave0 * RPW; r0 < rows; r0 += nwaves * RPW) {
    const int64_t r = r0 + sub;
    const bool ok = cok && r < rows;
    float v[8];
    uint4 u = make_uint4(0u, 0u, 0u, 0u);
    if (ok) u = reinterpret_cast<const uint4*>(x + r * xs)[c];
    unpack8(u, v);
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) sum += v[e];
    const float mean = group_sum(sum) * inv_d;
    float sq = 0.f;
    if (cok) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float t = v[e] - mean;
        sq += t * t;
      }
    }
    const float rstd = rsqrtf(group_sum(sq) * inv_d + eps);
    if (ok) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (v[e] - mean) * rstd * gg[e] + bb[e];
      reinterpret_cast<uint4*>(y + r * ys)[c] = pack8(o);
    }
  }
}

// d = 3 * LPR * 8 exactly (384, 768: DeiT-S / CaiT-S / ConvNeXt / ViT-B widths): LPR lanes per row with three
// 16-byte chunks each (c, c + LPR, c + 2 LPR), so every lane of the wave is busy -- the one-wave-per-row kernel would
// leave a third of its second chunk slots (d = 768) or whole lanes (d = 384) idle
template <int LPR>
__global__ void __launch_bounds__(256) layernorm_x3_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int64_t rows,
                                                           int64_t xs, int64_t ys, float eps) {
  constexpr int RPW = 64 / LPR;
  constexpr float inv_d = 1.f / (float)(24 * LPR);
  const int lane = threadIdx.x & 63;
  const int sub = lane / LPR, c = lane % LPR;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  float gg[3][8], bb[3][8];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int ch = c + i * LPR;
    const float4 g0 = reinterpret_cast<const float4*>(gamma)[2 * ch], g1 = reinterpret_cast<const float4*>(gamma)[2 * ch + 1];
    const float4 b0 = reinterpret_cast<const float4*>(beta)[2 * ch], b1 = reinterpret_cast<const float4*>(beta)[2 * ch + 1];
    gg[i][0] = g0.x; gg[i][1] = g0.y; gg[i][2] = g0.z; gg[i][3] = g0.w; gg[i][4] = g1.x; gg[i][5] = g1.y; gg[i][6] = g1.z; gg[i][7] = g1.w;
    bb[i][0] = b0.x; bb[i][1] = b0.y; bb[i][2] = b0.z; bb[i][3] = b0.w; bb[i][4] = b1.x; bb[i][5] = b1.y; bb[i][6] = b1.z; bb[i][7] = b1.w;
  }
  auto group_sum = [&](float v) -> float {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  };
  for (int64_t r0 = wave0 * RPW; r0 < rows; r0 += nwaves * RPW) {
    const int64_t r = r0 + sub;
    const bool ok = r < rows;
    float v[3][8];
    uint4 u[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) u[i] = ok ? reinterpret_cast<const uint4*>(x + r * xs)[c + i * LPR] : make_uint4(0u, 0u, 0u, 0u);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      unpack8(u[i], v[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += v[i][e];
    }
    const float mean = group_sum(sum) * inv_d;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float t = v[i][e] - mean;
        sq += t * t;
      }
    const float rstd = rsqrtf(group_sum(sq) * inv_d + eps);
    if (ok) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (v[i][e] - mean) * rstd * gg[i][e] + bb[i][e];
        reinterpret_cast<uint4*>(y + r * ys)[c + i * LPR] = pack8(o);
      }
    }
  }
}

__global__ void __launch_bounds__(256) layernorm_generic_kernel(const bf16_t* x, bf16_t* y, const float* gamma,
                                                                const float* beta, int64_t rows, int d,
                                                                int64_t xs, int64_t ys, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const float inv_d = 1.f / (float)d;
  for (int64_t r = wave0; r < rows; r += nwaves) {
    const bf16_t* xr = x + r * xs;
    float sum = 0.f;
    for (int c = lane; c < d; c += 64) sum += bf2f(xr[c]);
    const float mean = wave_sum(sum) * inv_d;
    float sq = 0.f;
    for (int c = lane; c < d; c += 64) {
      const float t = bf2f(xr[c]) - mean;
      sq += t * t;
    }
    const float rstd = rsqrtf(wave_sum(sq) * inv_d + eps);
    bf16_t* yr = y + r * ys;
    for (int c = lane; c < d; c += 64)
      yr[c] = (bf16_t)f2bf((bf2f(xr[c]) - mean) * rstd * gamma[c] + beta[c]);
  }
}

// ---------------------------------------------------------------------------------------
// maxpool (zero padding participates in the max, see header)
// ---------------------------------------------------------------------------------------
__global__ void maxpool_vec_kernel(const bf16_t* x, bf16_t* y, int B, int H, int W, int C, int k, int stride,
                                   int pad, int OH, int OW) {
  const int cg = C >> 3;
  const int64_t total = (int64_t)B * OH * OW * cg;
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total;
       id += (int64_t)gridDim.x * blockDim.x) {
    const int c8 = (int)(id % cg);
    int64_t t = id / cg;
    const int ox = (int)(t % OW); t /= OW;
    const int oy = (int)(t % OH);
    const int b = (int)(t / OH);
    float m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = -3.0e38f;
    for (int ky = 0; ky < k; ++ky) {
      const int iy = oy * stride - pad + ky;
      for (int kx = 0; kx < k; ++kx) {
        const int ix = ox * stride - pad + kx;
        float v[8];
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
          const uint4 u = *reinterpret_cast<const uint4*>(x + (((int64_t)b * H + iy) * W + ix) * C + c8 * 8);
          unpack8(u, v);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], v[e]);
      }
    }
    *reinterpret_cast<uint4*>(y + (((int64_t)b * OH + oy) * OW + ox) * C + c8 * 8) = pack8(m);
  }
}

__global__ void maxpool_generic_kernel(const bf16_t* x, bf16_t* y, int B, int H, int W, int C, int k, int stride,
                                       int pad, int OH, int OW) {
  const int64_t total = (int64_t)B * OH * OW * C;
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total;
       id += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(id % C);
    int64_t t = id / C;
    const int ox = (int)(t % OW); t /= OW;
    const int oy = (int)(t % OH);
    const int b = (int)(t / OH);
    float m = -3.0e38f;
    for (int ky = 0; ky < k; ++ky)
      for (int kx = 0; kx < k; ++kx) {
        const int iy = oy * stride - pad + ky, ix = ox * stride - pad + kx;
        float v = 0.f;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
          v = bf2f(x[(((int64_t)b * H + iy) * W + ix) * C + c]);
        m = fmaxf(m, v);
      }
    y[id] = (bf16_t)f2bf(m);
  }
}

// ---------------------------------------------------------------------------------------
// mean over rows: block = (image, 64-channel group...) -- one thread per channel, coalesced
// across channels, rows split over blockDim.y then reduced through LDS.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) mean_rows_kernel(const bf16_t* x, void* y, int B, int R, int C, int out_f32) {
  __shared__ float part[4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int cgroups = (C + 63) / 64;
  for (int blk = blockIdx.x; blk < B * cgroups; blk += gridDim.x) {
    const int b = blk / cgroups, c = (blk - b * cgroups) * 64 + cx;
    float s = 0.f;
    if (c < C) {
      const bf16_t* p = x + (int64_t)b * R * C + c;
      for (int r = ry; r < R; r += 4) s += bf2f(p[(int64_t)r * C]);
    }
    part[ry][cx] = s;
    __syncthreads();
    if (ry == 0 && c < C) {
      const float m = (part[0][cx] + part[1][cx] + part[2][cx] + part[3][cx]) / (float)R;
      if (out_f32) reinterpret_cast<float*>(y)[(int64_t)b * C + c] = m;
      else reinterpret_cast<bf16_t*>(y)[(int64_t)b * C + c] = (bf16_t)f2bf(m);
    }
    __syncthreads();
  }
}

// C % 8 == 0, 16-byte aligned rows: a lane sums 8 channels with 16-byte loads (1 KB of a row per wave instruction
// instead of 128 bytes), the block's 4 waves split the rows
__global__ void __launch_bounds__(256) mean_rows_vec_kernel(const bf16_t* x, void* y, int B, int R, int C, int out_f32) {
  __shared__ float part[4][64][8];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int cgroups = (C + 511) / 512;
  for (int blk = blockIdx.x; blk < B * cgroups; blk += gridDim.x) {
    const int b = blk / cgroups, c = (blk - b * cgroups) * 512 + cx * 8;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c < C) {
      const bf16_t* p = x + (int64_t)b * R * C + c;
      for (int r = ry; r < R; r += 4) {
        float v[8];
        unpack8(*reinterpret_cast<const uint4*>(p + (int64_t)r * C), v);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += v[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[ry][cx][e] = s[e];
    __syncthreads();
    if (ry == 0 && c < C) {
      float m[8];
      const float inv = 1.f / (float)R;
#pragma unroll
      for (int e = 0; e < 8; ++e) m[e] = (part[0][cx][e] + part[1][cx][e] + part[2][cx][e] + part[3][cx][e]) * inv;
      if (out_f32) {
        float4* o = reinterpret_cast<float4*>(reinterpret_cast<float*>(y) + (int64_t)b * C + c);
        o[0] = make_float4(m[0], m[1], m[2], m[3]);
        o[1] = make_float4(m[4], m[5], m[6], m[7]);
      } else {
        *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(y) + (int64_t)b * C + c) = pack8(m);
      }
    }
    __syncthreads();
  }
}

__global__ void bcast_rows_kernel(const bf16_t* src, bf16_t* dst, int B, int n_rows, int d, int dst_rpi) {
  const int64_t total = (int64_t)B * n_rows * d;
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total;
       id += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(id % d);
    const int64_t t = id / d;
    const int r = (int)(t % n_rows);
    const int64_t b = t / n_rows;
    dst[(b * dst_rpi + r) * d + c] = src[(int64_t)r * d + c];
  }
}

// ---------------------------------------------------------------------------------------
// depthwise conv: thread = (output pixel, 8-channel group); weights fp32 [k*k][C]
// ---------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(256) dwconv_kernel(const bf16_t* x, const float* w, const float* bias, bf16_t* y,
                                                     tfimm_sq_t* sum_out, int B, int H, int W, int C, int k, int stride,
                                                     int pad_t, int pad_l, int OH, int OW, int act) {
  constexpr int G = VEC ? 8 : 1;
  const int cg = VEC ? (C >> 3) : C;
  const int64_t total = (int64_t)B * OH * OW * cg;
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total;
       id += (int64_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(id % cg) * G;
    int64_t t = id / cg;
    const int ox = (int)(t % OW); t /= OW;
    const int oy = (int)(t % OH);
    const int b = (int)(t / OH);
    float acc[G];
#pragma unroll
    for (int e = 0; e < G; ++e) acc[e] = bias ? bias[c0 + e] : 0.f;
    for (int ky = 0; ky < k; ++ky) {
      const int iy = oy * stride - pad_t + ky;
      if ((unsigned)iy >= (unsigned)H) continue;
      for (int kx = 0; kx < k; ++kx) {
        const int ix = ox * stride - pad_l + kx;
        if ((unsigned)ix >= (unsigned)W) continue;
        const bf16_t* xp = x + (((int64_t)b * H + iy) * W + ix) * C + c0;
        const float* wp = w + (int64_t)(ky * k + kx) * C + c0;
        if constexpr (VEC) {
          float v[8];
          unpack8(*reinterpret_cast<const uint4*>(xp), v);
          const float4 w0 = reinterpret_cast<const float4*>(wp)[0];
          const float4 w1 = reinterpret_cast<const float4*>(wp)[1];
          const float ww[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += v[e] * ww[e];
        } else {
          acc[0] += bf2f(xp[0]) * wp[0];
        }
      }
    }
#pragma unroll
    for (int e = 0; e < G; ++e) acc[e] = apply_act(acc[e], act);
    bf16_t* yp = y + (((int64_t)b * OH + oy) * OW + ox) * C + c0;
    if constexpr (VEC) {
      const uint4 u = pack8(acc);
      *reinterpret_cast<uint4*>(yp) = u;
      if (sum_out) {
        float r[8];
        unpack8(u, r);  // squeeze sees the stored (bf16-rounded) activations
#pragma unroll
        for (int e = 0; e < 8; ++e) sq_add(sum_out + (int64_t)b * C + c0 + e, sq_from_float(r[e]));
      }
    } else {
      const uint32_t h = f2bf(acc[0]);
      yp[0] = (bf16_t)h;
      if (sum_out) sq_add(sum_out + (int64_t)b * C + c0, sq_from_float(bf2f(h)));
    }
  }
}

// Strip kernel (C % CV == 0, k/stride known at compile time): a thread owns CV (8 or 4) channels x PX
// horizontally adjacent output pixels.  Per filter row it loads each needed input column ONCE
// (16 / 8 B) and feeds every (pixel, tap) pair that touches it, with that row's weights held in
// registers -- k*k/PX-fold fewer loads than one-output-per-thread.  Consecutive lanes own
// consecutive channel groups, so every load/store instruction covers contiguous NHWC bytes.
// Everything is branch-free: out-of-image rows/columns are clamped addresses + zeroed values, the
// activation uses wave-uniform parameters.  The SE squeeze (sum of the stored, bf16-rounded outputs
// per image and channel) is reduced in LDS ([CV][C/CV], conflict-free ds_add) and leaves the block
// as ONE global atomic per channel.
template <int CV>
struct dwvec;
template <>
struct dwvec<8> { typedef uint4 type; };
template <>
struct dwvec<4> { typedef uint2 type; };

template <int CV>
__device__ __forceinline__ void dw_unpack(const typename dwvec<CV>::type& u, float* f) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&u);
#pragma unroll
  for (int i = 0; i < CV / 2; ++i) {
    f[2 * i] = bf2f(w[i] & 0xffffu);
    f[2 * i + 1] = bf2f(w[i] >> 16);
  }
}

template <int K, int S, int PX, int CV>
__global__ void __launch_bounds__(256) dwconv_strip_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, bf16_t* __restrict__ y,
                                                           tfimm_sq_t* sum_out, int H, int W, int C, int pad_t, int pad_l,
                                                           int OH, int OW, int act) {
  typedef typename dwvec<CV>::type vec_t;
  extern __shared__ tfimm_sq_t lsum[];  // [CV][cgs]
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int cgs = C / CV;
  const int sx = (OW + PX - 1) / PX;
  const int items = OH * sx * cgs;
  const ActParams actp = make_act(act);
  if (sum_out) {
    for (int i = tid; i < CV * cgs; i += 256) lsum[i] = 0;
    __syncthreads();
  }
  constexpr int COLS = (PX - 1) * S + K;
  for (int item = blockIdx.x * 256 + tid; item < items; item += gridDim.x * 256) {
    const int cg = item % cgs;
    const int t = item / cgs;
    const int sxi = t % sx, oy = t / sx;
    const int ox0 = sxi * PX, c0 = cg * CV;
    // channel PAIRS throughout (accumulators, taps and pixels are tfimm_f32x2 of channels 2i, 2i+1): written with scalars, the
    // SLP vectoriser paired registers of different origin and bridged them with operand selects (v_pk_fma_f32 ... op_sel:[0,1,0]),
    // which gfx950 gets wrong next to MFMA waves of another kernel (tools/isa_lint.py; profiles/NOTES_r04.md section 1)
    tfimm_f32x2 acc[PX][CV / 2];
#pragma unroll
    for (int i = 0; i < CV / 2; ++i) {
      const tfimm_f32x2 be = bias ? *reinterpret_cast<const tfimm_f32x2*>(bias + c0 + 2 * i) : tfimm_f32x2{0.f, 0.f};
#pragma unroll
      for (int px = 0; px < PX; ++px) acc[px][i] = be;
    }
    const int ixb = ox0 * S - pad_l;
    const bf16_t* ximg = x + (size_t)b * H * W * C + c0;
#pragma unroll 1
    for (int ky = 0; ky < K; ++ky) {
      const int iy = oy * S - pad_t + ky;
      const bool rok = (unsigned)iy < (unsigned)H;
      const int iyc = rok ? iy : 0;
      tfimm_f32x2 wr[K][CV / 2];
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const float* wp = w + (size_t)(ky * K + kx) * C + c0;
#pragma unroll
        for (int q = 0; q < CV / 4; ++q) {
          const float4 w4 = *reinterpret_cast<const float4*>(wp + 4 * q);
          wr[kx][2 * q] = tfimm_f32x2{w4.x, w4.y};
          wr[kx][2 * q + 1] = tfimm_f32x2{w4.z, w4.w};
        }
      }
      const bf16_t* xrow = ximg + (size_t)iyc * W * C;
      vec_t raw[COLS];
#pragma unroll
      for (int col = 0; col < COLS; ++col) {
        const int ix = ixb + col;
        const int ixc = min(max(ix, 0), W - 1);
        raw[col] = *reinterpret_cast<const vec_t*>(xrow + (size_t)ixc * C);
      }
#pragma unroll
      for (int col = 0; col < COLS; ++col) {
        const int ix = ixb + col;
        const float m = (rok && (unsigned)ix < (unsigned)W) ? 1.f : 0.f;
        const tfimm_f32x2 m2 = {m, m};
        float vs[CV];
        dw_unpack<CV>(raw[col], vs);
        tfimm_f32x2 v[CV / 2];
#pragma unroll
        for (int i = 0; i < CV / 2; ++i) v[i] = tfimm_f32x2{vs[2 * i], vs[2 * i + 1]} * m2;
#pragma unroll
        for (int px = 0; px < PX; ++px) {
          const int kx = col - px * S;   // compile-time after unrolling
          if (kx >= 0 && kx < K) {
#pragma unroll
            for (int i = 0; i < CV / 2; ++i) acc[px][i] = __builtin_elementwise_fma(v[i], wr[kx][i], acc[px][i]);
          }
        }
      }
    }
    float tot[CV];
#pragma unroll
    for (int e = 0; e < CV; ++e) tot[e] = 0.f;
    bf16_t* yrow = y + ((size_t)((size_t)b * OH + oy) * OW) * C + c0;
#pragma unroll
    for (int px = 0; px < PX; ++px) {
      uint32_t pk[CV / 2];
#pragma unroll
      for (int i = 0; i < CV / 2; ++i) pk[i] = pack_bf2(act1(acc[px][i][0], actp), act1(acc[px][i][1], actp));
      const bool ok = ox0 + px < OW;
      if (ok) {
        vec_t u;
        uint32_t* uw = reinterpret_cast<uint32_t*>(&u);
#pragma unroll
        for (int i = 0; i < CV / 2; ++i) uw[i] = pk[i];
        *reinterpret_cast<vec_t*>(yrow + (size_t)(ox0 + px) * C) = u;
      }
      const float m = ok ? 1.f : 0.f;   // the squeeze sees the stored (bf16-rounded) activations
#pragma unroll
      for (int i = 0; i < CV / 2; ++i) {
        tot[2 * i] += m * bf2f(pk[i] & 0xffffu);
        tot[2 * i + 1] += m * bf2f(pk[i] >> 16);
      }
    }
    if (sum_out) {
#pragma unroll
      for (int e = 0; e < CV; ++e) sq_add(&lsum[e * cgs + cg], sq_from_float(tot[e]));
    }
  }
  if (sum_out) {
    __syncthreads();
    for (int c = tid; c < C; c += 256) sq_add(sum_out + (size_t)b * C + c, lsum[(c % CV) * cgs + (c / CV)]);
  }
}

// ---------------------------------------------------------------------------------------
// Row-stationary depthwise kernel (k = 3 / 5 / 7 at stride 1, k = 3 / 5 at stride 2; EfficientNet, ConvNeXt).
// 25 / 49 MACs per output make k = 5 / 7 VALU-bound (12 / 24 flop per HBM byte), so the kernel is
// organised around packed FMAs with no register traffic besides them.  A thread owns ONE channel pair and PX = 4
// adjacent output columns and marches down a row segment.  Every INPUT row is loaded once ((PX - 1) S + K pixel pairs,
// requested one row ahead) and scattered into the ceil(K / S) output rows it contributes to: that many accumulator
// rows (x PX fp32 pairs) stay in registers, the row whose last contribution just arrived is stored and reset.  The
// loop is unrolled over the S * ceil(K / S) phases of that rotation, so accumulator slots are compile-time indices -- the
// sliding fp32 window this kernel replaced needed K x (PX + K - 1) pairs and register moves per row, which limited
// it to k <= 5.  Filter taps: LDS [K*K][channel pair], one conflict-free 8-byte read per
// (tap, thread) feeding PX packed FMAs.
// ---------------------------------------------------------------------------------------
// channel pairs per workgroup (CPB) and with it column strips per workgroup (256 / CPB): the split of the 256
// threads that wastes the fewest on channel-tile, strip-group and rounding remainders
// k <= 3 (9 MACs per output: the launch follows its memory traffic, not its arithmetic): a tile whose run of channels per pixel is
// a whole number of 64-byte segments (16 pairs) is worth more than the last few percent of busy threads -- C = 672 at 24 x 24
// with tiles of 85 pairs (340-byte runs that start anywhere) 118 us, with 112 or 128 pairs 97 us, C = 2688 at 12 x 12 111 -> 94 us
// with 80 pairs; the k = 5 / 7 launches, bound by their multiply-adds, lose with any tile but the fullest (tools/dw_diag.py,
// TFIMM_DW_CPB / TFIMM_DW_ALIGN_BONUS).  The bonus (20 % of the thread utilisation) applies to tiles of at least 80 pairs.
static int dw_rows_pairs_per_block(int cps, int sx, int k) {
  static const double bonus = getenv("TFIMM_DW_ALIGN_BONUS") ? atof(getenv("TFIMM_DW_ALIGN_BONUS")) : 0.2;
  int best = cps < 128 ? cps : 128;
  double best_u = -1.0;
  for (int c = 8; c <= 128 && c <= cps; ++c) {
    const int spb = 256 / c;
    const int ct = (cps + c - 1) / c, sg = (sx + spb - 1) / spb;
    double u = ((double)cps / (ct * c)) * ((double)sx / (sg * spb)) * (c * spb / 256.0);
    if (k <= 3 && (c % 16) == 0 && c >= 80) u *= 1.0 + bonus;      // (short runs lose: C = 144 with tiles of 32 pairs 425 us against 340)
    if (u > best_u + 1e-9 || (u > best_u - 1e-9 && c > best)) { best_u = u; best = c; }
  }
  return best;
}

// TFIMM_DW_ABLATE (probe builds only, tools/dw_diag.sh; 0 in the product): 1 no activation, 2 no multiply-adds, 4 no output
// stores, 8 filter taps from registers instead of LDS -- which part of a row's work the launch time follows
#ifndef TFIMM_DW_ABLATE
#define TFIMM_DW_ABLATE 0
#endif
// ACT >= 0: that TFIMM_ACT_* with its parameters folded into the instructions; ACT < 0: `act` from the arguments
template <int K, int S, int PX, int DEPTH, int ACT>
__global__ void __launch_bounds__(256) dwconv_rows_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, bf16_t* __restrict__ y,
                                                      tfimm_sq_t* sum_out, int H, int W, int C, int pad_t, int pad_l, int OH, int OW, int act,
                                                      int rows_per_seg, int nseg, int CPB) {
  constexpr int COLS = (PX - 1) * S + K;
  constexpr int NSLOT = (K + S - 1) / S;          // output rows with contributions pending
  constexpr int PERIOD = S * NSLOT;              // input rows per full rotation of the slots
  extern __shared__ tfimm_f32x2 dw7_lds[];       // [K*K][CPB] filter taps of this workgroup's channel pairs, then [2 CPB] squeeze sums (64-bit fixed point)
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int cps = C / 2;                          // channel pairs
  const int SPB = 256 / CPB;                      // column strips per workgroup
  const int ctiles = (cps + CPB - 1) / CPB;
  const int sx = (OW + PX - 1) / PX;
  const int sgroups = (sx + SPB - 1) / SPB;
  int bid = blockIdx.x;
  const int ct = bid % ctiles; bid /= ctiles;
  const int sg = bid % sgroups;
  const int seg = bid / sgroups;                  // row segment: uniform over the workgroup
  const int cpl = tid % CPB, sl = tid / CPB;
  const int cp = ct * CPB + cpl;
  const int strip = sg * SPB + sl;
  const bool live = sl < SPB && cp < cps && strip < sx;
  const ActParams actp = make_act(ACT >= 0 ? ACT : act);

  for (int i = tid; i < K * K * CPB; i += 256) {
    const int tap = i / CPB, c = i - tap * CPB;
    const int ch = (ct * CPB + c) * 2;
    dw7_lds[i] = ch < C ? tfimm_f32x2{w[(size_t)tap * C + ch], w[(size_t)tap * C + ch + 1]} : tfimm_f32x2{0.f, 0.f};
  }
  tfimm_sq_t* lsum = reinterpret_cast<tfimm_sq_t*>(dw7_lds + K * K * CPB);
  if (sum_out && tid < 2 * CPB) lsum[tid] = 0;
  __syncthreads();
  // squeeze sums: every finished output row converts ITS partial (four pixels, fixed order) to fixed point and the thread adds
  // integers from there on -- the sum no longer depends on how many rows a thread marches, i.e. on the row segmentation the
  // launch picks from the batch size (a thread-long fp32 partial made batch-2 and batch-256 forwards of EfficientNet-B4 differ
  // in the last bits of the squeeze, and through bf16 roundings further down by up to 1e-2 of the logit range)
  long long tot0 = 0, tot1 = 0;                     // 2^-16 units
  if (live) {

  const int c0 = cp * 2;
  const int ox0 = strip * PX;
  const int oy0 = seg * rows_per_seg, oy1 = min(OH, oy0 + rows_per_seg);
  const int r_begin = oy0 * S - pad_t, r_end = (oy1 - 1) * S + K - pad_t;   // input rows [r_begin, r_end) touch this segment
  const tfimm_f32x2 bias2 = bias ? tfimm_f32x2{bias[c0], bias[c0 + 1]} : tfimm_f32x2{0.f, 0.f};
  // Row loads go through a buffer descriptor that covers exactly ONE image row (W C elements): a column left or right of
  // the image has a byte offset that is negative (huge as unsigned) or >= the row's size and the load returns 0 -- no column
  // masks (8 VGPRs and a packed multiply per column and row), no clamped offsets: 118 -> 97 VGPRs at k = 5, 93 -> 79 at k = 3.
  // (Measured neutral on EfficientNet-B4 / ConvNeXt-T within +-1 %, like two rows in flight at the now equal occupancy: the
  // wave-state counters show these kernels parked 44-53 % of their wave cycles with the VALU 64 % busy, and neither more
  // resident waves nor fewer VALU instructions moved them.)
  const bf16_t* ximg = x + (size_t)b * H * W * C;            // wave-uniform
  const unsigned row_bytes = (unsigned)W * (unsigned)C * 2u;
  int voff[COLS];
#pragma unroll
  for (int col = 0; col < COLS; ++col) voff[col] = ((ox0 * S - pad_l + col) * C + c0) * 2;
  // Every VMEM instruction of the row loop is issued UNCONDITIONALLY and in a fixed order (loads of the row DEPTH ahead, then --
  // in the phases that finish an output row -- its PX stores): what must not touch memory goes through a descriptor with zero
  // records (a row beyond the segment, an output row of a neighbour segment) or has an offset beyond its row (columns right
  // of the image).  VMEM operations retire in issue order on gfx9 (one vmcnt for loads AND stores), and with loads or stores
  // inside branches hipcc cannot count them: the round-4 kernel waited `vmcnt(0)` at the top of every row, i.e. for the
  // write acknowledgements of the previous row's stores (tools/dw_diag.sh: without the stores the k = 3 launches of
  // EfficientNet-B4 ran 127 -> 71 us, the k = 5 ones 193 -> 160).  Now the wait in front of a row's first multiply leaves the
  // younger stores in flight (s_waitcnt vmcnt(PX) in the steady state).
  auto load_row = [&](int r, uint32_t* dst, bool valid) __attribute__((always_inline)) {
    const bf16_t* xrow = ximg + (size_t)min(max(r, 0), H - 1) * W * C;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(xrow), 0, valid ? (int)row_bytes : 0, 0x00020000);
#pragma unroll
    for (int col = 0; col < COLS; ++col) dst[col] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, voff[col], 0, 0);
  };
  // output: a descriptor per output row (OW C elements); column ox0 + px >= OW has an offset beyond it
  const unsigned orow_bytes = (unsigned)OW * (unsigned)C * 2u;
  int ooff[PX];
#pragma unroll
  for (int px = 0; px < PX; ++px) ooff[px] = ((ox0 + px) * C + c0) * 2;
  auto store_row = [&](int oy, const uint32_t* pk, bool valid) __attribute__((always_inline)) {
    bf16_t* yrow = y + ((size_t)((size_t)b * OH + min(max(oy, 0), OH - 1)) * OW) * C;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(yrow, 0, valid ? (int)orow_bytes : 0, 0x00020000);
#pragma unroll
    for (int px = 0; px < PX; ++px) __builtin_amdgcn_raw_buffer_store_b32(pk[px], rs, ooff[px], 0, 0);
  };
  tfimm_f32x2 acc[NSLOT][PX];
#pragma unroll
  for (int j = 0; j < NSLOT; ++j)
#pragma unroll
    for (int px = 0; px < PX; ++px) acc[j][px] = bias2;
  // two input rows in flight: one row's FMAs + activation (a few hundred cycles per wave) do not cover an HBM round trip at
  // 4-5 waves per SIMD, two do.  The phase loop is unrolled over lcm(PERIOD, 2) so the buffer index is a compile-time constant.
  constexpr int UNR = (DEPTH == 1 || PERIOD % 2 == 0) ? PERIOD : 2 * PERIOD;
  uint32_t raw[DEPTH][COLS];
  load_row(r_begin, raw[0], true);
  if (DEPTH == 2) load_row(r_begin + 1, raw[DEPTH - 1], r_begin + 1 < r_end);
  {
    // PX stores that write nothing, behind the first loads: on EVERY path into the loop the row's loads now have at least PX
    // younger VMEM operations, which is what lets the compiler's wait at the loop head be vmcnt(PX) instead of vmcnt(0)
    const uint32_t zero[PX] = {};
    store_row(0, zero, false);
  }
  const tfimm_f32x2* wl = dw7_lds + cpl;

  for (int rb = r_begin; rb < r_end; rb += UNR) {
#pragma unroll
    for (int ph2 = 0; ph2 < UNR; ++ph2) {
      const int ph = ph2 % PERIOD;
      const int r = rb + ph2;
      const bool row_live = r < r_end;                 // wave-uniform; rows beyond the segment only run their (empty) VMEM
      tfimm_f32x2 in[COLS];       // (rows outside the image are never multiplied: see the branch below)
#pragma unroll
      for (int col = 0; col < COLS; ++col)
        in[col] = tfimm_f32x2{__uint_as_float(raw[ph2 % DEPTH][col] << 16), __uint_as_float(raw[ph2 % DEPTH][col] & 0xffff0000u)};
      load_row(r + DEPTH, raw[ph2 % DEPTH], r + DEPTH < r_end);   // DEPTH rows ahead, into the buffer just consumed
      if (row_live && (unsigned)r < (unsigned)H) {
        // input row r = r_begin + ph (mod PERIOD) feeds output row oy = (r + pad_t - ky) / S for the ky of its
        // parity class (r_begin + pad_t is a multiple of S); oy lives in slot ((ph - ky) / S) mod NSLOT
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
          if ((ky % S) != (ph % S)) continue;      // compile time
          const int oy = (r + pad_t - ky) / S;
          if (r + pad_t - ky >= 0 && oy >= oy0 && oy < oy1) {   // wave-uniform: other rows belong to a neighbour segment
            const int slot = ((((ph - ky) / S) % NSLOT) + NSLOT) % NSLOT;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
              const tfimm_f32x2 wv = (TFIMM_DW_ABLATE & 8) ? tfimm_f32x2{bias2.x + (float)(ky * K + kx), bias2.y} : wl[(ky * K + kx) * CPB];
#pragma unroll
              for (int px = 0; px < PX; ++px) {
                if (TFIMM_DW_ABLATE & 2) { if (kx == 0 && ky == 0) acc[slot][px] += in[px * S + kx] * wv; }
                else acc[slot][px] = __builtin_elementwise_fma(in[px * S + kx], wv, acc[slot][px]);
              }
            }
          }
        }
      }
      // the output row whose LAST contribution (ky = K - 1) came from this input row is complete
      if (((ph % S) == ((K - 1) % S))) {
        const int dslot = ((((ph - (K - 1)) / S) % NSLOT) + NSLOT) % NSLOT;
        const int oyd = (r + pad_t - (K - 1)) / S;
        const bool row_done = row_live && r + pad_t - (K - 1) >= 0 && oyd >= oy0 && oyd < oy1;     // wave-uniform
        static_assert(PX == 4, "the activation runs on four packed pairs");
        uint32_t pk[PX] = {};
        if (row_done) {            // VALU only: the stores below are issued either way
          tfimm_f32x2 av[4] = {acc[dslot][0], acc[dslot][1], acc[dslot][2], acc[dslot][3]};
          if (!(TFIMM_DW_ABLATE & 1)) act8p(av, actp);            // packed (v_pk_*): the scalar form cost ~33 issue slots per pair for swish, this ~21
          tfimm_f32x2 rowtot = {0.f, 0.f};
#pragma unroll
          for (int px = 0; px < PX; ++px) {
            pk[px] = pack_bf2(av[px][0], av[px][1]);
            // the squeeze sees the stored (bf16-rounded) activations of the columns inside the image
            const uint32_t seen = (ox0 + px < OW) ? pk[px] : 0u;
            rowtot += tfimm_f32x2{__uint_as_float(seen << 16), __uint_as_float(seen & 0xffff0000u)};
          }
          if (sum_out) {               // (wave-uniform) 64-bit conversion: a 32-bit one saturates silently at |row partial| = 32768
            rowtot *= 65536.f;
            tot0 += __float2ll_rn(rowtot.x);
            tot1 += __float2ll_rn(rowtot.y);
          }
        }
        store_row(oyd, pk, row_done && !(TFIMM_DW_ABLATE & 4));
#pragma unroll
        for (int px = 0; px < PX; ++px) acc[dslot][px] = bias2;
      }
    }
  }
  }
  if (sum_out) {
    if (live) {
      sq_add(&lsum[2 * cpl], (tfimm_sq_t)(tot0 * 16));         // 2^-16 -> 2^-20 units
      sq_add(&lsum[2 * cpl + 1], (tfimm_sq_t)(tot1 * 16));
    }
    __syncthreads();
    if (tid < 2 * CPB && ct * CPB * 2 + tid < C) sq_add(sum_out + (size_t)b * C + ct * CPB * 2 + tid, lsum[tid]);
  }
}

template <int K, int S>
static int launch_dwconv_rows(const bf16_t* x, const float* w, const float* bias, bf16_t* y, tfimm_sq_t* sum_out, int B, int H,
                              int W, int C, int pad_t, int pad_l, int OH, int OW, int act, hipStream_t st) {
  constexpr int PX = 4;
  const int cps = C / 2;
  const int sx = (OW + PX - 1) / PX;
  static const int cpb_env = getenv("TFIMM_DW_CPB") ? atoi(getenv("TFIMM_DW_CPB")) : 0;      // (probe: force the channel-pair tile)
  const int CPB = (cpb_env >= 8 && cpb_env <= 128 && cpb_env <= cps) ? cpb_env : dw_rows_pairs_per_block(cps, sx, K), SPB = 256 / CPB;
  const int ctiles = (cps + CPB - 1) / CPB;
  const int sgroups = (sx + SPB - 1) / SPB;
  // row segments cost K - S halo rows each: split only until every CU has its three resident workgroups
  int nseg = 1;
  while (OH / (nseg + 1) >= 14 && (int64_t)B * ctiles * sgroups * nseg < 256 * 3) ++nseg;
  const int rows_per_seg = (OH + nseg - 1) / nseg;
  nseg = (OH + rows_per_seg - 1) / rows_per_seg;
  const int64_t gx = (int64_t)ctiles * sgroups * nseg;
  if (gx > 0x7fffffffLL) TFIMM_FAIL(TFIMM_EINVAL, "dwconv: grid too large");
  const size_t lds = (size_t)(K * K + 2) * CPB * sizeof(tfimm_f32x2);      // taps + 2 CPB fixed-point squeeze sums
  // input rows in flight per thread.  Round 2: two measured slower than one (EfficientNet-B4 depthwise 4.68 -> 5.36 ms).  With the
  // row loop's VMEM countable (round 5: the loop no longer drains its stores at every row) the second row pays for k = 5:
  // 266 -> 256, 194 -> 183, 84.5 -> 81.4 us on the three k = 5 shapes of EfficientNet-B4, k = 3 unchanged (tools/dw_diag.py,
  // interleaved on one box).  TFIMM_DW_DEPTH=1 / 2 forces either (swish flavour only).
  static const int depth_env = getenv("TFIMM_DW_DEPTH") ? atoi(getenv("TFIMM_DW_DEPTH")) : 0;
  const int depth = depth_env ? depth_env : (K == 5 ? 2 : 1);
  auto go = [&](auto kern) -> int {
    static tfimm_once_t attr_done;       // one flag set per kernel instantiation (generic lambda)
    if (attr_done.need()) {
      TFIMM_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
      attr_done.mark();
    }
    TFIMM_LAUNCH(kern, dim3((unsigned)gx, (unsigned)B), dim3(256), lds, st, x, w, bias, y, sum_out, H, W, C, pad_t, pad_l, OH, OW, act,
                 rows_per_seg, nseg, CPB);
    return 0;
  };
  if (act == TFIMM_ACT_SWISH) return depth == 2 ? go(dwconv_rows_kernel<K, S, PX, 2, TFIMM_ACT_SWISH>) : go(dwconv_rows_kernel<K, S, PX, 1, TFIMM_ACT_SWISH>);
  if (act == TFIMM_ACT_RELU6) return go(dwconv_rows_kernel<K, S, PX, 1, TFIMM_ACT_RELU6>);
  return go(dwconv_rows_kernel<K, S, PX, 1, -1>);
}


template <int K, int S>
static int launch_dwconv_strip(const bf16_t* x, const float* w, const float* bias, bf16_t* y, tfimm_sq_t* sum_out, int B,
                               int H, int W, int C, int pad_t, int pad_l, int OH, int OW, int act, hipStream_t st) {
  constexpr int PX = 4;
  // 4 channels per thread keep the accumulators + one filter row of weights under 64 VGPRs for the
  // large filters (8 waves per SIMD to hide the load latency); 8 channels halve the instruction
  // count where the filter is small
  constexpr int CV = K >= 5 ? 4 : 8;
  const int64_t items = (int64_t)OH * ((OW + PX - 1) / PX) * (C / CV);
  int64_t bpi = (items + 255) / 256;                    // blocks per image if every thread took one item
  const int64_t want = (8 * 256 + B - 1) / B;           // ~8 resident blocks per CU over the whole grid
  if (bpi > want) bpi = want < 1 ? 1 : want;
  const size_t lds = sum_out ? (size_t)C * sizeof(tfimm_sq_t) : 0;
  TFIMM_LAUNCH((dwconv_strip_kernel<K, S, PX, CV>), dim3((unsigned)bpi, (unsigned)B), dim3(256), lds, st, x, w, bias, y,
               sum_out, H, W, C, pad_t, pad_l, OH, OW, act);
  return 0;
}

// ---------------------------------------------------------------------------------------
// SE gate: one block per image
// ---------------------------------------------------------------------------------------
// One 1024-thread workgroup per image (the kernel is latency-bound: 16 waves share the rd reduction rows; packing 4
// images into a workgroup to reuse the weights measured 1.5x SLOWER).  w1 rows are read by whole waves and w2
// ([rd][C]: the Keras layout of the expand conv) by consecutive threads -- all loads coalesced.  (256 threads and a
// [C][rd] w2 walked row-per-thread took 67 us for C = 1632.)
#ifndef TFIMM_SE_IMG
#define TFIMM_SE_IMG 1
#endif
constexpr int SE_IMG = TFIMM_SE_IMG;      // images per block (1: measured best -- see profiles/NOTES_r06.md 10)
__global__ void __launch_bounds__(1024) se_gate_kernel(const void* __restrict__ sums_v, int sums_fixed, float inv_count,
                                                      const float* __restrict__ w1, const float* __restrict__ b1,
                                                      const float* __restrict__ w2, const float* __restrict__ b2,
                                                      float* __restrict__ gate, int B, int C, int rd, int act,
                                                      int gate_act) {
  extern __shared__ float sm[];  // [SE_IMG][C] means + [SE_IMG][rd] hidden
  float* mean = sm;
  float* hid = sm + SE_IMG * C;
  const int b0 = blockIdx.x * SE_IMG;
  for (int i = threadIdx.x; i < SE_IMG * C; i += blockDim.x) {
    const int im = i / C;
    float sv = 0.f;
    if (b0 + im < B)
      sv = sums_fixed ? sq_to_float(reinterpret_cast<const tfimm_sq_t*>(sums_v)[(int64_t)b0 * C + i])
                      : reinterpret_cast<const float*>(sums_v)[(int64_t)b0 * C + i];
    mean[i] = sv * inv_count;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int j = wave; j < rd; j += nw) {
    float s[SE_IMG];
#pragma unroll
    for (int im = 0; im < SE_IMG; ++im) s[im] = 0.f;
    const float* wr = w1 + (int64_t)j * C;
#pragma unroll 4
    for (int c = lane; c < C; c += 64) {
      const float wv = wr[c];
#pragma unroll
      for (int im = 0; im < SE_IMG; ++im) s[im] += wv * mean[im * C + c];
    }
#pragma unroll
    for (int im = 0; im < SE_IMG; ++im) {
      const float t = wave_sum(s[im]);
      if (lane == 0) hid[im * rd + j] = apply_act(t + (b1 ? b1[j] : 0.f), act);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s[SE_IMG];
    const float bv = b2 ? b2[c] : 0.f;
#pragma unroll
    for (int im = 0; im < SE_IMG; ++im) s[im] = bv;
    // (unrolled: the rd loads of a thread are independent, only the adds are a chain)
#pragma unroll 8
    for (int j = 0; j < rd; ++j) {
      const float wv = w2[(int64_t)j * C + c];
#pragma unroll
      for (int im = 0; im < SE_IMG; ++im) s[im] += wv * hid[im * rd + j];
    }
#pragma unroll
    for (int im = 0; im < SE_IMG; ++im)
      if (b0 + im < B) gate[(int64_t)(b0 + im) * C + c] = apply_act(s[im], gate_act);
  }
}

__global__ void scale_channels_kernel(const bf16_t* x, const float* gate, const bf16_t* residual, bf16_t* y, int B,
                                      int R, int C, int act_after) {
  const int64_t total = (int64_t)B * R * C;
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total;
       id += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(id % C);
    const int64_t b = id / ((int64_t)R * C);
    float v = bf2f(x[id]) * gate[b * C + c];
    if (residual) v += bf2f(residual[id]);
    if (act_after) v = fmaxf(v, 0.f);
    y[id] = (bf16_t)f2bf(v);
  }
}

// ---------------------------------------------------------------------------------------
// Swin PatchMerging gather + LayerNorm(4C): one wave per output token
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) patch_merge_ln_kernel(const bf16_t* x, bf16_t* y, const float* gamma,
                                                             const float* beta, int B, int H, int W, int C,
                                                             float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const int H2 = H / 2, W2 = W / 2, D = 4 * C;
  const int64_t rows = (int64_t)B * H2 * W2;
  const float inv_d = 1.f / (float)D;
  for (int64_t r = wave0; r < rows; r += nwaves) {
    const int x2 = (int)(r % W2);
    const int y2 = (int)((r / W2) % H2);
    const int64_t b = r / ((int64_t)W2 * H2);
    // concat order x0,x1,x2,x3 = (dy,dx) (0,0),(1,0),(0,1),(1,1)   (swin.py:353-357)
    auto src = [&](int j) -> float {
      const int part = j / C, c = j - part * C;
      const int dy = part & 1, dx = part >> 1;
      return bf2f(x[((b * H + (2 * y2 + dy)) * W + (2 * x2 + dx)) * C + c]);
    };
    float sum = 0.f;
    for (int j = lane; j < D; j += 64) sum += src(j);
    const float mean = wave_sum(sum) * inv_d;
    float sq = 0.f;
    for (int j = lane; j < D; j += 64) {
      const float t = src(j) - mean;
      sq += t * t;
    }
    const float rstd = rsqrtf(wave_sum(sq) * inv_d + eps);
    bf16_t* yr = y + r * D;
    for (int j = lane; j < D; j += 64) yr[j] = (bf16_t)f2bf((src(j) - mean) * rstd * gamma[j] + beta[j]);
  }
}

// Vector flavour (C % 8 == 0, 4C <= 64 * 8 * NCH): the gathered row lives in registers as NCH 16-byte
// chunks per lane -- one global read, two-pass statistics on registers, one 16-byte write per chunk.
// (The scalar kernel above re-reads the row three times with 2-byte loads and an integer division per
// element: 0.95 TB/s on Swin-B's three merges.)
template <int NCH>
__global__ void __launch_bounds__(256) patch_merge_ln_vec_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, int B, int H, int W,
                                                                 int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const int H2 = H / 2, W2 = W / 2, D = 4 * C, nchunk = D / 8;
  const int64_t rows = (int64_t)B * H2 * W2;
  const float inv_d = 1.f / (float)D;
  // chunk -> (part, channel) once per lane: concat order (dy,dx) = (0,0),(1,0),(0,1),(1,1) (swin.py:353-357)
  int coff[NCH];   // element offset of the chunk relative to pixel (2*y2, 2*x2), or -1
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int j8 = lane + i * 64;
    if (j8 < nchunk) {
      const int part = (j8 * 8) / C, c = j8 * 8 - part * C;
      coff[i] = ((part & 1) * W + (part >> 1)) * C + c;
    } else {
      coff[i] = -1;
    }
  }
  for (int64_t r = wave0; r < rows; r += nwaves) {
    const int x2 = (int)(r % W2);
    const int y2 = (int)((r / W2) % H2);
    const int64_t b = r / ((int64_t)W2 * H2);
    const bf16_t* base = x + ((b * H + 2 * y2) * W + 2 * x2) * C;
    float v[NCH][8];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      uint4 u = make_uint4(0u, 0u, 0u, 0u);
      if (coff[i] >= 0) u = *reinterpret_cast<const uint4*>(base + coff[i]);
      unpack8(u, v[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += v[i][e];
    }
    const float mean = wave_sum(sum) * inv_d;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      if (coff[i] >= 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float t = v[i][e] - mean;
          sq += t * t;
        }
      }
    const float rstd = rsqrtf(wave_sum(sq) * inv_d + eps);
    bf16_t* yr = y + r * D;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      if (coff[i] >= 0) {
        const int j = (lane + i * 64) * 8;
        const float4 g0 = *reinterpret_cast<const float4*>(gamma + j), g1 = *reinterpret_cast<const float4*>(gamma + j + 4);
        const float4 b0 = *reinterpret_cast<const float4*>(beta + j), b1 = *reinterpret_cast<const float4*>(beta + j + 4);
        const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (v[i][e] - mean) * rstd * gg[e] + bb[e];
        *reinterpret_cast<uint4*>(yr + j) = pack8(o);
      }
  }
}

__global__ void bias_act_kernel(const bf16_t* x, const float* bias, bf16_t* y, int64_t rows, int C, int act) {
  const int64_t total = rows * C;
  for (int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total;
       id += (int64_t)gridDim.x * blockDim.x) {
    float v = bf2f(x[id]);
    if (bias) v += bias[id % C];
    y[id] = (bf16_t)f2bf(apply_act(v, act));
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------
// C ABI wrappers
// ---------------------------------------------------------------------------------------
extern "C" int tfimm_hip_cast_input(const void* in, int in_dtype, void* out, int64_t n_pixels, int c_in,
                                    int c_out, void* stream) {
  if (!in || !out || n_pixels <= 0 || c_in <= 0 || c_out < c_in || (in_dtype != 0 && in_dtype != 1))
    TFIMM_FAIL(TFIMM_EINVAL, "cast_input: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = grid_for(n_pixels, 256);
  if (c_in == 3 && c_out == 4 && (((uintptr_t)out & 7) == 0)) {
    if (in_dtype && (n_pixels & 3) == 0 && (((uintptr_t)in & 7) == 0) && (((uintptr_t)out & 15) == 0)) {
      TFIMM_LAUNCH(cast_rgb4_quad_kernel, dim3(grid_for(n_pixels / 4, 256)), dim3(256), 0, st, (const uint2*)in, (uint4*)out, n_pixels / 4);
    } else if (in_dtype) {
      TFIMM_LAUNCH(cast_rgb4_kernel<true>, dim3(grid), dim3(256), 0, st, in, (uint2*)out, n_pixels);
    } else {
      TFIMM_LAUNCH(cast_rgb4_kernel<false>, dim3(grid), dim3(256), 0, st, in, (uint2*)out, n_pixels);
    }
  } else {
    if (in_dtype) TFIMM_LAUNCH(cast_input_kernel<true>, dim3(grid), dim3(256), 0, st, in, (bf16_t*)out, n_pixels, c_in, c_out);
    else TFIMM_LAUNCH(cast_input_kernel<false>, dim3(grid), dim3(256), 0, st, in, (bf16_t*)out, n_pixels, c_in, c_out);
  }
  return 0;
}

extern "C" int tfimm_hip_cast_input_pad(const void* in, int in_dtype, void* out, int B, int H, int W, int c_in,
                                        int pad_t, int pad_b, int pad_l, int pad_r, void* stream) {
  if (!in || !out || B <= 0 || H <= 0 || W <= 0 || c_in <= 0 || c_in > 4 || pad_t < 0 || pad_b < 0 || pad_l < 0 ||
      pad_r < 0 || (in_dtype != 0 && in_dtype != 1) || ((uintptr_t)out & 7))
    TFIMM_FAIL(TFIMM_EINVAL, "cast_input_pad: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int HP = H + pad_t + pad_b, WP = W + pad_l + pad_r;
  const unsigned grid = grid_for((int64_t)B * HP * WP, 256);
  if (in_dtype && c_in == 3 && (W & 3) == 0 && (((uintptr_t)in & 7) == 0)) {
    const int64_t work = (int64_t)B * H * (W / 4) + (int64_t)B * ((int64_t)HP * WP - (int64_t)H * W);
    TFIMM_LAUNCH(cast_pad4_quad_kernel, dim3(grid_for(work, 256)), dim3(256), 0, st, (const uint2*)in, (uint2*)out, B, H, W, pad_t, pad_l, HP, WP);
  } else if (in_dtype) {
    TFIMM_LAUNCH(cast_pad4_kernel<true>, dim3(grid), dim3(256), 0, st, in, (uint2*)out, B, H, W, c_in, pad_t, pad_l, HP, WP);
  } else {
    TFIMM_LAUNCH(cast_pad4_kernel<false>, dim3(grid), dim3(256), 0, st, in, (uint2*)out, B, H, W, c_in, pad_t, pad_l, HP, WP);
  }
  return 0;
}

static bool norm_params(NormParams& np, const float* mean, const float* std, int c_in) {
  if (!mean || !std || c_in <= 0 || c_in > TFIMM_PREPROCESS_MAX_CHANNELS) return false;
  for (int c = 0; c < TFIMM_PREPROCESS_MAX_CHANNELS; ++c) {
    np.mean[c] = c < c_in ? mean[c] : 0.f;
    np.std[c] = c < c_in ? std[c] : 1.f;
    if (!(np.std[c] != 0.f)) return false;
  }
  return true;
}

extern "C" int tfimm_hip_preprocess_input(const void* in, void* out, int64_t n_pixels, int c_in, int c_out,
                                          const float* mean, const float* std, void* stream) {
  NormParams np;
  if (!in || !out || n_pixels <= 0 || c_out < c_in || !norm_params(np, mean, std, c_in))
    TFIMM_FAIL(TFIMM_EINVAL, "preprocess_input: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (c_in == 3 && c_out == 4 && (((uintptr_t)out & 15) == 0) && (((uintptr_t)in & 3) == 0)) {
    const unsigned grid = grid_for((n_pixels + 3) / 4, 256);
    TFIMM_LAUNCH(preprocess_rgb4_kernel, dim3(grid), dim3(256), 0, st, (const uint8_t*)in, (uint2*)out, n_pixels, np);
  } else {
    const unsigned grid = grid_for(n_pixels, 256);
    TFIMM_LAUNCH(preprocess_kernel, dim3(grid), dim3(256), 0, st, (const uint8_t*)in, (bf16_t*)out, n_pixels, c_in, c_out, np);
  }
  return 0;
}

extern "C" int tfimm_hip_preprocess_input_pad(const void* in, void* out, int B, int H, int W, int c_in, int pad_t,
                                              int pad_b, int pad_l, int pad_r, const float* mean, const float* std,
                                              void* stream) {
  NormParams np;
  if (!in || !out || B <= 0 || H <= 0 || W <= 0 || c_in > 4 || pad_t < 0 || pad_b < 0 || pad_l < 0 || pad_r < 0 ||
      ((uintptr_t)out & 7) || !norm_params(np, mean, std, c_in))
    TFIMM_FAIL(TFIMM_EINVAL, "preprocess_input_pad: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int HP = H + pad_t + pad_b, WP = W + pad_l + pad_r;
  const unsigned grid = grid_for((int64_t)B * HP * WP, 256);
  TFIMM_LAUNCH(preprocess_pad4_kernel, dim3(grid), dim3(256), 0, st, (const uint8_t*)in, (uint2*)out, B, H, W, c_in, pad_t,
               pad_l, HP, WP, np);
  return 0;
}

// Row statistics for a LayerNorm that is folded into the following GEMM (tfimm_gemm_desc.ln_stats): the same fp32 two-pass
// mean / population variance as the LayerNorm kernels above, the row held in registers, but nothing is written except
// (mean, rstd) -- half the traffic of the normalising pass.  LPR lanes per row, up to 4 chunks of 16 bytes per lane.
template <int LPR>
__global__ void __launch_bounds__(256) row_stats_kernel(const bf16_t* __restrict__ x, float* __restrict__ stats, int64_t rows,
                                                        int d, int64_t xs, float eps) {
  constexpr int RPW = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int sub = lane / LPR, c = lane % LPR;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const int nchunks = d >> 3;
  const float inv_d = 1.f / (float)d;
  auto group_sum = [&](float v) -> float {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  };
  for (int64_t r0 = wave0 * RPW; r0 < rows; r0 += nwaves * RPW) {
    const int64_t r = r0 + sub;
    const bool rok = r < rows;
    float v[4][8];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint4 u = make_uint4(0u, 0u, 0u, 0u);
      if (rok && c + i * LPR < nchunks) u = reinterpret_cast<const uint4*>(x + r * xs)[c + i * LPR];
      unpack8(u, v[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += v[i][e];
    }
    const float mean = group_sum(sum) * inv_d;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (c + i * LPR < nchunks) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float t = v[i][e] - mean;
          sq += t * t;
        }
      }
    const float rstd = rsqrtf(group_sum(sq) * inv_d + eps);
    if (rok && c == 0) *reinterpret_cast<float2*>(stats + r * 2) = make_float2(mean, rstd);
  }
}

extern "C" int tfimm_hip_row_stats(const void* x, float* stats, int64_t rows, int d, int64_t x_stride, float eps, void* stream) {
  if (!x || !stats) TFIMM_FAIL(TFIMM_EINVAL, "row_stats: null pointer");
  if (rows <= 0 || d <= 0 || x_stride < d) TFIMM_FAIL(TFIMM_EINVAL, "row_stats: bad shape");
  if ((d & 7) || (x_stride & 7) || ((uintptr_t)x & 15) || ((uintptr_t)stats & 7) || d > 2048)
    TFIMM_FAIL(TFIMM_EUNSUP, "row_stats: rows of d %% 8 == 0 <= 2048 channels, 16-byte aligned");
  const int nchunks = d >> 3;
  hipStream_t st = (hipStream_t)stream;
  const bf16_t* xb = (const bf16_t*)x;
  auto grid_for = [&](int rpw) { return (unsigned)std::min<int64_t>((rows + 4 * rpw - 1) / (4 * rpw), 65536); };
  if (nchunks <= 32) TFIMM_LAUNCH(row_stats_kernel<8>, dim3(grid_for(8)), dim3(256), 0, st, xb, stats, rows, d, x_stride, eps);
  else if (nchunks <= 64) TFIMM_LAUNCH(row_stats_kernel<16>, dim3(grid_for(4)), dim3(256), 0, st, xb, stats, rows, d, x_stride, eps);
  else if (nchunks <= 128) TFIMM_LAUNCH(row_stats_kernel<32>, dim3(grid_for(2)), dim3(256), 0, st, xb, stats, rows, d, x_stride, eps);
  else TFIMM_LAUNCH(row_stats_kernel<64>, dim3(grid_for(1)), dim3(256), 0, st, xb, stats, rows, d, x_stride, eps);
  return 0;
}

extern "C" int tfimm_hip_layernorm(const void* x, void* y, const float* gamma, const float* beta, int64_t rows,
                                   int d, int64_t x_stride, int64_t y_stride, float eps, void* stream) {
  if (!x || !y || !gamma || !beta || rows <= 0 || d <= 0) TFIMM_FAIL(TFIMM_EINVAL, "layernorm: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = grid_for(rows, 4);
  const bool vec = (d % 8 == 0) && (x_stride % 8 == 0) && (y_stride % 8 == 0) && (((uintptr_t)x & 15) == 0) &&
                   (((uintptr_t)y & 15) == 0) && (((uintptr_t)gamma & 15) == 0) && (((uintptr_t)beta & 15) == 0) &&
                   d <= 4096;
  const bf16_t* xb = (const bf16_t*)x;
  bf16_t* yb = (bf16_t*)y;
  if (vec) {
    static const bool no_x3 = getenv("TFIMM_LN_NO_X3") != nullptr;      // (A/B switch for profiling)
    // (measured, MI355X: d = 768 71.6 -> 51.9 us for 100864 rows, d = 384 17.1 -> 15.2 us for 50176 rows; d = 192 / 96
    //  are no faster than the narrow kernel below -- 64-byte row pieces per lane group -- and stay there)
    if (!no_x3 && (d == 384 || d == 768)) {
      const int lpr = d / 24, rpw = 64 / lpr;
      const unsigned gr = grid_for((rows + rpw - 1) / rpw, 4);
      if (lpr == 16) TFIMM_LAUNCH(layernorm_x3_kernel<16>, dim3(gr), dim3(256), 0, st, xb, yb, gamma, beta, rows, x_stride, y_stride, eps);
      else TFIMM_LAUNCH(layernorm_x3_kernel<32>, dim3(gr), dim3(256), 0, st, xb, yb, gamma, beta, rows, x_stride, y_stride, eps);
      return 0;
    }
    if (d <= 64) {
      const unsigned g8 = grid_for((rows + 7) / 8, 4);
      TFIMM_LAUNCH(layernorm_narrow_kernel<8>, dim3(g8), dim3(256), 0, st, xb, yb, gamma, beta, rows, d, x_stride, y_stride, eps);
    } else if (d <= 128) {
      const unsigned g4 = grid_for((rows + 3) / 4, 4);
      TFIMM_LAUNCH(layernorm_narrow_kernel<16>, dim3(g4), dim3(256), 0, st, xb, yb, gamma, beta, rows, d, x_stride, y_stride, eps);
    } else if (d <= 256) {
      const unsigned g2 = grid_for((rows + 1) / 2, 4);
      TFIMM_LAUNCH(layernorm_narrow_kernel<32>, dim3(g2), dim3(256), 0, st, xb, yb, gamma, beta, rows, d, x_stride, y_stride, eps);
    } else if (d <= 512) TFIMM_LAUNCH(layernorm_vec_kernel<1>, dim3(grid), dim3(256), 0, st, xb, yb, gamma, beta, rows, d, x_stride, y_stride, eps);
    else if (d <= 1024) TFIMM_LAUNCH(layernorm_vec_kernel<2>, dim3(grid), dim3(256), 0, st, xb, yb, gamma, beta, rows, d, x_stride, y_stride, eps);
    else if (d <= 2048) TFIMM_LAUNCH(layernorm_vec_kernel<4>, dim3(grid), dim3(256), 0, st, xb, yb, gamma, beta, rows, d, x_stride, y_stride, eps);
    else TFIMM_LAUNCH(layernorm_vec_kernel<8>, dim3(grid), dim3(256), 0, st, xb, yb, gamma, beta, rows, d, x_stride, y_stride, eps);
  } else {
    TFIMM_LAUNCH(layernorm_generic_kernel, dim3(grid), dim3(256), 0, st, xb, yb, gamma, beta, rows, d, x_stride, y_stride, eps);
  }
  return 0;
}

extern "C" int tfimm_hip_maxpool(const void* x, void* y, int B, int H, int W, int C, int k, int stride, int pad,
                                 int OH, int OW, void* stream) {
  if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || k <= 0 || stride <= 0 || pad < 0 || OH <= 0 || OW <= 0)
    TFIMM_FAIL(TFIMM_EINVAL, "maxpool: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C % 8 == 0) && (((uintptr_t)x & 15) == 0) && (((uintptr_t)y & 15) == 0);
  if (vec) {
    const unsigned grid = grid_for((int64_t)B * OH * OW * (C / 8), 256);
    TFIMM_LAUNCH(maxpool_vec_kernel, dim3(grid), dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)y, B, H, W, C, k, stride, pad, OH, OW);
  } else {
    const unsigned grid = grid_for((int64_t)B * OH * OW * C, 256);
    TFIMM_LAUNCH(maxpool_generic_kernel, dim3(grid), dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)y, B, H, W, C, k, stride, pad, OH, OW);
  }
  return 0;
}

extern "C" int tfimm_hip_mean_rows(const void* x, void* y, int B, int R, int C, int out_f32, void* stream) {
  if (!x || !y || B <= 0 || R <= 0 || C <= 0) TFIMM_FAIL(TFIMM_EINVAL, "mean_rows: bad arguments");
  if ((C & 7) == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
    const int64_t vblocks = (int64_t)B * ((C + 511) / 512);
    const unsigned vgrid = (unsigned)(vblocks > 65535 * 16 ? 65535 * 16 : vblocks);
    TFIMM_LAUNCH(mean_rows_vec_kernel, dim3(vgrid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, y, B, R, C, out_f32);
    return 0;
  }
  const int64_t blocks = (int64_t)B * ((C + 63) / 64);
  const unsigned grid = (unsigned)(blocks > 65535 * 16 ? 65535 * 16 : blocks);
  TFIMM_LAUNCH(mean_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, y, B, R, C, out_f32);
  return 0;
}

extern "C" int tfimm_hip_bcast_rows(const void* src, void* dst, int B, int n_rows, int d, int dst_rows_per_image,
                                    void* stream) {
  if (!src || !dst || B <= 0 || n_rows <= 0 || d <= 0 || dst_rows_per_image < n_rows)
    TFIMM_FAIL(TFIMM_EINVAL, "bcast_rows: bad arguments");
  const unsigned grid = grid_for((int64_t)B * n_rows * d, 256);
  TFIMM_LAUNCH(bcast_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, (bf16_t*)dst, B, n_rows, d, dst_rows_per_image);
  return 0;
}

extern "C" int tfimm_hip_dwconv(const void* x, const float* w, const float* bias, void* y, void* sum_out_v, int B,
                                int H, int W, int C, int k, int stride, int pad_t, int pad_l, int OH, int OW,
                                int act, void* stream) {
  tfimm_sq_t* sum_out = reinterpret_cast<tfimm_sq_t*>(sum_out_v);
  if (!x || !w || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || k <= 0 || stride <= 0 || OH <= 0 || OW <= 0)
    TFIMM_FAIL(TFIMM_EINVAL, "dwconv: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (C % 8 == 0) && (((uintptr_t)x & 15) == 0) && (((uintptr_t)y & 15) == 0) &&
                   (((uintptr_t)w & 15) == 0);
  static int use_rows = -1;
  if (use_rows < 0) {
    const char* e = getenv("TFIMM_DW_NO_ROWS");
    use_rows = (e && e[0] == '1') ? 0 : 1;
  }
  if (use_rows && ((stride == 1 && (k == 3 || k == 5 || k == 7)) || (stride == 2 && (k == 3 || k == 5))) && (C % 2) == 0 && (((uintptr_t)x | (uintptr_t)y) & 3) == 0 && B <= 65535) {
    // row-stationary kernel (an earlier sliding-window "marching" kernel measured 10-35 % slower on every shape)
    if (stride == 2 && k == 3) return launch_dwconv_rows<3, 2>((const bf16_t*)x, w, bias, (bf16_t*)y, sum_out, B, H, W, C, pad_t, pad_l, OH, OW, act, st);
    if (stride == 2) return launch_dwconv_rows<5, 2>((const bf16_t*)x, w, bias, (bf16_t*)y, sum_out, B, H, W, C, pad_t, pad_l, OH, OW, act, st);
    if (k == 3) return launch_dwconv_rows<3, 1>((const bf16_t*)x, w, bias, (bf16_t*)y, sum_out, B, H, W, C, pad_t, pad_l, OH, OW, act, st);
    if (k == 5) return launch_dwconv_rows<5, 1>((const bf16_t*)x, w, bias, (bf16_t*)y, sum_out, B, H, W, C, pad_t, pad_l, OH, OW, act, st);
    return launch_dwconv_rows<7, 1>((const bf16_t*)x, w, bias, (bf16_t*)y, sum_out, B, H, W, C, pad_t, pad_l, OH, OW, act, st);
  }
  if (vec && C <= 8192 && B <= 65535) {
    const bf16_t* xb = (const bf16_t*)x;
    bf16_t* yb = (bf16_t*)y;
    if (k == 3 && stride == 1) return launch_dwconv_strip<3, 1>(xb, w, bias, yb, sum_out, B, H, W, C, pad_t, pad_l, OH, OW, act, st);
    if (k == 3 && stride == 2) return launch_dwconv_strip<3, 2>(xb, w, bias, yb, sum_out, B, H, W, C, pad_t, pad_l, OH, OW, act, st);
    if (k == 5 && stride == 1) return launch_dwconv_strip<5, 1>(xb, w, bias, yb, sum_out, B, H, W, C, pad_t, pad_l, OH, OW, act, st);
    if (k == 5 && stride == 2) return launch_dwconv_strip<5, 2>(xb, w, bias, yb, sum_out, B, H, W, C, pad_t, pad_l, OH, OW, act, st);
    if (k == 7 && stride == 1) return launch_dwconv_strip<7, 1>(xb, w, bias, yb, sum_out, B, H, W, C, pad_t, pad_l, OH, OW, act, st);
  }
  if (vec) {
    const unsigned grid = grid_for((int64_t)B * OH * OW * (C / 8), 256);
    TFIMM_LAUNCH(dwconv_kernel<true>, dim3(grid), dim3(256), 0, st, (const bf16_t*)x, w, bias, (bf16_t*)y, sum_out, B, H, W, C, k, stride, pad_t, pad_l, OH, OW, act);
  } else {
    const unsigned grid = grid_for((int64_t)B * OH * OW * C, 256);
    TFIMM_LAUNCH(dwconv_kernel<false>, dim3(grid), dim3(256), 0, st, (const bf16_t*)x, w, bias, (bf16_t*)y, sum_out, B, H, W, C, k, stride, pad_t, pad_l, OH, OW, act);
  }
  return 0;
}

extern "C" int tfimm_hip_se_gate(const void* sums, int sums_fixed, float inv_count, const float* w1, const float* b1,
                                 const float* w2, const float* b2, float* gate, int B, int C, int rd, int act,
                                 int gate_act, void* stream) {
  if (!sums || !w1 || !w2 || !gate || B <= 0 || C <= 0 || rd <= 0) TFIMM_FAIL(TFIMM_EINVAL, "se_gate: bad arguments");
  const size_t lds = (size_t)SE_IMG * (C + rd) * sizeof(float);
  if (lds > 160 * 1024) TFIMM_FAIL(TFIMM_EUNSUP, "se_gate: C + rd = %d too large", C + rd);
  static tfimm_once_t attr_done;
  if (attr_done.need()) {
    TFIMM_HIP_CHECK(hipFuncSetAttribute((const void*)se_gate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_done.mark();
  }
  TFIMM_LAUNCH(se_gate_kernel, dim3((B + SE_IMG - 1) / SE_IMG), dim3(1024), lds, (hipStream_t)stream, sums, sums_fixed, inv_count, w1, b1, w2, b2,
               gate, B, C, rd, act, gate_act);
  return 0;
}

extern "C" int tfimm_hip_scale_channels(const void* x, const float* gate, const void* residual, void* y, int B,
                                        int R, int C, int act_after, void* stream) {
  if (!x || !gate || !y || B <= 0 || R <= 0 || C <= 0) TFIMM_FAIL(TFIMM_EINVAL, "scale_channels: bad arguments");
  const unsigned grid = grid_for((int64_t)B * R * C, 256);
  TFIMM_LAUNCH(scale_channels_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, gate, (const bf16_t*)residual, (bf16_t*)y, B, R, C, act_after);
  return 0;
}

extern "C" int tfimm_hip_patch_merge_ln(const void* x, void* y, const float* gamma, const float* beta, int B,
                                        int H, int W, int C, float eps, void* stream) {
  if (!x || !y || !gamma || !beta || B <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || C <= 0)
    TFIMM_FAIL(TFIMM_EINVAL, "patch_merge_ln: bad arguments");
  const unsigned grid = grid_for((int64_t)B * (H / 2) * (W / 2), 4);
  hipStream_t st = (hipStream_t)stream;
  const int nchunk = C / 2;   // 16-byte chunks of the 4C-wide merged row
  const bool vec = (C % 8) == 0 && nchunk <= 64 * 8 && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0;
  if (vec && nchunk <= 64) TFIMM_LAUNCH(patch_merge_ln_vec_kernel<1>, dim3(grid), dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)y, gamma, beta, B, H, W, C, eps);
  else if (vec && nchunk <= 128) TFIMM_LAUNCH(patch_merge_ln_vec_kernel<2>, dim3(grid), dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)y, gamma, beta, B, H, W, C, eps);
  else if (vec && nchunk <= 256) TFIMM_LAUNCH(patch_merge_ln_vec_kernel<4>, dim3(grid), dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)y, gamma, beta, B, H, W, C, eps);
  else if (vec) TFIMM_LAUNCH(patch_merge_ln_vec_kernel<8>, dim3(grid), dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)y, gamma, beta, B, H, W, C, eps);
  else TFIMM_LAUNCH(patch_merge_ln_kernel, dim3(grid), dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)y, gamma, beta, B, H, W, C, eps);
  return 0;
}

__global__ void fill_bytes_kernel(uint32_t* dst, uint32_t word, size_t n_words) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (size_t)gridDim.x * blockDim.x) dst[i] = word;
}

__global__ void fill_odd_bytes_kernel(uint8_t* dst, uint8_t b, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = b;
}

extern "C" int tfimm_hip_memset_async(void* dst, int value, size_t bytes, void* stream) {
  if (!dst) TFIMM_FAIL(TFIMM_EINVAL, "memset_async: null pointer");
  // A fill KERNEL, not hipMemsetAsync: recorded into a HIP graph the latter becomes a memset node, and such a node writes the
  // recorded value on the first replay only -- afterwards a 16-byte pattern of host memory (the HIP 7.0 runtime of the PyTorch
  // wheel; graphs of nothing but memset nodes show it: tools/probes/memset_node_probe.py, profiles/r04_memset_node_probe.txt).
  // TFIMM_MEMSET_NODE=1 keeps the runtime call reachable for that probe.
  static const bool use_node = getenv("TFIMM_MEMSET_NODE") && atoi(getenv("TFIMM_MEMSET_NODE")) != 0;
  if (use_node) {
    TFIMM_HIP_CHECK(hipMemsetAsync(dst, value, bytes, (hipStream_t)stream));
    return 0;
  }
  if (bytes == 0) return 0;
  const uint32_t b = (uint32_t)(value & 0xff), word = b | (b << 8) | (b << 16) | (b << 24);
  if ((bytes & 3) == 0 && (((uintptr_t)dst) & 3) == 0) {
    const size_t n = bytes / 4;
    TFIMM_LAUNCH(fill_bytes_kernel, dim3(grid_for((int64_t)n, 256)), dim3(256), 0, (hipStream_t)stream, (uint32_t*)dst, word, n);
  } else {      // odd sizes / addresses: byte by byte (no caller on the model path has them)
    TFIMM_LAUNCH(fill_odd_bytes_kernel, dim3(grid_for((int64_t)bytes, 256)), dim3(256), 0, (hipStream_t)stream, (uint8_t*)dst, (uint8_t)b, bytes);
  }
  return 0;
}

extern "C" int tfimm_hip_bias_act(const void* x, const float* bias, void* y, int64_t rows, int C, int act,
                                  void* stream) {
  if (!x || !y || rows <= 0 || C <= 0) TFIMM_FAIL(TFIMM_EINVAL, "bias_act: bad arguments");
  const unsigned grid = grid_for(rows * C, 256);
  TFIMM_LAUNCH(bias_act_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, bias, (bf16_t*)y, rows, C, act);
  return 0;
}

// tfimm_hip_gemm host side: validate the descriptor, chunk tensors over 2 GiB, classify the operands, route to one of four
// kernel families, launch.  The families, in the order route() tries them:
//   strip   input-strip 3x3 convolution: conv_strip.hip
//   stream  persistent LDS-DMA, tile ids 0..9: gemm_stream_kernel.h, gemm_stream_inst.hip; 7 (deep ring) gemm_pipe_*; 9 (duo) gemm_duo_*
//   dma     one tile per workgroup, LDS-DMA, tile ids 0..5: gemm_dma_kernel.h, gemm_dma_inst.hip
//   reg     register-staged, tile ids 0..5, every operand flavour: gemm_kernel.h, gemm_inst.hip
// Who serves which tile_hint.  "else": the family's operand test fails (stream_applies / dma_applies: weights not K-padded to 64,
// a tensor over 2 GiB, TFIMM_GEMM_NO_STREAM / TFIMM_GEMM_NO_DMA); "scored": the cost model picks the tile; the scalar flavours
// (unaligned dense rows, Cin % 8 != 0) always run on reg 64x64, and C4 follows the reg entries of the first column.
//   hint    dense, conv (16-byte loads)               SE gate (a_scale)                  a2 [4] / LN-folded [4] / conv stride_w != stride
//   0       strip [1], else stream scored, else dma   stream scored [3], else reg        stream scored, else EUNSUP
//           scored, else reg pick_tile                pick_tile
//   1-6     reg tile hint-1 [2]                       reg tile hint-1 [2]                as hint 0: the hint is ignored
//   11-16   dma tile hint-11, else reg pick_tile      reg pick_tile                      as hint 0
//   21-30   stream tile hint-21 [5], else dma         stream tile hint-21 [3][5], else   stream tile hint-21 [5], else EUNSUP
//           scored, else reg pick_tile                reg pick_tile
//   31      strip when conv_strip_applies, else as hint 0 in every column
//   7-10 and 17-20 keep a layer off stream like 1-20 and are scored by dma; any other value is hint 0.
//   [1] the strip shape only, unless TFIMM_STRIP_CONV=0, and when M >= 128 x CUs (conv_strip_applies)
//   [2] when that tile has the flavour, else pick_tile's heuristic; 128x64 / 64x64 when the picked tile lacks the flavour
//   [3] reg pick_tile when a row tile touches more images than its waves can bring gate slices for (route_stream)
//   [4] a2 and LN-folded layers also need the residual-free vector epilogue (N % 8 == 0, 16-byte aligned bf16 rows), else EUNSUP
//   [5] 30 (duo) -> the 256x128 stream tile for the catch-all epilogue, K <= 32, SE gate, a2; a tile without the SE-gate / a2 /
//       LN flavour (28, the deep ring, has none of them; LN also when its LDS would pass 160 KiB) -> the 256x256 stream tile
#include "gemm_stream_kernel.h"

#include <algorithm>
#include <cstdlib>

using namespace tfimm_gemm;

// csrc/conv_strip.hip
int tfimm_launch_conv_strip(const tfimm_gemm::GemmArgs& g, int64_t a_bytes, int64_t w_bytes, int64_t out_bytes, int num_cu, hipStream_t stream);

// the per-tile records of a tile list (each defined in a translation unit of its own) and the lookup id -> record
#define TFIMM_TILE_EXTERN(ID, BM_, BN_, WM_, WN_, CFG, SYM) extern "C" const CFG SYM##ID;
#define TFIMM_TILE_CASE(ID, BM_, BN_, WM_, WN_, CFG, SYM) case ID: return &SYM##ID;
#define TFIMM_TILE_TABLE(LOOKUP, LIST, CFG, SYM) \
  LIST(TFIMM_TILE_EXTERN, CFG, SYM)              \
  static const CFG* LOOKUP(int i) {              \
    switch (i) {                                 \
      LIST(TFIMM_TILE_CASE, CFG, SYM)            \
      default: return nullptr;                   \
    }                                            \
  }
TFIMM_TILE_TABLE(tile_table, TFIMM_GEMM_TILES, TileCfg, tfimm_gemm_tile_)
TFIMM_TILE_TABLE(dma_tile_table, TFIMM_GEMM_DMA_TILES, DmaTileCfg, tfimm_gemm_dma_tile_)
TFIMM_TILE_TABLE(stream_tile_table, TFIMM_GEMM_STREAM_ALL_TILES, StreamTileCfg, tfimm_gemm_stream_tile_)

namespace {

constexpr int64_t kMaxBytes = 0x7fffff00LL;   // the LDS-DMA kernels address every tensor through a buffer descriptor with a 32-bit byte offset
constexpr size_t kMaxLds = 160 * 1024;

// ---- environment switches: each is read once, the first time a call asks for it
enum Env { ENV_NO_STREAM, ENV_NO_DMA, ENV_STRIP_CONV, ENV_NGROUP, ENV_DUO_DELAY_K, ENV_DUO_DELAY_0, ENV_DBG, ENV_DBG_PTR, ENV_AUTO_TILE,
           ENV_LIMIT, ENV_COUNT };
// parse: '1' = set when the first character is '1', 'i' = atoi, 'p' = strtoull of any base, 'l' = atoll; unset: the value without the variable
struct EnvSpec { const char* name; char parse; long long unset; };
constexpr EnvSpec kEnv[ENV_COUNT] = {
    {"TFIMM_GEMM_NO_STREAM", '1', 0},
    {"TFIMM_GEMM_NO_DMA", '1', 0},
    {"TFIMM_STRIP_CONV", 'i', 1},   // 0 disables
    {"TFIMM_GEMM_NGROUP", 'i', -1},
    {"TFIMM_DUO_DELAY_K", 'i', 256},
    {"TFIMM_DUO_DELAY_0", 'i', 2000},
    {"TFIMM_GEMM_DBG", 'i', 0},
    {"TFIMM_GEMM_DBG_PTR", 'p', 0},
    {"TFIMM_GEMM_AUTO_TILE", 'i', -1},   // probe builds only
    {"TFIMM_GEMM_LIMIT", 'l', kMaxBytes}};   // bytes: the tensor size from which chunk_rows splits a dense GEMM into row chunks (a test hook, as
                                             // TFIMM_CHAIN_LIMIT / TFIMM_MLP_LIMIT; the buffer-descriptor bounds keep kMaxBytes)
template <Env E> long long env() {
  static const long long v = [](const EnvSpec& s, const char* e) {
    if (!e) return s.unset;
    return s.parse == '1' ? (long long)(e[0] == '1') : s.parse == 'i' ? (long long)atoi(e) : s.parse == 'l' ? atoll(e) : (long long)strtoull(e, nullptr, 0);
  }(kEnv[E], getenv(kEnv[E].name));
  return v;
}

// ---- what the dispatcher knows about the device
struct Device {
  int num_cu;          // hipDeviceProp_t::multiProcessorCount
  int64_t l2_budget;   // bytes of weight panels a column-panel group may hold: 5/8 of the L2 of one XCD (hipDeviceProp_t::l2CacheSize; 4 MiB -> 2.5 MB)
  // Workgroups per CU of every stream tile: the minimum over the epilogue flavours of an operand kind [K_DENSE, K_CONV], queried
  // for ALL flavours on the first call.  (It used to be filled in flavour by flavour as launches came: the minimum -- and with
  // it the tile the heuristic picks for a shape without a table entry, and the grid -- depended on which OTHER layers
  // had been launched before, so the first forward of a model could differ in the last bits from its later ones:
  // tests/test_gpu_scored_batches.py under TFIMM_BRANCHES=2, cait_xxs24_224.)
  int occ[2][TFIMM_GEMM_STREAM_NUM_TILES];
  tfimm_once_t occ_ready;       // (attributes are per device; the occupancies are the same on every MI355X)
  int ln_occ[TFIMM_GEMM_STREAM_NUM_TILES];   // the LayerNorm-folded flavour, with its extra LDS: queried per tile when first used
  tfimm_once_t ln_ready[TFIMM_GEMM_STREAM_NUM_TILES];
};

Device& device() {
  static Device* const dv = [] {   // the properties: once per process; the occupancies: stream_occupancy, once per device
    static Device d = {};
    int dev = 0;
    hipDeviceProp_t prop;
    const bool ok = hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess;
    d.num_cu = ok && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    int64_t l2 = ok && prop.l2CacheSize > 0 ? prop.l2CacheSize : 4 << 20;
    if (l2 > (16 << 20)) l2 = 4 << 20;          // a runtime that reports the sum over the XCDs (or the MALL): the rule is per XCD
    d.l2_budget = l2 / 8 * 5;
    return &d;
  }();
  return *dv;
}

// resident workgroups per CU of a kernel (1..4); sets the dynamic-LDS attribute it needs first
int query_occupancy(const void* fn, int threads, size_t lds, int* occ) {
  TFIMM_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int nb = 0;
  TFIMM_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, threads, lds));
  *occ = nb < 1 ? 1 : (nb > 4 ? 4 : nb);
  return 0;
}

int stream_occupancy(Device& dv) {
  if (!dv.occ_ready.need()) return 0;
  for (int f = 0; f < 2; ++f)
    for (int e = 0; e < 3; ++e)
      for (int i = 0; i < TFIMM_GEMM_STREAM_NUM_TILES; ++i) {
        const StreamTileCfg* t = stream_tile_table(i);
        // the duo tile has no catch-all flavour (route_stream redirects): two workgroups per CU
        if (!t->fn[f][e]) { if (dv.occ[f][i] == 0) dv.occ[f][i] = 2; continue; }
        int nb = 0;
        if (int rc = query_occupancy((const void*)t->fn[f][e], t->threads, (size_t)t->lds_bytes, &nb)) return rc;
        if (dv.occ[f][i] == 0 || nb < dv.occ[f][i]) dv.occ[f][i] = nb;
      }
  dv.occ_ready.mark();
  return 0;
}

// hipFuncAttributeMaxDynamicSharedMemorySize of the kernels that need it at launch, once per device (tfimm_once_t), one slot per
// [kind][tile][flavour].  (The plain and LayerNorm-folded stream flavours get theirs with their occupancy query.)
enum AttrKind { ATTR_REG, ATTR_DMA, ATTR_STREAM_DUAL, ATTR_STREAM_SCALE, ATTR_KINDS };
tfimm_once_t g_attr[ATTR_KINDS][TFIMM_GEMM_STREAM_NUM_TILES][K_NUM];

int set_attr_once(tfimm_once_t& once, const void* fn, int lds) {
  if (once.need()) {
    TFIMM_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    once.mark();
  }
  return 0;
}

// ---- tile choice.  Register-staged tile ids: 0 128x128, 1 128x64, 2 64x64, 3 256x128, 4 128x256, 5 64x128
int pick_tile(const tfimm_gemm_desc& d, int kmode, int cus) {
  if (kmode == K_DENSE_SCALAR || kmode == K_CONV_SCALAR) return 2;
  if (d.tile_hint > 0 && d.tile_hint <= TFIMM_GEMM_NUM_TILES && tile_table(d.tile_hint - 1)->fn[kmode])
    return d.tile_hint - 1;
  const int64_t M = d.M, N = d.N;
  auto blocks = [&](int bm, int bn) { return cdiv64(M, bm) * cdiv64(N, bn); };
  // prefer the biggest tile that still gives every CU >= 2 blocks
  if (N > 64 && blocks(128, 128) >= 2 * cus) return 0;
  if (N <= 64 && blocks(128, 64) >= 2 * cus) return 1;
  if (N > 64 && blocks(64, 128) >= cus) return 5;
  if (blocks(128, 64) >= 2 * cus) return 1;
  return 2;
}

// Cost model of both LDS-DMA families.  Score = relative kernel efficiency x useful fraction of the padded tile area x fill of
// the last wave of blocks (dma) or of the ceil(tiles / slots) rounds a persistent grid runs (stream), slots = CUs x occ.
template <class Cfg>
int best_tile(int64_t M, int64_t N, const Cfg* (*table)(int), const double* eff, const int* occ, int n, int cus) {
  int best = 2;
  double best_score = -1.0;
  for (int i = 0; i < n; ++i) {
    const Cfg* t = table(i);
    const double tm = (double)cdiv64(M, t->bm), tn = (double)cdiv64(N, t->bn);
    const double useful = ((double)M * N) / (tm * t->bm * tn * t->bn);
    const double blocks = tm * tn, slots = (double)cus * occ[i];
    const double waves = (double)cdiv64((int64_t)blocks, (int64_t)slots);
    const double fill = blocks / (waves * slots);
    const double score = eff[i] * useful * fill;
    if (score > best_score) { best_score = score; best = i; }
  }
  return best;
}

// LDS-DMA tile ids: 0 256x256, 1 256x128, 2 128x128, 3 256x64, 4 128x64, 5 128x256.  Efficiency weights come from the
// measured table in DESIGN.md.
int pick_dma_tile(const tfimm_gemm_desc& d, int cus) {
  if (d.tile_hint > 10 && d.tile_hint <= 10 + TFIMM_GEMM_DMA_NUM_TILES) return d.tile_hint - 11;
  static const double eff[TFIMM_GEMM_DMA_NUM_TILES] = {1.00, 0.90, 0.70, 0.70, 0.50, 0.90};
  static const int occ[TFIMM_GEMM_DMA_NUM_TILES] = {1, 1, 2, 1, 3, 1};
  return best_tile(d.M, d.N, dma_tile_table, eff, occ, TFIMM_GEMM_DMA_NUM_TILES, cus);
}

// Persistent (stream) family: the DMA family's tile ids, then 6 256x64 (64x64 wave tiles), 7 deep ring, 8 256x32, 9 duo.
int pick_stream_tile(const tfimm_gemm_desc& d, const int* occ, int cus) {
  if (d.tile_hint > 20 && d.tile_hint <= 20 + TFIMM_GEMM_STREAM_NUM_TILES) return d.tile_hint - 21;
#ifdef TFIMM_PROBE_HOOKS
  // probe builds: TFIMM_GEMM_AUTO_TILE=k sends every launch WITHOUT a hint to stream tile k (0-based)
  const int forced = (int)env<ENV_AUTO_TILE>();
  if (forced >= 0 && forced < TFIMM_GEMM_STREAM_NUM_TILES && forced != 7) return forced;
#endif
  static const double eff[TFIMM_GEMM_STREAM_NUM_TILES] = {1.00, 0.90, 0.75, 0.70, 0.55, 0.90, 0.75, 0.0, 0.40, 0.0};
  return best_tile(d.M, d.N, stream_tile_table, eff, occ, TFIMM_GEMM_STREAM_NUM_TILES, cus);
}

// ---- step 1: everything that makes a descriptor TFIMM_EINVAL by itself
bool dense_vec(const tfimm_gemm_desc& d) { return ((d.lda & 7) == 0) && ((d.K & 7) == 0) && (((uintptr_t)d.a & 15) == 0); }
int64_t pad64(int64_t k) { return cdiv64(k, 64) * 64; }

int validate(const tfimm_gemm_desc& d) {
  if (!d.a || !d.wt || !d.out) TFIMM_FAIL(TFIMM_EINVAL, "gemm: null a/wt/out pointer");
  if (d.M <= 0 || d.N <= 0 || d.K <= 0) TFIMM_FAIL(TFIMM_EINVAL, "gemm: M=%d N=%d K=%d", d.M, d.N, d.K);
  if (d.ldw < d.K || (d.ldw & 7)) TFIMM_FAIL(TFIMM_EINVAL, "gemm: ldw=%d must be >= K=%d and a multiple of 8", d.ldw, d.K);
  if (((uintptr_t)d.wt & 15)) TFIMM_FAIL(TFIMM_EINVAL, "gemm: wt must be 16-byte aligned");
  if (d.ldc < d.N) TFIMM_FAIL(TFIMM_EINVAL, "gemm: ldc=%d < N=%d", d.ldc, d.N);
  if (d.mode < 0 || d.mode > 2) TFIMM_FAIL(TFIMM_EINVAL, "gemm: mode=%d", d.mode);
  if (d.remap_in < 0 || d.res_mod < 0) TFIMM_FAIL(TFIMM_EINVAL, "gemm: negative remap/res_mod");
  if (d.bias && ((uintptr_t)d.bias & 15)) TFIMM_FAIL(TFIMM_EINVAL, "gemm: bias must be 16-byte aligned");
  if ((d.ln_stats != nullptr) != (d.ln_c1 != nullptr)) TFIMM_FAIL(TFIMM_EINVAL, "gemm: ln_stats and ln_c1 go together");
  if (d.ln_stats && (d.mode != TFIMM_A_DENSE || d.residual || d.a_scale || d.out_f32 || (((uintptr_t)d.ln_stats | (uintptr_t)d.ln_c1) & 15)))
    TFIMM_FAIL(TFIMM_EINVAL, "gemm: LayerNorm folding needs a dense bf16 layer without residual / gate and 16-byte aligned tables");

  if (d.a2) {
    // second A operand (ABI v4): the shortcut convolution of a residual block as further k-tiles of this GEMM
    if ((d.mode != TFIMM_A_DENSE && d.mode != TFIMM_A_CONV) || d.residual || d.a_scale || d.ln_stats || d.out_f32 || d.remap_in || d.res_mod)
      TFIMM_FAIL(TFIMM_EINVAL, "gemm: a second A operand needs a bf16 layer (dense or TFIMM_A_CONV) without residual / gate / LayerNorm / row remap");
    if (d.K2 <= 0 || (d.K2 & 7) || d.lda2 < d.K2 || (d.lda2 & 7) || ((uintptr_t)d.a2 & 15))
      TFIMM_FAIL(TFIMM_EINVAL, "gemm: a2 needs K2=%d %% 8 == 0, lda2=%d >= K2 and %% 8 == 0, a 16-byte aligned pointer", d.K2, d.lda2);
    if (d.a2_stride < 1 || d.a2_window < 0 || d.a2_window > 4) TFIMM_FAIL(TFIMM_EINVAL, "gemm: a2_stride=%d a2_window=%d", d.a2_stride, d.a2_window);
    const int a2w = d.a2_window > 1 ? d.a2_window : 1;
    if (d.a2_stride > 1 || a2w > 1) {
      if (d.a2_H <= 0 || d.a2_W <= 0 || d.a2_OH <= 0 || d.a2_OW <= 0 || d.M % ((int64_t)d.a2_OH * d.a2_OW) ||
          (d.a2_OH - 1) * d.a2_stride + a2w > d.a2_H || (d.a2_OW - 1) * d.a2_stride + a2w > d.a2_W)
        TFIMM_FAIL(TFIMM_EINVAL, "gemm: a2 geometry %dx%d -> %dx%d at stride %d, window %d (M=%d)", d.a2_H, d.a2_W, d.a2_OH, d.a2_OW, d.a2_stride, a2w, d.M);
    }
    // the kernels read whole 64-wide k-tiles of every part, the last tap included (Extents::ldw_need)
    if (d.ldw < pad64(d.K) + (int64_t)(a2w * a2w) * pad64(d.K2))
      TFIMM_FAIL(TFIMM_EINVAL, "gemm: ldw=%d too small for K=%d + %d taps of K2=%d: wt holds K and every tap padded to whole 64-wide k-tiles (ldw >= %lld)",
                 d.ldw, d.K, a2w * a2w, d.K2, (long long)(pad64(d.K) + (int64_t)(a2w * a2w) * pad64(d.K2)));
  }

  if (d.mode == TFIMM_A_DENSE) {
    if (d.lda < d.K) TFIMM_FAIL(TFIMM_EINVAL, "gemm: lda=%d < K=%d", d.lda, d.K);
    if (d.a_scale && (!dense_vec(d) || d.rows_per_image <= 0 || ((uintptr_t)d.a_scale & 15)))
      TFIMM_FAIL(TFIMM_EINVAL, "gemm: a_scale needs aligned K %% 8 == 0 rows and rows_per_image > 0");
    return 0;
  }
  if (d.a_scale) TFIMM_FAIL(TFIMM_EINVAL, "gemm: a_scale only in dense mode");
  if (d.B <= 0 || d.H <= 0 || d.W <= 0 || d.KH <= 0 || d.KW <= 0 || d.stride <= 0 || d.OH <= 0 || d.OW <= 0)
    TFIMM_FAIL(TFIMM_EINVAL, "gemm: bad conv geometry");
  if ((int64_t)d.B * d.OH * d.OW != d.M) TFIMM_FAIL(TFIMM_EINVAL, "gemm: M != B*OH*OW");
  if (((uintptr_t)d.a & 15)) TFIMM_FAIL(TFIMM_EINVAL, "gemm: conv input must be 16-byte aligned");
  if (d.mode == TFIMM_A_CONV) {
    if (d.K != d.KH * d.KW * d.Cin) TFIMM_FAIL(TFIMM_EINVAL, "gemm: K != KH*KW*Cin");
    if (d.pix_pitch < 0 || (d.pix_pitch > 0 && d.pix_pitch < d.Cin)) TFIMM_FAIL(TFIMM_EINVAL, "gemm: pix_pitch=%d < Cin=%d", d.pix_pitch, d.Cin);
  } else {
    if (d.Cin != 4 || d.pix_pitch > 4) TFIMM_FAIL(TFIMM_EINVAL, "gemm: C4 mode needs Cin == 4 (and no pixel pitch)");
    if (d.K != d.KH * ((d.KW + 1) & ~1) * 4) TFIMM_FAIL(TFIMM_EINVAL, "gemm: K != KH*KWp*4 (K=%d)", d.K);
  }
  return 0;
}

// ---- step 2: a plain dense GEMM whose activation, output or residual exceeds 2 GiB (EfficientNet-B4's first expand layer at
// batch 256: 9.2 M rows x 144 channels) is run as row chunks that each fit kMaxBytes, instead of leaving the LDS-DMA families.
// Rows per chunk, 0 when the descriptor runs as it is.  TFIMM_GEMM_LIMIT (bytes, read once) stands in for kMaxBytes here and
// only here, so that a test can run the chunking on a small tensor (tests/test_gpu_gemm_contract.py).
int64_t chunk_rows(const tfimm_gemm_desc& d) {
  if (d.mode != TFIMM_A_DENSE || d.a_scale || d.a2 || d.remap_in != 0 || d.res_mod != 0) return 0;
  const int64_t row_bytes = std::max<int64_t>({(int64_t)d.lda * 2, (int64_t)d.ldc * (d.out_f32 ? 4 : 2), d.residual ? (int64_t)d.ldr * 2 : 0});
  const int64_t limit = std::min<int64_t>(std::max<int64_t>(env<ENV_LIMIT>(), 1), kMaxBytes);   // TFIMM_GEMM_LIMIT lowers the threshold only
  if (row_bytes <= 0 || (int64_t)d.M * row_bytes <= limit || row_bytes * 512 > limit) return 0;
  return (limit / row_bytes) / 256 * 256;
}

int run_chunks(const tfimm_gemm_desc& d, int64_t chunk, void* stream) {
  for (int64_t m0 = 0; m0 < d.M; m0 += chunk) {
    tfimm_gemm_desc c = d;
    c.M = (int32_t)std::min<int64_t>(chunk, d.M - m0);
    c.a = (const char*)d.a + m0 * d.lda * 2;
    c.out = (char*)d.out + m0 * d.ldc * (d.out_f32 ? 4 : 2);
    if (d.residual) c.residual = (const char*)d.residual + m0 * d.ldr * 2;
    if (d.ln_stats) c.ln_stats = d.ln_stats + m0 * 2;
    if (int rc = tfimm_hip_gemm(&c, stream)) return rc;
  }
  return 0;
}

// ---- step 3: operand flavour, epilogue flavour, buffer extents, the kernel arguments every family shares
struct Extents {   // bytes of every buffer as the kernels address it (the bounds of the LDS-DMA families' buffer descriptors)
  int64_t a_bytes, w_bytes, out_bytes, res_bytes, a2_bytes, s_bytes;   // s: the SE-gate table
  int a2win;         // taps per side of the second operand's window (1: a 1x1 view)
  int64_t ldw_need;  // weight pitch the LDS-DMA kernels read: whole 64-wide k-tiles of K and of each of the a2win^2 taps of K2
};
struct Class {
  int kmode;        // K_* of gemm_kernel.h
  int fi, vi, ei;   // LDS-DMA families: operand kind (0 K_DENSE and the SE gate, 1 K_CONV); vector epilogue (whole 16-byte groups per lane on
                    // aligned rows); epilogue flavour (0 catch-all, 1 vector, 2 vector without residual: arithmetic in the accumulator layout)
  bool scale, dual, ln_in;
  Extents x;
  GemmArgs g;       // (tiles_m / tiles_n: the route's)
};

Class classify(const tfimm_gemm_desc& d) {
  Class c;
  GemmArgs& g = c.g;
  g.a = (const bf16_t*)d.a; g.wt = (const bf16_t*)d.wt; g.bias = d.bias;
  g.residual = (const bf16_t*)d.residual; g.out = d.out; g.a_scale = d.a_scale;
  g.M = d.M; g.N = d.N; g.K = d.K; g.lda = d.lda; g.ldw = d.ldw; g.ldr = d.ldr; g.ldc = d.ldc;
  g.out_f32 = d.out_f32; g.act = d.act; g.act_after_res = d.act_after_res; g.res_mod = d.res_mod;
  g.remap_in = d.remap_in; g.remap_out = d.remap_out; g.remap_off = d.remap_off;
  g.B = d.B; g.H = d.H; g.W = d.W; g.Cin = d.Cin; g.KH = d.KH; g.KW = d.KW; g.KWp = (d.KW + 1) & ~1;
  g.stride = d.stride; g.pad_t = d.pad_t; g.pad_l = d.pad_l; g.OH = d.OH; g.OW = d.OW; g.rows_per_image = d.rows_per_image;
  g.stride_w = d.stride_w > 0 ? d.stride_w : d.stride;
  g.cpitch = d.pix_pitch > 0 ? d.pix_pitch : d.Cin;
  g.res_vec = d.residual ? (((d.ldr & 3) == 0) && (((uintptr_t)d.residual & 7) == 0)) : 0;
  g.res_vec16 = d.residual ? (((d.ldr & 7) == 0) && (((uintptr_t)d.residual & 15) == 0)) : 0;
  g.out_vec16 = ((d.ldc & 7) == 0) && (((uintptr_t)d.out & 15) == 0);
  g.out_vec = ((d.ldc & 3) == 0) && (((uintptr_t)d.out & (d.out_f32 ? 15 : 7)) == 0);
  g.tiles_m = g.tiles_n = 0;

  if (d.mode == TFIMM_A_DENSE) c.kmode = d.a_scale ? K_DENSE_SCALE : dense_vec(d) ? K_DENSE : K_DENSE_SCALAR;
  else if (d.mode == TFIMM_A_CONV) c.kmode = ((d.Cin | g.cpitch) & 7) ? K_CONV_SCALAR : K_CONV;  // odd channel counts: element loads
  else c.kmode = K_CONV_C4;
  c.scale = c.kmode == K_DENSE_SCALE; c.dual = d.a2 != nullptr; c.ln_in = d.ln_stats != nullptr;
  c.fi = c.kmode == K_CONV ? 1 : 0;
  c.vi = ((d.N % 8) == 0 && !d.out_f32 && g.out_vec16 && (!d.residual || g.res_vec16) &&
          (d.res_mod == 0 || d.res_mod >= 128) && (d.remap_in == 0 || d.remap_in >= 128)) ? 1 : 0;
  c.ei = c.vi ? (d.residual ? 1 : 2) : 0;
  Extents& x = c.x;
  x.a_bytes = (d.mode == TFIMM_A_DENSE ? (int64_t)(d.M - 1) * d.lda + d.K : ((int64_t)d.B * d.H * d.W - 1) * g.cpitch + d.Cin) * 2;
  x.w_bytes = (int64_t)d.N * d.ldw * 2;
  // output / residual as the epilogue addresses them (row remap included)
  const int64_t out_rows = d.remap_in > 0 ? ((int64_t)(d.M - 1) / d.remap_in) * d.remap_out + d.remap_in + d.remap_off : d.M;
  x.out_bytes = ((out_rows - 1) * d.ldc + d.N) * (d.out_f32 ? 4 : 2);
  const int64_t res_rows = d.res_mod > 0 ? (d.res_mod < d.M ? d.res_mod : d.M) : d.M;
  x.res_bytes = d.residual ? ((res_rows - 1) * d.ldr + d.N) * 2 : 0;
  x.a2win = d.a2_window > 1 ? d.a2_window : 1;
  const int64_t a2_rows = !c.dual ? 0 : (d.a2_stride > 1 || x.a2win > 1) ? (int64_t)(d.M / ((int64_t)d.a2_OH * d.a2_OW)) * d.a2_H * d.a2_W : d.M;
  x.a2_bytes = c.dual ? ((a2_rows - 1) * d.lda2 + d.K2) * 2 : 0;
  x.s_bytes = c.scale ? cdiv64(d.M, d.rows_per_image) * d.K * 4 : 0;
  x.ldw_need = pad64(d.K) + (c.dual ? (int64_t)x.a2win * x.a2win * pad64(d.K2) : 0);
  return c;
}

// ---- step 4: the route
enum Family { F_STRIP, F_STREAM, F_DMA, F_REG };
struct Route {
  Family family;
  int tile, tiles_m, tiles_n, threads;
  union { gemm_stream_fn stream; gemm_dma_fn dma; gemm_fn reg; } fn;   // the member of `family` (F_STRIP: conv_strip.hip has its one kernel and grid)
  int64_t grid;
  size_t lds;          // dynamic LDS bytes of the launch
  tfimm_once_t* attr;  // set_attr_once(fn, attr_lds) goes before the launch; nullptr: the kernel needs none here
  int attr_lds;
  int s_slots, s_gp;   // SE gate on the stream family: image slots per row tile, 1-KiB DMA pieces per k-tile
};

// what both LDS-DMA families ask of the operands: weights padded to 64 in k, tensors addressable with a 31-bit byte offset
bool lds_dma_operands(const tfimm_gemm_desc& d, const Class& c) { return d.ldw >= c.x.ldw_need && c.x.a_bytes <= kMaxBytes && c.x.w_bytes <= kMaxBytes; }

// 3x3 / stride 1 / pad 1, 128 -> 128 channels, rows of at most 31 pixels (ResNet-50 stage 2): the input-strip kernel
// (csrc/conv_strip.hip).  Tile hint 31 asks for it; hint 0 takes it unless TFIMM_STRIP_CONV=0 -- and only when its fixed
// 128-pixel x 128-channel tiles give every CU at least one (M >= 128 CUs: it was measured at 28 x 28 and batch >= 6;
// below that the 128 x 64 / 256 x 32 implicit-GEMM tiles make more workgroups and the cost model decides); any other
// hint keeps the implicit-GEMM tiles (the tuner's candidates).  tfimm/engine/tune.py strip_shape mirrors the shape part.
bool conv_strip_applies(const tfimm_gemm_desc& d, const Class& c, const Device& dv) {
  const GemmArgs& g = c.g;
  return c.kmode == K_CONV && d.KH == 3 && d.KW == 3 && d.stride == 1 && g.stride_w == 1 && d.pad_t == 1 && d.pad_l == 1 && d.OH == d.H &&
         d.OW == d.W && d.Cin == 128 && g.cpitch == 128 && d.N == 128 && !d.residual && !d.out_f32 && g.out_vec16 && d.remap_in == 0 &&
         !d.ln_stats && !d.a2 && d.W <= 31 && d.ldw >= d.K &&
         (d.tile_hint == 31 || (d.tile_hint == 0 && env<ENV_STRIP_CONV>() != 0 && cdiv64(d.M, 128) >= dv.num_cu)) &&
         c.x.a_bytes <= kMaxBytes && c.x.w_bytes <= kMaxBytes && c.x.out_bytes <= kMaxBytes;
}

// persistent LDS-DMA family (default).  A hint for another family (1..20) keeps a layer off it -- unless only this family has
// the layer's kernel: a second A operand, a folded LayerNorm, a horizontal stride of its own.
bool stream_applies(const tfimm_gemm_desc& d, const Class& c) {
  const bool hinted_other = d.tile_hint > 0 && d.tile_hint <= 20 && c.g.stride_w == c.g.stride && !d.ln_stats;
  return (c.kmode == K_DENSE || c.kmode == K_CONV || c.scale) && (!hinted_other || c.dual) && !env<ENV_NO_STREAM>() && !env<ENV_NO_DMA>() &&
         lds_dma_operands(d, c) && c.x.out_bytes <= kMaxBytes && c.x.res_bytes <= kMaxBytes && c.x.a2_bytes <= kMaxBytes &&
         (!c.dual || c.kmode == K_DENSE || c.kmode == K_CONV);
}

// one-tile-per-workgroup LDS-DMA family: aligned dense rows or Cin % 8 == 0 gathers; hints 1..6 name a register-staged tile
bool dma_applies(const tfimm_gemm_desc& d, const Class& c) {
  const bool hint_v1 = d.tile_hint > 0 && d.tile_hint <= TFIMM_GEMM_NUM_TILES;  // 11..16 = this family
  return (c.kmode == K_DENSE || c.kmode == K_CONV) && !hint_v1 && !env<ENV_NO_DMA>() && lds_dma_operands(d, c);
}

int set_tiles(Route* r, const tfimm_gemm_desc& d, int bm, int bn, int64_t* ntiles) {
  r->tiles_m = (int)cdiv64(d.M, bm); r->tiles_n = (int)cdiv64(d.N, bn);
  *ntiles = (int64_t)r->tiles_m * r->tiles_n;
  if (*ntiles > 0x7fffffffLL) TFIMM_FAIL(TFIMM_EINVAL, "gemm: grid too large");
  return 0;
}

// a persistent grid: occ workgroups on every CU, whole groups of 8 (one per XCD), no more than the tiles need
int64_t persistent_grid(int cus, int occ, int64_t ntiles) { return std::min<int64_t>(((int64_t)cus * occ + 7) / 8 * 8, (ntiles + 7) / 8 * 8); }

// Tile, flavour and grid on the stream family.  Leaves r->fn.stream null when an SE-gate layer has to go to the register-staged family.
int route_stream(const tfimm_gemm_desc& d, const Class& c, Device& dv, Route* r) {
  if (int rc = stream_occupancy(dv)) return rc;
  const int* occ = dv.occ[c.fi];
  int ti = pick_stream_tile(d, occ, dv.num_cu);
  // the two-workgroups-per-CU tile: vector epilogues only, at least two 32-wide k-tiles; otherwise the 256x128 stream tile
  if (ti == 9 && (c.ei == 0 || d.K <= 32 || c.scale || c.dual)) ti = 1;
  const StreamTileCfg* t = stream_tile_table(ti);
  bool has_flavour = !c.scale || t->fn_scale[c.ei];   // the deep-ring tile has no SE-gate flavour
  if (c.dual) {
    if (c.ei != 2) TFIMM_FAIL(TFIMM_EUNSUP, "gemm: a second A operand needs N %% 8 == 0 and 16-byte aligned bf16 output rows");
    has_flavour = has_flavour && t->fn_dual[c.fi];
  }
  if (c.ln_in) {
    if (c.ei != 2 || c.fi != 0 || c.scale)
      TFIMM_FAIL(TFIMM_EUNSUP, "gemm: LayerNorm folding needs dense bf16 rows, N %% 8 == 0, 16-byte aligned output, no residual");
    has_flavour = has_flavour && t->fn_ln && (size_t)t->lds_bytes + t->ln_lds <= kMaxLds;
  }
  if (!has_flavour) t = stream_tile_table(ti = 0);   // the 256x256 stream tile has every flavour
  int64_t ntiles;
  if (int rc = set_tiles(r, d, t->bm, t->bn, &ntiles)) return rc;
  r->family = F_STREAM; r->tile = ti; r->threads = t->threads;
  r->lds = (size_t)t->lds_bytes;
  r->grid = persistent_grid(dv.num_cu, occ[ti], ntiles);
  if (c.ln_in) {
    r->lds += t->ln_lds;
    if (dv.ln_ready[ti].need()) {
      if (int rc = query_occupancy((const void*)t->fn_ln, t->threads, r->lds, &dv.ln_occ[ti])) return rc;
      dv.ln_ready[ti].mark();
    }
    r->grid = persistent_grid(dv.num_cu, dv.ln_occ[ti], ntiles);
    r->fn.stream = t->fn_ln;
  } else if (c.dual) {
    r->fn.stream = t->fn_dual[c.fi];
    r->attr = &g_attr[ATTR_STREAM_DUAL][ti][c.fi]; r->attr_lds = t->lds_bytes;
  } else if (!c.scale) {
    r->fn.stream = t->fn[c.fi][c.ei];
  } else {
    // SE gate on A: per k-tile, 64 gate values of every image a row tile touches ride in LDS next to the operand stage
    // (1 KiB per four image slots and stage; wave w brings piece w)
    r->s_slots = (int)cdiv64(t->bm, d.rows_per_image) + 1;
    r->s_gp = (r->s_slots + 3) / 4;
    r->lds += (size_t)2 * r->s_gp * 1024;
    // more image slots per tile than waves to bring them (images of a few rows): the register-staged family
    if (r->s_gp > t->threads / 64 || r->lds > kMaxLds || c.x.s_bytes > kMaxBytes) return 0;
    // resident workgroups per CU with the gate slices counted in
    const int occ_s = std::max(1, std::min((int)(kMaxLds / r->lds), occ[ti]));
    r->grid = persistent_grid(dv.num_cu, occ_s, ntiles);
    r->fn.stream = t->fn_scale[c.ei];
    r->attr = &g_attr[ATTR_STREAM_SCALE][ti][c.ei]; r->attr_lds = (int)kMaxLds;
  }
  return 0;
}

int route(const tfimm_gemm_desc& d, const Class& c, Device& dv, Route* r) {
  *r = Route{F_STRIP};
  if (conv_strip_applies(d, c, dv)) return 0;
  if (stream_applies(d, c)) {
    if (int rc = route_stream(d, c, dv, r)) return rc;
    if (r->fn.stream) return 0;
  }
  if (d.ln_stats) TFIMM_FAIL(TFIMM_EUNSUP, "gemm: LayerNorm folding needs the persistent LDS-DMA family (K-padded weights, 16-byte aligned rows)");
  if (d.a2) TFIMM_FAIL(TFIMM_EUNSUP, "gemm: a second A operand needs the persistent LDS-DMA family (channel counts %% 8 == 0, K-padded weights, 16-byte aligned rows)");
  if (d.mode != TFIMM_A_DENSE && c.g.stride_w != c.g.stride)
    TFIMM_FAIL(TFIMM_EUNSUP, "gemm: stride_w != stride needs the persistent LDS-DMA family (Cin %% 8 == 0, 16-byte aligned input)");
  *r = Route{};
  int bm, bn;
  if (dma_applies(d, c)) {
    r->family = F_DMA;
    r->tile = pick_dma_tile(d, dv.num_cu);
    const DmaTileCfg* t = dma_tile_table(r->tile);
    bm = t->bm; bn = t->bn; r->threads = t->threads;
    r->lds = (size_t)(bm + bn) * 128 * 2;
    r->fn.dma = t->fn[c.fi];
    r->attr = &g_attr[ATTR_DMA][r->tile][c.fi];
  } else {
    r->family = F_REG;
    r->tile = pick_tile(d, c.kmode, dv.num_cu);
    if (!tile_table(r->tile)->fn[c.kmode]) {  // flavour not built for the picked tile: fall back to 64x64 / 128x64
      r->tile = c.scale ? 1 : 2;
      if (!tile_table(r->tile)->fn[c.kmode]) TFIMM_FAIL(TFIMM_EUNSUP, "gemm: no kernel for flavour %d", c.kmode);
    }
    const TileCfg* t = tile_table(r->tile);
    bm = t->bm; bn = t->bn; r->threads = t->threads;
    r->lds = (size_t)(bm + bn) * BK * 2 * 2;
    r->fn.reg = t->fn[c.kmode];
    r->attr = &g_attr[ATTR_REG][r->tile][c.kmode];
  }
  r->attr_lds = (int)r->lds;
  return set_tiles(r, d, bm, bn, &r->grid);   // one workgroup per tile
}

// ---- step 5: kernel arguments and launch
GemmStreamArgs stream_args(const tfimm_gemm_desc& d, const Class& c, const Route& r, const Device& dv, const GemmArgs& g) {
  GemmStreamArgs ga;
  ga.g = g;
  ga.a_bytes = (unsigned)c.x.a_bytes; ga.w_bytes = (unsigned)c.x.w_bytes;
  ga.out_bytes = (unsigned)c.x.out_bytes; ga.res_bytes = (unsigned)c.x.res_bytes;
  ga.n_tiles = r.tiles_m * r.tiles_n;
  // column-panel groups (GemmStreamArgs::ngroup).  TFIMM_GEMM_NGROUP: -1 (default) = the rule below, 0 = never, n = groups of n
  const int ng_env = (int)env<ENV_NGROUP>();
  int ng = ng_env > 0 ? ng_env : 0;
  if (ng_env < 0 && c.kmode == K_DENSE && !c.scale && c.x.w_bytes > (int64_t)(3 << 20) && r.tiles_m >= 64) {
    // as many weight panels as stay in one XCD's L2 next to the streaming rows: 5/8 of it (4 MiB on MI355X -> 2.5 MB;
    // ViT-B, K = 768, 256-column panels of 393 KB: groups of 6 -- measured -0.9 .. -1.1 % of a ViT-B step on three boxes;
    // 5, 7, 8 and the half split of 9 panels gain 0.2 .. 0.6 %, groups of 2 LOSE 2 %: A is re-read once per group).
    // Dense rows only (plain and LayerNorm-folded -- both ViT-B flavours were in that measurement): an implicit-GEMM
    // convolution re-gathers A per group and the SE-gate flavour re-scales it; their table entries were timed in
    // M-panel-major order.
    const int64_t panel = (int64_t)stream_tile_table(r.tile)->bn * d.ldw * 2;
    ng = (int)(dv.l2_budget / (panel > 0 ? panel : 1));
    if (ng < 3) ng = 0;
  }
  ga.ngroup = (ng > 0 && ng < r.tiles_n) ? ng : 0;
  ga.cin64 = (c.kmode == K_CONV && (d.Cin % (r.tile == 9 ? 32 : 64)) == 0) ? 1 : 0;   // whole k-tiles inside one filter tap
  ga.cin_magic = ga.kw_magic = 0;
  if (c.kmode == K_CONV && d.K < 65536) {
    if (d.Cin > 1) ga.cin_magic = (unsigned)(0x100000000ULL / (unsigned)d.Cin) + 1u;
    if (d.KW > 1) ga.kw_magic = (unsigned)(0x100000000ULL / (unsigned)d.KW) + 1u;
  }
  ga.duo_delay = 0; ga.duo_first = dv.num_cu / 8;
  if (r.tile == 9) {
    // phase shift of the second workgroup of a CU: about half a tile (a k-tile is 16 MFMAs = 512 cycles of one wave)
    const int c1 = (int)env<ENV_DUO_DELAY_K>(), c0 = (int)env<ENV_DUO_DELAY_0>();
    ga.duo_delay = (c1 == 0 && c0 == 0) ? 0 : (int)std::min<int64_t>(cdiv64(d.K, 32) * c1 + c0, 200000);
  }
  ga.dbg = (int)env<ENV_DBG>(); ga.dbg_ptr = (long long*)env<ENV_DBG_PTR>();
  ga.s_bytes = (unsigned)c.x.s_bytes; ga.s_slots = r.s_slots; ga.s_gp = r.s_gp;
  ga.a2 = (const bf16_t*)d.a2; ga.a2_bytes = (unsigned)c.x.a2_bytes; ga.a2_window = c.x.a2win;
  ga.K2 = d.K2; ga.lda2 = d.lda2; ga.a2_stride = d.a2_stride; ga.a2_H = d.a2_H; ga.a2_W = d.a2_W; ga.a2_OH = d.a2_OH; ga.a2_OW = d.a2_OW;
  ga.ln_stats = d.ln_stats; ga.ln_c1 = d.ln_c1;
  ga.ln_stats_bytes = c.ln_in ? (unsigned)((int64_t)d.M * 8) : 0u;
  ga.ln_c1_bytes = c.ln_in ? (unsigned)((int64_t)d.N * 32) : 0u;
  return ga;
}

int launch(const Route& r, const tfimm_gemm_desc& d, const Class& c, const Device& dv, hipStream_t stream) {
  if (r.family == F_STRIP) return tfimm_launch_conv_strip(c.g, c.x.a_bytes, c.x.w_bytes, c.x.out_bytes, dv.num_cu, stream);
  const void* fn = r.family == F_STREAM ? (const void*)r.fn.stream : r.family == F_DMA ? (const void*)r.fn.dma : (const void*)r.fn.reg;
  if (int rc = r.attr ? set_attr_once(*r.attr, fn, r.attr_lds) : 0) return rc;
  const dim3 grid((unsigned)r.grid), block(r.threads);
  GemmArgs g = c.g;
  g.tiles_m = r.tiles_m; g.tiles_n = r.tiles_n;
  if (r.family == F_STREAM) {
    const GemmStreamArgs ga = stream_args(d, c, r, dv, g);
    TFIMM_LAUNCH(r.fn.stream, grid, block, r.lds, stream, ga);
  } else if (r.family == F_DMA) {
    const GemmDmaArgs ga = {g, (unsigned)c.x.a_bytes, (unsigned)c.x.w_bytes};
    TFIMM_LAUNCH(r.fn.dma, grid, block, r.lds, stream, ga);
  } else {
    TFIMM_LAUNCH(r.fn.reg, grid, block, r.lds, stream, g);
  }
  return 0;
}

}  // namespace

extern "C" int tfimm_hip_gemm(const tfimm_gemm_desc* dp, void* stream) {
  if (!dp) TFIMM_FAIL(TFIMM_EINVAL, "gemm: null descriptor");
  const tfimm_gemm_desc& d = *dp;
  if (int rc = validate(d)) return rc;
  if (const int64_t rows = chunk_rows(d)) return run_chunks(d, rows, stream);
  const Class c = classify(d);
  Device& dv = device();
  Route r;
  if (int rc = route(d, c, dv, &r)) return rc;
  return launch(r, d, c, dv, (hipStream_t)stream);
}

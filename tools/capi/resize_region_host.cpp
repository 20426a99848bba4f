// Stand-alone host over tfimm_hip_resize_region_tables (csrc/resize_regions.hip) for a sanitizer run of the builder of records
// and table arenas of boxes inside larger frames: no GPU is touched, nothing is launched.  Build the translation units' host
// side with the sanitizers and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tensorflow-image-models_amd/csrc/resize.hip \
//         tensorflow-image-models_amd/csrc/resize_aa.hip tensorflow-image-models_amd/csrc/resize_batch.hip \
//         tensorflow-image-models_amd/csrc/resize_regions.hip tools/capi/resize_region_host.cpp -o resize_region_host \
//         && ./resize_region_host
// Every output array is allocated at exactly the size the sizing call asked for, so a write past a box's tables is a heap
// overflow the sanitizer reports.  The boxes are those of tests/test_gpu_regions.py.  Tables and records are compared with what
// tfimm_hip_resize_batch_tables gives for images of the boxes' sizes, the two addressing fields with their formula; a refused
// call must leave sizes, records and tables as they were.  Prints the number of sets checked; exit status 0 = clean.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/tfimm_hip.h"

// the library's error plumbing lives in another translation unit
void tfimm_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  va_end(ap);
}

struct Box {
  int frame, y0, x0, y1, x1, Rh, Rw, top, left;
};

static const int32_t FRAMES[] = {37, 53, 64, 41, 210, 40};
static const std::vector<Box> CASES = {
    {0, 3, 5, 20, 31, 18, 25, 1, 4},   {1, 0, 7, 30, 33, 25, 18, 4, 1},   {0, 15, 9, 37, 40, 18, 18, 1, 1},
    {1, 11, 0, 50, 19, 16, 20, 0, 2},  {0, 5, 22, 29, 53, 16, 16, 0, 0},  {1, 40, 20, 64, 41, 18, 25, 1, 4},
    {0, 0, 0, 37, 53, 18, 25, 1, 4},   {1, 10, 10, 11, 11, 16, 16, 0, 0}, {2, 5, 20, 205, 32, 16, 16, 0, 0},
    {0, 2, 17, 35, 18, 18, 18, 1, 1},  {1, 33, 4, 34, 39, 16, 20, 0, 2},  {0, 8, 8, 28, 38, 18, 25, 1, 4},
    {0, 12, 14, 34, 44, 25, 18, 4, 1}, {1, 20, 5, 45, 30, 18, 18, 1, 1},  {1, 20, 5, 45, 30, 18, 18, 1, 1}};

static int check_set(const std::vector<Box>& bs, int F, int H, int W, int c_in, const int32_t* pad, int method, int aa) {
  const int N = (int)bs.size();
  std::vector<int32_t> boxes(4 * N), frame(N), geo(4 * N), hw(2 * N);
  for (int n = 0; n < N; ++n) {
    const Box& b = bs[n];
    boxes[4 * n] = b.y0, boxes[4 * n + 1] = b.x0, boxes[4 * n + 2] = b.y1, boxes[4 * n + 3] = b.x1;
    frame[n] = b.frame;
    geo[4 * n] = b.Rh, geo[4 * n + 1] = b.Rw, geo[4 * n + 2] = b.top, geo[4 * n + 3] = b.left;
    hw[2 * n] = b.y1 - b.y0, hw[2 * n + 1] = b.x1 - b.x0;
  }
  tfimm_resize_batch_sizes need, again, packed;
  if (tfimm_hip_resize_region_tables(F, FRAMES, N, boxes.data(), frame.data(), geo.data(), H, W, c_in, pad, method, aa, &need,
                                     nullptr, nullptr, nullptr, nullptr) != 0)
    return 1;
  std::vector<tfimm_resize_region_rec> recs(N);
  std::vector<int32_t> ta((size_t)need.tab_elems), tb(aa ? (size_t)need.tab_elems : 0);
  std::vector<float> w((size_t)need.w_floats);
  if (tfimm_hip_resize_region_tables(F, FRAMES, N, boxes.data(), frame.data(), geo.data(), H, W, c_in, pad, method, aa, &again,
                                     recs.data(), ta.data(), aa ? tb.data() : nullptr, w.data()) != 0)
    return 1;
  if (std::memcmp(&need, &again, sizeof need) != 0 || need.bad_image != -1) return 1;
  // the slices as images of their own
  if (tfimm_hip_resize_batch_tables(N, hw.data(), geo.data(), H, W, c_in, pad, method, aa, &packed, nullptr, nullptr, nullptr,
                                    nullptr) != 0)
    return 1;
  if (packed.tab_elems != need.tab_elems || packed.w_floats != need.w_floats || packed.n_tiles != need.n_tiles ||
      packed.max_taps != need.max_taps || packed.lds_floats != need.lds_floats)
    return 1;
  std::vector<tfimm_resize_batch_rec> precs(N);
  std::vector<int32_t> pa((size_t)packed.tab_elems), pb(aa ? (size_t)packed.tab_elems : 0);
  std::vector<float> pw((size_t)packed.w_floats);
  if (tfimm_hip_resize_batch_tables(N, hw.data(), geo.data(), H, W, c_in, pad, method, aa, &packed, precs.data(), pa.data(),
                                    aa ? pb.data() : nullptr, pw.data()) != 0)
    return 1;
  if (std::memcmp(pa.data(), ta.data(), pa.size() * 4) || std::memcmp(pw.data(), w.data(), pw.size() * 4)) return 1;
  if (aa && std::memcmp(pb.data(), tb.data(), pb.size() * 4)) return 1;
  std::vector<int64_t> frame_off(F);
  int64_t in_bytes = 0;
  for (int f = 0; f < F; ++f) {
    frame_off[f] = in_bytes;
    in_bytes += (int64_t)FRAMES[2 * f] * FRAMES[2 * f + 1] * c_in;
  }
  if (need.in_bytes != in_bytes) return 1;
  for (int n = 0; n < N; ++n) {
    const tfimm_resize_region_rec& r = recs[n];
    const tfimm_resize_batch_rec& p = precs[n];
    const int64_t Wf = FRAMES[2 * bs[n].frame + 1];
    if (r.in_offset != frame_off[bs[n].frame] + ((int64_t)bs[n].y0 * Wf + bs[n].x0) * c_in || r.row_pitch != Wf * c_in) return 1;
    if (r.Hs != p.Hs || r.Ws != p.Ws || r.y_tab != p.y_tab || r.x_tab != p.x_tab || r.y_w != p.y_w || r.x_w != p.x_w ||
        r.y_taps != p.y_taps || r.x_taps != p.x_taps || r.tile_rows != p.tile_rows || r.cols_max != p.cols_max ||
        r.tile0 != p.tile0 || r.n_tiles != p.n_tiles)
      return 1;
    // the last pixel of the box lies inside the arena
    if (r.in_offset + (int64_t)(r.Hs - 1) * r.row_pitch + (int64_t)r.Ws * c_in > in_bytes) return 1;
  }
  return 0;
}

// a refused call: the invalid-argument code, and sizes, records and tables as they were
static int check_refused(const std::vector<Box>& bs, int F, int method, int aa, int want_bad) {
  const int N = (int)bs.size();
  std::vector<int32_t> boxes(4 * N), frame(N), geo(4 * N);
  for (int n = 0; n < N; ++n) {
    const Box& b = bs[n];
    boxes[4 * n] = b.y0, boxes[4 * n + 1] = b.x0, boxes[4 * n + 2] = b.y1, boxes[4 * n + 3] = b.x1;
    frame[n] = b.frame;
    geo[4 * n] = b.Rh, geo[4 * n + 1] = b.Rw, geo[4 * n + 2] = b.top, geo[4 * n + 3] = b.left;
  }
  tfimm_resize_batch_sizes s;
  std::memset(&s, 0x5a, sizeof s);
  const tfimm_resize_batch_sizes before = s;
  std::vector<tfimm_resize_region_rec> recs(N);
  std::memset(recs.data(), 0x5a, recs.size() * sizeof recs[0]);
  const std::vector<tfimm_resize_region_rec> recs_before = recs;
  std::vector<int32_t> ta((size_t)N * 32 * 4, 0x5a5a5a5a), tb = ta;
  std::vector<float> w((size_t)N * 32 * TFIMM_RESIZE_AA_MAX_TAPS, 7.f);
  const std::vector<int32_t> ta_before = ta;
  const std::vector<float> w_before = w;
  const int rc = tfimm_hip_resize_region_tables(F, FRAMES, N, boxes.data(), frame.data(), geo.data(), 16, 16, 3, nullptr, method,
                                                aa, &s, recs.data(), ta.data(), tb.data(), w.data());
  if (rc != TFIMM_EINVAL) return 1;
  if (want_bad < 0 ? std::memcmp(&s, &before, sizeof s) != 0 : s.bad_image != want_bad) return 1;
  return std::memcmp(recs.data(), recs_before.data(), recs.size() * sizeof recs[0]) != 0 || ta != ta_before || tb != ta_before ||
         w != w_before;
}

int main() {
  std::vector<Box> rev(CASES.rbegin(), CASES.rend()), first_frame, many;
  for (const Box& b : CASES)
    if (b.frame == 0) first_frame.push_back(b);
  for (int i = 0; i < 4200; ++i) many.push_back(first_frame[i % first_frame.size()]);
  const std::vector<Box> big = {{2, 3, 0, 203, 40, 44, 80, 2, 4}, {0, 1, 2, 36, 51, 40, 72, 0, 0}, {1, 9, 3, 60, 40, 48, 76, 5, 1}};
  const int32_t pads[][4] = {{0, 0, 0, 0}, {3, 3, 3, 3}, {0, 1, 0, 1}, {3, 2, 3, 2}};
  int n = 0, bad = 0;
  for (int method = 0; method < 2; ++method)
    for (int aa = 0; aa < 2; ++aa) {
      for (const auto& pad : pads) {
        bad += check_set(CASES, 3, 16, 16, 3, pad, method, aa), ++n;
        bad += check_set(big, 3, 40, 72, 3, pad, method, aa), ++n;
      }
      bad += check_set(CASES, 3, 16, 16, 3, nullptr, method, aa), ++n;
      bad += check_set(rev, 3, 16, 16, 3, nullptr, method, aa), ++n;
      for (int c_in : {1, 4, 8}) bad += check_set(CASES, 3, 16, 16, c_in, nullptr, method, aa), ++n;
      bad += check_set(first_frame, 1, 16, 16, 3, nullptr, method, aa), ++n;      // one frame of the three
      bad += check_set(many, 1, 16, 16, 3, nullptr, method, aa), ++n;
      // refusals: a box one row past its frame, left of it, in the other frame's size, empty, inverted, no such frame
      const Box ok = CASES[0];
      bad += check_refused({ok, {0, 5, 5, 38, 20, 18, 18, 1, 1}}, 3, method, aa, -1), ++n;
      bad += check_refused({ok, {0, 0, -1, 10, 10, 18, 18, 1, 1}}, 3, method, aa, -1), ++n;
      bad += check_refused({{1, 0, 0, 10, 42, 18, 18, 1, 1}}, 3, method, aa, -1), ++n;
      bad += check_refused({ok, {1, 4, 4, 4, 9, 18, 18, 1, 1}}, 3, method, aa, -1), ++n;
      bad += check_refused({ok, {1, 9, 9, 4, 12, 18, 18, 1, 1}}, 3, method, aa, -1), ++n;
      bad += check_refused({ok, {3, 0, 0, 10, 10, 18, 18, 1, 1}}, 3, method, aa, -1), ++n;
      bad += check_refused({ok, {-1, 0, 0, 10, 10, 18, 18, 1, 1}}, 3, method, aa, -1), ++n;
      bad += check_refused({ok, {2, 0, 0, 10, 10, 18, 18, 1, 1}}, 2, method, aa, -1), ++n;   // frame 2 of 2 frames
      // a box outside the antialias domain is named and nothing else is written: 200 rows -> 2 need 401 taps bicubic, 201 bilinear
      if (aa) bad += check_refused({ok, ok, {2, 5, 20, 205, 32, 2, 20, 0, 2}}, 3, method, aa, 2), ++n;
    }
  // refusals of the arguments themselves
  tfimm_resize_batch_sizes s;
  const int32_t box[] = {0, 0, 5, 7}, fr[] = {0}, g[] = {16, 16, 0, 0};
  if (tfimm_hip_resize_region_tables(0, FRAMES, 1, box, fr, g, 16, 16, 3, nullptr, 0, 0, &s, nullptr, nullptr, nullptr, nullptr) != TFIMM_EINVAL) ++bad;
  if (tfimm_hip_resize_region_tables(1, FRAMES, 0, box, fr, g, 16, 16, 3, nullptr, 0, 0, &s, nullptr, nullptr, nullptr, nullptr) != TFIMM_EINVAL) ++bad;
  if (tfimm_hip_resize_region_tables(1, FRAMES, 1, box, fr, g, 16, 16, 9, nullptr, 0, 0, &s, nullptr, nullptr, nullptr, nullptr) != TFIMM_EINVAL) ++bad;
  if (tfimm_hip_resize_region_tables(1, FRAMES, 1, box, fr, g, 16, 16, 3, nullptr, 2, 0, &s, nullptr, nullptr, nullptr, nullptr) != TFIMM_EINVAL) ++bad;
  if (tfimm_hip_resize_region_tables(1, FRAMES, 1, box, fr, g, 16, 16, 3, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) != TFIMM_EINVAL) ++bad;
  if (tfimm_hip_resize_region_tables(1, FRAMES, 1, nullptr, fr, g, 16, 16, 3, nullptr, 0, 0, &s, nullptr, nullptr, nullptr, nullptr) != TFIMM_EINVAL) ++bad;
  std::printf("resize_region_host: %d sets, %d bad\n", n, bad);
  return bad != 0;
}

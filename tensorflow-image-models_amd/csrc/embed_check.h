// The argument checks shared by the gallery searches (embed.hip, embed_wide.hip, embed_coarse.hip, embed_lists.hip,
// embed_lists_grouped.hip): every entry point and its _workspace twin refuse the same values with the same words, the entry
// point's name in front.  Host code only.  A check returns 0, or TFIMM_EINVAL with the error text set; `fn` is the entry point's
// name without "tfimm_hip_".
#pragma once
#include <initializer_list>
#include <string>

#include "common.h"

#define TFIMM_EMBED_TRY(check)     \
  do {                             \
    const int _rc = (check);       \
    if (_rc) return _rc;           \
  } while (0)

namespace embed_check {

// the widths every search accepts; the E-domain rule stands here alone
inline bool e_ok(int E) { return E >= TFIMM_EMBED_MIN_E && E <= TFIMM_EMBED_MAX_E && E % 16 == 0; }

inline int check_E(const char* fn, int E) {
  if (!e_ok(E))
    TFIMM_FAIL(TFIMM_EINVAL, "%s: E=%d, must be a multiple of 16 in [%d, TFIMM_EMBED_MAX_E = %d]", fn, E, TFIMM_EMBED_MIN_E,
               TFIMM_EMBED_MAX_E);
  return 0;
}

inline int check_N(const char* fn, int N) {
  if (N < 1) TFIMM_FAIL(TFIMM_EINVAL, "%s: N=%d, must be in [1, 2^31)", fn, N);
  return 0;
}

// the searches whose query tiles are a grid dimension
inline int check_B(const char* fn, int B) {
  if (B < 0 || B > TFIMM_EMBED_MAX_B) TFIMM_FAIL(TFIMM_EINVAL, "%s: B=%d, must be in [0, TFIMM_EMBED_MAX_B = %d]", fn, B, TFIMM_EMBED_MAX_B);
  return 0;
}

inline int check_ld_q(const char* fn, int64_t ld_q, int E) {
  if (ld_q < E) TFIMM_FAIL(TFIMM_EINVAL, "%s: ld_q=%lld is smaller than E=%d", fn, (long long)ld_q, E);
  return 0;
}

inline int check_ld_g(const char* fn, int64_t ld_g, int E) {
  if (ld_g < E || ld_g % 8 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: ld_g=%lld, must be a multiple of 8 elements and at least E=%d", fn, (long long)ld_g, E);
  return 0;
}

inline int check_ld_c(const char* fn, int64_t ld_c, int E) {
  if (ld_c < E || ld_c % 16 != 0)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: ld_c=%lld, must be a multiple of 16 bytes and at least E=%d", fn, (long long)ld_c, E);
  return 0;
}

inline int check_ld_p(const char* fn, int64_t ld_p, int nprobe) {
  if (ld_p < nprobe) TFIMM_FAIL(TFIMM_EINVAL, "%s: ld_p=%lld is smaller than nprobe=%d", fn, (long long)ld_p, nprobe);
  return 0;
}

// `need` is what tfimm_hip_<fn>_workspace returns for the same arguments
inline int check_workspace(const char* fn, int64_t workspace_bytes, int64_t need) {
  if (workspace_bytes < need)
    TFIMM_FAIL(TFIMM_EINVAL, "%s: workspace_bytes=%lld, tfimm_hip_%s_workspace asks for %lld", fn, (long long)workspace_bytes, fn,
               (long long)need);
  return 0;
}

// A pointer argument: its name in the error texts and the alignment the kernels need (16, 4, or 1: none).
struct Ptr {
  const char* name;
  const void* p;
  int align;
};

// "a", "a and b", "a, b and c": the arguments of `ptrs` with that alignment, and the OR of their addresses
inline std::string names_of(std::initializer_list<Ptr> ptrs, int align, uintptr_t* bits) {
  int n = 0, at = 0;
  for (const Ptr& a : ptrs) n += a.align == align ? 1 : 0;
  std::string s;
  *bits = 0;
  for (const Ptr& a : ptrs) {
    if (a.align != align) continue;
    if (at > 0) s += at == n - 1 ? " and " : ", ";
    s += a.name;
    *bits |= (uintptr_t)a.p;
    ++at;
  }
  return s;
}

// none null (the first one in argument order is named), then the 16-byte group, then the 4-byte group, each refused as a whole.
// `four_says` ends the 4-byte text: what the group holds differs between the entry points.
inline int check_pointers(const char* fn, std::initializer_list<Ptr> ptrs,
                          const char* four_says = "hold 4-byte elements and must be 4-byte aligned") {
  for (const Ptr& a : ptrs)
    if (!a.p) TFIMM_FAIL(TFIMM_EINVAL, "%s: %s is null", fn, a.name);
  uintptr_t bits = 0;
  const std::string wide = names_of(ptrs, 16, &bits);
  if (bits & 15) TFIMM_FAIL(TFIMM_EINVAL, "%s: %s must be 16-byte aligned", fn, wide.c_str());
  const std::string four = names_of(ptrs, 4, &bits);
  if (bits & 3) TFIMM_FAIL(TFIMM_EINVAL, "%s: %s %s", fn, four.c_str(), four_says);
  return 0;
}

}  // namespace embed_check

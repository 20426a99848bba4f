"""Element-wise bars of the MXFP8 kernels (csrc/mx.hip), numpy only: the CPU proof (tests/test_fp8.py) and the GPU tests
(tests/test_gpu_fp8.py) share these definitions.

* ``check_ln_quantize``: tfimm_hip_quantize_mx with a LayerNorm first.  Exact against ``pack.mx_quantize`` of the fp64
  LayerNorm, except where an honest fp32 kernel may provably land on either side of a rounding or scale boundary.
* ``gemm_tol``: the accumulation bar of tfimm_hip_gemm_mx against an fp64 product of the dequantized operands.
* ``check_mxfp8_output``: the scale and element rule of tfimm_hip_gemm_mx writing MXFP8.
"""
import numpy as np

from tfimm.engine import pack

U = 2.0 ** -24                     # unit roundoff of fp32
RSQRT_ERR = 2.0 ** -22             # relative error allowed to rsqrt (v_rsq_f32: 1 ulp)
LN_EXEMPT_CAP = 0.02               # largest share of elements the LN bar may exempt in one case


def ln_f64(x, gamma, beta, eps):
    """LayerNorm over the last axis in fp64: (y, mean, rstd, normalised value)"""
    x = np.asarray(x, np.float64)
    m = x.mean(-1, keepdims=True)
    d = x - m
    r = 1.0 / np.sqrt((d * d).mean(-1, keepdims=True) + eps)
    n = d * r
    return n * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64), m, r, n


def _sum_depth(C):
    """serial additions per row of an honest one-wave reduction: 8 values per lane per 512-channel piece, then a 6-level
    tree over the 64 lanes"""
    return 8 * -(-C // 512) + 6


def _sum_is_exact(x):
    """every partial sum of the row is a multiple of the smallest bf16 ulp among its nonzero elements, and bounded by
    sum |x| < 2^24 of those ulps: then fp32 represents each one exactly, in any order"""
    a = np.abs(np.asarray(x, np.float64))
    nz = np.where(a > 0, a, np.inf)
    lo = nz.min(-1)
    q = np.exp2(np.floor(np.log2(np.where(np.isfinite(lo), lo, 1.0))) - 7)      # bf16 has 8 significant bits
    q = np.maximum(q, 2.0 ** -133)                                               # bf16 subnormal spacing
    return a.sum(-1) < q * 2.0 ** 24


def ln_delta(x, gamma, beta, eps):
    """(y64, delta): per element, a bound on |y32 - y64| for an honest fp32 kernel -- two-pass statistics (the mean, then the
    mean square deviation from it), rsqrt, y = fma((x - mean) * rstd, gamma, beta).

    delta = |gamma| rstd |mean error| + |gamma n| (rstd error + 2u) + u |y|: the mean error is 0 for a sum that fp32 holds
    exactly (_sum_is_exact), else the recursive-summation bound depth * u * sum |x|, plus 2u |mean| for the scaling by 1 / C;
    the rstd error is half the relative error of the variance -- its sum, the two roundings of each term, the scaling, the
    + eps, the square of the mean error -- plus that of rsqrt."""
    x = np.asarray(x, np.float64)
    C = x.shape[-1]
    y, m, r, n = ln_f64(x, gamma, beta, eps)
    D = _sum_depth(C)
    s_abs = np.abs(x).sum(-1, keepdims=True)
    sum_err = np.where(_sum_is_exact(x)[..., None], 0.0, D * U * s_abs * (1 + 1e-6))
    dm = sum_err / C + 2 * U * np.abs(m) * (1 + 1e-6)
    var = 1.0 / (r * r)                                                          # var + eps
    r_rel = 0.5 * ((D + 6) * U + dm * dm / var) + RSQRT_ERR
    g = np.abs(np.asarray(gamma, np.float64))
    delta = g * r * dm + g * np.abs(n) * (r_rel + 2 * U) + U * np.abs(y)
    return y, delta * (1 + 1e-3)


def _quantize_at(v, k):
    """e4m3 codes of the fp64 values v [..., nb, 32] at the scale exponents k [..., nb] (beyond 448: clamped, so that a
    value too large for the scale gives another code than one that fits)"""
    s = np.exp2(-k.astype(np.float64))[..., None]
    return pack.e4m3_encode(np.clip(v * s, -464.0, 464.0).astype(np.float32))


def check_ln_quantize(codes, scales, x, gamma, beta, eps):
    """codes [rows, >= C] / scale bytes [rows, >= C / 32] of tfimm_hip_quantize_mx(x, gamma, beta, eps) against the fp64
    LayerNorm.  An element is EXEMPT when quantizing y64 - delta and y64 + delta gives different scales or codes; every other
    element and scale must equal pack.mx_quantize(y64) bit for bit.  An exempt element must still be what the rule gives
    for some value within delta of y64 (its scale between those of the two ends, its value between theirs at that scale).
    Returns (violations, exempt fraction)."""
    rows, C = x.shape
    nb = C // 32
    y, d = ln_delta(x, gamma, beta, eps)
    c = np.asarray(codes)[:, :C]
    k_got = np.asarray(scales)[:, :nb].astype(np.int64) - 127
    want_c, want_s = pack.mx_quantize(y)
    k_want = want_s.astype(np.int64) - 127
    ab = np.abs(y).reshape(rows, nb, 32)
    db = d.reshape(rows, nb, 32)
    k_lo = pack.mx_scale_exp(np.nextafter(np.maximum(ab - db, 0).max(-1).astype(np.float32), np.float32(0)))
    k_hi = pack.mx_scale_exp(np.nextafter((ab + db).max(-1).astype(np.float32), np.float32(np.inf)))
    lo, hi = (y - d).reshape(rows, nb, 32), (y + d).reshape(rows, nb, 32)
    c_lo, c_hi = _quantize_at(lo, k_got), _quantize_at(hi, k_got)
    exempt = (k_lo != k_hi)[..., None] | (c_lo != c_hi) | (_quantize_at(lo, k_want) != _quantize_at(hi, k_want))
    exact = (c.reshape(rows, nb, 32) == want_c.reshape(rows, nb, 32)) & (k_got == k_want)[..., None]
    # exempt: scale within the two ends' scales, value within the two ends' values at that scale (monotone rounding)
    k_ok = (k_got >= k_lo) & (k_got <= k_hi)
    v_got = pack.e4m3_decode(c.reshape(rows, nb, 32)).astype(np.float64)
    v_lo, v_hi = pack.e4m3_decode(c_lo).astype(np.float64), pack.e4m3_decode(c_hi).astype(np.float64)
    in_range = k_ok[..., None] & (v_got >= v_lo) & (v_got <= v_hi)
    bad = np.where(exempt, ~in_range, ~exact)
    return int(bad.sum()), float(exempt.mean())


# ---- tfimm_hip_gemm_mx -----------------------------------------------------------------------------------------------------
def gemm_tol(mag, v, act="", bias=None, residual=None):
    """bar on |got - v| of an fp32 result: ``mag`` = |A| . |W|^T of the dequantized operands, ``v`` the fp64 reference.
    The block-scaled MFMA does not sum its 64 products in full fp32 -- measured on MI355X up to ~2e-5 * sum |a b| at
    K = 32 .. 3072 (fp32 MFMA chains: ~1e-7) -- so the bar is 6e-5 * sum |a b| (x the slope of the activation, <= 1.2); + the
    polynomial GELU of the epilogues and the fp32 roundings of the bias / residual adds"""
    return (6e-5 * mag * 1.2 + (2e-5 if act == "gelu" else 0)
            + 2.0 ** -21 * (np.abs(v) + (0 if bias is None else np.abs(bias)) + (0 if residual is None else np.abs(residual)))
            + 1e-30)


def bf16_tol(ref, tol):
    """the bar of a bf16 result: the fp32 bar plus half a bf16 ulp of the fp32 value"""
    return tol + (np.abs(ref) + tol) * 2.0 ** -8


def e4m3_step(y):
    a = np.abs(y)
    return np.where(a < 2.0 ** -6, 2.0 ** -9, np.exp2(np.floor(np.log2(np.maximum(a, 2.0 ** -6))) - 3))


def check_mxfp8_output(codes, scales, ref, tol):
    """MXFP8 output (codes [M, >= N], scale bytes [M, >= N / 32]) of an fp32 result whose fp64 reference is ``ref`` [M, N]
    with the bar ``tol``.  A block's scale is that of the reference's amax, or its neighbour where the amax lies within the
    bar of a scale boundary; each element is the reference at the block's scale rounded to nearest, within half a step plus
    the bar (an element on a rounding boundary may take the neighbouring code); and more than 99 % of the elements are
    within half a step.  Returns a list of failure descriptions (empty: pass) and the worst |err| / (step / 2 + bar)."""
    M, N = ref.shape
    nb = N // 32
    codes, scales = np.asarray(codes)[:, :N], np.asarray(scales)[:, :nb]
    fails = []
    ref32 = ref.astype(np.float32)
    want_k = pack.mx_scale_exp(np.abs(ref32.reshape(M, nb, 32)).max(-1))
    got_k = scales.astype(np.int64) - 127
    amax = np.abs(ref.reshape(M, nb, 32)).max(-1)
    tol_blk = tol.reshape(M, nb, 32).max(-1)
    bnd = 448.0 * np.exp2(want_k.astype(np.float64))
    near = (np.abs(amax - bnd) <= tol_blk) | (np.abs(amax - bnd / 2) <= tol_blk)
    n_bad_k = int(((got_k != want_k) & ~near).sum())
    if n_bad_k:
        fails.append(f"{n_bad_k} scales")
    s = np.exp2(got_k.astype(np.float64))[..., None]
    y = ref.reshape(M, nb, 32) / s
    gv = pack.e4m3_decode(codes).astype(np.float64).reshape(M, nb, 32)
    err = np.abs(gv - y)
    lim = e4m3_step(y) * 0.5 + tol.reshape(y.shape) / s + 1e-12
    if not np.all(err <= lim):
        fails.append(f"{int((err > lim).sum())} elements, worst {float((err / e4m3_step(y)).max())} steps")
    exact = err <= e4m3_step(y) * 0.5 + 1e-12
    if exact.mean() <= 0.99:
        fails.append(f"only {float(exact.mean())} within half a step")
    return fails, float((err / lim).max())

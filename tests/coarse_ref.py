"""The rule of the coarse-to-fine gallery search (tfimm_hip_embed_quantize_rows / tfimm_hip_embed_search_coarse,
csrc/embed_coarse.hip), restated in numpy.

Row quantisation, for a bf16 row ``g`` of E values: ``a = max |g_e|``; ``e = 0`` if ``a == 0``, otherwise
``ceil(log2(a / 448))`` clamped to [EXP_MIN, EXP_MAX] = [-126, 126] (2^e and 2^-e are then normal float32 numbers; a finite bf16
row asks for at most 121, and only an amax below 2^-118 meets the lower clamp); ``code_e = e4m3fn_rne(g_e * 2^-e)``.  The scale
is a power of two, so scaling is exact, and ``|g_e * 2^-e| <= 448``: nothing saturates.  A non-finite entry becomes the NaN
code 0x7f with its sign.

Coarse key of (query, row): the query rounded to bf16 (``embed_ref.bf16_round``) and quantised by the same rule;
``acc = sum_e code_q[e] * code_g[e]`` (on the device a float32 MFMA sum from a zero accumulator, here float64);
``key = acc * 2^(e_row)``.  The query's exponent, a positive constant per query, is not applied.

Candidates: the ``candidates`` best rows per query by key descending, equal keys by ascending row.  Result: the ``k`` best of
the candidates by exact score (``embed_ref.scores64``) descending, equal scores by ascending row."""
import numpy as np

import embed_ref as er

EXP_MIN, EXP_MAX = -126, 126
E4M3_MAX = 448.0


def e4m3_encode(x) -> np.ndarray:
    """float -> OCP e4m3fn codes (uint8), round to nearest even; the sign is kept (-0.0 -> 0x80); what is not <= 448 in
    magnitude -> the NaN code 0x7f | sign"""
    x = np.asarray(x, np.float64)
    sign = np.where(np.signbit(x), 0x80, 0).astype(np.uint8)
    a = np.abs(x)
    ok = a <= E4M3_MAX                                      # False for NaN
    a = np.where(ok, a, 1.0)
    sub = np.rint(a * 512.0)                                # below 2^-6: multiples of 2^-9, ties to even; 8 is the least normal
    m, ex = np.frexp(np.where(a > 0, a, 1.0))               # a = m 2^ex, m in [0.5, 1)
    p = ex - 1
    frac = np.rint((2.0 * m - 1.0) * 8.0)                   # three mantissa bits, ties to even
    p = np.where(frac == 8, p + 1, p)
    frac = np.where(frac == 8, 0, frac)
    nrm = (p + 7) * 8 + frac
    code = np.where(a < 2.0 ** -6, sub, nrm).astype(np.int64)
    return (np.where(ok, code, 0x7f).astype(np.uint8) | sign).astype(np.uint8)


def e4m3_decode(codes) -> np.ndarray:
    """e4m3fn codes -> float64 (0x7f / 0xff -> NaN)"""
    c = np.asarray(codes, np.uint8).astype(np.int64)
    ex, fr = (c >> 3) & 15, c & 7
    v = np.where(ex == 0, fr * 2.0 ** -9, (1 + fr / 8.0) * 2.0 ** (ex - 7.0))
    v = np.where((c & 0x7f) == 0x7f, np.nan, v)
    return np.where(c & 0x80, -v, v)


def row_exponents(g) -> np.ndarray:
    """the int8 exponent of every row of ``g`` (bf16 values as float32 or float64), (N,)"""
    a = np.abs(np.asarray(g, np.float64)).max(axis=1)
    finite = np.isfinite(a)
    m, ex = np.frexp(np.where(finite & (a > 0), a, 1.0))    # a / 448 = (m / 0.875) 2^(ex - 9)
    e = np.where(m > 0.875, ex - 8, ex - 9)
    e = np.where(finite, e, 120)                            # the bits of inf and of the default NaN (a NaN's payload may add 1)
    e = np.where(a == 0, 0, e)
    return np.clip(e, EXP_MIN, EXP_MAX).astype(np.int8)


def quantize_rows(g):
    """(codes uint8 (N, E), exponents int8 (N,)) of bf16 rows"""
    g = np.asarray(g, np.float64)
    e = row_exponents(g)
    with np.errstate(invalid="ignore", over="ignore"):
        return e4m3_encode(np.ldexp(g, -e.astype(np.int64)[:, None])), e


def keys64(q, g):
    """(keys, bands) float64 (B, N): the coarse keys of float32 queries (rounded to bf16 here) against bf16 rows, exactly, and
    ``band = E * 2^-23 * sum_e |code_q code_g| * 2^e_row`` -- E exact products and at most E float32 additions at up to one ulp
    each (the band of DESIGN.md 3.18 on the codes); the device's float32 key lies within it"""
    cq, _ = quantize_rows(er.bf16_round(q))
    cg, eg = quantize_rows(g)
    dq, dg = e4m3_decode(cq), e4m3_decode(cg)
    scale = np.ldexp(1.0, eg.astype(np.int64))[None, :]
    E = dq.shape[1]
    return (dq @ dg.T) * scale, E * 2.0 ** -23 * (np.abs(dq) @ np.abs(dg).T) * scale


def candidates(keys, c) -> np.ndarray:
    """per query the ``c`` best rows by key descending, equal keys by ascending row: int32 (B, c)"""
    return er.select(keys, c)[0]


def margins(q, g, k, c):
    """What the bands prove about the candidates of every query, whatever the order of the float32 additions:
    ``held`` (B,): every exact top-``k`` row is surely a candidate -- its key minus its band exceeds the ``c``-th key plus the
    query's widest band, so fewer than ``c`` rows can beat it on the device;
    ``missed`` (B, k): this exact top-``k`` row is surely none -- its key plus its band is below the ``c``-th key minus the
    widest band, so ``c`` rows surely beat it;
    ``sure`` (B,): the candidate set on the device is the reference's -- the ``c``-th and the ``c + 1``-th key are further
    apart than two widest bands.  Also returns the exact top ``k`` (B, k) and the reference's candidates (B, c)."""
    keys, bands = keys64(q, g)
    widest = bands.max(1)
    ordered = -np.sort(-keys, axis=1)
    top = er.select(er.scores64(q, g), k)[0]
    at = top.astype(np.int64)
    held = (np.take_along_axis(keys - bands, at, 1) > (ordered[:, c - 1] + widest)[:, None]).all(1)
    missed = np.take_along_axis(keys + bands, at, 1) < (ordered[:, c - 1] - widest)[:, None]
    sure = ordered[:, c - 1] - widest > ordered[:, c] + widest if c < keys.shape[1] else np.ones(len(keys), bool)
    return held, missed, sure, top, candidates(keys, c)


#: the lossy case: (seed, E, centres, noise, N, B, k, candidates) -- unit rows around few centres, closer to each other than
#: fp8 tells apart: 30 of the 32 queries surely lose an exact top-k row to the scan, 2 do not
LOSSY = (1, 64, 4, 0.1, 256, 32, 4, 16)


def clustered(seed, E, centres, noise, N, B):
    """(queries float32 (B, E), bf16 rows (N, E)): unit vectors, each a random unit centre plus ``noise`` times a unit-scale
    normal vector, normalised"""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((centres, E))
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)

    def draw(n):
        x = cen[rng.integers(0, centres, n)] + noise * rng.standard_normal((n, E)) / np.sqrt(E)
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return draw(B), er.bf16_round(draw(N))


#: (k, candidates) of the random-data checks
RANDOM_PAIRS = ((5, 20), (20, 80), (64, 256))
_RANDOM = {}


def random_case(E):
    """(33 queries, 20000 gallery rows rounded to bf16), standard normal, computed once and never changed"""
    if E not in _RANDOM:
        rng = np.random.default_rng(E)
        q = rng.standard_normal((33, E)).astype(np.float32)
        g = er.bf16_round(rng.standard_normal((20000, E)).astype(np.float32))
        q.setflags(write=False)
        g.setflags(write=False)
        _RANDOM[E] = (q, g)
    return _RANDOM[E]


def grid(seed, shape):
    """entries from {-4, ..., 4} / 8: exact in bf16 and, scaled by a power of two, in e4m3; every partial sum of products is
    exact in float32 for E <= 2048, so keys and scores are bit-equal to the rule in any summation order"""
    return (np.random.default_rng(seed).integers(-4, 5, shape) / 8).astype(np.float32)


def search_coarse(q, g, k, c):
    """the rule with exact arithmetic: (indices int32 (B, k), scores float32 (B, k), candidates int32 (B, c))"""
    cand = candidates(keys64(q, g)[0], c)
    exact = np.take_along_axis(er.scores64(q, g), cand.astype(np.int64), 1)
    idx = np.empty((cand.shape[0], k), np.int32)
    sc = np.empty((cand.shape[0], k), np.float64)
    for b in range(cand.shape[0]):
        order = sorted(range(c), key=lambda j: (-exact[b, j], cand[b, j]))[:k]
        idx[b], sc[b] = cand[b, order], exact[b, order]
    return idx, sc.astype(np.float32), cand

"""Restatement of the ANTIALIASED resize + centre crop + normalise input step in plain numpy loops (test helper).

``tf.image.resize(float32(img), size, method, antialias=True)``, the ScaleAndTranslate formulation, every quantity a float32
and every step a float32 operation of its own.  Per axis resized from ``n_in`` to ``n_res``, for the output position ``o``:

* ``radius`` = 2 (bicubic) or 1 (bilinear); ``inv = f32(n_in) / f32(n_res)``; ``ks = max(inv, 1)``;
  ``T = min(2 * ceil(radius * ks) + 1, n_in)`` is the span pitch;
* ``s = (f32(o) + 0.5) * inv``; ``a = ceil(s - radius * ks - 0.5)`` and ``b = floor(s + radius * ks - 0.5)``, both clamped to
  ``[0, n_in - 1]``; ``start = a``, ``count = b - a + 1``;
* ``w_i = K(|(f32(i) + 0.5 - s) / ks|)`` for ``i = a..b``; ``total`` = their sum from 0.0 in order; if
  ``|total| >= 1000 * FLT_MIN`` every weight is multiplied by ``1 / total``; entries past ``count`` are +0.0;
* K bicubic: Keys with A = -0.5, computed directly; K bilinear: ``max(0, 1 - x)``.

The vertical pass runs first into a float32 intermediate, then the horizontal pass; each sum starts at 0.0 and adds ``w * x``
in tap order.  The normalisation is the one of tests/resize_ref.py.  There is no TensorFlow binary to ask: this rule is the
specification, and tests/test_resize_aa.py holds it to torch's independent ``interpolate(antialias=True)``.

Deliberately independent of the engine: nothing here imports tfimm or loads the library.
"""
import math

import numpy as np

from resize_ref import normalise, to_bf16  # noqa: F401  (re-exported for the tests)

f32 = np.float32
FLT_MIN = f32(np.finfo(np.float32).tiny)
RADIUS = {"bicubic": f32(2), "bilinear": f32(1)}


def keys(x):
    """Keys cubic convolution kernel, A = -0.5, of a float32 ``x >= 0``"""
    if x >= f32(2):
        return f32(0)
    if x >= f32(1):
        return ((f32(-0.5) * x + f32(2.5)) * x - f32(4)) * x + f32(2)
    return ((f32(1.5) * x - f32(2.5)) * x) * x + f32(1)


def triangle(x):
    return max(f32(0), f32(1) - x)


KERNEL = {"bicubic": keys, "bilinear": triangle}


def axis(n_in, n_res, method):
    """``(inv, ks, reach, T)`` of an axis, ``reach = radius * ks``"""
    inv = f32(n_in) / f32(n_res)
    ks = max(inv, f32(1))
    reach = RADIUS[method] * ks
    return inv, ks, reach, min(2 * math.ceil(float(reach)) + 1, n_in)


def span_taps(n_in, n_res, method):
    return axis(n_in, n_res, method)[3]


def spans(n_in, n_res, first, n_out, method):
    """start int32 [n_out], count int32 [n_out], w float32 [n_out][T] of the output positions [first, first + n_out)"""
    inv, ks, reach, T = axis(n_in, n_res, method)
    K = KERNEL[method]
    start, count, w = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros((n_out, T), np.float32)
    for k in range(n_out):
        s = (f32(first + k) + f32(0.5)) * inv
        a = math.ceil(float(s - reach - f32(0.5)))
        b = math.floor(float(s + reach - f32(0.5)))
        a, b = min(max(a, 0), n_in - 1), min(max(b, 0), n_in - 1)
        assert 1 <= b - a + 1 <= T, (n_in, n_res, first + k, a, b, T)
        ws = [K(f32(abs((f32(i) + f32(0.5) - s) / ks))) for i in range(a, b + 1)]
        total = f32(0)
        for v in ws:
            total = f32(total + v)
        if abs(total) >= f32(1000) * FLT_MIN:
            scale = f32(1) / total
            ws = [f32(v * scale) for v in ws]
        start[k], count[k] = a, b - a + 1
        w[k, :len(ws)] = ws
    return start, count, w


def resample(x, geometry, size, method):
    """float32 (B, Hs, Ws, C) -> the (B, H, W, C) crop window ``size`` at (top, left) of the image resized to (Rh, Rw) with
    antialiasing; ``geometry = (Rh, Rw, top, left)``.  Every output row / column sums over its own span only."""
    x = np.asarray(x, np.float32)
    B, Hs, Ws, C = x.shape
    (Rh, Rw, top, left), (H, W) = geometry, size
    ys, yc, yw = spans(Hs, Rh, top, H, method)
    xs, xc, xw = spans(Ws, Rw, left, W, method)
    rows = np.zeros((B, H, Ws, C), np.float32)
    for y in range(H):
        acc = np.zeros((B, Ws, C), np.float32)
        for t in range(yc[y]):
            acc = acc + yw[y, t] * x[:, ys[y] + t]
        rows[:, y] = acc
    out = np.zeros((B, H, W, C), np.float32)
    for c in range(W):
        acc = np.zeros((B, H, C), np.float32)
        for t in range(xc[c]):
            acc = acc + xw[c, t] * rows[:, :, xs[c] + t]
        out[:, :, c] = acc
    return out


def resize_crop_normalise(u8, geometry, size, method, mean, std):
    """uint8 (B, Hs, Ws, C) -> float32 (B, H, W, C): antialiased resize to (Rh, Rw), crop, normalise"""
    return normalise(resample(np.asarray(u8).astype(np.float32), geometry, size, method), mean, std)

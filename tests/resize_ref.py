"""Restatement of the resize + centre crop + normalise input step in plain numpy loops (test helper).

``tf.image.resize(float32(img), size, method, antialias=False)`` with half-pixel centres, every quantity float32:

* bilinear, restated here from TensorFlow's resize_bilinear_op (compute_interpolation_weights / compute_lerp):
  ``loc = (o + 0.5) * scale - 0.5``, ``lo = max(floor(loc), 0)``, ``hi = min(ceil(loc), n - 1)``, ``frac = loc - floor(loc)``;
  ``top = tl + (tr - tl) * xf``, ``bottom = bl + (br - bl) * xf``, ``out = top + (bottom - top) * yf``;
* bicubic is ``oracle.ops.resize_bicubic_tf`` (imported, unchanged); ``bicubic_taps`` writes its nested tap rule out once
  more in the fixed four-tap form of the C ABI (a dropped tap = weight +0.0 at a clamped index) and
  tests/test_resize.py holds it to the oracle.

Deliberately independent of the engine: nothing here imports tfimm.
"""
import math

import numpy as np
import torch

from oracle import ops

f32 = np.float32


def _loc(o, scale):
    return (f32(o) + f32(0.5)) * scale - f32(0.5)


def bilinear_taps(n_in, n_out):
    """idx int32 [n_out][2] = (lo, hi), w float32 [n_out][2] = (1 - frac, frac)"""
    idx, w = np.zeros((n_out, 2), np.int32), np.zeros((n_out, 2), np.float32)
    scale = f32(n_in) / f32(n_out)
    for o in range(n_out):
        loc = _loc(o, scale)
        fl = math.floor(float(loc))
        frac = loc - f32(fl)
        idx[o] = (max(fl, 0), min(math.ceil(float(loc)), n_in - 1))
        w[o] = (f32(1) - frac, frac)
    return idx, w


def bicubic_taps(n_in, n_out):
    """idx int32 [n_out][4], w float32 [n_out][4]: the taps of oracle.ops.resize_bicubic_tf, a tap outside the image
    carried as weight +0.0 at the clamped index"""
    A, TAB = f32(-0.5), 1024          # every constant a float32: the bits do not depend on NumPy's scalar promotion rules

    def near(i):
        t = f32(i) / f32(TAB)
        return ((A + f32(2)) * t - (A + f32(3))) * t * t + f32(1)

    def far(i):
        t = f32(i) / f32(TAB) + f32(1)
        return ((A * t - f32(5) * A) * t + f32(8) * A) * t - f32(4) * A

    idx, w = np.zeros((n_out, 4), np.int32), np.zeros((n_out, 4), np.float32)
    scale = f32(n_in) / f32(n_out)
    for o in range(n_out):
        loc = _loc(o, scale)
        base = math.floor(float(loc))
        off = int(np.rint((loc - f32(base)) * f32(TAB)))
        cand = [(base - 1, far(off)), (base, near(off)), (base + 1, near(TAB - off)), (base + 2, far(TAB - off))]
        tot = f32(0)
        for i, wt in cand:
            if 0 <= i < n_in:
                tot = tot + wt
        for t, (i, wt) in enumerate(cand):
            idx[o, t] = min(max(i, 0), n_in - 1)
            w[o, t] = f32(wt / tot) if 0 <= i < n_in else f32(0)
    return idx, w


def resize_bilinear(x, size):
    """x float32 (B, H, W, C) -> (B, size[0], size[1], C)"""
    x = np.asarray(x, np.float32)
    B, H, W, C = x.shape
    (iy, wy), (ix, wx) = bilinear_taps(H, size[0]), bilinear_taps(W, size[1])
    out = np.zeros((B, size[0], size[1], C), np.float32)
    for oy in range(size[0]):
        for ox in range(size[1]):
            tl, tr = x[:, iy[oy, 0], ix[ox, 0]], x[:, iy[oy, 0], ix[ox, 1]]
            bl, br = x[:, iy[oy, 1], ix[ox, 0]], x[:, iy[oy, 1], ix[ox, 1]]
            top = tl + (tr - tl) * wx[ox, 1]
            bottom = bl + (br - bl) * wx[ox, 1]
            out[:, oy, ox] = top + (bottom - top) * wy[oy, 1]
    return out


def resize(x, size, method):
    if method == "bicubic":
        return ops.resize_bicubic_tf(torch.from_numpy(np.asarray(x, np.float32)), tuple(size)).numpy()
    assert method == "bilinear", method
    return resize_bilinear(x, size)


def normalise(r, mean, std):
    """the three float32 operations of create_preprocessing (models/factory.py:165-167)"""
    return (np.asarray(r, np.float32) / f32(255.0) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)


def resize_crop_normalise(u8, geometry, size, method, mean, std):
    """uint8 (B, Hs, Ws, C) -> float32 (B, H, W, C): resize to (Rh, Rw), crop the window ``size`` at (top, left), normalise;
    ``geometry = (Rh, Rw, top, left)``"""
    Rh, Rw, top, left = geometry
    r = resize(np.asarray(u8).astype(np.float32), (Rh, Rw), method)
    return normalise(r[:, top:top + size[0], left:left + size[1]], mean, std)


def to_bf16(x):
    """float32 -> bf16 (nearest-even) -> float32"""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).float().numpy()

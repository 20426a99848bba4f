"""Antialiased resize + centre crop + normalise of uint8 images, the host side (no GPU): the restatement of the span rule
(tests/resize_aa_ref.py) pinned by hand-computed answers and held to torch's independent ``interpolate(antialias=True)``, the
library's host span function held to the restatement bit for bit, ``DeferredInput.numpy()`` with an antialiased resize spec,
the keys and specs of callers that do not set the flag, and the refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import resize_aa_ref as ra
import resize_ref as rr
import test_architectures  # noqa: F401  (registers the miniature configs)
import tfimm
from tfimm.engine import ffi
from tfimm.models import DeferredInput
from tfimm.models.factory import resize_geometry

METHODS = ["bicubic", "bilinear"]


# ---- the restatement, pinned ---------------------------------------------------------------------------------------
def test_bilinear_4_to_2_by_hand():
    """inv = ks = 2, reach 2, T = min(5, 4): s = 1, 3 -> [ceil(-1.5), floor(2.5)] = [0, 2] and [1, 3] after clamping; the
    triangle at |i + 0.5 - s| / 2 gives (.75, .75, .25) / 1.75 and its mirror"""
    start, count, w = ra.spans(4, 2, 0, 2, "bilinear")
    assert ra.span_taps(4, 2, "bilinear") == 4 and w.shape == (2, 4)
    assert start.tolist() == [0, 1] and count.tolist() == [3, 3]
    s = np.float32(1) / np.float32(1.75)
    assert w[0].tolist() == [np.float32(0.75) * s, np.float32(0.75) * s, np.float32(0.25) * s, 0.0]
    assert w[1].tolist() == [np.float32(0.25) * s, np.float32(0.75) * s, np.float32(0.75) * s, 0.0]
    np.testing.assert_allclose(w[0, :3], [3 / 7, 3 / 7, 1 / 7], rtol=3e-7)
    np.testing.assert_allclose(w[1, :3], [1 / 7, 3 / 7, 3 / 7], rtol=3e-7)


@pytest.mark.parametrize("method, T", [("bicubic", 5), ("bilinear", 3)])
def test_identity_axis_weights_are_exact_and_output_is_the_plain_normalisation(method, T):
    start, count, w = ra.spans(9, 9, 0, 9, method)
    assert w.shape == (9, T)
    for o in range(9):
        full = np.zeros(9, np.float32)
        full[start[o]:start[o] + count[o]] = w[o, :count[o]]
        assert full.tolist() == [1.0 if i == o else 0.0 for i in range(9)], o        # (0, 0, 1, 0, 0), clipped at the ends
    assert not np.signbit(w).any()
    u8 = np.random.default_rng(5).integers(0, 256, (2, 9, 11, 3), dtype=np.uint8)
    mean, std = np.float32([0.5, 0.4, 0.3]), np.float32([0.2, 0.3, 0.25])
    got = ra.resize_crop_normalise(u8, (9, 11, 0, 0), (9, 11), method, mean, std)
    assert np.array_equal(got, rr.normalise(u8.astype(np.float32), mean, std))


def test_bicubic_16_to_8_span_by_hand():
    """inv = ks = 2, reach 4, T = 9.  o = 3: s = 7, span [ceil(2.5), floor(10.5)] = [3, 10], x = 1.75, 1.25, .75, .25 and
    mirrored; Keys(-0.5) there is -3/128, -9/128, 29/128, 111/128 -- all exact in float32, the total is exactly 2"""
    start, count, w = ra.spans(16, 8, 3, 1, "bicubic")
    assert (start[0], count[0], w.shape) == (3, 8, (1, 9))
    half = [-3 / 256, -9 / 256, 29 / 256, 111 / 256]
    assert w[0].tolist() == half + half[::-1] + [0.0]
    # the first position: the span is cut at the image edge and renormalised over what is left
    start, count, w = ra.spans(16, 8, 0, 1, "bicubic")
    assert (start[0], count[0]) == (0, 5)                                             # s = 1: [ceil(-3.5) -> 0, floor(4.5)]
    raw = np.float32([111 / 128, 111 / 128, 29 / 128, -9 / 128, -3 / 128])            # x = .25, .25, .75, 1.25, 1.75
    tot = np.float32(0)
    for v in raw:
        tot = tot + v
    assert w[0, :5].tolist() == (raw * (np.float32(1) / tot)).tolist() and not w[0, 5:].any()


@pytest.mark.parametrize("method", METHODS)
def test_pitch_is_clamped_by_a_short_axis(method):
    """3 -> 2: 2 * ceil(radius * 1.5) + 1 = 7 (bicubic) or 5 (bilinear) taps do not fit 3 pixels"""
    assert ra.span_taps(3, 2, method) == 3
    start, count, w = ra.spans(3, 2, 0, 2, method)
    assert w.shape == (2, 3) and (start + count <= 3).all() and (count <= 3).all()
    assert count.tolist() == ([3, 3] if method == "bicubic" else [2, 2])
    for o in range(2):
        tot = np.float32(0)
        for v in w[o, :count[o]]:
            tot = tot + v
        assert abs(float(tot) - 1.0) < 3e-7


# ---- tfimm_hip_resize_spans against the restatement -------------------------------------------------------------------
AXES = [(37, 18, 1, 16), (53, 25, 4, 16), (120, 18, 1, 16), (5, 8, 0, 8), (640, 341, 58, 224), (3, 2, 0, 2), (16, 8, 0, 8),
        (9, 9, 0, 9), (1080, 224, 0, 224)]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n_in, n_resized, first, n_out", AXES)
def test_host_span_function_equals_restatement_bit_for_bit(n_in, n_resized, first, n_out, method):
    start_ref, count_ref, w_ref = ra.spans(n_in, n_resized, first, n_out, method)
    assert ffi.resize_span_taps(n_in, n_resized, method) == ra.span_taps(n_in, n_resized, method) == w_ref.shape[1]
    start, count, w = ffi.resize_spans(n_in, n_resized, first, n_out, method)
    assert start.dtype == count.dtype == np.int32 and w.dtype == np.float32
    assert np.array_equal(start, start_ref) and np.array_equal(count, count_ref)
    assert np.array_equal(w, w_ref) and np.array_equal(w.view(np.uint32), w_ref.view(np.uint32))
    assert start.min() >= 0 and (start + count).max() <= n_in and count.min() >= 1 and count.max() <= w.shape[1]
    # spans start and end in ascending order: what lets a tile stage one contiguous range of source columns
    assert (np.diff(start) >= 0).all() and (np.diff(start + count) >= 0).all()


def test_host_span_function_refuses_bad_windows():
    start, count, w = (ctypes.c_int32 * 16)(), (ctypes.c_int32 * 16)(), (ctypes.c_float * 256)()
    lib = ffi.lib
    assert lib.tfimm_hip_resize_spans(5, 8, 0, 4, 1, None, count, w) == -1
    assert lib.tfimm_hip_resize_spans(5, 8, 0, 4, 1, start, None, w) == -1
    assert lib.tfimm_hip_resize_spans(5, 8, 0, 4, 1, start, count, None) == -1
    assert lib.tfimm_hip_resize_spans(5, 8, -1, 4, 1, start, count, w) == -1
    assert lib.tfimm_hip_resize_spans(5, 8, 6, 4, 1, start, count, w) == -1           # window past the resized axis
    assert lib.tfimm_hip_resize_spans(5, 8, 0, 0, 1, start, count, w) == -1
    assert lib.tfimm_hip_resize_spans(0, 8, 0, 4, 1, start, count, w) == -1
    assert lib.tfimm_hip_resize_spans(5, 0, 0, 4, 1, start, count, w) == -1
    assert lib.tfimm_hip_resize_spans(5, 8, 0, 4, 2, start, count, w) == -1           # unknown method
    assert b"resize_spans" in lib.tfimm_hip_last_error()
    assert lib.tfimm_hip_resize_span_taps(0, 8, 1) == -1 and lib.tfimm_hip_resize_span_taps(5, 8, 2) == -1
    assert lib.tfimm_hip_resize_spans(5, 8, 4, 4, 1, start, count, w) == 0
    with pytest.raises(ffi.HipError):
        ffi.resize_spans(5, 8, 6, 4, "bicubic")


# ---- the restatement against an independent implementation of the same filter ------------------------------------------
GEOMETRIES = [((37, 53), (18, 25, 1, 4), (16, 16)), ((53, 37), (25, 18, 4, 1), (16, 16)), ((5, 7), (8, 8, 0, 0), (8, 8)),
              ((120, 97), (18, 18, 1, 1), (16, 16)), ((48, 56), (36, 42, 2, 5), (32, 32))]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("src, geometry, size", GEOMETRIES)
def test_restatement_against_torch_antialiased_interpolate(src, geometry, size, method):
    """torch's CPU ``interpolate(antialias=True)`` differs in float rounding order and in zero-weight edge taps only.  1e-3 on
    the 0..255 scale: 8 x the largest deviation measured when the rule was written down (1.22e-4), three orders of magnitude
    below what a dropped or shifted tap produces."""
    x = np.random.default_rng(src[0] * 131 + src[1]).integers(0, 256, (2, *src, 3), dtype=np.uint8).astype(np.float32)
    Rh, Rw, top, left = geometry
    want = torch.nn.functional.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=(Rh, Rw), mode=method, antialias=True,
                                           align_corners=False).permute(0, 2, 3, 1).numpy()
    want = want[:, top:top + size[0], left:left + size[1]]
    got = ra.resample(x, geometry, size, method)
    err = float(np.abs(got - want).max())
    print(f"{src} -> {geometry} -> {size} {method}: max |restatement - torch| = {err:.3e}")
    assert err <= 1e-3


# ---- DeferredInput.numpy() with an antialiased resize spec ------------------------------------------------------------
def _spec(name):
    cfg = tfimm.models.registry.model_config(name)
    n = cfg.in_channels
    mean = np.tile(np.asarray(cfg.mean, np.float64), n)[:n].astype(np.float32)
    std = np.tile(np.asarray(cfg.std, np.float64), n)[:n].astype(np.float32)
    return cfg, mean, std


@pytest.mark.parametrize("name, src", [
    ("vit_test_model", (37, 53)),                      # bicubic, 32 x 32, crop_pct 0.875
    ("vit_test_model", (20, 17)),                      # upscale, tall
    ("vit_test_model", (150, 40)),                     # one axis far down, one almost unchanged
    ("resnet_test_model_1", (53, 37)),                 # bilinear
    ("resnet_test_model_1", (32, 32)),                 # source = input size, crop_pct < 1: still resampled
    ("swin_shift_test_model", (70, 90)),               # non-square input size (64, 32)
])
def test_deferred_numpy_antialiased_equals_restatement_and_default_is_unchanged(name, src):
    cfg, mean, std = _spec(name)
    u8 = np.random.default_rng(11).integers(0, 256, (2, *src, cfg.in_channels), dtype=np.uint8)
    d = tfimm.create_preprocessing(name, defer=True, resize=True, antialias=True)(u8)
    assert isinstance(d, DeferredInput) and d.shape == u8.shape
    assert d.resize == (cfg.interpolation, float(cfg.crop_pct), tuple(cfg.input_size), True)
    geo = resize_geometry(src, cfg.input_size, cfg.crop_pct)
    want = ra.resize_crop_normalise(u8, geo, cfg.input_size, cfg.interpolation, mean, std)
    got = d.numpy()
    assert got.dtype == np.float32 and got.shape == (2, *cfg.input_size, cfg.in_channels)
    assert np.array_equal(got, want)
    pre = tfimm.create_preprocessing(name, defer=True, resize=True, antialias=True)
    assert np.array_equal(pre(u8[0]).numpy(), want[0])
    assert np.array_equal(pre(torch.from_numpy(u8)).numpy(), want)
    # the default: the spec, and the pixels, of a caller that does not know the keyword
    for plain in (tfimm.create_preprocessing(name, defer=True, resize=True)(u8),
                  tfimm.create_preprocessing(name, defer=True, resize=True, antialias=False)(u8)):
        assert plain.resize == (cfg.interpolation, float(cfg.crop_pct), tuple(cfg.input_size))
        assert np.array_equal(plain.numpy(), rr.resize_crop_normalise(u8, geo, cfg.input_size, cfg.interpolation, mean, std))
    assert not np.array_equal(got, plain.numpy())


def test_identity_geometry_is_the_plain_preprocessing():
    u8 = np.random.default_rng(12).integers(0, 256, (1, 9, 9, 3), dtype=np.uint8)
    plain = DeferredInput(u8, (0.5, 0.4, 0.3), (0.2, 0.3, 0.25)).numpy()
    for method in METHODS:
        d = DeferredInput(u8, (0.5, 0.4, 0.3), (0.2, 0.3, 0.25), resize=(method, 1.0, (9, 9), True))
        assert np.array_equal(d.numpy(), plain)


def test_spec_carries_the_flag_only_when_set():
    assert DeferredInput(np.zeros((1, 4, 4, 3), np.uint8), (0,) * 3, (1,) * 3, resize=("bicubic", 0.9, (4, 4), False)).resize == \
        ("bicubic", 0.9, (4, 4))
    assert DeferredInput(np.zeros((1, 4, 4, 3), np.uint8), (0,) * 3, (1,) * 3, resize=("bicubic", 0.9, (4, 4))).resize == \
        ("bicubic", 0.9, (4, 4))
    assert tfimm.create_preprocessing("vit_test_model", defer=True)(np.zeros((1, 40, 40, 3), np.uint8)).resize is None


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_antialias_without_resize_raises():
    with pytest.raises(ValueError, match="resize=True"):
        tfimm.create_preprocessing("vit_test_model", defer=True, antialias=True)
    with pytest.raises(ValueError):
        tfimm.create_preprocessing("vit_test_model", antialias=True)


@pytest.mark.parametrize("src, geometry, method", [((2000, 2000), (50, 50, 0, 0), "bicubic"),      # T = 161
                                                    ((40, 2100), (40, 64, 0, 0), "bilinear"),       # width only: T = 67
                                                    ((512, 32), (32, 32, 0, 0), "bicubic")])        # height only: T = 65
def test_sources_beyond_the_tap_limit_raise_before_the_device_is_touched(src, geometry, method):
    with pytest.raises(ValueError, match="TFIMM_RESIZE_AA_MAX_TAPS"):
        ffi.resize_aa_tables(src, geometry, geometry[:2], method)


def test_sources_at_the_tap_limit_are_tabulated():
    """the pitch is odd unless the axis itself cuts it: 63 is the largest below the limit, 64 needs a 64-pixel axis"""
    assert ffi.resize_span_taps(496, 32, "bicubic") == 63 and ffi.resize_span_taps(512, 32, "bicubic") == 65
    assert ffi.resize_span_taps(64, 2, "bicubic") == 64
    assert ffi.resize_aa_tables((64, 64), (2, 3, 0, 0), (2, 3), "bicubic")[0][2].shape == (2, 64)
    (ys, yc, yw), (xs, xc, xw) = ffi.resize_aa_tables((496, 992), (32, 32, 0, 0), (32, 32), "bilinear")
    assert yw.shape == (32, 33) and xw.shape == (32, 63)


# ---- descriptor refusals: nothing is launched ------------------------------------------------------------------------
def _desc(**over):
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = buf.data_ptr() // 16 * 16 + 16
    d = ffi.ResizeAADesc()
    d.in_ = d.out = d.y_start = d.y_count = d.y_w = d.x_start = d.x_count = d.x_w = p
    keep = [buf, (ctypes.c_float * 8)(*([0.5] * 8)), (ctypes.c_float * 8)(*([0.25] * 8))]
    d.mean_host, d.std_host = keep[1], keep[2]
    d.B, d.Hs, d.Ws, d.c_in, d.H, d.W, d.c_out, d.y_taps, d.x_taps = 1, 80, 90, 3, 4, 4, 4, 5, 7
    for k, v in over.items():
        setattr(d, k, v)
    return d, keep


@pytest.mark.parametrize("fn", ["tfimm_hip_preprocess_resize_aa", "tfimm_hip_ref_preprocess_resize_aa"])
def test_descriptor_refusals_before_any_launch(fn):
    call = getattr(ffi.lib, fn)
    zero_std = (ctypes.c_float * 3)(1.0, 0.0, 1.0)
    bad = [dict(in_=None), dict(out=None), dict(y_start=None), dict(y_count=None), dict(y_w=None), dict(x_start=None),
           dict(x_count=None), dict(x_w=None), dict(mean_host=None), dict(std_host=None),
           dict(B=0), dict(Hs=0), dict(Ws=-1), dict(c_in=0), dict(H=0), dict(W=0), dict(c_out=0),
           dict(y_taps=0), dict(x_taps=-1), dict(y_taps=65), dict(x_taps=65),           # over TFIMM_RESIZE_AA_MAX_TAPS
           dict(c_in=9, c_out=16),                          # over TFIMM_PREPROCESS_MAX_CHANNELS
           dict(c_in=5, c_out=4),                           # more channels than are stored
           dict(std_host=zero_std),
           dict(pad_t=1, c_out=8), dict(pad_r=2, c_in=5, c_out=8),    # the zero-bordered layout has 4 channels
           dict(pad_l=-1)]
    for over in bad:
        d, keep = _desc(**over)
        assert call(ctypes.byref(d), None) == -1, over
        assert b"preprocess_resize_aa" in ffi.lib.tfimm_hip_last_error(), over
    assert call(None, None) == -1


def test_resize_aa_desc_and_constants_match_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfimm_hip.h")).read()
    body = hdr[hdr.index("typedef struct tfimm_resize_aa_desc {"):hdr.index("} tfimm_resize_aa_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    names = []
    for decl in body.split(";"):
        toks = [t for t in decl.replace("*", " ").split() if t != "const"]
        if toks:
            names += [n.strip() for n in " ".join(toks[1:]).split(",")]
    assert names == [f[0].rstrip("_") for f in ffi.ResizeAADesc._fields_], names
    assert ctypes.sizeof(ffi.ResizeAADesc) == 10 * 8 + 13 * 4 + 4          # 13 ints, padded to the pointers' alignment
    for name in ("MAX_TAPS", "TILE_ROWS", "TILE_COLS", "MAX_BLOCKS"):
        assert int(re.search(rf"#define TFIMM_RESIZE_AA_{name} (\d+)", hdr).group(1)) == getattr(ffi, "RESIZE_AA_" + name)

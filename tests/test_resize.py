"""Resize + centre crop + normalise of uint8 images, the host side (no GPU): the geometry rule, the restatement of the
resampling (tests/resize_ref.py) pinned by hand-computed answers and by the oracle, the library's host tap function held to
the restatement bit for bit, ``DeferredInput.numpy()`` with a resize spec, the descriptor refusals of
tfimm_hip_preprocess_resize and the ``ValueError``s of ``create_preprocessing(resize=True)``."""
import ctypes

import numpy as np
import pytest
import torch

import resize_ref as rr
import test_architectures  # noqa: F401  (registers the miniature configs)
import tfimm
from oracle import ops
from tfimm.engine import ffi
from tfimm.models import DeferredInput
from tfimm.models.factory import resize_geometry


# ---- geometry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src, input_size, crop_pct, want", [
    ((480, 640), 224, 0.875, (256, 341, 16, 58)),        # 58.5 rounds to the even 58
    ((640, 480), 224, 0.875, (341, 256, 58, 16)),
    ((500, 500), 224, 0.9, (248, 248, 12, 12)),
    ((380, 380), 380, 1.0, (380, 380, 0, 0)),
    ((37, 53), 16, 0.875, (18, 25, 1, 4)),               # 4.5 rounds to the even 4
    ((53, 37), (16, 16), 0.875, (25, 18, 4, 1)),
    ((480, 640), (224, 224), 1.0, (224, 298, 0, 37)),    # crop_pct = 1: only the longer side is cropped
    ((100, 300), (64, 32), 0.875, (73, 36, 4, 2)),       # non-square input_size: no aspect preservation
    ((100, 300), (64, 32), 1.0, (64, 32, 0, 0)),
    ((7, 7), (72, 56), 0.9, (80, 62, 4, 3)),
])
def test_geometry_known_answers(src, input_size, crop_pct, want):
    assert resize_geometry(src, input_size, crop_pct) == want
    assert all(isinstance(v, int) for v in resize_geometry(src, input_size, crop_pct))


def test_geometry_refuses_nonsense():
    for bad in (((0, 4), 4, 1.0), ((4, 4), 4, 0.0), ((4, 4), 4, 1.5), ((4, 4), (0, 4), 0.9)):
        with pytest.raises(ValueError):
            resize_geometry(*bad)


# ---- the restatement, pinned ---------------------------------------------------------------------------------------
def test_bilinear_restatement_2x2_to_4x4_by_hand():
    """scale 0.5: loc = -0.25, 0.25, 0.75, 1.25 -> (lo, hi, frac) = (0, 0, .75), (0, 1, .25), (0, 1, .75), (1, 1, .25)"""
    idx, w = rr.bilinear_taps(2, 4)
    assert idx.tolist() == [[0, 0], [0, 1], [0, 1], [1, 1]]
    assert w.tolist() == [[0.25, 0.75], [0.75, 0.25], [0.25, 0.75], [0.75, 0.25]]
    x = np.array([[0.0, 10.0], [20.0, 30.0]], np.float32).reshape(1, 2, 2, 1)
    want = [[0.0, 2.5, 7.5, 10.0], [5.0, 7.5, 12.5, 15.0], [15.0, 17.5, 22.5, 25.0], [20.0, 22.5, 27.5, 30.0]]
    assert rr.resize_bilinear(x, (4, 4))[0, :, :, 0].tolist() == want


def test_bilinear_restatement_one_pixel_wide_by_hand():
    """a 3 x 1 image to 6 x 3: every column equals the vertical interpolation, loc = -0.25 ... 2.25"""
    x = np.array([0.0, 30.0, 60.0], np.float32).reshape(1, 3, 1, 1)
    out = rr.resize_bilinear(x, (6, 3))[0, :, :, 0]
    assert out.tolist() == [[v] * 3 for v in (0.0, 7.5, 22.5, 37.5, 52.5, 60.0)]
    assert rr.bilinear_taps(1, 3)[0].tolist() == [[0, 0]] * 3


def _from_taps(x, ty, tx):
    """bicubic sums over fixed four-tap tables, vertical pass first, each sum from 0.0 in tap order"""
    (iy, wy), (ix, wx) = ty, tx
    rows = np.zeros((x.shape[0], len(iy), x.shape[2], x.shape[3]), np.float32)
    for t in range(4):
        rows = rows + wy[None, :, t, None, None] * x[:, iy[:, t]]
    out = np.zeros((x.shape[0], len(iy), len(ix), x.shape[3]), np.float32)
    for t in range(4):
        out = out + wx[None, None, :, t, None] * rows[:, :, ix[:, t]]
    return out


@pytest.mark.parametrize("src, size", [((5, 7), (8, 8)), ((37, 53), (18, 25)), ((6, 6), (6, 6)), ((1, 3), (4, 2))])
def test_bicubic_taps_restatement_is_the_oracle(src, size):
    """the four-tap form (dropped tap = +0.0 at a clamped index) gives the oracle's bits"""
    x = np.random.default_rng(3).integers(0, 256, (2, *src, 3)).astype(np.float32)
    want = ops.resize_bicubic_tf(torch.from_numpy(x), size).numpy()
    got = _from_taps(x, rr.bicubic_taps(src[0], size[0]), rr.bicubic_taps(src[1], size[1]))
    assert np.array_equal(got, want)


def test_bicubic_identity_weights_are_exact():
    idx, w = rr.bicubic_taps(7, 7)
    assert w.tolist() == [[0.0, 1.0, 0.0, 0.0]] * 7 and idx[:, 1].tolist() == list(range(7))


# ---- tfimm_hip_resize_taps against the restatement -------------------------------------------------------------------
PAIRS = [(5, 8), (53, 25), (7, 7), (1, 4), (640, 341)]


@pytest.mark.parametrize("method", ["bicubic", "bilinear"])
@pytest.mark.parametrize("n_in, n_resized", PAIRS)
def test_host_tap_function_equals_restatement_bit_for_bit(n_in, n_resized, method):
    idx_ref, w_ref = (rr.bicubic_taps if method == "bicubic" else rr.bilinear_taps)(n_in, n_resized)
    windows = [(0, n_resized), (n_resized // 4, max(n_resized // 2, 1)), (n_resized - 1, 1)]
    for first, n_out in windows:
        idx, w = ffi.resize_taps(n_in, n_resized, first, n_out, method)
        assert idx.dtype == np.int32 and w.dtype == np.float32 and idx.shape == (n_out, 4 if method == "bicubic" else 2)
        assert np.array_equal(idx, idx_ref[first:first + n_out]), (first, n_out)
        assert np.array_equal(w.view(np.uint32), w_ref[first:first + n_out].view(np.uint32)), (first, n_out)
        assert idx.min() >= 0 and idx.max() < n_in


def test_host_tap_function_refuses_bad_windows():
    idx, w = (ctypes.c_int32 * 16)(), (ctypes.c_float * 16)()
    lib = ffi.lib
    assert lib.tfimm_hip_resize_taps(5, 8, 0, 4, 1, None, w) == -1
    assert lib.tfimm_hip_resize_taps(5, 8, 6, 4, 1, idx, w) == -1            # window past the resized axis
    assert lib.tfimm_hip_resize_taps(0, 8, 0, 4, 1, idx, w) == -1
    assert lib.tfimm_hip_resize_taps(5, 8, 0, 4, 2, idx, w) == -1            # unknown method
    assert b"resize_taps" in lib.tfimm_hip_last_error()
    assert lib.tfimm_hip_resize_taps(5, 8, 4, 4, 1, idx, w) == 0


# ---- DeferredInput.numpy() with a resize spec -----------------------------------------------------------------------
def _spec(name):
    cfg = tfimm.models.registry.model_config(name)
    n = cfg.in_channels
    mean = np.tile(np.asarray(cfg.mean, np.float64), n)[:n].astype(np.float32)
    std = np.tile(np.asarray(cfg.std, np.float64), n)[:n].astype(np.float32)
    return cfg, mean, std


@pytest.mark.parametrize("name, src", [
    ("vit_test_model", (37, 53)),                      # bicubic, 32 x 32, crop_pct 0.875 (ViTConfig defaults)
    ("vit_test_model", (20, 17)),                      # upscale, tall
    ("resnet_test_model_1", (53, 37)),                 # bilinear
    ("resnet_test_model_1", (32, 32)),                 # source = input size, crop_pct < 1: still resampled
    ("swin_shift_test_model", (70, 90)),               # non-square input size (64, 32)
])
def test_deferred_numpy_equals_cropped_restatement(name, src):
    cfg, mean, std = _spec(name)
    u8 = np.random.default_rng(11).integers(0, 256, (2, *src, cfg.in_channels), dtype=np.uint8)
    d = tfimm.create_preprocessing(name, defer=True, resize=True)(u8)
    assert isinstance(d, DeferredInput) and d.shape == u8.shape
    assert d.resize == (cfg.interpolation, float(cfg.crop_pct), tuple(cfg.input_size))
    geo = resize_geometry(src, cfg.input_size, cfg.crop_pct)
    want = rr.resize_crop_normalise(u8, geo, cfg.input_size, cfg.interpolation, mean, std)
    got = d.numpy()
    assert got.dtype == np.float32 and got.shape == (2, *cfg.input_size, cfg.in_channels)
    assert np.array_equal(got, want)
    # a single image and a torch tensor give the same pixels
    assert np.array_equal(tfimm.create_preprocessing(name, defer=True, resize=True)(u8[0]).numpy(), want[0])
    assert np.array_equal(tfimm.create_preprocessing(name, defer=True, resize=True)(torch.from_numpy(u8)).numpy(), want)


def test_both_interpolations_are_covered_by_the_minis():
    assert tfimm.models.registry.model_config("vit_test_model").interpolation == "bicubic"
    assert tfimm.models.registry.model_config("resnet_test_model_1").interpolation == "bilinear"


def test_identity_geometry_is_the_plain_preprocessing():
    """crop_pct = 1 and source = input size: weights (0, 1, 0, 0) / fraction 0, so nothing is resampled"""
    u8 = np.random.default_rng(12).integers(0, 256, (1, 9, 9, 3), dtype=np.uint8)
    plain = DeferredInput(u8, (0.5, 0.4, 0.3), (0.2, 0.3, 0.25)).numpy()
    for method in ("bicubic", "bilinear"):
        d = DeferredInput(u8, (0.5, 0.4, 0.3), (0.2, 0.3, 0.25), resize=(method, 1.0, (9, 9)))
        assert np.array_equal(d.numpy(), plain)


def test_resize_without_defer_or_with_float_input_raises():
    with pytest.raises(ValueError, match="defer"):
        tfimm.create_preprocessing("vit_test_model", resize=True)
    pre = tfimm.create_preprocessing("vit_test_model", defer=True, resize=True)
    with pytest.raises(ValueError, match="uint8"):
        pre(np.zeros((1, 40, 40, 3), np.float32))
    with pytest.raises(ValueError, match="uint8"):
        pre(torch.zeros(1, 40, 40, 3))
    # the flag changes nothing for callers that do not set it
    plain = tfimm.create_preprocessing("vit_test_model", defer=True)(np.zeros((1, 40, 40, 3), np.uint8))
    assert plain.resize is None


# ---- descriptor refusals: nothing is launched ------------------------------------------------------------------------
def _desc(**over):
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = buf.data_ptr() // 16 * 16 + 16
    d = ffi.ResizeDesc()
    d.in_ = d.out = d.y_idx = d.y_w = d.x_idx = d.x_w = p
    keep = [buf, (ctypes.c_float * 8)(*([0.5] * 8)), (ctypes.c_float * 8)(*([0.25] * 8))]
    d.mean_host, d.std_host = keep[1], keep[2]
    d.B, d.Hs, d.Ws, d.c_in, d.H, d.W, d.c_out, d.taps = 1, 5, 7, 3, 4, 4, 4, 4
    for k, v in over.items():
        setattr(d, k, v)
    return d, keep


@pytest.mark.parametrize("fn", ["tfimm_hip_preprocess_resize", "tfimm_hip_ref_preprocess_resize"])
def test_descriptor_refusals_before_any_launch(fn):
    call = getattr(ffi.lib, fn)
    zero_std = (ctypes.c_float * 3)(1.0, 0.0, 1.0)
    bad = [dict(in_=None), dict(out=None), dict(y_idx=None), dict(y_w=None), dict(x_idx=None), dict(x_w=None),
           dict(mean_host=None), dict(std_host=None),
           dict(B=0), dict(Hs=0), dict(Ws=-1), dict(c_in=0), dict(H=0), dict(W=0), dict(c_out=0),
           dict(taps=3), dict(taps=0), dict(taps=8),
           dict(c_in=9, c_out=16),                          # over TFIMM_PREPROCESS_MAX_CHANNELS
           dict(c_in=5, c_out=4),                           # more channels than are stored
           dict(std_host=zero_std),
           dict(pad_t=1, c_out=8), dict(pad_r=2, c_in=5, c_out=8),    # the zero-bordered layout has 4 channels
           dict(pad_l=-1)]
    for over in bad:
        d, keep = _desc(**over)
        assert call(ctypes.byref(d), None) == -1, over
        assert b"preprocess_resize" in ffi.lib.tfimm_hip_last_error(), over
    assert call(None, None) == -1


def test_resize_desc_layout_matches_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfimm_hip.h")).read()
    body = hdr[hdr.index("typedef struct tfimm_resize_desc {"):hdr.index("} tfimm_resize_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    names = []
    for decl in body.split(";"):
        toks = [t for t in decl.replace("*", " ").split() if t != "const"]
        if toks:
            names += [n.strip() for n in " ".join(toks[1:]).split(",")]
    assert names == [f[0].rstrip("_") for f in ffi.ResizeDesc._fields_], names
    assert ctypes.sizeof(ffi.ResizeDesc) == 8 * 8 + 12 * 4

"""pytest -m gpu: tfimm_hip_preprocess_resize -- resize + centre crop + normalise of a uint8 batch in one launch -- against
the host restatement (tests/resize_ref.py), BIT FOR BIT: the arithmetic is fully specified (tap tables from the host, every
product and sum a separate float32 operation in the restatement's order), so ``np.array_equal`` is the bar: bf16 output
against the bf16-rounded restatement, float32 output against the restatement itself.  Then the path through
``create_preprocessing(defer=True, resize=True)`` / ``Model.__call__``: a model fed the deferred uint8 batch computes what it
computes from ``DeferredInput.numpy()``, eagerly, from a replayed recording, for a second source size, on parallel
branches and on the float32 verification path."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hip_ops as ho
import resize_ref as rr
import test_architectures  # noqa: F401
import tfimm
from tfimm.architectures.resnet import ResNet, ResNetConfig
from tfimm.architectures.vit import ViT, ViTConfig
from tfimm.engine import ffi, precision
from tfimm.models import is_model, register_model
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406, 0.5, 0.45, 0.3, 0.6, 0.52)
STD = (0.229, 0.224, 0.225, 0.25, 0.21, 0.3, 0.27, 0.2)


def resize_op(u8, geometry, size, method, c_out, pad=(0, 0, 0, 0), f32=False):
    """the op through the C ABI: tap tables from the library's host function, uploaded; returns the output tensor"""
    B, Hs, Ws, c_in = u8.shape
    Rh, Rw, top, left = geometry
    H, W = size
    iy, wy = ffi.resize_taps(Hs, Rh, top, H, method)
    ix, wx = ffi.resize_taps(Ws, Rw, left, W, method)
    tabs = [torch.from_numpy(t).to(ho.DEV) for t in (iy, wy, ix, wx)]
    x = torch.from_numpy(u8).to(ho.DEV)
    pt, pb, pl, pr = pad
    out = torch.full((B, H + pt + pb, W + pl + pr, c_out), 7.0, dtype=torch.float32 if f32 else torch.bfloat16, device=ho.DEV)
    d = ffi.ResizeDesc()
    d.in_, d.out = x.data_ptr(), out.data_ptr()
    d.y_idx, d.y_w, d.x_idx, d.x_w = (t.data_ptr() for t in tabs)
    mean, std = (C.c_float * c_in)(*MEAN[:c_in]), (C.c_float * c_in)(*STD[:c_in])
    d.mean_host, d.std_host = mean, std
    d.B, d.Hs, d.Ws, d.c_in, d.H, d.W, d.c_out, d.taps = B, Hs, Ws, c_in, H, W, c_out, iy.shape[1]
    d.pad_t, d.pad_b, d.pad_l, d.pad_r = pad
    fn = ffi.lib.tfimm_hip_ref_preprocess_resize if f32 else ffi.lib.tfimm_hip_preprocess_resize
    ffi.check(fn(C.byref(d), ho.stream()), "preprocess_resize")
    ho.sync()
    return out.float().cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(batch, src, c_in, geometry, size, method):
    """seeded pixels and their restatement (float32, channels [0, c_in)), computed once per case"""
    u8 = np.random.default_rng(batch * 1000003 + src[0] * 1009 + src[1] * 13 + c_in).integers(0, 256, (batch, *src, c_in), dtype=np.uint8)
    ref = rr.resize_crop_normalise(u8, geometry, size, method, np.float32(MEAN[:c_in]), np.float32(STD[:c_in]))
    for a in (u8, ref):
        a.setflags(write=False)
    return u8, ref


def padded(ref, c_out):
    out = np.zeros(ref.shape[:3] + (c_out,), np.float32)
    out[..., :ref.shape[3]] = ref
    return out


UP = dict(src=(5, 7), geometry=(8, 8, 0, 0), size=(8, 8))                    # border taps dropped on all four sides
DOWN = dict(src=(37, 53), geometry=(18, 25, 1, 4), size=(16, 16))            # 2.3 x down, input 16, crop_pct 0.875
TALL = dict(src=(53, 37), geometry=(25, 18, 4, 1), size=(16, 16))
METHODS = ["bicubic", "bilinear"]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape, batch", [(UP, 3), (DOWN, 2), (TALL, 2)], ids=["up", "down", "tall"])
def test_bf16_output_equals_rounded_restatement(shape, batch, method):
    u8, ref = case(batch, shape["src"], 3, shape["geometry"], shape["size"], method)
    got = resize_op(u8, shape["geometry"], shape["size"], method, 4)
    assert np.array_equal(got, rr.to_bf16(padded(ref, 4)))


@pytest.mark.parametrize("method", METHODS)
def test_identity_equals_preprocess_input_bit_for_bit(method):
    """crop_pct = 1, source = input size: bilinear fraction 0, bicubic at table offset 0 = weights (0, 1, 0, 0) exactly"""
    u8 = np.random.default_rng(21).integers(0, 256, (2, 9, 11, 3), dtype=np.uint8)
    got = resize_op(u8, (9, 11, 0, 0), (9, 11), method, 4)
    plain = ho.preprocess_input(torch.from_numpy(u8).to(ho.DEV), 4, MEAN[:3], STD[:3])
    ho.sync()
    assert np.array_equal(got, plain.float().cpu().numpy())
    assert np.array_equal(got, rr.to_bf16(padded(rr.normalise(u8.astype(np.float32), np.float32(MEAN[:3]), np.float32(STD[:3])), 4)))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("c_in, c_out", [(1, 4), (4, 4), (5, 8), (8, 8), (3, 6)])
def test_channel_variants(c_in, c_out, method):
    u8, ref = case(2, DOWN["src"], c_in, DOWN["geometry"], DOWN["size"], method)
    got = resize_op(u8, DOWN["geometry"], DOWN["size"], method, c_out)
    assert np.array_equal(got, rr.to_bf16(padded(ref, c_out)))            # padded channels are 0


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("pad", [(3, 3, 3, 3), (0, 1, 0, 1)])
def test_padded_layout_border_zeros_and_interior(pad, method):
    u8, ref = case(2, DOWN["src"], 3, DOWN["geometry"], DOWN["size"], method)
    got = resize_op(u8, DOWN["geometry"], DOWN["size"], method, 4, pad=pad)
    pt, pb, pl, pr = pad
    H, W = DOWN["size"]
    assert got.shape == (2, H + pt + pb, W + pl + pr, 4)
    interior = got[:, pt:pt + H, pl:pl + W]
    assert np.array_equal(interior, resize_op(u8, DOWN["geometry"], DOWN["size"], method, 4))
    assert np.array_equal(interior, rr.to_bf16(padded(ref, 4)))
    border = got.copy()
    border[:, pt:pt + H, pl:pl + W] = 0
    assert not border.any()                                               # the kernel writes the border zeros itself


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", [UP, DOWN], ids=["up", "down"])
def test_float32_variant_equals_restatement(shape, method):
    u8, ref = case(2, shape["src"], 3, shape["geometry"], shape["size"], method)
    assert np.array_equal(resize_op(u8, shape["geometry"], shape["size"], method, 3, f32=True), ref)
    assert np.array_equal(resize_op(u8, shape["geometry"], shape["size"], method, 4, f32=True), padded(ref, 4))


def test_more_output_pixels_than_threads_in_the_grid():
    """5 x 464 x 464 output pixels: more than the 4096 blocks x 256 threads the launch is capped at, so threads stride on"""
    geo, size = (480, 470, 8, 3), (464, 464)
    assert 5 * 464 * 464 > 4096 * 256
    u8, ref = case(5, (150, 140), 3, geo, size, "bicubic")
    assert np.array_equal(resize_op(u8, geo, size, "bicubic", 4), rr.to_bf16(padded(ref, 4)))


# ---- through create_preprocessing / Model.__call__ ---------------------------------------------------------------------
def _model(name):
    model = tfimm.create_model(name)
    model.set_weights(synthetic_weights(model, 2021))
    return model, tfimm.create_preprocessing(name, defer=True, resize=True)


def _pixels(seed, src, batch=4):
    return np.random.default_rng(seed).integers(0, 256, (batch, *src, 3), dtype=np.uint8)


@pytest.mark.parametrize("name, src, src2", [
    ("resnet_test_model_1", (48, 56), (41, 35)),                  # bilinear, 32 x 32, the padded layout of the stem
    ("vit_test_model", (56, 48), (33, 70)),                       # bicubic
    ("efficientnet_same_test_model", (67, 75), (90, 61)),         # bicubic, odd 45 x 45
    ("swin_test_model", (96, 110), (100, 70)),                    # runs only at its configured size: the program still sees 64 x 64
])
def test_model_on_deferred_resize_equals_model_on_its_numpy(name, src, src2):
    model, pre = _model(name)
    first = None
    for call in range(3):                                         # eager, recording, replay with fresh pixels
        u8 = _pixels(100 + call, src)
        got = model(pre(u8)).numpy()
        assert got.shape[0] == 4 and np.isfinite(got).all()
        assert np.array_equal(got, model(pre(u8).numpy()).numpy()), f"call {call}"
        first = got if first is None else first
    recorded = [k for k in model._captured if k[-1] is not None and len(k[-1]) == 3]
    assert len(recorded) == 1 and ("src",) + src in recorded[0]
    for call in range(3):                                         # a second source size: a new recording, its own tables
        u8 = _pixels(200 + call, src2)
        got = model(pre(u8)).numpy()
        assert np.array_equal(got, model(pre(u8).numpy()).numpy()), f"second size, call {call}"
        assert not np.array_equal(got, first)
    assert len([k for k in model._captured if k[-1] is not None and len(k[-1]) == 3]) == 2
    # back to the first size: its recording, its tables
    u8 = _pixels(100, src)
    assert np.array_equal(model(pre(u8)).numpy(), first)
    plan = next(p for k, p in model._plans.items() if ("src",) + src in k)
    with pytest.raises(NotImplementedError, match="resize"):
        plan.export()


# crop_pct = 1.0 -- the default of several families: the geometry of a square model is (H, W, 0, 0) for EVERY square source and
# that of a non-square model for every source at all, so "nothing is cropped" must not be read as "nothing to resample"
if not is_model("vit_crop1_test_model"):

    @register_model
    def vit_crop1_test_model():
        return ViT, ViTConfig(name="vit_crop1_test_model", nb_classes=12, input_size=(32, 32), patch_size=8, embed_dim=4,
                              nb_blocks=2, nb_heads=2, crop_pct=1.0)

    @register_model
    def resnet_crop1_test_model():
        return ResNet, ResNetConfig(name="resnet_crop1_test_model", nb_classes=12, input_size=(32, 32), block="basic_block",
                                    nb_blocks=(1, 1, 1, 1), nb_channels=(2, 4, 6, 8), crop_pct=1.0)

    @register_model
    def resnet_crop1_wide_test_model():
        return ResNet, ResNetConfig(name="resnet_crop1_wide_test_model", nb_classes=12, input_size=(32, 48), block="basic_block",
                                    nb_blocks=(1, 1, 1, 1), nb_channels=(2, 4, 6, 8), crop_pct=1.0)


@pytest.mark.parametrize("name, sources", [
    ("vit_crop1_test_model", [(48, 48), (20, 20), (32, 32), (40, 50)]),           # bicubic: larger, smaller, equal, not square
    ("resnet_crop1_test_model", [(20, 20), (64, 64), (32, 32)]),                  # bilinear, the padded layout
    ("resnet_crop1_wide_test_model", [(50, 70), (20, 30), (32, 48)]),             # non-square input size: never cropped
])
def test_model_with_crop_pct_one_resamples_every_other_source_size(name, sources):
    from tfimm.models.factory import resize_geometry
    model, pre = _model(name)
    H, W = model.cfg.input_size
    seen = []
    for i, src in enumerate(sources):
        if src[0] == src[1] or H != W:
            assert resize_geometry(src, (H, W), 1.0) == (H, W, 0, 0)
        for call in range(2):                                     # eager, then the recording
            u8 = _pixels(600 + 10 * i + call, src)
            got = model(pre(u8)).numpy()
            assert np.isfinite(got).all()
            assert np.array_equal(got, model(pre(u8).numpy()).numpy()), f"{src}, call {call}"
        assert not any(np.array_equal(got, g) for g in seen)
        seen.append(got)
    # only the source that already has the input size takes the plain conversion
    plans = {k[-1][1:]: len(p._resize_tabs) for k, p in model._plans.items() if isinstance(k[-1], tuple)}
    assert plans == {tuple(s): (0 if tuple(s) == (H, W) else 1) for s in sources}, plans


def test_model_resize_on_parallel_branches():
    model, pre = _model("resnet_test_model_1")
    model.branches = 2
    for call in range(3):
        u8 = _pixels(300 + call, (50, 45))
        got = model(pre(u8)).numpy()
        assert np.array_equal(got, model(pre(u8).numpy()).numpy()), f"call {call}"
    assert [k for k in model._plans if "branches" in k and ("src", 50, 45) in k]
    model.branches = 1
    assert np.array_equal(model(pre(u8)).numpy(), got)


def test_model_resize_micro_batches_slice_the_uint8_batch():
    model, pre = _model("vit_test_model")
    u8 = _pixels(400, (40, 52), batch=5)
    model.micro_batch = 2                                         # chunks of 2, 2 and 1 images
    for call in range(3):
        assert np.array_equal(model(pre(u8)).numpy(), model(pre(u8).numpy()).numpy()), f"call {call}"
    assert [k for k in model._plans if k[3] == 1 and ("src", 40, 52) in k]


def test_model_resize_on_the_float32_path():
    model, pre = _model("vit_test_model")
    u8 = _pixels(500, (56, 48))
    with precision.use("fp32"):
        got = model(pre(u8))
        assert got.torch().element_size() == 4
        assert np.array_equal(got.numpy(), model(pre(u8).numpy()).numpy())
    bf16 = model(pre(u8)).numpy()
    assert np.array_equal(bf16, model(pre(u8).numpy()).numpy())
    assert not np.array_equal(bf16, got.numpy())

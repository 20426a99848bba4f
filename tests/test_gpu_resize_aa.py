"""pytest -m gpu: tfimm_hip_preprocess_resize_aa -- ANTIALIASED resize + centre crop + normalise of a uint8 batch in one
launch -- against the host restatement (tests/resize_aa_ref.py), BIT FOR BIT: the arithmetic is fully specified (span tables
from the host, every product and sum a separate float32 operation in the restatement's order), so ``np.array_equal`` is the
bar: bf16 output against the bf16-rounded restatement, float32 output against the restatement itself.  Then the path through
``create_preprocessing(defer=True, resize=True, antialias=True)`` / ``Model.__call__``: a model fed the deferred uint8 batch
computes what it computes from ``DeferredInput.numpy()``, eagerly, from a replayed recording, for a second source size, next
to the non-antialiased input of the same size, on parallel branches, in micro-batches and on the float32 path."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hip_ops as ho
import resize_aa_ref as ra
import test_architectures  # noqa: F401
import tfimm
from test_gpu_resize import MEAN, STD
from tfimm.engine import ffi, precision
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu

TR, TC, MAX_BLOCKS = ffi.RESIZE_AA_TILE_ROWS, ffi.RESIZE_AA_TILE_COLS, ffi.RESIZE_AA_MAX_BLOCKS


def launch(u8, tables, size, c_out, pad=(0, 0, 0, 0), f32=False, taps=None):
    """the op through the C ABI over the given span tables, uploaded; returns (return code, output tensor); the output is
    pre-filled with 7.0"""
    B, Hs, Ws, c_in = u8.shape
    H, W = size
    tabs = [torch.from_numpy(t).to(ho.DEV) for t in tables[0] + tables[1]]
    x = torch.from_numpy(u8).to(ho.DEV)
    pt, pb, pl, pr = pad
    out = torch.full((B, H + pt + pb, W + pl + pr, c_out), 7.0, dtype=torch.float32 if f32 else torch.bfloat16, device=ho.DEV)
    d = ffi.ResizeAADesc()
    d.in_, d.out = x.data_ptr(), out.data_ptr()
    d.y_start, d.y_count, d.y_w, d.x_start, d.x_count, d.x_w = (t.data_ptr() for t in tabs)
    mean, std = (C.c_float * c_in)(*MEAN[:c_in]), (C.c_float * c_in)(*STD[:c_in])
    d.mean_host, d.std_host = mean, std
    d.B, d.Hs, d.Ws, d.c_in, d.H, d.W, d.c_out = B, Hs, Ws, c_in, H, W, c_out
    d.y_taps, d.x_taps = taps or (tables[0][2].shape[1], tables[1][2].shape[1])
    d.pad_t, d.pad_b, d.pad_l, d.pad_r = pad
    fn = ffi.lib.tfimm_hip_ref_preprocess_resize_aa if f32 else ffi.lib.tfimm_hip_preprocess_resize_aa
    rc = fn(C.byref(d), ho.stream())
    ho.sync()
    return rc, out.float().cpu().numpy()


def resize_op(u8, geometry, size, method, c_out, pad=(0, 0, 0, 0), f32=False):
    tables = ffi.resize_aa_tables(u8.shape[1:3], geometry, size, method)
    rc, out = launch(u8, tables, size, c_out, pad, f32)
    ffi.check(rc, "preprocess_resize_aa")
    return out


@functools.lru_cache(maxsize=None)
def case(batch, src, c_in, geometry, size, method):
    """seeded pixels and their restatement (float32, channels [0, c_in)), computed once per case"""
    u8 = np.random.default_rng(batch * 1000003 + src[0] * 1009 + src[1] * 13 + c_in).integers(0, 256, (batch, *src, c_in), dtype=np.uint8)
    ref = ra.resize_crop_normalise(u8, geometry, size, method, np.float32(MEAN[:c_in]), np.float32(STD[:c_in]))
    for a in (u8, ref):
        a.setflags(write=False)
    return u8, ref


def padded(ref, c_out):
    out = np.zeros(ref.shape[:3] + (c_out,), np.float32)
    out[..., :ref.shape[3]] = ref
    return out


UP = dict(src=(5, 7), geometry=(8, 8, 0, 0), size=(8, 8))                    # spans clipped on all four sides
DOWN = dict(src=(37, 53), geometry=(18, 25, 1, 4), size=(16, 16))            # 2.1 x down: T = 11 (bicubic), 7 (bilinear)
TALL = dict(src=(53, 37), geometry=(25, 18, 4, 1), size=(16, 16))
STEEP = dict(src=(120, 97), geometry=(18, 18, 1, 1), size=(16, 16))          # 6.7 x and 5.4 x down: T = 29 and 23 bicubic
MIXED = dict(src=(40, 10), geometry=(16, 20, 0, 2), size=(16, 16))           # rows 2.5 x down, columns 2 x up
TINY = dict(src=(3, 4), geometry=(2, 2, 0, 0), size=(2, 2))                  # T clamped by the axis: 3 and 4
# larger than a tile in both directions, no multiple of it: (150, 200) -> (75, 100, 2, 5) -> (70, 90) for 16 x 32 tiles
BIG = dict(src=(2 * (4 * TR + 11), 2 * (2 * TC + 36)), geometry=(4 * TR + 11, 2 * TC + 36, 2, 5), size=(4 * TR + 6, 2 * TC + 26))
METHODS = ["bicubic", "bilinear"]
SHAPES = [(UP, 3), (DOWN, 2), (TALL, 2), (STEEP, 2), (MIXED, 2), (TINY, 3)]


def test_span_pitches_of_the_shapes():
    assert [ffi.resize_span_taps(*a, "bicubic") for a in ((37, 18), (53, 25), (120, 18), (97, 18), (3, 2), (4, 2))] == [11, 11, 29, 23, 3, 4]
    assert [ffi.resize_span_taps(*a, "bilinear") for a in ((37, 18), (53, 25), (5, 8))] == [7, 7, 3]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape, batch", SHAPES, ids=["up", "down", "tall", "steep", "mixed", "tiny"])
def test_bf16_output_equals_rounded_restatement(shape, batch, method):
    u8, ref = case(batch, shape["src"], 3, shape["geometry"], shape["size"], method)
    got = resize_op(u8, shape["geometry"], shape["size"], method, 4)
    assert np.array_equal(got, ra.to_bf16(padded(ref, 4)))


@pytest.mark.parametrize("method", METHODS)
def test_identity_equals_preprocess_input_bit_for_bit(method):
    """scale 1 on both axes: weights (0, 0, 1, 0, 0) exactly"""
    u8 = np.random.default_rng(21).integers(0, 256, (2, 9, 11, 3), dtype=np.uint8)
    got = resize_op(u8, (9, 11, 0, 0), (9, 11), method, 4)
    plain = ho.preprocess_input(torch.from_numpy(u8).to(ho.DEV), 4, MEAN[:3], STD[:3])
    ho.sync()
    assert np.array_equal(got, plain.float().cpu().numpy())


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("c_in, c_out", [(1, 4), (4, 4), (5, 8), (8, 8), (3, 6)])
def test_channel_variants(c_in, c_out, method):
    u8, ref = case(2, DOWN["src"], c_in, DOWN["geometry"], DOWN["size"], method)
    got = resize_op(u8, DOWN["geometry"], DOWN["size"], method, c_out)
    assert np.array_equal(got, ra.to_bf16(padded(ref, c_out)))            # padded channels are 0


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("pad", [(3, 3, 3, 3), (0, 1, 0, 1)])
def test_padded_layout_border_zeros_and_interior(pad, method):
    u8, ref = case(2, DOWN["src"], 3, DOWN["geometry"], DOWN["size"], method)
    got = resize_op(u8, DOWN["geometry"], DOWN["size"], method, 4, pad=pad)
    pt, pb, pl, pr = pad
    H, W = DOWN["size"]
    assert got.shape == (2, H + pt + pb, W + pl + pr, 4)
    interior = got[:, pt:pt + H, pl:pl + W]
    assert np.array_equal(interior, ra.to_bf16(padded(ref, 4)))
    border = got.copy()
    border[:, pt:pt + H, pl:pl + W] = 0
    assert not border.any()                                               # the kernel writes the border zeros itself


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", [UP, DOWN], ids=["up", "down"])
def test_float32_variant_equals_restatement(shape, method):
    u8, ref = case(2, shape["src"], 3, shape["geometry"], shape["size"], method)
    assert np.array_equal(resize_op(u8, shape["geometry"], shape["size"], method, 3, f32=True), ref)
    assert np.array_equal(resize_op(u8, shape["geometry"], shape["size"], method, 4, f32=True), padded(ref, 4))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("pad", [(0, 0, 0, 0), (3, 2, 3, 2)], ids=["plain", "padded"])
def test_output_larger_than_a_tile_in_both_directions(pad, method):
    """5 x 3 tiles per image, the last row and column of tiles partly filled; with the border the tiles sit at another offset
    of the image -- the result does not depend on the tiling"""
    H, W = BIG["size"]
    assert H > TR and W > TC and H % TR and W % TC and (H + 5) % TR and (W + 5) % TC
    u8, ref = case(2, BIG["src"], 3, BIG["geometry"], BIG["size"], method)
    got = resize_op(u8, BIG["geometry"], BIG["size"], method, 4, pad=pad)
    assert np.array_equal(got[:, pad[0]:pad[0] + H, pad[2]:pad[2] + W], ra.to_bf16(padded(ref, 4)))
    got[:, pad[0]:pad[0] + H, pad[2]:pad[2] + W] = 0
    assert not got.any()


def test_more_tiles_than_workgroups_in_the_grid():
    """one tile per image and more images than the launch has workgroups: they stride on"""
    batch = MAX_BLOCKS + 7
    assert DOWN["size"][0] <= TR and DOWN["size"][1] <= TC
    u8, ref = case(batch, DOWN["src"], 3, DOWN["geometry"], DOWN["size"], "bicubic")
    assert np.array_equal(resize_op(u8, DOWN["geometry"], DOWN["size"], "bicubic", 4), ra.to_bf16(padded(ref, 4)))


@pytest.mark.parametrize("method", METHODS)
def test_span_pitch_at_the_limit(method):
    """a 64-pixel axis shrunk far enough: T = 64 = TFIMM_RESIZE_AA_MAX_TAPS on both axes, every source pixel in every span"""
    src, geo, size = (64, 64), (2, 2, 0, 0), (2, 2)          # 2 * ceil(radius * 32) + 1 = 129 or 65 taps, cut to the axis
    assert ffi.resize_span_taps(64, 2, method) == ffi.RESIZE_AA_MAX_TAPS
    u8, ref = case(2, src, 3, geo, size, method)
    assert np.array_equal(resize_op(u8, geo, size, method, 4), ra.to_bf16(padded(ref, 4)))
    assert np.array_equal(resize_op(u8, geo, size, method, 3, f32=True), ref)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("taps", [(65, 64), (64, 65)])
def test_span_pitch_over_the_limit_is_refused_and_nothing_is_written(taps, f32):
    src, geo, size = (80, 80), (2, 3, 0, 0), (2, 3)
    u8 = np.random.default_rng(3).integers(0, 256, (1, *src, 3), dtype=np.uint8)
    tables = tuple((np.zeros(n, np.int32), np.full(n, t, np.int32), np.full((n, t), 1.0 / t, np.float32)) for n, t in zip(size, taps))
    rc, out = launch(u8, tables, size, 4, f32=f32, taps=taps)
    assert rc == -1 and b"TFIMM_RESIZE_AA_MAX_TAPS" in ffi.lib.tfimm_hip_last_error()
    assert (out == 7.0).all()
    rc, out = launch(u8, tables, size, 4, f32=f32, taps=(64, 64))                    # the same tables at the limit run
    assert rc == 0 and not (out == 7.0).any()


# ---- through create_preprocessing / Model.__call__ ---------------------------------------------------------------------
def _model(name):
    model = tfimm.create_model(name)
    model.set_weights(synthetic_weights(model, 2021))
    return model, tfimm.create_preprocessing(name, defer=True, resize=True, antialias=True)


def _pixels(seed, src, batch=4):
    return np.random.default_rng(seed).integers(0, 256, (batch, *src, 3), dtype=np.uint8)


def _resizing(model):
    return [k for k in model._captured if k[-1] is not None and len(k[-1]) == 3]


@pytest.mark.parametrize("name, src, src2", [
    ("resnet_test_model_1", (48, 56), (81, 35)),                  # bilinear, 32 x 32, the padded layout of the stem
    ("vit_test_model", (56, 48), (33, 90)),                       # bicubic
])
def test_model_on_deferred_antialiased_resize_equals_model_on_its_numpy(name, src, src2):
    model, pre = _model(name)
    first = None
    for call in range(3):                                         # eager, recording, replay with fresh pixels
        u8 = _pixels(100 + call, src)
        got = model(pre(u8)).numpy()
        assert got.shape[0] == 4 and np.isfinite(got).all()
        assert np.array_equal(got, model(pre(u8).numpy()).numpy()), f"call {call}"
        first = got if first is None else first
    assert len(_resizing(model)) == 1 and ("src",) + src + ("antialias",) in _resizing(model)[0]
    for call in range(3):                                         # a second source size: a new recording, its own tables
        u8 = _pixels(200 + call, src2)
        got = model(pre(u8)).numpy()
        assert np.array_equal(got, model(pre(u8).numpy()).numpy()), f"second size, call {call}"
        assert not np.array_equal(got, first)
    assert len(_resizing(model)) == 2
    # the first size without antialiasing: a third plan and recording, today's keys, another result
    plain = tfimm.create_preprocessing(name, defer=True, resize=True)
    u8 = _pixels(100, src)
    for call in range(2):
        got = model(plain(u8)).numpy()
        assert np.array_equal(got, model(plain(u8).numpy()).numpy()), f"not antialiased, call {call}"
    assert not np.array_equal(got, first)
    assert len(_resizing(model)) == 3 and sum(("src",) + src in k for k in _resizing(model)) == 1
    assert sum(("src",) + src in k for k in model._plans) == 1 and sum(("src",) + src + ("antialias",) in k for k in model._plans) == 1
    assert _resizing(model)[-1][-1][2] == (model.cfg.interpolation, float(model.cfg.crop_pct))
    # back to the first size, antialiased: its recording, its tables
    assert np.array_equal(model(pre(u8)).numpy(), first)
    plan = next(p for k, p in model._plans.items() if ("src",) + src + ("antialias",) in k)
    assert isinstance(next(iter(plan._resize_tabs.values()))[0], ffi.ResizeAADesc)
    with pytest.raises(NotImplementedError, match="resize"):
        plan.export()


def test_model_source_too_large_for_the_launch_raises():
    model, pre = _model("vit_test_model")
    with pytest.raises(ValueError, match="TFIMM_RESIZE_AA_MAX_TAPS"):
        model(pre(np.zeros((1, 600, 640, 3), np.uint8)))          # 600 -> 36: 16.7 x down, 69 taps


def test_model_antialiased_resize_on_parallel_branches():
    model, pre = _model("resnet_test_model_1")
    model.branches = 2
    for call in range(3):
        u8 = _pixels(300 + call, (70, 45))
        got = model(pre(u8)).numpy()
        assert np.array_equal(got, model(pre(u8).numpy()).numpy()), f"call {call}"
    assert [k for k in model._plans if "branches" in k and ("src", 70, 45, "antialias") in k]
    model.branches = 1
    assert np.array_equal(model(pre(u8)).numpy(), got)


def test_model_antialiased_resize_micro_batches_slice_the_uint8_batch():
    model, pre = _model("vit_test_model")
    u8 = _pixels(400, (60, 92), batch=5)
    model.micro_batch = 2                                         # chunks of 2, 2 and 1 images
    for call in range(3):
        assert np.array_equal(model(pre(u8)).numpy(), model(pre(u8).numpy()).numpy()), f"call {call}"
    assert [k for k in model._plans if k[3] == 1 and ("src", 60, 92, "antialias") in k]


def test_model_antialiased_resize_on_the_float32_path():
    model, pre = _model("vit_test_model")
    u8 = _pixels(500, (76, 48))
    with precision.use("fp32"):
        got = model(pre(u8))
        assert got.torch().element_size() == 4
        assert np.array_equal(got.numpy(), model(pre(u8).numpy()).numpy())
    bf16 = model(pre(u8)).numpy()
    assert np.array_equal(bf16, model(pre(u8).numpy()).numpy())
    assert not np.array_equal(bf16, got.numpy())

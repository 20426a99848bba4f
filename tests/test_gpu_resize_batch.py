"""pytest -m gpu: tfimm_hip_preprocess_resize_batch / _batch_aa -- resize + centre crop + normalise of a uint8 batch whose
images each have a SIZE OF THEIR OWN, in one launch -- BIT FOR BIT (``np.array_equal``) against the host restatement of every
image alone (tests/resize_ref.py, tests/resize_aa_ref.py) and against the uniform launches on that image at B = 1.  Then the
path through ``create_preprocessing(defer=True, resize=True[, antialias=True])`` / ``Model.__call__`` with the images passed
as a LIST: eagerly, recorded, replayed, for other sizes through the same plan and recording, after capacity growth, in
micro-batches, with ``branches = 2`` and on the float32 path."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hip_ops as ho
import resize_aa_ref as ra
import resize_ref as rr
import test_architectures  # noqa: F401
import test_gpu_resize as plain_t
import test_gpu_resize_aa as aa_t
import tfimm
from test_gpu_resize import MEAN, STD
from tfimm.engine import ffi, precision
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu

TR, TC, MAX_BLOCKS = ffi.RESIZE_AA_TILE_ROWS, ffi.RESIZE_AA_TILE_COLS, ffi.RESIZE_AA_MAX_BLOCKS
METHODS = ["bicubic", "bilinear"]
AA = [False, True]
AA_IDS = ["plain", "antialias"]

DOWN, TALL, STEEP, MIXED, BIG = aa_t.DOWN, aa_t.TALL, aa_t.STEEP, aa_t.MIXED, aa_t.BIG
UP = dict(src=(5, 7), geometry=(16, 16, 0, 0), size=(16, 16))                # upscaled, spans clipped on all four sides
IDENT = dict(src=(16, 16), geometry=(16, 16, 0, 0), size=(16, 16))           # tables (0, 1, 0, 0) / (0, 0, 1, 0, 0) exactly
M = [DOWN, TALL, STEEP, MIXED, UP, IDENT]                                    # the batch: odd byte offsets, many pitches
OUT = (16, 16)


@functools.lru_cache(maxsize=None)
def image(seed, src, c_in, geometry, size, method, aa):
    """seeded pixels of ONE image and its restatement (float32, channels [0, c_in)), computed once"""
    u8 = np.random.default_rng(seed * 1000003 + src[0] * 1009 + src[1] * 13 + c_in).integers(0, 256, (*src, c_in), dtype=np.uint8)
    ref = (ra if aa else rr).resize_crop_normalise(u8[None], geometry, size, method, np.float32(MEAN[:c_in]), np.float32(STD[:c_in]))[0]
    for a in (u8, ref):
        a.setflags(write=False)
    return u8, ref


def batch_of(cases, c_in, method, aa, seed=1):
    """(images, geometries, stacked restatement) of a list of cases going to one output size"""
    pairs = [image(seed + i, c["src"], c_in, c["geometry"], c["size"], method, aa) for i, c in enumerate(cases)]
    return [p[0] for p in pairs], [c["geometry"] for c in cases], np.stack([p[1] for p in pairs])


def padded(ref, c_out):
    out = np.zeros(ref.shape[:-1] + (c_out,), np.float32)
    out[..., :ref.shape[-1]] = ref
    return out


class Launch:
    """device buffers of the launch, allocated once at the given capacities, refilled and launched any number of times"""

    def __init__(self, B, c_in, size, method, aa, c_out, pad=(0, 0, 0, 0), f32=False, arena_bytes=1 << 20, w_floats=1 << 18,
                 taps_cap=ffi.RESIZE_AA_MAX_TAPS):
        H, W = size
        taps = 4 if method == "bicubic" else 2
        self.args = (size, method, aa, c_in, pad)
        self.f32, self.aa = f32, aa
        n_tab = B * (H + W) * (1 if aa else taps)
        self.arena = torch.zeros(arena_bytes, dtype=torch.uint8, device=ho.DEV)
        self.recs = torch.zeros(B * C.sizeof(ffi.ResizeBatchRec), dtype=torch.uint8, device=ho.DEV)
        self.ta = torch.zeros(n_tab, dtype=torch.int32, device=ho.DEV)
        self.tb = torch.zeros(n_tab, dtype=torch.int32, device=ho.DEV)
        self.w = torch.zeros(w_floats if aa else n_tab, dtype=torch.float32, device=ho.DEV)
        pt, pb, pl, pr = pad
        self.out = torch.full((B, H + pt + pb, W + pl + pr, c_out), 7.0, dtype=torch.float32 if f32 else torch.bfloat16, device=ho.DEV)
        d = self.d = ffi.ResizeBatchAADesc() if aa else ffi.ResizeBatchDesc()
        d.in_, d.recs, d.out, d.w = self.arena.data_ptr(), self.recs.data_ptr(), self.out.data_ptr(), self.w.data_ptr()
        d.in_bytes = arena_bytes
        if aa:
            d.start, d.count, d.w_floats, d.taps_cap, d.lds_bytes = self.ta.data_ptr(), self.tb.data_ptr(), w_floats, taps_cap, 0
        else:
            d.idx, d.taps = self.ta.data_ptr(), taps
        self.host = (C.c_float * c_in)(*MEAN[:c_in]), (C.c_float * c_in)(*STD[:c_in])
        d.mean_host, d.std_host = self.host
        d.B, d.c_in, d.H, d.W, d.c_out = B, c_in, H, W, c_out
        d.pad_t, d.pad_b, d.pad_l, d.pad_r = pad

    def fill(self, images, geometries):
        size, method, aa, c_in, pad = self.args
        t = ffi.resize_batch_tables([im.shape[:2] for im in images], geometries, size, method, aa, c_in=c_in, pad=pad)
        flat = np.concatenate([im.reshape(-1) for im in images])
        assert flat.size == t["in_bytes"] <= self.arena.numel() and t["w"].size <= self.w.numel()
        self.arena[:flat.size].copy_(torch.from_numpy(flat))
        self.recs.copy_(torch.from_numpy(t["recs"].view(np.uint8)))
        self.ta.copy_(torch.from_numpy(t["start"] if aa else t["idx"]))
        if aa:
            self.tb.copy_(torch.from_numpy(t["count"]))
        self.w[:t["w"].size].copy_(torch.from_numpy(t["w"]))
        return t

    def __call__(self):
        name = "tfimm_hip_" + ("ref_" if self.f32 else "") + "preprocess_resize_batch" + ("_aa" if self.aa else "")
        rc = getattr(ffi.lib, name)(C.byref(self.d), ho.stream())
        ho.sync()
        return rc, self.out.float().cpu().numpy()


def run(images, geometries, size, method, aa, c_out, **kw):
    """one launch over buffers a little larger than the batch needs"""
    kw.setdefault("arena_bytes", sum(im.size for im in images) + 1)
    kw.setdefault("w_floats", len(images) * (size[0] + size[1]) * ffi.RESIZE_AA_MAX_TAPS)
    L = Launch(len(images), images[0].shape[2], size, method, aa, c_out, **kw)
    L.fill(images, geometries)
    rc, out = L()
    ffi.check(rc, "preprocess_resize_batch")
    return out


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
def test_bf16_output_equals_rounded_restatement_of_every_image(method, aa):
    images, geos, ref = batch_of(M, 3, method, aa)
    assert len({im.shape[:2] for im in images}) == 6 and (images[0].size % 2) == 1        # the second image starts at an odd byte
    got = run(images, geos, OUT, method, aa, 4)
    for b in range(len(M)):
        assert np.array_equal(got[b], rr.to_bf16(padded(ref[b], 4))), f"image {b}"


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
def test_every_image_equals_the_uniform_launch_on_it_alone(method, aa):
    images, geos, _ = batch_of(M, 3, method, aa)
    got = run(images, geos, OUT, method, aa, 4)
    uniform = (aa_t if aa else plain_t).resize_op
    for b, (im, g) in enumerate(zip(images, geos)):
        assert np.array_equal(got[b], uniform(im[None], g, OUT, method, 4)[0]), f"image {b}"
    plain = ho.preprocess_input(torch.from_numpy(images[5][None].copy()).to(ho.DEV), 4, MEAN[:3], STD[:3])
    ho.sync()
    assert np.array_equal(got[5], plain.float().cpu().numpy()[0])                          # the identity image


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("c_in, c_out", [(1, 4), (4, 4), (5, 8), (8, 8), (3, 6)])
def test_channel_variants(c_in, c_out, method, aa):
    images, geos, ref = batch_of(M, c_in, method, aa)
    assert np.array_equal(run(images, geos, OUT, method, aa, c_out), rr.to_bf16(padded(ref, c_out)))


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("pad", [(3, 3, 3, 3), (0, 1, 0, 1)])
def test_padded_layout_border_zeros_and_interior(pad, method, aa):
    images, geos, ref = batch_of(M, 3, method, aa)
    got = run(images, geos, OUT, method, aa, 4, pad=pad)
    pt, pb, pl, pr = pad
    H, W = OUT
    assert got.shape == (len(M), H + pt + pb, W + pl + pr, 4)
    assert np.array_equal(got[:, pt:pt + H, pl:pl + W], rr.to_bf16(padded(ref, 4)))
    got[:, pt:pt + H, pl:pl + W] = 0
    assert not got.any()                                                                   # the kernel writes the border zeros itself


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
def test_float32_twins_equal_the_restatement_unrounded(method, aa):
    images, geos, ref = batch_of(M, 3, method, aa)
    assert np.array_equal(run(images, geos, OUT, method, aa, 3, f32=True), ref)
    assert np.array_equal(run(images, geos, OUT, method, aa, 4, f32=True), padded(ref, 4))


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("pad", [(0, 0, 0, 0), (3, 2, 3, 2)], ids=["plain", "padded"])
def test_two_sizes_to_an_output_larger_than_a_tile(pad, method, aa):
    """(150, 200) and (131, 1000) to 70 x 90: the second image's wide spans (10.5 x down) leave fewer rows to a tile, so tile
    shapes and tile counts differ inside one launch"""
    H, W = BIG["size"]
    other = dict(src=(131, 1000), geometry=(71, 95, 0, 2), size=BIG["size"])
    images, geos, ref = batch_of([BIG, other], 3, method, aa)
    L = Launch(2, 3, BIG["size"], method, aa, 4, pad=pad)
    t = L.fill(images, geos)
    if aa:
        assert t["recs"]["tile_rows"][0] == TR > t["recs"]["tile_rows"][1]
        assert t["recs"]["n_tiles"].tolist() == [-(-(H + pad[0] + pad[1]) // r) * 3 for r in t["recs"]["tile_rows"]]
    rc, got = L()
    assert rc == 0
    assert np.array_equal(got[:, pad[0]:pad[0] + H, pad[2]:pad[2] + W], rr.to_bf16(padded(ref, 4)))
    got[:, pad[0]:pad[0] + H, pad[2]:pad[2] + W] = 0
    assert not got.any()


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
def test_more_images_than_workgroups(aa):
    """MAX_BLOCKS + 7 images alternating two sizes, one tile each: the workgroups stride on"""
    n = MAX_BLOCKS + 7
    images, geos, ref = batch_of([DOWN, TALL], 3, "bicubic", aa)
    got = run([images[i % 2] for i in range(n)], [geos[i % 2] for i in range(n)], OUT, "bicubic", aa, 4)
    want = rr.to_bf16(padded(ref, 4))
    assert np.array_equal(got[0::2], np.broadcast_to(want[0], got[0::2].shape))
    assert np.array_equal(got[1::2], np.broadcast_to(want[1], got[1::2].shape))


@pytest.mark.parametrize("method", METHODS)
def test_span_pitch_at_the_limit_next_to_a_small_one(method):
    """64 x 64 -> 2 x 2: T = 64 on both axes, next to DOWN resized to 2 x 2 at its own pitches"""
    cases = [dict(src=(64, 64), geometry=(2, 2, 0, 0), size=(2, 2)), dict(src=DOWN["src"], geometry=(2, 3, 0, 0), size=(2, 2))]
    images, geos, ref = batch_of(cases, 3, method, True)
    L = Launch(2, 3, (2, 2), method, True, 4)
    t = L.fill(images, geos)
    assert t["max_taps"] == ffi.RESIZE_AA_MAX_TAPS == t["recs"]["y_taps"][0] and t["recs"]["y_taps"][1] < 64
    rc, got = L()
    assert rc == 0 and np.array_equal(got, rr.to_bf16(padded(ref, 4)))


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
def test_pitch_capacity_over_the_limit_is_refused_and_nothing_is_written(f32):
    images, geos, _ = batch_of(M, 3, "bicubic", True)
    L = Launch(len(M), 3, OUT, "bicubic", True, 4, f32=f32, taps_cap=ffi.RESIZE_AA_MAX_TAPS + 1)
    L.fill(images, geos)
    rc, out = L()
    assert rc == -1 and b"TFIMM_RESIZE_AA_MAX_TAPS" in ffi.lib.tfimm_hip_last_error()
    assert (out == 7.0).all()
    L.d.taps_cap = ffi.RESIZE_AA_MAX_TAPS                                                  # the same buffers at the limit run
    rc, out = L()
    assert rc == 0 and not (out == 7.0).any()


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
def test_refusals_launch_nothing(aa):
    images, geos, _ = batch_of(M, 3, "bilinear", aa)

    def refused(**kw):
        L = Launch(len(M), 3, OUT, "bilinear", aa, kw.pop("c_out", 4), pad=kw.pop("pad", (0, 0, 0, 0)))
        L.fill(images, geos)
        for k, v in kw.items():
            setattr(L.d, k, v)
        rc, out = L()
        return rc == -1 and (out == 7.0).all()

    assert refused(recs=None) and refused(in_=None) and refused(w=None)
    assert refused(B=0) and refused(H=0) and refused(in_bytes=0)
    assert refused(c_in=9) and refused(c_out=8, pad=(1, 1, 1, 1))
    L = Launch(len(M), 3, OUT, "bilinear", aa, 4)
    L.fill(images, geos)
    L.host[1][1] = 0.0                                                                     # std == 0
    rc, out = L()
    assert rc == -1 and (out == 7.0).all()


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
def test_the_launch_reads_the_buffers_not_baked_arguments(method, aa):
    """the same descriptor and device buffers, refilled with the batch in reverse order: the second batch's result"""
    images, geos, ref = batch_of(M, 3, method, aa)
    L = Launch(len(M), 3, OUT, method, aa, 4, pad=(3, 3, 3, 3))
    L.fill(images, geos)
    rc, first = L()
    assert rc == 0 and np.array_equal(first[:, 3:19, 3:19], rr.to_bf16(padded(ref, 4)))
    L.fill(images[::-1], geos[::-1])
    rc, second = L()
    assert rc == 0 and np.array_equal(second[:, 3:19, 3:19], rr.to_bf16(padded(ref[::-1], 4)))
    assert not np.array_equal(first, second)


# ---- through create_preprocessing / Model.__call__: the images always as a list -------------------------------------------
SIZES_A = [(48, 56), (81, 35), (33, 90), (40, 40)]
SIZES_B = [(56, 48), (35, 70), (64, 64), (37, 53)]
SIZES_LARGE = [(300, 260), (256, 384), (200, 333), (280, 280)]
MODELS = [("resnet_test_model_1", False), ("resnet_test_model_1", True), ("vit_test_model", False), ("vit_test_model", True)]
MODEL_IDS = ["resnet-bilinear", "resnet-bilinear-aa", "vit-bicubic", "vit-bicubic-aa"]


def _model(name, aa):
    model = tfimm.create_model(name)
    model.set_weights(synthetic_weights(model, 2021))
    return model, tfimm.create_preprocessing(name, defer=True, resize=True, antialias=aa)


def _images(seed, sizes):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _src(key):
    return [e for e in key if isinstance(e, tuple) and e and e[0] == "src"]


def _check(model, pre, imgs, what):
    got = model(pre(imgs)).numpy()
    assert got.shape[0] == len(imgs) and np.isfinite(got).all()
    assert np.array_equal(got, model(pre(imgs).numpy()).numpy()), what
    return got


@pytest.mark.parametrize("name, aa", MODELS, ids=MODEL_IDS)
def test_model_on_a_list_of_mixed_sizes_one_plan_one_recording(name, aa):
    model, pre = _model(name, aa)
    tag = ("src", "mixed") + (("antialias",) if aa else ())
    first = [_check(model, pre, _images(100 + call, SIZES_A), f"call {call}") for call in range(3)]   # eager, recording, replay
    assert not np.array_equal(first[0], first[2])
    recorded = [c for k, c in model._captured.items() if tag in k]
    assert len(recorded) == 1
    for call in range(3):                                          # four other sizes: the same plan, the same recording replayed
        _check(model, pre, _images(200 + call, SIZES_B), f"other sizes, call {call}")
    plans = [k for k in model._plans if _src(k)]
    caps = [k for k in model._captured if _src(k)]
    assert len(plans) == 1 and len(caps) == 1 and _src(plans[0]) == [tag] and _src(caps[0]) == [tag]
    assert model._captured[caps[0]] is recorded[0]                 # nothing re-recorded
    assert not any(isinstance(v, int) for k in list(model._plans) + list(model._captured) for e in _src(k) for v in e)
    # much larger images: capacities may grow and the step may be recorded again -- still one plan, one recording
    for call in range(2):
        _check(model, pre, _images(300 + call, SIZES_LARGE), f"large, call {call}")
    assert np.array_equal(model(pre(_images(100, SIZES_A))).numpy(), first[0])
    assert [k for k in model._plans if _src(k)] == plans and [k for k in model._captured if _src(k)] == caps
    plan = model._plans[plans[0]]
    assert isinstance(next(iter(plan._mixed.values()))["desc"], ffi.ResizeBatchAADesc if aa else ffi.ResizeBatchDesc)
    with pytest.raises(NotImplementedError, match="resize"):
        plan.export()


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
def test_model_micro_batches_slice_the_list(aa):
    model, pre = _model("vit_test_model", aa)
    imgs = _images(400, SIZES_A + [(60, 92)])
    model.micro_batch = 2                                          # chunks of 2, 2 and 1 images
    for call in range(3):
        _check(model, pre, imgs, f"call {call}")
    assert sorted(k[3] for k in model._plans if _src(k)) == [1, 2]


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
def test_model_with_branches_equals_one_branch(aa):
    model, pre = _model("resnet_test_model_1", aa)
    imgs = _images(500, SIZES_A)
    model.branches = 2
    got = [_check(model, pre, imgs, f"call {call}") for call in range(3)]
    model.branches = 1
    assert np.array_equal(model(pre(imgs)).numpy(), got[0]) and np.array_equal(got[0], got[2])


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
def test_model_on_the_float32_path(aa):
    model, pre = _model("vit_test_model", aa)
    imgs = _images(600, SIZES_B)
    with precision.use("fp32"):
        got = model(pre(imgs))
        assert got.torch().element_size() == 4
        assert np.array_equal(got.numpy(), model(pre(imgs).numpy()).numpy())
    bf16 = _check(model, pre, imgs, "bf16")
    assert not np.array_equal(bf16, got.numpy())


def test_model_image_outside_the_antialias_domain_raises_before_any_launch():
    model, pre = _model("vit_test_model", True)
    imgs = _images(700, SIZES_A[:2]) + [np.zeros((600, 640, 3), np.uint8)]       # 600 -> 36: 16.7 x down, 69 taps
    with pytest.raises(ValueError, match=r"image 2 .*TFIMM_RESIZE_AA_MAX_TAPS"):
        model(pre(imgs))
    assert not model._captured and not any(p._mixed for p in model._plans.values())

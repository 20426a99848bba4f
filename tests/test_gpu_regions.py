"""pytest -m gpu: tfimm_hip_preprocess_regions / _regions_aa -- resize + centre crop + normalise of BOXES inside larger uint8
frames, in one launch -- BIT FOR BIT (``np.array_equal``) against the host restatement of every slice (tests/resize_ref.py,
tests/resize_aa_ref.py) and against the tfimm_hip_preprocess_resize_batch[_aa] launch on the packed slices.  Then the path
through ``create_preprocessing(defer=True, resize=True[, antialias=True])`` / ``Model`` with ``pre(frames, boxes=...)``, held to
the list path ``pre([slices])`` on the same boxes: eagerly, recorded, replayed, for other frames and boxes through the same
plan and recording, after capacity growth, in micro-batches, with ``branches = 2``, on the float32 path, through ``top_k``,
``evaluate`` and ``EmbeddingModel.search``."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hip_ops as ho
import resize_aa_ref as ra
import resize_ref as rr
import test_architectures  # noqa: F401
import test_gpu_resize_batch as batch_t
import tfimm
from test_gpu_resize import MEAN, STD
from tfimm.engine import ffi, precision
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu

METHODS = ["bicubic", "bilinear"]
AA = [False, True]
AA_IDS = ["plain", "antialias"]
OUT = (16, 16)

# frames 0 and 1: odd row pitches (159 and 123 bytes at 3 channels); frame 2 is tall
FRAMES_HW = [(37, 53), (64, 41), (210, 40)]
# (frame, (y0, x0, y1, x1), (Rh, Rw, top, left)) to a 16 x 16 window; the frame indices interleaved and unsorted
CASES = [
    (0, (3, 5, 20, 31), (18, 25, 1, 4)),        # interior, odd corners
    (1, (0, 7, 30, 33), (25, 18, 4, 1)),        # touching the top edge
    (0, (15, 9, 37, 40), (18, 18, 1, 1)),       # the bottom edge
    (1, (11, 0, 50, 19), (16, 20, 0, 2)),       # the left edge
    (0, (5, 22, 29, 53), (16, 16, 0, 0)),       # the right edge
    (1, (40, 20, 64, 41), (18, 25, 1, 4)),      # the bottom right corner
    (0, (0, 0, 37, 53), (18, 25, 1, 4)),        # the whole frame
    (1, (10, 10, 11, 11), (16, 16, 0, 0)),      # 1 x 1
    (2, (5, 20, 205, 32), (16, 16, 0, 0)),      # 200 x 12 of the tall frame: 12.5 x down, T = 51 bicubic
    (0, (2, 17, 35, 18), (18, 18, 1, 1)),       # one column wide
    (1, (33, 4, 34, 39), (16, 20, 0, 2)),       # one row high
    (0, (8, 8, 28, 38), (18, 25, 1, 4)),        # two overlapping boxes
    (0, (12, 14, 34, 44), (25, 18, 4, 1)),
    (1, (20, 5, 45, 30), (18, 18, 1, 1)),       # the same box twice
    (1, (20, 5, 45, 30), (18, 18, 1, 1)),
]


@functools.lru_cache(maxsize=None)
def frames(seed, c_in, sizes=tuple(FRAMES_HW)):
    rng = np.random.default_rng(seed * 7919 + c_in)
    out = [rng.integers(0, 256, (h, w, c_in), dtype=np.uint8) for h, w in sizes]
    for f in out:
        f.setflags(write=False)
    return out


def slices_of(fr, cases):
    return [np.ascontiguousarray(fr[f][y0:y1, x0:x1]) for f, (y0, x0, y1, x1), _ in cases]


@functools.lru_cache(maxsize=None)
def reference(seed, c_in, method, aa, size=OUT, cases=tuple(CASES), sizes=tuple(FRAMES_HW)):
    """the stacked host restatement of every slice (float32, channels [0, c_in)), computed once and left unchanged"""
    mod = ra if aa else rr
    ref = np.stack([mod.resize_crop_normalise(s[None], c[2], size, method, np.float32(MEAN[:c_in]), np.float32(STD[:c_in]))[0]
                    for s, c in zip(slices_of(frames(seed, c_in, sizes), cases), cases)])
    ref.setflags(write=False)
    return ref


def padded(ref, c_out):
    return batch_t.padded(ref, c_out)


class Launch(batch_t.Launch):
    """the buffers of tests/test_gpu_resize_batch.py's launch behind the region descriptor, filled with frames and boxes"""

    def __init__(self, B, c_in, size, method, aa, c_out, **kw):
        super().__init__(B, c_in, size, method, aa, c_out, **kw)
        assert C.sizeof(ffi.ResizeRegionRec) == C.sizeof(ffi.ResizeBatchRec) + 8
        self.recs = torch.zeros(B * C.sizeof(ffi.ResizeRegionRec), dtype=torch.uint8, device=ho.DEV)
        d = ffi.ResizeRegionAADesc() if aa else ffi.ResizeRegionDesc()
        for name, _ in d._fields_:                                                   # the same fields, another record type
            setattr(d, name, getattr(self.d, name))
        d.recs = self.recs.data_ptr()
        self.d = d

    def fill(self, fr, cases):
        size, method, aa, c_in, pad = self.args
        t = ffi.resize_region_tables([f.shape[:2] for f in fr], [c[1] for c in cases], [c[0] for c in cases],
                                     [c[2] for c in cases], size, method, aa, c_in=c_in, pad=pad)
        flat = np.concatenate([f.reshape(-1) for f in fr])
        assert flat.size == t["in_bytes"] <= self.arena.numel() and t["w"].size <= self.w.numel()
        self.arena[:flat.size].copy_(torch.from_numpy(flat))
        self.recs.copy_(torch.from_numpy(t["recs"].view(np.uint8)))
        self.ta.copy_(torch.from_numpy(t["start"] if aa else t["idx"]))
        if aa:
            self.tb.copy_(torch.from_numpy(t["count"]))
        self.w[:t["w"].size].copy_(torch.from_numpy(t["w"]))
        return t

    def __call__(self):
        name = "tfimm_hip_" + ("ref_" if self.f32 else "") + "preprocess_regions" + ("_aa" if self.aa else "")
        rc = getattr(ffi.lib, name)(C.byref(self.d), ho.stream())
        ho.sync()
        return rc, self.out.float().cpu().numpy()


def run(fr, cases, size, method, aa, c_out, **kw):
    """one launch over buffers a little larger than the frames need"""
    kw.setdefault("arena_bytes", sum(f.size for f in fr) + 1)
    kw.setdefault("w_floats", len(cases) * (size[0] + size[1]) * ffi.RESIZE_AA_MAX_TAPS)
    L = Launch(len(cases), fr[0].shape[2], size, method, aa, c_out, **kw)
    L.fill(fr, cases)
    rc, out = L()
    ffi.check(rc, "preprocess_regions")
    return out


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
def test_bf16_output_equals_rounded_restatement_of_every_slice(method, aa):
    fr = frames(1, 3)
    assert {f.shape[1] * 3 for f in fr[:2]} == {159, 123}                            # odd pitches
    got = run(fr, CASES, OUT, method, aa, 4)
    want = rr.to_bf16(padded(reference(1, 3, method, aa), 4))
    for n in range(len(CASES)):
        assert np.array_equal(got[n], want[n]), f"box {n}"
    assert np.array_equal(got[13], got[14]) and not np.array_equal(got[11], got[12])


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
def test_output_equals_the_batch_launch_on_the_packed_slices(method, aa):
    fr = frames(1, 3)
    got = run(fr, CASES, OUT, method, aa, 4)
    packed = batch_t.run(slices_of(fr, CASES), [c[2] for c in CASES], OUT, method, aa, 4)
    assert np.array_equal(got, packed)
    t = ffi.resize_region_tables([f.shape[:2] for f in fr], [c[1] for c in CASES], [c[0] for c in CASES], [c[2] for c in CASES],
                                 OUT, method, aa)
    assert t["in_bytes"] == sum(f.size for f in fr)                                  # every frame once, whatever the boxes


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
def test_float32_twins_equal_the_restatement_unrounded(method, aa):
    fr, ref = frames(1, 3), reference(1, 3, method, aa)
    assert np.array_equal(run(fr, CASES, OUT, method, aa, 3, f32=True), ref)
    assert np.array_equal(run(fr, CASES, OUT, method, aa, 4, f32=True), padded(ref, 4))


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("c_in, c_out", [(1, 4), (3, 4), (4, 4), (1, 8), (3, 8), (4, 8)])
def test_channel_variants(c_in, c_out, method, aa):
    got = run(frames(2, c_in), CASES, OUT, method, aa, c_out)
    assert np.array_equal(got, rr.to_bf16(padded(reference(2, c_in, method, aa), c_out)))


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("pad", [(3, 3, 3, 3), (0, 1, 0, 1)])
def test_padded_layout_border_zeros_and_interior(pad, method, aa):
    got = run(frames(1, 3), CASES, OUT, method, aa, 4, pad=pad)
    pt, pb, pl, pr = pad
    H, W = OUT
    assert got.shape == (len(CASES), H + pt + pb, W + pl + pr, 4)
    assert np.array_equal(got[:, pt:pt + H, pl:pl + W], rr.to_bf16(padded(reference(1, 3, method, aa), 4)))
    got[:, pt:pt + H, pl:pl + W] = 0
    assert not got.any()                                                             # the kernel writes the border zeros itself


BIG_OUT = (40, 72)
BIG_CASES = (
    (2, (3, 0, 203, 40), (44, 80, 2, 4)),       # 4.5 x down and 2 x up: its wide tiles hold fewer rows than the next box's
    (0, (1, 2, 36, 51), (40, 72, 0, 0)),
    (1, (9, 3, 60, 40), (48, 76, 5, 1)),
)


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("pad", [(0, 0, 0, 0), (3, 2, 3, 2)], ids=["plain", "padded"])
def test_an_output_larger_than_a_tile(pad, method, aa):
    """40 x 72 is 3 x 3 tiles of 16 x 32, none of them whole at the far edges"""
    H, W = BIG_OUT
    got = run(frames(1, 3), BIG_CASES, BIG_OUT, method, aa, 4, pad=pad)
    ref = reference(1, 3, method, aa, BIG_OUT, BIG_CASES)
    assert np.array_equal(got[:, pad[0]:pad[0] + H, pad[2]:pad[2] + W], rr.to_bf16(padded(ref, 4)))
    got[:, pad[0]:pad[0] + H, pad[2]:pad[2] + W] = 0
    assert not got.any()


@pytest.mark.parametrize("aa, n", [(False, 4200), (True, 1100)], ids=AA_IDS)
def test_more_boxes_than_workgroups(aa, n):
    """4200 boxes of 256 pixels against at most 4096 workgroups of 256 threads; 1100 one-tile boxes against at most
    TFIMM_RESIZE_AA_MAX_BLOCKS = 1024 workgroups: the grid strides on.  All boxes lie in ONE small frame."""
    assert n > (ffi.RESIZE_AA_MAX_BLOCKS if aa else 4096)
    fr = frames(1, 3)[:1]
    kinds = [c for c in CASES if c[0] == 0]
    cases = [kinds[i % len(kinds)] for i in range(n)]
    got = run(fr, cases, OUT, "bicubic", aa, 4, w_floats=n * 32 * 16)
    ref = reference(1, 3, "bicubic", aa)
    want = rr.to_bf16(padded(np.stack([ref[CASES.index(k)] for k in kinds]), 4))
    for i in range(len(kinds)):
        assert np.array_equal(got[i::len(kinds)], np.broadcast_to(want[i], got[i::len(kinds)].shape)), f"kind {i}"


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
def test_isolation_no_pixel_outside_the_box_contributes(method, aa):
    """frames of 255 with zeros inside the boxes only: taps beyond a box's edge clamp to the box, so every output pixel is
    the one value (0 / 255 - mean) / std"""
    cases = [(0, (11, 13, 16, 20), (16, 16, 0, 0)),                                  # 5 x 7 upscaled: spans clipped on all sides
             (1, (9, 6, 50, 35), (18, 25, 1, 4)),
             (0, (20, 30, 21, 31), (16, 16, 0, 0)),                                  # 1 x 1
             (1, (0, 0, 12, 41), (18, 18, 1, 1)),                                    # along the frame's top edge, full width
             (2, (5, 20, 205, 32), (16, 16, 0, 0))]
    fr = [np.full((h, w, 3), 255, np.uint8) for h, w in FRAMES_HW]
    for f, (y0, x0, y1, x1), _ in cases:
        fr[f][y0:y1, x0:x1] = 0
    got = run(fr, cases, OUT, method, aa, 4)
    zero = (np.float32(0.0) / np.float32(255.0) - np.float32(MEAN[:3])) / np.float32(STD[:3])
    want = rr.to_bf16(padded(np.broadcast_to(zero, (len(cases), *OUT, 3)), 4))
    assert np.array_equal(got, want)
    grown = [(f, (y0, x0, y1 + 1, x1 + 1), g) for f, (y0, x0, y1, x1), g in cases[:3]]   # one row and column more: 255 shows
    assert not np.array_equal(run(fr, grown, OUT, method, aa, 4), want[:3])


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
def test_the_launch_reads_the_buffers_not_baked_arguments(method, aa):
    """the same descriptor and device buffers, refilled with other frames and other boxes: the second result"""
    L = Launch(len(CASES), 3, OUT, method, aa, 4, pad=(3, 3, 3, 3), arena_bytes=1 << 16)
    L.fill(frames(1, 3), CASES)
    rc, first = L()
    assert rc == 0 and np.array_equal(first[:, 3:19, 3:19], rr.to_bf16(padded(reference(1, 3, method, aa), 4)))
    sizes = ((64, 41), (210, 40), (37, 53))                                          # other frames in another order
    other = tuple(((f + 2) % 3, box, g) for f, box, g in CASES[::-1])
    L.fill(frames(5, 3, sizes), other)
    rc, second = L()
    assert rc == 0 and np.array_equal(second[:, 3:19, 3:19], rr.to_bf16(padded(reference(5, 3, method, aa, OUT, other, sizes), 4)))
    assert not np.array_equal(first, second)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
def test_refusals_launch_nothing(aa, f32):
    fr = frames(1, 3)

    def refused(what=None, **kw):
        L = Launch(len(CASES), 3, OUT, "bilinear", aa, kw.pop("c_out", 4), pad=kw.pop("pad", (0, 0, 0, 0)), f32=f32)
        L.fill(fr, CASES)
        for k, v in kw.items():
            setattr(L.d, k, v)
        rc, out = L()
        return rc == -1 and (out == 7.0).all() and (what is None or what in ffi.lib.tfimm_hip_last_error())

    assert refused(b"null", out=None) and refused(b"null", mean_host=None)
    assert refused(b"null", recs=None) and refused(b"null", in_=None) and refused(b"null", w=None)
    assert refused(b"null", **({"start": None} if aa else {"idx": None}))
    assert refused(B=0) and refused(H=0) and refused(W=-1) and refused(in_bytes=0) and refused(c_in=0)
    assert refused(c_in=9) and refused(b"4 stored channels", c_out=8, pad=(1, 1, 1, 1))
    if aa:
        assert refused(b"TFIMM_RESIZE_AA_MAX_TAPS", taps_cap=ffi.RESIZE_AA_MAX_TAPS + 1) and refused(taps_cap=0)
        assert refused(b"lds_bytes", lds_bytes=(64 << 10) + 4)
    else:
        assert refused(b"taps", taps=3)
    L = Launch(len(CASES), 3, OUT, "bilinear", aa, 4, f32=f32)                       # the same buffers inside the limits run
    L.fill(fr, CASES)
    if aa:
        L.d.lds_bytes = 64 << 10
    rc, out = L()
    assert rc == 0 and not (out == 7.0).any()


# ---- through create_preprocessing / Model: pre(frames, boxes=...) against pre([slices]) ---------------------------------------
MODELS = batch_t.MODELS
MODEL_IDS = batch_t.MODEL_IDS
FR_A = [(90, 120), (75, 101)]
BOX_A = np.array([[3, 5, 60, 77], [0, 0, 75, 101], [40, 60, 90, 120], [10, 11, 43, 36]])
IDX_A = np.array([0, 1, 0, 1])
FR_B = [(64, 64), (51, 140), (99, 33)]
BOX_B = np.array([[0, 0, 64, 64], [7, 7, 8, 8], [2, 100, 51, 140], [30, 1, 99, 33]])
IDX_B = np.array([0, 0, 1, 2])
FR_LARGE = [(600, 800), (480, 640)]
BOX_LARGE = np.array([[100, 100, 400, 300], [0, 0, 480, 640], [17, 333, 230, 799], [200, 200, 260, 290]])
IDX_LARGE = np.array([0, 1, 0, 1])


def _model(name, aa, **kw):
    model = tfimm.create_model(name)
    model.set_weights(synthetic_weights(model, 2021))
    return model, tfimm.create_preprocessing(name, defer=True, resize=True, antialias=aa, **kw)


def _frames(seed, sizes):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _src(key):
    return [e for e in key if isinstance(e, tuple) and e and e[0] == "src"]


def _regions_only(keys):
    return [k for k in keys if any(e[1] == "regions" for e in _src(k))]


def _check(model, pre, fr, boxes, idx, what):
    """boxes against the list of slices and against the host restatement fed as a float image"""
    x = pre(fr, boxes=boxes, box_indices=idx)
    got = model(x).numpy()
    assert got.shape[0] == len(boxes) and np.isfinite(got).all()
    assert np.array_equal(got, model(pre(x.slices())).numpy()), what + ": list of slices"
    assert np.array_equal(got, model(x.numpy()).numpy()), what + ": host restatement"
    return got


@pytest.mark.parametrize("name, aa", MODELS, ids=MODEL_IDS)
def test_model_on_boxes_one_plan_one_recording(name, aa):
    model, pre = _model(name, aa)
    tag = ("src", "regions") + (("antialias",) if aa else ())
    first = [_check(model, pre, _frames(100 + call, FR_A), BOX_A, IDX_A, f"call {call}") for call in range(3)]   # eager, recording, replay
    assert not np.array_equal(first[0], first[2])
    recorded = [c for k, c in model._captured.items() if tag in k]
    assert len(recorded) == 1
    for call in range(3):                                          # other frame sizes, other boxes: the same plan and recording
        _check(model, pre, _frames(200 + call, FR_B), BOX_B, IDX_B, f"other frames, call {call}")
    plans, caps = _regions_only(model._plans), _regions_only(model._captured)
    assert len(plans) == 1 and len(caps) == 1 and _src(plans[0]) == [tag] and _src(caps[0]) == [tag]
    assert model._captured[caps[0]] is recorded[0]                 # nothing re-recorded
    for call in range(2):                                          # much larger frames: capacities grow -- still one plan, one recording
        _check(model, pre, _frames(300 + call, FR_LARGE), BOX_LARGE, IDX_LARGE, f"large, call {call}")
    assert np.array_equal(model(pre(_frames(100, FR_A), boxes=BOX_A, box_indices=IDX_A)).numpy(), first[0])
    assert _regions_only(model._plans) == plans and _regions_only(model._captured) == caps
    plan = model._plans[plans[0]]
    st = next(iter(plan._regions.values()))
    assert isinstance(st["desc"], ffi.ResizeRegionAADesc if aa else ffi.ResizeRegionDesc) and not plan._mixed
    assert st["arena_cap"] >= sum(h * w * 3 for h, w in FR_LARGE)
    with pytest.raises(NotImplementedError, match="resize"):
        plan.export()


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
def test_model_one_frame_and_a_stack_of_frames(aa):
    model, pre = _model("vit_test_model", aa)
    fr = _frames(150, [(80, 96), (80, 96)])
    one = model(pre(fr[0], boxes=BOX_B[:2])).numpy()                                 # one frame: the indices default to zeros
    assert np.array_equal(one, model(pre([fr[0][0:64, 0:64], fr[0][7:8, 7:8]])).numpy())
    stack = model(pre(np.stack(fr), boxes=BOX_B[:2], box_indices=[1, 0])).numpy()
    assert np.array_equal(stack, model(pre([fr[1][0:64, 0:64], fr[0][7:8, 7:8]])).numpy())


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
def test_model_micro_batches_chunk_the_boxes(aa):
    model, pre = _model("vit_test_model", aa)
    fr = _frames(400, FR_B)
    boxes, idx = np.concatenate([BOX_B, [[5, 5, 40, 50]]]), np.concatenate([IDX_B, [0]])
    whole = model(pre(fr, boxes=boxes, box_indices=idx)).numpy()
    model.micro_batch = 2                                          # chunks of 2, 2 and 1 boxes
    for call in range(3):
        assert np.array_equal(_check(model, pre, fr, boxes, idx, f"call {call}"), whole)
    assert sorted(k[3] for k in _regions_only(model._plans)) == [1, 2, 5]


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
def test_model_with_branches_equals_one_branch(aa):
    model, pre = _model("resnet_test_model_1", aa)
    fr = _frames(500, FR_A)
    model.branches = 2
    got = [_check(model, pre, fr, BOX_A, IDX_A, f"call {call}") for call in range(3)]
    model.branches = 1
    assert np.array_equal(model(pre(fr, boxes=BOX_A, box_indices=IDX_A)).numpy(), got[0]) and np.array_equal(got[0], got[2])


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
def test_model_on_the_float32_path(aa):
    model, pre = _model("vit_test_model", aa)
    fr = _frames(600, FR_B)
    x = pre(fr, boxes=BOX_B, box_indices=IDX_B)
    with precision.use("fp32"):
        got = model(x)
        assert got.torch().element_size() == 4
        assert np.array_equal(got.numpy(), model(x.numpy()).numpy())
        assert np.array_equal(got.numpy(), model(pre(x.slices())).numpy())
    bf16 = _check(model, pre, fr, BOX_B, IDX_B, "bf16")
    assert not np.array_equal(bf16, got.numpy())


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
def test_top_k_evaluate_and_search_equal_the_list_path(aa):
    model, pre = _model("resnet_test_model_1", aa)
    fr = _frames(700, FR_A)
    x = pre(fr, boxes=BOX_A, box_indices=IDX_A)
    as_list = pre(x.slices())
    for a, b in zip(model.top_k(x, 3), model.top_k(as_list, 3)):
        assert a.shape == (4, 3) and np.array_equal(a.numpy(), b.numpy())
    labels = np.array([1, 0, 3, 2])
    meters = [tfimm.Meter(model.cfg.nb_classes) for _ in range(2)]
    for a, b in zip(model.evaluate(x, labels, meters[0]), model.evaluate(as_list, labels, meters[1])):
        assert a.shape == (4,) and np.array_equal(a.numpy(), b.numpy())
    assert np.array_equal(meters[0].state().words, meters[1].state().words)
    with pytest.raises(ValueError):
        model.evaluate(x, np.array([1, 0]))                                          # two labels for four boxes, one per frame
    emb = tfimm.EmbeddingModel(tfimm.create_model("vit_test_model"), 32, normalize=True)
    emb.set_weights(synthetic_weights(emb, 2021))
    pre = tfimm.create_preprocessing("vit_test_model", defer=True, resize=True, antialias=aa)
    x = pre(fr, boxes=BOX_A, box_indices=IDX_A)
    as_list = pre(x.slices())
    gallery = tfimm.Gallery(32)
    gallery.add(emb(pre(_frames(701, [(40, 40)] * 6))))
    a, b = emb.search(x, gallery, 3), emb.search(as_list, gallery, 3)
    assert a.indices.shape == (4, 3)
    assert np.array_equal(a.indices.numpy(), b.indices.numpy()) and np.array_equal(a.scores.numpy(), b.scores.numpy())
    assert np.array_equal(model.forward_features(x).numpy(), model.forward_features(as_list).numpy())


def test_fit_head_takes_the_boxes_as_the_batch():
    model, pre = _model("resnet_test_model_1", False)
    fr = _frames(750, FR_A)
    x = pre(fr, boxes=BOX_A, box_indices=IDX_A)
    labels = np.array([1, 0, 3, 2])
    results = []
    for inp in (x, pre(x.slices())):
        feat = model._head_input(inp)
        probe = tfimm.LinearProbe(feat.shape[1], model.cfg.nb_classes)
        results.append(model.fit_head(inp, labels, probe))
    for a, b in zip(*results):
        assert a.shape == (4,) and np.array_equal(a.numpy(), b.numpy())


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
def test_crop_pct_reaches_the_device_in_the_uniform_and_the_region_form(aa):
    """two values of crop_pct on one model: each equals its own host restatement, so they never share tables"""
    model, pre = _model("vit_test_model", aa)
    _, full = _model("vit_test_model", aa, crop_pct=1.0)
    u8 = np.stack(_frames(800, [(48, 56), (48, 56)]))
    for call in range(2):                                                            # eager, then recorded
        a, b = model(pre(u8)).numpy(), model(full(u8)).numpy()
        assert np.array_equal(a, model(pre(u8).numpy()).numpy()) and np.array_equal(b, model(full(u8).numpy()).numpy())
        assert not np.array_equal(a, b)
    fr = _frames(801, FR_A)
    x = full(fr, boxes=BOX_A, box_indices=IDX_A)
    assert x.resize[1] == 1.0
    got = model(x).numpy()
    assert np.array_equal(got, model(full(x.slices())).numpy()) and np.array_equal(got, model(x.numpy()).numpy())
    assert not np.array_equal(got, model(pre(fr, boxes=BOX_A, box_indices=IDX_A)).numpy())


def test_a_box_outside_the_antialias_domain_raises_before_any_launch():
    model, pre = _model("vit_test_model", True)
    fr = _frames(900, FR_A) + [np.zeros((700, 700, 3), np.uint8)]
    boxes = np.array([[0, 0, 50, 50], [3, 3, 70, 90], [10, 20, 610, 660], [0, 0, 40, 40]])   # 600 -> 36: 16.7 x down, 69 taps
    with pytest.raises(ValueError, match=r"box 2 .*TFIMM_RESIZE_AA_MAX_TAPS"):
        model(pre(fr, boxes=boxes, box_indices=[0, 1, 2, 2]))
    assert not model._captured and not any(p._regions for p in model._plans.values())
    model.micro_batch = 2                                                            # the box keeps its number in a later chunk
    with pytest.raises(ValueError, match=r"box 2 .*TFIMM_RESIZE_AA_MAX_TAPS"):
        model(pre(fr, boxes=boxes, box_indices=[0, 1, 2, 2]))
    assert not model._captured and not any(p._regions for p in model._plans.values())

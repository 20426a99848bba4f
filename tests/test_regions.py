"""Boxes of frames, the host side (no GPU): records and table arenas of ``ffi.resize_region_tables`` held, box by box, to
``ffi.resize_batch_tables`` on the slices -- every field but the two that address the frame, and those against their
formula; ``pre(frames, boxes=..., box_indices=...)`` against ``pre([slices])`` bit for bit, its refusals, ``crop_pct``, and the
layout of the new structures against the header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import test_architectures  # noqa: F401  (registers the miniature configs)
import tfimm
from tfimm.engine import ffi
from tfimm.models import DeferredInput
from tfimm.models.factory import resize_geometry

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfimm_hip.h")
METHODS = ["bicubic", "bilinear"]
AA = [False, True]
AA_IDS = ["plain", "antialias"]
OUT = (16, 16)
FRAMES_HW = [(37, 53), (64, 41)]
# (y0, x0, y1, x1): interior with odd corners, a whole frame, 1 x 1, touching two edges, one column wide -- five boxes in two
# frames, the frame indices interleaved
BOXES = np.array([[3, 5, 20, 31], [0, 0, 64, 41], [10, 10, 11, 11], [1, 0, 37, 53], [7, 3, 40, 4]])
INDEX = np.array([0, 1, 1, 0, 1])


def _frames(seed, sizes=FRAMES_HW, c=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for h, w in sizes]


def _slices(frames, boxes, index):
    return [frames[f][y0:y1, x0:x1] for (y0, x0, y1, x1), f in zip(np.asarray(boxes).tolist(), index)]


def _box_hw(boxes):
    return [(int(b[2] - b[0]), int(b[3] - b[1])) for b in boxes]


# ---- the tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [(0, 0, 0, 0), (3, 3, 3, 3)])
@pytest.mark.parametrize("c_in", [3, 1])
@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
@pytest.mark.parametrize("method", METHODS)
def test_records_and_tables_are_those_of_the_slices(method, aa, c_in, pad):
    hw = _box_hw(BOXES)
    geos = [resize_geometry(s, OUT, 0.875) for s in hw]
    t = ffi.resize_region_tables(FRAMES_HW, BOXES, INDEX, geos, OUT, method, aa, c_in=c_in, pad=pad)
    s = ffi.resize_batch_tables(hw, geos, OUT, method, aa, c_in=c_in, pad=pad)
    for name in ("start", "count") if aa else ("idx",):
        assert np.array_equal(t[name], s[name]), name
    assert np.array_equal(t["w"].view(np.uint32), s["w"].view(np.uint32))
    assert (t["max_taps"], t["lds_floats"], t["n_tiles"]) == (s["max_taps"], s["lds_floats"], s["n_tiles"])
    shared = [n for n, _ in ffi.RESIZE_BATCH_REC if n != "in_offset"]
    assert [n for n, _ in ffi.RESIZE_REGION_REC] == ["in_offset", "row_pitch"] + shared
    for name in shared:
        assert np.array_equal(t["recs"][name], s["recs"][name]), name
    # every frame once, back to back in list order, however many boxes name it
    frame_off = np.concatenate([[0], np.cumsum([h * w * c_in for h, w in FRAMES_HW])])
    assert t["in_bytes"] == frame_off[-1] == sum(h * w * c_in for h, w in FRAMES_HW)
    for n, ((y0, x0, y1, x1), f) in enumerate(zip(BOXES.tolist(), INDEX)):
        Wf = FRAMES_HW[f][1]
        assert t["recs"]["in_offset"][n] == frame_off[f] + (y0 * Wf + x0) * c_in, f"box {n}"
        assert t["recs"]["row_pitch"][n] == Wf * c_in, f"box {n}"
        assert (t["recs"]["Hs"][n], t["recs"]["Ws"][n]) == (y1 - y0, x1 - x0)
    if c_in == 3:
        assert set(t["recs"]["row_pitch"].tolist()) == {159, 123}                     # odd pitches


@pytest.mark.parametrize("aa", AA, ids=AA_IDS)
def test_the_sizing_call_reports_sizes_and_writes_nothing_else(aa):
    hw = _box_hw(BOXES)
    geo = np.ascontiguousarray([resize_geometry(s, OUT, 0.875) for s in hw], np.int32)
    fhw = np.ascontiguousarray(FRAMES_HW, np.int32)
    bx, idx = ffi.check_boxes(FRAMES_HW, BOXES, INDEX)
    i32p = ctypes.POINTER(ctypes.c_int32)
    need = ffi.ResizeBatchSizes()
    rc = ffi.lib.tfimm_hip_resize_region_tables(2, fhw.ctypes.data_as(i32p), 5, bx.ctypes.data_as(i32p), idx.ctypes.data_as(i32p),
                                                geo.ctypes.data_as(i32p), 16, 16, 3, None, 1, int(aa), ctypes.byref(need), None,
                                                None, None, None)
    assert rc == 0
    full = ffi.resize_region_tables(FRAMES_HW, BOXES, INDEX, geo, OUT, "bicubic", aa)
    assert need.in_bytes == full["in_bytes"] == 37 * 53 * 3 + 64 * 41 * 3 and need.bad_image == -1
    assert need.tab_elems == (full["start"] if aa else full["idx"]).size and need.w_floats == full["w"].size
    assert (need.max_taps, need.lds_floats, need.n_tiles) == (full["max_taps"], full["lds_floats"], full["n_tiles"])


def _c_call(frames_hw, boxes, index, method=1, aa=0, recs=None):
    """the C function itself, without the wrapper's own checks: (rc, sizes, last error)"""
    fhw = np.ascontiguousarray(frames_hw, np.int32)
    bx = np.ascontiguousarray(boxes, np.int32)
    idx = np.ascontiguousarray(index, np.int32)
    geo = np.ascontiguousarray([resize_geometry((max(int(b[2] - b[0]), 1), max(int(b[3] - b[1]), 1)), OUT, 0.875) for b in bx], np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    need = ffi.ResizeBatchSizes()
    need.in_bytes, need.bad_image = -5, -7                                           # untouched by a refusal
    rc = ffi.lib.tfimm_hip_resize_region_tables(len(fhw), fhw.ctypes.data_as(i32p), len(bx), bx.ctypes.data_as(i32p),
                                                idx.ctypes.data_as(i32p), geo.ctypes.data_as(i32p), 16, 16, 3, None, method, aa,
                                                ctypes.byref(need), recs, None, None, None)
    return rc, need, ffi.lib.tfimm_hip_last_error().decode()


@pytest.mark.parametrize("boxes, index, what", [
    ([[0, 0, 10, 10], [5, 5, 38, 20]], [0, 0], r"box 1 .*outside"),                  # one row past the 37-row frame
    ([[0, 0, 10, 10], [0, 40, 10, 54]], [1, 0], r"box 1 .*outside"),
    ([[0, 0, 10, 42]], [1], r"box 0 .*outside"),                                     # fits frame 0, not frame 1
    ([[-1, 0, 10, 10]], [0], r"box 0 .*outside"),
    ([[0, 0, 10, 10], [4, 4, 4, 9]], [0, 1], r"box 1 .*empty"),
    ([[0, 0, 10, 10], [9, 9, 4, 12]], [0, 1], r"box 1 .*empty"),
    ([[0, 0, 10, 10], [0, 0, 10, 10]], [0, 2], r"box 1 .*frame 2"),
    ([[0, 0, 10, 10]], [-1], r"box 0 .*frame -1"),
])
def test_refusals_name_the_box_and_write_nothing(boxes, index, what):
    rc, need, err = _c_call(FRAMES_HW, boxes, index)
    assert rc == -1 and re.search(what, err), err
    assert (need.in_bytes, need.bad_image) == (-5, -7)
    with pytest.raises(ValueError, match=what):
        ffi.resize_region_tables(FRAMES_HW, boxes, index, [(16, 16, 0, 0)] * len(boxes), OUT, "bicubic")


def test_a_box_beyond_the_tap_limit_is_reported_in_bad_image():
    frames_hw = [(48, 56), (700, 700)]
    boxes, index = [[0, 0, 48, 56], [0, 0, 40, 40], [50, 30, 650, 670], [0, 0, 700, 700]], [0, 1, 1, 1]      # 600 -> 18: 133 taps
    rc, need, err = _c_call(frames_hw, boxes, index, aa=1)
    assert rc == -1 and need.bad_image == 2 and re.search(r"box 2 .*TFIMM_RESIZE_AA_MAX_TAPS", err)
    assert need.in_bytes == 48 * 56 * 3 + 700 * 700 * 3
    geos = [resize_geometry(s, OUT, 0.875) for s in _box_hw(np.asarray(boxes))]
    with pytest.raises(ValueError, match=r"box 2 .*TFIMM_RESIZE_AA_MAX_TAPS"):
        ffi.resize_region_tables(frames_hw, boxes, index, geos, OUT, "bicubic", True)
    ffi.resize_region_tables(frames_hw, boxes, index, geos, OUT, "bicubic", False)   # the plain launch has no such limit
    assert _c_call(frames_hw, boxes, index, aa=0)[0] == 0


# ---- create_preprocessing with boxes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("antialias", AA, ids=AA_IDS)
@pytest.mark.parametrize("name", ["resnet_test_model_1", "vit_test_model"])          # bilinear, bicubic
def test_numpy_of_boxes_is_numpy_of_the_list_of_slices(name, antialias):
    pre = tfimm.create_preprocessing(name, defer=True, resize=True, antialias=antialias)
    frames = _frames(11)
    x = pre(frames, boxes=BOXES, box_indices=INDEX)
    assert isinstance(x, DeferredInput) and x.regions and not x.mixed
    assert x.shape == (5, None, None, 3)
    assert x.resize == pre(frames).resize and not pre(frames).regions and not pre(frames[0]).regions
    want = pre(_slices(frames, BOXES, INDEX)).numpy()
    got = x.numpy()
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(np.asarray(x), want)
    # lists of lists, torch frames
    assert np.array_equal(pre([torch.from_numpy(f) for f in frames], boxes=BOXES.tolist(), box_indices=INDEX.tolist()).numpy(), want)


def test_the_forms_of_frames_and_the_default_of_box_indices():
    pre = tfimm.create_preprocessing("vit_test_model", defer=True, resize=True)
    stack = np.stack(_frames(12, [(40, 50), (40, 50)]))
    boxes = np.array([[0, 0, 40, 50], [3, 4, 30, 17], [39, 49, 40, 50]])
    one = pre(stack[0], boxes=boxes)                                                 # one frame: the indices default to zeros
    assert one.shape == (3, None, None, 3) and one.box_indices.tolist() == [0, 0, 0]
    assert np.array_equal(one.numpy(), pre(_slices([stack[0]], boxes, [0, 0, 0])).numpy())
    assert np.array_equal(pre([stack[0]], boxes=boxes).numpy(), one.numpy())
    both = pre(stack, boxes=boxes, box_indices=[1, 0, 1])                            # an (F, Hf, Wf, C) array
    assert np.array_equal(both.numpy(), pre(_slices(list(stack), boxes, [1, 0, 1])).numpy())
    with pytest.raises(ValueError, match="box_indices is required"):
        pre(stack, boxes=boxes)
    with pytest.raises(ValueError, match="box_indices is required"):
        pre(list(stack), boxes=boxes)


def test_box_refusals():
    pre = tfimm.create_preprocessing("vit_test_model", defer=True, resize=True)
    frames = _frames(13)
    ok = [[0, 0, 10, 10]]
    with pytest.raises(ValueError, match="resize=True"):
        tfimm.create_preprocessing("vit_test_model", defer=True)(frames[0], boxes=ok)
    with pytest.raises(ValueError, match="resize=True"):
        tfimm.create_preprocessing("vit_test_model")(frames[0], boxes=ok)
    with pytest.raises(ValueError, match="integer"):
        pre(frames[0], boxes=[[0.0, 0.0, 10.0, 10.0]])                                # float boxes: the caller rounds
    with pytest.raises(ValueError, match="integer"):
        pre(frames[0], boxes=np.array(ok, np.float32))
    with pytest.raises(ValueError, match=r"\(N, 4\)"):
        pre(frames[0], boxes=np.zeros((0, 4), np.int64))                              # N == 0
    with pytest.raises(ValueError, match=r"\(N, 4\)"):
        pre(frames[0], boxes=[0, 0, 10, 10])
    with pytest.raises(ValueError, match=r"box 1 .*empty"):
        pre(frames[0], boxes=ok + [[5, 5, 5, 9]])
    with pytest.raises(ValueError, match=r"box 1 .*outside"):
        pre(frames[0], boxes=ok + [[0, 0, 38, 10]])
    with pytest.raises(ValueError, match=r"box 0 .*outside"):
        pre(frames, boxes=[[0, 0, 10, 42]], box_indices=[1])
    with pytest.raises(ValueError, match=r"box 1 .*frame 2"):
        pre(frames, boxes=ok * 2, box_indices=[0, 2])
    with pytest.raises(ValueError, match=r"box 0 .*frame -1"):
        pre(frames, boxes=ok, box_indices=[-1])
    with pytest.raises(ValueError, match="box_indices"):
        pre(frames, boxes=ok * 2, box_indices=[0])                                    # one index for two boxes
    with pytest.raises(ValueError, match="box_indices"):
        pre(frames, boxes=ok, box_indices=[0.0])
    with pytest.raises(ValueError, match="uint8"):
        pre(frames[0].astype(np.float32), boxes=ok)
    with pytest.raises(ValueError, match="uint8"):
        pre([frames[0], frames[1].astype(np.int32)], boxes=ok, box_indices=[0])
    with pytest.raises(ValueError, match="frame 0"):
        pre(frames[0][..., :2], boxes=ok)                                             # wrong channel count
    with pytest.raises(ValueError, match="frame 1"):
        pre([frames[0], frames[1][..., :1]], boxes=ok, box_indices=[0])
    with pytest.raises(ValueError, match="box_indices without boxes"):
        pre(frames, box_indices=[0])
    with pytest.raises(ValueError):
        pre([], boxes=ok, box_indices=[0])


# ---- crop_pct -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("antialias", AA, ids=AA_IDS)
def test_crop_pct_replaces_the_configs_value_in_every_form(antialias):
    name = "vit_test_model"
    cfg = tfimm.models.model_config(name)
    assert float(cfg.crop_pct) != 1.0
    size = tuple(cfg.input_size)
    pre = tfimm.create_preprocessing(name, defer=True, resize=True, antialias=antialias, crop_pct=1.0)
    default = tfimm.create_preprocessing(name, defer=True, resize=True, antialias=antialias)
    tail = (True,) if antialias else ()
    frames = _frames(14)
    forms = [lambda p: p(frames[0]), lambda p: p(frames[0][None]), lambda p: p(frames),
             lambda p: p(frames, boxes=BOXES, box_indices=INDEX)]
    for form in forms:
        assert form(pre).resize == (cfg.interpolation, 1.0, size) + tail
        assert form(default).resize == (cfg.interpolation, float(cfg.crop_pct), size) + tail
    # the geometry is resize_geometry's for that value: the whole 37 x 53 frame's shorter side becomes the input size
    assert resize_geometry((37, 53), size, 1.0)[:2] == (size[0], int(size[0] * 53 / 37))
    assert resize_geometry((37, 53), size, 1.0) != resize_geometry((37, 53), size, float(cfg.crop_pct))
    from tfimm.models.model import _resize_crop_host
    want = _resize_crop_host(frames[0][None].astype(np.float32), cfg.interpolation, 1.0, size, antialias)
    want = (want / np.float32(255.0) - np.asarray(pre(frames[0]).mean, np.float32)) / np.asarray(pre(frames[0]).std, np.float32)
    assert np.array_equal(pre(frames[0][None]).numpy(), want)
    assert not np.array_equal(pre(frames[0][None]).numpy(), default(frames[0][None]).numpy())
    # a box at crop_pct = 1 is its slice at crop_pct = 1
    x = pre(frames, boxes=BOXES, box_indices=INDEX)
    assert np.array_equal(x.numpy(), pre(_slices(frames, BOXES, INDEX)).numpy())


def test_crop_pct_none_is_todays_behaviour_and_bad_values_are_refused():
    name = "resnet_test_model_1"
    cfg = tfimm.models.model_config(name)
    frames = _frames(15)
    for kw in (dict(defer=True, resize=True), dict(defer=True, resize=True, antialias=True), dict(defer=True), dict()):
        a, b = tfimm.create_preprocessing(name, **kw), tfimm.create_preprocessing(name, crop_pct=None, **kw)
        xa, xb = a(frames[0]), b(frames[0])
        if isinstance(xa, DeferredInput):
            assert (xa.resize, xa.mean, xa.std) == (xb.resize, xb.mean, xb.std) and xa.data is xb.data
            assert xa.boxes is None and xa.box_indices is None and not xa.regions
            if kw.get("resize"):
                assert xa.resize[:3] == (cfg.interpolation, float(cfg.crop_pct), tuple(cfg.input_size))
                assert a(frames).resize == b(frames).resize and a(frames).mixed
        else:
            assert np.array_equal(xa, xb)
    for bad in (0.0, -0.5, 1.5, True):
        with pytest.raises(ValueError, match="crop_pct"):
            tfimm.create_preprocessing(name, defer=True, resize=True, crop_pct=bad)
    with pytest.raises(ValueError, match="resize=True"):
        tfimm.create_preprocessing(name, defer=True, crop_pct=1.0)


# ---- the structures against the header ----------------------------------------------------------------------------------
def _struct_fields(hdr, name):
    body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        toks = [t for t in decl.replace("*", " * ").split() if t != "const"]
        if not toks:
            continue
        ctype = "pointer" if "*" in toks else toks[0]
        fields += [(n.strip(), ctype) for n in " ".join(t for t in toks[1:] if t != "*" and not t.startswith("tfimm_")).split(",")]
    return fields


@pytest.mark.parametrize("name, mirror, twin", [
    ("tfimm_resize_region_rec", ffi.ResizeRegionRec, None),
    ("tfimm_resize_region_desc", ffi.ResizeRegionDesc, ffi.ResizeBatchDesc),
    ("tfimm_resize_region_aa_desc", ffi.ResizeRegionAADesc, ffi.ResizeBatchAADesc),
])
def test_struct_layouts_match_the_header(name, mirror, twin):
    fields = _struct_fields(open(HEADER).read(), name)
    assert [n.rstrip("_") for n, _ in mirror._fields_] == [n for n, _ in fields], fields
    # natural alignment, as the C compiler lays the struct out
    width = {"pointer": 8, "int64_t": 8, "int32_t": 4}
    off = 0
    for (fname, _), (_, ctype) in zip(mirror._fields_, fields):
        w = width[ctype]
        off = -(-off // w) * w
        assert getattr(mirror, fname).offset == off and getattr(mirror, fname).size == w, fname
        off += w
    assert ctypes.sizeof(mirror) == -(-off // 8) * 8
    if twin is not None:                                                              # the batch descriptor with another record
        assert ctypes.sizeof(mirror) == ctypes.sizeof(twin)
        assert [(n, getattr(mirror, n).offset) for n, _ in mirror._fields_] == [(n, getattr(twin, n).offset) for n, _ in twin._fields_]
    else:
        assert ctypes.sizeof(mirror) == 64 == np.dtype(ffi.RESIZE_REGION_REC).itemsize
        assert (mirror.in_offset.offset, mirror.row_pitch.offset, mirror.Hs.offset, mirror.n_tiles.offset) == (0, 8, 16, 60)
        assert [n for n, _ in mirror._fields_] == [n for n, _ in ffi.RESIZE_REGION_REC]


def test_the_five_new_symbols_are_exported():
    lib = ctypes.CDLL(ffi.LIB_PATH)
    for n in ("tfimm_hip_resize_region_tables", "tfimm_hip_preprocess_regions", "tfimm_hip_preprocess_regions_aa",
              "tfimm_hip_ref_preprocess_regions", "tfimm_hip_ref_preprocess_regions_aa"):
        assert hasattr(lib, n) and n in ffi.SYMBOLS

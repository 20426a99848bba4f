"""Mixed-size image batches, the host side (no GPU): records and table arenas of ``ffi.resize_batch_tables`` held, image by
image, to ``ffi.resize_taps`` / ``ffi.resize_spans`` of that image alone; ``create_preprocessing(defer=True, resize=True)`` on
a LIST of images of different sizes -- its ``numpy()`` against the per-image results, bit for bit -- the refusals, and array
input left as it was."""
import numpy as np
import pytest
import torch

import test_architectures  # noqa: F401  (registers the miniature configs)
import tfimm
from tfimm.engine import ffi
from tfimm.models import DeferredInput
from tfimm.models.factory import resize_geometry

METHODS = ["bicubic", "bilinear"]
# (Hs, Ws), (Rh, Rw, top, left) to a 16 x 16 window: the cases of tests/test_gpu_resize_aa.py, an upscale and an identity
SIZES = [(37, 53), (53, 37), (120, 97), (40, 10), (5, 7), (16, 16)]
GEOS = [(18, 25, 1, 4), (25, 18, 4, 1), (18, 18, 1, 1), (16, 20, 0, 2), (16, 16, 0, 0), (16, 16, 0, 0)]
OUT = (16, 16)


@pytest.mark.parametrize("c_in", [3, 1])
@pytest.mark.parametrize("method", METHODS)
def test_plain_records_and_tables_are_the_per_image_tables(method, c_in):
    taps = 4 if method == "bicubic" else 2
    t = ffi.resize_batch_tables(SIZES, GEOS, OUT, method, False, c_in=c_in)
    recs, H, W = t["recs"], *OUT
    assert t["idx"].shape == t["w"].shape == (len(SIZES) * (H + W) * taps,)          # the fixed size B * (H + W) * taps
    assert t["in_bytes"] == sum(h * w * c_in for h, w in SIZES) and t["max_taps"] == taps and t["n_tiles"] == 0
    off = 0
    for b, ((Hs, Ws), (Rh, Rw, top, left)) in enumerate(zip(SIZES, GEOS)):
        r = recs[b]
        assert (r["in_offset"], r["Hs"], r["Ws"]) == (off, Hs, Ws)
        off += Hs * Ws * c_in
        assert (r["y_tab"], r["x_tab"]) == (b * (H + W) * taps, (b * (H + W) + H) * taps)
        assert (r["y_w"], r["x_w"], r["y_taps"], r["x_taps"]) == (r["y_tab"], r["x_tab"], taps, taps)
        for tab, n_in, n_res, first, n_out in ((r["y_tab"], Hs, Rh, top, H), (r["x_tab"], Ws, Rw, left, W)):
            idx, w = ffi.resize_taps(n_in, n_res, first, n_out, method)
            assert np.array_equal(t["idx"][tab:tab + n_out * taps], idx.reshape(-1))
            assert np.array_equal(t["w"][tab:tab + n_out * taps].view(np.uint32), w.reshape(-1).view(np.uint32))
    assert recs["in_offset"][1] % 2 == 1                                             # 37 * 53 * c_in bytes: an odd address
    # the identity image: (0, 1, 0, 0) / fraction 0 at the pixel itself
    r = recs[5]
    w = t["w"][r["y_tab"]:r["y_tab"] + H * taps].reshape(H, taps)
    assert w[:, taps // 2].tolist() == [0.0] * H and w[:, taps // 2 - 1].tolist() == [1.0] * H
    assert t["idx"][r["y_tab"]:r["y_tab"] + H * taps].reshape(H, taps)[:, taps // 2 - 1].tolist() == list(range(H))


@pytest.mark.parametrize("pad", [(0, 0, 0, 0), (3, 3, 3, 3)])
@pytest.mark.parametrize("method", METHODS)
def test_antialiased_records_and_tables_are_the_per_image_spans(method, pad):
    t = ffi.resize_batch_tables(SIZES, GEOS, OUT, method, True, c_in=3, pad=pad)
    recs, H, W = t["recs"], *OUT
    HP, WP = H + pad[0] + pad[1], W + pad[2] + pad[3]
    assert t["start"].shape == t["count"].shape == (len(SIZES) * (H + W),)
    w_off = tile0 = 0
    pitches = []
    for b, ((Hs, Ws), (Rh, Rw, top, left)) in enumerate(zip(SIZES, GEOS)):
        r = recs[b]
        assert (r["y_tab"], r["x_tab"]) == (b * (H + W), b * (H + W) + H)
        for tab, wo, T, n_in, n_res, first, n_out in ((r["y_tab"], r["y_w"], r["y_taps"], Hs, Rh, top, H),
                                                      (r["x_tab"], r["x_w"], r["x_taps"], Ws, Rw, left, W)):
            start, count, w = ffi.resize_spans(n_in, n_res, first, n_out, method)
            assert T == w.shape[1] == ffi.resize_span_taps(n_in, n_res, method) and wo == w_off
            assert np.array_equal(t["start"][tab:tab + n_out], start) and np.array_equal(t["count"][tab:tab + n_out], count)
            assert np.array_equal(t["w"][wo:wo + n_out * T].view(np.uint32), w.reshape(-1).view(np.uint32))
            w_off += n_out * T
            pitches.append(T)
        # the tile bookkeeping: the rule of the uniform launch -- as many rows as the LDS budget holds, 16 at most
        assert 1 <= r["tile_rows"] <= min(ffi.RESIZE_AA_TILE_ROWS, HP) and 1 <= r["cols_max"] <= Ws
        assert r["tile_rows"] * r["cols_max"] * 3 <= min(16384, t["lds_floats"])
        n = -(-HP // r["tile_rows"]) * -(-WP // ffi.RESIZE_AA_TILE_COLS)
        assert (r["tile0"], r["n_tiles"]) == (tile0, n)
        tile0 += n
    assert t["w"].shape == (w_off,) and t["n_tiles"] == tile0 and t["max_taps"] == max(pitches)    # the sizes are exact
    assert len({(int(r["y_taps"]), int(r["x_taps"])) for r in recs}) >= 4                # several pitch pairs in one batch
    if method == "bicubic":                                                          # identity: (0, 0, 1, 0, 0), clipped at the ends
        r = recs[5]
        w = t["w"][r["y_w"]:r["y_w"] + H * 5].reshape(H, 5)
        assert (r["y_taps"], w[5].tolist()) == (5, [0.0, 0.0, 1.0, 0.0, 0.0])


def test_an_image_beyond_the_tap_limit_is_named_by_index():
    sizes, geos = [(48, 56), (600, 640), (700, 700)], [resize_geometry(s, (32, 32), 0.875) for s in [(48, 56), (600, 640), (700, 700)]]
    with pytest.raises(ValueError, match=r"image 1 .*TFIMM_RESIZE_AA_MAX_TAPS"):
        ffi.resize_batch_tables(sizes, geos, (32, 32), "bicubic", True)             # 600 -> 36: 69 taps
    ffi.resize_batch_tables(sizes, geos, (32, 32), "bilinear", True)                 # 35 and 41 taps: inside the domain
    ffi.resize_batch_tables(sizes, geos, (32, 32), "bicubic", False)                 # the plain launch has no such limit
    with pytest.raises(ValueError):
        ffi.resize_batch_tables([], [], (32, 32), "bicubic", True)


# ---- create_preprocessing on a list ---------------------------------------------------------------------------------
def _images(seed, sizes, c=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, c), dtype=np.uint8) for h, w in sizes]


@pytest.mark.parametrize("antialias", [False, True], ids=["plain", "antialias"])
@pytest.mark.parametrize("name", ["resnet_test_model_1", "vit_test_model"])          # bilinear, bicubic
def test_numpy_of_a_list_is_the_stack_of_the_per_image_results(name, antialias):
    pre = tfimm.create_preprocessing(name, defer=True, resize=True, antialias=antialias)
    imgs = _images(7, [(48, 56), (81, 35), (32, 32), (20, 90)])
    x = pre(imgs)
    assert isinstance(x, DeferredInput) and x.mixed and x.data is not imgs and all(a is b for a, b in zip(x.data, imgs))
    assert x.shape == (4, None, None, 3)
    assert x.resize[0] == tfimm.models.model_config(name).interpolation and (len(x.resize) == 4) == antialias
    got = x.numpy()
    want = np.stack([pre(im[None]).numpy()[0] for im in imgs])
    assert got.dtype == np.float32 and got.shape == (4,) + tuple(x.resize[2]) + (3,)
    assert np.array_equal(got, want)
    assert np.array_equal(np.asarray(x), want)
    # tuples and torch tensors are lists too
    assert np.array_equal(pre(tuple(torch.from_numpy(im) for im in imgs)).numpy(), want)


def test_list_refusals():
    pre = tfimm.create_preprocessing("vit_test_model", defer=True, resize=True)
    imgs = _images(8, [(48, 56), (81, 35)])
    with pytest.raises(ValueError, match="resize=True"):
        tfimm.create_preprocessing("vit_test_model", defer=True)(imgs)               # a list without resize=True
    with pytest.raises(ValueError, match="resize=True"):
        tfimm.create_preprocessing("vit_test_model")(imgs)
    with pytest.raises(ValueError, match="empty"):
        pre([])
    with pytest.raises(ValueError, match="uint8"):
        pre([imgs[0], imgs[1].astype(np.float32)])
    with pytest.raises(ValueError, match="uint8"):
        pre([torch.from_numpy(imgs[0]).float()])
    with pytest.raises(ValueError, match="image 1"):
        pre([imgs[0], imgs[1][None]])                                                # not 3-D
    with pytest.raises(ValueError, match="image 0"):
        pre([imgs[0][..., :2]])                                                      # wrong channel count
    with pytest.raises(ValueError, match="image 0"):
        pre([imgs[0][..., 0]])


@pytest.mark.parametrize("antialias", [False, True], ids=["plain", "antialias"])
def test_array_input_returns_what_it_returned(antialias):
    pre = tfimm.create_preprocessing("vit_test_model", defer=True, resize=True, antialias=antialias)
    u8 = np.random.default_rng(9).integers(0, 256, (2, 48, 56, 3), dtype=np.uint8)
    x = pre(u8)
    assert isinstance(x, DeferredInput) and not x.mixed and x.data is u8 and x.shape == (2, 48, 56, 3)
    cfg = tfimm.models.model_config("vit_test_model")
    assert x.resize == (cfg.interpolation, float(cfg.crop_pct), tuple(cfg.input_size)) + ((True,) if antialias else ())
    one = pre(u8[0])
    assert one.shape == (48, 56, 3) and np.array_equal(one.numpy(), x.numpy()[0])
    with pytest.raises(ValueError, match="uint8"):
        pre(u8.astype(np.float32))
    # without the flags a nested list of numbers is still an array-like
    plain = tfimm.create_preprocessing("vit_test_model")
    assert np.array_equal(plain(u8[0].tolist()), plain(u8[0]))

"""tfimm_hip_attention's descriptor contract, on the CPU: which kernel instantiation every attention case of hip_checks.py
launches (the library's route export: the entry point's own validate + route steps, no device), that the cases together reach
every instantiation the dispatcher has, what the environment switches do to the routes, and every refusal."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hip_checks as hc
import hip_ops as H
from tfimm.engine import ffi, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUP = -1, -2

# every name attn_route (csrc/attention.hip) can return: one per kernel instantiation the library compiles
ROUTES = ([f"generic<{hd},{k}>" for hd in (32, 64) for k in ("global", "swin")] + ["generic<96,global>", "generic<128,global>"]
          + [f"resident<{hd},{k},{t}>" for hd in (32, 64) for k in ("global", "swin") for t in ("4x1", "8x1", "8x2")]
          + ["stream<64>", "window_persist<32,hpw1>", "window_persist<32,hpw2>", "window_v1<32>"])
# names no descriptor reaches in the default environment, each with its reason
UNREACHABLE_BY_DEFAULT = {
    "window_v1<32>": "the one-window-per-workgroup kernel runs only under TFIMM_ATTN_WIN_V1 (an A/B switch); its shapes are "
                     "window_persist's, and the WIN_V1 environment below puts every window_persist row on it",
}


def test_every_case_reaches_its_route_and_every_route_is_reached():
    assert len(set(ROUTES)) == len(ROUTES) == 22
    reached = {}
    for name, row in hc.ATTN_ROWS.items():
        assert name in hc.CASES
        reached[name] = hc.attn_row_route(name)
    wrong = {n: (hc.ATTN_ROWS[n]["route"], r) for n, r in reached.items() if r != hc.ATTN_ROWS[n]["route"]}
    assert not wrong, f"(declared, reached): {wrong}"
    assert set(reached.values()) == set(ROUTES) - set(UNREACHABLE_BY_DEFAULT)
    # every route has a loose case and a tight one
    for route in set(ROUTES) - set(UNREACHABLE_BY_DEFAULT):
        hits = [n for n, r in reached.items() if r == route]
        assert any(n.startswith("tight_") for n in hits) and any(not n.startswith("tight_") for n in hits), (route, hits)


def test_every_attention_case_is_a_row():
    """a tfimm_hip_attention case registered past the table would run on a kernel nobody declared"""
    other = ("attn_probs_", "swin_b_")        # tfimm_hip_attention_probs; Swin-B's MLP and qkv GEMM layers
    rest = [n for n in hc.CASES if n.replace("tight_", "").startswith(("attn_", "swin_"))
            and not n.replace("tight_", "").startswith(other) and n not in hc.ATTN_ROWS]
    assert not rest, rest


def test_scalar_rows_are_scalar():
    """the rows that are there for the element-load path really leave the 16-byte path: head dim % 8, qkv % 16 or out % 8"""
    for name, row in hc.ATTN_ROWS.items():
        if "off" in name:
            assert (row["qkv_off"] % 16 or row["out_off"] % 8) and row["hd"] % 8 == 0, name
    scalar = {row["route"] for row in hc.ATTN_ROWS.values() if row["hd"] % 8 or row["qkv_off"] % 16 or row["out_off"] % 8}
    # element loads run in the four-wave and both eight-wave resident kernels, with and without windows and tiles, and in the
    # generic kernel of every head-dim class
    assert scalar >= {"resident<32,global,4x1>", "resident<32,global,8x1>", "resident<64,global,8x1>", "resident<64,global,8x2>",
                      "resident<64,swin,4x1>", "resident<32,swin,4x1>", "generic<32,global>", "generic<64,global>",
                      "generic<96,global>", "generic<128,global>"}, scalar


# ---- the switches: one child process per environment (each is read once per process) ----------------------------------------
SWITCHES = hc.ATTN_SWITCHES      # setting -> what a row's default route becomes under it


@pytest.mark.parametrize("setting", sorted(SWITCHES))
def test_switches_move_the_cases_onto_the_fall_back_routes(setting):
    code = ("import sys, json; sys.path[:0] = [%r, %r, %r]; import hip_checks as hc\n"
            "print('ROUTES=' + json.dumps({n: hc.attn_row_route(n) for n in hc.ATTN_ROWS}))\n"
            % (ROOT, os.path.join(ROOT, "tensorflow-image-models_amd"), os.path.join(ROOT, "tests")))
    key, value = setting.split("=")
    env = {k: v for k, v in os.environ.items() if not k.startswith("TFIMM_ATTN_")}
    env[key] = value
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROUTES=")][-1][len("ROUTES="):])
    assert set(got) == set(hc.ATTN_ROWS)
    want = {n: SWITCHES[setting](row["route"], row) for n, row in hc.ATTN_ROWS.items()}
    wrong = {n: (want[n], got[n]) for n in got if got[n] != want[n]}
    assert not wrong, f"{setting} (expected, reached): {wrong}"
    names = set(got.values())
    if key == "TFIMM_ATTN_NO_STREAM":
        assert not any(n.startswith("stream<") for n in names)
    if key == "TFIMM_ATTN_NO_WINDOW":
        assert not any(n.startswith("window_") for n in names)
    if setting == "TFIMM_ATTN_NO_RESIDENT=1":
        assert all(n.startswith("generic<") for n in names)
        assert names == {r for r in ROUTES if r.startswith("generic<")}       # the six generic instantiations, all of them
    if key == "TFIMM_ATTN_WIN_V1":
        assert "window_v1<32>" in names and not any(n.startswith("window_persist") for n in names)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _global(**kw):
    f = dict(qkv=0x100000, out=0x200000, batch=1, n_tokens=16, heads=1, hd=32, scale=1.0, window=0, shift=0, res=(0, 0),
             rel_bias=None, bias_log2=None)
    f.update(kw)
    return H.attn_desc(**f)


def _window(**kw):
    f = dict(window=7, shift=3, res=(14, 14), n_tokens=196, rel_bias=0x300000, bias_log2=0x400000)
    f.update(kw)
    return _global(**f)


REFUSALS = [
    # (what, descriptor, code, phrase of tfimm_hip_last_error())
    ("null descriptor", None, EINVAL, "null descriptor"),
    ("null qkv", _global(qkv=None), EINVAL, "null pointer"),
    ("null out", _global(out=None), EINVAL, "null pointer"),
    ("batch 0", _global(batch=0), EINVAL, "bad shape"),
    ("batch -3", _global(batch=-3), EINVAL, "bad shape"),
    ("n_tokens 0", _global(n_tokens=0), EINVAL, "bad shape"),
    ("n_tokens -3", _global(n_tokens=-3), EINVAL, "bad shape"),
    ("heads 0", _global(heads=0), EINVAL, "bad shape"),
    ("heads -3", _global(heads=-3), EINVAL, "bad shape"),
    ("hd 0", _global(hd=0), EINVAL, "bad shape"),
    ("hd -3", _global(hd=-3), EINVAL, "bad shape"),
    ("hd 129", _global(hd=129), EUNSUP, "head dim 129 > 128"),
    ("window with hd 65", _window(hd=65), EUNSUP, "windows with head dim 65"),
    # each geometry condition with every other one satisfied (res_h <= 0 alone would also break the product: both negative
    # keeps the product and, in C, the remainders)
    ("res_h 0", _window(res=(0, 14)), EINVAL, "bad window geometry"),
    ("res_h, res_w < 0", _window(res=(-14, -14)), EINVAL, "bad window geometry"),
    ("res_h % window", _window(res=(15, 14), n_tokens=210), EINVAL, "bad window geometry"),
    ("res_w % window", _window(res=(14, 15), n_tokens=210), EINVAL, "bad window geometry"),
    ("res_h * res_w != n_tokens", _window(n_tokens=195), EINVAL, "bad window geometry"),
    ("shift < 0", _window(shift=-1), EINVAL, "bad window geometry"),
    ("shift == window", _window(shift=7), EINVAL, "bad window geometry"),
    # the generic kernel reads rel_bias, the resident and window kernels the tiles: tiles alone are refused on every route
    ("tiles without rel_bias", _window(rel_bias=None), EINVAL, "without rel_bias"),
    ("tiles without rel_bias, window 17", _window(rel_bias=None, window=17, shift=8, res=(34, 34), n_tokens=1156), EINVAL, "without rel_bias"),
    ("grid of 2^31 blocks", _global(batch=1 << 20, heads=1 << 11, n_tokens=64, hd=1), EINVAL, "grid too large"),
]


def test_the_descriptors_next_to_the_refused_ones_are_accepted():
    assert H.attention_route(_global()) == (0, "resident<32,global,4x1>")
    assert H.attention_route(_window()) == (0, "window_persist<32,hpw1>")
    assert H.attention_route(_window(bias_log2=None)) == (0, "resident<32,swin,4x1>")
    assert H.attention_route(_window(rel_bias=None, bias_log2=None)) == (0, "resident<32,swin,4x1>")      # no bias at all
    assert H.attention_route(_window(hd=64)) == (0, "resident<64,swin,4x1>")
    assert H.attention_route(_global(hd=128)) == (0, "generic<128,global>")
    assert H.attention_route(_global(rel_bias=None, bias_log2=0x400000)) == (0, "resident<32,global,4x1>")   # window == 0: ignored
    assert H.attention_route(_global(batch=(1 << 20) - 1, heads=1 << 11, n_tokens=64, hd=1))[0] == 0          # 2^31 - 2^11 blocks


@pytest.mark.parametrize("what,d,code,phrase", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_attention_refusals(what, d, code, phrase):
    rc, msg = H.attention_route(d)
    assert rc == code and phrase in msg, (what, rc, msg)
    if torch.cuda.is_available():
        return       # with a device only the export: a check that went missing must not be able to launch with these addresses
    rc = ffi.lib.tfimm_hip_attention(None if d is None else C.byref(d), None)
    msg = ffi.lib.tfimm_hip_last_error().decode()
    assert rc == code and phrase in msg, (what, rc, msg)


def test_route_export_needs_a_name_buffer():
    d = _global()
    assert ffi.lib.tfimm_hip_dbg_attention_route(C.byref(d), None, 0) == EINVAL
    short = C.create_string_buffer(8)
    assert ffi.lib.tfimm_hip_dbg_attention_route(C.byref(d), short, len(short)) == 0
    assert short.value == b"residen"                        # truncated, terminated


@pytest.mark.skipif(torch.cuda.is_available(), reason="refusal rows of entry points without a route export run only without a device")
def test_cait_attention_refusals():
    """tfimm_hip_talking_heads_attention and tfimm_hip_class_attention: the shapes they have no kernel for"""
    lib = ffi.lib
    w = np.zeros(17 * 17, dtype=np.float32)

    def tha(heads, hd, n_tokens, batch=1):
        d = ffi.ThaDesc()
        d.qkv, d.out = 0x100000, 0x200000
        d.proj_l_w = d.proj_l_b = d.proj_w_w = d.proj_w_b = w.ctypes.data
        d.batch, d.n_tokens, d.heads, d.hd, d.scale = batch, n_tokens, heads, hd, 1.0
        return lib.tfimm_hip_talking_heads_attention(C.byref(d), None), lib.tfimm_hip_last_error().decode()

    rc, msg = tha(17, 48, 196)
    assert rc == EUNSUP and "17 heads > 16" in msg, (rc, msg)
    # 5 heads are not an MFMA instantiation: the fp32 kernel takes them while 2 * heads * n_tokens floats fit in 160 KiB of LDS
    rc, msg = tha(5, 48, 4097)
    assert rc == EUNSUP and "hd=48 heads=5 n=4097 has no kernel" in msg, (rc, msg)
    p = C.c_void_p(0x100000)
    rc = lib.tfimm_hip_class_attention(p, p, p, 1, 16385, 1, 48, 48, 96, 48, None)
    assert rc == EUNSUP and "16385 tokens" in lib.tfimm_hip_last_error().decode()
    rc = lib.tfimm_hip_class_attention(p, p, p, 1 << 20, 16, 1 << 12, 1, 1 << 12, 1 << 13, 1 << 12, None)
    assert rc == EINVAL and "grid too large" in lib.tfimm_hip_last_error().decode()


# ---- the host bias tiles are generic in the window ---------------------------------------------------------------------------
@pytest.mark.parametrize("ws", [4, 7, 8, 9, 11, 12, 16, 17])
def test_swin_bias_tiles_for_every_window(ws):
    """pack.swin_bias_tiles against the mask as swin.py builds it (region ids of the three slices per axis, -100 between
    regions), on a 3 x 2 grid of windows so that inner, last-row, last-column and corner windows all occur"""
    n, heads, log2e = ws * ws, 2, 1.4426950408889634
    bias = np.random.default_rng(ws).standard_normal((heads, n, n)).astype(np.float32)
    Hr, Wr = 3 * ws, 2 * ws
    for shift in (0, ws // 2, 1, ws - 1):
        tiles = pack.swin_bias_tiles(bias, ws, shift)
        nkp = (n + 63) // 64 * 64
        assert tiles.shape == (4 if shift else 1, heads, n, nkp) and tiles.dtype == np.float32
        assert not tiles[..., n:].any()
        img = np.zeros((Hr, Wr))
        if shift:
            cnt = 0
            for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                    img[hs, wsl] = cnt
                    cnt += 1
        mw = img.reshape(Hr // ws, ws, Wr // ws, ws).transpose(0, 2, 1, 3).reshape(-1, n)
        for w in range(mw.shape[0]):
            wy, wx = divmod(w, Wr // ws)
            kind = (2 * (wy == Hr // ws - 1) + (wx == Wr // ws - 1)) if shift else 0
            mask = np.where(mw[w][None, :] - mw[w][:, None] != 0, -100.0, 0.0)
            want = ((bias.astype(np.float64) + mask) * log2e).astype(np.float32)
            assert np.array_equal(tiles[kind][:, :, :n], want), (ws, shift, w)

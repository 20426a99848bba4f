"""The coarse-to-fine gallery search without a device: the written rule of tests/coarse_ref.py -- its e4m3
encoder against torch's, the row quantisation on exact data --, the refusals of tfimm_hip_embed_quantize_rows /
tfimm_hip_embed_search_coarse and of ``Gallery.search_coarse`` before any device work, and what the float32 bands prove about
the candidates: on random data every exact top-k row is surely a candidate (so the GPU tests may ask for the bits of the exact
search), in a clustered case some surely are not (so an implementation that ran the exact search would be caught)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import coarse_ref as cr
import embed_ref as er
import tfimm
from tfimm.engine import ffi

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def test_encoder_agrees_with_torch_on_every_bf16_value():
    v = (np.arange(1 << 16, dtype=np.uint32) << 16).view(f32)
    v = v[np.isfinite(v)].astype(np.float64)
    for j in range(-3, 4):
        x = np.ldexp(v, j)
        x = x[np.abs(x) <= 448]
        assert len(x) > 30000
        want = torch.from_numpy(x.astype(f32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        assert np.array_equal(cr.e4m3_encode(x), want), j
    codes = np.arange(256, dtype=np.uint8)
    back = torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    assert np.array_equal(cr.e4m3_decode(codes), back, equal_nan=True)
    assert cr.e4m3_encode([np.inf, -np.inf, np.nan, 449.0]).tolist()[:2] == [0x7f, 0xff] and cr.e4m3_encode([448.0])[0] == 0x7e


def test_grid_data_quantises_without_loss():
    g = cr.grid(3, (500, 48))
    g[7] = 0
    g[8, 0] = 0.5
    codes, exps = cr.quantize_rows(g)
    assert exps[8] == -9 and exps[7] == 0 and not codes[7].any()
    assert (exps[np.abs(g).max(1) == 0.5] == -9).all() and (np.abs(g).max(1) == 0.5).sum() > 400
    assert np.array_equal(np.ldexp(cr.e4m3_decode(codes), exps.astype(np.int64)[:, None]), g.astype(np.float64))
    # and so the coarse keys order the rows as the exact scores do: the rule gives the exact search
    q = cr.grid(4, (5, 48))
    keys, _ = cr.keys64(q, g)
    _, eq = cr.quantize_rows(q)
    assert np.array_equal(np.ldexp(keys, eq.astype(np.int64)[:, None]), er.scores64(q, g))
    idx, sc, _ = cr.search_coarse(q, g, 7, 28)
    want = er.search(q, g, 7)
    assert np.array_equal(idx, want[0]) and np.array_equal(er.bits(sc), er.bits(want[1]))


def test_row_exponents_at_their_edges():
    amax = np.array([448.0, 449.0, 448 * 2.0 ** -20, 2.0 ** 127, 2.0 ** -133, 2.0 ** -118, 2.0 ** -119, 0.0, 1.0])
    assert cr.row_exponents(amax[:, None]).tolist() == [0, 1, -20, 119, -126, -126, -126, 0, -8]
    rows = er.bf16_round(np.random.default_rng(0).standard_normal((200, 32)).astype(f32) * 1e3)
    codes, exps = cr.quantize_rows(rows)
    scaled = np.abs(np.ldexp(rows.astype(np.float64), -exps.astype(np.int64)[:, None])).max(1)
    assert (scaled <= 448).all() and (scaled > 224).all()                   # the smallest power of two that fits


# ---- the C entry points -------------------------------------------------------------------------------------------------------------
def _aligned(nbytes, align=64):
    raw = np.zeros(nbytes + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + nbytes]


def _search(q=True, ld_q=32, B=2, g=True, ld_g=32, codes=True, ld_c=32, exps=True, N=100, E=32, k=5, candidates=20, chunk=0,
            scores=True, indices=True, workspace=True, workspace_bytes=1 << 16, g_off=0, c_off=0, e_off=0):
    bufs = [_aligned(1 << 16) for _ in range(7)]
    on = (q, g, codes, exps, scores, indices, workspace)
    off = (0, g_off, c_off, e_off, 0, 0, 0)
    p = [C.c_void_p(b.ctypes.data + o) if f else None for b, f, o in zip(bufs, on, off)]
    rc = ffi.lib.tfimm_hip_embed_search_coarse(p[0], ld_q, B, p[1], ld_g, p[2], ld_c, p[3], N, E, k, candidates, chunk, p[4], p[5],
                                               p[6], workspace_bytes, None)
    return rc, ffi.lib.tfimm_hip_last_error().decode()


@pytest.mark.parametrize("kw, names", [
    (dict(q=False), "q is null"), (dict(g=False), "g is null"), (dict(codes=False), "codes is null"), (dict(exps=False), "exps is null"),
    (dict(scores=False), "scores is null"), (dict(indices=False), "indices is null"), (dict(workspace=False), "workspace is null"),
    (dict(g_off=8), "16-byte aligned"), (dict(c_off=8), "16-byte aligned"), (dict(e_off=1), "4-byte aligned"),
    (dict(E=0), "E=0"), (dict(E=24, ld_q=24, ld_g=24), "E=24"), (dict(E=2064, ld_q=2064, ld_g=2064, ld_c=2064), "E=2064"),
    (dict(N=0), "N=0"), (dict(k=0), "k=0"), (dict(k=21), "k=21"), (dict(k=21), "candidates = 20"),
    (dict(candidates=0), "candidates=0"), (dict(candidates=101), "candidates=101"), (dict(N=1000, candidates=257), "candidates=257"),
    (dict(N=1000, E=2048, ld_q=2048, ld_g=2048, ld_c=2048, candidates=255), "max_candidates(2048) = 254"),
    (dict(chunk=-32), "chunk=-32"), (dict(chunk=48), "chunk=48"), (dict(B=-1), "B=-1"), (dict(B=65535 * 32 + 1), "B=2097121"),
    (dict(ld_q=31), "ld_q=31"), (dict(ld_g=24), "ld_g=24"), (dict(ld_g=36), "ld_g=36"), (dict(ld_c=24), "ld_c=24"),
    (dict(ld_c=40), "ld_c=40"), (dict(workspace_bytes=8), "workspace_bytes=8"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_coarse_search_refusals_name_the_argument(kw, names):
    rc, msg = _search(**kw)
    assert rc == -1 and msg.startswith("embed_search_coarse:") and names in msg, (rc, msg)


def test_quantize_refusals_and_the_empty_call():
    a, b, c = (_aligned(1 << 12) for _ in range(3))
    ptr = lambda x, o=0: C.c_void_p(x.ctypes.data + o)      # noqa: E731
    fn = ffi.lib.tfimm_hip_embed_quantize_rows
    for args, names in (((None, 32, 4, 32, ptr(b), 32, ptr(c)), "g is null"), ((ptr(a), 32, 4, 32, None, 32, ptr(c)), "codes is null"),
                        ((ptr(a), 32, 4, 32, ptr(b), 32, None), "exps is null"), ((ptr(a, 8), 32, 4, 32, ptr(b), 32, ptr(c)), "aligned"),
                        ((ptr(a), 32, 4, 24, ptr(b), 32, ptr(c)), "E=24"), ((ptr(a), 32, -1, 32, ptr(b), 32, ptr(c)), "N=-1"),
                        ((ptr(a), 36, 4, 32, ptr(b), 32, ptr(c)), "ld_g=36"), ((ptr(a), 32, 4, 32, ptr(b), 40, ptr(c)), "ld_c=40"),
                        ((ptr(a), 32, 4, 32, ptr(b), 16, ptr(c)), "ld_c=16")):
        assert fn(*args, None) == -1
        msg = ffi.lib.tfimm_hip_last_error().decode()
        assert msg.startswith("embed_quantize_rows:") and names in msg, msg
    assert fn(ptr(a), 32, 0, 32, ptr(b), 32, ptr(c), None) == 0            # no rows: returns before any launch
    assert _search(B=0)[0] == 0


def test_max_candidates_workspace_and_constants():
    """32 (E + 16) + 32 * 8 * cap <= 160 KiB with cap >= candidates + 128, and candidates <= 256"""
    most = ffi.lib.tfimm_hip_embed_search_coarse_max_candidates
    for E in range(16, 2049, 16):
        assert most(E) == min(256, (160 * 1024 - 32 * (E + 16)) // (32 * 8) - 128), E
        assert most(E) == 256 if E <= 768 else most(E) >= 64
    assert most(2032) == 256 and most(2048) == 254 and most(0) == most(24) == most(2064) == 0
    ws = ffi.lib.tfimm_hip_embed_search_coarse_workspace
    assert ws(3, 5000, 64, 5, 20, 32) == 3 * (157 + 1) * 20 * 8            # candidates pairs per (query, chunk), and per query
    assert ws(3, 5000, 64, 5, 200, 4096) == 3 * (2 + 1) * 200 * 8
    assert ws(32, 1_000_000, 64, 5, 20, 0) == 32 * (-(-1_000_000 // 512) + 1) * 20 * 8      # chunk = 0: as the wide search's
    assert ws(0, 100, 32, 5, 20, 0) == ws(1, 100, 32, 5, 20, 0) > 0
    assert ws(1, 1000, 2048, 5, 254, 0) > 0 and ws(1, 1000, 2048, 5, 255, 0) == -1
    assert ws(1, 100, 32, 21, 20, 0) == -1 and "k=21" in ffi.lib.tfimm_hip_last_error().decode()
    hdr = open(os.path.join(ROOT, "include", "tfimm_hip.h")).read()
    assert int(re.search(r"#define TFIMM_EMBED_COARSE_MAX_CANDIDATES (\d+)", hdr).group(1)) == ffi.EMBED_COARSE_MAX_CANDIDATES == 256
    for name in ("tfimm_hip_embed_quantize_rows", "tfimm_hip_embed_search_coarse", "tfimm_hip_embed_search_coarse_workspace",
                 "tfimm_hip_embed_search_coarse_max_candidates"):
        assert f" {name}(" in hdr and hasattr(ffi.lib, name)
    assert ffi.lib.tfimm_hip_abi_version() == 4


# ---- Gallery.search_coarse before any device work -----------------------------------------------------------------------------------
@pytest.fixture
def hostless(monkeypatch):
    """``Gallery._store`` replaced by the bookkeeping alone (tests/test_search_wide.py): nothing is uploaded"""
    def store(self, t, up_labels, n):
        self._labelled = self._labelled or up_labels is not None
        first, self._n = self._n, self._n + n
        return range(first, self._n)
    monkeypatch.setattr(tfimm.Gallery, "_store", store)


def _gallery(n, dim=32):
    g = tfimm.Gallery(dim)
    g.add(np.zeros((n, dim), f32), np.arange(n) % 7)
    return g


def test_signatures():
    sig = inspect.signature(tfimm.Gallery.search_coarse).parameters
    assert list(sig) == ["self", "q", "k", "candidates", "chunk"]
    assert (sig["k"].default, sig["candidates"].default, sig["chunk"].default) == (5, None, 0)
    sig = inspect.signature(tfimm.EmbeddingModel.search_coarse).parameters
    assert list(sig) == ["self", "x", "gallery", "k", "candidates"] and (sig["k"].default, sig["candidates"].default) == (5, None)
    assert list(inspect.signature(tfimm.Gallery.build_coarse).parameters) == ["self"]
    assert isinstance(tfimm.Gallery.coarse, property)
    assert "coarse" not in tfimm.models.gallery._METHODS                    # "auto" never takes the coarse path


def test_search_coarse_value_errors_come_before_device_work(hostless):
    g = _gallery(1000)
    q = np.zeros((2, 32), f32)
    assert g.coarse is False
    with pytest.raises(ValueError, match="no coarse copy.*build_coarse"):
        g.search_coarse(q)
    g.build_coarse()                                                        # nothing on the device yet: bookkeeping alone
    assert g.coarse is True
    with pytest.raises(ValueError, match=r"k = 21, must be in \[1, candidates = 20\]"):
        g.search_coarse(q, 21, candidates=20)
    with pytest.raises(ValueError, match=r"k = 0"):
        g.search_coarse(q, 0)
    with pytest.raises(ValueError, match="integer"):
        g.search_coarse(q, 5.0)
    with pytest.raises(ValueError, match="integer"):
        g.search_coarse(q, 5, candidates=20.0)
    with pytest.raises(ValueError, match=r"candidates = 257: rows of dim 32 allow candidates <= 256"):
        g.search_coarse(q, 5, candidates=257)
    with pytest.raises(ValueError, match=r"candidates = 255: rows of dim 2048 allow candidates <= 254"):
        w = _gallery(1000, 2048)
        w.build_coarse()
        w.search_coarse(np.zeros((2, 2048), f32), 5, candidates=255)
    small = _gallery(100)
    small.build_coarse()
    with pytest.raises(ValueError, match=r"candidates = 101, must be in \[1, len = 100\]"):
        small.search_coarse(q, 5, candidates=101)
    with pytest.raises(ValueError, match=r"k = 101, must be in \[1, candidates = 100\]"):
        small.search_coarse(q, 101)                                         # the default is capped by len
    # the default: min(max(4 k, 32), max_candidates(dim), len)
    assert [g._coarse_args(k, None) for k in (1, 5, 8, 9, 20, 64, 200)] == [32, 32, 32, 36, 80, 256, 256]
    assert small._coarse_args(64, None) == 100 and w._coarse_args(64, None) == 254
    assert not g._work_coarse and not small._work_coarse and not g._work
    # galleries that others make start without a coarse copy
    assert tfimm.Gallery._of_rows(16, torch.zeros((3, 16)), torch.zeros(3, dtype=torch.int32)).coarse is False


# ---- what the bands prove --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [64, 768])
def test_on_random_data_every_exact_top_k_row_is_surely_a_candidate(E):
    q, g = cr.random_case(E)
    for k, c in cr.RANDOM_PAIRS:
        held, missed, _, _, _ = cr.margins(q, g, k, c)
        assert held.all() and not missed.any(), (k, c)


def test_the_lossy_case_surely_loses_exact_top_k_rows():
    seed, E, centres, noise, N, B, k, c = cr.LOSSY
    q, g = cr.clustered(seed, E, centres, noise, N, B)
    held, missed, sure, top, cand = cr.margins(q, g, k, c)
    assert missed.any(1).sum() == 30 and sure.sum() == 31 and (missed.any(1) & sure).sum() == 29
    assert not (held & missed.any(1)).any()
    for b in np.flatnonzero(missed.any(1)):                                 # the rule itself leaves those rows out
        assert not set(top[b][missed[b]].tolist()) & set(cand[b].tolist())
    idx, _, _ = cr.search_coarse(q, g, k, c)
    assert (idx != top).any(1).sum() >= 30

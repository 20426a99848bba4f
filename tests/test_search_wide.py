"""The search for up to 256 neighbours without a device: every refusal of tfimm_hip_embed_search_wide and its
workspace query names its argument and comes before any launch, tfimm_hip_embed_search_wide_max_k is the LDS formula of the
header, and ``Gallery.search`` / ``Gallery.search_with`` decide ``k`` and ``method`` before any device work."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import tfimm
from tfimm.engine import ffi
from tfimm.models import gallery as gallery_module

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _aligned(nbytes, align=64):
    raw = np.zeros(nbytes + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + nbytes]


def _search(q=True, ld_q=32, B=2, g=True, ld_g=32, N=100, E=32, k=5, chunk=0, scores=True, indices=True, workspace=True,
            workspace_bytes=None, g_off=0, q_off=0):
    bufs = [_aligned(1 << 16) for _ in range(5)]
    on = (q, g, scores, indices, workspace)
    off = (q_off, g_off, 0, 0, 0)
    ptr = [C.c_void_p(b.ctypes.data + o) if f else None for b, f, o in zip(bufs, on, off)]
    if workspace_bytes is None:
        workspace_bytes = 1 << 16
    rc = ffi.lib.tfimm_hip_embed_search_wide(ptr[0], ld_q, B, ptr[1], ld_g, N, E, k, chunk, ptr[2], ptr[3], ptr[4], workspace_bytes,
                                             None)
    return rc, ffi.lib.tfimm_hip_last_error().decode()


@pytest.mark.parametrize("kw, names", [
    (dict(q=False), "q is null"), (dict(g=False), "g is null"), (dict(scores=False), "scores is null"),
    (dict(indices=False), "indices is null"), (dict(workspace=False), "workspace is null"),
    (dict(g_off=8), "g must be 16-byte aligned"), (dict(q_off=2), "4-byte aligned"),
    (dict(E=0), "E=0"), (dict(E=8), "E=8"), (dict(E=24, ld_q=24, ld_g=24), "E=24"), (dict(E=2064, ld_q=2064, ld_g=2064), "E=2064"),
    (dict(N=0), "N=0"), (dict(N=-5), "N=-5"),
    (dict(k=0), "k=0"), (dict(k=-1), "k=-1"), (dict(k=101), "k=101"), (dict(N=1000, k=257), "k=257"),
    (dict(N=1000, E=2048, ld_q=2048, ld_g=2048, k=65), "k=65"), (dict(N=1000, E=2048, ld_q=2048, ld_g=2048, k=65), "E=2048"),
    (dict(N=1000, E=1024, ld_q=1024, ld_g=1024, k=255), "E=1024 with k=255"),
    (dict(chunk=-32), "chunk=-32"), (dict(chunk=48), "chunk=48"),
    (dict(ld_q=31), "ld_q=31"), (dict(ld_g=24), "ld_g=24"), (dict(ld_g=36), "ld_g=36"), (dict(B=-1), "B=-1"),
    (dict(B=65535 * 32 + 1), "B=2097121"),
    (dict(workspace_bytes=8), "workspace_bytes=8"),
    (dict(N=100000, k=200, chunk=32, workspace_bytes=1 << 16), "workspace_bytes=65536"),     # 3125 chunks: no limit but the bytes
], ids=lambda v: v if isinstance(v, str) else None)
def test_wide_search_refusals_name_the_argument(kw, names):
    rc, msg = _search(**kw)
    assert rc == -1 and msg.startswith("embed_search_wide:") and names in msg, (rc, msg)


@pytest.mark.parametrize("args, names", [
    ((1, 100, 24, 5, 0), "E=24"), ((1, 100, 32, 101, 0), "k=101"), ((1, 1000, 32, 257, 0), "k=257"), ((1, 100, 32, 5, 48), "chunk=48"),
    ((1, 0, 32, 1, 0), "N=0"), ((-1, 100, 32, 5, 0), "B=-1"), ((1, 1000, 2048, 65, 0), "E=2048 with k=65"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_wide_workspace_refusals_name_the_argument(args, names):
    assert ffi.lib.tfimm_hip_embed_search_wide_workspace(*args) == -1
    msg = ffi.lib.tfimm_hip_last_error().decode()
    assert msg.startswith("embed_search_wide:") and names in msg, msg


def test_workspace_sizes_chunks_and_the_empty_batch():
    ws = ffi.lib.tfimm_hip_embed_search_wide_workspace
    assert ws(3, 5000, 64, 5, 32) == 3 * 157 * 5 * 8                     # k (key, row) pairs per query and chunk
    assert ws(3, 5000, 64, 200, 4096) == 3 * 2 * 200 * 8
    assert ws(1, 1_000_000, 512, 200, 32) == 31250 * 200 * 8             # no limit on the number of chunks
    # chunk = 0: 2048 chunks per query tile wanted, in whole steps of 128 rows, never fewer than 4 k rows
    for B, N, k, chunk in ((32, 1_000_000, 5, 512), (32, 1_000_000, 200, 896), (32, 1_000_000, 256, 1024), (1, 257, 256, 1024),
                           (256, 100_000, 20, 512), (256, 100_000, 200, 896), (70, 40000, 64, 256), (1, 5000, 1, 128)):
        assert ws(B, N, 64, k, 0) == B * -(-N // chunk) * k * 8, (B, N, k)
    assert ws(0, 100, 32, 5, 0) == ws(1, 100, 32, 5, 0) > 0
    assert _search(B=0)[0] == 0                                           # returns before any launch
    assert ws(ffi.EMBED_MAX_B, 100, 32, 5, 0) > 0 and ws(ffi.EMBED_MAX_B + 1, 100, 32, 5, 0) < 0


def test_max_k_is_the_lds_formula():
    """32 (2 E + 16) + 32 * 8 * cap <= 160 KiB with cap >= k + 128, and k <= 256"""
    max_k = ffi.lib.tfimm_hip_embed_search_wide_max_k
    for E in (16, 512, 768, 1024, 2048):
        cap = (160 * 1024 - 32 * (2 * E + 16)) // (32 * 8)
        assert max_k(E) == min(256, cap - 128), E
    assert [max_k(E) for E in (16, 512, 768, 1024)] == [256, 256, 256, 254] and max_k(2048) <= 0
    assert max_k(784) == 256 and max_k(1008) == 256 and max_k(1040) < 254            # every k up to E = 768 and a little beyond
    assert max_k(0) == 0 and max_k(24) == 0 and max_k(2064) == 0                     # outside the domain: no k
    # the entry point agrees with it on both sides
    ws = ffi.lib.tfimm_hip_embed_search_wide_workspace
    assert ws(1, 1000, 1024, 254, 0) > 0 and ws(1, 1000, 1024, 255, 0) < 0 and ws(1, 1000, 768, 256, 0) > 0
    assert ws(1, 1000, 2048, 1, 0) < 0


def test_constants_header_and_abi():
    hdr = open(os.path.join(ROOT, "include", "tfimm_hip.h")).read()
    assert int(re.search(r"#define TFIMM_EMBED_WIDE_MAX_K (\d+)", hdr).group(1)) == ffi.EMBED_WIDE_MAX_K == 256
    assert int(re.search(r"#define TFIMM_EMBED_MAX_K (\d+)", hdr).group(1)) == ffi.EMBED_MAX_K == ffi.KNN_MAX_K == 64
    assert ffi.lib.tfimm_hip_abi_version() == 4
    for name in ("tfimm_hip_embed_search_wide", "tfimm_hip_embed_search_wide_workspace", "tfimm_hip_embed_search_wide_max_k"):
        assert f" {name}(" in hdr and hasattr(ffi.lib, name)
    assert gallery_module.SEARCH_BUFFER_FROM_K == 20                                 # profiles/search_wide_probe.txt; 65: never


@pytest.fixture
def hostless(monkeypatch):
    """``Gallery._store`` replaced by the bookkeeping alone (tests/test_knn.py): nothing is uploaded"""
    def store(self, t, up_labels, n):
        self._labelled = self._labelled or up_labels is not None
        first, self._n = self._n, self._n + n
        return range(first, self._n)
    monkeypatch.setattr(tfimm.Gallery, "_store", store)


def _gallery(n, dim=32):
    g = tfimm.Gallery(dim)
    g.add(np.zeros((n, dim), f32), np.arange(n) % 7)
    return g


def test_gallery_search_value_errors_come_before_device_work(hostless):
    assert list(inspect.signature(tfimm.Gallery.search).parameters) == ["self", "q", "k", "chunk"]      # as it was: "auto"
    sig = inspect.signature(tfimm.Gallery.search_with).parameters
    assert list(sig) == ["self", "q", "k", "chunk", "method"] and sig["method"].default == "auto"
    assert (sig["k"].default, sig["chunk"].default) == (5, 0)
    sig = inspect.signature(tfimm.EmbeddingModel.search).parameters
    assert list(sig) == ["self", "x", "gallery", "k", "method"] and sig["method"].default == "auto"
    g = _gallery(1000)
    q = np.zeros((2, 32), f32)
    for method in ("heap", "LIST", "", None, 1):
        with pytest.raises(ValueError, match="method"):
            g.search_with(q, 5, method=method)
    for method in ("auto", "list", "buffer"):
        with pytest.raises(ValueError, match="k = 257"):
            g.search_with(q, 257, method=method)
        with pytest.raises(ValueError, match="k = 257"):
            g.search(q, 257)
        with pytest.raises(ValueError, match="k = 0"):
            g.search_with(q, 0, method=method)
        with pytest.raises(ValueError, match="integer"):
            g.search_with(q, 5.0, method=method)
    with pytest.raises(ValueError, match=r"k = 65 with method='list'.*TFIMM_EMBED_MAX_K = 64"):
        g.search_with(q, 65, method="list")
    for method in ("auto", "buffer"):
        with pytest.raises(ValueError, match=r"k = 101.*len = 100\b"):
            _gallery(100).search_with(q, 101, method=method)
    # k beyond what the width allows: the message says which k it does allow
    wide = _gallery(1000, dim=1024)
    with pytest.raises(ValueError, match=r"k = 255: rows of dim 1024 allow k <= 254"):
        wide.search(np.zeros((2, 1024), f32), 255)
    with pytest.raises(ValueError, match=r"k = 255 with method='buffer': rows of dim 1024 allow k <= 254"):
        wide.search_with(np.zeros((2, 1024), f32), 255, method="buffer")
    widest = _gallery(1000, dim=2048)
    with pytest.raises(ValueError, match=r"k = 65: rows of dim 2048 allow k <= 64"):
        widest.search(np.zeros((2, 2048), f32), 65)
    with pytest.raises(ValueError, match=r"k = 5 with method='buffer': rows of dim 2048 allow no k"):
        widest.search_with(np.zeros((2, 2048), f32), 5, method="buffer")
    assert not g._work and not wide._work and not widest._work                      # no search ran


def test_auto_routes_by_k_and_width(hostless, monkeypatch):
    g, widest = _gallery(1000), _gallery(1000, dim=2048)
    assert g._route(65) == g._route(256) == g._route(5, "buffer") == g._route(64, "buffer") == "buffer"
    assert g._route(5, "list") == g._route(64, "list") == "list"
    assert widest._route(64) == widest._route(1) == "list"                          # no k fits the buffers: the list path
    for first in (1, 20, 64, 65):
        monkeypatch.setattr(gallery_module, "SEARCH_BUFFER_FROM_K", first)
        assert [k for k in range(1, 65) if g._route(k) == "buffer"] == list(range(first, 65))
        assert all(g._route(k) == "buffer" for k in (65, 200, 256))
        assert all(widest._route(k) == "list" for k in (1, 20, 64))


def test_vote_still_refuses_wide_matches(hostless):
    import torch
    g = _gallery(1000)
    with pytest.raises(ValueError, match="k = 100"):
        g.vote(tfimm.Matches(torch.zeros((4, 100), dtype=torch.int32), torch.zeros((4, 100))))
    for call in (lambda: g.classify(np.zeros((2, 32), f32), 65), lambda: g.evaluate(np.zeros((2, 32), f32), [0, 1], k=65, nb_classes=7)):
        with pytest.raises(ValueError, match="k = 65"):
            call()
    assert "64" in tfimm.Gallery.vote.__doc__ and "256" in tfimm.Gallery.search.__doc__

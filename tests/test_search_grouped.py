"""The grouped gallery search over inverted lists without a device (tfimm_hip_embed_search_lists_grouped,
csrc/embed_lists_grouped.hip; ``GalleryIndex.search_with`` / ``neighbours``): the refusals of the new entries
before any launch, the workspace formula, the bound on the tiles of a call against counts made in numpy, the signatures and
``ValueError``s of the Python methods before any device work, and the rule of ``neighbours`` (tests/neighbours_ref.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import coarse_ref as cr
import embed_ref as er
import index_ref as ir
import neighbours_ref as nr
import tfimm
from test_search_index import _aligned, _host_index, hostless  # noqa: F401  (hostless is a fixture)
from tfimm.engine import ffi

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
grid = cr.grid


# ---- the C entry points -------------------------------------------------------------------------------------------------------------
def _grouped(q=True, ld_q=32, B=2, g=True, ld_g=32, N=100, E=32, ids=True, offsets=True, L=4, probes=True, ld_p=2, nprobe=2, k=5, parts=0,
             scores=True, indices=True, workspace=True, workspace_bytes=1 << 16, g_off=0, i_off=0, o_off=0, p_off=0):
    bufs = [_aligned(1 << 16) for _ in range(8)]
    on = (q, g, ids, offsets, probes, scores, indices, workspace)
    off = (0, g_off, i_off, o_off, p_off, 0, 0, 0)
    p = [C.c_void_p(b.ctypes.data + o) if f else None for b, f, o in zip(bufs, on, off)]
    rc = ffi.lib.tfimm_hip_embed_search_lists_grouped(p[0], ld_q, B, p[1], ld_g, N, E, p[2], p[3], L, p[4], ld_p, nprobe, k, parts, p[5],
                                                      p[6], p[7], workspace_bytes, None)
    return rc, ffi.lib.tfimm_hip_last_error().decode()


def tiles(B, L, nprobe):
    """the bound as the header states it"""
    P = B * nprobe
    return min(P // 32 + min(L, P), min(L, P) * -(-B // 32))


def need(B, L, nprobe, k, parts):
    """the workspace as the header states it: the pair arrays, count, first, rank, list per tile, members"""
    B = max(B, 1)
    T = tiles(B, L, nprobe)
    return B * nprobe * parts * k * 8 + 4 * (L + (L + 1) + B * nprobe + T + 32 * T)


@pytest.mark.parametrize("kw, names", [
    (dict(q=False), "q is null"), (dict(g=False), "g is null"), (dict(ids=False), "ids is null"), (dict(offsets=False), "offsets is null"),
    (dict(probes=False), "probes is null"), (dict(scores=False), "scores is null"), (dict(indices=False), "indices is null"),
    (dict(workspace=False), "workspace is null"), (dict(g_off=8), "16-byte aligned"), (dict(i_off=2), "4-byte aligned"),
    (dict(o_off=1), "4-byte aligned"), (dict(p_off=3), "4-byte aligned"),
    (dict(E=0), "E=0"), (dict(E=24, ld_q=24, ld_g=24), "E=24"), (dict(E=2064, ld_q=2064, ld_g=2064), "E=2064"),
    (dict(N=0), "N=0"), (dict(N=-5), "N=-5"), (dict(k=0), "k=0"), (dict(k=257), "k=257"), (dict(k=257), "TFIMM_EMBED_WIDE_MAX_K = 256"),
    (dict(nprobe=0), "nprobe=0"), (dict(nprobe=257, ld_p=257), "nprobe=257"), (dict(ld_p=1), "ld_p=1"),
    (dict(L=0), "L=0"), (dict(L=65537), "L=65537"), (dict(parts=-1), "parts=-1"), (dict(parts=65), "parts=65"),
    (dict(B=-1), "B=-1"), (dict(B=65536), "B=65536"), (dict(ld_q=31), "ld_q=31"), (dict(ld_g=24), "ld_g=24"), (dict(ld_g=36), "ld_g=36"),
    (dict(workspace_bytes=8), "workspace_bytes=8"),
    (dict(parts=3, workspace_bytes=need(2, 4, 2, 5, 3) - 1), f"asks for {need(2, 4, 2, 5, 3)}"),
    # the width's limit: 32 buffers share LDS with the query tile
    (dict(E=2048, ld_q=2048, ld_g=2048, k=1), "E=2048 with k=1"), (dict(E=2048, ld_q=2048, ld_g=2048), "tfimm_hip_embed_search_wide_max_k(2048)"),
    (dict(E=1024, ld_q=1024, ld_g=1024, k=255), "E=1024 with k=255"),
    (dict(E=1024, ld_q=1024, ld_g=1024, k=255), "tfimm_hip_embed_search_wide_max_k(1024) = 254"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_grouped_search_refusals_name_the_argument(kw, names):
    rc, msg = _grouped(**kw)
    assert rc == -1 and msg.startswith("embed_search_lists_grouped:") and names in msg, (rc, msg)


def test_the_width_limit_is_the_buffer_paths():
    assert [ffi.lib.tfimm_hip_embed_search_wide_max_k(E) for E in (16, 512, 768, 1024)] == [256, 256, 256, 254]
    assert ffi.lib.tfimm_hip_embed_search_wide_max_k(2048) <= 0
    ws = ffi.lib.tfimm_hip_embed_search_lists_grouped_workspace
    assert ws(2, 100, 1024, 4, 2, 254, 0) > 0 and ws(2, 100, 768, 4, 2, 256, 0) > 0
    assert ws(2, 100, 1024, 4, 2, 255, 0) == -1 and "tfimm_hip_embed_search_wide_max_k" in ffi.lib.tfimm_hip_last_error().decode()
    assert ws(2, 100, 2048, 4, 2, 1, 0) == -1 and "tfimm_hip_embed_search_wide_max_k" in ffi.lib.tfimm_hip_last_error().decode()


def test_the_empty_call_the_workspace_formula_and_the_header():
    assert _grouped(B=0)[0] == 0                                            # no queries: returns before any launch
    assert _grouped(B=0, k=0)[0] == -1                                      # but not before the checks
    ws, single = ffi.lib.tfimm_hip_embed_search_lists_grouped_workspace, ffi.lib.tfimm_hip_embed_search_lists_workspace
    for B, L, nprobe, k, parts in ((3, 300, 2, 5, 1), (70, 300, 37, 200, 7), (1, 300, 256, 256, 64), (65535, 300, 8, 20, 3),
                                   (65535, 65536, 256, 1, 1), (1024, 1024, 32, 5, 4), (33, 1, 1, 5, 2), (2, 4, 2, 5, 3)):
        assert ws(B, 5000, 64, L, nprobe, k, parts) == need(B, L, nprobe, k, parts), (B, L, nprobe, k, parts)
        assert ws(B, 5000, 64, L, nprobe, k, parts) > single(B, 5000, 64, L, nprobe, k, parts) > 0     # the pair arrays, and the tables
    assert ws(3, 5000, 64, 300, 2, 5, 0) == ws(3, 5000, 64, 300, 2, 5, 1)   # parts = 0: the library chooses 1
    assert ws(0, 100, 32, 4, 2, 5, 0) == ws(1, 100, 32, 4, 2, 5, 0) > 0
    assert ws(1, 100, 32, 4, 2, 200, 0) > 0                                 # k may exceed N
    for args, names in (((1, 100, 24, 4, 2, 5, 0), "E=24"), ((1, 100, 32, 4, 2, 257, 0), "k=257"), ((1, 100, 32, 4, 257, 5, 0), "nprobe=257"),
                        ((1, 100, 32, 0, 2, 5, 0), "L=0"), ((1, 100, 32, 4, 2, 5, 65), "parts=65"), ((65536, 100, 32, 4, 2, 5, 0), "B=65536"),
                        ((1, 0, 32, 4, 2, 5, 0), "N=0")):
        assert ws(*args) == -1 and names in ffi.lib.tfimm_hip_last_error().decode(), args
    hdr = open(os.path.join(ROOT, "include", "tfimm_hip.h")).read()
    for name in ("tfimm_hip_embed_search_lists_grouped", "tfimm_hip_embed_search_lists_grouped_workspace",
                 "tfimm_hip_embed_search_lists_grouped_tiles"):
        assert f" {name}(" in hdr and hasattr(ffi.lib, name)
    assert "max(B, 1) * nprobe * parts * k * 8 + 4 * (L + (L + 1) + P + T_max + 32 * T_max)" in hdr          # the formula is stated
    assert "T_max = min(P / 32 + min(L, P), min(L, P) * ceil(B / 32))" in hdr
    assert ffi.EMBED_LISTS_GROUPED_TILE == 32
    assert ffi.lib.tfimm_hip_abi_version() == 4                             # the change is additive
    assert int(re.search(r"#define TFIMM_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 4


# ---- the bound on the tiles of a call ----------------------------------------------------------------------------------------------
def tiles_used(probes, L):
    """sum over the lists of ceil(live pairs / 32), every list taken as non-empty: a pair is live when its list is in [0, L)
    and no earlier slot of its query names it"""
    count = np.zeros(L, np.int64)
    for row in probes:
        named = {int(l) for l in row if 0 <= l < L}
        count[list(named)] += 1
    return int((-(-count // 32)).sum())


@pytest.mark.parametrize("B, L, nprobe", [(1, 1, 1), (70, 37, 5), (33, 300, 256), (1000, 16, 8), (257, 1000, 3), (4096, 64, 32), (31, 7, 7),
                                          (2000, 5, 1), (64, 4096, 17)])
def test_the_tile_bound_holds_for_random_probe_tables(B, L, nprobe):
    bound = ffi.lib.tfimm_hip_embed_search_lists_grouped_tiles(B, L, nprobe)
    assert bound == tiles(B, L, nprobe) >= 1
    rng = np.random.default_rng(B + L)
    for trial in range(4):
        if trial == 0:                                                       # distinct lists per query, as a probe gives them
            probes = np.stack([rng.permutation(max(L, nprobe))[:nprobe] for _ in range(B)])
        elif trial == 1:                                                     # repeats, -1 and L among them
            probes = rng.integers(-1, L + 1, (B, nprobe))
        elif trial == 2:                                                     # skewed: most pairs name a few lists
            probes = np.minimum(rng.geometric(0.3, (B, nprobe)) - 1, L - 1)
        else:                                                                # every list 1 mod 32 times, as far as the pairs go
            probes = (np.arange(B)[:, None] * nprobe + np.arange(nprobe)[None, :]) % L
        assert tiles_used(probes, L) <= bound, (trial, tiles_used(probes, L), bound)


def test_the_tile_bound_is_tight():
    t = ffi.lib.tfimm_hip_embed_search_lists_grouped_tiles
    for B in (1, 31, 32, 33, 64, 65, 1000, 65535):                           # every query names one list
        assert tiles_used(np.zeros((B, 1), int), 1) == t(B, 1, 1) == -(-B // 32)
        assert tiles_used(np.zeros((B, 4), int), 1) == t(B, 1, 4) == -(-B // 32)       # ... four times: it counts once
        assert tiles_used(np.full((B, 1), 3), 10) == -(-B // 32) <= t(B, 10, 1)        # (the bound does not know which list)
    for B, nprobe in ((1, 1), (4, 8), (32, 256), (7, 5)):                    # every pair names a list of its own: P < L
        P = B * nprobe
        probes = np.arange(P).reshape(B, nprobe)
        assert tiles_used(probes, P + 5) == t(B, P + 5, nprobe) == P
    for nprobe in (1, 2, 37, 256):                                           # B = 1
        assert tiles_used(np.arange(nprobe)[None, :], 300) == t(1, 300, nprobe) == nprobe
        assert tiles_used(np.arange(nprobe)[None, :] % 2, 2) == t(1, 2, nprobe) == min(2, nprobe)
    # 32 queries more than a whole number of tiles per list: one tile each on top of P / 32
    B, L = 33 * 8, 8
    probes = np.tile(np.arange(8), (B, 1))
    assert tiles_used(probes, L) == 8 * 9 == t(B, L, 8) == min(B * 8 // 32 + 8, 8 * 9)
    assert t(0, 10, 4) == 0
    assert t(65535, 65536, 256) == 65535 * 256 // 32 + 65536                # about 590 000: the x dimension of the grid
    for args, names in (((-1, 4, 2), "B=-1"), ((65536, 4, 2), "B=65536"), ((1, 0, 2), "L=0"), ((1, 65537, 2), "L=65537"), ((1, 4, 0), "nprobe=0"),
                        ((1, 4, 257), "nprobe=257")):
        assert t(*args) == -1 and names in ffi.lib.tfimm_hip_last_error().decode(), args


# ---- GalleryIndex.search_with / neighbours before any device work ---------------------------------------------------------------------
def test_signatures():
    sig = inspect.signature(tfimm.GalleryIndex.search_with).parameters
    assert list(sig) == ["self", "q", "k", "nprobe", "parts", "method"]
    assert [sig[n].default for n in list(sig)[2:]] == [5, 8, 0, "grouped"]
    sig = inspect.signature(tfimm.GalleryIndex.neighbours).parameters
    assert list(sig) == ["self", "k", "nprobe", "batch", "method"] and [sig[n].default for n in list(sig)[1:]] == [20, 8, 8192, "grouped"]
    sig = inspect.signature(tfimm.GalleryIndex.search).parameters           # search keeps the signature it had
    assert list(sig) == ["self", "q", "k", "nprobe", "parts"] and [sig[n].default for n in ("k", "nprobe", "parts")] == [5, 8, 0]
    assert tfimm.models.gallery_index._METHODS == ("grouped", "single")     # no "auto" until a measurement places it


def test_value_errors_come_before_device_work(hostless):
    g, _, index = _host_index(1000, 10)
    q = np.zeros((2, 32), f32)
    name = "GalleryIndex.search_with"
    for method in ("grouped", "single"):
        with pytest.raises(ValueError, match=name + r": k = 0, must be in \[1"):
            index.search_with(q, 0, method=method)
        with pytest.raises(ValueError, match=name + ": k must be an integer"):
            index.search_with(q, 5.0, method=method)
        with pytest.raises(ValueError, match=name + r": k = 257, must be in \[1, TFIMM_EMBED_WIDE_MAX_K = 256\]"):
            index.search_with(q, 257, method=method)
        with pytest.raises(ValueError, match=name + r": nprobe = 11, must be in \[1, min\(n_lists = 10"):
            index.search_with(q, 5, 11, method=method)
        with pytest.raises(ValueError, match=name + ": nprobe must be an integer"):
            index.search_with(q, 5, 2.0, method=method)
        with pytest.raises(ValueError, match=name + r": parts = 65"):
            index.search_with(q, 5, 2, 65, method)
        with pytest.raises(ValueError, match=name + r": parts = -1"):
            index.search_with(q, 5, 2, -1, method)
        with pytest.raises(ValueError, match=name + ": expected float32"):
            index.search_with(q.astype(np.float64), 5, 2, method=method)
        with pytest.raises(ValueError, match=name + r": expected shape \(n, 32\)"):
            index.search_with(np.zeros((2, 48), f32), 5, 2, method=method)
        with pytest.raises(ValueError, match=name + r": 65536 queries, at most 65535"):
            index.search_with(np.zeros((65536, 32), f32), 5, 2, method=method)
    for method in ("auto", "list", None, 0):
        with pytest.raises(ValueError, match=name + r": method = .*must be one of 'grouped', 'single'"):
            index.search_with(q, 5, 2, method=method)
        with pytest.raises(ValueError, match=r"neighbours: method = .*must be one of 'grouped', 'single'"):
            index.neighbours(5, 2, method=method)
    # the width's limit belongs to the grouped path alone
    at_1024, at_2048 = _host_index(1000, 10, 1024)[2], _host_index(1000, 10, 2048)[2]
    with pytest.raises(ValueError, match=r"search_with: k = 255 with method='grouped': rows of dim 1024 allow k <= 254 .*tfimm_hip_embed_search_wide_max_k"):
        at_1024.search_with(np.zeros((2, 1024), f32), 255, 2)
    with pytest.raises(ValueError, match=r"search_with: k = 1 with method='grouped': rows of dim 2048 allow no k .*tfimm_hip_embed_search_wide_max_k"):
        at_2048.search_with(np.zeros((2, 2048), f32), 1, 2)
    assert at_1024._method_args(254, 2, 0, "grouped", "x") == 1 and at_1024._method_args(256, 2, 3, "single", "x") == 3
    assert at_2048._method_args(256, 2, 0, "single", "x") == 1 and index._method_args(256, 10, 7, "grouped", "x") == 7

    name = "GalleryIndex.neighbours"
    with pytest.raises(ValueError, match=name + ": k must be an integer"):
        index.neighbours(5.0)
    with pytest.raises(ValueError, match=name + ": k = 0, must be at least 1"):
        index.neighbours(0)
    with pytest.raises(ValueError, match=name + r": k = 256 \(\+ 1 for the row itself\), must be in \[1, TFIMM_EMBED_WIDE_MAX_K = 256\]"):
        index.neighbours(256)
    with pytest.raises(ValueError, match=name + r": k = 254 \(\+ 1 for the row itself\) with method='grouped'.*tfimm_hip_embed_search_wide_max_k"):
        at_1024.neighbours(254, 2)
    with pytest.raises(ValueError, match=name + r": k = 1 \(\+ 1 for the row itself\) with method='grouped'.*allow no k"):
        at_2048.neighbours(1, 2)
    with pytest.raises(ValueError, match=name + r": nprobe = 11"):
        index.neighbours(5, 11)
    with pytest.raises(ValueError, match=name + r": nprobe = 0"):
        index.neighbours(5, 0)
    with pytest.raises(ValueError, match=name + ": batch must be an integer"):
        index.neighbours(5, 2, 64.0)
    for batch in (0, -1, 65536):
        with pytest.raises(ValueError, match=name + rf": batch = {batch}, must be in \[1, 65535\]"):
            index.neighbours(5, 2, batch)
    for ix in (index, at_1024, at_2048):
        assert not ix._work and not ix._gallery._work and not ix.centroids._work       # nothing was launched or allocated


# ---- the rule of neighbours ----------------------------------------------------------------------------------------------------------
def best_others(g, k):
    """per row the k best OTHER rows over the whole gallery: score descending, equal scores by ascending row"""
    s = er.scores64(g, g)
    idx = np.empty((len(g), k), np.int32)
    sc = np.empty((len(g), k), f32)
    for i in range(len(g)):
        order = [n for n in np.lexsort((np.arange(len(g)), -s[i])) if n != i][:k]
        idx[i], sc[i] = order, s[i][order].astype(f32)
    return idx, sc


@pytest.mark.parametrize("N, L, k", [(120, 1, 5), (300, 7, 20), (90, 16, 3)])
def test_neighbours_rule_on_duplicated_rows(N, L, k):
    """grid data with a run of k + 3 equal rows of the LARGEST norm in the gallery (each is its own and the others' best
    match): the later ones have more than k lower-numbered duplicates, are absent from their own k + 1 and drop the last"""
    rng = np.random.default_rng(N)
    g, cen = grid(N, (N, 32)), grid(N + 1, (L, 32))
    dup = np.sort(rng.choice(N, k + 3, replace=False))
    g[dup] = np.where(np.arange(32) % 2, 0.5, -0.5).astype(f32)             # |row|^2 = 8: above every score of another pair
    pairs = rng.choice(np.setdiff1d(np.arange(N), dup), 8, replace=False)
    g[pairs[4:]] = g[pairs[:4]]                                              # and a few plain pairs
    assignment = rng.integers(0, L, N)
    # every list probed: the k best other rows of the whole gallery, whatever the lists are
    idx, sc = nr.neighbours(g, cen, assignment, L, k)
    want = best_others(g, k)
    assert np.array_equal(idx, want[0]) and np.array_equal(er.bits(sc), er.bits(want[1]))
    assert not (idx == np.arange(N)[:, None]).any()                          # no row is its own neighbour
    full = ir.search_index(g, g, cen, assignment, L, k + 1)
    last, first = dup[-1], dup[0]
    assert last not in full[0][last] and full[0][last].tolist() == dup[:k + 1].tolist()        # absent: k + 1 lower duplicates
    assert idx[last].tolist() == dup[:k].tolist() and idx[dup[k + 1]].tolist() == dup[:k].tolist()
    assert full[0][first][0] == first and idx[first].tolist() == dup[1:k + 1].tolist()
    # fewer probes: every neighbour lies in a probed list, the row itself is gone, short results end in -1 / -inf
    if L > 1:
        nprobe = 2
        idx, sc = nr.neighbours(g, cen, assignment, nprobe, k)
        probes = er.search(g, cen, nprobe)[0]
        for i in range(N):
            found = idx[i][idx[i] >= 0]
            assert i not in found and set(assignment[found].tolist()) <= set(probes[i].tolist())
            assert (idx[i][len(found):] == -1).all() and np.isneginf(sc[i][len(found):]).all()
            others = np.flatnonzero(np.isin(assignment, probes[i]) & (np.arange(N) != i))
            assert len(found) == min(k, len(others))


def test_drop_self():
    idx = np.array([[3, 0, 5, -1], [1, 2, 3, 4], [7, 8, 2, -1], [-1, -1, -1, -1]], np.int32)
    sc = np.array([[4, 3, 2, -np.inf], [4, 3, 2, 1], [4, 3, 2, -np.inf], [-np.inf] * 4], f32)
    out_idx, out_sc = nr.drop_self(idx, sc, np.array([0, 9, 2, 3]))
    assert out_idx.tolist() == [[3, 5, -1], [1, 2, 3], [7, 8, -1], [-1, -1, -1]]
    assert out_sc[0].tolist() == [4, 2, -np.inf] and out_sc[1].tolist() == [4, 3, 2] and out_sc[2].tolist() == [4, 3, -np.inf]

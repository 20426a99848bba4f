"""The gallery search over inverted lists without a device: the written rule of tests/index_ref.py -- with every
list probed it is the exact search, a row in an unprobed list is absent, short results fill with -1 / -inf --, the refusals of
tfimm_hip_embed_search_lists before any launch, and the signatures and ``ValueError``s of ``Gallery.build_index`` /
``GalleryIndex`` / ``EmbeddingModel.search_index`` before any device work."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import coarse_ref as cr
import embed_ref as er
import index_ref as ir
import tfimm
from tfimm.engine import ffi

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
grid = cr.grid


# ---- the rule --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, L, k", [(40, 1, 5), (300, 7, 20), (1000, 37, 64), (700, 300, 200), (257, 16, 257)])
def test_probing_every_list_is_the_exact_search(N, L, k):
    """grid data: ties are frequent, and duplicated rows sit in different lists, so that equal scores are decided by the
    original row ACROSS lists"""
    rng = np.random.default_rng(N + L)
    q, g, cen = grid(N, (6, 32)), grid(N + 1, (N, 32)), grid(N + 2, (L, 32))
    assignment = rng.integers(0, L, N)
    dup = rng.choice(N, 12, replace=False)
    g[dup] = g[dup[0]]
    assignment[dup] = np.arange(12) % L
    idx, sc = ir.search_index(q, g, cen, assignment, L, k)
    want_idx, want_sc = er.search(q, g, k)
    assert np.array_equal(idx, want_idx) and np.array_equal(er.bits(sc), er.bits(want_sc))
    g_sorted, ids, offsets = ir.build_lists(g, assignment, L)
    assert sorted(ids.tolist()) == list(range(N)) and offsets[0] == 0 and offsets[-1] == N and (np.diff(offsets) >= 0).all()
    for l in range(L):
        part = ids[offsets[l]:offsets[l + 1]]
        assert (np.diff(part) > 0).all() and (assignment[part] == l).all()
    assert np.array_equal(g_sorted, g[ids])


def test_a_row_in_an_unprobed_list_is_absent():
    """the best row of the query equals the query, and its list's centroid is the NEGATED query: with one probe that list is
    the last to be looked at.  An implementation that ran the exact search would return the row."""
    q = grid(5, (1, 32))
    q[0, 0] = 0.5
    g = np.concatenate([q, q / 2, q / 4, -q])                  # row 0 is the query itself
    cen = np.concatenate([-q, q])
    assignment = np.array([0, 1, 1, 1])
    assert er.search(q, g, 1)[0].tolist() == [[0]]
    idx, sc = ir.search_index(q, g, cen, assignment, 1, 2)
    assert idx.tolist() == [[1, 2]] and 0 not in idx
    idx, _ = ir.search_index(q, g, cen, assignment, 2, 2)
    assert idx.tolist() == [[0, 1]]


def test_short_results_fill_with_none():
    q, g, cen = grid(1, (3, 16)), grid(2, (50, 16)), grid(3, (5, 16))
    assignment = np.arange(50) % 5
    g_sorted, ids, offsets = ir.build_lists(g, assignment, 5)
    probes = np.array([[0, 1], [2, -1], [-1, 5]])              # -1 and L: no list
    idx, sc = ir.search_lists(q, g_sorted, ids, offsets, probes, 25)
    assert (idx[0, :20] >= 0).all() and (idx[0, 20:] == -1).all() and np.isneginf(sc[0, 20:]).all()
    assert set(idx[0, :20].tolist()) == set(range(0, 50, 5)) | set(range(1, 50, 5))
    assert (idx[1, :10] % 5 == 2).all() and (idx[1, 10:] == -1).all() and np.isneginf(sc[1, 10:]).all() and np.isfinite(sc[1, :10]).all()
    assert (idx[2] == -1).all() and np.isneginf(sc[2]).all()
    want = er.search(q[:1], g[np.isin(assignment, (0, 1))], 20)
    assert np.array_equal(er.bits(sc[0, :20]), er.bits(want[1][0]))


def test_a_repeated_list_counts_once():
    q, g = grid(1, (2, 16)), grid(2, (50, 16))
    g_sorted, ids, offsets = ir.build_lists(g, np.arange(50) % 5, 5)
    once = ir.search_lists(q, g_sorted, ids, offsets, np.array([[3, 1, -1, -1], [2, -1, -1, -1]]), 25)
    again = ir.search_lists(q, g_sorted, ids, offsets, np.array([[3, 1, 3, 1], [2, 2, 2, 2]]), 25)
    assert np.array_equal(once[0], again[0]) and np.array_equal(er.bits(once[1]), er.bits(again[1]))
    for row in again[0]:
        found = row[row >= 0]
        assert len(set(found.tolist())) == len(found) and (row[len(found):] == -1).all()      # no row twice, no hole in front


# ---- the C entry points -------------------------------------------------------------------------------------------------------------
def _aligned(nbytes, align=64):
    raw = np.zeros(nbytes + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + nbytes]


def _lists(q=True, ld_q=32, B=2, g=True, ld_g=32, N=100, E=32, ids=True, offsets=True, L=4, probes=True, ld_p=2, nprobe=2, k=5, parts=0,
           scores=True, indices=True, workspace=True, workspace_bytes=1 << 16, g_off=0, i_off=0, o_off=0, p_off=0):
    bufs = [_aligned(1 << 16) for _ in range(8)]
    on = (q, g, ids, offsets, probes, scores, indices, workspace)
    off = (0, g_off, i_off, o_off, p_off, 0, 0, 0)
    p = [C.c_void_p(b.ctypes.data + o) if f else None for b, f, o in zip(bufs, on, off)]
    rc = ffi.lib.tfimm_hip_embed_search_lists(p[0], ld_q, B, p[1], ld_g, N, E, p[2], p[3], L, p[4], ld_p, nprobe, k, parts, p[5], p[6],
                                              p[7], workspace_bytes, None)
    return rc, ffi.lib.tfimm_hip_last_error().decode()


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
    (dict(workspace_bytes=8), "workspace_bytes=8"), (dict(parts=3, workspace_bytes=2 * 2 * 3 * 5 * 8 - 1), "asks for 480"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_lists_search_refusals_name_the_argument(kw, names):
    rc, msg = _lists(**kw)
    assert rc == -1 and msg.startswith("embed_search_lists:") and names in msg, (rc, msg)


def test_the_empty_call_workspace_and_constants():
    assert _lists(B=0)[0] == 0                                              # no queries: returns before any launch
    assert _lists(B=0, k=0)[0] == -1                                        # but not before the checks
    ws = ffi.lib.tfimm_hip_embed_search_lists_workspace
    for B, nprobe, k, parts in ((3, 2, 5, 1), (70, 37, 200, 7), (1, 256, 256, 64), (65535, 8, 20, 3)):
        assert ws(B, 5000, 64, 300, nprobe, k, parts) == B * nprobe * parts * k * 8      # k pairs per (query, slot, part)
    assert ws(3, 5000, 64, 300, 2, 5, 0) == ws(3, 5000, 64, 300, 2, 5, 1)   # parts = 0: the library chooses 1
    assert ws(0, 100, 32, 4, 2, 5, 0) == ws(1, 100, 32, 4, 2, 5, 0) > 0
    assert ws(1, 100, 32, 4, 2, 200, 0) > 0                                 # k may exceed N
    for args, names in (((1, 100, 24, 4, 2, 5, 0), "E=24"), ((1, 100, 32, 4, 2, 257, 0), "k=257"), ((1, 100, 32, 4, 257, 5, 0), "nprobe=257"),
                        ((1, 100, 32, 0, 2, 5, 0), "L=0"), ((1, 100, 32, 4, 2, 5, 65), "parts=65"), ((65536, 100, 32, 4, 2, 5, 0), "B=65536"),
                        ((1, 0, 32, 4, 2, 5, 0), "N=0")):
        assert ws(*args) == -1 and names in ffi.lib.tfimm_hip_last_error().decode(), args
    hdr = open(os.path.join(ROOT, "include", "tfimm_hip.h")).read()
    assert int(re.search(r"#define TFIMM_EMBED_LISTS_MAX_PROBE (\d+)", hdr).group(1)) == ffi.EMBED_LISTS_MAX_PROBE == 256
    assert (ffi.EMBED_LISTS_MAX_PARTS, ffi.EMBED_LISTS_MAX_B) == (64, 65535)
    for name in ("tfimm_hip_embed_search_lists", "tfimm_hip_embed_search_lists_workspace"):
        assert f" {name}(" in hdr and hasattr(ffi.lib, name)
    assert ffi.lib.tfimm_hip_abi_version() == 4                             # the change is additive
    assert int(re.search(r"#define TFIMM_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 4


# ---- Gallery.build_index / GalleryIndex before any device work ------------------------------------------------------------------------
def test_signatures():
    sig = inspect.signature(tfimm.Gallery.build_index).parameters
    assert list(sig) == ["self", "n_lists", "iters", "init", "seed", "clusters"]
    assert [sig[n].default for n in list(sig)[1:]] == [None, 10, None, 0, None]
    sig = inspect.signature(tfimm.GalleryIndex.search).parameters
    assert list(sig) == ["self", "q", "k", "nprobe", "parts"] and [sig[n].default for n in ("k", "nprobe", "parts")] == [5, 8, 0]
    sig = inspect.signature(tfimm.GalleryIndex.probe).parameters
    assert list(sig) == ["self", "q", "nprobe"] and sig["nprobe"].default == 8
    sig = inspect.signature(tfimm.GalleryIndex.classify).parameters
    assert list(sig) == ["self", "q", "k", "nprobe", "temperature", "top", "reduce", "exclude"]
    assert [sig[n].default for n in list(sig)[2:]] == [20, 8, 0.07, 5, "sum", None]
    sig = inspect.signature(tfimm.EmbeddingModel.search_index).parameters
    assert list(sig) == ["self", "x", "index", "k", "nprobe"] and (sig["k"].default, sig["nprobe"].default) == (5, 8)
    assert isinstance(tfimm.GalleryIndex.stale, property)
    assert "index" not in tfimm.models.gallery._METHODS                     # "auto" never takes the index
    assert tfimm.models.GalleryIndex is tfimm.GalleryIndex


@pytest.fixture
def hostless(monkeypatch):
    """``Gallery._store`` replaced by the bookkeeping alone (tests/test_search_wide.py): nothing is uploaded"""
    def store(self, t, up_labels, n):
        self._labelled = self._labelled or up_labels is not None
        first, self._n = self._n, self._n + n
        return range(first, self._n)
    monkeypatch.setattr(tfimm.Gallery, "_store", store)


def _gallery(n, dim=32, labels=True):
    g = tfimm.Gallery(dim)
    g.add(np.zeros((n, dim), f32), np.arange(n) % 7 if labels else None)
    return g


def _host_index(n=1000, L=10, dim=32, labels=True):
    """an index whose plumbing ran in ``torch`` on the host: the rows, the centroids and the assignment are host tensors, so
    everything up to the first launch can be looked at without a device"""
    g = _gallery(n, dim, labels)
    g._buf = torch.zeros((n, g.pitch), dtype=torch.bfloat16)
    g._buf[:, 0] = torch.arange(n) % 128                                    # exact in bf16: a row knows where it came from
    if labels:
        g._lab = (torch.arange(n) % 7).to(torch.int32)
    assignment = torch.from_numpy(((np.arange(n) * 7) % L).astype(np.int32))
    cen = tfimm.Gallery._of_rows(dim, torch.zeros((L, dim)), torch.arange(L, dtype=torch.int32))
    counts = torch.bincount(assignment.long(), minlength=L).to(torch.int32)
    clusters = tfimm.Clusters(cen, tfimm.models.model.Tensor(assignment), None, tfimm.models.model.Tensor(counts), None)
    return g, clusters, g.build_index(clusters=clusters)


def test_build_index_value_errors_come_before_device_work(hostless):
    with pytest.raises(ValueError, match="build_index: the gallery is empty"):
        tfimm.Gallery(32).build_index()
    g = _gallery(1000)
    with pytest.raises(ValueError, match="n_clusters = 0"):
        g.build_index(0)
    with pytest.raises(ValueError, match="n_clusters = 1001"):
        g.build_index(1001)
    with pytest.raises(ValueError, match="iters = -1"):
        g.build_index(iters=-1)
    with pytest.raises(ValueError, match="clusters must be the Clusters of gallery.kmeans"):
        g.build_index(clusters=(1, 2))
    g, clusters, index = _host_index()
    with pytest.raises(ValueError, match="n_lists = 11 with clusters of 10 centroids"):
        g.build_index(11, clusters=clusters)
    with pytest.raises(ValueError, match="clusters of dim 32, this gallery holds rows of 48"):
        _gallery(1000, 48).build_index(clusters=clusters)
    with pytest.raises(ValueError, match=r"clusters assign \(1000,\) rows, the gallery holds 900"):
        _gallery(900).build_index(clusters=clusters)
    # n_lists=None: round(sqrt(len)), clamped to [1, TFIMM_CLUSTER_MAX_C]
    from tfimm.models.gallery_index import _plan_index
    assert [_plan_index(_gallery(n), None, 10, None, 0, None) for n in (1, 2, 3, 1000, 1_000_000)] == [1, 1, 2, 32, 1000]
    big = _gallery(10)
    big._n = 2 ** 31 - 1
    assert _plan_index(big, None, 10, None, 0, None) == 46341 and ffi.CLUSTER_MAX_C == 65536


def test_the_index_is_a_partition_and_a_snapshot(hostless):
    g, clusters, index = _host_index(1000, 10)
    assert (index.size, index.n_lists, index.dim, index.stale, index.centroids) == (1000, 10, 32, False, clusters.centroids)
    ids, offsets = index.lists()
    assert ids.dtype == offsets.dtype == np.int32 and sorted(ids.tolist()) == list(range(1000))
    assert offsets.tolist() == list(range(0, 1001, 100)) and index.counts.numpy().tolist() == [100] * 10
    for l in range(10):
        part = ids[offsets[l]:offsets[l + 1]]
        assert (np.diff(part) > 0).all() and ((part * 7) % 10 == l).all()
    assert np.array_equal(index._rows[:, 0].float().numpy(), ids % 128)     # the index owns the rows in list order
    assert index.longest == 100 and index.parts == 1
    g.add(np.zeros((5, 32), f32), np.zeros(5, np.int64))
    assert index.stale and index.size == 1000 and len(g) == 1005
    # parts: about 2048 rows of the longest list per workgroup, at most 64
    one = torch.zeros(300_000, dtype=torch.int32)
    one[:5000] = 1
    for n, want in ((2048, 1), (2049, 2), (5000, 3), (300_000, 64)):
        gg = _gallery(n)
        gg._buf = torch.zeros((n, 32), dtype=torch.bfloat16)
        cen = tfimm.Gallery._of_rows(32, torch.zeros((2, 32)), torch.arange(2, dtype=torch.int32))
        a = tfimm.models.model.Tensor(one[:n] * 0 if n != 300_000 else 1 - one)
        idx = gg.build_index(clusters=tfimm.Clusters(cen, a, None, None, None))
        assert idx.parts == want and idx.longest == (n if n != 300_000 else 295_000), n


def test_search_value_errors_come_before_device_work(hostless):
    g, _, index = _host_index(1000, 10)
    q = np.zeros((2, 32), f32)
    for call in (index.search, index.classify):
        name = "GalleryIndex." + call.__name__
        with pytest.raises(ValueError, match=name + r": k = 0, must be in \[1"):
            call(q, 0)
        with pytest.raises(ValueError, match=name + ": k must be an integer"):
            call(q, 5.0)
        with pytest.raises(ValueError, match=name + r": nprobe = 11, must be in \[1, min\(n_lists = 10, TFIMM_EMBED_LISTS_MAX_PROBE = 256\)\]"):
            call(q, 5, 11)
        with pytest.raises(ValueError, match=name + r": nprobe = 0"):
            call(q, 5, 0)
        with pytest.raises(ValueError, match=name + ": nprobe must be an integer"):
            call(q, 5, 2.0)
        with pytest.raises(ValueError, match=name + ": expected float32"):
            call(q.astype(np.float64), 5, 2)
        with pytest.raises(ValueError, match=name + r": expected shape \(n, 32\)"):
            call(np.zeros((2, 48), f32), 5, 2)
    with pytest.raises(ValueError, match=r"search: k = 257, must be in \[1, TFIMM_EMBED_WIDE_MAX_K = 256\]"):
        index.search(q, 257)
    with pytest.raises(ValueError, match=r"search: parts = 65"):
        index.search(q, 5, 2, parts=65)
    with pytest.raises(ValueError, match=r"search: parts = -1"):
        index.search(q, 5, 2, parts=-1)
    with pytest.raises(ValueError, match=r"search: 65536 queries, at most 65535"):
        index.search(np.zeros((65536, 32), f32), 5, 2)
    with pytest.raises(ValueError, match=r"probe: nprobe = 11"):
        index.probe(q, 11)
    with pytest.raises(ValueError, match=r"classify: k = 65, must be in \[1, TFIMM_KNN_MAX_K = 64\]"):
        index.classify(q, 65)
    with pytest.raises(ValueError, match=r"classify: k = 64 \(\+ 1 for the excluded row\)"):
        index.classify(q, 64, exclude=[0, 1])
    with pytest.raises(ValueError, match="classify: top = 0"):
        index.classify(q, 5, 2, top=0)
    with pytest.raises(ValueError, match="classify: temperature = 0"):
        index.classify(q, 5, 2, temperature=0)
    with pytest.raises(ValueError, match="classify: reduce = 'mean'"):
        index.classify(q, 5, 2, reduce="mean")
    with pytest.raises(ValueError, match="classify: this gallery has no labels"):
        _host_index(100, 4, labels=False)[2].classify(q, 5, 2)
    # a probe is a search of the centroids: at dim 2048 they allow no more than 64 neighbours
    wide = _host_index(1000, 100, 2048)[2]
    with pytest.raises(ValueError, match=r"search: nprobe = 65: the probe is centroids.search"):
        wide.search(np.zeros((2, 2048), f32), 5, 65)
    assert wide._args(5, 64) == 1
    assert index._args(256, 10) == 1 and index._args(5, 1, 7) == 7
    assert not index._work and not g._work and not index.centroids._work     # nothing was launched or allocated
    # and the model's front door checks before its forward pass
    class Model:
        name, embed_dim = "m", 32

        def _embeddings_for(self, x, index):
            raise AssertionError("the forward pass ran")
    with pytest.raises(ValueError, match="m: embeddings have 32 columns, the index holds rows of 2048"):
        tfimm.EmbeddingModel.search_index(Model(), None, wide)
    with pytest.raises(ValueError, match="nprobe = 11"):
        tfimm.EmbeddingModel.search_index(Model(), None, index, 5, 11)

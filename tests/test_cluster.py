"""The cluster end without a GPU: the written rules (tests/cluster_ref.py) on cases answered by hand, the refusals of
tfimm_hip_cluster_assign / tfimm_hip_segment_mean (include/tfimm_hip.h), and the ``ValueError`` cases of ``Gallery.assign`` /
``prototypes`` / ``kmeans`` / ``set_labels`` -- all of them raised before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cluster_ref as cr
import embed_ref as er
import tfimm
from tfimm.engine import ffi

f32, i32 = np.float32, np.int32


def rows2(*pairs, E=16):
    """rows of E columns whose first two are given, the rest zero"""
    x = np.zeros((len(pairs), E), f32)
    x[:, :2] = pairs
    return x


# ---- the rules ---------------------------------------------------------------------------------------------------------
def test_assign_by_hand_a_tie_between_equal_centroids_goes_to_the_lower():
    g = rows2((1, 0), (0, 1), (0.5, 0.5), (0, 0), (-1, -1))
    c = rows2((0, 1), (1, 0), (1, 0), (0, 1))                          # 0 == 3 and 1 == 2
    a, s = cr.assign(g, c)
    assert a.tolist() == [1, 0, 0, 0, 0] and s.tolist() == [1, 1, 0.5, 0, -1] and a.dtype == i32 and s.dtype == f32
    # -0.0 == +0.0: a score of -0.0 ahead of a +0.0 keeps its place
    a, s = cr.assign(rows2((1, 0)), rows2((-0.0, 0), (0.0, 0), (0.0, 1)))
    assert a.tolist() == [0]
    # a centroid's score does not depend on the other centroids, a row's not on the other rows
    a2, s2 = cr.assign(g[2:4], c[:3])
    assert a2.tolist() == [0, 0] and s2.tolist() == [0.5, 0]


def test_segment_mean_by_hand_empty_segments_entries_outside_and_the_order_of_the_runs():
    g = rows2((1, 2), (3, 4), (5, 6), (-8, 0))
    rows = [0, 1, 2, -1, 4, 7, 3, 3, 1]
    mean, counts = cr.segment_mean(g, rows, [0, 3, 3, 6, 9])
    # segment 1 is empty; segment 2 holds only entries outside [0, 4): not counted; a row may appear twice
    assert counts.tolist() == [3, 0, 0, 3] and mean.dtype == f32 and counts.dtype == i32
    assert mean[:, :2].tolist() == [[3, 4], [0, 0], [0, 0], [f32(-13) / f32(3), f32(4) / f32(3)]]
    assert not er.bits(mean[1:3]).any()                                  # +0.0
    # offsets are clamped to [0, M]; an end below its begin is an empty segment
    mean, counts = cr.segment_mean(g, rows, [-5, 2, 1, 100])
    assert counts.tolist() == [2, 0, 5] and mean[0, :2].tolist() == [2, 3]
    # the order: runs counted from the segment's begin, each summed from +0.0, then added in ascending run order.  In one run
    # 2^24 swallows every 1 that follows it; cut into runs of 2, the last two ones are added to each other first and survive
    big = rows2((2.0 ** 24, 0), (1, 0), (1, 0))
    seq = cr.segment_mean(big, [0, 1, 2], [0, 3], run=4)[0][0, 0]       # (2^24 + 1) + 1 = 2^24
    cut = cr.segment_mean(big, [0, 1, 2, 2], [0, 4], run=2)[0][0, 0]    # (2^24 + 1) + (1 + 1) = 2^24 + 2, / 4
    assert seq == f32(2.0 ** 24) / f32(3) and cut == f32(2.0 ** 24 + 2) / f32(4)
    # the runs are the segment's own: the same entries behind another segment give the same bits
    a = cr.segment_mean(big, [0, 1, 2, 2], [0, 4], run=2)[0]
    b = cr.segment_mean(big, [1, 0, 1, 2, 2], [0, 1, 5], run=2)[0]
    assert np.array_equal(er.bits(a[0]), er.bits(b[1]))
    assert cr.RUN == ffi.SEGMENT_RUN == 256


SIX = rows2((1, 0), (1, 0), (0, 1), (0, 1), (0, 1), (0.5, 0.25))


def test_kmeans_by_hand_moved_on_six_rows_and_an_empty_cluster_keeps_its_centroid():
    # centroids from rows 0 and 5.  Pass 0: row 5 scores 0.5 against (1, 0) and 0.559 against its own direction, the (0, 1)
    # rows 0 and 0.447: [0 0 1 1 1 1].  Update: c1 = (0.125, 0.8125) normalised = (0.152, 0.988): row 5 now scores 0.323
    # there and 0.5 at c0 and moves; nothing else does.  Update: c0 = (5/6, 1/12) normalised, c1 = (0, 1): nothing moves.
    cen, a, s, n, moved = cr.kmeans(SIX, SIX[[0, 5]], 2)
    assert moved.tolist() == [1, 0] and a.tolist() == [0, 0, 1, 1, 1, 0] and n.tolist() == [3, 3]
    assert cen[1, :2].tolist() == [0, 1] and np.array_equal(cen, er.bf16_round(cen))
    assert abs(float(cen[0, 0]) - (5 / 6) / np.hypot(5 / 6, 1 / 12)) < 2.0 ** -8
    assert cr.kmeans(SIX, SIX[[0, 5]], 0)[1].tolist() == [0, 0, 1, 1, 1, 1]             # iters = 0 only assigns
    # a third centroid at (-1, 0) wins no row at any pass: it stays what it was, bit for bit, and counts 0
    init = np.concatenate([SIX[[0, 5]], rows2((-1, 0))])
    cen3, a3, _, n3, moved3 = cr.kmeans(SIX, init, 2)
    assert n3.tolist() == [3, 3, 0] and a3.tolist() == a.tolist() and moved3.tolist() == [1, 0]
    assert cen3[2, :2].tolist() == [-1, 0] and np.array_equal(er.bits(cen3[:2]), er.bits(cen))


def test_prototypes_by_hand_and_the_csr_form():
    labels = [1, 1, -1, 3, 3, 7]
    rows, offsets = cr.csr(labels, 5)
    assert rows.tolist() == [2, 0, 1, 3, 4, 5] and offsets.tolist() == [1, 1, 3, 3, 5, 5]      # -1 in front, 7 behind
    p, lab = cr.prototypes(SIX, labels, 5, normalize=False)
    assert lab.tolist() == [-1, 1, -1, 3, -1] and p[:, :2].tolist() == [[0, 0], [1, 0], [0, 0], [0, 1], [0, 0]]
    p, lab = cr.prototypes(SIX, [0, 0, 0, 0, 0, 0], 1)
    want = np.array([2.5 / 6, 3.25 / 6]) / np.hypot(2.5 / 6, 3.25 / 6)
    assert lab.tolist() == [0] and np.abs(p[0, :2] - want).max() < 2.0 ** -8 and np.array_equal(p, er.bf16_round(p))


def test_the_float32_normaliser_of_the_device_agrees_with_the_float64_one_to_rounding():
    x = np.random.default_rng(1).standard_normal((50, 80)).astype(f32)
    a, b = cr.l2_normalize_f32(x), er.l2_normalize(x)
    assert a.dtype == f32 and np.abs(a - b).max() <= 4 * 2.0 ** -24 * np.abs(b).max()


# ---- refusals: before any launch, so no GPU is involved ------------------------------------------------------------------
ASSIGN_ARGS = ("g", "c", "assign", "score")
SEGMENT_ARGS = ("g", "rows", "offsets", "mean", "counts", "workspace")


def _ptrs(names, null, off):
    bufs = {n: np.zeros(4096, np.int64) for n in names}
    base = {n: (bufs[n].ctypes.data + 15) // 16 * 16 for n in names}
    return {n: None if n in null else C.c_void_p(base[n] + (off or {}).get(n, 0)) for n in names}, bufs


def _assign(ld_g=32, N=10, ld_c=32, Cn=4, E=32, null=(), off=None):
    """tfimm_hip_cluster_assign over host buffers (a refusal never touches them)"""
    p, keep = _ptrs(ASSIGN_ARGS, null, off)
    rc = ffi.lib.tfimm_hip_cluster_assign(p["g"], ld_g, N, p["c"], ld_c, Cn, E, p["assign"], p["score"], None)
    return rc, ffi.lib.tfimm_hip_last_error().decode()


def _segment(ld_g=32, N=10, E=32, M=20, Cn=4, ld_m=32, ws=None, null=(), off=None):
    p, keep = _ptrs(SEGMENT_ARGS, null, off)
    if ws is None:
        ws = 1 << 40
    rc = ffi.lib.tfimm_hip_segment_mean(p["g"], ld_g, N, E, p["rows"], M, p["offsets"], Cn, p["mean"], ld_m, p["counts"],
                                        p["workspace"], ws, None)
    return rc, ffi.lib.tfimm_hip_last_error().decode()


@pytest.mark.parametrize("kw, names", [
    (dict(null=("g",)), "g is null"), (dict(null=("c",)), "c is null"), (dict(null=("assign",)), "assign is null"),
    (dict(null=("score",)), "score is null"), (dict(off={"g": 8}), "16-byte"), (dict(off={"c": 4}), "16-byte"),
    (dict(off={"assign": 2}), "4-byte"), (dict(off={"score": 1}), "4-byte"),
    (dict(E=0), "E=0"), (dict(E=8, ld_g=8, ld_c=8), "E=8"), (dict(E=24), "E=24"), (dict(E=2064, ld_g=2064, ld_c=2064), "E=2064"),
    (dict(Cn=0), "C=0"), (dict(Cn=-2), "C=-2"), (dict(Cn=65537), "C=65537"), (dict(N=-1), "N=-1"),
    (dict(ld_g=24), "ld_g=24"), (dict(ld_g=36), "ld_g=36"), (dict(ld_c=16), "ld_c=16"), (dict(ld_c=33), "ld_c=33"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_assign_refusals_return_minus_one_and_name_the_argument(kw, names):
    rc, msg = _assign(**kw)
    assert rc == -1 and msg.startswith("cluster_assign:") and names in msg, (rc, msg)


@pytest.mark.parametrize("kw, names", [
    (dict(null=("g",)), "g is null"), (dict(null=("rows",)), "rows is null"), (dict(null=("offsets",)), "offsets is null"),
    (dict(null=("mean",)), "mean is null"), (dict(null=("counts",)), "counts is null"), (dict(null=("workspace",)), "workspace is null"),
    (dict(off={"g": 8}), "16-byte"), (dict(off={"workspace": 8}), "16-byte"), (dict(off={"rows": 2}), "4-byte"),
    (dict(off={"offsets": 1}), "4-byte"), (dict(off={"mean": 2}), "4-byte"), (dict(off={"counts": 3}), "4-byte"),
    (dict(E=0), "E=0"), (dict(E=40), "E=40"), (dict(E=4096, ld_g=4096, ld_m=4096), "E=4096"),
    (dict(Cn=0), "C=0"), (dict(Cn=-1), "C=-1"), (dict(M=-1), "M=-1"), (dict(N=-1), "N=-1"),
    (dict(ld_g=16), "ld_g=16"), (dict(ld_g=44), "ld_g=44"), (dict(ld_m=31), "ld_m=31"),
    (dict(ws=0), "workspace_bytes=0"), (dict(ws=(20 // 256 + 4) * (32 * 4 + 4) - 1), "workspace_bytes="),
], ids=lambda v: v if isinstance(v, str) else None)
def test_segment_mean_refusals_return_minus_one_and_name_the_argument(kw, names):
    rc, msg = _segment(**kw)
    assert rc == -1 and msg.startswith("segment_mean:") and names in msg, (rc, msg)


def test_constants_agree_the_workspace_and_an_empty_gallery_is_no_launch():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfimm_hip.h")).read()
    assert int(re.search(r"#define TFIMM_CLUSTER_MAX_C (\d+)", hdr).group(1)) == ffi.CLUSTER_MAX_C == 65536
    assert int(re.search(r"#define TFIMM_SEGMENT_RUN (\d+)", hdr).group(1)) == ffi.SEGMENT_RUN == cr.RUN
    assert "CLUSTER END" in hdr and ffi.lib.tfimm_hip_abi_version() == 4
    # N == 0 returns before any launch, at the limits of every argument
    assert _assign(N=0)[0] == 0 and _assign(N=0, Cn=65536, E=2048, ld_g=2048, ld_c=1 << 40)[0] == 0
    assert _assign(N=0, Cn=1, E=16, ld_g=16, ld_c=16)[0] == 0
    # the workspace: a slot of E sums and one count per possible run, M / R + C of them, in whole 16 bytes
    ws = ffi.lib.tfimm_hip_segment_mean_workspace
    for M, Cn, E in ((0, 1, 16), (255, 1, 16), (256, 3, 48), (10 ** 6, 1024, 512), (2 ** 31 - 1, 2 ** 31 - 1, 2048)):
        slots = M // cr.RUN + Cn
        assert ws(M, Cn, E) == (slots * (E * 4 + 4) + 15) // 16 * 16, (M, Cn, E)
    for bad, name in (((-1, 1, 16), "M=-1"), ((0, 0, 16), "C=0"), ((0, 1, 24), "E=24")):
        assert ws(*bad) == -1 and name in ffi.lib.tfimm_hip_last_error().decode()


# ---- Python: what is refused, before any device work ---------------------------------------------------------------------
@pytest.fixture
def hostless(monkeypatch):
    """``Gallery._store`` replaced by the bookkeeping alone (tests/test_knn.py): nothing is uploaded"""
    def store(self, t, up_labels, n):
        self._labelled = self._labelled or up_labels is not None
        first, self._n = self._n, self._n + n
        return range(first, self._n)
    monkeypatch.setattr(tfimm.Gallery, "_store", store)


def _gallery(n=100, labelled=True, dim=32):
    g = tfimm.Gallery(dim)
    if n:
        g.add(np.zeros((n, dim), f32), np.arange(n) % 7 if labelled else None)
    return g


def test_the_new_names_and_signatures():
    import inspect
    assert tfimm.Assigned._fields == ("clusters", "scores")
    assert tfimm.Clusters._fields == ("centroids", "assignment", "scores", "counts", "moved")
    sig = inspect.signature(tfimm.Gallery.kmeans).parameters
    assert list(sig) == ["self", "n_clusters", "iters", "init", "seed"]
    assert (sig["iters"].default, sig["init"].default, sig["seed"].default) == (10, None, 0)
    sig = inspect.signature(tfimm.Gallery.prototypes).parameters
    assert (sig["nb_classes"].default, sig["normalize"].default) == (None, True)
    assert list(inspect.signature(tfimm.Gallery.assign).parameters) == ["self", "centroids"]
    assert list(inspect.signature(tfimm.Gallery.set_labels).parameters) == ["self", "labels"]


def test_kmeans_value_errors_need_no_device(hostless):
    g = _gallery(100, labelled=False)
    for n in (0, -1, 101, 2.5, True, None, "8"):
        with pytest.raises(ValueError, match="n_clusters"):
            g.kmeans(n)
    big = _gallery(70000, labelled=False)
    with pytest.raises(ValueError, match="n_clusters = 65537"):
        big.kmeans(65537)
    for it in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="iters"):
            g.kmeans(4, iters=it)
    with pytest.raises(ValueError, match="empty"):
        _gallery(0).kmeans(1)
    import torch
    for bad in (np.zeros((4, 32), np.float64), np.zeros((4, 32), np.float16), np.zeros(4, bool), torch.zeros((4, 32), dtype=torch.float64),
                np.zeros((3, 32), f32), np.zeros((4, 16), f32), np.zeros(4 * 32, f32), tfimm.Tensor(torch.zeros((5, 32))),
                [0, 1, 2], [[0, 1, 2, 3]], [0, 1, 2, 2], [0, 1, 2, 100], [0, 1, 2, -1], np.array([3, 3, 3, 3], np.uint8),
                torch.tensor([0, 1, 100, 2]), _gallery(4, dim=48), _gallery(5), _gallery(0)):
        with pytest.raises(ValueError, match="init"):
            g.kmeans(4, init=bad)
    assert not g._work and g._buf is None                                       # nothing touched a device


def test_assign_prototypes_and_set_labels_value_errors_need_no_device(hostless):
    g = _gallery(100)
    for bad in (_gallery(5, dim=48), _gallery(0), None, np.zeros((4, 32), f32)):
        with pytest.raises(ValueError, match="centroids"):
            g.assign(bad)
    with pytest.raises(ValueError, match="centroids"):
        _gallery(70000).assign(_gallery(65537))
    with pytest.raises(ValueError, match="empty"):
        _gallery(0).assign(_gallery(5))
    with pytest.raises(ValueError, match="no labels"):
        _gallery(100, labelled=False).prototypes(7)
    for n in (0, -3, 2.5, True, 2 ** 31):
        with pytest.raises(ValueError, match="nb_classes"):
            g.prototypes(n)
    empty = tfimm.Gallery(32)
    empty.set_labels(np.zeros(0, np.int64))                                                         # labelled, and still empty
    assert empty.labelled
    with pytest.raises(ValueError, match="empty"):
        empty.prototypes(3)
    # set_labels: one label per row, in the forms add takes
    for bad in ([0] * 99, [0] * 101, np.zeros((100, 1), np.int64), 7):
        with pytest.raises(ValueError, match="labels"):
            g.set_labels(bad)
    for bad in ([0.0] * 100, np.zeros(100, f32), np.zeros(100, bool)):
        with pytest.raises(ValueError, match="labels"):
            g.set_labels(bad)
    with pytest.raises(ValueError, match=r"\[0, 2\^31 - 1\] or -1"):
        g.set_labels([0] * 99 + [-2])
    u = _gallery(10, labelled=False)
    with pytest.raises(ValueError, match="labels"):
        u.set_labels([0] * 9)
    assert not u.labelled                                                        # a refused set_labels decides nothing
    # add's rules are what they were
    with pytest.raises(ValueError, match="holds 10 rows without"):
        u.add(np.zeros((2, 32), f32), [0, 1])
    with pytest.raises(ValueError, match="100 rows need|rows need"):
        g.add(np.zeros((2, 32), f32))

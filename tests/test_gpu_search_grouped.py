"""pytest -m gpu: the grouped gallery search over inverted lists (tfimm_hip_embed_search_lists_grouped,
csrc/embed_lists_grouped.hip; ``GalleryIndex.search_with`` / ``neighbours``) against the written rule of
tests/index_ref.py and against tfimm_hip_embed_search_lists, bit for bit: a covering set of widths, list shapes, probes, k and
parts on exact data; the edges of a tile on the query side; a list that forces prune after prune in two tiles; odd probes;
independence of parts, batch, order, repetition and replay; and ``GalleryIndex`` end to end with the kNN graph of its rows
(tests/neighbours_ref.py).  Every launch of the C entry runs over buffers with guards behind outputs and workspace and NaN in
the padding columns of q and g.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import coarse_ref as cr
import embed_ref as er
import index_ref as ir
import neighbours_ref as nr
from test_gpu_search_index import CENTRES, GUARD, Lists, clustered_grid, cycling_probes, hand_made, same, the_index
from tfimm.engine import ffi

pytestmark = pytest.mark.gpu
f32 = np.float32
grid = cr.grid


def grouped(d, probes, k, parts=0, rows=None, sync=True, ld_extra=3):
    """tfimm_hip_embed_search_lists_grouped over the uploaded index ``d`` (a ``Lists``), as ``Lists.search`` runs the single
    entry: ``probes`` (B, nprobe) stored at pitch nprobe + ld_extra (the columns behind hold list 0: reading them would change
    the result), guards behind outputs and workspace -> (indices, scores) as numpy arrays, or the device buffers if not ``sync``"""
    lo, hi = (0, d.B) if rows is None else rows
    B, nprobe = hi - lo, probes.shape[1]
    ld_p = nprobe + ld_extra
    hp = np.zeros((B, ld_p), np.int32)
    hp[:, :nprobe] = probes[lo:hi]
    dp = d._probes.get(hp.tobytes() + bytes([ld_extra]))
    if dp is None:
        dp = d._probes[hp.tobytes() + bytes([ld_extra])] = torch.from_numpy(hp).cuda()
    need = ffi.lib.tfimm_hip_embed_search_lists_grouped_workspace(B, d.N, d.E, d.L, nprobe, k, parts)
    assert need > 0, ffi.lib.tfimm_hip_last_error().decode()
    work = torch.empty(need + 4 * GUARD, dtype=torch.uint8, device="cuda")
    work[need:] = 0x5a
    scores = torch.full((B * k + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    indices = torch.full((B * k + GUARD,), -7, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ffi.check(ffi.lib.tfimm_hip_embed_search_lists_grouped(d.q.data_ptr() + 4 * lo * d.ld_q, d.ld_q, B, d.g.data_ptr(), d.ld_g, d.N, d.E,
                                                           d.ids.data_ptr(), d.offsets.data_ptr(), d.L, dp.data_ptr(), ld_p, nprobe, k,
                                                           parts, scores.data_ptr(), indices.data_ptr(), work.data_ptr(), need, st),
              "tfimm_hip_embed_search_lists_grouped")
    if not sync:
        return indices, scores, (work, dp)
    torch.cuda.synchronize()
    i, s = indices.cpu().numpy(), scores.cpu().numpy()
    assert (i[B * k:] == -7).all() and (s[B * k:] == -7).all() and (work[need:] == 0x5a).all(), "a launch wrote behind a buffer"
    return i[:B * k].reshape(B, k), s[:B * k].reshape(B, k)


def check(d, probes, k, parts=0, **kw):
    idx, sc = grouped(d, probes, k, parts, **kw)
    lo, hi = kw.get("rows") or (0, d.B)
    want_idx, want_sc = ir.search_lists(d.host[0][lo:hi], *d.host[1:], probes[lo:hi], k)
    assert np.array_equal(idx, want_idx), (np.argwhere(idx != want_idx)[:8], idx[idx != want_idx][:8], want_idx[idx != want_idx][:8])
    assert np.array_equal(er.bits(sc), er.bits(want_sc))
    return idx, sc


# ---- the C entry on hand-made lists: a covering set ----------------------------------------------------------------------------
#: (E, L, nprobe, k, B, parts): every value of the issue's axes occurs -- nprobe == L where L <= 256, the limit 256 at L = 300,
#: k = 254 at E = 1024; the lists of hand_made have the edge lengths 0, 1, 31, 32, 33, 127, 128, 129 and one of over half the rows
COVER = [(16, 1, 1, 1, 1, 1), (48, 3, 2, 5, 31, 2), (64, 37, 37, 64, 33, 7), (80, 300, 256, 5, 33, 1), (512, 37, 2, 200, 70, 64),
         (1024, 300, 2, 254, 70, 2), (512, 3, 3, 256, 1, 64), (16, 37, 1, 256, 70, 7), (1024, 1, 1, 64, 31, 7), (80, 3, 1, 200, 33, 1),
         (64, 300, 256, 64, 31, 2), (48, 37, 37, 1, 65, 0)]


@pytest.mark.parametrize("E, L, nprobe, k, B, parts", COVER)
def test_grouped_search_is_bit_equal_to_the_rule(E, L, nprobe, k, B, parts):
    d = hand_made(E, L, B, 5000 if L == 300 else 3000, 1000 * L + E + k)
    assert nprobe == min(L, 256) or nprobe <= 2
    check(d, cycling_probes(B, L, nprobe), k, parts)


def test_the_covering_set_covers():
    for axis, values in enumerate(((16, 48, 64, 80, 512, 1024), (1, 3, 37, 300), None, (1, 5, 64, 200, 254, 256), None, (1, 2, 7, 64))):
        if values:
            assert {c[axis] for c in COVER} >= set(values)
    assert {1, 2} <= {c[2] for c in COVER} and {c[1] for c in COVER if c[2] == min(c[1], 256)} == {1, 3, 37, 300}      # nprobe == L
    assert all(k <= ffi.lib.tfimm_hip_embed_search_wide_max_k(E) for E, _, _, k, _, _ in COVER)
    assert (1024, 254) in {(c[0], c[3]) for c in COVER}


# ---- the edges of a tile on the query side ------------------------------------------------------------------------------------------
def test_lists_named_by_1_31_32_33_64_and_65_queries():
    """six lists are named by exactly that many queries of one batch: tiles with one lane, 31 lanes, a full tile, a full tile
    and a lane, two full tiles, two and a lane.  The second slot of a query names none of the six."""
    L, sizes = 37, (1, 31, 32, 33, 64, 65)
    B = sum(sizes)
    d = hand_made(64, L, B, 3000, 21)
    lens = np.diff(d.host[3])
    six = [int(np.argmax(lens))] + [int(np.flatnonzero(lens == n)[0]) for n in (1, 31, 33, 128, 129)]
    rest = [l for l in range(L) if l not in six]
    rng = np.random.default_rng(5)
    probes = np.empty((B, 2), np.int32)
    probes[:, 0] = rng.permutation(np.repeat(six, sizes))                    # the queries of a list are scattered over the batch
    probes[:, 1] = np.where(rng.random(B) < 0.5, -1, rng.choice(rest, B))
    assert sorted(np.bincount(probes[:, 0], minlength=L)[six].tolist()) == sorted(sizes)
    for k, parts in ((20, 2), (200, 1)):
        check(d, probes, k, parts)


def test_one_list_for_all_a_list_per_pair_and_a_single_query():
    L = 300
    d = hand_made(80, L, 70, 5000, 22)
    lens = np.diff(d.host[3])
    big = int(np.argmax(lens))
    check(d, np.full((70, 1), big, np.int32), 20, 3)                         # all 70 queries name one list: tiles of 32, 32 and 6
    check(d, np.stack([np.full(70, big), np.arange(70) % 2 * 5 + 1], 1).astype(np.int32), 5, 1)
    probes = cycling_probes(33, L, 8)                                        # every pair names a list of its own: 264 tiles of one lane
    assert len(set(probes.ravel().tolist())) == probes.size
    check(d, probes, 20, 2, rows=(0, 33))
    check(d, np.arange(37, dtype=np.int32)[None, :], 64, 2, rows=(0, 1))     # B = 1
    check(d, np.array([[big]], np.int32), 5, 7, rows=(0, 1))


@pytest.mark.parametrize("k", [5, 200])
def test_a_list_in_ascending_score_order_is_pruned_again_and_again(k):
    """4000 rows in ascending score order for query 0 and its copies: each step appends all its 128 rows to their buffers,
    which are pruned every other step; the other queries see the rows unordered.  33 queries: two tiles, one lane in the second"""
    q = grid(3, (33, 48))
    q[2::3] = q[0]
    g = grid(4, (4000, 48))
    g = g[np.argsort(er.scores64(q[:1], g)[0], kind="stable")]
    d = Lists(q, g, np.zeros(4000, np.int64), 1)
    probes = np.zeros((33, 1), np.int32)
    idx, _ = check(d, probes, k, 1)
    assert idx[0, 0] >= 3990 and np.array_equal(idx[2], idx[0])              # the best rows of query 0 are the last ones
    assert same(grouped(d, probes, k, 3), (idx, _))


# ---- odd probes ------------------------------------------------------------------------------------------------------------------------
def test_skipped_probes_and_queries_without_a_live_pair():
    L = 37
    d = hand_made(16, L, 8, 3000, 9)
    lens = np.diff(d.host[3])
    probes = cycling_probes(8, L, 4)
    base = d.rule(probes, 20)
    holes = probes.copy()
    holes[0, 1], holes[1, 0], holes[2, 3] = -1, L, L + 1000                 # -1, L and beyond: no list
    holes[3] = -1                                                            # a query that probes nothing
    holes[4, :] = [-1, 5, -2 ** 31, 2 ** 31 - 1]                             # the ends of int32
    holes[6] = int(np.flatnonzero(lens == 0)[0])                             # a query whose only list is empty
    holes[7] = [L, -1, int(np.flatnonzero(lens == 0)[0]), 2 ** 31 - 1]       # nothing live in four ways
    idx, sc = check(d, holes, 20, 3)
    for b in (3, 6, 7):
        assert (idx[b] == -1).all() and (er.bits(sc[b]) == 0xff800000).all()
    assert np.array_equal(idx[5], base[0][5])
    assert same((idx, sc), d.search(holes, 20, 3))
    none = np.full((8, 4), -1, np.int32)                                     # a call without a single tile
    idx, sc = check(d, none, 5, 2)
    assert (idx == -1).all()


def test_short_results_hold_none_and_nothing_is_written_behind_them():
    d = hand_made(80, 37, 9, 3000, 5)
    lens = np.diff(d.host[3])
    at = {n: int(np.flatnonzero(lens == n)[0]) for n in (0, 1, 31, 33)}
    probes = np.array([[at[0], at[1]], [at[31], at[33]], [at[1], at[31]]] * 3, np.int32)
    for k in (64, 256):
        idx, sc = check(d, probes, k, 7)                                     # (the guards are checked by grouped)
        for b, have in ((0, 1), (1, 64), (2, 32)):
            assert (idx[b, :have] >= 0).all() and (idx[b, have:] == -1).all() and (er.bits(sc[b, have:]) == 0xff800000).all()


def test_a_repeated_list_counts_once():
    L = 37
    d = hand_made(80, L, 5, 3000, 13)
    lens = np.diff(d.host[3])
    big, one, some = int(np.argmax(lens)), int(np.flatnonzero(lens == 1)[0]), int(np.flatnonzero(lens == 33)[0])
    probes = np.array([[big, big, big, big], [some, one, some, one], [one, one, some, big], [some, -1, some, L], [big, some, one, 3]], np.int32)
    closed = np.array([[big, -1, -1, -1], [some, one, -1, -1], [one, -1, some, big], [some, -1, -1, -1], [big, some, one, 3]], np.int32)
    for k, parts in ((5, 1), (64, 2), (256, 7)):
        idx, sc = check(d, probes, k, parts)
        assert same((idx, sc), grouped(d, closed, k, parts))
        for row in idx:
            found = row[row >= 0]
            assert len(set(found.tolist())) == len(found) and (row[len(found):] == -1).all()
    wide_probes = np.full((5, 256), some, np.int32)                          # one list 256 times, k above its rows
    wide_probes[:, 100] = one
    idx, _ = check(d, wide_probes, 256, 2)
    assert ((idx >= 0).sum(1) == 34).all()


# ---- invariance ------------------------------------------------------------------------------------------------------------------------
def test_the_bits_of_the_single_entry_whatever_parts_batch_order_repetition_or_replay():
    rng = np.random.default_rng(31)
    E, N, L, B, k, nprobe = 64, 3000, 16, 70, 20, 4
    q = rng.standard_normal((B, E)).astype(f32)
    g = er.bf16_round(rng.standard_normal((N, E)).astype(f32))
    assignment = rng.integers(0, L, N)
    d = Lists(q, g, assignment, L, pad_q=1, pad_g=8)
    probes = np.stack([rng.permutation(L)[:nprobe] for _ in range(B)]).astype(np.int32)
    first = d.search(probes, k, 1)                                           # tfimm_hip_embed_search_lists
    for parts in (1, 2, 7, 64, 0):
        assert same(grouped(d, probes, k, parts), first), parts
        assert same(d.search(probes, k, parts), first), parts
    for b in (0, 1, 31, 32, 33, 69):                                         # a query alone
        i1, s1 = grouped(d, probes, k, 2, rows=(b, b + 1))
        assert np.array_equal(i1[0], first[0][b]) and np.array_equal(er.bits(s1[0]), er.bits(first[1][b])), b
    perm = rng.permutation(B)                                                # a permuted batch gives permuted results
    other = Lists(q[perm], g, assignment, L, pad_q=2)
    assert same(grouped(other, probes[perm], k, 2), (first[0][perm], first[1][perm]))
    for _ in range(3):                                                       # the ranks differ from run to run; no bit does
        assert same(grouped(d, probes, k, 7), first)
    # a captured graph of the six launches, replayed three times
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        grouped(d, probes, k, 2, sync=False)                                 # one-time setup outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            indices, scores, _keep = grouped(d, probes, k, 2, sync=False)
    for _ in range(3):
        indices.fill_(-7)
        scores.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(indices.cpu().numpy()[:B * k].reshape(B, k), first[0])
        assert np.array_equal(er.bits(scores.cpu().numpy()[:B * k].reshape(B, k)), er.bits(first[1]))
        assert (indices.cpu().numpy()[B * k:] == -7).all()


# ---- GalleryIndex end to end ----------------------------------------------------------------------------------------------------------
def as_numpy(m):
    return m.indices.numpy(), m.scores.numpy()


@pytest.mark.parametrize("k, nprobe, parts", [(5, 1, 0), (20, 8, 0), (200, 3, 5), (256, 16, 2)])
def test_search_with_of_both_methods_is_search(k, nprobe, parts):
    rows, _, gallery, index = the_index()
    q = clustered_grid(80 + k, 70, CENTRES)
    want = as_numpy(index.search(q, k, nprobe, parts))
    ids, offsets = index.lists()
    rule = ir.search_lists(q, rows[ids], ids, offsets, index.probe(q, nprobe).numpy(), k)
    assert same(want, rule)
    for method in ("grouped", "single"):
        got = index.search_with(q, k, nprobe, parts, method)
        assert got.indices.shape == got.scores.shape == (70, k) and same(as_numpy(got), want), method
        assert (method, 70, k, nprobe, parts or index.parts) in index._work
    assert same(as_numpy(index.search_with(q, k, nprobe, parts)), want)      # the default is "grouped"
    empty = index.search_with(q[:0], k, nprobe, parts)
    assert empty.indices.shape == empty.scores.shape == (0, k)


_GRAPH = {}


def graph_rule(nprobe, k):
    """the numpy rule of ``neighbours`` on the device's own probes, computed once"""
    if (nprobe, k) not in _GRAPH:
        rows, _, gallery, index = the_index()
        ids, offsets = index.lists()
        probes = index.probe(rows, nprobe).numpy()
        idx, sc = ir.search_lists(rows, rows[ids], ids, offsets, probes, k + 1)
        _GRAPH[(nprobe, k)] = nr.drop_self(idx, sc, np.arange(len(rows)))
    return _GRAPH[(nprobe, k)]


@pytest.mark.parametrize("method, batch", [("grouped", 8192), ("grouped", 1500), ("single", 1500), ("grouped", 37 * 32 + 1)])
def test_neighbours_is_the_rule_on_the_devices_own_probes(method, batch):
    rows, _, gallery, index = the_index()
    want = graph_rule(4, 5)
    got = index.neighbours(5, 4, batch, method)
    assert got.indices.shape == got.scores.shape == (4000, 5) and 4000 % batch != 0
    assert same(as_numpy(got), want)
    assert not (got.indices.numpy() == np.arange(4000)[:, None]).any()       # no row is its own neighbour

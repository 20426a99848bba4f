"""pytest -m gpu: the gallery search over inverted lists (tfimm_hip_embed_search_lists, csrc/embed_lists.hip; ``tfimm.GalleryIndex``;
DESIGN.md 3.28) against the written rule of tests/index_ref.py, bit for bit, on exact data (tests/coarse_ref.py ``grid``: every
partial sum is exact in float32, ties are frequent): a covering set of widths, list shapes, probes, k, batches and parts; a list
that forces prune after prune; independence of parts, batch, repetition and replay; short results and skipped probes; the score
bits of the exact search on random data; and ``GalleryIndex`` end to end.  Every launch of the C entry runs over buffers with
guards behind outputs and workspace and NaN in the padding columns of q and g.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import coarse_ref as cr
import embed_ref as er
import index_ref as ir
import model_checks as mc
import test_architectures  # noqa: F401
import tfimm
from tfimm.engine import ffi
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 8          # elements behind every output buffer that a launch must leave alone
grid = cr.grid


class Lists:
    """an index uploaded once: q float32 [B][E + pad_q], the rows in list order bf16 [N][E + pad_g], NaN in every padding
    column -- a launch that read them would show it --, ids and offsets"""

    def __init__(self, q, g, assignment, L, pad_q=0, pad_g=0):
        q, g = np.ascontiguousarray(q, f32), np.ascontiguousarray(g, f32)
        assert np.array_equal(er.bf16_round(g), g) and pad_g % 8 == 0
        (self.B, self.E), self.N, self.L = q.shape, g.shape[0], L
        self.host = (q,) + ir.build_lists(g, assignment, L)                  # q, rows in list order, ids, offsets
        self.ld_q, self.ld_g = self.E + pad_q, self.E + pad_g
        hq = np.full((self.B, self.ld_q), np.nan, f32)
        hq[:, :self.E] = q
        hg = np.full((self.N, self.ld_g), np.nan, f32)
        hg[:, :self.E] = self.host[1]
        self.q, self.g = torch.from_numpy(hq).cuda(), torch.from_numpy(hg).cuda().bfloat16()
        self.ids, self.offsets = torch.from_numpy(self.host[2]).cuda(), torch.from_numpy(self.host[3]).cuda()
        assert self.g.data_ptr() % 16 == 0
        self._probes = {}                                                    # uploaded once each: a capture must not upload

    def search(self, probes, k, parts=0, rows=None, sync=True, ld_extra=3):
        """tfimm_hip_embed_search_lists for the queries ``rows`` (a slice; default all) with ``probes`` (B, nprobe) stored at
        pitch nprobe + ld_extra (the columns behind hold list 0: reading them would change the result) -> (indices, scores)
        as numpy arrays, or the device buffers if not ``sync``"""
        lo, hi = (0, self.B) if rows is None else rows
        B, nprobe = hi - lo, probes.shape[1]
        ld_p = nprobe + ld_extra
        hp = np.zeros((B, ld_p), np.int32)
        hp[:, :nprobe] = probes[lo:hi]
        dp = self._probes.get(hp.tobytes() + bytes([ld_extra]))
        if dp is None:
            dp = self._probes[hp.tobytes() + bytes([ld_extra])] = torch.from_numpy(hp).cuda()
        need = ffi.lib.tfimm_hip_embed_search_lists_workspace(B, self.N, self.E, self.L, nprobe, k, parts)
        assert need > 0, ffi.lib.tfimm_hip_last_error().decode()
        work = torch.empty(need + 4 * GUARD, dtype=torch.uint8, device="cuda")
        work[need:] = 0x5a
        scores = torch.full((B * k + GUARD,), -7.0, dtype=torch.float32, device="cuda")
        indices = torch.full((B * k + GUARD,), -7, dtype=torch.int32, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_embed_search_lists(self.q.data_ptr() + 4 * lo * self.ld_q, self.ld_q, B, self.g.data_ptr(), self.ld_g,
                                                       self.N, self.E, self.ids.data_ptr(), self.offsets.data_ptr(), self.L,
                                                       dp.data_ptr(), ld_p, nprobe, k, parts, scores.data_ptr(), indices.data_ptr(),
                                                       work.data_ptr(), need, st), "tfimm_hip_embed_search_lists")
        if not sync:
            return indices, scores, (work, dp)
        torch.cuda.synchronize()
        i, s = indices.cpu().numpy(), scores.cpu().numpy()
        assert (i[B * k:] == -7).all() and (s[B * k:] == -7).all() and (work[need:] == 0x5a).all(), "a launch wrote behind a buffer"
        return i[:B * k].reshape(B, k), s[:B * k].reshape(B, k)

    def rule(self, probes, k):
        return ir.search_lists(*self.host, probes, k)

    def check(self, probes, k, parts=0, **kw):
        idx, sc = self.search(probes, k, parts, **kw)
        want_idx, want_sc = self.rule(probes, k)
        assert np.array_equal(idx, want_idx), (np.argwhere(idx != want_idx)[:8], idx[idx != want_idx][:8], want_idx[idx != want_idx][:8])
        assert np.array_equal(er.bits(sc), er.bits(want_sc))
        return idx, sc


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(er.bits(a[1]), er.bits(b[1]))


# ---- the C entry on hand-made lists: a covering set ----------------------------------------------------------------------------
EDGES = (0, 1, 31, 32, 33, 127, 128, 129)


def list_lengths(L, N, seed):
    """L list lengths that sum to N: the edge lengths of a tile and a step, one list that holds over half the rows, the rest
    short (several empty)"""
    if L == 1:
        return [N]
    if L == 3:
        return [0, N - 129, 129]
    rng = np.random.default_rng(seed)
    rest = rng.integers(0, 12, L - len(EDGES) - 1).tolist()
    lens = list(EDGES) + rest
    lens.insert(5, N - sum(lens))
    assert lens[5] > N // 2 and len(lens) == L
    return lens


def hand_made(E, L, B, N, seed):
    rng = np.random.default_rng(seed)
    assignment = rng.permutation(np.repeat(np.arange(L), list_lengths(L, N, seed)))
    return Lists(grid(seed + 1, (B, E)), grid(seed + 2, (N, E)), assignment, L, pad_q=seed % 4, pad_g=8 * (seed % 3))


def cycling_probes(B, L, nprobe):
    """distinct lists per query; over the batch every list is probed (as far as B * nprobe goes)"""
    return ((np.arange(B)[:, None] * nprobe + np.arange(nprobe)[None, :]) % L).astype(np.int32)


#: (E, L, nprobe, k, B, parts): every value of the issue's axes occurs -- nprobe == L where L <= 256, the limit 256 at L = 300
COVER = [(16, 1, 1, 1, 1, 1), (80, 3, 2, 5, 31, 3), (512, 37, 37, 64, 33, 7), (2048, 300, 2, 256, 70, 64), (80, 300, 256, 5, 33, 1),
         (512, 3, 3, 200, 1, 64), (16, 37, 1, 256, 70, 7), (2048, 1, 1, 64, 31, 3), (80, 37, 2, 200, 1, 1), (16, 300, 256, 64, 31, 3),
         (512, 1, 1, 5, 70, 64), (2048, 37, 37, 1, 33, 7), (80, 3, 1, 256, 33, 0)]


@pytest.mark.parametrize("E, L, nprobe, k, B, parts", COVER)
def test_lists_search_is_bit_equal_to_the_rule(E, L, nprobe, k, B, parts):
    N = 2500 if E == 2048 and L < 300 else 5000
    d = hand_made(E, L, B, N, 1000 * L + E + k)
    assert nprobe == min(L, 256) or nprobe <= 2
    d.check(cycling_probes(B, L, nprobe), k, parts)


def test_the_covering_set_covers():
    for axis, values in enumerate(((16, 80, 512, 2048), (1, 3, 37, 300), None, (1, 5, 64, 200, 256), (1, 31, 33, 70), (1, 3, 7, 64))):
        if values:
            assert {c[axis] for c in COVER} >= set(values)
    assert {1, 2} <= {c[2] for c in COVER} and {c[1] for c in COVER if c[2] == min(c[1], 256)} == {1, 3, 37, 300}      # nprobe == L
    for E, L, _, k, _, _ in COVER:
        list_lengths(L, 2500 if E == 2048 and L < 300 else 5000, 1000 * L + E + k)       # (asserts the long list)
    lens = list_lengths(37, 5000, 0)
    assert set(EDGES) <= set(lens) and max(lens) > 2500 and sum(lens) == 5000 == sum(list_lengths(300, 5000, 0))


@pytest.mark.parametrize("k", [5, 200])
def test_a_list_in_ascending_score_order_is_pruned_again_and_again(k):
    """every row beats the threshold of the rows before it: each step appends all its 128 rows, and the one buffer is pruned
    every other step"""
    q = grid(3, (2, 48))
    g = grid(4, (4000, 48))
    g = g[np.argsort(er.scores64(q[:1], g)[0], kind="stable")]               # ascending for query 0; query 1 sees them unordered
    d = Lists(q, g, np.zeros(4000, np.int64), 1)
    probes = np.zeros((2, 1), np.int32)
    idx, _ = d.check(probes, k, 1)
    assert idx[0, 0] >= 3990                                                 # the best rows of query 0 are the last ones
    assert same(d.search(probes, k, 3), d.search(probes, k, 1))


def test_results_do_not_depend_on_parts_batch_repetition_or_replay():
    E, L, B, k, nprobe = 80, 37, 70, 20, 5
    d = hand_made(E, L, B, 5000, 77)
    probes = cycling_probes(B, L, nprobe)
    first = d.check(probes, k, 1)
    for parts in (3, 7, 64, 0):
        assert same(d.search(probes, k, parts), first), parts
    for b in range(B):                                                       # the same queries one at a time
        i1, s1 = d.search(probes, k, 3, rows=(b, b + 1))
        assert np.array_equal(i1[0], first[0][b]) and np.array_equal(er.bits(s1[0]), er.bits(first[1][b])), b
    for _ in range(3):
        assert same(d.search(probes, k, 7), first)
    # a captured graph of the two launches, replayed three times
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d.search(probes, k, 3, sync=False)                                   # one-time setup outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            indices, scores, _keep = d.search(probes, k, 3, sync=False)
    for _ in range(3):
        indices.fill_(-7)
        scores.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(indices.cpu().numpy()[:B * k].reshape(B, k), first[0])
        assert np.array_equal(er.bits(scores.cpu().numpy()[:B * k].reshape(B, k)), er.bits(first[1]))
        assert (indices.cpu().numpy()[B * k:] == -7).all()


def test_short_results_hold_none_and_nothing_is_written_behind_them():
    d = hand_made(80, 37, 9, 5000, 5)
    ids, offsets = d.host[2], d.host[3]
    lens = np.diff(offsets)
    at = {n: int(np.flatnonzero(lens == n)[0]) for n in (0, 1, 31, 33)}      # a list of each of these lengths
    probes = np.array([[at[0], at[1]], [at[31], at[33]], [at[1], at[31]]] * 3, np.int32)
    for k in (64, 256):
        idx, sc = d.check(probes, k, 7)                                      # (the guards are checked by search)
        for b, have in ((0, 1), (1, 64), (2, 32)):
            assert (idx[b, :have] >= 0).all() and (idx[b, have:] == -1).all() and (er.bits(sc[b, have:]) == 0xff800000).all()
            assert np.isfinite(sc[b, :have]).all()


def test_skipped_probes():
    L = 37
    d = hand_made(16, L, 6, 5000, 9)
    probes = cycling_probes(6, L, 4)
    base = d.rule(probes, 20)
    holes = probes.copy()
    holes[0, 1], holes[1, 0], holes[2, 3] = -1, L, L + 1000                 # -1, L and beyond: no list
    holes[3] = -1                                                            # a query that probes nothing
    holes[4, :] = [-1, 5, -2 ** 31, 2 ** 31 - 1]                             # the ends of int32
    idx, sc = d.check(holes, 20, 3)
    assert (idx[3] == -1).all() and (er.bits(sc[3]) == 0xff800000).all()
    assert np.array_equal(idx[5], base[0][5])
    # the same with the skipped slots closed up: a hole changes nothing else
    want = ir.search_lists(d.host[0][:1], *d.host[1:], np.array([[probes[0, 0], probes[0, 2], probes[0, 3]]], np.int32), 20)
    assert np.array_equal(idx[0], want[0][0])


def test_a_repeated_list_counts_once():
    """equal (key, row) pairs must never reach pass 2: a list named again is "no list", whatever k, parts and the batch are"""
    L = 37
    d = hand_made(80, L, 5, 5000, 13)
    lens = np.diff(d.host[3])
    big, one, some = int(np.argmax(lens)), int(np.flatnonzero(lens == 1)[0]), int(np.flatnonzero(lens == 33)[0])
    probes = np.array([[big, big, big, big], [some, one, some, one], [one, one, some, big], [some, -1, some, L], [big, some, one, 3]], np.int32)
    closed = np.array([[big, -1, -1, -1], [some, one, -1, -1], [one, -1, some, big], [some, -1, -1, -1], [big, some, one, 3]], np.int32)
    for k, parts in ((5, 1), (64, 3), (256, 7)):
        idx, sc = d.check(probes, k, parts)
        assert same((idx, sc), d.search(closed, k, parts))
        for row in idx:
            found = row[row >= 0]
            assert len(set(found.tolist())) == len(found) and (row[len(found):] == -1).all()
    wide_probes = np.full((5, 256), some, np.int32)                          # one list 256 times, k above its rows
    wide_probes[:, 100] = one
    idx, _ = d.check(wide_probes, 256, 2)
    assert ((idx >= 0).sum(1) == 34).all()


# ---- random data: the bits of the exact search -------------------------------------------------------------------------------------
def wide(q, g, k):
    """tfimm_hip_embed_search_wide of float32 queries over bf16 rows -> (indices, scores)"""
    B, E = q.shape
    N = g.shape[0]
    dq, dg = torch.from_numpy(np.ascontiguousarray(q)).cuda(), torch.from_numpy(np.ascontiguousarray(g)).cuda().bfloat16()
    need = ffi.lib.tfimm_hip_embed_search_wide_workspace(B, N, E, k, 0)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    scores = torch.empty((B, k), dtype=torch.float32, device="cuda")
    indices = torch.empty((B, k), dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ffi.check(ffi.lib.tfimm_hip_embed_search_wide(dq.data_ptr(), E, B, dg.data_ptr(), E, N, E, k, 0, scores.data_ptr(), indices.data_ptr(),
                                                  work.data_ptr(), need, st), "tfimm_hip_embed_search_wide")
    torch.cuda.synchronize()
    return indices.cpu().numpy(), scores.cpu().numpy()


def test_scores_have_the_bits_of_the_exact_search_on_random_data():
    rng = np.random.default_rng(11)
    E, N, L, B = 64, 256, 8, 33
    q = rng.standard_normal((B, E)).astype(f32)
    g = er.bf16_round(rng.standard_normal((N, E)).astype(f32))
    d = Lists(q, g, rng.integers(0, L, N), L, pad_q=1, pad_g=8)
    all_idx, all_sc = wide(q, g, N)                                          # N = 256: the exact score of every row
    table = np.empty((B, N), np.uint32)
    np.put_along_axis(table, all_idx.astype(np.int64), er.bits(all_sc), 1)
    probes = cycling_probes(B, L, 2)
    idx, sc = d.search(probes, 20, 3)
    assert (idx >= 0).all() and np.array_equal(er.bits(sc), np.take_along_axis(table, idx.astype(np.int64), 1))
    # the rows are the best of the probed lists under the device's own scores, in the rule's order
    ids, offsets = d.host[2], d.host[3]
    value = table.view(f32)
    for b in range(B):
        cand = np.concatenate([ids[offsets[l]:offsets[l + 1]] for l in probes[b]])
        assert idx[b].tolist() == sorted(cand.tolist(), key=lambda n: (-value[b, n], n))[:20], b


@pytest.mark.parametrize("k", [5, 64, 200])
def test_probing_every_list_is_the_exact_search_on_random_data(k):
    rng = np.random.default_rng(12)
    E, N, L, B = 64, 3000, 16, 33
    q = rng.standard_normal((B, E)).astype(f32)
    g = er.bf16_round(rng.standard_normal((N, E)).astype(f32))
    d = Lists(q, g, rng.integers(0, L, N), L)
    probes = np.stack([rng.permutation(L) for _ in range(B)]).astype(np.int32)
    assert same(d.search(probes, k, 3), wide(q, g, k))


# ---- GalleryIndex end to end ----------------------------------------------------------------------------------------------------------
def clustered_grid(seed, n, centres, E=64, changed=10):
    """rows on the grid {-4 .. 4} / 8 around ``centres``: a centre with ``changed`` of its entries drawn anew -- clustered, and
    every score exact in float32"""
    rng = np.random.default_rng(seed)
    x = centres[rng.integers(0, len(centres), n)].copy()
    at = rng.integers(0, E, (n, changed))
    np.put_along_axis(x, at, grid(seed + 1, (n, changed)), 1)
    return x


CENTRES = grid(40, (16, 64))
_INDEX = {}


def the_index():
    """(rows, labels, gallery, index): about 4000 clustered rows of 64 in 16 lists, built once"""
    if not _INDEX:
        rows = clustered_grid(41, 4000, CENTRES)
        labels = (np.arange(4000) * 13 % 29).astype(np.int64)
        gallery = tfimm.Gallery(64)
        gallery.add(rows, labels)
        _INDEX["it"] = (rows, labels, gallery, gallery.build_index(16, iters=4))
    return _INDEX["it"]


def test_index_lists_are_a_partition_that_agrees_with_assign():
    rows, _, gallery, index = the_index()
    assert (index.size, index.n_lists, index.dim, index.stale) == (4000, 16, 64, False) and len(index.centroids) == 16
    ids, offsets = index.lists()
    assert sorted(ids.tolist()) == list(range(4000)) and offsets[0] == 0 and offsets[-1] == 4000
    counts = index.counts.numpy()
    assert np.array_equal(np.diff(offsets), counts) and counts.sum() == 4000 and (counts > 0).sum() >= 8
    assigned = gallery.assign(index.centroids).clusters.numpy()
    for l in range(16):
        part = ids[offsets[l]:offsets[l + 1]]
        assert (np.diff(part) > 0).all() and (assigned[part] == l).all(), l
    assert np.array_equal(index._rows[:, :64].float().cpu().numpy(), rows[ids])      # the list-ordered copy
    assert index.longest == counts.max() and index.parts == -(-int(counts.max()) // 2048)


@pytest.mark.parametrize("k, nprobe, parts", [(5, 1, 0), (20, 8, 0), (200, 3, 5), (256, 16, 2)])
def test_index_search_is_the_rule_over_its_own_probe_and_lists(k, nprobe, parts):
    rows, _, gallery, index = the_index()
    q = clustered_grid(50 + k, 33, CENTRES)
    ids, offsets = index.lists()
    probes = index.probe(q, nprobe)
    assert probes.shape == (33, nprobe) and probes.dtype == torch.int32
    assert np.array_equal(probes.numpy(), index.centroids.search(q, nprobe).indices.numpy())
    got = index.search(q, k, nprobe, parts)
    want = ir.search_lists(q, rows[ids], ids, offsets, probes.numpy(), k)
    assert np.array_equal(got.indices.numpy(), want[0]) and np.array_equal(er.bits(got.scores.numpy()), er.bits(want[1]))
    if nprobe == 16:                                                         # every list: the exact search
        exact = gallery.search(q, k)
        assert same((got.indices.numpy(), got.scores.numpy()), (exact.indices.numpy(), exact.scores.numpy()))
    else:                                                                    # and otherwise every row found is in a probed list
        assigned, gi = gallery.assign(index.centroids).clusters.numpy(), got.indices.numpy()
        for b in range(33):
            assert set(assigned[gi[b][gi[b] >= 0]].tolist()) <= set(probes.numpy()[b].tolist()), b
    assert (33, k, nprobe, parts or index.parts) in index._work


def test_index_is_a_snapshot():
    rows = clustered_grid(60, 1500, CENTRES)
    q = clustered_grid(61, 9, CENTRES)
    gallery = tfimm.Gallery(64, capacity=1500)
    gallery.add(rows[:1000])
    index = gallery.build_index(8, iters=3)
    before = index.search(q, 20, 8)
    want = er.search(q, rows[:1000], 20)
    assert np.array_equal(before.indices.numpy(), want[0]) and np.array_equal(er.bits(before.scores.numpy()), er.bits(want[1]))
    assert not index.stale
    gallery.add(rows[1000:1400])
    assert index.stale and index.size == 1000
    gallery.add(rows[1400:])
    assert index.stale and index.size == 1000 and len(gallery) == 1500 and gallery.capacity == 1500
    gallery.add(q)                                                           # a regrow: the gallery's buffer moves, the index's does not
    assert gallery.capacity > 1500 and len(gallery) == 1509
    after = index.search(q, 20, 8)                                           # the index still answers for its 1000 rows
    assert same((after.indices.numpy(), after.scores.numpy()), (before.indices.numpy(), before.scores.numpy()))
    # an index over given clusters: no k-means runs
    clusters = gallery.kmeans(8, iters=2)
    again = gallery.build_index(clusters=clusters)
    assert again.size == 1509 and not again.stale and again.centroids is clusters.centroids
    assert np.array_equal(again.counts.numpy(), clusters.counts.numpy())
    full, exact = again.search(q, 20, 8), gallery.search(q, 20)
    assert same((full.indices.numpy(), full.scores.numpy()), (exact.indices.numpy(), exact.scores.numpy()))
    assert not same((full.indices.numpy(), full.scores.numpy()), (before.indices.numpy(), before.scores.numpy()))     # the new rows count


def test_index_classify_is_the_vote_on_the_rules_matches():
    rows, labels, gallery, index = the_index()
    q = clustered_grid(70, 9, CENTRES)

    def check(index, gallery, rows, q, k, nprobe, **kw):
        ids, offsets = index.lists()
        ks = k + (1 if kw.get("exclude") is not None else 0)
        idx, sc = ir.search_lists(q, rows[ids], ids, offsets, index.probe(q, nprobe).numpy(), ks)
        m = tfimm.Matches(tfimm.models.model.Tensor(torch.from_numpy(idx).cuda()), tfimm.models.model.Tensor(torch.from_numpy(sc).cuda()))
        got, want = index.classify(q, k, nprobe, **kw), gallery.vote(m, **kw)
        for x, y in zip(got, want):
            assert np.array_equal(x.numpy().view(np.uint32), y.numpy().view(np.uint32))
        return idx, got

    check(index, gallery, rows, q, 20, 8)
    check(index, gallery, rows, q, 63, 2, temperature=None, top=3)
    check(index, gallery, rows, q, 10, 4, reduce="max", exclude=np.arange(9))
    # lists of a few rows: queries with fewer than k candidates, whose -1 slots are no candidates of the vote
    small_rows = clustered_grid(71, 60, CENTRES)
    small = tfimm.Gallery(64)
    small.add(small_rows, np.arange(60) % 5)
    small_index = small.build_index(16, iters=2)
    idx, got = check(small_index, small, small_rows, q, 40, 2)
    assert (idx == -1).any()
    assert (got.counts.numpy().sum(1) == (idx >= 0).sum(1)).all()


def test_model_search_index():
    bb = tfimm.create_model("vit_test_model")
    m = tfimm.EmbeddingModel(bb, 48, normalize=True)
    m.set_weights(synthetic_weights(m, 2021))
    x = mc.make_input(m.cfg, 4)
    gallery = tfimm.Gallery(48)
    gallery.add(m(x))
    gallery.add((np.random.default_rng(3).standard_normal((300, 48)) / 7).astype(f32))
    index = gallery.build_index(6, iters=3)
    with pytest.raises(ValueError, match="nprobe = 7"):
        m.search_index(x, index, nprobe=7)
    got = m.search_index(x, index, k=10, nprobe=6)
    want = index.search(m(x), 10, 6)
    assert got.indices.shape == got.scores.shape == (4, 10)
    assert same((got.indices.numpy(), got.scores.numpy()), (want.indices.numpy(), want.scores.numpy()))
    assert got.indices.numpy()[:, 0].tolist() == [0, 1, 2, 3]               # every list is probed: every image finds itself
    one, want = m.search_index(x, index, k=3, nprobe=1), index.search(m(x), 3, 1)
    assert one.indices.shape == (4, 3) and same((one.indices.numpy(), one.scores.numpy()), (want.indices.numpy(), want.scores.numpy()))

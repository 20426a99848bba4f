"""pytest -m gpu: the index that follows its gallery against the written rules of tests/live_ref.py, bit for bit,
on exact data (tests/coarse_ref.py ``grid``: every partial sum is exact in float32, ties are frequent): tfimm_hip_matches_merge
over guarded buffers on a covering set of sets, widths, k and batches, with repetition, replay and slices of the batch;
``Gallery.search_range``; ``GalleryIndex.search_live`` end to end while the gallery grows; ``absorb``; ``classify_live``; and
``EmbeddingModel.search_live``.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import coarse_ref as cr
import embed_ref as er
import live_ref as lr
import model_checks as mc
import test_architectures  # noqa: F401
import tfimm
from tfimm.engine import ffi
from tfimm.models.model import Tensor
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 8          # elements behind every output buffer that a launch must leave alone
NINF, QNAN = 0xff800000, 0x7fffffff
grid = cr.grid


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(er.bits(a[1]), er.bits(b[1]))


def host(m):
    return m.indices.numpy(), m.scores.numpy()


# ---- the C entry over guarded buffers ------------------------------------------------------------------------------------------
class Sets:
    """S sets of matches uploaded once: set s float32 / int32 [B][k_s + pad] with NaN scores and index -7 in the padding
    columns -- a launch that read them would show it"""

    def __init__(self, parts, bases, pad=3):
        self.parts = [(np.ascontiguousarray(i, np.int32), np.ascontiguousarray(s, f32)) for i, s in parts]
        self.bases, self.B = list(bases), self.parts[0][0].shape[0]
        self.dev = []
        for i, s in self.parts:
            hi = np.full((self.B, i.shape[1] + pad), -7, np.int32)
            hs = np.full((self.B, i.shape[1] + pad), np.nan, f32)
            hi[:, :i.shape[1]], hs[:, :i.shape[1]] = i, s
            self.dev.append((torch.from_numpy(hi).cuda(), torch.from_numpy(hs).cuda()))

    def merge(self, k, rows=None, sync=True, pad_out=2):
        """tfimm_hip_matches_merge for the queries ``rows`` (a slice; default all) into outputs of pitch k + pad_out ->
        (indices, scores) as numpy arrays, or the device buffers if not ``sync``"""
        lo, hi = (0, self.B) if rows is None else rows
        B, ld = hi - lo, k + pad_out
        arr = (ffi.MatchSet * len(self.dev))()
        for rec, (i, s), (hi_, _), base in zip(arr, self.dev, self.parts, self.bases):
            rec.indices, rec.scores = i.data_ptr() + 4 * lo * i.shape[1], s.data_ptr() + 4 * lo * i.shape[1]
            rec.ld, rec.k, rec.base = i.shape[1], hi_.shape[1], base
        scores = torch.full((B * ld + GUARD,), -7.0, dtype=torch.float32, device="cuda")
        indices = torch.full((B * ld + GUARD,), -7, dtype=torch.int32, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_matches_merge(arr, len(self.dev), B, k, scores.data_ptr(), indices.data_ptr(), ld, st),
                  "tfimm_hip_matches_merge")
        if not sync:
            return indices, scores
        torch.cuda.synchronize()
        return self.unpack(indices, scores, B, k, ld)

    @staticmethod
    def unpack(indices, scores, B, k, ld):
        i, s = indices.cpu().numpy(), scores.cpu().numpy()
        assert (i[B * ld:] == -7).all() and (s[B * ld:] == -7).all(), "a launch wrote behind a buffer"
        i, s = i[:B * ld].reshape(B, ld), s[:B * ld].reshape(B, ld)
        assert (i[:, k:] == -7).all() and (s[:, k:] == -7).all(), "a launch wrote into the padding columns"
        return np.ascontiguousarray(i[:, :k]), np.ascontiguousarray(s[:, :k])

    def check(self, k, **kw):
        got = self.merge(k, **kw)
        lo, hi = kw.get("rows") or (0, self.B)
        want = lr.merge([(i[lo:hi], s[lo:hi]) for i, s in self.parts], self.bases, k)
        assert np.array_equal(got[0], want[0]), (np.argwhere(got[0] != want[0])[:8], got[0][got[0] != want[0]][:8])
        assert np.array_equal(er.bits(got[1]), er.bits(want[1]))
        return got


def made_sets(widths, B, seed, interleave=True):
    """sets as the searches leave them: per query and set a run of valid entries of every length 0 .. k_s -- whole sets empty,
    all sets empty (query 1) and full ones among them --, ordered by (key descending, row ascending), -1 behind them with
    scores that must not be looked at.  Scores come from a grid of 9 values, so equal scores across sets are the rule; the
    rows of set s are S t + s with base s (``interleave``: the rows of the sets alternate) or t with base 1000 s."""
    rng = np.random.default_rng(seed)
    S = len(widths)
    parts = []
    for s, w in enumerate(widths):
        idx = np.full((B, w), -1, np.int32)
        sc = rng.choice(np.array([99.0, -np.inf, 0.0], f32), (B, w)).astype(f32)       # behind the valid entries: anything
        for b in range(B):
            n = (b * 11 + s * 3) % (w + 1) if b % 5 else (w if b % 2 == 0 else 0)       # every length; b = 0: full, b = 5: empty
            if b == 1:
                n = 0                                                                    # query 1: every set is empty
            t = rng.choice(1000, n, replace=False)
            v = (rng.integers(-4, 5, n) / 4).astype(f32)
            row = t * S + s if interleave else t
            order = np.lexsort((row, -lr.key_of(er.bits(v)).astype(np.int64)))
            idx[b, :n], sc[b, :n] = (t * S if interleave else t)[order], v[order]
        parts.append((idx, sc))
    return Sets(parts, [s if interleave else 1000 * s for s in range(S)], pad=seed % 4)


#: (set widths, k, B): S in 1, 2, 3, 8; k in 1, 5, 64, 65, 256; widths shorter and longer than k; B in 1, 3, 64, 65, 1000
COVER = [((5,), 5, 1), ((256,), 1, 3), ((3, 256), 64, 64), ((256, 256, 1), 256, 65), ((5, 20, 1, 64, 65, 200, 7, 256), 65, 1000),
         ((256,) * 8, 256, 3), ((5, 20), 5, 1000), ((64, 1, 200), 5, 65), ((64, 65), 65, 64), ((1,) * 8, 1, 1), ((20, 5, 64), 256, 3)]


@pytest.mark.parametrize("widths, k, B", COVER)
def test_merge_is_bit_equal_to_the_rule(widths, k, B):
    made_sets(widths, B, 100 * len(widths) + k + B).check(k)
    made_sets(widths, min(B, 9), 7 * len(widths) + k, interleave=False).check(k)


def test_the_covering_set_covers():
    assert {len(w) for w, _, _ in COVER} >= {1, 2, 3, 8} and {k for _, k, _ in COVER} >= {1, 5, 64, 65, 256}
    assert {B for _, _, B in COVER} >= {1, 3, 64, 65, 1000}
    assert any(min(w) < k < max(w) for w, k, _ in COVER) and any(max(w) < k for w, k, _ in COVER)
    d = made_sets((5, 20, 3), 64, 1)
    lens = [(i >= 0).sum(1) for i, _ in d.parts]
    assert all(set(n.tolist()) == set(range(i.shape[1] + 1)) for n, (i, _) in zip(lens, d.parts))     # -1 runs of every length
    assert all(n[1] == 0 for n in lens) and all(n[0] == i.shape[1] for n, (i, _) in zip(lens, d.parts))


def test_merge_special_values():
    nan_neg = np.array([0xffc12345], np.uint32).view(f32)[0]
    a = (np.array([[5, 6, 7, 8]], np.int32), np.array([[np.inf, -0.0, -1.0, -np.inf]], f32))
    b = (np.array([[0, 1, 2]], np.int32), np.array([[nan_neg, 0.0, -np.inf]], f32))
    idx, sc = Sets([a, b], [0, 0]).check(8)
    # NaN first, above +inf; the two zeros are equal and decided by row; -inf with a valid index before the fill, by row
    assert idx.tolist() == [[0, 5, 1, 6, 7, 2, 8, -1]]
    assert er.bits(sc)[0].tolist() == [QNAN, 0x7f800000, 0, 0, 0xbf800000, NINF, NINF, NINF]
    idx, sc = Sets([a, b], [0, 10]).check(4)                                 # with a base the zero of row 6 comes first
    assert idx.tolist() == [[10, 5, 6, 11]] and er.bits(sc)[0].tolist() == [QNAN, 0x7f800000, 0, 0]
    idx, sc = Sets([a], [2 ** 31 - 9]).check(6)                              # the largest rows an int32 holds
    assert idx.tolist() == [[2 ** 31 - 4, 2 ** 31 - 3, 2 ** 31 - 2, 2 ** 31 - 1, -1, -1]]


def test_merge_does_not_depend_on_repetition_replay_or_the_batch():
    widths, k, B = (20, 64, 5), 20, 70
    d = made_sets(widths, B, 77)
    first = d.check(k)
    for _ in range(2):
        assert same(d.merge(k), first)
    for lo, hi in ((0, 1), (3, 7), (64, 70), (69, 70), (1, 66)):             # rows [lo, hi) merged alone
        got = d.check(k, rows=(lo, hi))
        assert same(got, (first[0][lo:hi], first[1][lo:hi])), (lo, hi)
    # a captured graph of the one launch, replayed three times: the sets travelled as kernel arguments
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d.merge(k, sync=False)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            indices, scores = d.merge(k, sync=False)
    for _ in range(3):
        indices.fill_(-7)
        scores.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert same(Sets.unpack(indices, scores, B, k, k + 2), first)


def test_merge_matches_is_the_rule_on_matches():
    d = made_sets((20, 64, 5), 33, 5, interleave=False)
    parts = [tfimm.Matches(Tensor(torch.from_numpy(i).cuda()), Tensor(torch.from_numpy(s).cuda())) for i, s in d.parts]
    for k in (None, 5, 100):
        assert same(host(tfimm.merge_matches(parts, d.bases, k)), lr.merge(d.parts, d.bases, k))
    assert same(host(tfimm.merge_matches(parts[:1])), lr.merge(d.parts[:1]))
    empty = tfimm.merge_matches([tfimm.Matches(Tensor(m.indices.torch()[:0]), Tensor(m.scores.torch()[:0])) for m in parts], k=7)
    assert empty.indices.shape == empty.scores.shape == (0, 7)


# ---- Gallery.search_range ---------------------------------------------------------------------------------------------------------
_STATE = {}


def the_gallery():
    """(rows, gallery): 1000 grid rows of 64, uploaded once"""
    if "gallery" not in _STATE:
        rows = grid(30, (1000, 64))
        rows[[3, 510, 600, 999]] = rows[0]                                   # equal rows: ties decided by the row, in and across ranges
        gallery = tfimm.Gallery(64)
        gallery.add(rows)
        _STATE["gallery"] = (rows, gallery)
    return _STATE["gallery"]


def range_rule(q, rows, k, start, stop):
    idx = np.full((q.shape[0], k), -1, np.int32)
    sc = np.full((q.shape[0], k), -np.inf, f32)
    n = min(k, stop - start)
    if n:
        i, s = er.search(q, rows[start:stop], n)
        idx[:, :n], sc[:, :n] = i + start, s
    return idx, sc


@pytest.mark.parametrize("start, stop", [(0, 1000), (0, 1), (999, 1000), (37, 37), (500, 700)])
def test_search_range_is_the_exact_search_of_the_slice(start, stop):
    rows, gallery = the_gallery()
    q = np.concatenate([grid(31, (8, 64)), rows[:1]])                       # the last query equals rows 0, 3, 510, 600 and 999
    for k in (1, 5, 20, 200):                                               # above and below the range's length; both routes
        want = range_rule(q, rows, k, start, stop)
        got = host(gallery.search_range(q, k, start, stop))
        assert same(got, want), (k, start, stop)
        if stop - start >= k:
            for method in ("list", "buffer") if k <= 64 else ("buffer",):
                assert same(host(gallery.search_range(q, k, start, stop, method)), want), (k, method)
    if (start, stop) == (0, 1000):
        whole, part = gallery.search(q, 20), gallery.search_range(q, 20)    # the defaults: every row
        assert same(host(whole), host(part))
        assert gallery._range_args(5, 0, None, "auto")[3] == "list" and gallery._range_args(20, 0, None, "auto")[3] == "buffer"


def test_search_range_gives_the_bits_of_search_on_random_rows_and_merges_back():
    rng = np.random.default_rng(21)
    g = rng.standard_normal((256, 64)).astype(f32)
    q = rng.standard_normal((9, 64)).astype(f32)
    gallery = tfimm.Gallery(64)
    gallery.add(g)
    all_idx, all_sc = host(gallery.search(q, 256))                           # the score of every row
    table = np.empty((9, 256), np.uint32)
    np.put_along_axis(table, all_idx.astype(np.int64), er.bits(all_sc), 1)
    for start, stop, k in ((0, 100, 20), (100, 101, 20), (101, 256, 200), (0, 256, 256)):
        m = gallery.search_range(q, k, start, stop)
        idx, sc = host(m)
        found = idx >= 0
        assert (found.sum(1) == min(k, stop - start)).all() and ((idx[found] >= start) & (idx[found] < stop)).all()
        assert np.array_equal(er.bits(sc)[found], np.take_along_axis(table, np.maximum(idx, 0).astype(np.int64), 1)[found])
    assert same((idx, sc), (all_idx, all_sc))
    # a gallery searched in three pieces and joined is the gallery searched at once
    pieces = [gallery.search_range(q, 64, start, stop) for start, stop in ((0, 100), (100, 101), (101, 256))]
    for k in (5, 64):
        assert same(host(tfimm.merge_matches(pieces, k=k)), host(gallery.search(q, k)))


# ---- GalleryIndex.search_live end to end -----------------------------------------------------------------------------------------------
def clustered_grid(seed, n, centres, E=64, changed=10):
    """rows on the grid {-4 .. 4} / 8 around ``centres`` (tests/test_gpu_search_index.py): clustered, every score exact"""
    rng = np.random.default_rng(seed)
    x = centres[rng.integers(0, len(centres), n)].copy()
    at = rng.integers(0, E, (n, changed))
    np.put_along_axis(x, at, grid(seed + 1, (n, changed)), 1)
    return x


CENTRES = grid(40, (16, 64))
ROWS = clustered_grid(41, 2805, CENTRES)
ROWS[[1000, 1003, 1700, 2804]] = ROWS[7]                                     # equal rows on both sides of the snapshot boundary
QUERIES = np.concatenate([clustered_grid(42, 8, CENTRES), ROWS[7:8]])


def grown(fresh, labels=False):
    """(gallery, index): 1000 rows clustered into 16 lists and indexed, then ``fresh`` rows added in the steps 1, 4, 300, 1500"""
    gallery = tfimm.Gallery(64, capacity=1000)
    lab = (np.arange(2805) % 29).astype(np.int64)
    gallery.add(ROWS[:1000], lab[:1000] if labels else None)
    index = gallery.build_index(16, iters=3)
    at = 1000
    for step in (1, 4, 300, 1500):
        if at - 1000 < fresh:
            gallery.add(ROWS[at:at + step], lab[at:at + step] if labels else None)
            at += step
    assert len(gallery) == 1000 + fresh and index.size == 1000 and index.fresh == fresh and index.stale == (fresh > 0)
    return gallery, index


def assignment_of(index):
    ids, offsets = index.lists()
    a = np.empty(index.size, np.int64)
    for l in range(index.n_lists):
        a[ids[offsets[l]:offsets[l + 1]]] = l
    return a


@pytest.mark.parametrize("fresh", [0, 1, 5, 305, 1805])
def test_search_live_is_the_rule_while_the_gallery_grows(fresh):
    gallery, index = grown(fresh)
    assert (gallery.capacity > 2000) == (fresh == 1805)                      # the last step makes the gallery's buffer grow
    n = 1000 + fresh
    cen, a = index.centroids.numpy(), assignment_of(index)
    for nprobe in (1, 4, 16):
        probes = index.probe(QUERIES, nprobe).numpy()
        for k in (5, 20, 200):
            want = lr.search_live(QUERIES, ROWS[:n], cen, a, nprobe, k, probes=probes)
            single = host(index.search_live(QUERIES, k, nprobe))
            assert same(single, want), (fresh, nprobe, k)
            assert same(host(index.search_live(QUERIES, k, nprobe, "grouped")), single), (fresh, nprobe, k)
            if nprobe == 16:                                                 # every list: the exact search over every row
                assert same(single, host(gallery.search(QUERIES, k))), (fresh, k)
            if not fresh:
                assert same(single, host(index.search_with(QUERIES, k, nprobe, 0, "single")))
            elif k == 20:                                                    # the snapshot's answer misses rows the live one has
                snap = host(index.search_with(QUERIES, k, nprobe, 0, "single"))
                assert (snap[0] < 1000).all() and (single[0][-1] >= 1000).any()
    assert host(index.search_live(QUERIES[:0], 5, 4))[0].shape == (0, 5)


def test_search_live_finds_a_fresh_row_whose_list_is_not_probed():
    """the planted row of tests/test_search_live.py on the device: ``search`` misses it, ``search_live`` finds it"""
    q = grid(5, (1, 64))
    q[0, 0] = 0.5
    g = np.concatenate([q / 2, q / 4, -q, q])
    cen = tfimm.Gallery._of_rows(64, torch.from_numpy(np.concatenate([-q, q])).cuda(), torch.arange(2, dtype=torch.int32, device="cuda"))

    def build(n, assignment):
        gallery = tfimm.Gallery(64)
        gallery.add(g[:n])
        a = Tensor(torch.tensor(assignment, dtype=torch.int32, device="cuda"))
        return gallery, gallery.build_index(clusters=tfimm.Clusters(cen, a, None, None, None))

    gallery, index = build(4, [1, 1, 1, 0])                                  # an index over all rows: row 3's list is probed last
    assert host(index.search(q, 2, 1))[0].tolist() == [[0, 1]] and host(index.search_live(q, 2, 1))[0].tolist() == [[0, 1]]
    gallery, index = build(3, [1, 1, 1])
    gallery.add(g[3:])                                                       # the best row arrives after the build
    assert host(index.search(q, 2, 1))[0].tolist() == [[0, 1]]
    got = host(index.search_live(q, 2, 1))
    assert got[0].tolist() == [[3, 0]] and same(got, lr.search_live(q, g, np.concatenate([-q, q]), np.array([1, 1, 1]), 1, 2))
    assert same(got, host(gallery.search(q, 2)))
    got = host(index.search_live(q, 6, 2, "grouped"))                        # short: four rows, then the fill
    assert got[0].tolist() == [[3, 0, 1, 2, -1, -1]] and (er.bits(got[1])[0, 4:] == NINF).all()


# ---- absorb on the device -----------------------------------------------------------------------------------------------------------------
def same_index(a, b):
    for x, y in zip(a.lists(), b.lists()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.counts.numpy(), b.counts.numpy()) and torch.equal(a._rows, b._rows)
    assert (a.size, a.longest, a.parts, a.stale, a.fresh) == (b.size, b.longest, b.parts, False, 0)


def test_absorb_is_the_index_built_over_the_joined_assignment():
    gallery, index = grown(305)
    old = torch.from_numpy(assignment_of(index)).int().cuda()
    new = gallery.assign(index.centroids).clusters.torch()[1000:]
    assert torch.equal(index._assignment(), old)
    index.search_live(QUERIES, 5, 4)                                         # fills the workspace cache
    assert index._work and index.absorb() == 305
    assert not index._work and not index.stale and index.size == 1305
    clusters = tfimm.Clusters(index.centroids, Tensor(torch.cat([old, new])), None, None, None)
    built = gallery.build_index(clusters=clusters)
    same_index(index, built)
    assert np.array_equal(assignment_of(index)[:1000], old.cpu().numpy())    # old rows keep their list
    for k, nprobe in ((5, 1), (20, 4), (200, 16)):
        live = host(index.search_live(QUERIES, k, nprobe))
        assert same(live, host(index.search_with(QUERIES, k, nprobe, 0, "single")))
        assert same(live, host(built.search_with(QUERIES, k, nprobe, 0, "single")))
    # a second add, absorbed with a routing of the caller's choice
    gallery.add(ROWS[1305:1405])
    assert index.fresh == 100 and index.absorb(assignment=torch.full((100,), 3, dtype=torch.int32, device="cuda")) == 100
    ids, offsets = index.lists()
    assert ids[offsets[3]:offsets[4]][-100:].tolist() == list(range(1305, 1405)) and index.size == 1405
    every = torch.cat([old, new, torch.full((100,), 3, dtype=torch.int32, device="cuda")])
    same_index(index, gallery.build_index(clusters=tfimm.Clusters(index.centroids, Tensor(every), None, None, None)))
    assert same(host(index.search_live(QUERIES, 20, 16)), host(gallery.search(QUERIES, 20)))
    # and a third from the host, with the centroids' own choice again
    gallery.add(ROWS[1405:1500])
    want = gallery.assign(index.centroids).clusters.numpy()[1405:]
    assert index.absorb() == 95 and np.array_equal(assignment_of(index)[1405:], want) and index.absorb() == 0


# ---- classify_live and the model's front door ----------------------------------------------------------------------------------------------
def test_classify_live_is_the_vote_on_the_live_matches_and_a_new_identity_wins():
    gallery, index = grown(305, labels=True)
    q = QUERIES
    for kw in (dict(k=20, nprobe=4), dict(k=63, nprobe=2, temperature=None, top=3), dict(k=10, nprobe=16, reduce="max", exclude=np.arange(9))):
        k, nprobe = kw.pop("k"), kw.pop("nprobe")
        ks = k + (1 if kw.get("exclude") is not None else 0)
        got, want = index.classify_live(q, k, nprobe, **kw), gallery.vote(index.search_live(q, ks, nprobe), **kw)
        for x, y in zip(got, want):
            assert np.array_equal(x.numpy().view(np.uint32), y.numpy().view(np.uint32))
    assert index.classify_live(q[:0], 5, 2).classes.shape == (0, 5)          # no queries: nothing is launched
    # enrol, then recognise: three rows of a new identity, far from every list the query probes first
    person = -CENTRES[:1] + grid(90, (1, 64)) / 8
    shots = np.concatenate([person, person, person])
    shots[1, 0] += 0.125
    shots[2, 1] -= 0.125
    before = index.classify_live(person, 10, 1)
    gallery.add(shots, np.full(3, 99))
    votes = index.classify_live(person, 10, 1)
    assert votes.classes.numpy()[0, 0] == 99 and votes.counts.numpy()[0, 0] == 3 and 99 not in before.classes.numpy()
    assert 99 not in index.classify(person, 10, 1).classes.numpy()           # the snapshot does not know the person


def test_model_search_live():
    bb = tfimm.create_model("vit_test_model")
    m = tfimm.EmbeddingModel(bb, 48, normalize=True)
    m.set_weights(synthetic_weights(m, 2021))
    x = mc.make_input(m.cfg, 4)
    gallery = tfimm.Gallery(48)
    gallery.add((np.random.default_rng(3).standard_normal((300, 48)) / 7).astype(f32))
    index = gallery.build_index(6, iters=3)
    gallery.add(m(x))                                                        # enrolled after the build: rows 300 .. 303
    with pytest.raises(ValueError, match="nprobe = 7"):
        m.search_live(x, index, nprobe=7)
    got, want = m.search_live(x, index, k=10, nprobe=1), index.search_live(m(x), 10, 1)
    assert got.indices.shape == got.scores.shape == (4, 10) and same(host(got), host(want))
    assert got.indices.numpy()[:, 0].tolist() == [300, 301, 302, 303]       # every image finds itself, whatever is probed
    assert (m.search_index(x, index, k=10, nprobe=6).indices.numpy() < 300).all()

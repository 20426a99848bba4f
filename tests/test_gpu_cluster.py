"""pytest -m gpu: the cluster end on the device.  tfimm_hip_cluster_assign and tfimm_hip_segment_mean
(csrc/cluster.hip) against the written rules of tests/cluster_ref.py -- bit-equal on exact data, inside derived bands on random
data --, and ``Gallery.prototypes`` / ``kmeans`` / ``assign`` / ``set_labels`` end to end on planted clusters."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import cluster_ref as cr
import embed_ref as er
import tfimm
from tfimm.engine import ffi

pytestmark = pytest.mark.gpu
f32, i32 = np.float32, np.int32
GUARD = 8          # elements behind every output buffer that a launch must leave alone
R = cr.RUN
ROW_TILE = CEN_TILE = 128      # csrc/cluster.hip: gallery rows per workgroup, centroids per LDS tile


def grid(seed, shape):
    """test_gpu_embedding.grid: entries from {-4, ..., 4} / 8 -- exact in bf16, every partial sum exact in float32 for
    E <= 2048, so scores are bit-equal to the rule in any summation order, and ties are plentiful"""
    return (np.random.default_rng(seed).integers(-4, 5, shape) / 8).astype(f32)


def upload_bf16(x, pad):
    """bf16 values (float32) -> a bf16 device matrix with ``pad`` NaN columns behind every row"""
    x = np.ascontiguousarray(x, f32)
    assert np.array_equal(er.bf16_round(x), x) and pad % 8 == 0
    h = np.full((x.shape[0], x.shape[1] + pad), np.nan, f32)
    h[:, :x.shape[1]] = x
    t = torch.from_numpy(h).cuda().bfloat16()
    assert t.data_ptr() % 16 == 0
    return t


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- op level: assign ---------------------------------------------------------------------------------------------------------
class Assign:
    """gallery and centroids uploaded once, NaN in every padding column: a launch that read them would show it"""

    def __init__(self, g, c, pad_g=0, pad_c=0):
        (self.N, self.E), self.C = g.shape, c.shape[0]
        self.ld_g, self.ld_c = self.E + pad_g, self.E + pad_c
        self.g, self.c = upload_bf16(g, pad_g), upload_bf16(c, pad_c)

    def run(self, rows=None, C_=None, sync=True):
        """tfimm_hip_cluster_assign for the gallery rows ``rows`` (a slice; default all) against the first ``C_`` centroids
        (default all) -> (assign, score) as numpy arrays, or the device buffers if not ``sync``"""
        lo, hi = (0, self.N) if rows is None else rows
        n, nc = hi - lo, self.C if C_ is None else C_
        assign = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda")
        score = torch.full((n + GUARD,), -7.0, dtype=torch.float32, device="cuda")
        ffi.check(ffi.lib.tfimm_hip_cluster_assign(self.g.data_ptr() + 2 * lo * self.ld_g, self.ld_g, n, self.c.data_ptr(), self.ld_c,
                                                   nc, self.E, assign.data_ptr(), score.data_ptr(), stream()), "tfimm_hip_cluster_assign")
        if not sync:
            return assign, score
        torch.cuda.synchronize()
        a, s = assign.cpu().numpy(), score.cpu().numpy()
        assert (a[n:] == -7).all() and (s[n:] == -7).all(), "a launch wrote behind a buffer"
        return a[:n], s[:n]


def check_exact(g, c, **pads):
    a, s = Assign(g, c, **pads).run()
    want_a, want_s = cr.assign(g, c)
    assert np.array_equal(a, want_a), (np.flatnonzero(a != want_a)[:8], a[a != want_a][:8], want_a[a != want_a][:8])
    assert np.array_equal(er.bits(s), er.bits(want_s))
    return a, s


ES, NS, CS = (16, 48, 512, 2048), (1, 31, 33, 129, 5000), (1, 2, 31, 33, 257, 1000)


def _pairs(case):
    E, N, Cn = case
    return {("EN", E, N), ("EC", E, Cn), ("NC", N, Cn)}


def _covering():
    """a subset of the 120 combinations in which every pair of (E, N, C) values occurs: greedily those that bring three new
    pairs, then two, then one"""
    out, seen = [], set()
    for least in (3, 2, 1):
        for case in itertools.product(ES, NS, CS):
            if len(_pairs(case) - seen) >= least:
                out.append(case)
                seen |= _pairs(case)
    return out


@pytest.mark.parametrize("E, N, Cn", _covering())
def test_assign_is_bit_equal_to_the_rule_on_exact_data(E, N, Cn):
    """both pitches padded with NaN columns (0, 8 or 16 of them, at different rates), guards behind both outputs"""
    check_exact(grid(E + N, (N, E)), grid(Cn + 7, (Cn, E)), pad_g=8 * ((E + N + Cn) % 3), pad_c=8 * ((N + Cn) % 3))


def test_covering_set_covers():
    c = _covering()
    assert len(c) <= 45
    assert {(x[0], x[1]) for x in c} == set(itertools.product(ES, NS))
    assert {(x[0], x[2]) for x in c} == set(itertools.product(ES, CS))
    assert {(x[1], x[2]) for x in c} == set(itertools.product(NS, CS))


@pytest.mark.parametrize("N, Cn", [(ROW_TILE - 1, CEN_TILE + 1), (ROW_TILE, CEN_TILE), (ROW_TILE + 1, CEN_TILE - 1),
                                   (2 * ROW_TILE, 2 * CEN_TILE + 1), (2 * ROW_TILE + 1, 2 * CEN_TILE), (2 * ROW_TILE - 1, 2 * CEN_TILE - 1)])
def test_assign_around_the_row_tile_and_the_centroid_tile(N, Cn):
    check_exact(grid(N, (N, 80)), grid(Cn, (Cn, 80)))          # E = 80: one full chunk of 64 columns and a part of one


def test_assign_padded_rows_are_never_read():
    g, c = grid(1, (129, 48)), grid(2, (33, 48))
    check_exact(g, c, pad_g=8, pad_c=24)
    check_exact(g, c, pad_g=16, pad_c=0)
    check_exact(grid(3, (70, 2048)), grid(4, (130, 2048)), pad_g=8, pad_c=8)


def test_assign_one_centroid_repeated_gives_the_first():
    g = grid(5, (300, 48))
    a, _ = check_exact(g, np.tile(grid(6, (1, 48)), (300, 1)))
    assert not a.any()


def test_assign_duplicated_centroids_on_either_side_of_a_tile_border():
    c = grid(7, (300, 64)) / 4                       # |score| <= 64 * 0.125 * 0.5 = 4
    g = grid(8, (5, 64))
    g[:, 0] = 0.5
    best = np.sign(g[0]).astype(f32) / 2             # the centroid that row 0 likes best: score = sum |g| / 2
    assert float(cr.scores64(g[:1], best[None])[0, 0]) > 4
    for dup in ([127, 128], [126, 129], [255, 256, 299], [128, 127 + 128], [4, 36, 200]):      # tile borders at 128, 256
        h = c.copy()
        h[dup] = best
        a, _ = check_exact(g, h)
        assert a[0] == min(dup)


def test_assign_does_not_depend_on_the_other_rows_the_other_centroids_or_replay():
    g, c = grid(9, (700, 48)), grid(10, (340, 48))
    c[300:] = c[:40] / 2                                                    # the last 40 score half of what others score
    want, _ = cr.assign(g, c)
    assert (want < 300).all() and (cr.assign(g, c[:300])[1] > 0).all()      # ... which is lower: every best score is positive
    d = Assign(g, c)
    a, s = d.run(C_=300)
    assert np.array_equal(a, want)
    for lo, hi in ((0, 1), (1, 130), (130, 700), (699, 700), (128, 256)):   # slices of the rows
        a1, s1 = d.run(rows=(lo, hi), C_=300)
        assert np.array_equal(a1, a[lo:hi]) and np.array_equal(er.bits(s1), er.bits(s[lo:hi])), (lo, hi)
    a2, s2 = d.run()                                                        # 340 centroids: another tile count
    assert np.array_equal(a2, a) and np.array_equal(er.bits(s2), er.bits(s))
    # an eager launch and a captured graph replayed twice
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d.run(C_=300, sync=False)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            assign, score = d.run(C_=300, sync=False)
    for _ in range(2):
        assign.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(assign.cpu().numpy()[:700], a) and np.array_equal(er.bits(score.cpu().numpy()[:700]), er.bits(s))
        assert (assign.cpu().numpy()[700:] == -7).all()


@pytest.mark.parametrize("E", [64, 768])
def test_assign_on_random_data(E):
    """``band = E * 2^-23 * sum_e |g_e c_e|`` per (row, centroid): E exact products and at most E float32 additions at up to
    one ulp each (the matrix unit may truncate) -- check_band's derivation in test_gpu_embedding.py; nothing measured enters"""
    rng = np.random.default_rng(E)
    g = er.bf16_round(rng.standard_normal((2000, E)).astype(f32))
    c = er.bf16_round(rng.standard_normal((300, E)).astype(f32))
    a, s = Assign(g, c).run()
    assert ((a >= 0) & (a < 300)).all()
    ref = cr.scores64(g, c)
    band = E * 2.0 ** -23 * (np.abs(g.astype(np.float64)) @ np.abs(c.astype(np.float64)).T)
    rows = np.arange(2000)
    own, own_band = ref[rows, a], band[rows, a]
    print(f"E={E}: max |score - score64| / band = {float((np.abs(s - own) / own_band).max()):.3g}, "
          f"rows not at the float64 argmax: {int((a != ref.argmax(1)).sum())}")
    assert (np.abs(s - own) <= own_band).all()
    assert (own >= ref.max(1) - 2 * band.max(1)).all()


# ---- op level: segment mean -----------------------------------------------------------------------------------------------------
class Segments:
    """a gallery uploaded once (NaN padding); ``run`` calls tfimm_hip_segment_mean with guards behind mean, counts and the
    workspace and a sentinel in the padding columns of mean"""

    def __init__(self, g, pad_g=0, before=0, after=0):
        """``before`` / ``after``: NaN rows around the gallery inside one allocation"""
        self.N, self.E = g.shape
        self.ld_g = self.E + pad_g
        full = np.concatenate([np.full((before, self.E), np.nan, f32), g, np.full((after, self.E), np.nan, f32)])
        h = np.full((full.shape[0], self.ld_g), np.nan, f32)
        h[:, :self.E] = full
        self.buf = torch.from_numpy(h).cuda().bfloat16()
        self.ptr = self.buf.data_ptr() + 2 * before * self.ld_g
        assert self.ptr % 16 == 0

    @staticmethod
    def upload(rows, offsets):
        rows, offsets = np.asarray(rows, i32).reshape(-1), np.asarray(offsets, i32)
        return torch.from_numpy(np.concatenate([rows, np.zeros(1, i32)])).cuda(), torch.from_numpy(offsets).cuda()

    def run(self, rows, offsets, pad_m=0, sync=True):
        """``rows`` / ``offsets``: arrays, or the device tensors of ``upload`` (inside a capture nothing is uploaded)"""
        d_rows, d_off = (rows, offsets) if isinstance(rows, torch.Tensor) else self.upload(rows, offsets)
        M, nc, ld_m = d_rows.shape[0] - 1, d_off.shape[0] - 1, self.E + pad_m
        need = ffi.lib.tfimm_hip_segment_mean_workspace(M, nc, self.E)
        assert need > 0, ffi.lib.tfimm_hip_last_error().decode()
        work = torch.full((need + 16,), 0x5a, dtype=torch.uint8, device="cuda")
        mean = torch.full((nc * ld_m + GUARD,), -7.0, dtype=torch.float32, device="cuda")
        counts = torch.full((nc + GUARD,), -7, dtype=torch.int32, device="cuda")
        assert work.data_ptr() % 16 == 0
        ffi.check(ffi.lib.tfimm_hip_segment_mean(self.ptr, self.ld_g, self.N, self.E, d_rows.data_ptr(), M, d_off.data_ptr(), nc,
                                                 mean.data_ptr(), ld_m, counts.data_ptr(), work.data_ptr(), need, stream()),
                  "tfimm_hip_segment_mean")
        if not sync:
            return mean, counts, (d_rows, d_off, work)
        torch.cuda.synchronize()
        m, n = mean.cpu().numpy(), counts.cpu().numpy()
        assert (m[nc * ld_m:] == -7).all() and (n[nc:] == -7).all() and (work[need:] == 0x5a).all(), "a launch wrote behind a buffer"
        m = m[:nc * ld_m].reshape(nc, ld_m)
        assert (m[:, self.E:] == -7).all(), "a launch wrote into the padding of mean"
        return m[:, :self.E], n[:nc]


SIZES = (0, 1, 2, R - 1, R, R + 1, 3 * R + 5)


def segments(seed, N, sizes=SIZES):
    """segments of the given sizes in shuffled order over rows drawn from [0, N) with repetition: a row may appear in two
    segments, and twice in one -> (rows, offsets, sizes in their order)"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes)[rng.permutation(len(sizes))]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(i32)
    return rng.integers(0, N, int(offsets[-1])).astype(i32), offsets, sizes


def exact_mean(g, rows, offsets):
    """float32(sum64) / float32(count): what any order of exact additions gives"""
    g64 = g.astype(np.float64)
    out, counts = np.zeros((len(offsets) - 1, g.shape[1]), f32), np.zeros(len(offsets) - 1, i32)
    for c in range(len(offsets) - 1):
        r = np.asarray(rows[offsets[c]:offsets[c + 1]], np.int64)
        r = r[(r >= 0) & (r < g.shape[0])]
        counts[c] = r.size
        if r.size:
            out[c] = g64[r].sum(0).astype(f32) / f32(r.size)
    return out, counts


@pytest.mark.parametrize("E, pad_g, pad_m", [(16, 0, 0), (48, 8, 3), (2048, 16, 1), (64, 0, 0)])
def test_segment_mean_is_bit_equal_on_exact_data(E, pad_g, pad_m):
    g = grid(E, (600, E))
    rows, offsets, sizes = segments(E + 1, 600)
    mean, counts = Segments(g, pad_g).run(rows, offsets, pad_m)
    want, want_n = exact_mean(g, rows, offsets)
    assert counts.tolist() == want_n.tolist() == sizes.tolist()
    assert np.array_equal(er.bits(mean), er.bits(want))
    assert not er.bits(mean[sizes == 0]).any()                              # an empty segment: +0.0


def test_segment_mean_one_segment_all_empty_and_no_entries():
    g = grid(11, (300, 32))
    d = Segments(g)
    rows = np.random.default_rng(12).integers(0, 300, 2 * R + 3).astype(i32)
    mean, counts = d.run(rows, [0, rows.size])                              # C = 1
    want, _ = exact_mean(g, rows, [0, rows.size])
    assert counts.tolist() == [rows.size] and np.array_equal(er.bits(mean), er.bits(want))
    mean, counts = d.run(rows, [5, 5, 5, 5])                                # all segments empty
    assert not counts.any() and not er.bits(mean).any()
    mean, counts = d.run(rows, [7, 3, 3, rows.size + 50, 2])                # ends below begins; an end beyond M is M
    want, want_n = exact_mean(g, rows, [7, 7, 3, rows.size, rows.size])
    assert counts.tolist() == [0, 0, rows.size - 3, 0] and np.array_equal(er.bits(mean), er.bits(want))
    mean, counts = d.run(np.zeros(0, i32), [0, 0, 0])                       # M = 0
    assert not counts.any() and not er.bits(mean).any() and mean.shape == (2, 32)


@pytest.mark.parametrize("E", [64, 512])
def test_segment_mean_on_random_data(E):
    """bit-equal to the stated order (cluster_ref.segment_mean), and per element within ``gamma_n * (sum_i |x_i|) / n`` of the
    float64 mean, ``gamma_n = n u / (1 - n u)``, ``u = 2^-24``: n - 1 additions and one division; nothing measured enters.
    A segment's bits do not depend on the other segments, nor on eager launch or replay."""
    rng = np.random.default_rng(E)
    g = er.bf16_round(rng.standard_normal((5000, E)).astype(f32))
    rows, offsets, sizes = segments(E + 2, 5000)
    d = Segments(g)
    mean, counts = d.run(rows, offsets)
    want, want_n = cr.segment_mean(g, rows, offsets)
    assert counts.tolist() == want_n.tolist() == sizes.tolist()
    assert np.array_equal(er.bits(mean), er.bits(want))
    m64, mass = cr.mean64(g, rows, offsets)
    n = np.maximum(sizes, 1)[:, None].astype(np.float64)
    u = 2.0 ** -24
    bound = n * u / (1 - n * u) * mass / n
    print(f"E={E}: max |mean - mean64| / bound = {float((np.abs(mean - m64)[sizes > 0] / bound[sizes > 0]).max()):.3g}")
    assert (np.abs(mean - m64) <= bound).all()
    # every segment alone; alone behind an empty one; the list of a segment moved to another place of rows
    for c in range(len(sizes)):
        own = rows[offsets[c]:offsets[c + 1]]
        m1, n1 = d.run(own, [0, own.size])
        assert n1.tolist() == [sizes[c]] and np.array_equal(er.bits(m1[0]), er.bits(mean[c])), c
        m2, _ = d.run(np.concatenate([rows[:77], own]), [0, 0, 77, 77 + own.size])
        assert np.array_equal(er.bits(m2[2]), er.bits(mean[c])), c
    # eager and replayed from a graph
    side = torch.cuda.Stream()
    up = d.upload(rows, offsets)
    with torch.cuda.stream(side):
        d.run(*up, sync=False)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            dm, dn, keep = d.run(*up, sync=False)
    for _ in range(2):
        dm.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(er.bits(dm.cpu().numpy()[:len(sizes) * E].reshape(-1, E)), er.bits(mean))
        assert dn.cpu().numpy()[:len(sizes)].tolist() == sizes.tolist()


def test_segment_mean_entries_outside_the_gallery_are_not_read_and_not_counted():
    """the gallery is a slice in the middle of a larger allocation whose other rows are NaN: the entries -1, N and N + 3 point
    into that allocation -- a kernel that used them shows NaN and a wrong count, and never leaves the buffer"""
    N, E = 200, 64
    g = grid(13, (N, E))
    d = Segments(g, before=4, after=8)
    rows, offsets, sizes = segments(14, N, (0, 5, R + 1, 40))
    rows = rows.copy()
    hit = np.random.default_rng(15).choice(rows.size, 30, replace=False)
    rows[hit] = np.resize(np.array([-1, N, N + 3, -4, N + 7], i32), 30)
    first = int(offsets[np.flatnonzero(sizes == 5)[0]])
    rows[first:first + 5] = [-1, N, N + 3, -1, N]                           # a segment of nothing but entries outside
    mean, counts = d.run(rows, offsets)
    want, want_n = exact_mean(g, rows, offsets)
    assert np.isfinite(mean).all() and counts.tolist() == want_n.tolist() and counts.sum() < sizes.sum()
    assert np.array_equal(er.bits(mean), er.bits(want))
    five = int(np.flatnonzero(sizes == 5)[0])
    assert counts[five] == 0 and not er.bits(mean[five]).any()


# ---- prototypes and k-means end to end, on planted data ---------------------------------------------------------------------
SIZES_PLANTED = [1, 3, 40, 64, 65, 127, 300, 700]


@pytest.fixture(scope="module")
def planted():
    """8 clusters around the first unit vectors of R^64, noise 0.05: in float64 the planted partition is the argmax at every
    pass, with a smallest margin of 0.58 against a band of 8e-6 -- only a wrong kernel can change it"""
    rng = np.random.default_rng(7)
    E, K = 64, 8
    label = np.repeat(np.arange(K), SIZES_PLANTED)
    label = label[rng.permutation(label.size)]
    x = np.eye(K, E)[label] + 0.05 * rng.standard_normal((label.size, E))
    x = er.bf16_round(er.l2_normalize(x).astype(f32))
    gallery = tfimm.Gallery(E)
    gallery.add(x, label)
    first = np.array([np.flatnonzero(label == c)[0] for c in range(K)])
    return gallery, x, label.astype(i32), first


def test_prototypes_are_bit_equal_and_classify_every_row(planted):
    gallery, x, label, _ = planted
    p = gallery.prototypes(nb_classes=10)
    want, want_lab = cr.prototypes(x, label, 10)
    assert isinstance(p, tfimm.Gallery) and len(p) == 10 and p.labelled and p.dim == 64
    assert np.array_equal(er.bits(p.numpy()), er.bits(want)) and p.labels().tolist() == want_lab.tolist()
    assert not er.bits(p.numpy()[8:]).any() and p.labels()[8:].tolist() == [-1, -1]
    m = p.search(x, 1)
    assert np.array_equal(m.indices.numpy()[:, 0], label)
    assert np.array_equal(p.classify(x[:50], k=1, top=1).classes.numpy()[:, 0], label[:50])      # nearest class mean
    # nb_classes read from the device; not normalised: the means themselves, rounded
    q = gallery.prototypes()
    assert len(q) == 8 and np.array_equal(er.bits(q.numpy()), er.bits(want[:8]))
    raw, _ = cr.prototypes(x, label, 8, normalize=False)
    assert np.array_equal(er.bits(gallery.prototypes(8, normalize=False).numpy()), er.bits(raw))


def test_kmeans_recovers_the_planted_clusters_bit_for_bit(planted):
    gallery, x, label, first = planted
    one = gallery.kmeans(8, iters=1, init=first)
    want = cr.kmeans(x, x[first], 1)
    assert np.array_equal(one.assignment.numpy(), label) and one.counts.numpy().tolist() == SIZES_PLANTED
    assert np.array_equal(er.bits(one.centroids.numpy()), er.bits(want[0]))
    assert one.centroids.labelled and one.centroids.labels().tolist() == list(range(8)) and one.moved.numpy().tolist() == [0]
    assert one.assignment.numpy().dtype == i32 and one.counts.numpy().dtype == i32 and one.moved.numpy().dtype == i32
    result = gallery.kmeans(8, iters=3, init=first)
    assert result.moved.numpy().tolist() == [0, 0, 0]
    again = gallery.kmeans(8, iters=3, init=first)
    assigned = gallery.assign(result.centroids)
    for r in (one, again):
        assert np.array_equal(er.bits(r.centroids.numpy()), er.bits(result.centroids.numpy()))
        assert np.array_equal(r.assignment.numpy(), result.assignment.numpy())
        assert np.array_equal(er.bits(r.scores.numpy()), er.bits(result.scores.numpy()))
        assert np.array_equal(r.counts.numpy(), result.counts.numpy())
    assert np.array_equal(assigned.clusters.numpy(), result.assignment.numpy())
    assert np.array_equal(er.bits(assigned.scores.numpy()), er.bits(result.scores.numpy()))
    # the other forms of init give the same centroids: values as an array, as a Tensor on the device, as a Gallery
    seeds = tfimm.Gallery(64)
    seeds.add(x[first])
    for init in (x[first], tfimm.Tensor(torch.from_numpy(x[first]).cuda()), seeds):
        r = gallery.kmeans(8, iters=1, init=init)
        assert np.array_equal(er.bits(r.centroids.numpy()), er.bits(one.centroids.numpy()))
    assert np.array_equal(gallery.kmeans(8, iters=0, init=first).assignment.numpy(), label)       # iters = 0 only assigns


def test_kmeans_from_a_seeded_start_keeps_its_invariants(planted):
    """seed 0 puts several seeds into one planted cluster: recovery is not expected, the invariants are"""
    gallery, x, label, _ = planted
    r = gallery.kmeans(8, iters=4, seed=0)
    a, n, cen = r.assignment.numpy(), r.counts.numpy(), r.centroids.numpy()
    assert n.tolist() == np.bincount(a, minlength=8).tolist() and n.sum() == len(gallery) and r.moved.numpy().shape == (4,)
    ref = cr.scores64(x, cen)
    band = 64 * 2.0 ** -23 * (np.abs(x.astype(np.float64)) @ np.abs(cen.astype(np.float64)).T)
    rows = np.arange(len(x))
    assert (ref[rows, a] >= ref.max(1) - 2 * band.max(1)).all()
    assert (np.abs(r.scores.numpy() - ref[rows, a]) <= band[rows, a]).all()
    start = cr.normalize_bf16(x[np.random.default_rng(0).choice(len(x), 8, replace=False)])
    for j in np.flatnonzero(n == 0):
        assert np.array_equal(er.bits(cen[j]), er.bits(start[j]))
    # an empty cluster for certain: a ninth start opposite to all eight directions scores about -0.35 where the row's own
    # seed scores about 1; it keeps its centroid through the updates, and the planted partition is what it was
    _, _, _, first = planted
    far = -np.eye(8, 64, dtype=f32).sum(0, keepdims=True)
    init = np.concatenate([x[first], far])
    e = gallery.kmeans(9, iters=2, init=init)
    assert e.counts.numpy().tolist() == SIZES_PLANTED + [0] and np.array_equal(e.assignment.numpy(), label)
    assert np.array_equal(er.bits(e.centroids.numpy()[8]), er.bits(cr.normalize_bf16(far)[0]))
    assert np.array_equal(er.bits(e.centroids.numpy()), er.bits(cr.kmeans(x, init, 2)[0]))


def test_set_labels_lets_the_knn_end_answer_with_clusters(planted):
    _, x, label, first = planted
    gallery = tfimm.Gallery(64)
    gallery.add(x)                                                          # an unlabelled gallery
    result = gallery.kmeans(8, iters=3, init=first)
    assert not gallery.labelled
    gallery.set_labels(result.assignment)
    assert gallery.labelled and np.array_equal(gallery.labels(), label)
    some = np.concatenate([first, [5, 50, 500, 1000]])
    votes = gallery.classify(x[some], k=5)
    assert np.array_equal(votes.classes.numpy()[:, 0], label[some])
    gallery.set_labels(np.zeros(len(x), np.int64))                          # host labels replace them
    assert not gallery.labels().any()

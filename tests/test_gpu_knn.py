"""pytest -m gpu: the kNN end on the device.  tfimm_hip_knn_vote / tfimm_hip_knn_score (csrc/knn.hip) on
hand-made matches against the written rule of tests/knn_ref.py -- bit-equal wherever expf is exact, under bars computed from
the shape where it is not --, the meter's integer state, and ``tfimm.Gallery`` / ``tfimm.EmbeddingModel`` end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

import embed_ref as er
import knn_ref as kr
import model_checks as mc
import score_ref as sr
import test_architectures  # noqa: F401
import tfimm
from tfimm.engine import ffi
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu
f32, i32 = np.float32, np.int32
GUARD = 8          # elements behind every output buffer that a launch must leave alone
U = 2.0 ** -24     # unit roundoff of float32
INV_T = float(f32(1.0) / f32(0.07))
TOPMOST = 2 ** 31 - 1


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(bits(u), bits(v)) if u.dtype == f32 else np.array_equal(u, v) for u, v in zip(a, b))


class Matches:
    """hand-made matches uploaded once: indices int32 / scores float32 [B][k + pad] -- the padding columns hold a row that
    would vote and NaN: a launch that read them would show it -- and the gallery's labels as the LAST N elements of their
    allocation, so that an index >= N used as one would read past its end."""

    def __init__(self, indices, scores, glabels, pad=0, exclude=None):
        indices, scores = np.ascontiguousarray(indices, i32), np.ascontiguousarray(scores, f32)
        self.B, self.k = indices.shape
        self.ld, self.N = self.k + pad, len(glabels)
        hi, hs = np.zeros((self.B, self.ld), i32), np.full((self.B, self.ld), np.nan, f32)
        hi[:, :self.k], hs[:, :self.k] = indices, scores
        self.indices, self.scores = torch.from_numpy(hi).cuda(), torch.from_numpy(hs).cuda()
        room = torch.full((1 << 19,), 3, dtype=torch.int32, device="cuda")          # 2 MiB: a block of its own
        self.glabels = room[room.numel() - self.N:]
        self.glabels.copy_(torch.from_numpy(np.ascontiguousarray(glabels, i32)))
        self._room = room
        self.exclude = None if exclude is None else torch.from_numpy(np.ascontiguousarray(exclude, i32)).cuda()

    def _common(self, lo, B, inv_t):
        ex = None if self.exclude is None else self.exclude.data_ptr() + 4 * lo
        return (self.indices.data_ptr() + 4 * lo * self.ld, self.scores.data_ptr() + 4 * lo * self.ld, self.ld, B, self.k,
                self.glabels.data_ptr(), self.N, ex, inv_t)

    def vote(self, inv_t=0.0, reduce=kr.SUM, top=5, rows=None, sync=True):
        lo, hi = (0, self.B) if rows is None else rows
        B = hi - lo
        outs = [torch.full((n + GUARD,), -7, dtype=dt, device="cuda") for n, dt in
                ((B * top, torch.int32), (B * top, torch.float32), (B * top, torch.int32), (B, torch.float32))]
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_knn_vote(*self._common(lo, B, inv_t), reduce, top, *(t.data_ptr() for t in outs), st),
                  "tfimm_hip_knn_vote")
        if not sync:
            return outs
        torch.cuda.synchronize()
        return self.read(outs, B, top)

    @staticmethod
    def read(outs, B, top):
        res = []
        for t, shape in zip(outs, ((B, top), (B, top), (B, top), (B,))):
            a, n = t.cpu().numpy(), int(np.prod(shape))
            assert (a[n:] == -7).all(), "the launch wrote behind an output"
            res.append(a[:n].reshape(shape))
        return tuple(res)

    def score(self, labels, nb_classes, inv_t=0.0, rows=None, state=None, per_class=None, confusion=None):
        lo, hi = (0, self.B) if rows is None else rows
        B = hi - lo
        y = torch.from_numpy(np.asarray(labels, np.int64)[lo:hi].astype(i32)).cuda()
        outs = [torch.full((B + GUARD,), -7, dtype=dt, device="cuda") for dt in (torch.float32, torch.int32, torch.int32, torch.float32)]
        acc = [None if t is None else t.data_ptr() for t in (state, per_class, confusion)]
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_knn_score(*self._common(lo, B, inv_t), nb_classes, y.data_ptr(), *(t.data_ptr() for t in outs),
                                              *acc, st), "tfimm_hip_knn_score")
        torch.cuda.synchronize()
        res = []
        for t in outs:
            a = t.cpu().numpy()
            assert (a[B:] == -7).all(), "the launch wrote behind an output"
            res.append(a[:B])
        return tuple(res)


N_GALLERY = 200
PATTERNS = {
    "one": np.full(N_GALLERY, 7),
    "distinct": np.arange(N_GALLERY) * 3 + 1,
    "two": np.where(np.arange(N_GALLERY) % 2 == 0, 5, 2),
    "huge": TOPMOST - np.arange(N_GALLERY) % 3,
    "minus": np.where(np.arange(N_GALLERY) % 4 == 1, -1, np.arange(N_GALLERY) % 7),
}


def _rows(seed, B, k, N=N_GALLERY):
    """k distinct gallery rows per query, as a search returns them"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(N, k, replace=False) for _ in range(B)]).astype(i32)


def _grid_scores(seed, B, k):
    """scores from {-4 ... 4} / 8, both zeros among them"""
    rng = np.random.default_rng(seed)
    s = (rng.integers(-4, 5, (B, k)) / 8).astype(f32)
    s[(s == 0) & (rng.integers(0, 2, (B, k)) == 1)] = -0.0
    return s


def _check_lists(got, want, top):
    """the first ``top`` slots of the reference's full list (it was computed with top = 64), bit for bit"""
    for g, w in zip(got[:3], want[:3]):
        assert g.shape == w[:, :top].shape
        assert np.array_equal(bits(g), bits(w[:, :top])) if g.dtype == f32 else np.array_equal(g, w[:, :top]), (g[:2], w[:2, :top])
    assert np.array_equal(bits(got[3]), bits(want[3]))


# ---- exact cases: weights of 1, and MAX ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 5, 63, 64])
@pytest.mark.parametrize("B", [1, 4, 5, 70])
def test_exact_votes_are_bit_equal_to_the_rule(B, k):
    idx, sc = _rows(B * 100 + k, B, k), _grid_scores(B + k, B, k)
    for name, glabels in PATTERNS.items():
        m = Matches(idx, sc, glabels)
        for reduce in (kr.SUM, kr.MAX):
            want = kr.vote(idx, sc, glabels.astype(i32), reduce=reduce, top=64)
            for top in (1, 5, 64):
                _check_lists(m.vote(0.0, reduce, top), want, top)
            if reduce == kr.SUM:                                                # every weight is 1: counts, as floats
                assert np.array_equal(want[1], want[2].astype(f32)) and (want[3] <= k).all()
            else:
                assert not want[3].any() and not np.signbit(want[3]).any()


def test_the_excluded_row_never_votes():
    B, k = 6, 5
    idx, sc = _rows(11, B, k), _grid_scores(12, B, k)
    glabels = PATTERNS["minus"].astype(i32)
    absent = [int(np.setdiff1d(np.arange(N_GALLERY), idx[b])[0]) for b in range(B)]
    exclude = np.array([idx[0, 0], idx[1, k - 1], absent[2], -1, idx[4, 2], absent[5]], i32)      # present, absent, none
    m = Matches(idx, sc, glabels, exclude=exclude)
    for reduce in (kr.SUM, kr.MAX):
        want = kr.vote(idx, sc, glabels, exclude=exclude, reduce=reduce, top=64)
        plain = kr.vote(idx, sc, glabels, reduce=reduce, top=64)
        assert not np.array_equal(want[2], plain[2])                            # the exclusion changes the answer
        _check_lists(m.vote(0.0, reduce, 5), want, 5)
    # the whole list excluded or unlabelled: no valid candidate
    one = Matches(idx[:2, :1], sc[:2, :1], glabels, exclude=idx[:2, 0])
    c, v, n, t = one.vote(0.0, kr.SUM, 3)
    assert (c == -1).all() and not bits(v).any() and not n.any() and not bits(t).any()


def test_indices_outside_the_gallery_read_no_label():
    B, k = 5, 6
    idx, sc = _rows(21, B, k), _grid_scores(22, B, k)
    idx[0, 1], idx[1, 0], idx[2, 5], idx[3, 2], idx[4, :] = -1, N_GALLERY, TOPMOST, -2 ** 31, [-5, N_GALLERY + 1, -1, 2 ** 30, N_GALLERY, -7]
    for name in ("two", "huge"):
        glabels = PATTERNS[name].astype(i32)
        m = Matches(idx, sc, glabels)
        for reduce in (kr.SUM, kr.MAX):
            want = kr.vote(idx, sc, glabels, reduce=reduce, top=64)
            assert (want[0][4] == -1).all() and want[2][:4].sum() == 4 * k - 4
            _check_lists(m.vote(0.0, reduce, 5), want, 5)
    loss, rank, pred, prob = m.score([0, 1, -1, 5, 3], 8)                       # no label is below 8: nobody votes
    assert rank.tolist() == [0, 1, -1, 5, 3] and not pred.any() and not bits(prob).any()
    assert np.isposinf(loss[[0, 1, 3, 4]]).all() and bits(loss)[2] == 0


@pytest.mark.parametrize("pad", [1, 3, 64])
def test_padding_columns_are_never_read(pad):
    B, k = 5, 7
    idx, sc = _rows(31, B, k), _grid_scores(32, B, k)
    glabels = PATTERNS["minus"].astype(i32)
    want = Matches(idx, sc, glabels).vote(0.0, kr.MAX, 5)
    assert _same(Matches(idx, sc, glabels, pad=pad).vote(0.0, kr.MAX, 5), want)
    want = Matches(idx, sc, glabels).vote(INV_T, kr.SUM, 5)
    got = Matches(idx, sc, glabels, pad=pad).vote(INV_T, kr.SUM, 5)
    assert _same(got, want) and np.isfinite(got[1]).all() and np.isfinite(got[3]).all()


# ---- weighted cases ----------------------------------------------------------------------------------------------------------
def value_bar(k, inv_t, spread=2.0):
    """Relative error of a class sum (and of the total) of ``w_j = expf((s_j - m) * inv_t)`` against the float64 rule, for
    scores ``spread`` apart at most: with ``a_max = spread * inv_t`` the largest magnitude of an exponent,

        a_max u      the rounding of ``s_j - m``: u relative on a difference whose product with inv_t is at most a_max, an
                     absolute error of the exponent, which the exponential turns into the same RELATIVE error of w_j
      + a_max u      the rounding of the product, likewise
      + 2 u          expf
      + (k - 1) u    at most k - 1 additions of non-negative terms, u relative each
      + 4 u          slack, for the second-order terms.
    ``(2 a_max + 2 + k + 4) u`` bounds it.  Nothing measured enters it."""
    return (2 * spread * inv_t + 2 + k + 4) * U


def _weighted_case(seed, B, k, classes=10):
    rng = np.random.default_rng(seed)
    idx = _rows(seed + 1, B, k)
    sc = rng.uniform(-1, 1, (B, k)).astype(f32)
    glabels = rng.integers(0, classes, N_GALLERY).astype(i32)
    return idx, sc, glabels


@pytest.mark.parametrize("k", [20, 64])
def test_weighted_votes_within_the_bar_of_the_float64_rule(k):
    B, classes = 70, 10
    idx, sc, glabels = _weighted_case(40 + k, B, k)
    bar = value_bar(k, INV_T)
    c, v, n, t = Matches(idx, sc, glabels).vote(INV_T, kr.SUM, 64)
    want_v, want_t = kr.dense(idx, sc, glabels, classes, inv_temperature=INV_T, dtype=np.float64)
    want_c, _, want_n, _ = kr.vote(idx, sc, glabels, inv_temperature=INV_T, top=64, dtype=np.float64)
    worst = 0.0
    for b in range(B):
        d = int((c[b] >= 0).sum())
        assert d == int((want_c[b] >= 0).sum()) and (c[b, d:] == -1).all() and not bits(v[b, d:]).any() and not n[b, d:].any()
        cls, val = c[b, :d], v[b, :d].astype(np.float64)
        assert len(set(cls.tolist())) == d and set(cls.tolist()) == set(want_c[b, :d].tolist())          # distinct, the same set
        assert dict(zip(cls.tolist(), n[b, :d].tolist())) == dict(zip(want_c[b, :d].tolist(), want_n[b, :d].tolist()))
        ref = want_v[b, cls]
        worst = max(worst, float((np.abs(val - ref) / ref).max()), abs(float(t[b]) - want_t[b]) / want_t[b])
        assert (np.diff(v[b, :d]) <= 0).all()                                                             # non-increasing
        assert all(cls[p] < cls[p + 1] for p in range(d - 1) if v[b, p] == v[b, p + 1])                    # ties by class
        best = np.sort(want_v[b][want_v[b] > 0])[::-1]
        assert (ref >= best[:d] * (1 - 2 * bar)).all()                     # position p holds a class as good as the p-th best
    print(f"knn vote k={k}: max relative error {worst / U:.2f} u, bar {bar / U:.1f} u")
    assert worst <= bar


def test_separated_values_give_the_reference_s_classes_exactly():
    """5 classes of 4 candidates each, every candidate of class c at score -0.05 c: the values 4 exp(-0.05 c / 0.07) lie a
    factor two apart -- far more than twice the bar, which is asserted before the launch -- so the order is the reference's"""
    k, B = 20, 9
    rng = np.random.default_rng(51)
    glabels = (np.arange(N_GALLERY) % 5 * 11 + 3).astype(i32)               # classes 3, 14, 25, 36, 47
    idx = np.stack([rng.permutation(np.concatenate([rng.choice(np.arange(c, N_GALLERY, 5), 4, replace=False) for c in range(5)]))
                    for _ in range(B)]).astype(i32)
    sc = (-0.05 * (glabels[idx] // 11)).astype(f32)
    want = kr.vote(idx, sc, glabels, inv_temperature=INV_T, top=5, dtype=np.float64)
    bar = value_bar(k, INV_T)
    assert (want[1][:, 1:] < want[1][:, :-1] * (1 - 2 * bar)).all() and (want[2] == 4).all()
    c, v, n, t = Matches(idx, sc, glabels).vote(INV_T, kr.SUM, 5)
    assert np.array_equal(c, want[0]) and np.array_equal(n, want[2])
    assert (np.abs(v - want[1]) <= bar * want[1]).all() and (np.abs(t - want[3]) <= bar * want[3]).all()


def _underflow_case():
    """one candidate 0.1 above all others and inv_temperature = 1e4: every other exponent is below -1000, far under the
    -104 where expf still returns a denormal: all weights but the maximum's are exactly 0"""
    B, k = 8, 12
    idx = _rows(61, B, k)
    sc = np.random.default_rng(62).uniform(-1, 0.8, (B, k)).astype(f32)
    sc[np.arange(B), np.arange(B) % k] = 0.9
    glabels = (np.arange(N_GALLERY) % 9).astype(i32)
    return idx, sc, glabels


def test_underflowed_weights_are_exactly_zero_and_tie_by_class():
    idx, sc, glabels = _underflow_case()
    want = kr.vote(idx, sc, glabels, inv_temperature=1e4, top=64)
    assert (want[1][:, 0] == 1).all() and not want[1][:, 1:].any() and (want[2][:, 1] > 0).all() and (want[3] == 1).all()
    assert all((np.diff(row[1:][row[1:] >= 0]) > 0).all() for row in want[0])           # behind the winner: ascending class
    m = Matches(idx, sc, glabels)
    _check_lists(m.vote(1e4, kr.SUM, 64), want, 64)
    _check_lists(m.vote(1e4, kr.SUM, 3), want, 3)
    # scored: a voted class of value 0 ties with the unvoted ones; every class as the label in turn
    for shift in range(9):
        y = (np.arange(8) + shift) % 11
        loss, rank, pred, prob = m.score(y, 11, inv_t=1e4)
        v, total = kr.dense(idx, sc, glabels, 11, inv_temperature=1e4)
        _, want_rank, want_pred, _ = sr.score(v, y)
        assert np.array_equal(rank, want_rank) and np.array_equal(pred, want_pred)
        assert np.array_equal(prob, v[np.arange(8), y]) and set(prob.tolist()) <= {0.0, 1.0}
        assert np.array_equal(bits(loss), bits(np.where(prob == 1, f32(0), f32(np.inf))))     # +0.0 and +inf


# ---- scoring -------------------------------------------------------------------------------------------------------------------
def loss_bar(k, loss):
    """Absolute error of the float32 ``0 - logf(prob)`` against ``-log`` of the float64 share, where the device's ``prob`` is
    within ``(k + 4) u`` relative of that share (the bar on ``prob`` below):

        (k + 4) u      the logarithm turns the relative error of its argument into the same absolute error
      + 2 u |loss|     logf: 2 u relative on a value of magnitude |loss|
      + 1 u |loss|     the subtraction from 0
      + 1 u            slack, for the second-order terms.
    Nothing measured enters it."""
    return ((k + 4) + 3 * abs(loss) + 1) * U


def _scoring_case(k):
    """70 queries over 12 classes; gallery labels 12 and 13 (not below nb_classes) and -1 never vote; the true labels visit
    voted and unvoted classes, -1, nb_classes and beyond"""
    B, classes = 70, 12
    idx, sc = _rows(70 + k, B, k), _grid_scores(71 + k, B, k)
    glabels = np.random.default_rng(72).choice([-1, 0, 2, 3, 5, 7, 8, 11, 12, 13], N_GALLERY).astype(i32)     # 1, 4, 6, 9, 10: never voted
    y = np.random.default_rng(73 + k).integers(0, classes, B)
    y[[3, 17, 30, 44]] = [-1, classes, -2, TOPMOST]
    return idx, sc, glabels, y, classes


@pytest.mark.parametrize("k", [5, 64])
def test_scores_rank_and_pred_are_score_ref_on_the_dense_vote(k):
    idx, sc, glabels, y, classes = _scoring_case(k)
    loss, rank, pred, prob = Matches(idx, sc, glabels).score(y, classes)
    v, total = kr.dense(idx, sc, glabels, classes)                          # counts: rows full of ties, zeros for the unvoted
    _, want_rank, want_pred, _ = sr.score(v, y)
    assert np.array_equal(rank, want_rank) and np.array_equal(pred, want_pred)
    assert rank[[3, 17, 30, 44]].tolist() == [-1, -2, -2, -2]
    ref = kr.score(idx, sc, glabels, y, classes, dtype=np.float64)
    assert np.array_equal(ref[1], rank) and np.array_equal(ref[2], pred)   # the counted rank of the rule is score_ref's
    on = rank >= 0
    unvoted = on & (v[np.arange(70), np.clip(y, 0, classes - 1)] == 0)
    assert unvoted.any() and (on & ~unvoted).any() and (rank[on] > 0).any() and (rank[on] == 0).any()
    assert not bits(loss[~on]).any() and not bits(prob[~on]).any()
    assert not bits(prob[unvoted]).any() and np.isposinf(loss[unvoted]).all()
    hit = on & ~unvoted
    assert (np.abs(prob[hit] - ref[3][hit]) <= (k + 4) * U * ref[3][hit]).all()
    err = np.abs(loss[hit].astype(np.float64) - ref[0][hit])
    assert all(e <= loss_bar(k, w) for e, w in zip(err, ref[0][hit])) and not np.signbit(loss).any()
    print(f"knn score k={k}: loss max absolute error {err.max() / U:.2f} u")


def test_rank_among_two_billion_classes_is_counted_not_looped():
    idx, sc = _rows(81, 4, 6), _grid_scores(82, 4, 6)
    glabels = PATTERNS["huge"].astype(i32)                                   # classes 2^31 - 1, - 2, - 3
    y = [TOPMOST - 1, 12345, TOPMOST - 3, 0]
    loss, rank, pred, prob = Matches(idx, sc, glabels).score(y, TOPMOST)      # class 2^31 - 1 is not below nb_classes
    want = kr.score(idx, sc, glabels, y, TOPMOST)
    assert np.array_equal(rank, want[1]) and np.array_equal(pred, want[2]) and np.array_equal(bits(prob), bits(want[3]))
    voted = [len({int(g) for g in glabels[row] if g < TOPMOST}) for row in idx]      # distinct voting classes per query
    assert min(voted) >= 1 and (pred >= TOPMOST - 2).all()
    # an unvoted class ties with every other unvoted one: all of those below it come first, behind the voted ones
    assert rank[1] == voted[1] + 12345 and rank[2] == voted[2] + TOPMOST - 3 and rank[3] == voted[3] and rank[0] <= 1


def _state(m, y, classes, rows_list, inv_t=0.0):
    bufs = [torch.zeros(n, dtype=dt, device="cuda") for n, dt in
            ((sr.STATE_WORDS, torch.int64), (2 * classes, torch.int64), (classes * classes, torch.int32))]
    outs = [m.score(y, classes, inv_t, rows=r, state=bufs[0], per_class=bufs[1], confusion=bufs[2]) for r in rows_list]
    return [np.concatenate(o) for o in zip(*outs)], [b.cpu().numpy() for b in bufs]


def test_meter_state_is_the_rule_and_does_not_depend_on_split_or_order():
    idx, sc, glabels, y, classes = _scoring_case(5)
    m = Matches(idx, sc, glabels)
    (loss, rank, pred, prob), got = _state(m, y, classes, [(0, 70)])
    words, per_class, confusion = sr.state(loss, rank, y, classes, pred)
    assert np.array_equal(got[0], words) and np.array_equal(got[1].reshape(2, classes), per_class)
    assert np.array_equal(got[2].reshape(classes, classes), confusion)
    assert (words[sr.SCORED], words[sr.IGNORED], words[sr.INVALID]) == (66, 1, 3) and words[sr.LOSS_EXCLUDED] > 0
    for split in ([(0, 33), (33, 70)], [(b, b + 1) for b in range(70)], [(b, b + 1) for b in range(69, -1, -1)]):
        _, other = _state(m, y, classes, split)
        assert all(np.array_equal(a, b) for a, b in zip(got, other))
    # the weighted vote, too: its per-row bits do not depend on the batch, so neither does the sum of the losses
    _, one = _state(m, y, classes, [(0, 70)], INV_T)
    _, many = _state(m, y, classes, [(b, b + 7) for b in range(0, 70, 7)], INV_T)
    assert all(np.array_equal(a, b) for a, b in zip(one, many)) and one[0][sr.LOSS_Q] > 0


# ---- independence --------------------------------------------------------------------------------------------------------------
def test_rows_are_independent_of_the_batch_and_replays_are_bit_equal():
    idx, sc, glabels = _weighted_case(91, 70, 20)
    m = Matches(idx, sc, glabels)
    whole = m.vote(INV_T, kr.SUM, 5)
    for b in range(70):
        assert _same([a[b:b + 1] for a in whole], m.vote(INV_T, kr.SUM, 5, rows=(b, b + 1))), b
    for _ in range(3):
        assert _same(whole, m.vote(INV_T, kr.SUM, 5))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = m.vote(INV_T, kr.SUM, 5, sync=False)
    for _ in range(3):
        for t in outs:
            t[:70].fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(whole, Matches.read(outs, 70, 5))


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def grid(seed, shape):
    """entries from {-4 ... 4} / 8: exact in bf16, every score exact in float32 (tests/test_gpu_embedding.py)"""
    return (np.random.default_rng(seed).integers(-4, 5, shape) / 8).astype(f32)


def _labelled_gallery(n=300, dim=32, classes=9):
    rows = grid(101, (n, dim))
    labels = np.random.default_rng(102).integers(-1, classes, n).astype(i32)
    g = tfimm.Gallery(dim)
    assert not g.labelled
    assert g.add(rows[:100], labels[:100].tolist()) == range(0, 100) and g.labelled        # a list, int64 on the device, int32
    g.add(rows[100:150], torch.from_numpy(labels[100:150].astype(np.int64)).cuda())
    g.add(torch.from_numpy(rows[150:]), labels[150:])
    assert np.array_equal(g.labels(), labels) and g.labels().dtype == i32 and np.array_equal(g.numpy(), rows)
    return g, rows, labels


_REDUCE = {"sum": kr.SUM, "max": kr.MAX}


def _votes(v):
    return tuple(t.numpy() for t in v)


def test_classify_is_vote_of_search_and_the_rule_on_the_reference_search():
    g, rows, labels = _labelled_gallery()
    q = grid(103, (33, 32))
    for k, temperature, reduce, top in ((20, None, "sum", 5), (7, None, "max", 3), (64, 0.07, "max", 64), (20, 0.07, "sum", 5)):
        got = g.classify(q, k, temperature, top, reduce)
        m = g.search(q, k)
        assert _same(_votes(got), _votes(g.vote(m, temperature, top, reduce)))
        assert all(t.torch().is_cuda for t in got) and got.classes.shape == (33, top) and got.total.shape == (33,)
        idx, sc = er.search(q, rows, k)
        assert np.array_equal(m.indices.numpy(), idx) and np.array_equal(g.labels_of(m.indices).numpy(), labels[idx])
        if temperature is None or reduce == "max":                             # expf is not involved: bit-equal to the rule
            want = kr.vote(idx, sc, labels, reduce=_REDUCE[reduce], top=top)
            assert _same(_votes(got), want)
    e = g.classify(np.zeros((0, 32), f32), 5)
    assert e.classes.shape == (0, 5) and e.total.shape == (0,)


def test_leave_one_out_the_self_row_never_votes():
    g, rows, labels = _labelled_gallery()
    q = rows[:40] + f32(0)
    ex = np.arange(40)
    idx, sc = er.search(q, rows, 21)
    assert (idx == ex[:, None]).any(1).sum() >= 30                              # most rows find themselves
    for exclude in (ex.tolist(), torch.from_numpy(ex).cuda(), ex.astype(i32)):
        got = g.classify(q, 20, None, 64, exclude=exclude)
        assert _same(_votes(got), kr.vote(idx, sc, labels, exclude=ex, top=64))
    found = (idx == ex[:, None]).any(1)
    assert (got.counts.numpy().sum(1)[found] <= 20).all()
    mx = g.classify(q, 20, top=64, reduce="max", exclude=ex)
    assert _same(_votes(mx), kr.vote(idx, sc, labels, exclude=ex, reduce=kr.MAX, top=64))
    s = g.evaluate(q, labels[:40], k=20, temperature=None, nb_classes=9, exclude=ex)
    want = kr.score(idx, sc, labels, labels[:40], 9, exclude=ex)
    assert np.array_equal(s.rank.numpy(), want[1]) and np.array_equal(s.pred.numpy(), want[2])
    assert np.array_equal(bits(s.prob.numpy()), bits(want[3]))                  # counts: the quotient is correctly rounded


def test_one_meter_fed_by_score_and_by_evaluate_equals_two_meters_merged():
    g, rows, labels = _labelled_gallery()
    q, y = grid(104, (24, 32)), np.random.default_rng(105).integers(-1, 10, 24)
    logits = np.random.default_rng(106).uniform(-4, 4, (24, 9)).astype(f32)
    both, a, b = (tfimm.Meter(9, per_class=True, confusion=True) for _ in range(3))
    for lo in range(0, 24, 8):
        rows_ = slice(lo, lo + 8)
        s1 = tfimm.score(logits[rows_], y[rows_], both)
        s2 = g.evaluate(q[rows_], y[rows_], k=20, meter=both)
        assert _same(_votes(s1), _votes(tfimm.score(logits[rows_], y[rows_], a)))
        assert _same(_votes(s2), _votes(g.evaluate(q[rows_], y[rows_], k=20, meter=b, nb_classes=9)))
    assert b.result().count == a.result().count == int(((y >= 0) & (y < 9)).sum())
    a.merge(b)
    sa, sb = a.state(), both.state()
    assert all(np.array_equal(u, v) for u, v in zip(sa, sb)) and sb.words[sr.SCORED] == 2 * b.result().count
    # without a meter: the same four outputs, nothing accumulated
    assert _same(_votes(g.evaluate(q[:8], y[:8], k=20, nb_classes=9)), _votes(g.evaluate(q[:8], y[:8], k=20, meter=tfimm.Meter(9))))


def test_embedding_model_classify_and_evaluate_knn_equal_the_gallery_methods():
    bb = tfimm.create_model("vit_test_model")
    model = tfimm.EmbeddingModel(bb, 32, normalize=True)
    model.set_weights(synthetic_weights(model, 2021))
    x = mc.make_input(model.cfg, 12)
    emb = model(x)
    g = tfimm.Gallery(32)
    labels = (np.arange(12) % 4).astype(i32)
    g.add(emb, labels)
    y = [0, 1, 2, 3, -1, 1, 2, 3, 0, 0, 2, 4]
    for make in (lambda: x, lambda: torch.from_numpy(x).to(torch.bfloat16)):
        e = model(make())
        assert _same(_votes(model.classify(make(), g, k=5, top=4)), _votes(g.classify(e, 5, top=4)))
        assert _same(_votes(model.classify(make(), g, k=5, top=4, reduce="max", exclude=np.arange(12))),
                     _votes(g.classify(e, 5, top=4, reduce="max", exclude=np.arange(12))))
        ma, mb = tfimm.Meter(4), tfimm.Meter(4)
        assert _same(_votes(model.evaluate_knn(make(), y, g, k=5, meter=ma)), _votes(g.evaluate(e, y, k=5, meter=mb)))
        assert np.array_equal(ma.state().words, mb.state().words) and ma.result().count == 10 and ma.result().invalid == 1
    pre = tfimm.create_preprocessing("vit_test_model", defer=True, resize=True)
    u8 = np.random.default_rng(3).integers(0, 256, (3, 40, 52, 3), dtype=np.uint8)
    assert _same(_votes(model.classify(pre(u8), g, k=5)), _votes(g.classify(model(pre(u8)), 5)))
    assert _same(_votes(model.evaluate_knn(pre(u8), [1, 2, 3], g, k=5, nb_classes=4)),
                 _votes(g.evaluate(model(pre(u8)), [1, 2, 3], k=5, nb_classes=4)))

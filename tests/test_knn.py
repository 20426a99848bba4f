"""The kNN end without a GPU: the written rule (tests/knn_ref.py) on matches answered by hand, the refusals of
tfimm_hip_knn_vote / tfimm_hip_knn_score (include/tfimm_hip.h), and the ``ValueError`` cases of the labelled
``tfimm.Gallery`` and of ``EmbeddingModel.classify`` / ``evaluate_knn`` -- all of them raised before any device work."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import knn_ref as kr
import score_ref as sr
import test_architectures  # noqa: F401  (registers the miniature configs)
import tfimm
from tfimm.engine import ffi
from tfimm.utils.init import synthetic_weights

f32, i32 = np.float32, np.int32
TOPMOST = 2 ** 31 - 1


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def one(indices, scores):
    return np.array([indices], i32), np.array([scores], f32)


# ---- the rule ----------------------------------------------------------------------------------------------------------
GLABELS = np.array([4, 2, 4, -1, 9, 2, 7, 4], i32)        # rows 0, 2, 7: class 4; 1, 5: class 2; 3 never votes


def test_majority_vote_by_hand_ties_split_classes_and_rows_that_do_not_vote():
    # class 4 at candidates 0 and 3 (not adjacent), class 2 at 1 and 4: a tie the lower class wins; row 3 carries -1;
    # index 8 (= N) and -1 are outside the gallery; class 9 once
    idx, sc = one([0, 1, 3, 2, 5, 8, 4, -1], [.9, .8, .7, .6, .5, .4, .3, .2])
    c, v, n, t = kr.vote(idx, sc, GLABELS, top=5)
    assert c.tolist() == [[2, 4, 9, -1, -1]] and v.tolist() == [[2, 2, 1, 0, 0]] and n.tolist() == [[2, 2, 1, 0, 0]]
    assert t.tolist() == [5] and c.dtype == i32 and n.dtype == i32 and v.dtype == f32 and t.dtype == f32
    assert not bits(v[0, 3:]).any()                                              # empty slots: +0.0
    assert kr.vote(idx, sc, GLABELS, top=1)[0].tolist() == [[2]]                 # top below the number of classes
    # an excluded row: class 4 loses a vote, class 2 wins alone; an exclusion that is not in the list, or -1, changes nothing
    c, v, n, t = kr.vote(idx, sc, GLABELS, exclude=[2], top=3)
    assert c.tolist() == [[2, 4, 9]] and n.tolist() == [[2, 1, 1]] and t.tolist() == [4]
    for ex in ([6], [-1], [100]):
        assert kr.vote(idx, sc, GLABELS, exclude=ex, top=5)[0].tolist() == [[2, 4, 9, -1, -1]]
    # k: columns behind it are never read
    c, _, n, t = kr.vote(idx, sc, GLABELS, k=2, top=3)
    assert c.tolist() == [[2, 4, -1]] and n.tolist() == [[1, 1, 0]] and t.tolist() == [2]
    # no valid candidate
    c, v, n, t = kr.vote(*one([3, 8, -5, 0], [1, 1, 1, 1]), GLABELS, exclude=[0], top=2)
    assert c.tolist() == [[-1, -1]] and not bits(v).any() and not n.any() and not bits(t).any()


def test_weighted_vote_by_hand():
    idx, sc = one([0, 1, 2, 5], [0.5, 0.5, 0.25, 0.0])
    inv_t = 4.0
    c, v, n, t = kr.vote(idx, sc, GLABELS, inv_temperature=inv_t, top=2, dtype=np.float64)
    w = [1.0, 1.0, math.exp(-1.0), math.exp(-2.0)]
    assert c.tolist() == [[4, 2]] and n.tolist() == [[2, 2]]
    assert v[0].tolist() == [w[0] + w[2], w[1] + w[3]] and t[0] == ((w[0] + w[1]) + w[2]) + w[3]       # ascending j
    # m is the largest VALID score: the best candidate excluded, the weights move
    c, v, _, t = kr.vote(idx, sc, GLABELS, exclude=[0], inv_temperature=inv_t, top=2, dtype=np.float64)
    assert c.tolist() == [[2, 4]] and v[0].tolist() == [1.0 + w[3], w[2]] and t[0] == (1.0 + w[2]) + w[3]
    # float32: one subtraction, one product, expf -- and a temperature of 0 is the majority vote, exactly
    c, v, _, _ = kr.vote(idx, sc, GLABELS, inv_temperature=inv_t, top=2)
    assert v.dtype == f32 and v[0, 0] == f32(1) + np.exp(f32(f32(0.25 - 0.5) * f32(4)))
    assert kr.vote(idx, sc, GLABELS, inv_temperature=0.0, top=2)[1].tolist() == [[2, 2]]
    # weights that underflow: the classes stay in the list with value 0, by ascending class
    c, v, n, t = kr.vote(idx, sc, GLABELS, exclude=[1], inv_temperature=1e4, top=3)
    assert c.tolist() == [[4, 2, -1]] and v.tolist() == [[1, 0, 0]] and n.tolist() == [[2, 1, 0]] and t.tolist() == [1]


def test_max_by_hand_signed_zeros_and_the_first_of_equal_maxima():
    z, nz = f32(0.0), f32(-0.0)
    # class 4: -0.0 then +0.0 -> the first is written; class 2: +0.0; equal values (-0.0 == +0.0): ascending class
    idx, sc = one([0, 1, 2, 4], [nz, z, z, -0.5])
    c, v, n, t = kr.vote(idx, sc, GLABELS, reduce=kr.MAX, top=4)
    assert c.tolist() == [[2, 4, 9, -1]] and n.tolist() == [[1, 2, 1, 0]]
    assert bits(v[0]).tolist() == [bits(z)[()], bits(nz)[()], bits(f32(-0.5))[()], 0] and bits(t).tolist() == [0]
    # the temperature plays no part; a larger later score replaces, an equal one does not
    idx, sc = one([0, 2, 7, 1], [0.25, 0.75, 0.75, 0.5])
    for inv_t in (0.0, 3.0):
        c, v, n, _ = kr.vote(idx, sc, GLABELS, reduce=kr.MAX, inv_temperature=inv_t, top=2)
        assert c.tolist() == [[4, 2]] and v.tolist() == [[0.75, 0.5]] and n.tolist() == [[3, 1]]


def test_scoring_by_hand():
    idx, sc = one([0, 1, 2, 4, 6], [.9, .8, .7, .6, .5])                       # classes 4, 2, 4, 9, 7: votes 2, 1, 1, 1
    C_ = 10
    rows = lambda y: kr.score(np.repeat(idx, len(y), 0), np.repeat(sc, len(y), 0), GLABELS, y, C_)
    loss, rank, pred, prob = rows([4, 2, 7, 9, 0, 3, 8, -1, 10, -2, TOPMOST])
    # v = [0 0 1 0 2 0 0 1 0 1]: 4 first, then 2, 7, 9 by class, then the unvoted ones by class
    assert pred.tolist() == [4] * 11
    assert rank.tolist() == [0, 1, 2, 3, 4, 6, 9, -1, -2, -2, -2]
    assert prob[:4].tolist() == [f32(2) / f32(5), f32(1) / f32(5), f32(1) / f32(5), f32(1) / f32(5)] and not prob[4:].any()
    assert np.allclose(loss[:4], -np.log(prob[:4].astype(np.float64)), rtol=1e-6) and np.isposinf(loss[4:7]).all()
    assert not bits(loss[7:]).any() and not bits(prob[7:]).any()               # not scored: +0.0
    # the same from score_ref on the dense vector
    v, total = kr.dense(idx, sc, GLABELS, C_)
    assert v.tolist() == [[0, 0, 1, 0, 2, 0, 0, 1, 0, 1]] and total.tolist() == [5]
    y = [4, 2, 7, 9, 0, 3, 8, -1, 10, -2]
    _, want_rank, want_pred, _ = sr.score(np.repeat(v, len(y), 0), y)
    assert rank[:10].tolist() == want_rank.tolist() and pred[:10].tolist() == want_pred.tolist()
    # gallery labels that are not below nb_classes do not vote: with 5 classes only 2 and 4 remain
    loss, rank, pred, prob = kr.score(idx, sc, GLABELS, [2], 5)
    assert (rank[0], pred[0], prob[0]) == (1, 4, f32(1) / f32(3))
    # all the vote on the true class: prob 1, loss +0.0
    loss, rank, pred, prob = kr.score(*one([0, 2], [1, 1]), GLABELS, [4], 5)
    assert (rank[0], pred[0], prob[0]) == (0, 4, 1) and bits(loss).tolist() == [0]
    # no valid candidate: pred 0, rank y, prob 0, loss inf
    loss, rank, pred, prob = kr.score(*one([3, 8], [1, 1]), GLABELS, [6], 9)
    assert (rank[0], pred[0], prob[0]) == (6, 0, 0) and np.isposinf(loss[0])


def test_a_voted_class_of_value_zero_ties_with_the_unvoted_ones():
    # inv_temperature 1e4: only the best candidate (class 7) keeps a weight; classes 2 and 9 are voted with value 0
    idx, sc = one([6, 1, 4, 5], [0.9, 0.5, 0.4, 0.3])
    C_ = 12
    v, total = kr.dense(idx, sc, GLABELS, C_, inv_temperature=1e4)
    assert v[0].tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0] and total.tolist() == [1]
    y = list(range(C_))
    loss, rank, pred, prob = kr.score(np.repeat(idx, C_, 0), np.repeat(sc, C_, 0), GLABELS, y, C_, inv_temperature=1e4)
    # 7 first; every other class holds 0 -- voted (2, 9) or not -- and follows by ascending class
    assert rank.tolist() == [1, 2, 3, 4, 5, 6, 7, 0, 8, 9, 10, 11] and pred.tolist() == [7] * C_
    _, want_rank, want_pred, _ = sr.score(np.repeat(v, C_, 0), y)
    assert rank.tolist() == want_rank.tolist() and pred.tolist() == want_pred.tolist()
    assert prob.tolist() == v[0].tolist() and bits(loss)[7] == 0 and np.isposinf(np.delete(loss, 7)).all()
    # the meter state follows score_ref.state on these outputs: the infinite losses are excluded, their ranks count
    words, per_class, confusion = sr.state(loss, rank, y, C_, pred)
    assert (words[sr.SCORED], words[sr.LOSS_EXCLUDED], words[sr.LOSS_Q]) == (12, 11, 0)
    assert words[sr.RANK_HIST:sr.RANK_HIST + 12].tolist() == [1] * 12 and confusion[:, 7].tolist() == [1] * 12


def test_random_rows_agree_with_score_ref_on_the_dense_vector():
    rng = np.random.default_rng(5)
    B, k, N, C_ = 60, 9, 40, 7
    idx = np.stack([rng.choice(N + 4, k, replace=False) - 2 for _ in range(B)]).astype(i32)       # some outside [0, N)
    sc = (rng.integers(-4, 5, (B, k)) / 8).astype(f32)
    glabels = rng.integers(-1, C_ + 2, N).astype(i32)
    y = rng.integers(-2, C_ + 1, B)
    ex = rng.integers(-1, N, B)
    for inv_t in (0.0, 2.0):
        loss, rank, pred, prob = kr.score(idx, sc, glabels, y, C_, exclude=ex, inv_temperature=inv_t)
        v, total = kr.dense(idx, sc, glabels, C_, exclude=ex, inv_temperature=inv_t)
        _, want_rank, want_pred, _ = sr.score(v, y)
        assert np.array_equal(rank, want_rank) and np.array_equal(pred, want_pred)
        c, val, n, t = kr.vote(idx, sc, np.where(glabels >= C_, -1, glabels).astype(i32), exclude=ex, inv_temperature=inv_t, top=C_)
        assert np.array_equal(bits(t), bits(total))
        for b in range(B):
            d = int((c[b] >= 0).sum())
            assert np.array_equal(bits(v[b, c[b, :d]]), bits(val[b, :d])) and int((v[b] != 0).sum()) <= d


# ---- refusals: before any launch, so no GPU is involved ------------------------------------------------------------------
VOTE_ARGS = ("indices", "scores", "glabels", "exclude", "classes", "values", "counts", "total")
SCORE_ARGS = ("indices", "scores", "glabels", "exclude", "labels", "loss", "rank", "pred", "prob", "state", "per_class", "confusion")
OPTIONAL = ("exclude", "state", "per_class", "confusion")


def _ptrs(names, null, off, extra):
    bufs = {n: np.zeros(4096, np.int64) for n in names}
    return {n: (C.c_void_p(bufs[n].ctypes.data + (off or {}).get(n, 0)) if n not in null and (n not in OPTIONAL or extra.get(n)) else None)
            for n in names}, bufs


def _vote(ld=8, B=2, k=5, N=100, inv_t=0.0, reduce=0, top=5, null=(), off=None, **extra):
    """tfimm_hip_knn_vote over host buffers (a refusal never touches them)"""
    p, keep = _ptrs(VOTE_ARGS, null, off, extra)
    rc = ffi.lib.tfimm_hip_knn_vote(p["indices"], p["scores"], ld, B, k, p["glabels"], N, p["exclude"], inv_t, reduce, top,
                                    p["classes"], p["values"], p["counts"], p["total"], None)
    return rc, ffi.lib.tfimm_hip_last_error().decode()


def _score(ld=8, B=2, k=5, N=100, inv_t=0.0, nb_classes=10, null=(), off=None, **extra):
    p, keep = _ptrs(SCORE_ARGS, null, off, extra)
    rc = ffi.lib.tfimm_hip_knn_score(p["indices"], p["scores"], ld, B, k, p["glabels"], N, p["exclude"], inv_t, nb_classes,
                                     p["labels"], p["loss"], p["rank"], p["pred"], p["prob"], p["state"], p["per_class"],
                                     p["confusion"], None)
    return rc, ffi.lib.tfimm_hip_last_error().decode()


COMMON_REFUSALS = [
    (dict(null=("indices",)), "indices is null"), (dict(null=("scores",)), "scores is null"), (dict(null=("glabels",)), "glabels is null"),
    (dict(off={"indices": 2}), "4-byte"), (dict(off={"scores": 1}), "4-byte"), (dict(off={"glabels": 2}), "4-byte"),
    (dict(off={"exclude": 2}, exclude=True), "exclude"),
    (dict(k=0), "k=0"), (dict(k=-3), "k=-3"), (dict(k=65, ld=65), "k=65"), (dict(ld=4), "ld=4"), (dict(N=0), "N=0"), (dict(N=-7), "N=-7"),
    (dict(B=-1), "B=-1"), (dict(inv_t=-1.0), "inv_temperature=-1"), (dict(inv_t=float("nan")), "inv_temperature=nan"),
    (dict(inv_t=float("inf")), "inv_temperature=inf"),
]


@pytest.mark.parametrize("kw, names", COMMON_REFUSALS + [
    (dict(null=("classes",)), "classes is null"), (dict(null=("values",)), "values is null"), (dict(null=("counts",)), "counts is null"),
    (dict(null=("total",)), "total is null"), (dict(off={"classes": 2}), "4-byte"), (dict(off={"total": 1}), "4-byte"),
    (dict(reduce=2), "reduce=2"), (dict(reduce=-1), "reduce=-1"), (dict(top=0), "top=0"), (dict(top=65), "top=65"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_vote_refusals_return_minus_one_and_name_the_argument(kw, names):
    rc, msg = _vote(**kw)
    assert rc == -1 and msg.startswith("knn_vote:") and names in msg, (rc, msg)


@pytest.mark.parametrize("kw, names", COMMON_REFUSALS + [
    (dict(null=("labels",)), "labels is null"), (dict(null=("loss",)), "loss is null"), (dict(null=("rank",)), "rank is null"),
    (dict(null=("pred",)), "pred is null"), (dict(null=("prob",)), "prob is null"),
    (dict(off={"labels": 2}), "4-byte"), (dict(off={"prob": 2}), "4-byte"), (dict(off={"confusion": 2}, confusion=True), "confusion"),
    (dict(off={"state": 4}, state=True), "state"), (dict(off={"per_class": 4}, per_class=True), "per_class"),
    (dict(nb_classes=0), "nb_classes=0"), (dict(nb_classes=-5), "nb_classes=-5"), (dict(nb_classes=4097, confusion=True), "confusion"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_score_refusals_return_minus_one_and_name_the_argument(kw, names):
    rc, msg = _score(**kw)
    assert rc == -1 and msg.startswith("knn_score:") and names in msg, (rc, msg)


def test_constants_agree_the_limits_are_accepted_and_an_empty_batch_is_no_launch():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfimm_hip.h")).read()

    def define(name):
        return re.search(rf"#define TFIMM_KNN_{name} (\S+)", hdr).group(1)
    assert define("MAX_K") == "TFIMM_EMBED_MAX_K" and ffi.KNN_MAX_K == ffi.EMBED_MAX_K == 64
    assert int(define("MAX_TOP")) == ffi.KNN_MAX_TOP == 64
    assert (int(define("SUM")), int(define("MAX"))) == (ffi.KNN_SUM, ffi.KNN_MAX) == (kr.SUM, kr.MAX) == (0, 1)
    assert ffi.lib.tfimm_hip_abi_version() == 4
    # B == 0 returns before any launch, at the limits of every argument
    assert _vote(B=0)[0] == 0 and _score(B=0)[0] == 0
    assert _vote(B=0, k=64, ld=64, top=64, reduce=1, N=TOPMOST, inv_t=3e38, exclude=True)[0] == 0
    assert _vote(B=0, k=1, ld=1, top=1, N=1)[0] == 0
    assert _score(B=0, k=64, ld=1 << 40, nb_classes=TOPMOST, N=TOPMOST, state=True, per_class=True, exclude=True)[0] == 0
    assert _score(B=0, nb_classes=4096, state=True, per_class=True, confusion=True)[0] == 0
    assert _score(B=0, nb_classes=1)[0] == 0


# ---- Python: what is refused, before any device work ---------------------------------------------------------------------
@pytest.fixture
def hostless(monkeypatch):
    """``Gallery._store`` -- the device part of ``add``, behind every check -- replaced by the bookkeeping alone: rows and
    labels are counted, nothing is uploaded"""
    def store(self, t, up_labels, n):
        self._labelled = self._labelled or up_labels is not None
        first, self._n = self._n, self._n + n
        return range(first, self._n)
    monkeypatch.setattr(tfimm.Gallery, "_store", store)


def _gallery(n=100, labelled=True):
    g = tfimm.Gallery(32)
    g.add(np.zeros((n, 32), f32), np.arange(n) % 7 if labelled else None)
    return g


def test_an_unlabelled_gallery_keeps_its_signature_defaults_and_its_behaviour(hostless):
    sig = inspect.signature(tfimm.Gallery.add)
    assert list(sig.parameters) == ["self", "x", "labels"] and sig.parameters["labels"].default is None
    assert str(inspect.signature(tfimm.Gallery.search)) == "(self, q, k: int = 5, chunk: int = 0) -> tfimm.models.gallery.Matches"
    assert str(inspect.signature(tfimm.Gallery.__init__)) == "(self, dim: int, capacity: int = 0)"
    assert tfimm.Matches._fields == ("indices", "scores") and tfimm.Votes._fields == ("classes", "values", "counts", "total")
    g = tfimm.Gallery(32, capacity=4)
    assert not g.labelled and len(g) == 0 and g.capacity == 4 and g.numpy().shape == (0, 32)
    assert g.add(np.zeros((3, 32), f32)) == range(0, 3) and g.add(np.zeros((2, 32), f32)) == range(3, 5) and not g.labelled
    with pytest.raises(ValueError, match="float32"):
        g.add(np.zeros((2, 32), np.float64))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        g.add(np.zeros((2, 48), f32))
    with pytest.raises(ValueError, match="k = 6"):
        g.search(np.zeros((1, 32), f32), 6)
    # labels on an unlabelled gallery that holds rows; every labelled method on it
    with pytest.raises(ValueError, match="holds 5 rows without"):
        g.add(np.zeros((2, 32), f32), [0, 1])
    q = np.zeros((2, 32), f32)
    for call in (lambda: g.labels(), lambda: g.labels_of([0]), lambda: g.vote(None), lambda: g.classify(q, 2),
                 lambda: g.evaluate(q, [0, 1], k=2, nb_classes=3)):
        with pytest.raises(ValueError, match="no labels"):
            call()
    assert len(g) == 5                                                          # a refused add adds nothing


def test_gallery_label_forms_lengths_and_mixing(hostless):
    import torch
    rows = np.zeros((3, 32), f32)
    g = tfimm.Gallery(32)
    for bad in ([0.0, 1.0, 2.0], np.zeros(3, f32), np.zeros(3, bool), torch.zeros(3), torch.zeros(3, dtype=torch.int16)):
        with pytest.raises(ValueError, match="labels"):
            g.add(rows, bad)
    for bad in ([[0, 1, 2]], np.zeros((3, 1), np.int64), 7, [0, 1], torch.zeros(4, dtype=torch.int64)):
        with pytest.raises(ValueError, match="labels"):
            g.add(rows, bad)
    for bad in ([0, -2, 1], np.array([0, 2 ** 31, 1]), np.array([0, 1, 2 ** 40], np.uint64), torch.tensor([0, 1, -5]),
                torch.tensor([0, 2 ** 31, 1])):
        with pytest.raises(ValueError, match=r"\[0, 2\^31 - 1\] or -1"):
            g.add(rows, bad)
    assert len(g) == 0 and not g.labelled                                       # nothing was added, nothing decided
    assert g.add(rows, [0, -1, TOPMOST]) == range(0, 3) and g.labelled         # -1 and 2^31 - 1 are labels
    assert g.add(rows, np.array([1, 2, 3], np.uint8)) == range(3, 6)
    assert g.add(rows, torch.tensor([1, 2, 3], dtype=torch.int32)) == range(6, 9)
    with pytest.raises(ValueError, match="3 rows need 3 labels"):
        g.add(rows)
    assert g.add(np.zeros((0, 32), f32), np.zeros(0, np.int64)) == range(9, 9)
    assert len(g) == 9


def test_vote_classify_and_evaluate_value_errors_need_no_device(hostless):
    g = _gallery(100)
    q = np.zeros((4, 32), f32)
    for kw in (dict(top=0), dict(top=65), dict(top=2.5), dict(top=True), dict(top=None)):
        with pytest.raises(ValueError, match="top"):
            g.classify(q, **kw)
    for t in (0, 0.0, -0.07, float("nan"), 1e-45, "cold", True):            # 1e-45: its inverse is no finite float32
        with pytest.raises(ValueError, match="temperature"):
            g.classify(q, temperature=t)
        with pytest.raises(ValueError, match="temperature"):
            g.evaluate(q, [0, 1, 2, 3], nb_classes=7, temperature=t)
    for r in ("mean", "SUM", 0, None):
        with pytest.raises(ValueError, match="reduce"):
            g.classify(q, reduce=r)
    for k in (0, -1, 65, 101, 2.0, True, None):
        with pytest.raises(ValueError, match="k"):
            g.classify(q, k)
    # with exclude the search asks for one row more: k + 1 <= 64 and k + 1 <= len
    with pytest.raises(ValueError, match=r"k = 64 \(\+ 1 for the excluded row\)"):
        g.classify(q, 64, exclude=[0, 1, 2, 3])
    with pytest.raises(ValueError, match=r"\+ 1 for the excluded row"):
        g.evaluate(q, [0, 1, 2, 3], k=64, nb_classes=7, exclude=[0, 1, 2, 3])
    small = _gallery(20)
    with pytest.raises(ValueError, match=r"k = 20 \(\+ 1"):
        small.classify(q, 20, exclude=[0, 1, 2, 3])
    with pytest.raises(ValueError, match="k = 21"):
        small.classify(q, 21)
    for bad in ([0, 1, 2], [0.5, 1, 2, 3], [[0, 1, 2, 3]], 3):
        with pytest.raises(ValueError, match="exclude"):
            g.classify(q, 5, exclude=bad)
    for bad in (np.zeros((4, 32), np.float64), np.zeros((4, 16), f32), np.zeros(32, f32)):
        with pytest.raises(ValueError, match="Gallery.classify"):
            g.classify(bad, 5)
    # evaluate: labels, and where nb_classes comes from
    for bad in ([0, 1, 2], [0.5, 1, 2, 3], 3):
        with pytest.raises(ValueError, match="labels"):
            g.evaluate(q, bad, nb_classes=7)
    with pytest.raises(ValueError, match="nb_classes is needed"):
        g.evaluate(q, [0, 1, 2, 3])
    for n in (0, -1, 2 ** 31, 2.5, True):
        with pytest.raises(ValueError, match="nb_classes"):
            g.evaluate(q, [0, 1, 2, 3], nb_classes=n)
    with pytest.raises(ValueError, match="meter counts 10 classes, nb_classes = 7"):
        g.evaluate(q, [0, 1, 2, 3], meter=tfimm.Meter(10), nb_classes=7)
    with pytest.raises(ValueError, match="tfimm.Meter"):
        g.evaluate(q, [0, 1, 2, 3], meter="meter")
    # vote: what is no Matches of a search
    import torch
    i, s = torch.zeros((4, 5), dtype=torch.int32), torch.zeros((4, 5))
    for bad in (None, 5, (i,), tfimm.Matches(i.long(), s), tfimm.Matches(i, s.double()), tfimm.Matches(i, s[:, :4]),
                tfimm.Matches(i[0], s[0]), tfimm.Matches(torch.zeros((4, 65), dtype=torch.int32), torch.zeros((4, 65))),
                tfimm.Matches(tfimm.Tensor(i), tfimm.Tensor(s))):                # the last: right in form, but on the host
        with pytest.raises(ValueError, match="matches"):
            g.vote(bad)
    with pytest.raises(ValueError, match="top"):
        g.vote(tfimm.Matches(i, s), top=0)
    assert len(g) == 100 and not g._work                                        # no search ran


def test_embedding_model_knn_value_errors_come_before_the_forward_pass(hostless):
    bb = tfimm.create_model("vit_test_model")
    bb.set_weights(synthetic_weights(bb))
    m = tfimm.EmbeddingModel(bb, 32)
    x = np.zeros((2, 32, 32, 3), f32)
    g = _gallery(50)
    with pytest.raises(ValueError, match="gallery holds rows of 32"):
        tfimm.EmbeddingModel(bb, 16).classify(x, g)
    with pytest.raises(ValueError, match="gallery holds rows of 32"):
        tfimm.EmbeddingModel(bb, 16).evaluate_knn(x, [0, 1], g, nb_classes=7)
    with pytest.raises(ValueError, match="no labels"):
        m.classify(x, _gallery(50, labelled=False))
    with pytest.raises(ValueError, match="k = 51"):
        m.classify(x, g, k=51)
    with pytest.raises(ValueError, match="reduce"):
        m.classify(x, g, reduce="median")
    with pytest.raises(ValueError, match="exclude"):
        m.classify(x, g, exclude=[0, 1, 2])                                     # three for a batch of two
    with pytest.raises(ValueError, match="labels for a batch of 2"):
        m.evaluate_knn(x, [0, 1, 2], g, nb_classes=7)
    with pytest.raises(ValueError, match="nb_classes is needed"):
        m.evaluate_knn(x, [0, 1], g)
    with pytest.raises(ValueError, match="meter counts 5"):
        m.evaluate_knn(x, [0, 1], g, meter=tfimm.Meter(5), nb_classes=7)
    with pytest.raises(ValueError, match="temperature"):
        m.evaluate_knn(x, [0, 1], g, nb_classes=7, temperature=0)
    # the classifier's methods keep raising as they did
    with pytest.raises(ValueError, match="classifier"):
        m.evaluate(x, [0, 1])
    with pytest.raises(ValueError, match="classifier"):
        m.top_k(x, 1)
    assert not m._plans and not m._captured                                     # nothing touched a device

"""The scoring end without a GPU: the written rule (tests/score_ref.py) on rows answered by hand, the refusals of
tfimm_hip_score (include/tfimm_hip.h), the ``ValueError`` cases of ``tfimm.score`` / ``tfimm.Meter`` / ``Model.evaluate``, and
the host arithmetic of ``MeterResult`` and ``Meter.merge``."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import score_ref as sr
import test_architectures  # noqa: F401  (registers the miniature configs)
import tfimm
import topk_ref as tr
from tfimm.engine import ffi
from tfimm.utils.init import synthetic_weights

f32 = np.float32
NAN, INF = f32(np.nan), f32(np.inf)


# ---- the rule ----------------------------------------------------------------------------------------------------------
def test_rule_by_hand_ties_zeros_nan_and_labels_outside_the_row():
    x = np.array([[1.0, 3.0, 3.0, -2.0, 3.0],            # ties: the lower column wins
                  [1.0, 3.0, 3.0, -2.0, 3.0],
                  [-0.0, 0.0, -1.0, -0.0, 0.0],          # zeros of both signs are equal: the column decides
                  [2.0, NAN, 7.0, -INF, 7.0],            # a NaN is first, whatever else the row holds
                  [0.5, 0.25, 0.0, 0.0, 0.0],            # label -1: not scored
                  [0.5, 0.25, 0.0, 0.0, 0.0]], f32)      # label N: out of range
    labels = [4, 0, 3, 2, -1, 5]
    loss, rank, pred, prob = sr.score(x, labels)
    assert pred.tolist() == [1, 1, 0, 1, 0, 0]
    assert rank.tolist() == [2, 3, 2, 1, -1, -2]
    assert rank.dtype == np.int32 and pred.dtype == np.int32 and loss.dtype == np.float64
    s = 3 + math.exp(-2) + math.exp(-5)
    assert loss[0] == pytest.approx(math.log(s), rel=1e-15) and prob[0] == pytest.approx(1 / s, rel=1e-15)
    assert loss[1] == pytest.approx(math.log(s) + 2, rel=1e-15) and prob[1] == pytest.approx(math.exp(-2) / s, rel=1e-15)
    assert loss[2] == pytest.approx(math.log(4 + math.exp(-1)), rel=1e-15)
    assert np.isnan(loss[3]) and np.isnan(prob[3])                              # not specified for such a row
    assert loss[4:].tolist() == [0, 0] and prob[4:].tolist() == [0, 0]
    # one class: the loss is exactly zero, the probability exactly one
    loss, rank, pred, prob = sr.score(np.array([[-3.5]], f32), [0])
    assert (loss[0], rank[0], pred[0], prob[0]) == (0.0, 0, 0, 1.0) and not np.signbit(loss[0])


def test_rank_is_the_position_in_top_k_and_differs_from_in_top_k_on_ties():
    x = np.random.default_rng(3).integers(-2, 3, (40, 9)).astype(f32)           # many ties
    labels = np.random.default_rng(4).integers(0, 9, 40)
    _, rank, pred, _ = sr.score(x, labels)
    for k in (1, 3, 9):
        idx = tr.topk(x, k, probs=False)[0]
        hit = (idx == labels[:, None]).any(1)
        assert np.array_equal(rank < k, hit)
        assert all(idx[b, rank[b]] == labels[b] for b in np.nonzero(hit)[0])
    assert np.array_equal(pred, tr.topk(x, 1, probs=False)[0][:, 0])
    # an all-equal row: tf.math.in_top_k(k = 1) would call every label a hit; here only class 0 has rank 0
    _, rank, pred, _ = sr.score(np.full((4, 4), 1.5, f32), [0, 1, 2, 3])
    assert rank.tolist() == [0, 1, 2, 3] and pred.tolist() == [0] * 4


def test_state_rule_by_hand():
    loss = np.array([0.5, 1023.99994, 1024.0, NAN, 3.0, 0.0, 2.0 ** -33, 3 * 2.0 ** -33], f32)
    rank = [0, 63, 64, 5, -1, -2, 0, 40000]
    labels = [1, 2, 2, 0, -1, 7, 1, 3]
    pred = [1, 0, 0, 0, 0, 0, 1, 0]
    w, pc, cm = sr.state(loss, rank, labels, 4, pred)
    assert (w[sr.SCORED], w[sr.IGNORED], w[sr.INVALID], w[sr.LOSS_EXCLUDED]) == (6, 1, 1, 2)
    # 2^-33 * 2^32 = 0.5 rounds to 0 and 1.5 to 2: half to even
    assert w[sr.LOSS_Q] == 2 ** 31 + int(np.float64(f32(1023.99994)) * 2 ** 32) + 0 + 2
    hist = w[sr.RANK_HIST:]
    assert hist.shape == (65,) and hist[0] == 2 and hist[5] == 1 and hist[63] == 1 and hist[64] == 2 and hist.sum() == 6
    assert pc.tolist() == [[1, 2, 2, 1], [0, 2, 0, 0]]
    assert cm.tolist() == [[1, 0, 0, 0], [0, 2, 0, 0], [2, 0, 0, 0], [1, 0, 0, 0]]


# ---- refusals: before any launch, so no GPU is involved ------------------------------------------------------------------
ARGS = ("logits", "labels", "loss", "rank", "pred", "prob", "state", "per_class", "confusion")


def _call(ld=16, B=2, N=16, null=(), off=None, **extra):
    """tfimm_hip_score over host buffers (a refusal never touches them); ``null``: pointers passed as NULL; ``off``:
    {name: bytes} added to a pointer; state / per_class / confusion are NULL unless named in ``extra``"""
    bufs = {n: np.zeros(4096, np.int64) for n in ARGS}
    ptr = []
    for n in ARGS:
        on = n not in null and (n in ARGS[:6] or extra.get(n, False))
        ptr.append(C.c_void_p(bufs[n].ctypes.data + (off or {}).get(n, 0)) if on else None)
    rc = ffi.lib.tfimm_hip_score(ptr[0], ld, B, N, *ptr[1:], None)
    return rc, ffi.lib.tfimm_hip_last_error().decode()


@pytest.mark.parametrize("kw, names", [
    (dict(null=("logits",)), "logits"), (dict(null=("labels",)), "labels"), (dict(null=("loss",)), "loss"),
    (dict(null=("rank",)), "rank"), (dict(null=("pred",)), "pred"), (dict(null=("prob",)), "prob"),
    (dict(off={"logits": 2}), "4-byte"), (dict(off={"labels": 1}), "4-byte"), (dict(off={"prob": 2}), "4-byte"),
    (dict(off={"confusion": 2}, confusion=True), "confusion"),
    (dict(off={"state": 4}, state=True), "state"), (dict(off={"per_class": 4}, per_class=True), "per_class"),
    (dict(N=0), "N=0"), (dict(N=-4), "N=-4"), (dict(N=32769, ld=32769), "N=32769"),
    (dict(ld=15), "ld=15"), (dict(B=-1), "B=-1"),
    (dict(N=4097, ld=4097, confusion=True), "confusion"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_refusals_return_minus_one_and_name_the_argument(kw, names):
    rc, msg = _call(**kw)
    assert rc == -1 and msg.startswith("score:") and names in msg, (rc, msg)


def test_constants_in_the_header_and_the_binding_agree_and_an_empty_batch_is_no_launch():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfimm_hip.h")).read()

    def define(name):
        return re.search(rf"#define TFIMM_SCORE_{name} (\S+)", hdr).group(1)
    assert define("MAX_N") == "TFIMM_TOPK_MAX_N" and ffi.SCORE_MAX_N == ffi.TOPK_MAX_N == 32768
    assert int(define("MAX_CONFUSION_N")) == ffi.SCORE_MAX_CONFUSION_N == 4096
    assert define("IGNORE") == "(-1)" and ffi.SCORE_IGNORE == sr.IGNORE == -1
    for name, ref in (("SCORED", sr.SCORED), ("IGNORED", sr.IGNORED), ("INVALID", sr.INVALID), ("LOSS_EXCLUDED", sr.LOSS_EXCLUDED),
                      ("LOSS_Q", sr.LOSS_Q), ("RANK_HIST", sr.RANK_HIST), ("RANK_BINS", sr.RANK_BINS),
                      ("STATE_WORDS", sr.STATE_WORDS)):
        assert int(define(name)) == getattr(ffi, "SCORE_" + name) == ref, name
    assert ffi.SCORE_RANK_HIST + ffi.SCORE_RANK_BINS == ffi.SCORE_STATE_WORDS and ffi.SCORE_RANK_BINS == ffi.TOPK_MAX_K + 1
    assert "sparse_softmax_cross_entropy_with_logits" in hdr and "in_top_k" in hdr and "2^21 rows" in hdr
    assert _call(B=0)[0] == 0                                                    # returns before any launch
    assert _call(B=0, state=True, per_class=True, confusion=True)[0] == 0
    assert _call(N=4096, ld=4096, B=0, confusion=True)[0] == 0                   # the largest confusion matrix is accepted


# ---- Python: what is refused, before any device work ---------------------------------------------------------------------
def _model(name, **kw):
    m = tfimm.create_model(name, **kw)
    m.set_weights(synthetic_weights(m))
    return m


def test_score_and_meter_value_errors_need_no_device():
    import torch
    ok = np.zeros((3, 12), f32)
    for bad in (np.zeros((3, 12), np.float64), np.zeros((3, 12), np.int32), torch.zeros(3, 12, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="float32"):
            tfimm.score(bad, [0, 1, 2])
    for bad in (np.zeros(12, f32), np.zeros((3, 1, 12), f32), np.zeros((3, 0), f32)):
        with pytest.raises(ValueError, match="logits"):
            tfimm.score(bad, [0, 1, 2])
    with pytest.raises(ValueError, match="32768"):
        tfimm.score(np.zeros((1, 32769), f32), [0])
    for bad in ([0.0, 1.0, 2.0], np.zeros(3, f32), np.zeros(3, bool), torch.zeros(3), torch.zeros(3, dtype=torch.int16)):
        with pytest.raises(ValueError, match="labels"):
            tfimm.score(ok, bad)
    for bad in ([[0, 1, 2]], np.zeros((3, 1), np.int64), 7, [0, 1], torch.zeros(4, dtype=torch.int64)):
        with pytest.raises(ValueError, match="labels"):
            tfimm.score(ok, bad)
    for n in (0, -1, 32769, 2.5, None, True):
        with pytest.raises(ValueError, match="nb_classes"):
            tfimm.Meter(n)
    with pytest.raises(ValueError, match="4096"):
        tfimm.Meter(4097, confusion=True)
    assert tfimm.Meter(4097, per_class=True).nb_classes == 4097 and tfimm.Meter(4096, confusion=True).confusion
    meter = tfimm.Meter(10)
    with pytest.raises(ValueError, match=r"\(B, 10\)"):
        meter.update(ok, [0, 1, 2])                                             # 12 columns for a meter of 10 classes
    with pytest.raises(ValueError, match="labels"):
        tfimm.score(ok, [0, 1], meter=tfimm.Meter(12))
    assert tfimm.Scores._fields == ("loss", "rank", "pred", "prob")


def test_model_evaluate_value_errors_need_no_device():
    x = np.zeros((2, 32, 32, 3), f32)
    with pytest.raises(ValueError, match="nb_classes == 0"):
        _model("vit_test_model", nb_classes=0).evaluate(x, [0, 1])
    with pytest.raises(ValueError, match="32768"):
        _model("vit_test_model", nb_classes=32769).evaluate(x, [0, 1])
    with pytest.raises(ValueError, match="2 heads"):
        _model("deit_test_model").evaluate(x, [0, 1])
    m = _model("vit_test_model")
    with pytest.raises(ValueError, match="meter counts 10"):
        m.evaluate(x, [0, 1], meter=tfimm.Meter(10))
    for bad in ([0], [0, 1, 2], np.zeros(3, np.int64)):
        with pytest.raises(ValueError, match="labels for a batch of 2"):
            m.evaluate(x, bad)
    with pytest.raises(ValueError, match="labels"):
        m.evaluate(x, 5)
    pre = tfimm.create_preprocessing("vit_test_model", defer=True, resize=True)
    imgs = [np.zeros((40, 30, 3), np.uint8), np.zeros((20, 50, 3), np.uint8), np.zeros((33, 33, 3), np.uint8)]
    with pytest.raises(ValueError, match="labels for a batch of 3"):
        m.evaluate(pre(imgs), [0, 1])
    with pytest.raises(ValueError, match="labels"):
        m.evaluate(x, [0.5, 1.0])                                               # the right length, not integers
    with pytest.raises(NotImplementedError):
        m.evaluate(x, [0, 1], training=True)
    assert not m._plans and not m._captured                                     # nothing touched a device
    e = tfimm.EmbeddingModel(_model("vit_test_model"), 16)
    with pytest.raises(ValueError, match="classifier"):
        e.evaluate(x, [0, 1])


# ---- MeterResult and merge: host arithmetic --------------------------------------------------------------------------------
def _hand_state():
    w = np.zeros(sr.STATE_WORDS, np.int64)
    w[sr.SCORED], w[sr.IGNORED], w[sr.INVALID], w[sr.LOSS_EXCLUDED] = 20, 4, 1, 2
    w[sr.LOSS_Q] = 27 * 2 ** 32 + 2 ** 31                    # 27.5 over 18 rows
    w[sr.RANK_HIST + 0], w[sr.RANK_HIST + 1], w[sr.RANK_HIST + 4], w[sr.RANK_HIST + 5] = 10, 3, 2, 1
    w[sr.RANK_HIST + 63], w[sr.RANK_HIST + 64] = 1, 3
    return w


def test_meter_result_from_a_hand_made_state():
    pc = np.array([[12, 8, 0], [7, 3, 0]])
    cm = np.array([[7, 5, 0], [4, 3, 1], [0, 0, 0]])
    r = tfimm.MeterResult.from_state(_hand_state(), pc, cm)
    assert (r.count, r.ignored, r.invalid, r.loss_excluded) == (20, 4, 1, 2)
    assert r.loss == 27.5 / 18 and isinstance(r.loss, float)
    assert r.accuracy(1) == r.top1 == 0.5 and r.accuracy(2) == 13 / 20 and r.accuracy(5) == 15 / 20
    assert r.accuracy(6) == 16 / 20 and r.accuracy(63) == 16 / 20 and r.accuracy(64) == 17 / 20
    assert r.rank_hist.shape == (65,) and r.rank_hist.sum() == r.count
    assert r.per_class_support.tolist() == [12, 8, 0] and r.per_class_hits.tolist() == [7, 3, 0]
    assert np.array_equal(r.confusion, cm)
    for k in (0, 65, -1, 1.5, None, True):
        with pytest.raises(ValueError, match="k"):
            r.accuracy(k)
    bare = tfimm.MeterResult.from_state(_hand_state())
    assert bare.per_class_support is None and bare.per_class_hits is None and bare.confusion is None
    with pytest.raises(ValueError, match="70"):
        tfimm.MeterResult.from_state(np.zeros(69, np.int64))
    with pytest.raises(ValueError, match="integer"):
        tfimm.MeterResult.from_state(np.zeros(70, np.float64))


def test_an_empty_state_gives_nan_without_raising():
    r = tfimm.MeterResult.from_state(np.zeros(sr.STATE_WORDS, np.int64))
    assert r.count == 0 and math.isnan(r.loss) and math.isnan(r.accuracy(1)) and math.isnan(r.accuracy(64)) and math.isnan(r.top1)
    w = np.zeros(sr.STATE_WORDS, np.int64)
    w[sr.SCORED] = w[sr.LOSS_EXCLUDED] = w[sr.RANK_HIST] = 3          # every scored row's loss was excluded
    r = tfimm.MeterResult.from_state(w)
    assert math.isnan(r.loss) and r.top1 == 1.0
    assert "nan" in repr(tfimm.Meter(5).result())                      # a meter that never saw a batch: no device involved


def test_merge_adds_host_arrays_and_state_round_trips():
    m = tfimm.Meter(3, per_class=True, confusion=True)
    s0 = m.state()
    assert s0.words.shape == (70,) and s0.per_class.shape == (2, 3) and s0.confusion.shape == (3, 3)
    assert not s0.words.any() and not s0.per_class.any() and not s0.confusion.any()
    pc = np.array([[12, 8, 0], [7, 3, 0]])
    cm = np.array([[7, 5, 0], [4, 3, 1], [0, 0, 0]])
    m.merge((_hand_state(), pc, cm))
    m.merge(tfimm.MeterState(_hand_state(), pc, cm.astype(np.uint32)))
    other = tfimm.Meter(3, per_class=True, confusion=True)
    other.merge(m)                                                     # a Meter, too
    for meter, times in ((m, 2), (other, 2)):
        s = meter.state()
        assert np.array_equal(s.words, times * _hand_state()) and np.array_equal(s.per_class, times * pc)
        assert np.array_equal(s.confusion, times * cm)
    r = m.result()
    assert r.count == 40 and r.loss == 27.5 / 18 and r.top1 == 0.5 and r.per_class_hits.tolist() == [14, 6, 0]
    # a meter that keeps less takes what it keeps; one that keeps more refuses a state without it
    plain = tfimm.Meter(3)
    plain.merge(m)
    assert plain.state().per_class is None and plain.result().count == 40
    with pytest.raises(ValueError, match="per_class"):
        m.merge(plain)
    with pytest.raises(ValueError, match="shape"):
        m.merge((_hand_state(), np.zeros((2, 4), np.int64), cm))
    with pytest.raises(ValueError, match="words"):
        m.merge((np.zeros(70), pc, cm))                               # floats
    assert m.result().count == 40                                      # a refused merge adds nothing
    m.reset()
    assert not m.state().words.any() and not m.state().confusion.any() and m.result().count == 0

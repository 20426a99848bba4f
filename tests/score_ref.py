"""Restatement of the scoring end -- ``tf.nn.sparse_softmax_cross_entropy_with_logits``, ``tf.argmax`` and the rank of the
true class behind ``model(x)`` -- in plain numpy (test helper): the single written rule that tfimm_hip_score
(csrc/score.hip), ``tfimm.score`` and ``tfimm.Meter`` are held to.

Per row ``x`` of ``N`` float32 logits with label ``y``:

* ``pred``: the first column in the selection order of tests/topk_ref.py (a NaN before every number, then by value
  descending with ``-0.0 == +0.0``, equal entries by ascending column): ``tf.argmax`` on a row of numbers;
* ``rank``: the position of column ``y`` in that order, i.e. how many columns come before it.  ``rank < k`` exactly when ``y``
  is among ``topk_ref.topk(x, k)``'s indices.  (``tf.math.in_top_k`` counts every tie with the k-th value as a hit; this rule
  follows ``tf.math.top_k``.)
* ``loss = log(sum_i exp(x_i - m)) - (x_y - m)`` and ``prob = exp(x_y - m) / sum_i exp(x_i - m)``, ``m`` the row maximum, in
  float64 -- specified for rows whose entries are all finite, NaN here otherwise;
* ``y == -1``: the row is not scored: ``loss = 0``, ``prob = 0``, ``rank = -1``; any other ``y`` outside ``[0, N)``: the same
  with ``rank = -2``.  ``pred`` is defined for every row.

The meter state (``state``) is integer arithmetic on the per-sample float32 ``loss`` and ``rank``; its layout is restated here.

Deliberately independent of the engine: nothing here imports tfimm.
"""
import numpy as np

import topk_ref as tr

IGNORE = -1
SCORED, IGNORED, INVALID, LOSS_EXCLUDED, LOSS_Q, RANK_HIST, RANK_BINS, STATE_WORDS = 0, 1, 2, 3, 4, 5, 65, 70
LOSS_CAP = np.float32(1024.0)


def score(x, labels):
    """x float32 (B, N), labels integers (B,) -> (loss float64, rank int32, pred int32, prob float64), each (B,)"""
    x = np.ascontiguousarray(x, np.float32)
    labels = np.asarray(labels, np.int64)
    B, N = x.shape
    assert labels.shape == (B,)
    loss, prob = np.zeros(B, np.float64), np.zeros(B, np.float64)
    rank, pred = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        order = tr.order(x[b])
        pred[b] = order[0]
        y = int(labels[b])
        if not 0 <= y < N:
            rank[b] = -1 if y == IGNORE else -2
            continue
        rank[b] = int(np.nonzero(order == y)[0][0])
        if np.isfinite(x[b]).all():
            d = x[b].astype(np.float64) - np.float64(x[b].max())
            s = np.exp(d).sum()
            loss[b], prob[b] = np.log(s) - d[y], np.exp(d[y]) / s
        else:
            loss[b] = prob[b] = np.nan
    return loss, rank, pred, prob


def state(loss_f32, rank, labels, N, pred=None):
    """The integers a meter holds after these rows: (words int64 (70,), per_class int64 (2, N), confusion int64 (N, N) or
    None without ``pred``).  ``loss_f32``: the per-sample float32 losses; a scored row whose loss is not below 1024 (NaN
    included) is counted in LOSS_EXCLUDED instead of the sum; the others add rint(loss * 2^32), half to even."""
    loss_f32 = np.asarray(loss_f32)
    assert loss_f32.dtype == np.float32
    rank, labels = np.asarray(rank, np.int64), np.asarray(labels, np.int64)
    words = np.zeros(STATE_WORDS, np.int64)
    per_class = np.zeros((2, N), np.int64)
    confusion = None if pred is None else np.zeros((N, N), np.int64)
    for b, y in enumerate(labels.tolist()):
        if not 0 <= y < N:
            words[IGNORED if y == IGNORE else INVALID] += 1
            continue
        words[SCORED] += 1
        if loss_f32[b] < LOSS_CAP:
            words[LOSS_Q] += int(np.rint(np.float64(loss_f32[b]) * 2.0 ** 32))
        else:
            words[LOSS_EXCLUDED] += 1
        words[RANK_HIST + min(int(rank[b]), RANK_BINS - 1)] += 1
        per_class[0, y] += 1
        per_class[1, y] += int(rank[b] == 0)
        if confusion is not None:
            confusion[y, int(pred[b])] += 1
    return words, per_class, confusion

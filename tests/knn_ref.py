"""Restatement of the kNN end -- the matches of a gallery search turned into classes through a label per gallery row -- in
plain numpy (test helper): the single written rule that tfimm_hip_knn_vote / tfimm_hip_knn_score (csrc/knn.hip),
``Gallery.vote`` / ``classify`` / ``evaluate`` are held to.

Per query ``b``, from ``indices[b][0:k]`` (int32), ``scores[b][0:k]`` (float32), the gallery labels ``glabels[0:N]``, optionally
``exclude[b]`` (-1 = none), ``inv_temperature >= 0``, ``reduce`` and ``top``:

* candidate ``j`` is VALID when ``0 <= indices[j] < N``, ``indices[j] != exclude[b]``, ``glabels[indices[j]] >= 0`` and -- in
  ``score`` only -- the label is ``< nb_classes``.  An invalid candidate contributes nothing; no label is read for an index
  outside ``[0, N)``; columns ``>= k`` are never read.  Specified for finite scores.
* SUM: ``m`` = the largest valid score, ``w_j = expf((s_j - m) * inv_temperature)`` (one subtraction, one product, expf: with
  ``inv_temperature == 0`` every weight is exactly 1), ``value[c]`` = the sum of ``w_j`` over the valid candidates of class ``c``
  in ascending ``j``, ``count[c]`` their number, ``total`` the sum over all valid candidates in ascending ``j``.
* MAX: ``value[c]`` = the largest raw score among the class's candidates (``-0.0 == +0.0``; of equal maxima the one at the lowest
  ``j`` is written), ``count[c]`` as in SUM, ``total = +0.0``.
* the list: classes by ``value`` descending, equal values by ascending class; the first ``top``; the slots beyond the number of
  distinct classes hold class -1, value +0.0, count 0.
* ``score`` (SUM): with the dense vector ``v[0:C)`` (``value`` of the voted classes, 0 elsewhere) ``pred`` and ``rank`` are what
  tests/score_ref.py gives for the logits row ``v``; ``prob = v[y] / total`` (0 when ``total == 0``), ``loss = 0 - log(prob)``;
  ``y == -1``: ``loss = 0, prob = 0, rank = -1``; any other ``y`` outside ``[0, C)``: the same with ``rank = -2``.

``dtype`` is the arithmetic: ``np.float32`` is the rule the device is bit-equal to wherever expf is exact (weights of 1, MAX);
``np.float64`` is the same rule without rounding, what the weighted cases are measured against.

Deliberately independent of the engine: nothing here imports tfimm.
"""
import numpy as np

SUM, MAX = 0, 1


def _row(idx, sc, glabels, ex, inv_t, reduce, label_end, dtype):
    """one query -> ([(class, value, count)] in list order, total)"""
    N = glabels.shape[0]
    cand = []                                             # (j, label, score) of the valid candidates, ascending j
    for j in range(idx.shape[0]):
        i = int(idx[j])
        if not 0 <= i < N or i == ex:
            continue
        c = int(glabels[i])
        if c < 0 or (label_end is not None and c >= label_end):
            continue
        cand.append((j, c, dtype(sc[j])))
    value, count = {}, {}
    total = dtype(0)
    if reduce == SUM:
        if cand:
            m = max(s for _, _, s in cand)
        with np.errstate(under="ignore", over="ignore"):
            for _, c, s in cand:
                w = np.exp(dtype(dtype(s - m) * dtype(inv_t)))
                assert w.dtype == dtype
                value[c] = dtype(value.get(c, dtype(0)) + w)
                count[c] = count.get(c, 0) + 1
                total = dtype(total + w)
    else:
        for _, c, s in cand:
            if c not in value or s > value[c]:            # of equal maxima the first stays; -0.0 > +0.0 is false
                value[c] = s
            count[c] = count.get(c, 0) + 1
    order = sorted(value, key=lambda c: (-float(value[c]), c))      # -(-0.0) == -(+0.0): the class decides
    return [(c, value[c], count[c]) for c in order], total


def _inputs(indices, scores, glabels, k, exclude):
    indices, scores = np.asarray(indices), np.asarray(scores)
    assert indices.dtype == np.int32 and scores.dtype == np.float32 and indices.shape == scores.shape and indices.ndim == 2
    glabels = np.asarray(glabels)
    assert glabels.dtype == np.int32 and glabels.ndim == 1 and glabels.shape[0] >= 1
    B = indices.shape[0]
    k = indices.shape[1] if k is None else k
    assert 1 <= k <= indices.shape[1]
    ex = np.full(B, -1, np.int64) if exclude is None else np.asarray(exclude, np.int64)
    assert ex.shape == (B,)
    return indices[:, :k], scores[:, :k], glabels, ex


def vote(indices, scores, glabels, k=None, exclude=None, inv_temperature=0.0, reduce=SUM, top=5, dtype=np.float32):
    """-> (classes int32 (B, top), values dtype (B, top), counts int32 (B, top), total dtype (B,))"""
    assert reduce in (SUM, MAX) and top >= 1 and inv_temperature >= 0
    idx, sc, glabels, ex = _inputs(indices, scores, glabels, k, exclude)
    B = idx.shape[0]
    classes = np.full((B, top), -1, np.int32)
    values, counts = np.zeros((B, top), dtype), np.zeros((B, top), np.int32)
    total = np.zeros(B, dtype)
    for b in range(B):
        lst, total[b] = _row(idx[b], sc[b], glabels, int(ex[b]), np.float32(inv_temperature), reduce, None, dtype)
        for p, (c, v, n) in enumerate(lst[:top]):
            classes[b, p], values[b, p], counts[b, p] = c, v, n
    return classes, values, counts, total


def dense(indices, scores, glabels, nb_classes, k=None, exclude=None, inv_temperature=0.0, dtype=np.float32):
    """the SUM vote as the dense vector: (v dtype (B, nb_classes), total dtype (B,))"""
    idx, sc, glabels, ex = _inputs(indices, scores, glabels, k, exclude)
    B = idx.shape[0]
    v, total = np.zeros((B, nb_classes), dtype), np.zeros(B, dtype)
    for b in range(B):
        lst, total[b] = _row(idx[b], sc[b], glabels, int(ex[b]), np.float32(inv_temperature), SUM, nb_classes, dtype)
        for c, val, _ in lst:
            v[b, c] = val
    return v, total


def score(indices, scores, glabels, labels, nb_classes, k=None, exclude=None, inv_temperature=0.0, dtype=np.float32):
    """-> (loss dtype, rank int32, pred int32, prob dtype), each (B,).  ``rank`` and ``pred`` are counted from the voted classes
    (``nb_classes`` may be 2^31 - 1): the classes that come before ``y`` in the order (value descending, equal values by
    ascending class) are the voted ones that beat it and, when ``v[y] == 0``, every unvoted class below ``y``."""
    idx, sc, glabels, ex = _inputs(indices, scores, glabels, k, exclude)
    labels = np.asarray(labels, np.int64)
    B = idx.shape[0]
    assert labels.shape == (B,) and nb_classes >= 1
    loss, prob = np.zeros(B, dtype), np.zeros(B, dtype)
    rank, pred = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        lst, total = _row(idx[b], sc[b], glabels, int(ex[b]), np.float32(inv_temperature), SUM, nb_classes, dtype)
        voted = {c: v for c, v, _ in lst}
        # the first class of the order: every value is >= 0, so it is the best voted class when that one holds more than the 0
        # of the unvoted classes, and class 0 (the lowest class of an all-zero row) otherwise
        pred[b] = lst[0][0] if lst and lst[0][1] > 0 else 0
        y = int(labels[b])
        if not 0 <= y < nb_classes:
            rank[b] = -1 if y == -1 else -2
            continue
        vy = voted.get(y, dtype(0))
        r = sum(1 for c, v in voted.items() if c != y and (v > vy or (v == vy and c < y)))
        if vy == 0:
            r += y - sum(1 for c in voted if c < y)
        rank[b] = r
        with np.errstate(divide="ignore"):
            prob[b] = dtype(vy / total) if total != 0 else dtype(0)
            loss[b] = dtype(0) - np.log(prob[b])
    return loss, rank, pred, prob

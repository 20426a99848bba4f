"""Restatement of the output end -- ``tf.nn.softmax`` + ``tf.math.top_k`` behind ``model(x)`` -- in plain numpy (test
helper): the single written rule that tfimm_hip_topk (csrc/topk.hip) and ``Model.top_k`` are held to.

Order of the ``k`` entries of a row, as a three-level sort key:

1. a NaN comes before every number, whatever its sign or payload (it orders above ``+inf``: a poisoned row shows in the
   answer instead of vanishing);
2. then by value descending, compared as floats -- so ``-0.0`` and ``+0.0`` are equal;
3. equal under 1 and 2 (two NaNs, two equal numbers, two zeros of either sign): the lower column first.  This is
   ``tf.math.top_k``'s documented rule for ties.

``values`` are the selected entries themselves (bit for bit: a selected ``-0.0`` stays ``-0.0``, a NaN keeps its payload),
``indices`` their columns (int32), ``probs`` the float64 softmax over ALL columns of the row at those columns:
``exp(v - m) / sum_i exp(x_i - m)`` with ``m`` the row maximum -- specified for rows whose entries are all finite.

Deliberately independent of the engine: nothing here imports tfimm.
"""
import numpy as np


def order(row):
    """every column of a 1-D float32 row in selection order"""
    row = np.asarray(row, np.float32)
    nan = np.isnan(row)
    value = np.where(nan, np.float32(0), row).astype(np.float64)      # (-0.0 == +0.0 as sort keys, as they are as floats)
    # np.lexsort: the LAST key is the primary one
    return np.lexsort((np.arange(row.size), -value, ~nan))


def softmax64(x):
    """float64 softmax over the last axis of an all-finite array"""
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def topk(x, k, probs=True):
    """x float32 (B, N) -> (indices int32 (B, k), values float32 (B, k), probs float64 (B, k) or None).  ``probs`` of a row
    with a non-finite entry are NaN: not specified."""
    x = np.ascontiguousarray(x, np.float32)
    assert x.ndim == 2 and 1 <= k <= x.shape[1], (x.shape, k)
    idx = np.stack([order(r)[:k] for r in x]).astype(np.int32)
    values = np.take_along_axis(x, idx.astype(np.int64), axis=1)
    if not probs:
        return idx, values, None
    p = np.full(idx.shape, np.nan, np.float64)
    finite = np.isfinite(x).all(axis=1)
    if finite.any():
        p[finite] = np.take_along_axis(softmax64(x[finite]), idx[finite].astype(np.int64), axis=1)
    return idx, values, p


def bits(a):
    """float32 array -> its bit patterns (uint32): what "bit-equal" compares"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)

"""The rule of ``GalleryIndex.neighbours``, restated in numpy on top of tests/index_ref.py.

Every indexed row is its own query (exact: the rows are bf16 values).  Row ``i`` is searched for ``k + 1`` by the rule of the
index -- its probes, the rows of the probed lists, score descending, equal scores by ascending original row -- and of the result
the entry whose index is ``i`` is dropped; if ``i`` is absent (more than ``k`` rows equal to it with lower numbers come first:
they tie with it at its best score) the LAST entry is dropped.  What remains keeps its order: the ``k`` nearest OTHER rows among
the lists that row ``i`` probes, -1 / -inf behind short results."""
import numpy as np

import index_ref as ir


def drop_self(idx, sc, own):
    """(indices (n, k + 1), scores (n, k + 1)) of queries that are the rows ``own`` (n,) -> the same without the own row, or
    without the last column where the own row is absent: (n, k) each"""
    idx, sc, own = np.asarray(idx), np.asarray(sc), np.asarray(own)
    n, k1 = idx.shape
    out_idx, out_sc = np.empty((n, k1 - 1), idx.dtype), np.empty((n, k1 - 1), sc.dtype)
    for i in range(n):
        at = np.flatnonzero(idx[i] == own[i])
        assert len(at) <= 1                                    # a row is never returned twice
        keep = np.delete(np.arange(k1), at[0] if len(at) else k1 - 1)
        out_idx[i], out_sc[i] = idx[i][keep], sc[i][keep]
    return out_idx, out_sc


def neighbours(g, centroids, assignment, nprobe, k):
    """the whole rule for rows ``g`` (N, E) of bf16 values: ``ir.search_index`` of the rows themselves at ``k + 1``, then the drop"""
    g = np.asarray(g, np.float32)
    idx, sc = ir.search_index(g, g, centroids, assignment, nprobe, k + 1)
    return drop_self(idx, sc, np.arange(g.shape[0]))

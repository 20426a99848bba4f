"""The rule of the gallery search over inverted lists (tfimm_hip_embed_search_lists, csrc/embed_lists.hip; ``tfimm.GalleryIndex``;
DESIGN.md 3.28), restated in numpy next to tests/embed_ref.py.

An index over N bf16 rows of E values: L bf16 centroids; the rows in LIST ORDER -- list ``l`` is positions
``offsets[l] : offsets[l + 1]`` --; ``ids[pos]``, the original row of every position.  Inside a list the positions are in
ascending original row: the build makes them so by a stable sort of the assignment.

For a float32 query ``q`` (rounded to bf16 as everywhere): ``probes = er.search(q, centroids, nprobe)[0]``, the ``nprobe`` best
centroids by score descending, equal scores by ascending centroid.  The candidates are the rows of the probed lists; an entry
of ``probes`` outside [0, L) (-1 is the documented "no list") contributes nothing, and a list named more than once counts once:
a row is never a candidate twice.  The result is the ``k`` best candidates by ``er``'s order -- score descending, equal scores
by ascending ORIGINAL row --, the score being ``sum_e bf16(q)[e] * row[e]``.  If the probed lists hold fewer than ``k`` rows the
remaining slots hold index -1 and score -inf."""
import numpy as np

import embed_ref as er


def build_lists(g, assignment, L):
    """(rows in list order, ids int32 (N,), offsets int32 (L + 1,)) of rows ``g`` (N, E) whose list is ``assignment`` (N,): a
    stable sort, so that the original rows ascend inside every list"""
    a = np.asarray(assignment, np.int64)
    order = np.argsort(a, kind="stable")
    offsets = np.searchsorted(a[order], np.arange(L + 1)).astype(np.int32)
    return np.asarray(g)[order], order.astype(np.int32), offsets


def search_lists(q, g_sorted, ids, offsets, probes, k):
    """the rule of tfimm_hip_embed_search_lists: ``q`` float32 (B, E), ``g_sorted`` bf16 values (N, E) in list order, ``ids``
    (N,), ``offsets`` (L + 1,), ``probes`` int (B, nprobe) -> (indices int32 (B, k), scores float32 (B, k))"""
    q, g_sorted = np.asarray(q, np.float32), np.asarray(g_sorted)
    ids, offsets, probes = np.asarray(ids, np.int64), np.asarray(offsets, np.int64), np.asarray(probes, np.int64)
    N, L = g_sorted.shape[0], len(offsets) - 1
    idx = np.full((q.shape[0], k), -1, np.int32)
    sc = np.full((q.shape[0], k), -np.inf, np.float32)
    for b in range(q.shape[0]):
        named = [l for s, l in enumerate(probes[b]) if 0 <= l < L and l not in probes[b][:s]]       # a repeated list counts once
        pos = [np.arange(min(max(offsets[l], 0), N), min(max(offsets[l + 1], 0), N)) for l in named]
        pos = np.concatenate(pos) if pos else np.zeros(0, np.int64)
        if not len(pos):
            continue
        s = er.scores64(q[b:b + 1], g_sorted[pos])[0]
        order = np.lexsort((ids[pos], -s))[:k]                 # score descending, then the ORIGINAL row ascending
        idx[b, :len(order)] = ids[pos][order]
        sc[b, :len(order)] = s[order].astype(np.float32)
    return idx, sc


def search_index(q, g, centroids, assignment, nprobe, k):
    """the whole rule: probe the centroids, then ``search_lists`` over the lists of ``assignment``"""
    centroids = np.asarray(centroids)
    g_sorted, ids, offsets = build_lists(g, assignment, centroids.shape[0])
    probes = er.search(q, centroids, nprobe)[0]
    return search_lists(q, g_sorted, ids, offsets, probes, k)

"""The rules of the index that follows its gallery (tfimm_hip_matches_merge, csrc/embed_merge.hip; ``tfimm.merge_matches``,
``GalleryIndex.search_live``), restated in numpy next to tests/embed_ref.py and tests/index_ref.py.

``merge``: S sets of matches per query, set ``s`` with ``k_s`` (index, score) entries and a ``base``.  Entry ``j`` of set ``s`` is
a candidate iff its index is not negative; its row is ``index + base_s``; its key is the order-preserving key of its score
(csrc/topk_select.h): every NaN ranks above +inf, the two zeros are equal.  The result holds the ``k`` best candidates of all
sets, key descending, equal keys by ascending row; a score is written as the float its key stands for (-0.0 becomes +0.0, any
NaN the one quiet NaN, everything else keeps its bits); the slots behind the last candidate hold index -1 and score -inf.  A
candidate with score -inf is a candidate and comes before that fill.

``search_live``: the index search over the first ``size`` rows (``index_ref.search_index``) and the exact search over the rows
``size ..`` (``embed_ref.search``) with base ``size``, merged."""
import numpy as np

import embed_ref as er
import index_ref as ir


def key_of(bits) -> np.ndarray:
    """topk_sel::key_of over uint32 bit patterns"""
    b = np.asarray(bits, np.uint32).copy()
    nan = (b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    b[b == np.uint32(0x80000000)] = 0
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[nan] = np.uint32(0xffffffff)
    return key


def bits_of(key) -> np.ndarray:
    """topk_sel::bits_of: the float32 bits a key stands for"""
    key = np.asarray(key, np.uint32)
    return np.where(key & np.uint32(0x80000000), key ^ np.uint32(0x80000000), ~key).astype(np.uint32)


def merge(parts, bases=None, k=None):
    """``parts``: a sequence of (indices int (B, k_s), scores float32 (B, k_s)); ``bases``: an offset per part (default 0);
    ``k``: default the widest part -> (indices int32 (B, k), scores float32 (B, k))"""
    parts = [(np.asarray(i, np.int64), np.ascontiguousarray(s, np.float32)) for i, s in parts]
    bases = [0] * len(parts) if bases is None else list(bases)
    k = max(i.shape[1] for i, _ in parts) if k is None else k
    B = parts[0][0].shape[0]
    idx = np.full((B, k), -1, np.int32)
    sc = np.full((B, k), 0xff800000, np.uint32)                  # -inf
    for b in range(B):
        rows = np.concatenate([i[b][i[b] >= 0] + base for (i, _), base in zip(parts, bases)])
        keys = np.concatenate([key_of(er.bits(s[b]))[i[b] >= 0] for i, s in parts]).astype(np.int64)
        order = np.lexsort((rows, -keys))[:k]                    # key descending, then row ascending
        idx[b, :len(order)] = rows[order]
        sc[b, :len(order)] = bits_of(keys[order].astype(np.uint32))
    return idx, sc.view(np.float32)


def search_live(q, g, centroids, assignment, nprobe, k, probes=None):
    """the rule of ``GalleryIndex.search_live``: ``g`` (N, E) are all rows of the gallery, ``assignment`` (size,) the lists of
    the first ``size`` of them -- the snapshot --; the rows behind it are searched exactly.  ``probes`` (B, nprobe), if given,
    stand for ``er.search(q, centroids, nprobe)[0]``: centroids that k-means left are no grid data, and where two of them
    score within a float32 rounding of each other the probe -- tfimm_hip_embed_search, held to its own rule elsewhere -- is
    taken from the device as tests/test_gpu_search_index.py takes it"""
    g, size = np.asarray(g), len(assignment)
    if probes is None:
        head = ir.search_index(q, g[:size], centroids, assignment, nprobe, k)
    else:
        head = ir.search_lists(q, *ir.build_lists(g[:size], assignment, np.asarray(centroids).shape[0]), probes, k)
    fresh = g.shape[0] - size
    if not fresh:
        return head
    return merge([head, er.search(q, g[size:], min(k, fresh))], [0, size], k)

"""The cluster end's rules, restated in numpy (include/tfimm_hip.h, CLUSTER END): the assignment of
tfimm_hip_cluster_assign, the summation order of tfimm_hip_segment_mean, and the host loops ``Gallery.prototypes`` and
``Gallery.kmeans`` compose from them."""
import numpy as np

import embed_ref as er

f32, i32 = np.float32, np.int32
RUN = 256              # TFIMM_SEGMENT_RUN: entries per run of the summation rule


def scores64(g, c) -> np.ndarray:
    """float64 scores (N, C) of gallery rows against centroids, both bf16 values already"""
    return np.asarray(g, np.float64) @ np.asarray(c, np.float64).T


def assign(g, c):
    """the rule of tfimm_hip_cluster_assign: ``s[n][j] = sum_e g[n][e] * c[j][e]`` (here in float64), per row the ``j`` with
    the largest score, of equal scores the lowest -> (assign int32 (N,), score float32 (N,))"""
    s = scores64(g, c)
    j = np.argmax(s, axis=1)                                  # the first of equal maxima; -0.0 == +0.0
    return j.astype(i32), s[np.arange(s.shape[0]), j].astype(f32)


def segment_mean(g, rows, offsets, run=RUN):
    """the rule of tfimm_hip_segment_mean: segment ``c`` is ``rows[offsets[c]:offsets[c + 1]]`` (offsets clamped to [0, M], an
    end below its begin: empty); its entries, valid or not, are cut into runs of ``run`` counted from the segment's begin; a
    run's partial sum starts at +0.0 and adds the run's valid rows (those inside [0, N)) one by one in list order; the
    segment's sum starts at +0.0 and adds the partial sums in ascending run order; every addition is a float32 addition;
    one float32 division by ``float32(count)``.  -> (mean float32 (C, E), counts int32 (C,))"""
    g = np.ascontiguousarray(g, f32)
    rows = np.asarray(rows, np.int64).reshape(-1)
    offsets = np.asarray(offsets, np.int64)
    (N, E), M, C = g.shape, rows.shape[0], offsets.shape[0] - 1
    mean, counts = np.zeros((C, E), f32), np.zeros(C, i32)
    for c in range(C):
        s = int(np.clip(offsets[c], 0, M))
        e = max(int(np.clip(offsets[c + 1], 0, M)), s)
        total, n = np.zeros(E, f32), 0
        for p in range(s, e, run):
            part = np.zeros(E, f32)
            for i in rows[p:min(p + run, e)]:
                if 0 <= i < N:
                    part = part + g[i]
                    n += 1
            total = total + part
        if n:
            mean[c] = total / f32(n)
        counts[c] = n
    return mean, counts


def mean64(g, rows, offsets):
    """the exact means (float64) of the valid entries, and per element ``sum_i |x_i|`` -- what the error bound is made of"""
    g = np.asarray(g, np.float64)
    rows, offsets = np.asarray(rows, np.int64).reshape(-1), np.asarray(offsets, np.int64)
    C = offsets.shape[0] - 1
    mean, mass = np.zeros((C, g.shape[1])), np.zeros((C, g.shape[1]))
    for c in range(C):
        r = rows[offsets[c]:offsets[c + 1]]
        r = r[(r >= 0) & (r < g.shape[0])]
        if r.size:
            mean[c], mass[c] = g[r].sum(0) / r.size, np.abs(g[r]).sum(0)
    return mean, mass


def csr(groups, nb):
    """the CSR form ``Gallery`` builds with torch: a stable sort of the groups, ``searchsorted`` of 0 .. nb -> (rows, offsets).
    A group outside [0, nb) lies before offsets[0] or behind offsets[nb]: it belongs to no segment"""
    groups = np.asarray(groups, np.int64)
    order = np.argsort(groups, kind="stable")
    return order.astype(i32), np.searchsorted(groups[order], np.arange(nb + 1), side="left").astype(i32)


def normalize_bf16(x) -> np.ndarray:
    """float32 rows -> L2-normalised (embed_ref.l2_normalize) -> float32 -> bf16 (nearest even), as float32"""
    return er.bf16_round(er.l2_normalize(np.asarray(x, f32)).astype(f32))


def prototypes(g, labels, nb_classes, normalize=True):
    """``Gallery.prototypes``: row ``c`` the mean of the rows labelled ``c``, normalised if asked, rounded to bf16; a class
    without rows: a zero row labelled -1 -> (rows float32 (nb_classes, E) of bf16 values, labels int32)"""
    mean, counts = segment_mean(g, *csr(labels, nb_classes))
    rows = normalize_bf16(mean) if normalize else er.bf16_round(mean)
    return rows, np.where(counts > 0, np.arange(nb_classes), -1).astype(i32)


def kmeans(g, init, iters):
    """``Gallery.kmeans`` from initial centroid values ``init`` (float32 (K, E)): normalise and round them; ``iters`` times
    assign -> means of the groups -> normalise, round (an empty cluster keeps its centroid); one more assign
    -> (centroids float32 (K, E) of bf16 values, assignment, scores, counts, moved)"""
    g = np.ascontiguousarray(g, f32)
    cen = normalize_bf16(init)
    K = cen.shape[0]
    a, s = assign(g, cen)
    moved = np.zeros(iters, i32)
    for it in range(iters):
        mean, counts = segment_mean(g, *csr(a, K))
        cen = np.where((counts > 0)[:, None], normalize_bf16(mean), cen)
        a2, s = assign(g, cen)
        moved[it] = int((a2 != a).sum())
        a = a2
    return cen, a, s, np.bincount(a, minlength=K).astype(i32), moved


def l2_normalize_f32(x) -> np.ndarray:
    """tfimm_hip_l2_normalize's float32 rule (include/tfimm_hip.h) step by step: lane l sums the squares of columns l, l + 64,
    ... in ascending order with a fused multiply-add, the 64 partial sums go through the six-step butterfly, then a correctly
    rounded square root, reciprocal and product.  (The fused multiply-add is formed in float64 -- the product is exact
    there -- and rounded once more to float32: equal to the device's single rounding except in double-rounding corner cases.)"""
    x = np.ascontiguousarray(x, f32)
    B, E = x.shape
    lanes = np.zeros((B, 64), f32)
    for c0 in range(0, E, 64):
        v = np.zeros((B, 64), np.float64)
        v[:, :min(64, E - c0)] = x[:, c0:c0 + 64]
        lanes = (v * v + lanes.astype(np.float64)).astype(f32)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, np.arange(64) ^ o]
    inv = f32(1) / np.sqrt(np.maximum(lanes[:, :1], f32(1e-12)))
    return x * inv

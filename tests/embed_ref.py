"""The embedding end's rules, restated in numpy: the head of ``EmbeddingModel`` in float64 from its
unfolded weights, bf16 rounding, ``tf.math.l2_normalize`` and the gallery search of tfimm_hip_embed_search with its order."""
import numpy as np

BN_EPS = 1e-3          # tf.keras.layers.BatchNormalization's default


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def bf16_round(x) -> np.ndarray:
    """float32 -> the nearest bf16 (ties to even), returned as float32; finite inputs"""
    b = bits(x).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) >> 16 << 16
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def head(features, weights, normalize=False) -> np.ndarray:
    """Dense(with bias) -> BatchNormalization(scale=False, eps=1e-3, inference) over the last axis of ``features``, in
    float64 from the UNFOLDED weights ``emb/fc/kernel``, ``emb/fc/bias``, ``emb/bn/beta``, ``emb/bn/moving_mean``,
    ``emb/bn/moving_variance`` (reference tfimm/models/embedding_model.py:31-32); then ``l2_normalize`` if asked"""
    w = {k: np.asarray(weights["emb/" + k], np.float64) for k in ("fc/kernel", "fc/bias", "bn/beta", "bn/moving_mean", "bn/moving_variance")}
    y = np.asarray(features, np.float64) @ w["fc/kernel"] + w["fc/bias"]
    y = (y - w["bn/moving_mean"]) / np.sqrt(w["bn/moving_variance"] + BN_EPS) + w["bn/beta"]
    return l2_normalize(y) if normalize else y


def l2_normalize(x) -> np.ndarray:
    """tf.math.l2_normalize(x, axis=-1) in float64: x * rsqrt(max(sum(x^2), 1e-12))"""
    x = np.asarray(x, np.float64)
    return x / np.sqrt(np.maximum((x * x).sum(-1, keepdims=True), 1e-12))


def scores64(q, g) -> np.ndarray:
    """float64 scores (B, N) of float32 queries (rounded to bf16 here) against gallery rows that are bf16 values already"""
    return bf16_round(q).astype(np.float64) @ np.asarray(g, np.float64).T


def select(scores, k):
    """per row the k best of ``scores``: score descending, equal scores by ascending index -> (indices int32, scores)"""
    s = np.asarray(scores)
    idx = np.empty((s.shape[0], k), np.int32)
    for b, row in enumerate(s):
        order = sorted(range(row.shape[0]), key=lambda n: (-row[n], n)) if row.shape[0] <= 64 else \
            np.lexsort((np.arange(row.shape[0]), -row))
        idx[b] = np.asarray(order[:k], np.int32)
    return idx, np.take_along_axis(s, idx.astype(np.int64), 1)


def search(q, g, k):
    """the rule of tfimm_hip_embed_search: ``score[b][n] = sum_e bf16(q)[b][e] * g[n][e]`` (here exactly, in float64),
    the k best per query by (score descending, index ascending) -> (indices int32 (B, k), scores float32 (B, k))"""
    idx, s = select(scores64(q, g), k)
    return idx, s.astype(np.float32)

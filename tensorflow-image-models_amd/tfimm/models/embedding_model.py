"""``EmbeddingModel``: any backbone of this package + a Dense layer + a BatchNorm without scale behind its
``forward_features`` (reference tfimm/models/embedding_model.py), lowered into ONE layer program: the head is the last GEMM
of the program and of its recording, with the BatchNorm folded into it on the host."""
import dataclasses
from collections import OrderedDict
from typing import List, Optional

import numpy as np

from ..engine.graph import Builder
from .model import Model, Tensor, WeightSpec

#: tf.keras.layers.BatchNormalization's default epsilon (the reference passes none, embedding_model.py:18-20)
BN_EPS = 1e-3


def fold_head(kernel, bias, beta, mean, var, eps: float = BN_EPS):
    """Dense + BatchNorm(scale=False) at inference as one Dense: ``s = 1 / sqrt(var + eps)``, ``W' = W * s``,
    ``b' = (b - mean) * s + beta`` -- evaluated in float64, returned as float32 (kernel (F, E), bias (E,))."""
    s = 1.0 / np.sqrt(np.asarray(var, np.float64) + eps)
    w = np.asarray(kernel, np.float64) * s[None, :]
    b = (np.asarray(bias, np.float64) - np.asarray(mean, np.float64)) * s + np.asarray(beta, np.float64)
    return w.astype(np.float32), b.astype(np.float32)


class EmbeddingModel(Model):
    """``EmbeddingModel(backbone, embed_dim)``: ``backbone.forward_features`` -> Dense(embed_dim, with bias) ->
    BatchNormalization(scale=False, epsilon=1e-3), the reference's class of the same name (embedding_model.py:12-34) at
    inference.  A ``Model`` like every other: ``model(x)`` takes what every model takes (float / bf16 arrays, ``pre(img)``,
    the ``resize`` / ``antialias`` forms, lists of mixed sizes; ``branches`` and ``micro_batch`` as usual) and runs one layer
    program whose last GEMM is the head; the classifier of the backbone is not part of it.

    Weights: all of the backbone's under their own names (its classifier included: the variable inventory is the union, the
    program does not read it) plus ``emb/fc/kernel`` (F, embed_dim), ``emb/fc/bias``, ``emb/bn/beta``,
    ``emb/bn/moving_mean``, ``emb/bn/moving_variance`` -- no gamma.  The backbone's weights are a SNAPSHOT taken at
    construction: a later ``backbone.set_weights`` does not propagate (set them here, under the same names); the backbone
    object itself -- its programs, plans, recordings and keys -- is never touched.

    ``model(x)`` is (B, embed_dim) float32 for a backbone whose ``forward_features`` is (B, F).  The head applies to the
    last axis, as Keras' Dense and BatchNorm(axis=-1) do: a backbone whose features are a map (B, H, W, C) -- ResNet -- gives
    (B, H, W, embed_dim), what the reference gives.  A backbone with several feature rows per image that are no map
    (distilled DeiT: (B, 2, D)) is refused.

    Construction builds a classifier-free instance of the backbone's class (with initialised weights of its own, never
    used) and lowers it once over the snapshot to learn ``F`` and the layout of ``features``: for a ViT-L-sized backbone that
    is a second weight set on the host and one host-side lowering per constructor call -- seconds, once per model.

    ``normalize=True`` (an extension; the default is the reference's behaviour) appends ``tf.math.l2_normalize`` over the
    last axis (tfimm_hip_l2_normalize); the marked output is the normalised tensor."""

    def __init__(self, backbone: Model, embed_dim: int, normalize: bool = False, name: Optional[str] = None):
        if not isinstance(backbone, Model) or isinstance(backbone, EmbeddingModel):
            raise ValueError(f"EmbeddingModel: backbone must be a tfimm model, got {type(backbone).__name__}")
        if isinstance(embed_dim, bool) or not isinstance(embed_dim, (int, np.integer)) or embed_dim < 1:
            raise ValueError(f"EmbeddingModel: embed_dim = {embed_dim!r}, must be an integer >= 1")
        self.embed_dim = int(embed_dim)
        self.normalize = bool(normalize)
        # the backbone without its classifier: an instance of its class on nb_classes = 0 that only LOWERS (every family
        # lowers that configuration); it holds no weights of interest -- the builder reads this model's
        self._shadow = type(backbone)(dataclasses.replace(backbone.cfg, nb_classes=0), name=backbone.name)
        self._backbone_specs = OrderedDict(backbone._specs)
        self._backbone_feature_names = list(backbone.feature_names)
        snapshot = {k: np.array(v, dtype=np.float32, copy=True) for k, v in backbone.weights.items()}
        # the width (and the layout) of `features`: one throw-away lowering of the classifier-free backbone
        b = Builder(snapshot)
        self._shadow.lower(b, *backbone.cfg.input_size, False)
        f = b.p.outputs["features"]
        # what forward_features hands out for one image, as Model._run shapes it before the family's _shape_output
        raw = (1, f.H, f.W, f.C) if f.H > 0 else (1, f.C) if f.rows == 1 else (1, f.rows, f.C)
        import torch
        shaped = self._shadow._shape_output("features", torch.zeros(raw))
        if not (f.rows == 1 or f.H * f.W == f.rows) or shaped.ndim not in (2, 4):
            raise ValueError(f"EmbeddingModel: forward_features of {backbone.name} is {('B',) + tuple(shaped.shape[1:])}, not "
                             f"(B, F): a backbone with several feature rows per image (a distilled DeiT) is not supported")
        self.nb_features = int(f.C)
        super().__init__(backbone.cfg, name or f"{backbone.name}_embedding")
        self._weights.update(snapshot)

    # -- weights ---------------------------------------------------------------------------------
    def weight_specs(self):
        s = OrderedDict(self._backbone_specs)
        s["emb/fc/kernel"] = WeightSpec((self.nb_features, self.embed_dim), "dense")          # glorot_uniform
        s["emb/fc/bias"] = WeightSpec((self.embed_dim,), "bias")
        s["emb/bn/beta"] = WeightSpec((self.embed_dim,), "beta")
        s["emb/bn/moving_mean"] = WeightSpec((self.embed_dim,), "mean")
        s["emb/bn/moving_variance"] = WeightSpec((self.embed_dim,), "var")
        return s

    @property
    def keys_to_ignore_on_load(self):
        return self._shadow.keys_to_ignore_on_load

    @property
    def feature_names(self) -> List[str]:
        names = self._backbone_feature_names
        return names[:names.index("features") + 1] + ["embeddings"]

    # -- lowering --------------------------------------------------------------------------------
    def lower(self, b: Builder, H: int, W: int, want_features: bool):
        p = b.p
        self._shadow.lower(b, H, W, want_features)
        feats = p.outputs["features"]
        # a classifier-free backbone hands its (pooled) features out as "logits": not an output here, and the op that only
        # made them (ResNet's pooling behind the map) is not part of the program
        stale = p.outputs.pop("logits")
        if stale.id != feats.id:
            p.tensors[stale.id].keep = False
            self._drop_dead_ops(p, stale.id)
        w = self._weights
        kernel, bias = fold_head(w["emb/fc/kernel"], w["emb/fc/bias"], w["emb/bn/beta"], w["emb/bn/moving_mean"],
                                 w["emb/bn/moving_variance"])
        b.define("emb/fc/kernel:bn", kernel)
        b.define("emb/fc/bias:bn", bias)
        emb = b.dense(feats, "emb/fc/kernel:bn", "emb/fc/bias:bn", out_f32=True, mx=False, cite="embedding_model.py:31-32",
                      name="embeddings")
        if self.normalize:
            emb = b.l2_normalize(emb, name="embeddings")
        p.mark_output("embeddings", emb)

    @staticmethod
    def _drop_dead_ops(p, stale_id: int) -> None:
        """Remove the ops that only served the dropped tensor ``stale_id``: walking backwards, an op all of whose outputs are
        dead (read by no remaining op, not kept) goes, and inputs that lose their last reader that way become dead in turn.
        Ends with the check that nothing left in the program writes a tensor of that chain."""
        dead = {stale_id}
        for i in range(len(p.ops) - 1, -1, -1):
            op = p.ops[i]
            outs = ([op.output] if op.output is not None else []) + list(op.extra_outputs)
            if not outs or not set(outs) <= dead:
                continue
            del p.ops[i]
            still_read = {t for o in p.ops for t in o.inputs}
            dead.update(t for t in op.inputs if t not in still_read and not p.tensors[t].keep)
        written = {t for o in p.ops for t in ([o.output] if o.output is not None else []) + list(o.extra_outputs)}
        read = {t for o in p.ops for t in o.inputs}
        left = [t for t in dead & written if t not in read]
        assert not left, f"ops behind `features` still write tensors nobody reads: {left}"

    def program(self, H=None, W=None, want_features=False, top_k=None):
        if top_k:
            raise ValueError(f"{self.name}: top_k needs a classifier, an embedding model has none")
        return super().program(H, W, want_features)

    def _shape_output(self, name, v):
        if name == "embeddings":
            return v
        return self._shadow._shape_output(name, v)

    # -- forward -----------------------------------------------------------------------------------
    def __call__(self, x, training: bool = False, return_features: bool = False):
        """(B, embed_dim) float32; with ``return_features`` also the dictionary of the backbone's features in order, up to
        and including ``features``, then ``embeddings`` (embedding_model.py:26-34)."""
        if training:
            raise NotImplementedError("This engine implements the inference forward path only (training=False).")
        out = self._run(x, return_features)
        return self._finish(out, "embeddings", return_features)

    def top_k(self, x, k: int = 5, training: bool = False):
        raise ValueError(f"{self.name}: top_k needs a classifier, an embedding model has none (search a Gallery instead)")

    def evaluate(self, x, labels, meter=None, training: bool = False):
        raise ValueError(f"{self.name}: evaluate needs a classifier, an embedding model has none (search a Gallery instead)")

    def search(self, x, gallery, k: int = 5, method: str = "auto"):
        """``gallery.search_with(model(x), k, method=method)``: the model's recording, then the two launches of the search, on the
        same stream; ``Matches(indices, scores)``, each (B, k), ``k`` up to 256.  The embeddings never leave the device."""
        if gallery.dim != self.embed_dim:
            raise ValueError(f"{self.name}: embeddings have {self.embed_dim} columns, the gallery holds rows of {gallery.dim}")
        gallery._route(k, method)
        emb = self(x)
        if len(emb.shape) != 2:
            raise ValueError(f"{self.name}: embeddings are a map {emb.shape} (the backbone's forward_features is one): a gallery "
                             f"holds one row per image, pool the map first")
        return gallery.search_with(emb, k, method=method)

    def search_coarse(self, x, gallery, k: int = 5, candidates=None):
        """``gallery.search_coarse(model(x), k, candidates)``: the model's recording, then the three launches of the
        coarse-to-fine search (fp8 scan, merge, exact bf16 rerank), on the same stream; ``Matches(indices, scores)``, each
        (B, k).  The gallery needs its coarse copy (``gallery.build_coarse()``)."""
        if gallery.dim != self.embed_dim:
            raise ValueError(f"{self.name}: embeddings have {self.embed_dim} columns, the gallery holds rows of {gallery.dim}")
        gallery._coarse_args(k, candidates)
        return gallery.search_coarse(self._embeddings_for(x, gallery), k, candidates)

    def search_index(self, x, index, k: int = 5, nprobe: int = 8):
        """``index.search(model(x), k, nprobe)`` for a ``tfimm.GalleryIndex``: the model's recording, then the probe of the
        centroids and the search of the probed lists, on the same stream; ``Matches(indices, scores)``, each (B, k).  Every
        argument is checked before the forward pass runs."""
        if index.dim != self.embed_dim:
            raise ValueError(f"{self.name}: embeddings have {self.embed_dim} columns, the index holds rows of {index.dim}")
        index._args(k, nprobe)
        return index.search(self._embeddings_for(x, index), k, nprobe)

    def search_live(self, x, index, k: int = 5, nprobe: int = 8):
        """``index.search_live(model(x), k, nprobe)`` for a ``tfimm.GalleryIndex`` whose gallery has grown: the probed lists
        and every row added since the build; ``Matches(indices, scores)``, each (B, k).  Every argument is
        checked before the forward pass runs."""
        if index.dim != self.embed_dim:
            raise ValueError(f"{self.name}: embeddings have {self.embed_dim} columns, the index holds rows of {index.dim}")
        index._live_args(k, nprobe, "single", "GalleryIndex.search_live")
        return index.search_live(self._embeddings_for(x, index), k, nprobe)

    def _embeddings_for(self, x, gallery):
        emb = self(x)
        if len(emb.shape) != 2:
            raise ValueError(f"{self.name}: embeddings are a map {emb.shape} (the backbone's forward_features is one): a gallery "
                             f"holds one row per image, pool the map first")
        return emb

    def classify(self, x, gallery, k: int = 20, temperature=0.07, top: int = 5, reduce: str = "sum", exclude=None):
        """``gallery.classify(model(x), ...)``: the classes of the images from their ``k`` nearest labelled gallery rows --
        ``Votes(classes, values, counts, total)`` -- behind the model's recording on the same stream; neither embeddings
        nor matches leave the device.  Every argument is checked before the forward pass runs."""
        if gallery.dim != self.embed_dim:
            raise ValueError(f"{self.name}: embeddings have {self.embed_dim} columns, the gallery holds rows of {gallery.dim}")
        run = gallery._plan_classify(f"{self.name}: classify", int(self._batch_of(x)), k, temperature, top, reduce, exclude)
        return run(self._embeddings_for(x, gallery))

    def evaluate_knn(self, x, labels, gallery, k: int = 20, temperature=0.07, meter=None, nb_classes=None, exclude=None):
        """``gallery.evaluate(model(x), labels, ...)``: the kNN probe of this embedding -- ``Scores(loss, rank, pred, prob)``
        of the weighted vote against the true labels, added to ``meter`` on the device (what ``LinearProbe`` is to a
        classifier head, without any training).  Every argument is checked before the forward pass runs."""
        if gallery.dim != self.embed_dim:
            raise ValueError(f"{self.name}: embeddings have {self.embed_dim} columns, the gallery holds rows of {gallery.dim}")
        run = gallery._plan_evaluate(f"{self.name}: evaluate_knn", int(self._batch_of(x)), labels, k, temperature, meter,
                                     nb_classes, exclude)
        return run(self._embeddings_for(x, gallery))

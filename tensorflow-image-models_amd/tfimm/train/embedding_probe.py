"""``EmbeddingProbe``: an embedding head distilled from a teacher's embeddings on frozen features, on the device (DESIGN.md
3.23).

The reference's ``DistillationProblem`` (tfimm/train/problems/distillation.py) with a frozen student backbone: the student's
``fc`` layer is trained so that its L2-normalised embeddings reproduce the teacher's, ``loss = mean_b sum_e (l2(student) -
l2(teacher))^2 + weight_decay * sum(w^2) / nb_variables``.  A step is three launches on the current stream and no host
synchronisation:

1. ``tfimm_hip_gemm``          student = f16 . W16^T + bias   (float32 out)
2. ``tfimm_hip_distill_grad``  loss, cosine and the bf16 rows d loss / d student
3. ``tfimm_hip_head_update``   the weight gradient and the optimizer step (``C = embed_dim``, ``labels = valid``)

The contract of launch 2 is in include/tfimm_hip.h; tests/distill_ref.py restates the step on the CPU.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from ..engine import ffi
from ..models.model import Tensor
from ._head_probe import _HeadProbe

#: what ``EmbeddingProbe.step`` and ``Model.distill_head`` return: two float32 ``Tensor`` of shape (B,) -- every row's loss and
#: the cosine between student and teacher BEFORE the step (both 0 for an ignored row)
DistillResult = namedtuple("DistillResult", ["loss", "cosine"])


class EmbeddingProbe(_HeadProbe):
    """``EmbeddingProbe(dim, embed_dim, normalize_embeddings=True, optimizer="sgd", lr=0.1, betas=(0.9, 0.999), epsilon=1e-7,
    weight_decay=0.0, seed=0)`` -- the optimizer arguments are ``LinearProbe``'s, ``normalize_embeddings`` is the reference's
    ``DistillationConfig`` field: both sides are L2-normalised before they are compared (without it the loss is the plain
    squared distance).

    The probe trains ONE Dense layer (dim, embed_dim) with bias: the inference form of ``EmbeddingModel``'s ``fc`` +
    ``bn(scale=False)``, which is what ``install`` writes back.  Training-mode BatchNorm statistics are out of scope.

    ``weight_decay`` follows the reference's distillation rule, ``reg = weight_decay * sum(w^2) / nb_variables`` over kernel
    and bias with ``nb_variables = dim * embed_dim + embed_dim`` -- NOT ``LinearProbe``'s ``weight_decay * sum(w^2)``."""

    _NAME, _COLS = "EmbeddingProbe", "embed_dim"
    _COLS_MAX, _COLS_MAX_NAME = ffi.DISTILL_MAX_E, f"TFIMM_DISTILL_MAX_E = {ffi.DISTILL_MAX_E}"

    def __init__(self, dim, embed_dim, normalize_embeddings=True, optimizer="sgd", lr=0.1, betas=(0.9, 0.999), epsilon=1e-7,
                 weight_decay=0.0, seed=0):
        super().__init__(dim, embed_dim, optimizer, lr, betas, epsilon, weight_decay, seed)
        self.normalize_embeddings = bool(normalize_embeddings)

    @classmethod
    def for_model(cls, model, **kw):
        """a probe of an ``EmbeddingModel``'s feature width and embedding size that starts from its head as the model runs
        it: ``fold_head`` of its ``emb/*`` weights"""
        from ..models.embedding_model import EmbeddingModel, fold_head
        if not isinstance(model, EmbeddingModel):
            raise ValueError(f"EmbeddingProbe.for_model: expected a tfimm.EmbeddingModel, got {type(model).__name__}")
        w = model.weights
        kernel, bias = fold_head(w["emb/fc/kernel"], w["emb/fc/bias"], w["emb/bn/beta"], w["emb/bn/moving_mean"],
                                 w["emb/bn/moving_variance"])
        probe = cls(int(kernel.shape[0]), int(kernel.shape[1]), **kw)
        probe._host = probe._zero_state(kernel.copy(), bias.copy())
        return probe

    def _decay(self) -> float:
        return self.weight_decay / (self.dim * self.embed_dim + self.embed_dim)

    # -- inputs --------------------------------------------------------------------------------------
    def _targets(self, teacher, valid, B, what):
        """``teacher`` and ``valid`` checked on the host against a batch of ``B``; returns the callable that uploads them:
        (float32 (B, embed_dim), int32 (B,) of 0 / -1), both on the device"""
        import torch
        t = teacher.torch() if isinstance(teacher, Tensor) else teacher if isinstance(teacher, torch.Tensor) else np.asarray(teacher)
        dt = str(t.dtype).replace("torch.", "")
        if dt not in ("float32", "bfloat16"):
            raise ValueError(f"{what}: teacher: expected float32 or bfloat16, got {t.dtype}")
        if t.ndim != 2 or t.shape[1] != self.embed_dim:
            raise ValueError(f"{what}: teacher: expected shape (B, {self.embed_dim}), got {tuple(t.shape)} (one embedding per "
                             f"image: pool a map first)")
        if t.shape[0] != B:
            raise ValueError(f"{what}: teacher: {t.shape[0]} rows for a batch of {B}")
        v = valid
        if v is not None:
            v = v.torch() if isinstance(v, Tensor) else v if isinstance(v, torch.Tensor) else np.asarray(v)
            kind = ("b" if v.dtype == torch.bool else "f" if v.dtype.is_floating_point or v.dtype.is_complex else "i") \
                if isinstance(v, torch.Tensor) else v.dtype.kind
            if kind not in "biu":
                raise ValueError(f"{what}: valid: expected a boolean or integer mask, got {v.dtype}")
            if v.ndim != 1 or v.shape[0] != B:
                raise ValueError(f"{what}: valid: expected shape ({B},), got {tuple(v.shape)}")

        def upload():
            if not torch.cuda.is_available():
                raise RuntimeError("tfimm (MI355X engine) needs a ROCm GPU: no CPU execution path exists.")
            src = t
            if isinstance(src, np.ndarray):
                src = torch.from_numpy(np.ascontiguousarray(src.view(np.int16) if dt == "bfloat16" else src))
                if dt == "bfloat16":
                    src = src.view(torch.bfloat16)
            tt = src.to("cuda", non_blocking=True).to(torch.float32).contiguous()      # bf16 is widened on the device
            if v is None:
                y = torch.zeros(B, dtype=torch.int32, device="cuda")
            else:
                m = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v != 0))
                y = (m.to("cuda", non_blocking=True) != 0).to(torch.int32) - 1              # true -> 0, false -> -1
            return tt, y
        return upload

    # -- the public surface ----------------------------------------------------------------------------
    def __call__(self, features, normalize: bool = False):
        """float32 embeddings (B, embed_dim) of ``features`` under the current weights: the product a step starts with --
        raw, like ``EmbeddingModel``'s; L2-normalised (tfimm_hip_l2_normalize) if the probe was built with
        ``normalize_embeddings`` AND ``normalize=True`` is passed"""
        import torch
        B = self._forward(features)
        out = self._out[:B].clone()
        if B and normalize and self.normalize_embeddings:
            ffi.check(ffi.lib.tfimm_hip_l2_normalize(out.data_ptr(), self.embed_dim, B, self.embed_dim, out.data_ptr(), self.embed_dim,
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tfimm_hip_l2_normalize")
        return Tensor(out)

    def step(self, features, teacher, valid=None) -> DistillResult:
        """One optimizer step on a batch: ``features`` (B, dim) as ``LinearProbe.step`` takes them; ``teacher`` (B, embed_dim),
        float32 or bf16 -- a ``tfimm.Tensor``, a torch tensor on either side or a numpy array; ``valid`` ``None`` or a (B,)
        boolean / integer mask, a row whose entry is false / zero is ignored.  Returns ``DistillResult(loss, cosine)`` of the
        batch under the weights BEFORE the step; nothing waits for the device."""
        import torch
        B, stage = self._features(features, "EmbeddingProbe.step")
        up_targets = teacher if callable(teacher) else self._targets(teacher, valid, B, "EmbeddingProbe.step")
        stage()
        t, y = up_targets()
        loss = torch.empty(B, dtype=torch.float32, device="cuda")
        cosine = torch.empty(B, dtype=torch.float32, device="cuda")
        if B == 0:
            return DistillResult(Tensor(loss), Tensor(cosine))
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        E = self.embed_dim
        self._gemm(B, st)
        ffi.check(ffi.lib.tfimm_hip_distill_grad(self._out.data_ptr(), E, t.data_ptr(), E, B, E, y.data_ptr(),
                                                 int(self.normalize_embeddings), self._g.data_ptr(), self._ldg, loss.data_ptr(),
                                                 cosine.data_ptr(), st), "tfimm_hip_distill_grad")
        self._update(B, y, st)
        self._keep = (t, y)                              # the launches read them asynchronously
        return DistillResult(Tensor(loss), Tensor(cosine))

    def install(self, model) -> None:
        """hand the head to an ``EmbeddingModel``: ``emb/fc/kernel = W``, ``emb/fc/bias = b``, ``emb/bn/beta = 0``,
        ``emb/bn/moving_mean = 0`` and ``emb/bn/moving_variance = float32(1 - 1e-3)``, with which ``fold_head`` gives W and b
        back to the float32 bit (``model.set_weights(..., strict=False)``: its programs, plans and recordings are rebuilt on the
        next call)"""
        from ..models.embedding_model import BN_EPS, EmbeddingModel
        if not isinstance(model, EmbeddingModel):
            raise ValueError(f"EmbeddingProbe.install: expected a tfimm.EmbeddingModel, got {type(model).__name__}")
        shape = (model.nb_features, model.embed_dim)
        if shape != (self.dim, self.embed_dim):
            raise ValueError(f"EmbeddingProbe.install: the probe is ({self.dim}, embed_dim = {self.embed_dim}), the head of "
                             f"{model.name} is (nb_features, embed_dim) = {shape}")
        w = self.weights
        zero = np.zeros(self.embed_dim, np.float32)
        model.set_weights({"emb/fc/kernel": w["kernel"], "emb/fc/bias": w["bias"], "emb/bn/beta": zero,
                           "emb/bn/moving_mean": zero.copy(),
                           "emb/bn/moving_variance": np.full(self.embed_dim, np.float32(1.0 - BN_EPS), np.float32)}, strict=False)

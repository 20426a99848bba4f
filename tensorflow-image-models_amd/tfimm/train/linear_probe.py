"""``LinearProbe``: a classifier head fitted on frozen features with softmax cross-entropy, on the device.

The part of the reference's ``tfimm/train`` (``ClassificationProblem`` + ``OptimizerFactory``) that needs no backward pass
through the backbone.  A step is three launches on the current stream and no host synchronisation:

1. ``tfimm_hip_gemm``          logits = f16 . W16^T + bias   (float32 out)
2. ``tfimm_hip_softmax_grad``  loss, pred and the bf16 rows p - onehot
3. ``tfimm_hip_head_update``   the weight gradient and the optimizer step on the float32 master weights, their bf16 shadow
                               rewritten for the next step's product

The contract of launches 2 and 3 is in include/tfimm_hip.h; tests/head_fit_ref.py restates it on the CPU.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from ..engine import ffi
from ..models.meter import _labels
from ..models.model import Tensor
from ._head_probe import OPTIMIZERS, _HeadProbe, _is_int, step_scalars  # noqa: F401

#: what ``LinearProbe.step`` and ``Model.fit_head`` return: two ``Tensor`` of shape (B,) -- the float32 cross-entropy of every
#: row BEFORE the step (0 for an ignored row) and the int32 predicted class
StepResult = namedtuple("StepResult", ["loss", "pred"])


def classifier_names(model):
    """(kernel name, bias name) of ``model``'s classifier among its weights; ``ValueError`` for a model without one or with
    several heads"""
    cls = getattr(model.cfg, "classifier", None)
    if int(model.cfg.nb_classes) == 0 or not cls:
        raise ValueError(f"{model.name}: the model has no classifier (nb_classes == 0)")
    if not isinstance(cls, str):
        raise ValueError(f"{model.name}: the logits hold {len(cls)} heads ({', '.join(cls)}); a probe fits one")
    for k in model._specs:
        if k == cls + "/kernel" or k.endswith("/" + cls + "/kernel"):
            return k, k[:-len("kernel")] + "bias"
    raise ValueError(f"{model.name}: no weight '{cls}/kernel'")


class LinearProbe(_HeadProbe):
    """``LinearProbe(dim, nb_classes, optimizer="sgd", lr=0.1, betas=(0.9, 0.999), epsilon=1e-7, weight_decay=0.0, seed=0)``
    -- names and defaults of the reference's ``OptimizerConfig``.  ``lr`` is a float or a callable ``step -> float`` (step
    counts from 0, as a Keras schedule's ``iterations``); ``betas[0]`` is the sgd momentum; ``weight_decay`` is the reference's
    ``reg_loss = weight_decay * sum(w^2)`` over kernel AND bias.  Gradient clipping is not offered.

    The kernel starts glorot-uniform from ``seed``, the bias at zero (Keras' Dense); ``for_model`` starts from a model's
    classifier.  Float32 master weights, optimizer slots and a bf16 shadow of the kernel live in device memory from the
    first call on; ``weights`` / ``state_dict`` copy them to the host."""

    _NAME, _COLS = "LinearProbe", "nb_classes"
    _COLS_MAX, _COLS_MAX_NAME = min(ffi.HEAD_MAX_C, ffi.SCORE_MAX_N), f"TFIMM_HEAD_MAX_C = {ffi.HEAD_MAX_C}"

    def __init__(self, dim, nb_classes, optimizer="sgd", lr=0.1, betas=(0.9, 0.999), epsilon=1e-7, weight_decay=0.0, seed=0):
        super().__init__(dim, nb_classes, optimizer, lr, betas, epsilon, weight_decay, seed)

    @classmethod
    def for_model(cls, model, **kw):
        """a probe of the model's feature width and class count that starts from its classifier's kernel and bias"""
        kn, bn = classifier_names(model)
        kernel = np.asarray(model.weights[kn], np.float32)
        probe = cls(int(kernel.shape[0]), int(kernel.shape[1]), **kw)
        probe._host = probe._zero_state(kernel.copy(), np.asarray(model.weights[bn], np.float32).copy())
        return probe

    # -- the public surface ----------------------------------------------------------------------------
    def __call__(self, features):
        """float32 logits (B, nb_classes) of ``features`` under the current weights: the product a step starts with"""
        B = self._forward(features)
        return Tensor(self._out[:B].clone())

    def step(self, features, labels) -> StepResult:
        """One optimizer step on a batch: ``features`` (B, dim) -- a ``tfimm.Tensor``, a torch tensor on either side or a
        numpy array, float32 or bf16, rounded once to bf16 -- and ``labels`` (B,) as ``Meter.update`` takes them (-1: the row
        is ignored).  Returns ``StepResult(loss, pred)`` of the batch under the weights BEFORE the step; nothing waits for
        the device."""
        import torch
        B, stage = self._features(features, "LinearProbe.step")
        up_labels = labels if callable(labels) else _labels(labels, B, "LinearProbe.step")
        stage()
        y = up_labels()
        loss = torch.empty(B, dtype=torch.float32, device="cuda")
        pred = torch.empty(B, dtype=torch.int32, device="cuda")
        if B == 0:
            return StepResult(Tensor(loss), Tensor(pred))
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self._gemm(B, st)
        ffi.check(ffi.lib.tfimm_hip_softmax_grad(self._out.data_ptr(), self.nb_classes, B, self.nb_classes, y.data_ptr(),
                                                 self._g.data_ptr(), self._ldg, loss.data_ptr(), pred.data_ptr(), st),
                  "tfimm_hip_softmax_grad")
        self._update(B, y, st)
        self._keep = y                                   # the launches read it asynchronously
        return StepResult(Tensor(loss), Tensor(pred))

    def install(self, model) -> None:
        """hand kernel and bias to ``model``'s classifier (``model.set_weights(..., strict=False)``: its programs, plans and
        recordings are rebuilt on the next call)"""
        kn, bn = classifier_names(model)
        shape = tuple(model._specs[kn].shape)
        if shape != (self.dim, self.nb_classes):
            raise ValueError(f"LinearProbe.install: the probe is ({self.dim}, nb_classes = {self.nb_classes}), the classifier "
                             f"of {model.name} is {shape}")
        w = self.weights
        model.set_weights({kn: w["kernel"], bn: w["bias"]}, strict=False)

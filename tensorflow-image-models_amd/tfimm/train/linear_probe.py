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

from ..engine import ffi, pack, tune
from ..models.meter import _labels
from ..models.model import Tensor

#: what ``LinearProbe.step`` and ``Model.fit_head`` return: two ``Tensor`` of shape (B,) -- the float32 cross-entropy of every
#: row BEFORE the step (0 for an ignored row) and the int32 predicted class
StepResult = namedtuple("StepResult", ["loss", "pred"])

OPTIMIZERS = {"sgd": ffi.HEAD_SGD, "adam": ffi.HEAD_ADAM}


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


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


def step_scalars(optimizer: str, lr: float, betas, epsilon: float, weight_decay: float, t: int):
    """The five float32 scalars of tfimm_head_update_desc for step ``t`` (1-based): ``(lr, mom_or_one_minus_b1,
    one_minus_b2, eps, wd2)``.  Everything is formed in float64 and rounded once.  adam: lr = alpha_t =
    lr * sqrt(1 - beta2^t) / (1 - beta1^t) (keras Adam); sgd: betas[0] is the momentum."""
    b1, b2 = float(betas[0]), float(betas[1])
    if optimizer == "adam":
        vals = (float(lr) * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t), 1.0 - b1, 1.0 - b2, float(epsilon), 2.0 * float(weight_decay))
    else:
        vals = (float(lr), b1, 0.0, float(epsilon), 2.0 * float(weight_decay))
    return tuple(np.float32(v) for v in vals)


class LinearProbe:
    """``LinearProbe(dim, nb_classes, optimizer="sgd", lr=0.1, betas=(0.9, 0.999), epsilon=1e-7, weight_decay=0.0, seed=0)``
    -- names and defaults of the reference's ``OptimizerConfig``.  ``lr`` is a float or a callable ``step -> float`` (step
    counts from 0, as a Keras schedule's ``iterations``); ``betas[0]`` is the sgd momentum; ``weight_decay`` is the reference's
    ``reg_loss = weight_decay * sum(w^2)`` over kernel AND bias.  Gradient clipping is not offered.

    The kernel starts glorot-uniform from ``seed``, the bias at zero (Keras' Dense); ``for_model`` starts from a model's
    classifier.  Float32 master weights, optimizer slots and a bf16 shadow of the kernel live in device memory from the
    first call on; ``weights`` / ``state_dict`` copy them to the host."""

    def __init__(self, dim, nb_classes, optimizer="sgd", lr=0.1, betas=(0.9, 0.999), epsilon=1e-7, weight_decay=0.0, seed=0):
        if not _is_int(dim) or dim % 8 != 0 or not 8 <= dim <= ffi.HEAD_MAX_D:
            raise ValueError(f"LinearProbe: dim = {dim!r}, must be a multiple of 8 in [8, TFIMM_HEAD_MAX_D = {ffi.HEAD_MAX_D}]")
        if not _is_int(nb_classes) or not 1 <= nb_classes <= min(ffi.HEAD_MAX_C, ffi.SCORE_MAX_N):
            raise ValueError(f"LinearProbe: nb_classes = {nb_classes!r}, must be an integer in [1, TFIMM_HEAD_MAX_C = "
                             f"{ffi.HEAD_MAX_C}]")
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"LinearProbe: unknown optimizer {optimizer!r}, must be one of {sorted(OPTIMIZERS)}")
        if not callable(lr) and (isinstance(lr, bool) or not isinstance(lr, (int, float, np.floating, np.integer))):
            raise ValueError(f"LinearProbe: lr = {lr!r}, must be a float or a callable step -> float")
        if len(tuple(betas)) != 2:
            raise ValueError(f"LinearProbe: betas = {betas!r}, must be two numbers")
        self.dim, self.nb_classes = int(dim), int(nb_classes)
        self.optimizer, self.lr = optimizer, lr
        self.betas, self.epsilon, self.weight_decay = (float(betas[0]), float(betas[1])), float(epsilon), float(weight_decay)
        self.step_count = 0
        lim = np.sqrt(6.0 / (self.dim + self.nb_classes))
        kernel = np.random.default_rng(seed).uniform(-lim, lim, size=(self.dim, self.nb_classes)).astype(np.float32)
        # the state on the host until the first device call (and again after load_state_dict / set_weights)
        self._host = self._zero_state(kernel, np.zeros(self.nb_classes, np.float32))
        self._dev = None
        self._ldw = pack.ceil_to(self.dim, 64)            # the pitch pack_matrix gives a Dense layer's weights
        self._ldg = pack.ceil_to(self.nb_classes, 8)
        self._cap = 0                                     # rows the per-batch buffers hold
        self._keep = None

    @classmethod
    def for_model(cls, model, **kw):
        """a probe of the model's feature width and class count that starts from its classifier's kernel and bias"""
        kn, bn = classifier_names(model)
        kernel = np.asarray(model.weights[kn], np.float32)
        probe = cls(int(kernel.shape[0]), int(kernel.shape[1]), **kw)
        probe._host = probe._zero_state(kernel.copy(), np.asarray(model.weights[bn], np.float32).copy())
        return probe

    def _zero_state(self, kernel, bias):
        z = lambda a: np.zeros_like(a)                    # noqa: E731
        return {"kernel": kernel, "bias": bias, "s1": z(kernel), "s2": z(kernel), "bias_s1": z(bias), "bias_s2": z(bias)}

    # -- device state ------------------------------------------------------------------------------
    def _device(self):
        import torch
        if self._dev is None:
            if not torch.cuda.is_available():
                raise RuntimeError("tfimm (MI355X engine) needs a ROCm GPU: no CPU execution path exists.")
            h, d = self._host, {}
            C_, D, ld = self.nb_classes, self.dim, self._ldw
            for name in ("kernel", "s1", "s2"):
                m = np.zeros((C_, ld), np.float32)
                m[:, :D] = h[name].T
                d[name] = torch.from_numpy(m).to("cuda")
            for name in ("bias", "bias_s1", "bias_s2"):
                d[name] = torch.from_numpy(np.ascontiguousarray(h[name], dtype=np.float32)).to("cuda")
            d["w16"] = torch.from_numpy(pack.pack_matrix(np.ascontiguousarray(h["kernel"].T)).view(np.int16)).to("cuda")
            self._dev, self._host = d, None
        return self._dev

    def _to_host(self):
        """the six arrays in the Keras layout (one synchronising copy each)"""
        if self._dev is None:
            return {k: v.copy() for k, v in self._host.items()}
        d, D = self._dev, self.dim
        out = {k: np.ascontiguousarray(d[k].cpu().numpy()[:, :D].T) for k in ("kernel", "s1", "s2")}
        out.update({k: d[k].cpu().numpy().copy() for k in ("bias", "bias_s1", "bias_s2")})
        return out

    def _buffers(self, B):
        import torch
        if B > self._cap:
            self._f16 = torch.zeros((B, self.dim), dtype=torch.bfloat16, device="cuda")
            self._logits = torch.zeros((B, self.nb_classes), dtype=torch.float32, device="cuda")
            self._g = torch.zeros((B, self._ldg), dtype=torch.bfloat16, device="cuda")
            self._cap = B

    # -- inputs --------------------------------------------------------------------------------------
    def _features(self, x, what):
        """``x`` checked on the host; returns (B, callable that rounds it into the probe's bf16 buffer)"""
        import torch
        t = x.torch() if isinstance(x, Tensor) else x if isinstance(x, torch.Tensor) else np.asarray(x)
        dt = str(t.dtype).replace("torch.", "")
        if dt not in ("float32", "bfloat16"):
            raise ValueError(f"{what}: features: expected float32 or bfloat16, got {t.dtype}")
        if t.ndim != 2 or t.shape[1] != self.dim:
            raise ValueError(f"{what}: features: expected shape (B, {self.dim}), got {tuple(t.shape)}")
        B = int(t.shape[0])
        if B > ffi.HEAD_MAX_B:
            raise ValueError(f"{what}: a batch of {B} rows, more than TFIMM_HEAD_MAX_B = {ffi.HEAD_MAX_B}")

        def stage():
            src = t
            if isinstance(src, np.ndarray):
                src = torch.from_numpy(np.ascontiguousarray(src.view(np.int16) if dt == "bfloat16" else src))
                if dt == "bfloat16":
                    src = src.view(torch.bfloat16)
            self._device()
            self._buffers(max(B, 1))
            self._f16[:B].copy_(src, non_blocking=True)          # float32 -> bf16: round to nearest even, once
        return B, stage

    def _gemm(self, B, st):
        d = ffi.GemmDesc()
        dev = self._dev
        d.a, d.wt, d.bias, d.out = self._f16.data_ptr(), dev["w16"].data_ptr(), dev["bias"].data_ptr(), self._logits.data_ptr()
        d.M, d.N, d.K = B, self.nb_classes, self.dim
        d.lda, d.ldw, d.ldc = self.dim, self._ldw, self.nb_classes
        d.out_f32, d.rows_per_image = 1, 1
        d.tile_hint = tune.lookup(d)
        ffi.check(ffi.lib.tfimm_hip_gemm(C.byref(d), st), "tfimm_hip_gemm")

    # -- the public surface ----------------------------------------------------------------------------
    def __call__(self, features):
        """float32 logits (B, nb_classes) of ``features`` under the current weights: the product a step starts with"""
        import torch
        B, stage = self._features(features, "LinearProbe")
        stage()
        if B:
            self._gemm(B, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return Tensor(self._logits[:B].clone())

    def _lr_now(self) -> float:
        return float(self.lr(self.step_count)) if callable(self.lr) else float(self.lr)

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
        lr, m1, m2, eps, wd2 = step_scalars(self.optimizer, self._lr_now(), self.betas, self.epsilon, self.weight_decay,
                                            self.step_count + 1)
        self._gemm(B, st)
        ffi.check(ffi.lib.tfimm_hip_softmax_grad(self._logits.data_ptr(), self.nb_classes, B, self.nb_classes, y.data_ptr(),
                                                 self._g.data_ptr(), self._ldg, loss.data_ptr(), pred.data_ptr(), st),
                  "tfimm_hip_softmax_grad")
        dev, d = self._dev, ffi.HeadUpdateDesc()
        d.f, d.g, d.labels = self._f16.data_ptr(), self._g.data_ptr(), y.data_ptr()
        d.w, d.w16, d.s1, d.s2 = dev["kernel"].data_ptr(), dev["w16"].data_ptr(), dev["s1"].data_ptr(), dev["s2"].data_ptr()
        d.bias, d.bias_s1, d.bias_s2 = dev["bias"].data_ptr(), dev["bias_s1"].data_ptr(), dev["bias_s2"].data_ptr()
        d.B, d.D, d.C = B, self.dim, self.nb_classes
        d.ldf, d.ldg, d.ldw, d.ldw16 = self.dim, self._ldg, self._ldw, self._ldw
        d.opt = OPTIMIZERS[self.optimizer]
        d.lr, d.mom_or_one_minus_b1, d.one_minus_b2, d.eps, d.wd2 = lr, m1, m2, eps, wd2
        ffi.check(ffi.lib.tfimm_hip_head_update(C.byref(d), st), "tfimm_hip_head_update")
        self._keep = y                                   # the launches read it asynchronously
        self.step_count += 1
        return StepResult(Tensor(loss), Tensor(pred))

    @property
    def weights(self):
        """``{"kernel": (dim, nb_classes), "bias": (nb_classes,)}`` float32, the Keras Dense layout"""
        h = self._to_host()
        return {"kernel": h["kernel"], "bias": h["bias"]}

    def set_weights(self, new) -> None:
        """replace kernel and bias (the optimizer slots and the step count stay)"""
        h = self._to_host()
        h.update(self._checked(new, ("kernel", "bias"), "set_weights"))
        self._host, self._dev = h, None

    def _checked(self, new, names, what):
        shapes = {"kernel": (self.dim, self.nb_classes), "bias": (self.nb_classes,)}
        out = {}
        for k in names:
            if k not in new:
                raise ValueError(f"LinearProbe.{what}: '{k}' is missing")
            v = np.array(new[k], dtype=np.float32)
            want = shapes["kernel" if k in ("kernel", "s1", "s2") else "bias"]
            if v.shape != want:
                raise ValueError(f"LinearProbe.{what}: '{k}' has shape {v.shape}, expected {want}")
            out[k] = v
        return out

    def state_dict(self):
        """weights, optimizer slots and the step count as numpy arrays: ``load_state_dict`` of it continues bit for bit"""
        out = self._to_host()
        out["step"] = np.int64(self.step_count)
        out["optimizer"] = self.optimizer
        return out

    def load_state_dict(self, state) -> None:
        if str(state.get("optimizer", self.optimizer)) != self.optimizer:
            raise ValueError(f"LinearProbe.load_state_dict: the state is of optimizer {state['optimizer']!r}, this probe runs "
                             f"{self.optimizer!r}")
        h = self._checked(state, ("kernel", "bias", "s1", "s2", "bias_s1", "bias_s2"), "load_state_dict")
        self._host, self._dev = h, None
        self.step_count = int(state["step"])

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

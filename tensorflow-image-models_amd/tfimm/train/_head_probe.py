"""What ``LinearProbe`` and ``EmbeddingProbe`` share: ONE Dense layer (dim, columns) with bias trained on frozen features on
the device -- float32 master weights, optimizer slots and the bf16 shadow in device memory, the staging of a batch of
features, the descriptors of the first launch of a step (``tfimm_hip_gemm``, float32 out) and of its last
(``tfimm_hip_head_update``), and the state dict.  The launch between the two -- the loss and its gradient rows -- is the
subclass's."""
import ctypes as C

import numpy as np

from ..engine import ffi, pack, tune
from ..models.model import Tensor

OPTIMIZERS = {"sgd": ffi.HEAD_SGD, "adam": ffi.HEAD_ADAM}


def _is_int(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


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


class _HeadProbe:
    """The subclass names itself (``_NAME``), its column count (``_COLS``: the attribute of that name is set here) and the
    limit on it (``_COLS_MAX``, ``_COLS_MAX_NAME``) for the messages."""

    _NAME = _COLS = _COLS_MAX_NAME = ""
    _COLS_MAX = 0

    def __init__(self, dim, cols, optimizer, lr, betas, epsilon, weight_decay, seed):
        me = self._NAME
        if not _is_int(dim) or dim % 8 != 0 or not 8 <= dim <= ffi.HEAD_MAX_D:
            raise ValueError(f"{me}: dim = {dim!r}, must be a multiple of 8 in [8, TFIMM_HEAD_MAX_D = {ffi.HEAD_MAX_D}]")
        if not _is_int(cols) or not 1 <= cols <= self._COLS_MAX:
            raise ValueError(f"{me}: {self._COLS} = {cols!r}, must be an integer in [1, {self._COLS_MAX_NAME}]")
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"{me}: unknown optimizer {optimizer!r}, must be one of {sorted(OPTIMIZERS)}")
        if not callable(lr) and (isinstance(lr, bool) or not isinstance(lr, (int, float, np.floating, np.integer))):
            raise ValueError(f"{me}: lr = {lr!r}, must be a float or a callable step -> float")
        if len(tuple(betas)) != 2:
            raise ValueError(f"{me}: betas = {betas!r}, must be two numbers")
        self.dim, self._n = int(dim), int(cols)
        setattr(self, self._COLS, self._n)
        self.optimizer, self.lr = optimizer, lr
        self.betas, self.epsilon, self.weight_decay = (float(betas[0]), float(betas[1])), float(epsilon), float(weight_decay)
        self.step_count = 0
        lim = np.sqrt(6.0 / (self.dim + self._n))
        kernel = np.random.default_rng(seed).uniform(-lim, lim, size=(self.dim, self._n)).astype(np.float32)
        # the state on the host until the first device call (and again after load_state_dict / set_weights)
        self._host = self._zero_state(kernel, np.zeros(self._n, np.float32))
        self._dev = None
        self._ldw = pack.ceil_to(self.dim, 64)            # the pitch pack_matrix gives a Dense layer's weights
        self._ldg = pack.ceil_to(self._n, 8)
        self._cap = 0                                     # rows the per-batch buffers hold
        self._keep = None

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
            C_, D, ld = self._n, self.dim, self._ldw
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
            self._out = torch.zeros((B, self._n), dtype=torch.float32, device="cuda")     # the product a step starts with
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

    # -- the launches both probes make ---------------------------------------------------------------
    def _gemm(self, B, st):
        d = ffi.GemmDesc()
        dev = self._dev
        d.a, d.wt, d.bias, d.out = self._f16.data_ptr(), dev["w16"].data_ptr(), dev["bias"].data_ptr(), self._out.data_ptr()
        d.M, d.N, d.K = B, self._n, self.dim
        d.lda, d.ldw, d.ldc = self.dim, self._ldw, self._n
        d.out_f32, d.rows_per_image = 1, 1
        d.tile_hint = tune.lookup(d)
        ffi.check(ffi.lib.tfimm_hip_gemm(C.byref(d), st), "tfimm_hip_gemm")

    def _forward(self, features):
        """the product of ``features`` and the current weights in ``self._out[:B]``; returns B"""
        import torch
        B, stage = self._features(features, self._NAME)
        stage()
        if B:
            self._gemm(B, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return B

    def _lr_now(self) -> float:
        return float(self.lr(self.step_count)) if callable(self.lr) else float(self.lr)

    def _decay(self) -> float:
        """the factor of sum(w^2) in the loss: half of what tfimm_hip_head_update's wd2 multiplies w by"""
        return self.weight_decay

    def _update(self, B, y, st):
        """tfimm_hip_head_update on the staged features and the gradient rows in ``self._g``; ``y`` (B,) int32 on the device
        is what it counts n from"""
        lr, m1, m2, eps, wd2 = step_scalars(self.optimizer, self._lr_now(), self.betas, self.epsilon, self._decay(),
                                            self.step_count + 1)
        dev, d = self._dev, ffi.HeadUpdateDesc()
        d.f, d.g, d.labels = self._f16.data_ptr(), self._g.data_ptr(), y.data_ptr()
        d.w, d.w16, d.s1, d.s2 = dev["kernel"].data_ptr(), dev["w16"].data_ptr(), dev["s1"].data_ptr(), dev["s2"].data_ptr()
        d.bias, d.bias_s1, d.bias_s2 = dev["bias"].data_ptr(), dev["bias_s1"].data_ptr(), dev["bias_s2"].data_ptr()
        d.B, d.D, d.C = B, self.dim, self._n
        d.ldf, d.ldg, d.ldw, d.ldw16 = self.dim, self._ldg, self._ldw, self._ldw
        d.opt = OPTIMIZERS[self.optimizer]
        d.lr, d.mom_or_one_minus_b1, d.one_minus_b2, d.eps, d.wd2 = lr, m1, m2, eps, wd2
        ffi.check(ffi.lib.tfimm_hip_head_update(C.byref(d), st), "tfimm_hip_head_update")
        self.step_count += 1

    # -- weights and state -----------------------------------------------------------------------------
    @property
    def weights(self):
        """``{"kernel": (dim, columns), "bias": (columns,)}`` float32, the Keras Dense layout"""
        h = self._to_host()
        return {"kernel": h["kernel"], "bias": h["bias"]}

    def set_weights(self, new) -> None:
        """replace kernel and bias (the optimizer slots and the step count stay)"""
        h = self._to_host()
        h.update(self._checked(new, ("kernel", "bias"), "set_weights"))
        self._host, self._dev = h, None

    def _checked(self, new, names, what):
        shapes = {"kernel": (self.dim, self._n), "bias": (self._n,)}
        out = {}
        for k in names:
            if k not in new:
                raise ValueError(f"{self._NAME}.{what}: '{k}' is missing")
            v = np.array(new[k], dtype=np.float32)
            want = shapes["kernel" if k in ("kernel", "s1", "s2") else "bias"]
            if v.shape != want:
                raise ValueError(f"{self._NAME}.{what}: '{k}' has shape {v.shape}, expected {want}")
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
            raise ValueError(f"{self._NAME}.load_state_dict: the state is of optimizer {state['optimizer']!r}, this probe runs "
                             f"{self.optimizer!r}")
        h = self._checked(state, ("kernel", "bias", "s1", "s2", "bias_s1", "bias_s2"), "load_state_dict")
        self._host, self._dev = h, None
        self.step_count = int(state["step"])

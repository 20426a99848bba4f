"""LoRA ConvNeXt on the MI355X engine (reference tfimm/architectures/lora/convnext.py).

The two Dense layers of every block's MLP carry a low-rank update ``scaling * A @ B`` next to their kernel
(``LoRADense``, lora/layers.py:81-113: ``x W + scaling * (x A) B + bias``, then the activation).  Two lowerings:

* merged (after ``merge_lora_weights``): exactly ``ConvNeXt.lower`` over kernels ``W + scaling * A @ B`` -- the base program.
* unmerged: the update is an op of its own (tfimm_hip_lora_delta) whose result is the residual operand of the layer's GEMM:

      y  = dwconv(x)
      n  = layernorm(y)                                        (written out: the LayerNorm fold takes no residual)
      d1 = lora_delta(n, fc1 A, fc1 B)
      h  = dense(n, fc1, act, residual=d1, act_after_res)      act(n W1 + b1 + d1)
      r2 = lora_delta(h, fc2 A, fc2 B * gamma, residual=x)
      x  = dense(h, fc2 * gamma, residual=r2)

  The base kernels' packed constants do not depend on the adapter, so ``set_lora_weights`` swaps an adapter by rewriting the
  A / B constants in place, under the plans and recordings that point at them.
"""
import zlib
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict

import numpy as np

from ...engine import pack
from ..convnext import ConvNeXt, ConvNeXtConfig
from .factory import lora_non_trainable_weights, lora_trainable_weights
from .layers import LORA_MAX_RANK, LORA_MIN_RANK, convert_to_lora_layer, is_lora_weight, merge_kernel
from .registry import register_lora_architecture

__all__ = ["LoRAConvNeXt", "LoRAConvNeXtConfig"]


@dataclass
class LoRAConvNeXtConfig(ConvNeXtConfig):
    lora_rank: int = 4
    lora_alpha: float = 1.0
    lora_train_bias: str = "none"
    lora_train_classifer: bool = True       # (the reference's spelling)


@register_lora_architecture
class LoRAConvNeXt(ConvNeXt):
    cfg_class = LoRAConvNeXtConfig

    def __init__(self, cfg: LoRAConvNeXtConfig, *args, **kwargs):
        r = cfg.lora_rank
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not LORA_MIN_RANK <= r <= LORA_MAX_RANK:
            raise ValueError(f"lora_rank = {r!r}: tfimm_hip_lora_delta takes integer ranks {LORA_MIN_RANK}..{LORA_MAX_RANK}")
        #: the kernels the programs are built from are W + scaling * A @ B (merge_lora_weights / unmerge_lora_weights)
        self.merged = False
        super().__init__(cfg, *args, **kwargs)

    @property
    def scaling(self) -> float:
        return self.cfg.lora_alpha / self.cfg.lora_rank

    # -- variables ---------------------------------------------------------------------------
    def weight_specs(self):
        base = super().weight_specs()
        lora_layers = [k[:-len("kernel")] for k in base if k.endswith(("/mlp/fc1/kernel", "/mlp/fc2/kernel"))]
        converted = {p: convert_to_lora_layer(p, base, self.cfg.lora_rank) for p in lora_layers}
        s, done = OrderedDict(), set()
        for k, v in base.items():
            p = k.rsplit("/", 1)[0] + "/"
            if p not in converted:
                s[k] = v
            elif p not in done:         # the layer's own variables, then kernel_lora_a and kernel_lora_b (LoRADense.build)
                s.update(converted[p])
                done.add(p)
        return s

    def lora_layers(self):
        """Prefixes of the layers that carry a low-rank update, in model order"""
        return [k[:-len("kernel_lora_a")] for k in self._specs if k.endswith("/kernel_lora_a")]

    def merged_weights(self) -> Dict[str, np.ndarray]:
        """``model.weights`` with every LoRA layer's kernel replaced by ``W + scaling * A @ B`` (float32)"""
        w = OrderedDict(self._weights)
        for p in self.lora_layers():
            w[p + "kernel"] = merge_kernel(w[p + "kernel"], w[p + "kernel_lora_a"], w[p + "kernel_lora_b"], self.scaling)
        return w

    @property
    def trainable_weights(self):
        classifier = [self.cfg.classifier] if self.cfg.lora_train_classifer else []
        return lora_trainable_weights(self, train_bias=self.cfg.lora_train_bias, trainable_layers=classifier)

    @property
    def non_trainable_weights(self):
        classifier = [self.cfg.classifier] if self.cfg.lora_train_classifer else []
        return lora_non_trainable_weights(self, train_bias=self.cfg.lora_train_bias, trainable_layers=classifier)

    # -- merge state --------------------------------------------------------------------------
    def _drop_programs(self):
        self._programs.clear()
        self._const_cache.clear()
        self._plans.clear()
        self._captured.clear()
        self._plan_uses.clear()

    def _set_merged(self, merged: bool):
        self.merged = bool(merged)
        self._drop_programs()

    # -- lowering -----------------------------------------------------------------------------
    def lower(self, b, H, W, want_features):
        if self.merged:
            b.w = b._orig_w = self.merged_weights()
        super().lower(b, H, W, want_features)

    def lower_block(self, b, x, p: str, eps: float):
        if self.merged:
            return super().lower_block(b, x, p, eps)
        c = self.cfg
        y, _ = b.dwconv(x, p + "conv_dw/depthwise_kernel", stride=1, padding=3, bias=p + "conv_dw/bias",
                        cite="convnext.py:224-225")
        n = b.layernorm(y, p + "norm", eps, cite="convnext.py:226")
        d1 = b.lora_delta(n, p + "mlp/fc1/kernel_lora_a", p + "mlp/fc1/kernel_lora_b", scaling=self.scaling,
                          cite="lora/layers.py:93-94, 100")
        # (mx=False: under TFIMM_PRECISION=fp8 the layers that carry an adapter stay bf16)
        h = b.dense(n, p + "mlp/fc1/kernel", p + "mlp/fc1/bias", act=c.act_layer, residual=d1, act_after_res=True, mx=False,
                    cite="lora/layers.py:92, 100-111")
        r2 = b.lora_delta(h, p + "mlp/fc2/kernel_lora_a", p + "mlp/fc2/kernel_lora_b", scaling=self.scaling,
                          out_scale=p + "gamma", residual=x, cite="lora/layers.py:93-94, 100 + convnext.py:228-230")
        return b.dense(h, p + "mlp/fc2/kernel", p + "mlp/fc2/bias", out_scale=p + "gamma", residual=r2, mx=False,
                       cite="lora/layers.py:92, 100-108 + convnext.py:228-230")

    # -- adapter swap -------------------------------------------------------------------------
    def set_lora_weights(self, new: Dict[str, np.ndarray]):
        """Replace LoRA variables (``.../kernel_lora_a``, ``.../kernel_lora_b``) by name; any other name is a ``KeyError``, a
        wrong shape a ``ValueError``, both before anything is committed.  Unmerged, the packed constants of the affected
        ``lora_delta`` ops are rewritten where they are -- on the device by a copy on the current stream into the buffers the
        plans and recordings already point at -- and no program, plan or recording is dropped.  Merged, every kernel
        changes: the call is ``set_weights(new, strict=False)``."""
        staged: Dict[str, np.ndarray] = {}
        for k, v in new.items():
            if k.startswith(self.name + "/"):
                k = k[len(self.name) + 1:]
            if k.endswith(":0"):
                k = k[:-2]
            if k not in self._specs or not is_lora_weight(k):
                raise KeyError(f"{self.name}: set_lora_weights takes kernel_lora_a / kernel_lora_b variables only, got '{k}'")
            v = np.asarray(v, dtype=np.float32)
            if tuple(v.shape) != tuple(self._specs[k].shape):
                raise ValueError(f"{self.name}: weight '{k}' has shape {v.shape}, expected {self._specs[k].shape}")
            staged[k] = v
        if self.merged:
            self.set_weights(staged, strict=False)
            return
        self._weights.update(staged)
        for prog in self._programs.values():
            for op in prog.ops:
                if op.kind != "lora_delta" or not (op.attrs["a_name"] in staged or op.attrs["b_name"] in staged):
                    continue
                a = op.attrs
                scale = None if a["out_scale"] is None else self._weights[a["out_scale"]]
                at, bt = pack.pack_lora(self._weights[a["a_name"]], self._weights[a["b_name"]], a["scaling"], scale,
                                        fp32=prog.precision == "fp32")
                _rewrite_const(prog, op.consts["a"], at)
                _rewrite_const(prog, op.consts["b"], bt)


def _rewrite_const(prog, cid: int, host: np.ndarray):
    """New contents for the constant ``cid`` of ``prog``, same shape and type: into its device tensor if it has been uploaded
    (torch copy on the current stream: ordered behind the launches already queued and in front of the next replay), else
    into its host copy.  The key follows the contents, so a program built later shares or uploads the right values."""
    import torch
    c = prog.consts[cid]
    host = np.ascontiguousarray(host)
    assert c.key[1] == host.shape and c.key[2] == host.dtype.str, (c.key, host.shape, host.dtype)
    key = (c.name, host.shape, host.dtype.str, zlib.crc32(host.view(np.uint8).reshape(-1)))
    if prog._dev_consts is not None:
        t = prog._dev_consts[cid]
        t.copy_(torch.from_numpy(host.view(np.int16) if host.dtype == np.uint16 else host))
        cache, dev = prog.const_cache, prog._dev_consts_device
        if cache is not None:
            if cache.get((dev,) + c.key) is t:
                del cache[(dev,) + c.key]
            cache[(dev,) + key] = t
        if c.host is not None:
            c.host = host
    else:
        c.host = host
    c.key = key

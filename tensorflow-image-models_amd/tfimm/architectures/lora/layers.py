"""The LoRA Dense layer as this engine sees it: two more variables per layer and a rule for merging them
(reference tfimm/architectures/lora/layers.py, LoRADense).

The engine has no layer objects; a layer is a name prefix in ``Model.weight_specs()``.  ``convert_to_lora_layer`` therefore
maps the SPECS of a Dense layer to those of its LoRA version, and ``merge_kernel`` is ``LoRADense.merge_weights`` on arrays.
The unmerged forward (``LoRADense.call``) is lowered by the model (lora/convnext.py) onto tfimm_hip_lora_delta.
"""
from collections import OrderedDict

import numpy as np

from ...models.model import WeightSpec

LORA_WEIGHT_NAMES = ["kernel_lora_a", "kernel_lora_b"]
"""Patterns that match the LoRA variables, to keep them out of weight transfers between a model and its LoRA version."""

#: ranks tfimm_hip_lora_delta takes (the rank is padded to 16, 32, 48 or 64 on the device)
LORA_MIN_RANK, LORA_MAX_RANK = 1, 64


def is_lora_weight(name: str) -> bool:
    return name.rsplit("/", 1)[-1] in LORA_WEIGHT_NAMES


def convert_to_lora_layer(prefix: str, specs, lora_rank: int = 4) -> "OrderedDict[str, WeightSpec]":
    """The variables of the Dense layer ``prefix`` (``prefix + "kernel"`` [, ``prefix + "bias"``] in ``specs``) followed by the
    two that ``LoRADense.build`` adds: ``kernel_lora_a`` (in, r), glorot-uniform, and ``kernel_lora_b`` (r, out), zeros.
    Only Dense layers convert: anything else (the 1x1 convolutions of a ConvMLP) is a ``ValueError`` (layers.py:280-286)."""
    kernel = specs[prefix + "kernel"]
    if kernel.kind != "dense" or len(kernel.shape) != 2:
        raise ValueError(f"Unsupported layer type for conversion to LoRA: {prefix.rstrip('/')} is a {kernel.kind} layer with "
                         f"kernel shape {tuple(kernel.shape)}.")
    kin, kout = kernel.shape
    out = OrderedDict((k, v) for k, v in specs.items() if k.startswith(prefix) and "/" not in k[len(prefix):])
    out[prefix + "kernel_lora_a"] = WeightSpec((kin, lora_rank), "dense")
    out[prefix + "kernel_lora_b"] = WeightSpec((lora_rank, kout), "dense", init="zeros")
    return out


def merge_kernel(kernel, lora_a, lora_b, scaling: float) -> np.ndarray:
    """``kernel + scaling * (A @ B)`` in float32 (``LoRADense.merge_weights``, layers.py:120-127)."""
    a, b = np.asarray(lora_a, dtype=np.float32), np.asarray(lora_b, dtype=np.float32)
    return (np.asarray(kernel, dtype=np.float32) + np.float32(scaling) * (a @ b)).astype(np.float32)

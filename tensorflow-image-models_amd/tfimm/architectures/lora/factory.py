"""Creating, converting and merging LoRA models (surface of reference tfimm/architectures/lora/factory.py).

The engine has no ``tf.Variable``: wherever the reference returns variables, these functions return weight NAMES (keys of
``model.weights``), in the reference's order.
"""
import dataclasses
from typing import List, Optional

from ...models import create_model as create_full_model
from ...models import model_class, transfer_weights
from ...models.factory import _layer_name
from .layers import LORA_WEIGHT_NAMES, is_lora_weight
from .registry import lora_architecture, lora_base_architecture, lora_config


def create_model(model_name: str, pretrained: bool = False, model_path: str = "", **kwargs):
    """The LoRA version of the registered model ``model_name``.  Arguments starting with ``lora_`` go into the LoRA config, all
    others to ``tfimm.create_model``; the base weights are carried over, A and B keep their initial values."""
    cls = model_class(model_name)
    lora_cls, lora_cfg_cls = lora_architecture(cls), lora_config(cls)
    lora_kwargs = {k: v for k, v in kwargs.items() if k.startswith("lora_")}
    full_kwargs = {k: v for k, v in kwargs.items() if not k.startswith("lora_")}
    full_model = create_full_model(model_name, pretrained=pretrained, model_path=model_path, **full_kwargs)
    model = lora_cls(lora_cfg_cls(**dataclasses.asdict(full_model.cfg), **lora_kwargs))
    transfer_weights(src_model=full_model, dst_model=model, weights_to_ignore=LORA_WEIGHT_NAMES)
    return model


def convert_to_lora_model(model, **kwargs):
    """The LoRA version of ``model`` (an instance of a class with a registered LoRA architecture); ``kwargs`` update the
    config (``lora_rank``, ``lora_alpha``, ...)."""
    lora_cls, lora_cfg_cls = lora_architecture(type(model)), lora_config(type(model))
    cfg = dataclasses.asdict(model.cfg)
    cfg.update(kwargs)
    lora_model = lora_cls(lora_cfg_cls(**cfg))
    transfer_weights(src_model=model, dst_model=lora_model, weights_to_ignore=LORA_WEIGHT_NAMES)
    return lora_model


def convert_to_regular_model(model):
    """A model of the base class whose kernels are ``W + scaling * A @ B``; ``model`` keeps its merge state."""
    base_cls = lora_base_architecture(type(model))
    cfg = {k: v for k, v in dataclasses.asdict(model.cfg).items() if not k.startswith("lora_")}
    base_model = base_cls(base_cls.cfg_class(**cfg))
    base_model.set_weights({k: v for k, v in model.merged_weights().items() if not is_lora_weight(k)})
    return base_model


def merge_lora_weights(model):
    """Fold every LoRA update of ``model`` into its layer's kernel, in place: from here on the model runs the base model's
    program.  Does nothing on a model that is merged already."""
    if not model.merged:
        model._set_merged(True)


def unmerge_lora_weights(model):
    """Back to separate low-rank updates (``LoRADense.unmerge_weights`` for every layer of ``model``)."""
    if not model.merged:
        raise ValueError("LoRA updates have not been merged yet.")
    model._set_merged(False)


def lora_trainable_weights(model, train_bias: str = "none", trainable_layers: Optional[List[str]] = None) -> List[str]:
    """Names of the weights that LoRA training updates, to use instead of ``model.trainable_weights``.

    Order as the reference builds it: layers in model order -- a LoRA layer gives A, B and, unless ``train_bias == "none"``,
    its bias; with ``train_bias == "all"`` every other layer gives its bias (``beta`` for a normalisation) -- followed by all
    weights of ``trainable_layers`` in ``model.weights`` order.  As in the reference, the second part does not look at the
    first: with ``train_bias == "all"`` the bias of a layer in ``trainable_layers`` is listed twice."""
    if train_bias not in {"none", "all", "lora_only"}:
        raise ValueError(f"Unknown value for train_bias: {train_bias}.")
    names = list(model.weights)
    lora_layers = {_layer_name(n) for n in names if is_lora_weight(n)}
    out, seen = [], set()
    for n in names:
        layer = _layer_name(n)
        if layer in seen:
            continue
        seen.add(layer)
        if layer in lora_layers:
            out += [f"{layer}/{w}" for w in LORA_WEIGHT_NAMES]
            if train_bias != "none" and f"{layer}/bias" in model.weights:
                out.append(f"{layer}/bias")
        elif train_bias == "all":
            out += [f"{layer}/{w}" for w in ("bias", "beta") if f"{layer}/{w}" in model.weights]
    trainable_layers = trainable_layers or []
    out += [n for n in names if _layer_name(n) in trainable_layers]
    return out


def lora_non_trainable_weights(model, train_bias: str = "none", trainable_layers: Optional[List[str]] = None) -> List[str]:
    """All weight names of ``model`` that ``lora_trainable_weights`` does not list, in ``model.weights`` order."""
    trainable = set(lora_trainable_weights(model, train_bias=train_bias, trainable_layers=trainable_layers))
    return [n for n in model.weights if n not in trainable]

"""Registry of LoRA architectures (surface of reference tfimm/architectures/lora/registry.py).

Keyed by model CLASS: ``ConvNeXt -> (LoRAConvNeXt, LoRAConvNeXtConfig)``.  It is separate from the model registry of
``tfimm.models.registry`` (keyed by model name) and does not add to ``list_models()``.
"""
import warnings

_lora_of_base = {}      # base class -> LoRA class
_base_of_lora = {}      # LoRA class -> base class
_config_of_base = {}    # base class -> config class of the LoRA class


def register_lora_architecture(lora_cls=None, *, base_cls=None):
    """Register ``lora_cls`` as the LoRA variant of ``base_cls``.  Three call forms:

    * ``@register_lora_architecture`` on a subclass of the base model: the base is ``lora_cls.__base__``;
    * ``@register_lora_architecture(base_cls=Base)`` on a class that does not derive from the base;
    * ``register_lora_architecture(Cls, base_cls=Cls)`` after the definition, for a class that is its own LoRA variant.

    ``lora_cls`` must have a ``cfg_class`` attribute.  Registering a second variant for a base warns and overwrites."""
    if lora_cls is None:
        def decorator(cls):
            return register_lora_architecture(cls, base_cls=base_cls)
        return decorator
    base = lora_cls.__base__ if base_cls is None else base_cls
    if base in _lora_of_base:
        warnings.warn(f"Model class {base} has already registered a LoRA version {_lora_of_base[base]}. "
                      f"Registering {lora_cls} will overwrite this.")
    _lora_of_base[base] = lora_cls
    _base_of_lora[lora_cls] = base
    _config_of_base[base] = lora_cls.cfg_class
    return lora_cls


def lora_architecture(model_cls):
    """The LoRA class registered for the base model class ``model_cls``."""
    if model_cls not in _lora_of_base:
        raise ValueError(f"No LoRA variant has been registered for architecture {model_cls}.")
    return _lora_of_base[model_cls]


def lora_base_architecture(lora_cls):
    """The base model class that ``lora_cls`` is registered as the LoRA variant of."""
    if lora_cls not in _base_of_lora:
        raise ValueError(f"The class {lora_cls} is not registered as the LoRA variant of any architecture.")
    return _base_of_lora[lora_cls]


def lora_config(model_cls):
    """The config class of the LoRA variant registered for the base model class ``model_cls``."""
    if model_cls not in _lora_of_base:
        raise ValueError(f"No LoRA variant has been registered for architecture {model_cls}.")
    return _config_of_base[model_cls]

"""LoRA (low-rank adaptation) versions of model architectures (reference tfimm/architectures/lora)."""
from .convnext import *  # noqa: F401,F403
from .factory import (  # noqa: F401
    convert_to_lora_model,
    convert_to_regular_model,
    create_model,
    lora_non_trainable_weights,
    lora_trainable_weights,
    merge_lora_weights,
    unmerge_lora_weights,
)
from .layers import LORA_WEIGHT_NAMES, convert_to_lora_layer, merge_kernel  # noqa: F401
from .registry import (  # noqa: F401
    lora_architecture,
    lora_base_architecture,
    lora_config,
    register_lora_architecture,
)

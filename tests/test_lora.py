"""``tfimm.architectures.lora`` without a GPU: the registry, the config and the variable inventory, the factory
functions, the two lowerings of ``LoRAConvNeXt`` and the checks of ``set_lora_weights``."""
import dataclasses
import warnings

import numpy as np
import pytest

import tfimm  # noqa: F401
from tfimm.architectures.convnext import ConvNeXt, ConvNeXtConfig
from tfimm.architectures.lora import (
    LORA_WEIGHT_NAMES,
    LoRAConvNeXt,
    LoRAConvNeXtConfig,
    convert_to_lora_model,
    convert_to_regular_model,
    create_model,
    lora_architecture,
    lora_base_architecture,
    lora_config,
    lora_non_trainable_weights,
    lora_trainable_weights,
    merge_lora_weights,
    register_lora_architecture,
    registry,
    unmerge_lora_weights,
)
from tfimm.engine.graph import Plan
from tfimm.utils.init import synthetic_weights

MINI = dict(name="lora_mini", input_size=(32, 32), embed_dim=(16, 32, 64, 128), nb_blocks=(1, 1, 2, 1), nb_classes=12)
N_BLOCKS = 5


def mini(**kw):
    return LoRAConvNeXt(LoRAConvNeXtConfig(**{**MINI, **kw}))


def kinds(model):
    return [op.kind for op in model.program().ops]


# ---- registry ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def scratch_registry():
    saved = [dict(d) for d in (registry._lora_of_base, registry._base_of_lora, registry._config_of_base)]
    yield
    for d, s in zip((registry._lora_of_base, registry._base_of_lora, registry._config_of_base), saved):
        d.clear()
        d.update(s)


def test_convnext_is_registered_and_the_model_registry_is_untouched():
    assert lora_architecture(ConvNeXt) is LoRAConvNeXt
    assert lora_base_architecture(LoRAConvNeXt) is ConvNeXt
    assert lora_config(ConvNeXt) is LoRAConvNeXtConfig
    assert LORA_WEIGHT_NAMES == ["kernel_lora_a", "kernel_lora_b"]
    assert not [n for n in tfimm.list_models() if "lora" in n.lower()]


def test_three_registration_forms(scratch_registry):
    class Cfg:
        pass

    class Base:
        pass

    @register_lora_architecture
    class Sub(Base):
        cfg_class = Cfg

    assert lora_architecture(Base) is Sub and lora_base_architecture(Sub) is Base and lora_config(Base) is Cfg

    class Other:
        pass

    @register_lora_architecture(base_cls=Other)
    class Unrelated:
        cfg_class = Cfg

    assert lora_architecture(Other) is Unrelated and lora_base_architecture(Unrelated) is Other

    class Flexible:
        cfg_class = Cfg

    assert register_lora_architecture(Flexible, base_cls=Flexible) is Flexible
    assert lora_architecture(Flexible) is Flexible and lora_base_architecture(Flexible) is Flexible


def test_registering_twice_warns_and_overwrites(scratch_registry):
    class Base:
        pass

    class First(Base):
        cfg_class = int

    class Second(Base):
        cfg_class = float

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        register_lora_architecture(First)
    with pytest.warns(UserWarning, match="already registered a LoRA version"):
        register_lora_architecture(Second)
    assert lora_architecture(Base) is Second and lora_config(Base) is float


def test_unknown_classes_raise_value_error():
    class Nobody:
        pass

    for fn in (lora_architecture, lora_base_architecture, lora_config):
        with pytest.raises(ValueError):
            fn(Nobody)
    with pytest.raises(ValueError):
        lora_base_architecture(ConvNeXt)          # a base class is not a LoRA class


# ---- config and variables ----------------------------------------------------------------------------------------------------
def test_config_fields_and_defaults():
    cfg = LoRAConvNeXtConfig()
    assert isinstance(cfg, ConvNeXtConfig)
    assert (cfg.lora_rank, cfg.lora_alpha, cfg.lora_train_bias, cfg.lora_train_classifer) == (4, 1.0, "none", True)
    extra = {f.name for f in dataclasses.fields(LoRAConvNeXtConfig)} - {f.name for f in dataclasses.fields(ConvNeXtConfig)}
    assert extra == {"lora_rank", "lora_alpha", "lora_train_bias", "lora_train_classifer"}


@pytest.mark.parametrize("rank", [1, 4, 17, 64])
def test_four_variables_per_block_and_param_count(rank):
    model = mini(lora_rank=rank)
    base = ConvNeXt(ConvNeXtConfig(**MINI))
    added = [k for k in model.weights if k not in base.weights]
    assert [k for k in model.weights if k in base.weights] == list(base.weights)
    assert len(added) == 4 * N_BLOCKS
    for j, (D, nb) in enumerate(zip(MINI["embed_dim"], MINI["nb_blocks"])):
        for i in range(nb):
            p = f"stages/{j}/blocks/{i}/mlp/"
            assert model.weights[p + "fc1/kernel_lora_a"].shape == (D, rank)
            assert model.weights[p + "fc1/kernel_lora_b"].shape == (rank, 4 * D)
            assert model.weights[p + "fc2/kernel_lora_a"].shape == (4 * D, rank)
            assert model.weights[p + "fc2/kernel_lora_b"].shape == (rank, D)
    # the order LoRADense.build creates them in: kernel, bias, kernel_lora_a, kernel_lora_b
    names = list(model.weights)
    i = names.index("stages/0/blocks/0/mlp/fc1/kernel")
    assert [n.rsplit("/", 1)[1] for n in names[i:i + 4]] == ["kernel", "bias", "kernel_lora_a", "kernel_lora_b"]
    per_block = sum(2 * rank * (D + 4 * D) * nb for D, nb in zip(MINI["embed_dim"], MINI["nb_blocks"]))
    assert model.count_params() == base.count_params() + per_block
    # initialisation: A glorot-uniform (not all zero, inside its limit), B zeros
    a, b = model.weights["stages/0/blocks/0/mlp/fc1/kernel_lora_a"], model.weights["stages/0/blocks/0/mlp/fc1/kernel_lora_b"]
    assert np.any(a) and np.abs(a).max() <= np.sqrt(6.0 / (16 + rank)) and not np.any(b)


def test_conv_mlp_block_and_bad_ranks_are_refused():
    with pytest.raises(ValueError, match="Unsupported layer type for conversion to LoRA"):
        mini(conv_mlp_block=True)
    for rank in (0, 65, -1, 2.0):
        with pytest.raises(ValueError, match="lora_rank"):
            mini(lora_rank=rank)


# ---- factory -------------------------------------------------------------------------------------------------------------------
def _with_adapter(model, seed=7, scale=0.5):
    """``model`` with synthetic base weights and non-zero seeded A and B"""
    w = synthetic_weights(model, 2021)
    rng = np.random.default_rng(seed)
    for k in w:
        if k.rsplit("/", 1)[1] in LORA_WEIGHT_NAMES:
            w[k] = (scale * rng.standard_normal(w[k].shape)).astype(np.float32)
    model.set_weights(w)
    return model


def test_convert_to_lora_model_copies_the_base_and_keeps_a_and_b():
    base = ConvNeXt(ConvNeXtConfig(**MINI))
    base.set_weights(synthetic_weights(base, 2021))
    model = convert_to_lora_model(base, lora_rank=8, lora_alpha=16.0)
    assert type(model) is LoRAConvNeXt and (model.cfg.lora_rank, model.cfg.lora_alpha) == (8, 16.0)
    fresh = mini(lora_rank=8, lora_alpha=16.0)
    for k, v in model.weights.items():
        want = fresh.weights[k] if k.rsplit("/", 1)[1] in LORA_WEIGHT_NAMES else base.weights[k]
        assert np.array_equal(v, want), k
    assert not model.merged


def test_create_model_by_name():
    model = create_model("convnext_tiny", nb_classes=10, lora_rank=2, lora_alpha=3.0)
    assert type(model) is LoRAConvNeXt and model.cfg.nb_classes == 10 and model.cfg.lora_rank == 2 and model.cfg.lora_alpha == 3.0
    base = tfimm.create_model("convnext_tiny", nb_classes=10)
    for k, v in base.weights.items():
        assert np.array_equal(model.weights[k], v), k
    assert not np.any(model.weights["stages/3/blocks/2/mlp/fc2/kernel_lora_b"])
    assert model.weights["stages/3/blocks/2/mlp/fc2/kernel_lora_a"].shape == (3072, 2)
    with pytest.raises(ValueError):
        create_model("resnet18")             # no LoRA architecture registered for ResNet


@pytest.mark.parametrize("merged", [False, True])
def test_convert_to_regular_model_merges_in_float32_and_leaves_the_merge_state(merged):
    model = _with_adapter(mini(lora_rank=3, lora_alpha=6.0))
    if merged:
        merge_lora_weights(model)
    base = convert_to_regular_model(model)
    assert type(base) is ConvNeXt and type(base.cfg) is ConvNeXtConfig and model.merged == merged
    assert not [k for k in base.weights if "lora" in k]
    w = model.weights
    assert "stages/0/blocks/0/mlp/fc1/kernel_lora_a" in w          # model.weights reports the unmerged variables
    for k, v in base.weights.items():
        if k.endswith(("mlp/fc1/kernel", "mlp/fc2/kernel")):
            a, b = w[k + "_lora_a"], w[k + "_lora_b"]
            want = w[k] + np.float32(6.0 / 3) * (a @ b)
            assert want.dtype == np.float32 and np.array_equal(v, want) and not np.array_equal(v, w[k]), k
        else:
            assert np.array_equal(v, w[k]), k


# ---- lowering ------------------------------------------------------------------------------------------------------------------
def test_unmerged_lowering_has_two_lora_deltas_per_block():
    model = _with_adapter(mini())
    prog = model.program()
    ops = prog.ops
    assert [op.kind for op in ops].count("lora_delta") == 2 * N_BLOCKS
    assert "mlp_fused" not in kinds(model) and "row_stats" not in kinds(model)
    for i, op in enumerate(ops):
        if op.kind != "lora_delta":
            continue
        gemm = ops[i + 1]
        assert gemm.kind == "gemm" and gemm.attrs["has_residual"] and gemm.inputs[-1] == op.output
        fc1 = op.attrs["a_name"].endswith("fc1/kernel_lora_a")
        assert gemm.attrs["act_after_res"] == fc1 and gemm.attrs["act"] == ("gelu" if fc1 else "")
        assert op.attrs["has_residual"] == (not fc1) and (op.attrs["out_scale"] is None) == fc1
        assert op.attrs["Rp"] == 16 and prog.consts[op.consts["a"]].host.shape == (16, op.attrs["K"])
        assert prog.consts[op.consts["b"]].host.shape == (op.attrs["N"], 16)


def test_merged_lowering_is_the_base_program_and_unmerging_restores():
    model = _with_adapter(mini())
    unmerged = kinds(model)
    base = convert_to_regular_model(model)
    merge_lora_weights(model)
    assert model.merged and not model._programs
    merge_lora_weights(model)                    # a second call does nothing
    assert model.merged
    assert kinds(model) == kinds(base) and "mlp_fused" in kinds(model) and "lora_delta" not in kinds(model)
    assert model.program().flops_per_image() == base.program().flops_per_image()
    for cm, cb in zip(model.program().consts, base.program().consts):
        assert cm.key == cb.key                  # the very constants of the base model over the merged kernels
    unmerge_lora_weights(model)
    assert not model.merged and kinds(model) == unmerged
    with pytest.raises(ValueError, match="LoRA updates have not been merged yet."):
        unmerge_lora_weights(model)


def test_dense_act_after_res_defaults_to_false_everywhere_else():
    base = ConvNeXt(ConvNeXtConfig(**MINI))
    assert not any(op.attrs["act_after_res"] for op in base.program().ops if op.kind == "gemm")


def test_plan_with_lora_delta_is_not_exported():
    model = _with_adapter(mini())
    plan = Plan(model.program(), 2, device="cpu")
    assert [fn.__name__ for fn, _ in plan.calls if fn != "memset"].count("tfimm_hip_lora_delta") == 2 * N_BLOCKS
    with pytest.raises(NotImplementedError, match="lora_delta"):
        plan.export()


# ---- trainable names -----------------------------------------------------------------------------------------------------------
def test_trainable_names_for_the_three_bias_modes():
    model = mini()
    names = list(model.weights)
    lora = [n for n in names if n.rsplit("/", 1)[1] in LORA_WEIGHT_NAMES]
    assert lora_trainable_weights(model) == lora
    got = lora_trainable_weights(model, train_bias="lora_only")
    assert got[:3] == ["stages/0/blocks/0/mlp/fc1/kernel_lora_a", "stages/0/blocks/0/mlp/fc1/kernel_lora_b",
                       "stages/0/blocks/0/mlp/fc1/bias"]
    assert sorted(got) == sorted(lora + [n for n in names if n.endswith(("mlp/fc1/bias", "mlp/fc2/bias"))])
    got = lora_trainable_weights(model, train_bias="all")
    assert got[:6] == ["stem/0/bias", "stem/1/beta", "stages/0/blocks/0/conv_dw/bias", "stages/0/blocks/0/norm/beta",
                       "stages/0/blocks/0/mlp/fc1/kernel_lora_a", "stages/0/blocks/0/mlp/fc1/kernel_lora_b"]
    assert sorted(got) == sorted(lora + [n for n in names if n.endswith(("/bias", "/beta"))])
    with pytest.raises(ValueError, match="Unknown value for train_bias"):
        lora_trainable_weights(model, train_bias="some")
    # the classifier
    got = lora_trainable_weights(model, trainable_layers=["head/fc"])
    assert got == lora + ["head/fc/kernel", "head/fc/bias"]
    assert lora_non_trainable_weights(model, trainable_layers=["head/fc"]) == [n for n in names if n not in set(got)]
    # as in the reference, the classifier pass does not look at what the bias pass listed
    assert lora_trainable_weights(model, "all", ["head/fc"])[-3:] == ["head/fc/bias", "head/fc/kernel", "head/fc/bias"]


def test_model_properties_honour_the_config():
    model = mini()
    assert model.trainable_weights == lora_trainable_weights(model, "none", ["head/fc"])
    assert set(model.trainable_weights) | set(model.non_trainable_weights) == set(model.weights)
    assert not set(model.trainable_weights) & set(model.non_trainable_weights)
    model = mini(lora_train_classifer=False, lora_train_bias="lora_only")
    assert model.trainable_weights == lora_trainable_weights(model, "lora_only")
    assert "head/fc/kernel" in model.non_trainable_weights and "stages/0/blocks/0/mlp/fc1/bias" in model.trainable_weights


# ---- set_lora_weights ----------------------------------------------------------------------------------------------------------
def test_set_lora_weights_validates_before_committing():
    model = _with_adapter(mini())
    prog = model.program()
    before = {k: v.copy() for k, v in model.weights.items()}
    keys = [c.key for c in prog.consts]
    good = "stages/0/blocks/0/mlp/fc1/kernel_lora_a"
    with pytest.raises(KeyError):
        model.set_lora_weights({good: np.ones((16, 4), np.float32), "stages/0/blocks/0/mlp/fc1/kernel": np.ones((16, 64))})
    with pytest.raises(KeyError):
        model.set_lora_weights({"no/such/kernel_lora_a": np.ones((16, 4))})
    with pytest.raises(ValueError):
        model.set_lora_weights({good: np.ones((16, 4), np.float32), "stages/0/blocks/0/mlp/fc1/kernel_lora_b": np.ones((5, 64))})
    assert all(np.array_equal(before[k], v) for k, v in model.weights.items())
    assert model.program() is prog and [c.key for c in prog.consts] == keys


def test_set_lora_weights_rewrites_the_packed_constants_in_place():
    model = _with_adapter(mini())
    prog = model.program()
    new = {k: (v + 1).astype(np.float32) for k, v in model.weights.items() if k.rsplit("/", 1)[1] in LORA_WEIGHT_NAMES}
    model.set_lora_weights(new)
    assert model.program() is prog and all(np.array_equal(model.weights[k], v) for k, v in new.items())
    fresh = mini()
    fresh.set_weights(model.weights)
    for c, f in zip(prog.consts, fresh.program().consts):
        assert c.key == f.key and np.array_equal(c.host, f.host), c.name
    # merged: every kernel changes, so the programs go
    merge_lora_weights(model)
    merged = model.program()
    model.set_lora_weights({k: v * 0 for k, v in new.items()})
    assert model.merged and model.program() is not merged
    assert not np.any(model.weights["stages/0/blocks/0/mlp/fc1/kernel_lora_a"])

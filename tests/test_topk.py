"""The output end without a GPU: the written rule (tests/topk_ref.py) against an independent formulation and hand-written
answers, the refusals of tfimm_hip_topk (include/tfimm_hip.h), the lowering of ``Model.program(top_k=k)`` and the
``ValueError`` cases of ``Model.top_k``."""
import ctypes as C

import numpy as np
import pytest

import test_architectures  # noqa: F401  (registers the miniature configs)
import tfimm
import topk_ref as tr
from tfimm.engine import ffi
from tfimm.utils.init import synthetic_weights

f32 = np.float32
NAN, INF = f32(np.nan), f32(np.inf)


# ---- the rule ----------------------------------------------------------------------------------------------------------
def _argsort_rule(x, k):
    """the independent formulation: a stable sort of the negated row keeps equal values in column order"""
    return np.stack([np.argsort(-r, kind="stable")[:k] for r in x]).astype(np.int32)


def _rows():
    rng = np.random.default_rng(7)
    zeros = np.array([0.0, -0.0, -1.0, -0.0, 0.0, -2.0, 0.0, -0.0], f32)
    return {
        "random": rng.standard_normal((5, 301)).astype(f32),
        "repeated": rng.integers(-3, 4, (5, 200)).astype(f32),                  # seven distinct values in 200 columns
        "all_equal": np.full((2, 70), 1.25, f32),
        "signed_zero": np.stack([zeros, -zeros]),
    }


@pytest.mark.parametrize("case", list(_rows()))
def test_rule_equals_a_stable_sort_of_the_negated_row(case):
    x = _rows()[case]
    for k in (1, 5, x.shape[1]):
        idx, values, _ = tr.topk(x, k)
        assert idx.dtype == np.int32 and values.dtype == np.float32
        assert np.array_equal(idx, _argsort_rule(x, k)), (case, k)
        assert np.array_equal(tr.bits(values), tr.bits(np.take_along_axis(x, idx.astype(np.int64), 1)))


def test_all_equal_row_and_zeros_come_in_column_order_with_their_own_bits():
    idx, _, _ = tr.topk(np.full((1, 9), -3.5, f32), 9)
    assert idx.tolist() == [list(range(9))]
    x = np.array([[-0.0, 0.0, -1.0, -0.0, 0.0]], f32)
    idx, values, _ = tr.topk(x, 4)
    assert idx.tolist() == [[0, 1, 3, 4]]                                        # -0.0 == +0.0: the column decides
    assert np.signbit(values[0]).tolist() == [True, False, True, False]         # and each keeps its sign


def test_nan_and_inf_rules_by_hand():
    neg_nan = np.array([0xffc00001], np.uint32).view(f32)[0]                    # sign set, payload 1
    x = np.array([[1.0, INF, -INF, NAN, 5.0, neg_nan, INF, -7.0]], f32)
    idx, values, probs = tr.topk(x, 8)
    #                  NaNs by column, then +inf twice by column, then the numbers, -inf last
    assert idx.tolist() == [[3, 5, 1, 6, 4, 0, 7, 2]]
    assert np.array_equal(tr.bits(values), tr.bits(x[0, idx[0]])[None])         # the negative NaN keeps sign and payload
    assert tr.bits(values)[0, 1] == 0xffc00001
    assert np.isnan(probs).all()                                                # not specified for such a row
    idx, values, _ = tr.topk(np.array([[-INF, -INF, -3.0]], f32), 2)
    assert idx.tolist() == [[2, 0]] and values.tolist() == [[-3.0, -np.inf]]


def test_probs_are_the_float64_softmax_at_the_selected_columns():
    x = np.random.default_rng(11).uniform(-8, 8, (4, 97)).astype(f32)
    idx, values, probs = tr.topk(x, 6)
    x64 = x.astype(np.float64)
    full = np.exp(x64) / np.exp(x64).sum(-1, keepdims=True)                     # (|x| <= 8: no need to subtract the maximum)
    assert probs.dtype == np.float64
    np.testing.assert_allclose(probs, np.take_along_axis(full, idx.astype(np.int64), 1), rtol=1e-13)
    assert (np.diff(probs, axis=1) <= 0).all() and abs(tr.softmax64(x).sum(-1) - 1).max() < 1e-12
    assert tr.topk(x, 6, probs=False)[2] is None


# ---- refusals: before any launch, so no GPU is involved ------------------------------------------------------------------
def _call(logits=True, ld=16, B=2, N=16, k=5, values=True, indices=True, probs=True):
    bufs = [np.zeros(64, f32), np.zeros(64, f32), np.zeros(64, np.int32), np.zeros(64, f32)]
    ptr = [C.c_void_p(b.ctypes.data) if on else None for b, on in zip(bufs, (logits, values, indices, probs))]
    rc = ffi.lib.tfimm_hip_topk(ptr[0], ld, B, N, k, ptr[1], ptr[2], ptr[3], None)
    return rc, ffi.lib.tfimm_hip_last_error().decode()


@pytest.mark.parametrize("kw, names", [
    (dict(logits=False), "logits"), (dict(values=False), "values"), (dict(indices=False), "indices"),
    (dict(k=0), "k=0"), (dict(k=-1), "k=-1"), (dict(k=17), "k=17"), (dict(N=100, ld=100, k=65), "k=65"),
    (dict(N=0), "N=0"), (dict(N=-4), "N=-4"), (dict(N=32769, ld=32769), "N=32769"),
    (dict(ld=15), "ld=15"), (dict(B=-1), "B=-1"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_refusals_return_minus_one_and_name_the_argument(kw, names):
    rc, msg = _call(**kw)
    assert rc == -1 and msg.startswith("topk:") and names in msg, (rc, msg)


def test_limits_in_the_header_and_the_binding_agree_and_an_empty_batch_is_no_launch():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfimm_hip.h")).read()
    assert int(re.search(r"#define TFIMM_TOPK_MAX_K (\d+)", hdr).group(1)) == ffi.TOPK_MAX_K == 64
    assert int(re.search(r"#define TFIMM_TOPK_MAX_N (\d+)", hdr).group(1)) == ffi.TOPK_MAX_N == 32768
    assert "tf.nn.softmax" in hdr and "tf.math.top_k" in hdr
    assert _call(B=0)[0] == 0                                                    # returns before any launch
    assert _call(B=0, probs=False)[0] == 0


# ---- lowering ------------------------------------------------------------------------------------------------------------
def _model(name, **kw):
    m = tfimm.create_model(name, **kw)
    m.set_weights(synthetic_weights(m))
    return m


def _op_list(prog):
    return [(op.kind, tuple(op.inputs), op.output, tuple(op.extra_outputs), sorted(op.attrs)) for op in prog.ops]


@pytest.mark.parametrize("name", ["resnet_test_model_1", "vit_test_model"])
def test_program_with_top_k_ends_in_one_topk_op_and_the_plain_program_is_untouched(name):
    before = _op_list(_model(name).program())            # a model that never saw top_k
    m = _model(name)
    p5 = m.program(top_k=5)
    plain = m.program()
    assert plain is not p5 and m.program(top_k=5) is p5 and m.program(top_k=3) is not p5
    assert _op_list(plain) == before and "topk" not in [op.kind for op in plain.ops]
    assert set(plain.outputs) == {"logits", "features"}
    assert _op_list(p5)[:-1] == before and p5.ops[-1].kind == "topk"
    assert [op.kind for op in p5.ops].count("topk") == 1
    assert sorted(p5.outputs) == ["features", "logits", "topk_indices", "topk_probs", "topk_values"]
    for out, dtype in (("topk_values", "f32"), ("topk_indices", "i32"), ("topk_probs", "f32")):
        t = p5.outputs[out]
        assert (t.rows, t.C, t.dtype, t.itemsize, t.keep) == (1, 5, dtype, 4, True), out
    op, logits = p5.ops[-1], p5.outputs["logits"]
    assert op.inputs == [logits.id] and logits.dtype == "f32" and logits.keep
    assert (op.attrs["N"], op.attrs["k"], op.attrs["ld"], op.attrs["rows"]) == (12, 5, logits.C, 1)
    assert p5.supports_branches()
    # program keys: the old ones as they were, the new one with its ("topk", k) element
    (old,) = [k for k in m._programs if len(k) == 4]
    assert old == (*m.cfg.input_size, False, "bf16")
    assert sorted(k for k in m._programs if k != old) == [old + (("topk", 3),), old + (("topk", 5),)]


@pytest.mark.parametrize("mode", ["bf16", "fp8", "fp32"])
def test_the_plan_binds_the_same_kernel_under_every_precision(mode):
    from tfimm.engine import precision
    with precision.use(mode):
        m = _model("vit_test_model")
        plan = m.program(top_k=4).make_plan(3, device="cpu")
        assert plan.check_marshalling() == len([c for c in plan.calls if c[0] != "memset"])
        fn, args = plan.calls[-1]
        assert fn.__name__ == "tfimm_hip_topk"
        t = plan.prog.outputs
        assert args == (plan.tptr(t["logits"].id), 12, 3, 12, 4, plan.tptr(t["topk_values"].id),
                        plan.tptr(t["topk_indices"].id), plan.tptr(t["topk_probs"].id))
        assert len({plan.assign[t[n].id] for n in ("logits", "topk_values", "topk_indices", "topk_probs")}) == 4
        assert tuple(plan.tensor_view(t["topk_indices"]).shape) == (3, 1, 4)
        assert str(plan.tensor_view(t["topk_indices"]).dtype) == "torch.int32"


def test_distilled_logits_are_two_heads_side_by_side_and_each_is_a_row():
    m = _model("deit_test_model")
    p = m.program(top_k=3)
    op = p.ops[-1]
    assert (op.attrs["rows"], op.attrs["N"], op.attrs["ld"], op.attrs["k"]) == (2, 12, 12, 3)
    assert (p.outputs["topk_indices"].rows, p.outputs["topk_indices"].C) == (2, 3)
    plan = p.make_plan(2, device="cpu")
    assert plan.calls[-1][1][1:5] == (12, 4, 12, 3)              # ld, B * heads, N, k


# ---- Model.top_k: what it refuses, before any device work ------------------------------------------------------------------
def test_top_k_value_errors_need_no_device():
    x = np.zeros((1, 32, 32, 3), f32)
    m = _model("vit_test_model")
    for k in (0, -2, 13, 65, 2.5, None):
        with pytest.raises(ValueError, match="k"):
            m.top_k(x, k)
    with pytest.raises(ValueError, match="64"):
        _model("vit_test_model", nb_classes=100).top_k(x, 65)
    with pytest.raises(ValueError, match="nb_classes == 0"):
        _model("vit_test_model", nb_classes=0).top_k(x, 1)
    with pytest.raises(ValueError, match="32768"):
        _model("vit_test_model", nb_classes=32769).top_k(x, 5)
    with pytest.raises(NotImplementedError):
        m.top_k(x, 5, training=True)
    assert not m._plans and not m._programs               # nothing was lowered, nothing touched a device


def test_tensor_numpy_keeps_int32_and_converts_floats_as_before():
    import torch
    i = tfimm.Tensor(torch.tensor([[3, 1]], dtype=torch.int32))
    assert i.numpy().dtype == np.int32 and i.numpy().tolist() == [[3, 1]]
    assert tfimm.Tensor(torch.tensor([1.5], dtype=torch.bfloat16)).numpy().dtype == np.float32
    assert tfimm.TopK._fields == ("indices", "values", "probs")

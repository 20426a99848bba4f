"""The embedding end without a GPU: the written rules (tests/embed_ref.py) against independent formulations and hand-written
answers, the surface and the lowering of ``tfimm.EmbeddingModel``, the ``ValueError`` cases of model and ``tfimm.Gallery``,
and the refusals of tfimm_hip_l2_normalize / tfimm_hip_embed_search (include/tfimm_hip.h)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import embed_ref as er
import test_architectures  # noqa: F401  (registers the miniature configs)
import tfimm
from tfimm.engine import ffi, precision
from tfimm.models.embedding_model import fold_head
from tfimm.utils.init import synthetic_weights

f32 = np.float32
EMB = ["emb/fc/kernel", "emb/fc/bias", "emb/bn/beta", "emb/bn/moving_mean", "emb/bn/moving_variance"]


# ---- the rules -----------------------------------------------------------------------------------------------------------
def _grid(rng, shape):
    return (rng.integers(-4, 5, shape) / 8).astype(f32)


@pytest.mark.parametrize("case", ["random", "ties"])
def test_search_rule_equals_a_stable_sort_of_the_negated_scores(case):
    rng = np.random.default_rng(3)
    if case == "random":
        q, g = rng.standard_normal((5, 48)).astype(f32), er.bf16_round(rng.standard_normal((301, 48)).astype(f32))
    else:
        q, g = _grid(rng, (5, 16)), _grid(rng, (200, 16))                  # a handful of distinct scores in 200 rows
    s = er.bf16_round(q).astype(np.float64) @ g.astype(np.float64).T
    for k in (1, 5, 64):
        idx, sc = er.search(q, g, k)
        assert idx.dtype == np.int32 and sc.dtype == np.float32 and idx.shape == sc.shape == (5, k)
        want = np.stack([np.argsort(-row, kind="stable")[:k] for row in s]).astype(np.int32)
        assert np.array_equal(idx, want), (case, k)
        assert np.array_equal(sc, np.take_along_axis(s, want.astype(np.int64), 1).astype(f32))


def test_ties_and_duplicates_by_hand():
    g = np.array([[1, 0], [0, 1], [1, 0], [2, 0], [1, 0], [0, 1]], f32).repeat(8, axis=1)     # E = 16
    q = np.array([[1] * 8 + [0] * 8, [0] * 8 + [1] * 8, [0] * 16], f32)
    idx, sc = er.search(q, g, 4)
    assert idx.tolist() == [[3, 0, 2, 4], [1, 5, 0, 2], [0, 1, 2, 3]]      # equal scores: the lower row first
    assert sc.tolist() == [[16, 8, 8, 8], [8, 8, 0, 0], [0, 0, 0, 0]]
    idx, _ = er.search(q[:1], np.tile(g[:1], (300, 1)), 7)                 # one row repeated: the first rows
    assert idx.tolist() == [list(range(7))]


def test_bf16_rounding_is_to_nearest_even():
    x = np.array([0x3f800000, 0x3f808000, 0x3f818000, 0x3f808001, 0x3f807fff, 0xbf818000], np.uint32).view(f32)
    want = np.array([0x3f800000, 0x3f800000, 0x3f820000, 0x3f810000, 0x3f800000, 0xbf820000], np.uint32)
    assert er.bits(er.bf16_round(x)).tolist() == want.tolist()
    import torch
    y = np.random.default_rng(0).standard_normal(4096).astype(f32)
    assert np.array_equal(er.bf16_round(y), torch.from_numpy(y).bfloat16().float().numpy())


def test_the_batchnorm_fold_reproduces_dense_plus_batchnorm():
    rng = np.random.default_rng(5)
    F, E = 24, 40
    w = {"emb/fc/kernel": rng.standard_normal((F, E)), "emb/fc/bias": rng.standard_normal(E), "emb/bn/beta": rng.standard_normal(E),
         "emb/bn/moving_mean": rng.standard_normal(E), "emb/bn/moving_variance": rng.uniform(0.01, 3.0, E)}
    x = rng.standard_normal((7, F))
    s = 1.0 / np.sqrt(w["emb/bn/moving_variance"] + 1e-3)
    kernel, bias = w["emb/fc/kernel"] * s, (w["emb/fc/bias"] - w["emb/bn/moving_mean"]) * s + w["emb/bn/beta"]
    ref = er.head(x, w)
    assert np.abs(x @ kernel + bias - ref).max() <= 1e-12 * np.abs(ref).max()
    # the library's own fold (evaluated in float64, handed out as float32) is that one, rounded once
    k32, b32 = fold_head(*[w[n] for n in EMB])
    assert k32.dtype == b32.dtype == np.float32
    assert np.array_equal(k32, kernel.astype(f32)) and np.array_equal(b32, bias.astype(f32))
    n = er.head(x, w, normalize=True)
    assert np.abs((n * n).sum(-1) - 1).max() < 1e-12 and np.array_equal(er.l2_normalize(np.zeros((2, 5))), np.zeros((2, 5)))


# ---- the model's surface ---------------------------------------------------------------------------------------------------
def _backbone(name="resnet_test_model_1", **kw):
    m = tfimm.create_model(name, **kw)
    m.set_weights(synthetic_weights(m))
    return m


def _op_list(prog):
    return [(op.kind, tuple(op.inputs), op.output, tuple(op.extra_outputs), sorted(op.attrs)) for op in prog.ops]


def test_weight_names_shapes_and_count():
    bb = _backbone()
    m = tfimm.EmbeddingModel(bb, 32)
    assert isinstance(m, tfimm.models.Model) and tfimm.models.EmbeddingModel is tfimm.EmbeddingModel
    F = bb.weights["remove/fc/kernel"].shape[0]
    assert m.weight_names() == bb.weight_names() + EMB
    assert [tuple(m.weights[n].shape) for n in EMB] == [(F, 32), (32,), (32,), (32,), (32,)]
    assert not any("gamma" in n for n in EMB)                                   # BatchNormalization(scale=False)
    assert m.count_params() == bb.count_params() + F * 32 + 4 * 32
    # Keras' defaults: glorot_uniform, zeros, zeros, zeros, ones
    lim = np.sqrt(6.0 / (F + 32))
    k = m.weights["emb/fc/kernel"]
    assert np.abs(k).max() <= lim and k.std() > lim / 3
    assert all(not m.weights[n].any() for n in EMB[1:4]) and (m.weights["emb/bn/moving_variance"] == 1).all()
    assert all(np.array_equal(m.weights[n], bb.weights[n]) for n in bb.weights)
    assert m.cfg is bb.cfg and np.array_equal(m.dummy_inputs, bb.dummy_inputs) and m.embed_dim == 32
    assert set(synthetic_weights(m)) == set(m.weights)                          # goes through WeightSpec / winit
    assert m.feature_names == bb.feature_names[:-1] + ["embeddings"] and m.feature_names[-2:] == ["features", "embeddings"]


def test_the_weights_are_a_snapshot_of_the_backbone():
    bb = _backbone()
    m = tfimm.EmbeddingModel(bb, 16)
    before = {k: v.copy() for k, v in m.weights.items()}
    bb.set_weights(synthetic_weights(bb, seed=7))
    assert all(np.array_equal(m.weights[k], before[k]) for k in before)
    assert not np.array_equal(bb.weights["conv1/kernel"], m.weights["conv1/kernel"])


def test_save_then_load_into_a_fresh_instance(tmp_path):
    m = tfimm.EmbeddingModel(_backbone(), 32)
    m.set_weights(synthetic_weights(m, seed=11))
    path = str(tmp_path / "emb.npz")
    m.save_weights(path)
    fresh = tfimm.EmbeddingModel(tfimm.create_model("resnet_test_model_1"), 32)
    assert not np.array_equal(fresh.weights["emb/bn/beta"], m.weights["emb/bn/beta"])
    fresh.load_weights(path)
    assert list(fresh.weights) == list(m.weights)
    assert all(np.array_equal(fresh.weights[k], m.weights[k]) for k in m.weights)
    with pytest.raises(KeyError):
        fresh.set_weights({k: v for k, v in m.weights.items() if k != "emb/fc/bias"})       # strict, as elsewhere


# ---- lowering ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["resnet_test_model_1", "vit_test_model", "swin_test_model", "efficientnet_test_model",
                                  "convnext_test_model", "cait_test_model"])
def test_program_has_the_head_and_no_classifier_and_leaves_the_backbone_alone(name):
    bb = _backbone(name)
    assert bb.cfg.nb_classes > 0
    before = _op_list(bb.program())
    keys = [list(d) for d in (bb._programs, bb._plans, bb._captured, bb._plan_uses, bb._const_cache)]
    m = tfimm.EmbeddingModel(bb, 32)
    m.set_weights(synthetic_weights(m))
    p = m.program()
    # the backbone's own outputs without "logits" (ConvNeXt always hands out conv_features too), plus the head's
    assert set(p.outputs) == (set(bb.program().outputs) - {"logits"}) | {"embeddings"} and "features" in p.outputs
    e, f = p.outputs["embeddings"], p.outputs["features"]
    assert (e.dtype, e.C, e.rows, e.keep) == ("f32", 32, f.rows, True)
    # the last op is the head: one GEMM over `features` with the folded weights, float32 out
    head = p.ops[-1]
    assert head.kind == "gemm" and head.inputs == [f.id] and head.output == e.id and head.attrs["out_f32"] == 1
    assert (head.attrs["K"], head.attrs["N"]) == (m.nb_features, 32)
    # nothing reads the classifier's kernel: no constant of the program is made from it
    cls_names = [n for n in bb.weights if n not in tfimm.create_model(name, nb_classes=0).weights]
    assert cls_names and all(n in m.weights for n in cls_names)
    const_names = {c.name for c in p.consts}
    assert not any(c.split(":")[0] in cls_names for c in const_names), const_names
    assert any(c.startswith("emb/fc/kernel") for c in const_names)
    # one op more than the classifier-free backbone (ResNet: its pooling behind the map is gone, the head took its place)
    bare = _backbone(name, nb_classes=0).program()
    assert len(p.ops) == len(bare.ops) + (0 if name.startswith("resnet") else 1)
    # normalize=True: exactly one op more, float32 to float32, and the marked output is its result
    n = tfimm.EmbeddingModel(bb, 32, normalize=True)
    n.set_weights(m.weights)
    pn = n.program()
    assert _op_list(pn)[:-1] == _op_list(p) and pn.ops[-1].kind == "l2_normalize"
    assert pn.ops[-1].output == pn.outputs["embeddings"].id and pn.outputs["embeddings"].dtype == "f32"
    assert pn.ops[-1].attrs == dict(rows=f.rows, E=32)
    # the backbone: same program object content, same keys in every cache
    assert _op_list(bb.program()) == before
    assert [list(d) for d in (bb._programs, bb._plans, bb._captured, bb._plan_uses, bb._const_cache)] == keys
    assert list(m._programs) == [(*m.cfg.input_size, False, "bf16")]


def test_dropping_the_stale_logits_removes_the_whole_chain_that_only_served_them():
    """a family whose classifier-free logits came from SEVERAL ops behind `features` must not keep dead launches: a synthetic
    program features -> a -> b -> stale (+ a side tensor that `a` alone reads), and one whose chain something else still reads"""
    from tfimm.engine.graph import Program
    from tfimm.models.embedding_model import EmbeddingModel
    p = Program()
    x, feats, side, a, b, stale = (p.new_tensor(1, 8, name=n) for n in ("x", "features", "side", "a", "b", "stale"))
    p.add("op0", [x], feats)
    p.add("op_side", [x], side)
    p.add("op_a", [feats, side], a)
    p.add("op_b", [a], b)
    p.add("op_stale", [b], stale)
    p.mark_output("features", feats)
    EmbeddingModel._drop_dead_ops(p, stale.id)
    assert [op.kind for op in p.ops] == ["op0"]
    q = Program()
    x, feats, a, stale, other = (q.new_tensor(1, 8, name=n) for n in ("x", "features", "a", "stale", "other"))
    q.add("op0", [x], feats)
    q.add("op_a", [feats], a)
    q.add("op_stale", [a], stale)
    q.add("op_other", [a], other)
    q.mark_output("features", feats)
    q.mark_output("other", other)
    EmbeddingModel._drop_dead_ops(q, stale.id)
    assert [op.kind for op in q.ops] == ["op0", "op_a", "op_other"]         # `a` still has a reader: it stays


@pytest.mark.parametrize("mode", ["bf16", "fp8", "fp32"])
def test_the_plan_binds_the_same_normalise_kernel_under_every_precision(mode):
    with precision.use(mode):
        bb = _backbone("vit_test_model")
        m = tfimm.EmbeddingModel(bb, 48, normalize=True)
        plan = m.program().make_plan(3, device="cpu")
        assert plan.check_marshalling() == len([c for c in plan.calls if c[0] != "memset"])
        fn, args = plan.calls[-1]
        assert fn.__name__ == "tfimm_hip_l2_normalize"
        assert args[1:4] == (48, 3, 48) and args[5] == 48 and args[4] == plan.tptr(plan.prog.outputs["embeddings"].id)
        assert tuple(plan.tensor_view(plan.prog.outputs["embeddings"]).shape) == (3, 1, 48)


def test_export_refuses_a_program_with_the_normalise_op():
    m = tfimm.EmbeddingModel(_backbone("vit_test_model"), 16, normalize=True)
    plan = m.program().make_plan(2, device="cpu")
    with pytest.raises(NotImplementedError, match="l2_normalize"):
        plan.export()


# ---- ValueError cases: before any device work ------------------------------------------------------------------------------
def test_value_errors_need_no_device():
    bb = _backbone("vit_test_model")
    for dim in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="embed_dim"):
            tfimm.EmbeddingModel(bb, dim)
    with pytest.raises(ValueError, match=r"\(B, F\)"):
        tfimm.EmbeddingModel(_backbone("deit_test_model"), 8)
    m = tfimm.EmbeddingModel(bb, 32)
    x = np.zeros((1, 32, 32, 3), f32)
    with pytest.raises(ValueError, match="classifier"):
        m.top_k(x, 1)
    with pytest.raises(ValueError, match="classifier"):
        m.program(top_k=3)
    with pytest.raises(NotImplementedError):
        m(x, training=True)
    with pytest.raises(ValueError, match="dim"):
        tfimm.Gallery(dim=24)
    with pytest.raises(ValueError, match="dim"):
        tfimm.Gallery(dim=4096)
    for dim in (0, 8, 2064, 16.0):
        with pytest.raises(ValueError, match="dim"):
            tfimm.Gallery(dim)
    g = tfimm.Gallery(32, capacity=4)
    assert (len(g), g.dim, g.numpy().shape) == (0, 32, (0, 32))
    with pytest.raises(ValueError, match="k = 1"):
        g.search(np.zeros((1, 32), f32), 1)                                   # k > len(g)
    with pytest.raises(ValueError, match="float32"):
        g.add(np.zeros((2, 32), np.float64))
    with pytest.raises(ValueError, match=r"\(n, 32\)"):
        g.add(np.zeros((2, 48), f32))
    with pytest.raises(ValueError, match="gallery holds rows of 48"):
        m.search(x, tfimm.Gallery(48), 1)
    assert not m._plans and tfimm.Matches._fields == ("indices", "scores")


# ---- refusals of the two entry points: before any launch, so no GPU is involved ----------------------------------------------
def _aligned(nbytes, align=64):
    raw = np.zeros(nbytes + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + nbytes]


def _normalize(x=True, ld_x=16, B=2, E=16, y=True, ld_y=16, x_off=0):
    bufs = [_aligned(4096), _aligned(4096)]
    ptr = [C.c_void_p(b.ctypes.data + o) if on else None for b, on, o in zip(bufs, (x, y), (x_off, 0))]
    rc = ffi.lib.tfimm_hip_l2_normalize(ptr[0], ld_x, B, E, ptr[1], ld_y, None)
    return rc, ffi.lib.tfimm_hip_last_error().decode()


@pytest.mark.parametrize("kw, names", [
    (dict(x=False), "x is null"), (dict(y=False), "y is null"), (dict(E=0), "E=0"), (dict(E=-2), "E=-2"),
    (dict(ld_x=15), "ld_x=15"), (dict(ld_y=15), "ld_y=15"), (dict(B=-1), "B=-1"), (dict(x_off=2), "aligned"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_normalize_refusals_name_the_argument(kw, names):
    rc, msg = _normalize(**kw)
    assert rc == -1 and msg.startswith("l2_normalize:") and names in msg, (rc, msg)


def _search(q=True, ld_q=32, B=2, g=True, ld_g=32, N=100, E=32, k=5, chunk=0, scores=True, indices=True, workspace=True,
            workspace_bytes=None, g_off=0, q_off=0):
    bufs = [_aligned(1 << 16) for _ in range(5)]
    on = (q, g, scores, indices, workspace)
    off = (q_off, g_off, 0, 0, 0)
    ptr = [C.c_void_p(b.ctypes.data + o) if f else None for b, f, o in zip(bufs, on, off)]
    if workspace_bytes is None:
        workspace_bytes = 1 << 16
    rc = ffi.lib.tfimm_hip_embed_search(ptr[0], ld_q, B, ptr[1], ld_g, N, E, k, chunk, ptr[2], ptr[3], ptr[4], workspace_bytes, None)
    return rc, ffi.lib.tfimm_hip_last_error().decode()


@pytest.mark.parametrize("kw, names", [
    (dict(q=False), "q is null"), (dict(g=False), "g is null"), (dict(scores=False), "scores is null"),
    (dict(indices=False), "indices is null"), (dict(workspace=False), "workspace is null"),
    (dict(g_off=8), "g must be 16-byte aligned"), (dict(q_off=2), "4-byte aligned"),
    (dict(E=0), "E=0"), (dict(E=8), "E=8"), (dict(E=24, ld_q=24, ld_g=24), "E=24"), (dict(E=2064, ld_q=2064, ld_g=2064), "E=2064"),
    (dict(N=0), "N=0"), (dict(N=-5), "N=-5"),
    (dict(k=0), "k=0"), (dict(k=-1), "k=-1"), (dict(k=101), "k=101"), (dict(N=1000, k=65), "k=65"),
    (dict(chunk=-32), "chunk=-32"), (dict(chunk=48), "chunk=48"), (dict(N=100000, k=64, chunk=32), "chunk=32"),
    (dict(ld_q=31), "ld_q=31"), (dict(ld_g=24), "ld_g=24"), (dict(ld_g=36), "ld_g=36"), (dict(B=-1), "B=-1"),
    (dict(B=65535 * 32 + 1), "B=2097121"),
    (dict(workspace_bytes=8), "workspace_bytes=8"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_search_refusals_name_the_argument(kw, names):
    rc, msg = _search(**kw)
    assert rc == -1 and msg.startswith("embed_search:") and names in msg, (rc, msg)


def test_workspace_limits_and_the_empty_batch():
    ws = ffi.lib.tfimm_hip_embed_search_workspace
    sizes = [ws(B, 100000, 512, 5, 0) for B in (1, 2, 31, 32, 33, 70, 256)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert all(ws(B, 5000, 64, 5, 32) < ws(B + 1, 5000, 64, 5, 32) for B in (1, 32, 100))
    assert ws(3, 5000, 64, 5, 32) == 3 * 157 * 5 * 8                     # k (key, row) pairs per query and chunk
    assert ws(1, 100, 24, 5, 0) < 0 and ws(1, 100, 32, 101, 0) < 0 and ws(1, 100, 32, 5, 48) < 0
    assert ffi.lib.tfimm_hip_last_error().decode().startswith("embed_search:")
    assert _search(B=0)[0] == 0 and _normalize(B=0)[0] == 0               # return before any launch
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfimm_hip.h")).read()
    for name, value in (("MIN_E", ffi.EMBED_MIN_E), ("MAX_E", ffi.EMBED_MAX_E), ("MAX_K", ffi.EMBED_MAX_K)):
        assert int(re.search(rf"#define TFIMM_EMBED_{name} (\d+)", hdr).group(1)) == value
    assert (ffi.EMBED_MIN_E, ffi.EMBED_MAX_E, ffi.EMBED_MAX_K) == (16, 2048, 64)
    assert int(re.search(r"#define TFIMM_EMBED_MAX_B (\d+)", hdr).group(1)) == ffi.EMBED_MAX_B == 65535 * 32
    assert ws(ffi.EMBED_MAX_B, 100, 32, 5, 0) > 0 and ws(ffi.EMBED_MAX_B + 1, 100, 32, 5, 0) < 0       # the same limit in both
    assert ffi.lib.tfimm_hip_abi_version() == 4

"""The distillation of an embedding head without a GPU: the written rule of tests/distill_ref.py against central differences
of its own loss and against numbers computed by hand; every refusal of tfimm_hip_distill_grad through the C ABI (nothing is
launched); the ``ValueError``s, the weight-decay scalar, the host state and the ``install`` identity of
``tfimm.EmbeddingProbe``."""
import os
import re

import numpy as np
import pytest
import torch

import distill_ref as dr
import head_fit_ref as hr
import test_architectures  # noqa: F401
import tfimm
from tfimm.engine import ffi
from tfimm.models.embedding_model import fold_head
from tfimm.train._head_probe import step_scalars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


# ---- the rule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
def test_row_gradient_against_central_differences(normalize):
    """d loss_b / d s against (L(s + h e) - L(s - h e)) / 2h in float64, h = 1e-6 |s|_max: |g - g_num| <= 1e-7 max |g|.
    (Truncation h^2 / 6 |L'''| and rounding 2^-53 |L| / h are both some 1e-10 of max |g| at this h.)"""
    rng = np.random.default_rng(5)
    worst = 0.0
    for E in (1, 2, 7, 64, 129):
        s, t = rng.normal(0, 2.0, (4, E)), rng.normal(0, 0.7, (4, E))
        g = dr.rows(s, t, None, normalize)[0]
        h = 1e-6 * np.abs(s).max()
        num = np.zeros_like(g)
        for e in range(E):
            d = np.zeros_like(s)
            d[:, e] = h
            num[:, e] = (dr.rows(s + d, t, None, normalize)[1] - dr.rows(s - d, t, None, normalize)[1]) / (2 * h)
        if E == 1 and normalize:
            assert np.abs(g).max() < 1e-15                      # a 1-vector normalises to +-1 whatever its length
            continue
        err = float(np.abs(g - num).max() / np.abs(g).max())
        worst = max(worst, err)
        assert err <= 1e-7, (E, err)
    print(f"row gradient against central differences, normalize={normalize}: worst |g - g_num| / max |g| = {worst:.3g}")


def test_the_short_form_is_the_projected_form():
    """2 inv_s (c u - v) == 2 inv_s ((u - v) - u (u . (u - v)))"""
    rng = np.random.default_rng(6)
    s, t = rng.normal(0, 1, (5, 33)), rng.normal(0, 1, (5, 33))
    u, inv_s, _ = dr.l2_normalize(s)
    v = dr.l2_normalize(t)[0]
    long_form = 2 * inv_s[:, None] * ((u - v) - u * (u * (u - v)).sum(axis=1, keepdims=True))
    assert np.abs(dr.rows(s, t)[0] - long_form).max() < 1e-14


def test_rows_by_hand_clamp_and_ignored():
    # s = (3, 4), t = (0, 2): u = (.6, .8), v = (0, 1), c = .8, loss = .36 + .04, grad = 2 / 5 (c u - v) = .4 (.48, -.36)
    g, loss, cos = dr.rows([[3.0, 4.0]], [[0.0, 2.0]])
    assert np.allclose(g, [[0.192, -0.144]], rtol=0, atol=1e-15) and abs(loss[0] - 0.4) < 1e-15 and abs(cos[0] - 0.8) < 1e-15
    g, loss, cos = dr.rows([[3.0, 4.0]], [[0.0, 2.0]], normalize=False)
    assert g.tolist() == [[6.0, 4.0]] and loss.tolist() == [13.0] and abs(cos[0] - 0.8) < 1e-15
    # s == t: loss 0, gradient 0, cosine 1; s == -t: loss 4, gradient 0 (a maximum), cosine -1
    g, loss, cos = dr.rows([[1.0, 2.0, 2.0]] * 2, [[1.0, 2.0, 2.0], [-1.0, -2.0, -2.0]])
    assert np.abs(g).max() < 1e-15 and np.allclose(loss, [0, 4], atol=1e-15) and np.allclose(cos, [1, -1], atol=1e-15)
    # the clamp: a row of 1e-8s has sum s^2 = 4e-16 < 1e-12: inv_s = 1e6, u = 0.01, grad = 2e6 (u - v), against central
    # differences of the clamped loss too
    s, t = np.full((1, 4), 1e-8), np.array([[0.5, 0.5, 0.5, -0.5]])
    g, loss, cos = dr.rows(s, t)
    assert np.allclose(g, 2e6 * (0.01 - t), rtol=1e-12) and abs(loss[0] - (3 * 0.49 ** 2 + 0.51 ** 2)) < 1e-12
    assert abs(cos[0] - 0.01) < 1e-12
    h = 1e-12
    for e in range(4):
        d = np.zeros_like(s)
        d[0, e] = h
        num = (dr.rows(s + d, t)[1] - dr.rows(s - d, t)[1]) / (2 * h)
        assert abs(num[0] - g[0, e]) <= 1e-7 * np.abs(g).max()
    # an ignored row: zeros in all three outputs, whatever it holds; the others are untouched by it
    g, loss, cos = dr.rows([[3.0, 4.0], [1.0, 1.0], [3.0, 4.0]], [[0.0, 2.0]] * 3, valid=[0, -1, 0])
    assert not g[1].any() and loss[1] == 0 and cos[1] == 0 and np.array_equal(g[0], g[2]) and g[0].any()


@pytest.mark.parametrize("normalize", [True, False])
def test_step_gradient_is_the_gradient_of_the_total_loss(normalize):
    """head_update's gr on the reference's rows (nothing rounded, ft = float64) against central differences of
    ``total_loss``: mean over the trained rows and the distillation weight-decay rule"""
    rng = np.random.default_rng(1)
    B, D, E, wd = 6, 8, 3, 0.3
    f, t = rng.normal(0, 1, (B, D)), rng.normal(0, 1, (B, E))
    w, bias = rng.normal(0, 0.5, (E, D)), rng.normal(0, 0.5, E)
    valid = [0, 0, -1, 0, -1, 0]
    g = dr.rows(f @ w.T + bias, t, valid, normalize)[0]
    out = hr.head_update(f, g, valid, w, np.zeros_like(w), None, bias, np.zeros_like(bias), None, hr.SGD,
                         (1.0, 0.0, 0.0, 0.0, dr.wd2(D, E, wd)), ft=f64)
    h = 1e-6
    for idx in np.ndindex(E, D):
        e = np.zeros_like(w)
        e[idx] = h
        fd = (dr.total_loss(w + e, bias, f, t, valid, wd, normalize) - dr.total_loss(w - e, bias, f, t, valid, wd, normalize)) / (2 * h)
        assert abs(fd + out["s1"][idx]) <= 1e-7 * np.abs(out["s1"]).max()
    for c in range(E):
        e = np.zeros_like(bias)
        e[c] = h
        fd = (dr.total_loss(w, bias + e, f, t, valid, wd, normalize) - dr.total_loss(w, bias - e, f, t, valid, wd, normalize)) / (2 * h)
        assert abs(fd + out["bias_s1"][c]) <= 1e-7 * np.abs(out["bias_s1"]).max()


# ---- the C ABI: refusals before any launch -----------------------------------------------------------------------------------
def test_distill_grad_refuses_before_any_launch():
    hdr = open(os.path.join(ROOT, "include", "tfimm_hip.h")).read()
    assert int(re.search(r"#define TFIMM_DISTILL_MAX_E (\d+)", hdr).group(1)) == ffi.DISTILL_MAX_E == 4096
    assert re.search(r"#define TFIMM_HIP_ABI_VERSION (\d+)", hdr).group(1) == "4"
    buf = torch.zeros(8192, dtype=torch.uint8)                  # host memory: the entry point returns before touching it
    p = (buf.data_ptr() + 15) // 16 * 16
    s, t, valid, grad, loss, cosine = p, p + 1024, p + 2048, p + 3072, p + 4096, p + 4224

    def call(s=s, ld_s=40, t=t, ld_t=37, B=2, E=37, valid=valid, normalize=1, grad=grad, ldg=40, loss=loss, cosine=cosine):
        rc = ffi.lib.tfimm_hip_distill_grad(s, ld_s, t, ld_t, B, E, valid, normalize, grad, ldg, loss, cosine, None)
        return rc, ffi.lib.tfimm_hip_last_error().decode()
    assert call(B=0)[0] == 0                                    # validated, nothing launched
    for k in ("s", "t", "valid", "grad", "loss", "cosine"):
        rc, msg = call(**{k: None})
        assert rc == -1 and msg.startswith("distill_grad:") and f" {k} is null" in msg, msg
    for k, v in (("s", s + 2), ("t", t + 1), ("valid", valid + 3), ("loss", loss + 2), ("cosine", cosine + 1)):
        rc, msg = call(**{k: v})
        assert rc == -1 and "4-byte aligned" in msg and k in msg, msg
    for off in (2, 4, 8):
        rc, msg = call(grad=grad + off)
        assert rc == -1 and "grad must be 16-byte aligned" in msg, msg
    for kw, word in ((dict(ld_s=36), "ld_s=36"), (dict(ld_t=36), "ld_t=36"), (dict(ldg=32), "ldg=32"), (dict(ldg=44), "ldg=44"),
                     (dict(E=0), "E=0"), (dict(E=-3), "E=-3"), (dict(E=4097, ld_s=4104, ld_t=4104, ldg=4104), "E=4097"),
                     (dict(B=-1), "B=-1"), (dict(normalize=2), "normalize=2"), (dict(normalize=-1), "normalize=-1")):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("distill_grad:") and word in msg, (kw, rc, msg)
    assert call(B=0, E=4096, ld_s=4096, ld_t=4096, ldg=4096, normalize=0)[0] == 0


# ---- EmbeddingProbe: ValueError before any device work -------------------------------------------------------------------------
def test_embedding_probe_value_errors():
    for dim in (12, 0, 4, 8200, 8.0, True):
        with pytest.raises(ValueError, match="dim"):
            tfimm.EmbeddingProbe(dim, 16)
    for n in (0, -1, 4097, 2.0, True):
        with pytest.raises(ValueError, match="embed_dim"):
            tfimm.EmbeddingProbe(16, n)
    with pytest.raises(ValueError, match="TFIMM_DISTILL_MAX_E = 4096"):
        tfimm.EmbeddingProbe(16, 4097)
    with pytest.raises(ValueError, match="TFIMM_HEAD_MAX_D"):
        tfimm.EmbeddingProbe(8200, 16)
    with pytest.raises(ValueError, match="optimizer"):
        tfimm.EmbeddingProbe(16, 8, optimizer="rmsprop")
    with pytest.raises(ValueError, match="lr"):
        tfimm.EmbeddingProbe(16, 8, lr="fast")
    probe = tfimm.EmbeddingProbe(16, 8)
    good_f, good_t = np.zeros((3, 16), f32), np.zeros((3, 8), f32)
    for bad in (np.zeros((3, 8), f32), np.zeros((3, 16), f64), np.zeros(16, f32), torch.zeros(3, 24)):
        with pytest.raises(ValueError, match="features"):
            probe.step(bad, good_t)
        with pytest.raises(ValueError, match="features"):
            probe(bad)
    # the teacher: rank (the (B, H, W, E) of an EmbeddingModel over a ResNet), width, dtype, batch
    for bad in (np.zeros((3, 2, 2, 8), f32), np.zeros((3, 9), f32), np.zeros(8, f32), torch.zeros(3, 8, dtype=torch.float64),
                np.zeros((3, 8), np.int32), torch.zeros(2, 8), tfimm.Tensor(torch.zeros(4, 8))):
        with pytest.raises(ValueError, match="teacher"):
            probe.step(good_f, bad)
    with pytest.raises(ValueError, match="a batch of 3"):
        probe.step(good_f, np.zeros((2, 8), f32))
    with pytest.raises(ValueError, match="TFIMM_HEAD_MAX_B"):
        probe.step(np.zeros((65536, 16), f32), np.zeros((65536, 8), f32))
    for bad in ([1, 0], np.ones((3, 1), bool), [0.5, 1.0, 1.0], torch.ones(3)):
        with pytest.raises(ValueError, match="valid"):
            probe.step(good_f, good_t, bad)
    assert probe.step_count == 0 and probe._dev is None        # nothing reached the device


def test_weight_decay_follows_the_distillation_rule():
    """reg = weight_decay * sum(w^2) / nb_variables, nb_variables = D E + E: wd2 = float32(2 wd / (D E + E)), formed in
    float64 and rounded once"""
    p = tfimm.EmbeddingProbe(64, 16, weight_decay=1e-4)
    assert p._decay() == 1e-4 / (64 * 16 + 16)
    for name in ("sgd", "adam"):
        sc = step_scalars(name, 0.1, (0.9, 0.999), 1e-7, p._decay(), 3)
        assert sc[4] == f32(2.0 * 1e-4 / (64 * 16 + 16)) == f32(dr.wd2(64, 16, 1e-4))
        assert sc[:4] == step_scalars(name, 0.1, (0.9, 0.999), 1e-7, 0.0, 3)[:4]
        want = dr.scalars(hr.ADAM if name == "adam" else hr.SGD, 0.1, (0.9, 0.999), 1e-7, 1e-4, 3, 64, 16)
        assert sc == tuple(f32(v) for v in want)
    assert tfimm.LinearProbe(64, 16, weight_decay=1e-4)._decay() == 1e-4       # the classification rule is untouched


def test_embedding_probe_host_state_round_trip():
    a, b = tfimm.EmbeddingProbe(64, 24, seed=3), tfimm.EmbeddingProbe(64, 24, seed=3)
    w = a.weights
    assert w["kernel"].shape == (64, 24) and w["kernel"].dtype == f32 and not w["bias"].any()
    assert np.array_equal(w["kernel"], b.weights["kernel"]) and np.abs(w["kernel"]).max() <= np.sqrt(6.0 / 88)
    assert np.array_equal(w["kernel"], tfimm.LinearProbe(64, 24, seed=3).weights["kernel"])       # the same Dense initialiser
    assert a.embed_dim == 24 and a.normalize_embeddings and not tfimm.EmbeddingProbe(64, 24, False).normalize_embeddings
    sd = a.state_dict()
    assert sorted(sd) == ["bias", "bias_s1", "bias_s2", "kernel", "optimizer", "s1", "s2", "step"] and sd["step"] == 0
    rng = np.random.default_rng(0)
    for k in ("kernel", "s1", "s2", "bias", "bias_s1", "bias_s2"):
        sd[k] = rng.normal(0, 1, sd[k].shape).astype(f32)
    sd["step"] = np.int64(9)
    b.load_state_dict(sd)
    back = b.state_dict()
    assert b.step_count == 9 and all(np.array_equal(back[k].view(np.uint32), sd[k].view(np.uint32)) for k in sd if k not in ("step", "optimizer"))
    b.set_weights({"kernel": w["kernel"], "bias": w["bias"] + 1})
    assert np.array_equal(b.weights["bias"], w["bias"] + 1) and np.array_equal(b.state_dict()["s1"], sd["s1"]) and b.step_count == 9
    with pytest.raises(ValueError, match="EmbeddingProbe.set_weights: 'kernel' has shape"):
        b.set_weights({"kernel": np.zeros((24, 64)), "bias": np.zeros(24)})
    with pytest.raises(ValueError, match="optimizer"):
        tfimm.EmbeddingProbe(64, 24, optimizer="adam").load_state_dict(sd)


def test_for_model_and_the_install_identity():
    """``install`` writes values with which ``fold_head`` -- what the EmbeddingModel lowers -- gives the probe's W and b back
    as float32 bits; ``for_model`` starts from the folded head"""
    student = tfimm.create_model("vit_hd80_test_model")
    model = tfimm.EmbeddingModel(student, 16)
    rng = np.random.default_rng(4)
    model.set_weights({"emb/bn/moving_mean": rng.normal(0, 1, 16).astype(f32), "emb/bn/beta": rng.normal(0, 1, 16).astype(f32),
                       "emb/bn/moving_variance": rng.uniform(0.5, 2, 16).astype(f32)}, strict=False)
    w = model.weights
    folded = fold_head(w["emb/fc/kernel"], w["emb/fc/bias"], w["emb/bn/beta"], w["emb/bn/moving_mean"], w["emb/bn/moving_variance"])
    probe = tfimm.EmbeddingProbe.for_model(model, optimizer="adam", lr=0.01)
    assert (probe.dim, probe.embed_dim, probe.optimizer) == (160, 16, "adam")
    assert np.array_equal(probe.weights["kernel"], folded[0]) and np.array_equal(probe.weights["bias"], folded[1])
    # a head of values that exercise every float32 exponent around 1, installed and folded again
    fitted = tfimm.EmbeddingProbe(160, 16, seed=5)
    k = (rng.normal(0, 1, (160, 16)) * 10.0 ** rng.integers(-6, 3, (160, 16))).astype(f32)
    b = rng.normal(0, 3, 16).astype(f32)
    fitted.set_weights({"kernel": k, "bias": b})
    before = {n: v.copy() for n, v in model.weights.items()}
    fitted.install(model)
    w = model.weights
    again = fold_head(w["emb/fc/kernel"], w["emb/fc/bias"], w["emb/bn/beta"], w["emb/bn/moving_mean"], w["emb/bn/moving_variance"])
    assert np.array_equal(again[0].view(np.uint32), k.view(np.uint32)) and np.array_equal(again[1].view(np.uint32), b.view(np.uint32))
    assert w["emb/bn/moving_variance"].tolist() == [float(f32(1 - 1e-3))] * 16 and not w["emb/bn/beta"].any()
    assert all(np.array_equal(w[n], v) for n, v in before.items() if not n.startswith("emb/"))
    # refusals: another shape, a model that is no EmbeddingModel
    with pytest.raises(ValueError, match="embed_dim = 8"):
        tfimm.EmbeddingProbe(160, 8).install(model)
    with pytest.raises(ValueError, match="install"):
        tfimm.EmbeddingProbe(168, 16).install(model)
    for bad in (student, None):
        with pytest.raises(ValueError, match="EmbeddingModel"):
            fitted.install(bad)
        with pytest.raises(ValueError, match="EmbeddingModel"):
            tfimm.EmbeddingProbe.for_model(bad)


def test_distill_head_checks_the_teacher_before_any_device_work():
    student = tfimm.create_model("vit_hd80_test_model")
    probe = tfimm.EmbeddingProbe(160, 16)
    x = np.zeros((4,) + tuple(student.cfg.input_size) + (student.cfg.in_channels,), f32)
    for bad in (np.zeros((3, 16), f32), np.zeros((4, 2, 2, 16), f32), np.zeros((4, 8), f32)):
        with pytest.raises(ValueError, match="distill_head: teacher"):
            student.distill_head(x, bad, probe)
    with pytest.raises(ValueError, match="distill_head: valid"):
        student.distill_head(x, np.zeros((4, 16), f32), probe, valid=[True, False])
    assert probe.step_count == 0 and probe._dev is None

"""The head fit without a GPU: the written rule of tests/head_fit_ref.py against finite differences of its own loss and against
numbers computed by hand; every refusal of tfimm_hip_softmax_grad and tfimm_hip_head_update through the C ABI (nothing is
launched); the ctypes mirror of the descriptor against the header; the ``ValueError``s of ``tfimm.LinearProbe``."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import head_fit_ref as hr
import test_architectures  # noqa: F401
import tfimm
from tfimm.engine import ffi
from tfimm.train.linear_probe import step_scalars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def test_gradient_of_the_reference_against_central_differences_of_its_loss():
    """d total_loss / d (w, bias) against (L(x + h) - L(x - h)) / 2h, h = 1e-5, one row ignored (-1) and one label out of range.
    The bar: truncation h^2 / 6 |L'''| (third derivatives of a softmax cross-entropy over features of size <= 2 are below
    10: 2e-10) plus rounding 2^-53 |L| / h (|L| <= 4: 5e-11); 1e-8 leaves two orders of slack and is seven orders below the
    gradient's entries."""
    rng = np.random.default_rng(0)
    B, D, Cn, wd = 6, 8, 4, 0.05
    f = rng.uniform(-2, 2, (B, D))
    w, bias = rng.uniform(-0.5, 0.5, (Cn, D)), rng.uniform(-0.5, 0.5, Cn)
    labels = [0, 3, -1, 1, Cn, 2]
    gw, gb = hr.total_grad(w, bias, f, labels, wd)
    h, worst = 1e-5, 0.0
    for idx in np.ndindex(Cn, D):
        e = np.zeros_like(w)
        e[idx] = h
        fd = (hr.total_loss(w + e, bias, f, labels, wd) - hr.total_loss(w - e, bias, f, labels, wd)) / (2 * h)
        worst = max(worst, abs(fd - gw[idx]))
    for c in range(Cn):
        e = np.zeros_like(bias)
        e[c] = h
        fd = (hr.total_loss(w, bias + e, f, labels, wd) - hr.total_loss(w, bias - e, f, labels, wd)) / (2 * h)
        worst = max(worst, abs(fd - gb[c]))
    print(f"gradient against central differences: max |error| {worst:.3g}")
    assert worst <= 1e-8 and np.abs(gw).max() > 1e-2
    # the rows that are not scored contribute nothing, and n counts the four others
    keep = [0, 1, 3, 5]
    gw4, gb4 = hr.total_grad(w, bias, f[keep], [labels[i] for i in keep], wd)
    assert np.allclose(gw, gw4, rtol=0, atol=1e-15) and np.allclose(gb, gb4, rtol=0, atol=1e-15)
    # ... and head_update's gr is that gradient when nothing is rounded
    g = hr.p_minus_onehot(f @ w.T + bias, labels)
    out = hr.head_update(f, g, labels, w, np.zeros_like(w), None, bias, np.zeros_like(bias), None, hr.SGD,
                         (1.0, 0.0, 0.0, 0.0, 2 * wd), ft=f64)
    assert np.allclose(-out["s1"], gw, rtol=0, atol=1e-15) and np.allclose(-out["bias_s1"], gb, rtol=0, atol=1e-15)


F8 = np.arange(1.0, 9.0)          # the features of the 1 x 8 head: f = 1 .. 8, g = 0.5, n = 1: acc = f / 2, accb = 0.5


def _one_by_eight(opt, sc, s1=0.0, s2=0.0, ft=f32):
    w = np.ones((1, 8))
    return hr.head_update(F8[None, :], [[0.5]], [0], w, np.full((1, 8), s1), np.full((1, 8), s2), [1.0], [s1], [s2], opt, sc, ft=ft)


@pytest.mark.parametrize("ft", [f32, f64])
def test_weight_decay_sgd_and_adam_steps_by_hand(ft):
    # wd2 = 0.5 on w = 1: gr = f / 2 + 1 / 2 = 1, 1.5, .. 4.5.  sgd, lr 1/4, momentum 1/2 on s1 = 2:
    #   s1 = 1 - gr / 4 = 0.75, 0.625, .. -0.125 ; w = 1 + s1
    o = _one_by_eight(hr.SGD, (0.25, 0.5, 0.0, 0.0, 0.5), s1=2.0, ft=ft)
    assert o["grad_out"].tolist() == [[0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0]]
    assert o["s1"].tolist() == [[0.75, 0.625, 0.5, 0.375, 0.25, 0.125, 0.0, -0.125]]
    assert o["w"].tolist() == [[1.75, 1.625, 1.5, 1.375, 1.25, 1.125, 1.0, 0.875]]
    assert o["w16"].tolist() == o["w"].tolist()                                  # all of them bf16 values
    # the bias: accb = 0.5, gr = 1: s1 = 1 - 1 / 4, bias = 1.75
    assert (o["bias_grad_out"].tolist(), o["bias_s1"].tolist(), o["bias"].tolist()) == ([0.5], [0.75], [1.75])
    # without weight decay and momentum: w = 1 - lr * f / 2
    o = _one_by_eight(hr.SGD, (0.25, 0.0, 0.0, 0.0, 0.0), ft=ft)
    assert o["w"].tolist() == [[0.875, 0.75, 0.625, 0.5, 0.375, 0.25, 0.125, 0.0]]
    # adam from zero slots, 1 - b1 = 1/2, 1 - b2 = 1/4, lr_t = 1/2, eps = 0, wd2 = 0.5:
    #   s1 = gr / 2, s2 = gr^2 / 4, sqrt(s2) = gr / 2: w = 1 - (gr / 4) / (gr / 2) = 1/2 everywhere
    o = _one_by_eight(hr.ADAM, (0.5, 0.5, 0.25, 0.0, 0.5), ft=ft)
    assert o["s1"].tolist() == [[0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0, 2.25]]
    assert o["s2"].tolist() == [[0.25, 0.5625, 1.0, 1.5625, 2.25, 3.0625, 4.0, 5.0625]]
    assert o["w"].tolist() == [[0.5] * 8] and o["bias"].tolist() == [0.5]
    # eps = 1/2 moves the denominator: element 0 has sqrt(s2) + eps = 1: w = 1 - 1/4; element 2: 1 - (1/2) / (3/2) = 2/3
    o = _one_by_eight(hr.ADAM, (0.5, 0.5, 0.25, 0.5, 0.5), ft=ft)
    assert o["w"][0, 0] == 0.75 and o["w"][0, 2] == ft(1.0) - ft(0.5) / ft(1.5)
    # nonzero slots: s1 = 1 + (gr - 1) / 2, s2 = 4 + (gr^2 - 4) / 4 ; element 0 (gr = 1): s1 = 1, s2 = 3.25
    o = _one_by_eight(hr.ADAM, (0.5, 0.5, 0.25, 0.0, 0.5), s1=1.0, s2=4.0, ft=ft)
    assert (o["s1"][0, 0], o["s2"][0, 0]) == (1.0, 3.25) and o["w"][0, 0] == ft(1.0) - ft(0.5) / np.sqrt(ft(3.25))


def test_an_all_ignored_batch_is_a_defined_step():
    """n = 0: inv_n = 1, the data gradient is zero; weight decay and the slots' decay act"""
    z = np.zeros((2, 1))
    o = hr.head_update(np.ones((2, 8)), z, [-1, 5], np.ones((1, 8)), np.full((1, 8), 2.0), None, [1.0], [2.0], None, hr.SGD,
                       (0.25, 0.5, 0.0, 0.0, 0.5))
    assert not o["grad_out"].any() and o["s1"].tolist() == [[0.875] * 8] and o["w"].tolist() == [[1.875] * 8]
    assert np.isfinite(o["bias"]).all()


def test_bf16_roundings_and_scalars():
    a = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-41], f32)       # ties: to even; a subnormal
    assert hr.bf16_rne(a).tolist()[:4] == [1.0, 1.0, 1.015625, -1.0]
    assert hr.bf16_trunc(a).tolist()[:4] == [1.0, 1.0, 1.0078125, -1.0]
    for t in (1, 7):
        want = hr.scalars(hr.ADAM, 0.01, (0.9, 0.999), 1e-7, 1e-4, t)
        assert step_scalars("adam", 0.01, (0.9, 0.999), 1e-7, 1e-4, t) == tuple(f32(v) for v in want)
    assert step_scalars("sgd", 0.1, (0.9, 0.999), 1e-7, 1e-4, 3) == (f32(0.1), f32(0.9), f32(0), f32(1e-7), f32(2e-4))


# ---- the C ABI: refusals before any launch -----------------------------------------------------------------------------------
def _struct_fields(hdr, open_marker, close_marker):
    body = hdr[hdr.index(open_marker):hdr.index(close_marker)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split("{", 1)[1].split(";"):
        toks = [t for t in decl.strip().replace("*", " ").split() if t != "const"]
        if toks:
            names += [n.strip() for n in " ".join(toks[1:]).split(",")]
    return names


def test_head_update_desc_layout_matches_header():
    hdr = open(os.path.join(ROOT, "include", "tfimm_hip.h")).read()
    names = _struct_fields(hdr, "typedef struct tfimm_head_update_desc {", "} tfimm_head_update_desc;")
    assert names == [f[0] for f in ffi.HeadUpdateDesc._fields_], names
    assert C.sizeof(ffi.HeadUpdateDesc) == 12 * 8 + 8 * 4 + 5 * 4 + 4        # 12 pointers, 8 int32, 5 floats, tail padding
    for name in ("HEAD_SGD", "HEAD_ADAM", "HEAD_MAX_D", "HEAD_MAX_C", "HEAD_MAX_B"):
        assert int(re.search(rf"#define TFIMM_{name} (\d+)", hdr).group(1)) == getattr(ffi, name)
    assert re.search(r"#define TFIMM_HIP_ABI_VERSION (\d+)", hdr).group(1) == "4"


B0, D0, C0 = 4, 16, 5             # the valid descriptor every refusal departs from; pitches 24 / 8 / 20 / 24


class _Host:
    """host memory behind a descriptor: the entry point validates and returns before anything would touch it"""

    def __init__(self):
        self.t = {k: torch.zeros(n, dtype=torch.uint8) for k, n in
                  (("f", B0 * 24 * 2 + 64), ("g", B0 * 8 * 2 + 64), ("labels", B0 * 4 + 64), ("w", C0 * 20 * 4 + 64),
                   ("w16", C0 * 24 * 2 + 64), ("s1", C0 * 20 * 4 + 64), ("s2", C0 * 20 * 4 + 64), ("bias", 64 + 64),
                   ("bias_s1", 128), ("bias_s2", 128), ("grad_out", C0 * 20 * 4 + 64), ("bias_grad_out", 128))}

    def ptr(self, k):
        return (self.t[k].data_ptr() + 15) // 16 * 16

    def desc(self, opt=ffi.HEAD_ADAM):
        d = ffi.HeadUpdateDesc()
        for k in self.t:
            setattr(d, k, self.ptr(k))
        d.B, d.D, d.C = B0, D0, C0
        d.ldf, d.ldg, d.ldw, d.ldw16 = 24, 8, 20, 24
        d.opt = opt
        d.lr, d.mom_or_one_minus_b1, d.one_minus_b2, d.eps, d.wd2 = 0.1, 0.1, 0.001, 1e-7, 0.0
        return d


def _refused(d, code, *words):
    rc = ffi.lib.tfimm_hip_head_update(C.byref(d), None)
    msg = ffi.lib.tfimm_hip_last_error().decode()
    assert rc == code, (rc, msg)
    assert msg.startswith("head_update:") and all(w in msg for w in words), msg


def test_head_update_refuses_before_any_launch():
    h = _Host()
    assert ffi.lib.tfimm_hip_head_update(None, None) == -1
    # B == 0: validated, nothing launched, 0
    d = h.desc()
    d.B = 0
    assert ffi.lib.tfimm_hip_head_update(C.byref(d), None) == 0
    d.opt = ffi.HEAD_SGD
    d.s2 = d.bias_s2 = d.grad_out = d.bias_grad_out = None                      # sgd needs no second slot; the outputs are optional
    assert ffi.lib.tfimm_hip_head_update(C.byref(d), None) == 0
    # a NULL required pointer
    for k in ("f", "g", "labels", "w", "w16", "s1", "bias", "bias_s1"):
        d = h.desc()
        setattr(d, k, None)
        _refused(d, -1, f" {k} is null")
    for k in ("s2", "bias_s2"):                                                  # adam keeps two slots
        d = h.desc()
        setattr(d, k, None)
        _refused(d, -1, f" {k} is null", "adam")
    # pitches: below the row, or not a multiple of 8 (ldw: 4)
    for k, bad in (("ldf", (8, 20)), ("ldg", (0, 12)), ("ldw16", (8, 20)), ("ldw", (12, 18))):
        for v in bad:
            d = h.desc()
            setattr(d, k, v)
            _refused(d, -1, f"{k}={v}")
    # alignment: 16 bytes for the matrices, 4 for labels and the bias vectors
    for k in ("f", "g", "w", "w16", "s1", "s2", "grad_out"):
        d = h.desc()
        setattr(d, k, h.ptr(k) + 8)
        _refused(d, -1, "16-byte aligned", k)
    for k in ("labels", "bias", "bias_s1", "bias_s2", "bias_grad_out"):
        d = h.desc()
        setattr(d, k, h.ptr(k) + 2)
        _refused(d, -1, "4-byte aligned", k)
    # limits: TFIMM_EUNSUP
    for k, bad in (("D", (12, 0, 8200)), ("C", (0, -1, 32769)), ("B", (65536,))):
        for v in bad:
            d = h.desc()
            setattr(d, k, v)
            if k == "D":
                d.ldf = d.ldw = d.ldw16 = 8208
            if k == "C":
                d.ldg = 32776
            _refused(d, -2, f"{k}={v}")
    d = h.desc()
    d.B = -1
    _refused(d, -1, "B=-1")
    d = h.desc()
    d.opt = 2
    _refused(d, -1, "opt=2")
    # an output overlapping another operand: in place on an input, two outputs on each other, a partial overlap
    for out, other in (("w", "f"), ("grad_out", "w"), ("s1", "s2"), ("w16", "g"), ("bias", "labels"), ("bias_grad_out", "bias_s1")):
        d = h.desc()
        setattr(d, out, getattr(d, other))
        _refused(d, -1, "overlaps", out, other)
    d = h.desc()
    d.grad_out = h.ptr("w") + 16 * 20                                            # row 4 of w
    _refused(d, -1, "grad_out overlaps w")
    d = h.desc(ffi.HEAD_SGD)
    d.s2 = d.w                                                                   # sgd never touches s2: no overlap to refuse ...
    d.B = 0
    assert ffi.lib.tfimm_hip_head_update(C.byref(d), None) == 0


def test_softmax_grad_refuses_before_any_launch():
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = (buf.data_ptr() + 15) // 16 * 16
    x, y, g, loss, pred = p, p + 1024, p + 2048, p + 3072, p + 3200

    def call(x=x, ld=40, B=2, N=37, y=y, g=g, ldg=40, loss=loss, pred=pred):
        rc = ffi.lib.tfimm_hip_softmax_grad(x, ld, B, N, y, g, ldg, loss, pred, None)
        return rc, ffi.lib.tfimm_hip_last_error().decode()
    assert call(B=0)[0] == 0
    for k in ("x", "y", "g", "loss", "pred"):
        rc, msg = call(**{k: None})
        assert rc == -1 and "is null" in msg and msg.startswith("softmax_grad:"), msg
    for kw, word in ((dict(N=0), "N=0"), (dict(N=32769, ld=32776, ldg=32776), "N=32769"), (dict(ld=36), "ld=36"),
                     (dict(ldg=32), "ldg=32"), (dict(ldg=44), "ldg=44"), (dict(B=-1), "B=-1"), (dict(g=g + 8), "grad"),
                     (dict(x=x + 2), "4-byte"), (dict(loss=loss + 1), "4-byte"), (dict(pred=pred + 2), "4-byte"),
                     (dict(y=y + 3), "4-byte")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)


# ---- LinearProbe: ValueError before any device work ----------------------------------------------------------------------------
def test_linear_probe_value_errors():
    for dim in (12, 0, 4, 8200, 8.0, True):
        with pytest.raises(ValueError, match="dim"):
            tfimm.LinearProbe(dim, 5)
    for n in (0, -1, 32769, 2.0):
        with pytest.raises(ValueError, match="nb_classes"):
            tfimm.LinearProbe(16, n)
    with pytest.raises(ValueError, match="optimizer"):
        tfimm.LinearProbe(16, 5, optimizer="rmsprop")
    with pytest.raises(ValueError, match="lr"):
        tfimm.LinearProbe(16, 5, lr="fast")
    for kw in ("clipnorm", "clipvalue"):
        with pytest.raises(TypeError):
            tfimm.LinearProbe(16, 5, **{kw: 1.0})
    probe = tfimm.LinearProbe(16, 5)
    for bad in (np.zeros((3, 8), f32), np.zeros((3, 16), np.float64), np.zeros(16, f32), torch.zeros(3, 24)):
        with pytest.raises(ValueError, match="features"):
            probe.step(bad, [0, 1, 2])
        with pytest.raises(ValueError, match="features"):
            probe(bad)
    with pytest.raises(ValueError, match="labels"):
        probe.step(np.zeros((3, 16), f32), [0, 1])
    with pytest.raises(ValueError, match="labels"):
        probe.step(np.zeros((3, 16), f32), [0.5, 1, 2])
    assert probe.step_count == 0


def test_linear_probe_host_state_for_model_and_install():
    a, b = tfimm.LinearProbe(64, 5, seed=3), tfimm.LinearProbe(64, 5, seed=3)
    w = a.weights
    assert w["kernel"].shape == (64, 5) and w["kernel"].dtype == f32 and not w["bias"].any()
    assert np.array_equal(w["kernel"], b.weights["kernel"]) and not np.array_equal(w["kernel"], tfimm.LinearProbe(64, 5, seed=4).weights["kernel"])
    assert np.abs(w["kernel"]).max() <= np.sqrt(6.0 / 69)                        # glorot uniform
    sd = a.state_dict()
    assert sorted(sd) == ["bias", "bias_s1", "bias_s2", "kernel", "optimizer", "s1", "s2", "step"] and sd["step"] == 0
    sd["kernel"] = sd["kernel"] + 1
    sd["step"] = np.int64(9)
    b.load_state_dict(sd)
    assert b.step_count == 9 and np.array_equal(b.weights["kernel"], w["kernel"] + 1)
    with pytest.raises(ValueError, match="shape"):
        b.set_weights({"kernel": np.zeros((5, 64)), "bias": np.zeros(5)})
    with pytest.raises(ValueError, match="optimizer"):
        tfimm.LinearProbe(64, 5, optimizer="adam").load_state_dict(sd)

    model = tfimm.create_model("vit_hd80_test_model")
    before = {k: v.copy() for k, v in model.weights.items()}
    probe = tfimm.LinearProbe.for_model(model, optimizer="adam", lr=0.01)
    assert (probe.dim, probe.nb_classes) == (160, model.cfg.nb_classes) == (160, 10)
    assert np.array_equal(probe.weights["kernel"], model.weights["head/kernel"])
    with pytest.raises(ValueError, match="nb_classes"):
        tfimm.LinearProbe(probe.dim, 9).install(model)
    with pytest.raises(ValueError, match="install"):
        tfimm.LinearProbe(probe.dim + 8, 10).install(model)
    assert all(np.array_equal(model.weights[k], v) for k, v in before.items())
    fitted = tfimm.LinearProbe(probe.dim, 10, seed=5)
    fitted.install(model)
    assert np.array_equal(model.weights["head/kernel"], fitted.weights["kernel"])
    assert all(np.array_equal(model.weights[k], v) for k, v in before.items() if not k.startswith("head/"))
    res = tfimm.create_model("resnet50_mini_test_model")
    assert tfimm.LinearProbe.for_model(res).weights["kernel"].shape == res.weights["remove/fc/kernel"].shape == (128, 10)
    with pytest.raises(ValueError, match="no classifier"):
        tfimm.LinearProbe.for_model(tfimm.create_model("vit_hd80_test_model", nb_classes=0))
    with pytest.raises(ValueError, match="dim = 4"):                              # a feature width the launch does not take
        tfimm.LinearProbe.for_model(tfimm.create_model("vit_test_model"))
    with pytest.raises(ValueError, match="2 heads"):
        tfimm.LinearProbe.for_model(tfimm.create_model("deit_test_model"))

"""pytest -m gpu: the head fit on the device.  tfimm_hip_softmax_grad and tfimm_hip_head_update (csrc/head_fit.hip) against
the written rule of tests/head_fit_ref.py -- bit for bit where the data make every sum exact, under bars derived from the
shape otherwise -- and ``tfimm.LinearProbe`` / ``Model.fit_head`` on top of them."""
import ctypes as C

import numpy as np
import pytest
import torch

import head_fit_ref as hr
import model_checks as mc
import test_architectures  # noqa: F401
import tfimm
from test_gpu_score import _placed_labels, prob_bar
from tfimm.engine import ffi
from tfimm.train.linear_probe import step_scalars
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
U = 2.0 ** -24                      # unit roundoff of float32
NAN32, NAN16 = 0x7FC00BAD, 0x7FC5   # what padding and guard elements hold: NaNs with a payload of their own
GUARD = 8


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf:
    """A matrix [rows][ld] of 2- or 4-byte elements on the device with one guard row behind it; the valid part [rows][cols]
    holds ``a``, everything else ``fill``.  ``after()`` returns the valid part's bits and asserts that nothing else changed."""

    def __init__(self, a, ld, bits, fill):
        a = np.asarray(a)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        self.rows, self.cols = a.shape
        self.ut, self.it = (np.uint16, np.int16) if bits == 16 else (np.uint32, np.int32)
        self.host = np.full((self.rows + 1, ld), fill, self.ut)
        self.host[:self.rows, :self.cols] = hr.bf16_bits(a) if bits == 16 else np.ascontiguousarray(a, f32).view(np.uint32)
        self.dev = torch.from_numpy(self.host.view(self.it)).cuda()
        assert self.dev.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.dev.data_ptr()

    def after(self, what=""):
        now = self.dev.cpu().numpy().view(self.ut)
        keep = np.ones(now.shape, bool)
        keep[:self.rows, :self.cols] = False
        assert np.array_equal(now[keep], self.host[keep]), f"{what}: the launch wrote padding or the guard row"
        return now[:self.rows, :self.cols]


def bits32(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- softmax_grad --------------------------------------------------------------------------------------------------------------
def softmax_grad(x, labels, pad=3):
    """tfimm_hip_softmax_grad and tfimm_hip_score on the same device buffer (ld = N + pad, NaN in the padding columns and
    behind the rows).  Returns (grad as float64 values, loss, pred, score's loss, score's pred)."""
    x = np.ascontiguousarray(x, f32)
    B, N = x.shape
    xb = Buf(x, N + pad, 32, NAN32)
    ldg = (N + 7) // 8 * 8 + 8
    g = Buf(np.zeros((B, N)), ldg, 16, NAN16)
    g.dev.fill_(int(np.array(NAN16, np.uint16).view(np.int16)))               # the valid part too: it must be written
    y = torch.from_numpy(np.asarray(labels, np.int64).astype(np.int32)).cuda()
    outs = [torch.full((B + GUARD,), -7, dtype=dt, device="cuda") for dt in (torch.float32, torch.int32)]
    ffi.check(ffi.lib.tfimm_hip_softmax_grad(xb.ptr, N + pad, B, N, y.data_ptr(), g.ptr, ldg, outs[0].data_ptr(), outs[1].data_ptr(),
                                             _stream()), "tfimm_hip_softmax_grad")
    sc = [torch.full((B + GUARD,), -7, dtype=dt, device="cuda") for dt in (torch.float32, torch.int32, torch.int32, torch.float32)]
    ffi.check(ffi.lib.tfimm_hip_score(xb.ptr, N + pad, B, N, y.data_ptr(), *(t.data_ptr() for t in sc), None, None, None, _stream()),
              "tfimm_hip_score")
    torch.cuda.synchronize()
    res = []
    for t in outs + [sc[0], sc[2]]:
        a = t.cpu().numpy()
        assert (a[B:] == -7).all(), "the launch wrote behind an output"
        res.append(a[:B])
    g.host[:B, :N] = g.after("grad")                                             # (the valid part is what was written)
    grad = g.host[:B, :N]
    assert not (grad == NAN16).any(), "a column of [0, N) was not written"
    xb.after("logits")
    return hr.bits_to_f32(grad).astype(f64), grad, res[0], res[1], res[2], res[3]


SG_SHAPES = [(3, 1000), (1, 1), (2, 37), (2, 257), (1, 32768)]


@pytest.mark.parametrize("B, N", SG_SHAPES)
def test_softmax_grad_rows_loss_and_pred(B, N):
    """grad within one bf16 rounding (2^-8 relative: half a unit of 8 significant bits) of the float64 p - onehot, widened
    by what the float32 row can be off: p's relative bar of tests/test_gpu_score.py and the rounding of the subtraction;
    loss and pred carry tfimm_hip_score's bits; rows that are not scored are +0.0"""
    x = np.random.default_rng(N + B).uniform(-8, 8, (B, N)).astype(f32)
    sets = _placed_labels(x)
    for v in (-1, -2, N):
        sets.append([v] + sets[len(sets) % 5][1:])
    sets.append([(-1, -2, N)[b % 3] for b in range(B)])
    worst = 0.0
    for labels in sets:
        got, raw, loss, pred, s_loss, s_pred = softmax_grad(x, labels)
        assert np.array_equal(bits32(loss), bits32(s_loss)) and np.array_equal(pred, s_pred)
        ok = hr.scored(labels, N)
        assert not raw[~ok].any(), "a row that is not scored must be +0.0 in every column"
        want = hr.p_minus_onehot(x, labels)
        p = hr.softmax64(x)
        bar = 2.0 ** -8 * np.abs(want) + (1 + 2.0 ** -8) * (prob_bar(N) * p + U * np.abs(want))
        err = np.abs(got - want)
        worst = max(worst, float((err[ok] / bar[ok]).max()) if ok.any() else 0.0)
        assert (err[ok] <= bar[ok]).all(), (labels, float((err[ok] / bar[ok]).max()))
        assert (loss[ok] >= 0).all()
    print(f"softmax_grad B={B} N={N}: worst error / bar {worst:.3f}")


def test_softmax_grad_is_reproducible_and_rows_do_not_depend_on_the_batch():
    x = np.random.default_rng(3).integers(-2, 3, (9, 70)).astype(f32)
    labels = [0, 69, -1, 5, 70, 33, 1, 2, 3]
    a, b = softmax_grad(x, labels), softmax_grad(x, labels)
    assert all(np.array_equal(u, v) for u, v in zip(a[1:4], b[1:4]))
    for r in (0, 4, 8):
        one = softmax_grad(x[r:r + 1], labels[r:r + 1])
        assert np.array_equal(one[1][0], a[1][r]) and bits32(one[2])[0] == bits32(a[2])[r]


# ---- head_update ---------------------------------------------------------------------------------------------------------------
def head_update(f, g, labels, st, opt, sc, want_grad=True, pads=(8, 8, 4, 8)):
    """tfimm_hip_head_update on padded buffers: NaN in every input's padding columns and behind row B, sentinels in the
    outputs' padding and guard rows (``Buf``).  ``st``: dict of float32 arrays w (C, D), s1, s2, bias, bias_s1, bias_s2.
    Returns the same dict after the step plus w16 (bits), grad_out and bias_grad_out."""
    B, D = f.shape
    Cn = g.shape[1]
    ldf, ldg, ldw, ldw16 = D + pads[0], (Cn + 7) // 8 * 8 + pads[1], D + pads[2], D + pads[3]
    fb, gb = Buf(f, ldf, 16, NAN16), Buf(g, ldg, 16, NAN16)
    bufs = {k: Buf(st[k], ldw if st[k].ndim == 2 else Cn + 3, 32, NAN32) for k in ("w", "s1", "s2", "bias", "bias_s1", "bias_s2")}
    bufs["w16"] = Buf(np.zeros((Cn, D)), ldw16, 16, NAN16)
    bufs["grad_out"] = Buf(np.zeros((Cn, D)), ldw, 32, NAN32)
    bufs["bias_grad_out"] = Buf(np.zeros(Cn), Cn + 3, 32, NAN32)
    y = torch.from_numpy(np.asarray(labels, np.int64).astype(np.int32)).cuda()
    d = ffi.HeadUpdateDesc()
    d.f, d.g, d.labels = fb.ptr, gb.ptr, y.data_ptr()
    for k, b in bufs.items():
        setattr(d, k, b.ptr)
    if not want_grad:
        d.grad_out = d.bias_grad_out = None
    if opt == hr.SGD:
        d.s2 = d.bias_s2 = None
    d.B, d.D, d.C = B, D, Cn
    d.ldf, d.ldg, d.ldw, d.ldw16 = ldf, ldg, ldw, ldw16
    d.opt = opt
    d.lr, d.mom_or_one_minus_b1, d.one_minus_b2, d.eps, d.wd2 = (float(v) for v in sc)
    ffi.check(ffi.lib.tfimm_hip_head_update(C.byref(d), _stream()), "tfimm_hip_head_update")
    torch.cuda.synchronize()
    fb.after("f"), gb.after("g")
    out = {}
    for k, b in bufs.items():
        a = b.after(k)
        out[k] = a if k == "w16" else a.view(f32).ravel() if k.startswith("bias") else a.view(f32)
    return out


def _state(rng, Cn, D):
    return {"w": rng.normal(0, 0.3, (Cn, D)).astype(f32), "s1": rng.normal(0, 0.1, (Cn, D)).astype(f32),
            "s2": rng.uniform(0, 0.2, (Cn, D)).astype(f32), "bias": rng.normal(0, 0.3, Cn).astype(f32),
            "bias_s1": rng.normal(0, 0.1, Cn).astype(f32), "bias_s2": rng.uniform(0, 0.2, Cn).astype(f32)}


def _labels_with_holes(rng, B, Cn):
    y = rng.integers(0, Cn, B)
    y[rng.random(B) < 0.2] = -1
    if B > 2:
        y[1] = Cn                                                    # out of range: not counted either
    return y


OPTS = [("sgd", 0.0, 1), ("sgd", 0.9, 1), ("adam", 0.9, 1), ("adam", 0.9, 7)]
HU_SHAPES = [(1, 8, 1), (17, 72, 5), (64, 128, 33), (130, 136, 70), (16, 8192, 3)]


def _same_bits(got, want, opt, what):
    for k in ("w", "s1", "bias", "bias_s1", "grad_out", "bias_grad_out") + (("s2", "bias_s2") if opt == hr.ADAM else ()):
        a, b = bits32(got[k]).ravel(), bits32(want[k]).ravel()
        assert np.array_equal(a, b), f"{what}: {k} differs in {(a != b).sum()} of {a.size} elements"
    assert np.array_equal(got["w16"], hr.bf16_bits(want["w"])), f"{what}: w16"


@pytest.mark.parametrize("B, D, Cn", HU_SHAPES)
def test_head_update_is_bit_equal_to_the_float32_restatement_on_exact_data(B, D, Cn):
    """f integers in [-4, 4], g multiples of 1/8 in [-1, 1]: every partial sum is a multiple of 1/8 below 2^12, exact in
    float32 in any order -- so everything behind acc must agree with numpy's float32 operations bit for bit"""
    rng = np.random.default_rng(B * 7 + Cn)
    f = rng.integers(-4, 5, (B, D)).astype(f64)
    g = rng.integers(-8, 9, (B, Cn)).astype(f64) / 8
    labels = _labels_with_holes(rng, B, Cn)
    for name, mom, t in OPTS:
        opt = hr.ADAM if name == "adam" else hr.SGD
        sc = step_scalars(name, 0.05, (mom, 0.999), 1e-7, 0.01, t)
        st = _state(rng, Cn, D)
        got = head_update(f, g, labels, st, opt, sc)
        want = hr.head_update(f, g, labels, st["w"], st["s1"], st["s2"], st["bias"], st["bias_s1"], st["bias_s2"], opt, sc)
        _same_bits(got, want, opt, f"{name} mom={mom} t={t}")
        if opt == hr.SGD:                                            # s2 is not an operand of sgd: untouched
            assert np.array_equal(bits32(got["s2"]), bits32(st["s2"]))
    plain = head_update(f, g, labels, st, opt, sc, want_grad=False, pads=(0, 0, 0, 0))      # no optional outputs, tight pitches
    assert np.array_equal(bits32(plain["w"]), bits32(got["w"])) and (bits32(plain["grad_out"]) == 0).all()


def grad_bar(f, g, labels):
    """|device gd - float64 gd| per element: a float32 sum of B products in ANY order is off by at most (B - 1) u of
    sum |g f| to first order; B + 2 covers the second-order terms (B u < 2^-8) and the multiplication by inv_n and its own
    rounding; the factor 2 admits an accumulator that rounds toward zero (twice the error of round to nearest)."""
    B = f.shape[0]
    n = max(int(hr.scored(labels, g.shape[1]).sum()), 1)
    return 2.0 * (B + 2) * U / n * (np.abs(g).T @ np.abs(f)), n


RANDOM_SHAPES = HU_SHAPES + [(256, 768, 1000)]


@pytest.mark.parametrize("B, D, Cn", RANDOM_SHAPES)
def test_head_update_gradient_on_random_data_against_float64(B, D, Cn):
    rng = np.random.default_rng(B + D + Cn)
    f = hr.bf16_rne(rng.normal(0, 1, (B, D)))
    g = hr.bf16_rne(rng.uniform(-1, 1, (B, Cn)))
    labels = _labels_with_holes(rng, B, Cn)
    bar, n = grad_bar(f, g, labels)
    want = g.T @ f / n
    # the bar can tell a wrong sum from a right one: on the reference alone, a batch row left out moves > 95 % of the elements past it
    r = B // 2
    moved = np.abs(np.outer(g[r], f[r])) / n > bar
    print(f"head_update B={B} D={D} C={Cn}: dropping row {r} moves {100 * moved.mean():.1f} % of the elements past the bar")
    assert moved.mean() > 0.95
    st = _state(rng, Cn, D)
    got = head_update(f, g, labels, st, hr.SGD, step_scalars("sgd", 0.1, (0.9, 0.999), 1e-7, 1e-4, 1))
    err = np.abs(got["grad_out"].astype(f64) - want)
    print(f"    max error / bar {float((err / bar).max()):.4f}")
    assert (err <= bar).all()
    errb = np.abs(got["bias_grad_out"].astype(f64) - g.sum(axis=0) / n)
    assert (errb <= 2.0 * (B + 2) * U / n * np.abs(g).sum(axis=0)).all()


def test_an_all_ignored_batch_moves_the_weights_by_weight_decay_alone():
    rng = np.random.default_rng(11)
    B, D, Cn = 5, 40, 7
    x = rng.uniform(-3, 3, (B, Cn)).astype(f32)
    labels = [-1, -1, Cn, -2, -1]
    g = softmax_grad(x, labels)[0]
    assert not g.any()
    f = hr.bf16_rne(rng.normal(0, 1, (B, D)))
    for name in ("sgd", "adam"):
        opt = hr.ADAM if name == "adam" else hr.SGD
        sc = step_scalars(name, 0.1, (0.9, 0.999), 1e-7, 0.05, 2)
        st = _state(rng, Cn, D)
        got = head_update(f, g, labels, st, opt, sc)
        assert (bits32(got["grad_out"]) == 0).all() and (bits32(got["bias_grad_out"]) == 0).all()
        want = hr.head_update(f, g, labels, st["w"], st["s1"], st["s2"], st["bias"], st["bias_s1"], st["bias_s2"], opt, sc)
        _same_bits(got, want, opt, name)
        assert np.isfinite(got["w"]).all() and not np.array_equal(got["w"], st["w"])


# ---- LinearProbe -------------------------------------------------------------------------------------------------------------
def _prototype_rows(seed=0, Cn=5, D=64, rows=320):
    rng = np.random.default_rng(seed)
    protos = rng.normal(0, 1, (Cn, D))
    y = np.arange(rows) % Cn
    rng.shuffle(y)
    return (0.25 * (protos[y] + rng.normal(0, 1, (rows, D)))).astype(f32), y


@pytest.mark.parametrize("name, lr", [("sgd", 0.1), ("adam", 0.01)])
def test_trajectory_stays_within_the_freedom_of_the_contract(name, lr):
    """Six epochs over 320 prototype-plus-noise rows in batches of 64 (30 steps), weight_decay 1e-4.  The float64 reference
    runs twice: as written, and with every bf16 rounding replaced by truncation -- a perturbation of the size of the freedom
    the contract leaves, made systematic.  The device must stay within twice the distance between the two, and that bar
    must be below 2 % of rms(W).

    Measured, max |W - W_ref| over the kernel: truncating reference 1.04e-3 (sgd) / 2.22e-3 (adam) against rms(W_ref) = 0.389 /
    0.270; the device 2.8e-7 (sgd) / 1.4e-7 (adam)."""
    Cn, D = 5, 64
    x, y = _prototype_rows()
    opt = hr.ADAM if name == "adam" else hr.SGD
    probe = tfimm.LinearProbe(D, Cn, optimizer=name, lr=lr, weight_decay=1e-4, seed=0)
    w0 = probe.weights
    batches = [(x[i:i + 64], y[i:i + 64]) for _ in range(6) for i in range(0, 320, 64)]
    ref = hr.run(w0["kernel"], w0["bias"], batches, opt, lr, (0.9, 0.999), 1e-7, 1e-4)
    trunc = hr.run(w0["kernel"], w0["bias"], batches, opt, lr, (0.9, 0.999), 1e-7, 1e-4, rnd=hr.bf16_trunc)
    dist = float(np.abs(ref["w"] - trunc["w"]).max())
    rms = float(np.sqrt((ref["w"] ** 2).mean()))
    for f, lab in batches:
        probe.step(f, lab)
    w = probe.weights
    dev = float(np.abs(w["kernel"].T.astype(f64) - ref["w"]).max())
    print(f"trajectory {name}: truncating reference {dist:.3g}, device {dev:.3g}, rms(W_ref) {rms:.3g}")
    assert 2 * dist < 0.02 * rms
    assert dev <= 2 * dist
    assert np.abs(w["bias"].astype(f64) - ref["bias"]).max() <= 2 * max(dist, float(np.abs(ref["bias"] - trunc["bias"]).max()))
    ref_pred = (hr.bf16_rne(x) @ hr.bf16_rne(ref["w"]).T + ref["bias"]).argmax(axis=1)
    assert (ref_pred == y).mean() == 1.0
    assert (probe(x).numpy().argmax(axis=1) == y).mean() == 1.0
    assert probe.step_count == 30


def _bits_of_state(sd):
    return {k: bits32(v) for k, v in sd.items() if k not in ("step", "optimizer")}


@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_state_dict_round_trip_and_two_runs_are_bit_equal(name):
    x, y = _prototype_rows(seed=1, rows=192)
    y[::7] = -1
    kw = dict(optimizer=name, lr=(lambda step: 0.05 / (1 + step)), weight_decay=1e-3, seed=2)
    batches = [(x[i:i + 48], y[i:i + 48]) for i in range(0, 192, 48)] * 2

    def run(stop=None):
        p = tfimm.LinearProbe(64, 5, **kw)
        res = None
        for i, (f, lab) in enumerate(batches):
            if i == stop:
                q = tfimm.LinearProbe(64, 5, **kw)
                q.load_state_dict(p.state_dict())
                p = q
            res = p.step(torch.from_numpy(f).cuda() if i % 2 else f, lab)
        return p, res
    (a, ra), (b, rb), (c, rc) = run(), run(), run(stop=3)
    sa = _bits_of_state(a.state_dict())
    assert a.step_count == b.step_count == c.step_count == 8
    for other in (b, c):
        so = _bits_of_state(other.state_dict())
        assert all(np.array_equal(sa[k], so[k]) for k in sa)
    assert np.array_equal(bits32(ra.loss.numpy()), bits32(rc.loss.numpy())) and np.array_equal(ra.pred.numpy(), rc.pred.numpy())
    assert ra.loss.shape == (48,) and ra.pred.numpy().dtype == np.int32 and ra.loss.numpy()[y[144:192] == -1].max() == 0
    assert sa["s1"].any() and (sa["s2"].any() == (name == "adam"))
    # bf16 features give what their float32 values give
    p1, p2 = tfimm.LinearProbe(64, 5, **kw), tfimm.LinearProbe(64, 5, **kw)
    xb = torch.from_numpy(x[:48]).to(torch.bfloat16)
    p1.step(xb, y[:48])
    p2.step(tfimm.Tensor(xb.float().cuda()), torch.from_numpy(y[:48]).cuda())
    assert np.array_equal(bits32(p1.weights["kernel"]), bits32(p2.weights["kernel"]))
    e = p1.step(np.zeros((0, 64), f32), np.zeros(0, np.int64))                   # an empty batch is no step
    assert e.loss.shape == (0,) and p1.step_count == 1
    assert tfimm.LinearProbe(64, 5)(np.zeros((0, 64), f32)).shape == (0, 5)       # ... on a probe that has allocated nothing yet, too


def _model(name):
    model = tfimm.create_model(name)
    model.set_weights(synthetic_weights(model, 2021))
    return model


@pytest.mark.parametrize("name", ["vit_hd80_test_model", "resnet50_mini_test_model"])
def test_fit_head_lowers_the_loss_leaves_the_model_alone_and_installs(name):
    model = _model(name)
    B = 8
    x = mc.make_input(model.cfg, B)
    labels = np.arange(B) % model.cfg.nb_classes
    labels[3] = -1
    before = model(x).numpy()
    plans, captured = len(model._plans), len(model._captured)
    probe = tfimm.LinearProbe.for_model(model, optimizer="sgd", lr=0.05)
    losses = []
    for _ in range(20):
        r = model.fit_head(x, labels, probe)
        losses.append(float(r.loss.numpy()[labels >= 0].mean()))
    print(f"fit_head {name}: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] < losses[0] and probe.step_count == 20 and r.loss.numpy()[3] == 0
    # the first step's loss is the model's own evaluate: same features, same head
    assert abs(losses[0] - float(model.evaluate(x, labels).loss.numpy()[labels >= 0].mean())) < 1e-3
    # the model was not touched: same bits, no program dropped
    assert np.array_equal(bits32(model(x).numpy()), bits32(before))
    assert len(model._captured) >= captured and len(model._plans) >= plans
    # after install the model's logits are the probe's, bit for bit
    f = model._head_input(x)                                          # ResNet: the map averaged over H and W
    assert f.shape == (B, probe.dim)
    probe.install(model)
    after = model(x).numpy()
    assert not np.array_equal(after, before)
    assert np.array_equal(bits32(probe(f).numpy()), bits32(after))


def test_fit_head_refuses_a_model_with_two_heads():
    deit = _model("deit_test_model")
    with pytest.raises(ValueError, match="heads"):
        deit.fit_head(mc.make_input(deit.cfg, 2), [0, 1], tfimm.LinearProbe(8, 12))

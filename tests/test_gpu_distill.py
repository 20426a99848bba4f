"""pytest -m gpu: the distillation of an embedding head on the device.  tfimm_hip_distill_grad (csrc/distill.hip) against the
written rule of tests/distill_ref.py -- under the bars derived there, bit for bit where the data make every operation exact --
and ``tfimm.EmbeddingProbe`` / ``Model.distill_head`` on top of it."""
import numpy as np
import pytest
import torch

import distill_ref as dr
import head_fit_ref as hr
import model_checks as mc
import test_architectures  # noqa: F401
import tfimm
from test_gpu_head_fit import GUARD, NAN16, NAN32, Buf, _bits_of_state, _stream, bits32
from tfimm.engine import ffi
from tfimm.train._head_probe import step_scalars
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def distill_grad(s, t, valid, normalize, pad=4):
    """tfimm_hip_distill_grad on padded buffers: ld_s = ceil4(E) + pad, ld_t one piece wider, NaN behind column E and behind
    row B of both inputs, NaN sentinels in ALL of grad (its valid part must be written, nothing else may be), -7 behind loss
    and cosine.  ``pad`` = 4 keeps the rows 16-byte aligned (vector loads), 5 does not.
    Returns (grad bits (B, E) uint16, loss (B,), cosine (B,))."""
    s, t = np.ascontiguousarray(s, f32), np.ascontiguousarray(t, f32)
    B, E = s.shape
    ld_s = (E + 3) // 4 * 4 + pad
    ld_t = ld_s + 4
    ldg = (E + 7) // 8 * 8 + 8
    sb, tb = Buf(s, ld_s, 32, NAN32), Buf(t, ld_t, 32, NAN32)
    g = Buf(np.zeros((B, E)), ldg, 16, NAN16)
    g.dev.fill_(int(np.array(NAN16, np.uint16).view(np.int16)))
    y = torch.from_numpy(np.asarray(valid, np.int64).astype(np.int32)).cuda()
    outs = [torch.full((B + GUARD,), -7, dtype=torch.float32, device="cuda") for _ in range(2)]
    ffi.check(ffi.lib.tfimm_hip_distill_grad(sb.ptr, ld_s, tb.ptr, ld_t, B, E, y.data_ptr(), int(normalize), g.ptr, ldg,
                                             outs[0].data_ptr(), outs[1].data_ptr(), _stream()), "tfimm_hip_distill_grad")
    torch.cuda.synchronize()
    res = []
    for o in outs:
        a = o.cpu().numpy()
        assert (a[B:] == -7).all(), "the launch wrote behind an output"
        res.append(a[:B])
    sb.after("s"), tb.after("t")
    g.host[:B, :E] = g.after("grad")                            # (the valid part is what was written)
    grad = g.host[:B, :E].copy()
    assert not (grad == NAN16).any(), "a column of [0, E) was not written"
    return grad, res[0], res[1]


def _cases(B, E, seed):
    """(s, t, valid): random rows of scales 1e-2 .. 1e2 with every third row ignored; a row with s == t; a row with s == -t"""
    rng = np.random.default_rng(seed)
    s = (rng.normal(0, 1, (B, E)) * 10.0 ** rng.uniform(-2, 2, (B, 1))).astype(f32)
    t = rng.normal(0, 0.7, (B, E)).astype(f32)
    all_valid = np.zeros(B, np.int64)
    same, opposite = t.copy(), t.copy()
    same[0] = s[0]
    opposite[B - 1] = -s[B - 1]
    return [("random", s, t, np.where(np.arange(B) % 3 == 1, -1, 0)), ("s == t", s, same, all_valid),
            ("s == -t", s, opposite, all_valid)]


ROW_SHAPES = [(1, 1), (3, 7), (5, 8), (4, 64), (2, 65), (3, 129), (2, 1000), (2, 2048), (1, 4096), (70, 16)]


@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("B, E", ROW_SHAPES)
def test_rows_against_float64(B, E, normalize):
    """The bars of tests/distill_ref.py (derived there, L = E / 64):
        gradient  |g - g64| <= h(g64) + 2 inv_s (L + 8) 2^-23           (inv_s = 1 for normalize = 0)
        loss, cosine        <= (L + 8) 2^-23 max(1, |value|)
    h(g) = 2^(floor(log2 |g|) - 8) is half a unit in the last place of bf16, between 2^-9 |g| and 2^-8 |g|.  (With 2^-9 |g64|
    in its place -- half a unit of nine bits -- the bf16 rounding alone is up to twice the bar: measured 1.48 at (1, 1),
    normalize = 0, where the rounding is the only error.)
    on lane tails, an odd last column, the largest E and a ragged last workgroup; padding and ignored rows are looked at by
    ``distill_grad``; aligned rows (vector loads) and unaligned ones give the same bits."""
    unit = (E / 64 + 8) * 2.0 ** -23
    worst = [0.0, 0.0, 0.0]
    for what, s, t, valid in _cases(B, E, 100 * E + B):
        grad, loss, cos = distill_grad(s, t, valid, normalize)
        other = distill_grad(s, t, valid, normalize, pad=5)
        assert all(np.array_equal(bits32(a) if a.dtype == f32 else a, bits32(b) if b.dtype == f32 else b)
                   for a, b in zip((grad, loss, cos), other)), f"{what}: the bits depend on the alignment of the rows"
        ok = dr.trained(valid)
        assert not grad[~ok].any() and not bits32(loss)[~ok].any() and not bits32(cos)[~ok].any(), f"{what}: an ignored row must be +0.0"
        g64, loss64, cos64 = dr.rows(s, t, valid, bool(normalize))
        inv_s = dr.l2_normalize(s)[1] if normalize else np.ones(B)
        bar = dr.half_ulp_bf16(g64) + (2 * inv_s * unit)[:, None]
        errs = (np.abs(hr.bits_to_f32(grad).astype(f64) - g64) / bar, np.abs(loss.astype(f64) - loss64) / (unit * np.maximum(1, np.abs(loss64))),
                np.abs(cos.astype(f64) - cos64) / unit)
        for i, e in enumerate(errs):
            worst[i] = max(worst[i], float(e[ok].max()) if ok.any() else 0.0)
        print(f"distill_grad B={B} E={E} normalize={normalize} {what}: error / bar  grad {errs[0][ok].max():.3f}  "
              f"loss {errs[1][ok].max():.3f}  cosine {errs[2][ok].max():.3f}")
        assert all((e[ok] <= 1).all() for e in errs), (what, [float(e[ok].max()) for e in errs])
        if what == "s == t":
            assert loss[0] == 0, "u == v bit for bit: the loss of a row with s == t is exactly zero"
        if what == "s == -t" and normalize:
            assert abs(loss[B - 1] - 4) <= 4 * unit and abs(cos[B - 1] + 1) <= unit
    print(f"distill_grad B={B} E={E} normalize={normalize}: worst error / bar  grad {worst[0]:.3f}  loss {worst[1]:.3f}  cosine {worst[2]:.3f}")


def test_the_clamp_branch_on_the_device():
    """rows of 1e-8s (sum s^2 = E * 1e-16 < 1e-12): inv_s = 1e6, the gradient is 2e6 (u - v)"""
    E = 40
    s = np.full((2, E), 1e-8, f32)
    s[1, ::2] = -1e-8
    t = np.random.default_rng(2).normal(0, 1, (2, E)).astype(f32)
    grad, loss, cos = distill_grad(s, t, [0, 0], 1)
    g64, loss64, cos64 = dr.rows(s, t, [0, 0], True)
    assert np.allclose(g64, 2e6 * (s.astype(f64) * 1e6 - dr.l2_normalize(t)[0]), rtol=1e-12)
    unit = (E / 64 + 8) * 2.0 ** -23
    assert (np.abs(hr.bits_to_f32(grad).astype(f64) - g64) <= dr.half_ulp_bf16(g64) + 2e6 * unit).all()
    assert (np.abs(loss - loss64) <= unit * np.maximum(1, loss64)).all() and (np.abs(cos - cos64) <= unit).all()


def test_exact_data_is_bit_equal():
    """normalize = 0, s and t integers over 8 in [-2, 2]: 2 (s - t) is a multiple of 1/4 below 8 (a bf16 value), every
    partial sum of (s - t)^2 a multiple of 1/64 below 2^12: the gradient's bits and the loss must be the reference's"""
    rng = np.random.default_rng(9)
    B, E = 6, 129
    s, t = rng.integers(-16, 17, (B, E)) / 8, rng.integers(-16, 17, (B, E)) / 8
    valid = [0, 0, -1, 0, 0, 0]
    grad, loss, cos = distill_grad(s, t, valid, 0)
    g64, loss64, _ = dr.rows(s, t, valid, False)
    assert np.array_equal(grad, hr.bf16_bits(g64)) and np.array_equal(hr.bits_to_f32(grad).astype(f64), g64)
    assert np.array_equal(bits32(loss), bits32(loss64.astype(f32))) and loss64.max() < 2 ** 12


def test_two_launches_agree_and_rows_do_not_depend_on_the_batch():
    _, s, t, valid = _cases(70, 16, 1)[0]
    for normalize in (1, 0):
        a, b = distill_grad(s, t, valid, normalize), distill_grad(s, t, valid, normalize)
        assert all(np.array_equal(u.view(np.uint32) if u.dtype == f32 else u, v.view(np.uint32) if v.dtype == f32 else v)
                   for u, v in zip(a, b))
        for r in (0, 3, 33, 68, 69):                             # first and last wave of a workgroup, the ragged last one
            one = distill_grad(s[r:r + 1], t[r:r + 1], valid[r:r + 1], normalize)
            assert np.array_equal(one[0][0], a[0][r]) and bits32(one[1])[0] == bits32(a[1])[r] and bits32(one[2])[0] == bits32(a[2])[r]
            assert valid[r] == 0 and a[0][r].any()


# ---- EmbeddingProbe ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, t_step", [("sgd", 1), ("adam", 1), ("adam", 7)])
@pytest.mark.parametrize("B, D, E", [(5, 64, 8), (130, 72, 24)])
def test_one_step_is_bit_equal_to_the_float32_restatement_on_exact_data(B, D, E, name, t_step):
    """normalize_embeddings = False.  f integers in [-4, 4], W multiples of 1/4 in [-1/2, 1/2], bias multiples of 1/4: the
    student s = f . W + b is a sum of multiples of 1/4 below 2^10, exact in float32 in any order.  The teacher is s - g / 2
    for a chosen g of multiples of 1/8 in [-1, 1]: the device's 2 (s - t) is g exactly, a bf16 value, and g^T f is exact as in
    tests/test_gpu_head_fit.py -- so weights and slots must agree with numpy's float32 operations bit for bit, under the
    distillation weight-decay scalar."""
    rng = np.random.default_rng(B + E + t_step)
    f = rng.integers(-4, 5, (B, D)).astype(f64)
    w = rng.integers(-2, 3, (E, D)) / 4
    bias = rng.integers(-4, 5, E) / 4
    g = rng.integers(-8, 9, (B, E)) / 8
    valid = np.where(rng.random(B) < 0.2, -1, 0)
    valid[0] = 0
    s = f @ w.T + bias
    t = s - g / 2
    assert np.array_equal(t.astype(f32).astype(f64), t)
    st = {"w": w.astype(f32), "bias": bias.astype(f32)}
    for k, like, lo, hi in (("s1", w, -0.1, 0.1), ("s2", w, 0, 0.2), ("bias_s1", bias, -0.1, 0.1), ("bias_s2", bias, 0, 0.2)):
        st[k] = (rng.uniform(lo, hi, like.shape) if t_step > 1 else np.zeros(like.shape)).astype(f32)
    probe = tfimm.EmbeddingProbe(D, E, normalize_embeddings=False, optimizer=name, lr=0.05, weight_decay=0.01)
    probe.load_state_dict({"kernel": st["w"].T, "s1": st["s1"].T, "s2": st["s2"].T, "bias": st["bias"], "bias_s1": st["bias_s1"],
                           "bias_s2": st["bias_s2"], "step": t_step - 1, "optimizer": name})
    res = probe.step(f.astype(f32), t.astype(f32), valid == 0)
    sc = step_scalars(name, 0.05, (0.9, 0.999), 1e-7, 0.01 / (D * E + E), t_step)
    assert sc[4] == f32(dr.wd2(D, E, 0.01))
    opt = hr.ADAM if name == "adam" else hr.SGD
    gm = np.where((valid == 0)[:, None], g, 0.0)
    want = hr.head_update(f, gm, valid, st["w"], st["s1"], st["s2"], st["bias"], st["bias_s1"], st["bias_s2"], opt, sc)
    got = probe.state_dict()
    for k, wk in (("kernel", "w"), ("s1", "s1"), ("bias", "bias"), ("bias_s1", "bias_s1")) + ((("s2", "s2"), ("bias_s2", "bias_s2")) if opt == hr.ADAM else ()):
        a = bits32(got[k].T if got[k].ndim == 2 else got[k]).ravel()
        b = bits32(want[wk]).ravel()
        assert np.array_equal(a, b), f"{k} differs in {(a != b).sum()} of {a.size} elements"
    assert not np.array_equal(got["kernel"].T, st["w"]) and got["step"] == t_step
    # the loss is exact too: sum (g / 2)^2, multiples of 1/256
    assert np.array_equal(bits32(res.loss.numpy()), bits32(((gm / 2) ** 2).sum(axis=1).astype(f32)))
    assert not bits32(res.cosine.numpy())[valid != 0].any()


def _recipe():
    rng = np.random.default_rng(0)
    x = (0.5 * rng.normal(0, 1, (320, 64))).astype(f32)
    a = rng.normal(0, 1, (64, 16)) / 8
    t = (x @ a + 0.05 * rng.normal(0, 1, (320, 16))).astype(f32)
    return x, t, np.where(np.arange(320) % 9 == 8, -1, 0)


@pytest.mark.parametrize("normalize, name, lr, epochs, cap", [(True, "sgd", 0.5, 6, 0.05), (True, "adam", 0.03, 10, 0.05),
                                                             (False, "sgd", 0.02, 6, 0.1)])
def test_trajectory_stays_within_the_freedom_of_the_contract(normalize, name, lr, epochs, cap):
    """D = 64, E = 16, 320 rows x = 0.5 N(0, 1) in batches of 64, teacher = x A + 0.05 N(0, 1) with A = N(0, 1) / 8, every
    ninth row ignored, weight_decay 1e-4.  The float64 reference runs twice: as written, and with every bf16 rounding
    replaced by truncation.  The device must stay within twice the distance between the two, and that bar must be below
    ``cap`` of rms(W).

    The reference alone, 2 * dist / rms(W) and the mean loss of the first and the last step: normalised sgd 0.0109,
    2.02 -> 0.050; normalised adam 0.0135, 2.02 -> 0.022; un-normalised sgd 0.0448, 10.5 -> 0.39.
    Measured, max |W - W_ref| over the kernel, truncating reference / device: 2.35e-3 / 1.2e-4 (normalised sgd), 2.17e-3 /
    2.1e-4 (normalised adam), 2.95e-3 / 3.5e-7 (un-normalised sgd); the device's losses are the reference's to four digits."""
    x, t, valid = _recipe()
    opt = hr.ADAM if name == "adam" else hr.SGD
    probe = tfimm.EmbeddingProbe(64, 16, normalize_embeddings=normalize, optimizer=name, lr=lr, weight_decay=1e-4, seed=0)
    w0 = probe.weights
    batches = [(x[i:i + 64], t[i:i + 64], valid[i:i + 64]) for _ in range(epochs) for i in range(0, 320, 64)]
    ref, ref_loss = dr.run(w0["kernel"], w0["bias"], batches, opt, lr, (0.9, 0.999), 1e-7, 1e-4, normalize)
    trunc, _ = dr.run(w0["kernel"], w0["bias"], batches, opt, lr, (0.9, 0.999), 1e-7, 1e-4, normalize, rnd=hr.bf16_trunc)
    dist = float(np.abs(ref["w"] - trunc["w"]).max())
    rms = float(np.sqrt((ref["w"] ** 2).mean()))
    results = [probe.step(f, tt, v == 0) for f, tt, v in batches]
    mean = [float(r.loss.numpy()[v == 0].mean()) for r, (_, _, v) in ((results[0], batches[0]), (results[-1], batches[-1]))]
    w = probe.weights
    dev = float(np.abs(w["kernel"].T.astype(f64) - ref["w"]).max())
    print(f"trajectory normalize={normalize} {name}: truncating reference {dist:.3g}, device {dev:.3g}, rms(W_ref) {rms:.3g}, "
          f"2 dist / rms {2 * dist / rms:.4f}; device loss {mean[0]:.4f} -> {mean[1]:.4f} (reference {ref_loss[0]:.4f} -> {ref_loss[-1]:.4f})")
    assert 2 * dist < cap * rms
    assert dev <= 2 * dist
    assert np.abs(w["bias"].astype(f64) - ref["bias"]).max() <= 2 * max(dist, float(np.abs(ref["bias"] - trunc["bias"]).max()))
    assert mean[1] < 0.1 * mean[0]
    assert probe.step_count == 5 * epochs


@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_state_dict_round_trip_and_two_runs_are_bit_equal(name):
    x, t, valid = _recipe()
    x, t, valid = x[:192], t[:192], valid[:192]
    kw = dict(optimizer=name, lr=(lambda step: 0.3 / (1 + step)), weight_decay=1e-3, seed=2)
    batches = [(x[i:i + 48], t[i:i + 48], valid[i:i + 48] == 0) for i in range(0, 192, 48)] * 2

    def run(stop=None):
        p = tfimm.EmbeddingProbe(64, 16, **kw)
        res = None
        for i, (f, tt, v) in enumerate(batches):
            if i == stop:
                q = tfimm.EmbeddingProbe(64, 16, **kw)
                q.load_state_dict(p.state_dict())
                p = q
            dev = i % 2 == 1
            res = p.step(torch.from_numpy(f).cuda() if dev else f, torch.from_numpy(tt).cuda() if dev else tt,
                         torch.from_numpy(v).cuda() if dev else v)
        return p, res
    (a, ra), (b, rb), (c, rc) = run(), run(), run(stop=3)
    sa = _bits_of_state(a.state_dict())
    assert a.step_count == b.step_count == c.step_count == 8
    for other in (b, c):
        so = _bits_of_state(other.state_dict())
        assert all(np.array_equal(sa[k], so[k]) for k in sa)
    assert np.array_equal(bits32(ra.loss.numpy()), bits32(rc.loss.numpy())) and np.array_equal(bits32(ra.cosine.numpy()), bits32(rc.cosine.numpy()))
    gone = valid[144:192] != 0
    assert ra.loss.shape == (48,) and ra.cosine.numpy().dtype == f32 and gone.any()
    assert not bits32(ra.loss.numpy())[gone].any() and not bits32(ra.cosine.numpy())[gone].any()
    assert bits32(ra.cosine.numpy())[~gone].all() and (np.abs(ra.cosine.numpy()) <= 1 + 2.0 ** -20).all()
    assert sa["s1"].any() and (sa["s2"].any() == (name == "adam"))
    # bf16 features and a bf16 teacher give what their float32 values give; an integer mask is a boolean one
    p1, p2 = tfimm.EmbeddingProbe(64, 16, **kw), tfimm.EmbeddingProbe(64, 16, **kw)
    xb, tb = torch.from_numpy(x[:48]).to(torch.bfloat16), torch.from_numpy(t[:48]).to(torch.bfloat16)
    p1.step(xb, tb, batches[0][2])
    p2.step(tfimm.Tensor(xb.float().cuda()), tfimm.Tensor(tb.float().cuda()), batches[0][2].astype(np.int64))
    assert np.array_equal(bits32(p1.weights["kernel"]), bits32(p2.weights["kernel"]))
    e = p1.step(np.zeros((0, 64), f32), np.zeros((0, 16), f32))                 # an empty batch is no step
    assert e.loss.shape == (0,) and e.cosine.shape == (0,) and p1.step_count == 1
    assert tfimm.EmbeddingProbe(64, 16)(np.zeros((0, 64), f32)).shape == (0, 16)     # ... on a probe that has allocated nothing yet, too
    # probe(features): raw by default; normalised only if the probe normalises AND the caller asks
    raw, unit = p1(x[:48]).numpy(), p1(x[:48], normalize=True).numpy()
    assert np.abs(np.linalg.norm(raw, axis=1) - 1).max() > 1e-2 and np.abs(np.linalg.norm(unit.astype(f64), axis=1) - 1).max() < 1e-6
    plain = tfimm.EmbeddingProbe(64, 16, normalize_embeddings=False, **kw)
    assert np.array_equal(bits32(plain(x[:48]).numpy()), bits32(plain(x[:48], normalize=True).numpy()))


@pytest.mark.parametrize("name", ["sgd", "adam"])
def test_an_all_invalid_batch_moves_the_weights_by_weight_decay_alone(name):
    x, t, _ = _recipe()
    opt = hr.ADAM if name == "adam" else hr.SGD
    probe = tfimm.EmbeddingProbe(64, 16, optimizer=name, lr=0.1, weight_decay=0.5, seed=3)
    w0 = probe.weights
    res = probe.step(x[:7], t[:7], np.zeros(7, bool))
    assert not bits32(res.loss.numpy()).any() and not bits32(res.cosine.numpy()).any()
    z = lambda a: np.zeros_like(a)                                                    # noqa: E731
    w, b = np.ascontiguousarray(w0["kernel"].T), w0["bias"]
    want = hr.head_update(hr.bf16_rne(x[:7]), np.zeros((7, 16)), [-1] * 7, w, z(w), z(w), b, z(b), z(b), opt,
                          step_scalars(name, 0.1, (0.9, 0.999), 1e-7, 0.5 / (64 * 16 + 16), 1))
    got = probe.weights
    assert np.array_equal(bits32(got["kernel"].T), bits32(want["w"])) and np.array_equal(bits32(got["bias"]), bits32(want["bias"]))
    assert not np.array_equal(got["kernel"], w0["kernel"]) and np.isfinite(got["kernel"]).all() and probe.step_count == 1


# ---- Model.distill_head ------------------------------------------------------------------------------------------------------
def _model(name, seed):
    model = tfimm.create_model(name)
    model.set_weights(synthetic_weights(model, seed))
    return model


def test_distill_head_lowers_the_loss_leaves_the_student_alone_and_installs():
    student = _model("vit_hd80_test_model", 2021)
    teacher = tfimm.EmbeddingModel(_model("vit_hd80_test_model", 7), 16)
    B = 8
    x = mc.make_input(student.cfg, B)
    valid = np.ones(B, bool)
    valid[3] = False
    before = student(x).numpy()
    plans, captured = len(student._plans), len(student._captured)
    target = teacher(x)
    assert target.shape == (B, 16)
    probe = tfimm.EmbeddingProbe(160, 16, optimizer="adam", lr=1e-3)
    losses = []
    for _ in range(20):
        r = student.distill_head(x, target, probe, valid)
        losses.append(float(r.loss.numpy()[valid].mean()))
    print(f"distill_head: loss {losses[0]:.4f} -> {losses[-1]:.4f}, cosine {float(r.cosine.numpy()[valid].mean()):.4f}")
    assert losses[-1] < losses[0] and probe.step_count == 20
    assert bits32(r.loss.numpy())[3] == 0 and bits32(r.cosine.numpy())[3] == 0
    # the student was not touched: same bits, no program dropped
    assert np.array_equal(bits32(student(x).numpy()), bits32(before))
    assert len(student._captured) >= captured and len(student._plans) >= plans
    # after install the embedding model's output is the probe's, bit for bit: the same GEMM on the same bf16 operands
    served = tfimm.EmbeddingModel(student, 16)
    probe.install(served)
    f = student._head_input(x)
    assert f.shape == (B, probe.dim)
    assert np.array_equal(bits32(probe(f).numpy()), bits32(served(x).numpy()))
    # a teacher whose embeddings are a map is refused before any launch
    res = tfimm.EmbeddingModel(_model("resnet50_mini_test_model", 7), 16)
    xr = mc.make_input(res.cfg, 2)
    tmap = res(xr)
    assert len(tmap.shape) == 4 and tmap.shape[-1] == 16
    with pytest.raises(ValueError, match="teacher"):
        student.distill_head(x[:2], tmap, probe)
    assert probe.step_count == 20

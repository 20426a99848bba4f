"""Restatement of the head fit -- one optimizer step of a Dense classifier on frozen features under softmax cross-entropy, the
reference's ``ClassificationProblem`` + ``OptimizerFactory`` restricted to the head -- in plain numpy (test helper): the
single written rule that tfimm_hip_softmax_grad, tfimm_hip_head_update (csrc/head_fit.hip) and ``tfimm.LinearProbe`` are
held to.  Stated twice: in float64 with the bf16 roundings where the contract has them, and, for the update behind the
matrix product, in numpy float32 operation by operation (numpy never fuses a multiply with an add).

Weights are kept as ``w[C][D]``, the head's kernel transposed (the layout of the device's master weights).

    logits = f16 . w16^T + bias                f16 = bf16(f), w16 = bf16(w)
    g[b]   = bf16(softmax(logits[b]) - onehot(y_b))          zeros for a label outside [0, C)
    n      = number of labels in [0, C);  inv_n = 1 / max(n, 1)
    gd     = (g^T . f16) * inv_n ;  gdb = (sum_b g[b]) * inv_n
    gr     = gd + wd2 * w                      wd2 = 2 * weight_decay: d/dw of weight_decay * sum(w^2), kernel and bias alike
    sgd :  s1 = mom * s1 - lr * gr ;  w = w + s1
    adam:  s1 = s1 + (gr - s1) * (1 - b1) ;  s2 = s2 + (gr * gr - s2) * (1 - b2) ;  w = w - (s1 * lr_t) / (sqrt(s2) + eps)
           lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t),  t = 1, 2, ...

Deliberately independent of the engine: nothing here imports tfimm.
"""
import numpy as np

f32, f64 = np.float32, np.float64
SGD, ADAM = 0, 1


# ---- bf16 ------------------------------------------------------------------------------------------------------------------
def bf16_bits(a):
    """float32 -> bf16 bit patterns (uint16), round to nearest even"""
    u = np.ascontiguousarray(a, f32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bits_to_f32(b):
    return (np.asarray(b).astype(np.uint32) << 16).view(f32)


def bf16_rne(a):
    """the nearest bf16 value (ties to even) of every element, as float64.  The input goes through float32 first: every value
    rounded here is one the device holds in float32, or a float64 stand-in for it whose float32 rounding is 2^-16 of a bf16 ulp"""
    return bits_to_f32(bf16_bits(np.asarray(a, f64).astype(f32))).astype(f64)


def bf16_trunc(a):
    """bf16 by truncation (round toward zero): the systematic perturbation of the trajectory test"""
    u = np.ascontiguousarray(np.asarray(a, f64).astype(f32)).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(f32).astype(f64)


# ---- scalars ---------------------------------------------------------------------------------------------------------------
def scalars(opt, lr, betas, eps, weight_decay, t):
    """(lr, mom_or_one_minus_b1, one_minus_b2, eps, wd2) in float64 for step t (1-based)"""
    b1, b2 = float(betas[0]), float(betas[1])
    if opt == ADAM:
        return (float(lr) * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t), 1.0 - b1, 1.0 - b2, float(eps), 2.0 * float(weight_decay))
    return (float(lr), b1, 0.0, float(eps), 2.0 * float(weight_decay))


# ---- the loss and its gradient, float64, no rounding anywhere --------------------------------------------------------------
def scored(labels, C):
    y = np.asarray(labels, np.int64)
    return (y >= 0) & (y < C)


def softmax64(x):
    d = np.asarray(x, f64) - np.asarray(x, f64).max(axis=1, keepdims=True)
    e = np.exp(d)
    return e / e.sum(axis=1, keepdims=True)


def row_losses(x, labels):
    """float64 cross-entropy per row of logits x (B, C); 0 for a row that is not scored"""
    x = np.asarray(x, f64)
    ok = scored(labels, x.shape[1])
    d = x - x.max(axis=1, keepdims=True)
    lse = np.log(np.exp(d).sum(axis=1))
    y = np.where(ok, np.asarray(labels, np.int64), 0)
    return np.where(ok, lse - d[np.arange(len(y)), y], 0.0)


def total_loss(w, bias, f, labels, weight_decay):
    """mean cross-entropy over the scored rows + weight_decay * (sum w^2 + sum bias^2): the reference's loss + reg_loss"""
    w, bias, f = np.asarray(w, f64), np.asarray(bias, f64), np.asarray(f, f64)
    n = max(int(scored(labels, w.shape[0]).sum()), 1)
    return row_losses(f @ w.T + bias, labels).sum() / n + weight_decay * ((w * w).sum() + (bias * bias).sum())


def p_minus_onehot(x, labels):
    """float64 softmax(x) - onehot(labels); zero rows where the label is -1 or outside [0, C)"""
    x = np.asarray(x, f64)
    ok = scored(labels, x.shape[1])
    g = softmax64(x)
    y = np.asarray(labels, np.int64)
    g[np.nonzero(ok)[0], y[ok]] -= 1.0
    g[~ok] = 0.0
    return g


def total_grad(w, bias, f, labels, weight_decay):
    """d total_loss / d (w, bias), float64"""
    w, bias, f = np.asarray(w, f64), np.asarray(bias, f64), np.asarray(f, f64)
    g = p_minus_onehot(f @ w.T + bias, labels)
    n = max(int(scored(labels, w.shape[0]).sum()), 1)
    return g.T @ f / n + 2.0 * weight_decay * w, g.sum(axis=0) / n + 2.0 * weight_decay * bias


# ---- the update behind the matrix product ----------------------------------------------------------------------------------
def _step(opt, acc, inv_n, w, s1, s2, sc, ft):
    """one element-wise optimizer step in the float type ``ft``: every line is one operation per element"""
    lr, m1, m2, eps, wd2 = (ft(v) for v in sc)
    gd = acc * inv_n
    t = wd2 * w
    gr = gd + t
    if opt == SGD:
        a = m1 * s1
        b = lr * gr
        s1 = a - b
        w = w + s1
        return w, s1, s2, gd
    d = gr - s1
    d = d * m1
    s1 = s1 + d
    q = gr * gr
    q = q - s2
    q = q * m2
    s2 = s2 + q
    num = s1 * lr
    den = np.sqrt(s2)
    den = den + eps
    w = w - num / den
    return w, s1, s2, gd


def head_update(f, g, labels, w, s1, s2, bias, bias_s1, bias_s2, opt, sc, ft=f32):
    """tfimm_hip_head_update in the float type ``ft`` (float32: the operation-by-operation restatement, bit-equal to the
    device whenever the sums are exact; float64: the reference).  f (B, D) and g (B, C) hold bf16 values; sc = the five
    scalars.  The sums are formed in float64 and rounded once to ``ft``: exact data makes that the identity.
    Returns a dict: w, s1, s2, bias, bias_s1, bias_s2, w16 (bf16 values, float32), grad_out, bias_grad_out."""
    f, g = np.asarray(f, f64), np.asarray(g, f64)
    C = g.shape[1]
    n = max(int(scored(labels, C).sum()), 1)
    inv_n = ft(1.0) / ft(n)
    acc = (g.T @ f).astype(ft)
    accb = g.sum(axis=0).astype(ft)
    z = lambda a: None if a is None else np.asarray(a, ft)       # noqa: E731
    zero = lambda a, like: np.zeros_like(like) if a is None else a      # noqa: E731
    w, s1, bias, bias_s1 = z(w), z(s1), z(bias), z(bias_s1)
    s2, bias_s2 = zero(z(s2), w), zero(z(bias_s2), bias)
    w_, s1_, s2_, gd = _step(opt, acc, inv_n, w, s1, s2, sc, ft)
    b_, bs1_, bs2_, gdb = _step(opt, accb, inv_n, bias, bias_s1, bias_s2, sc, ft)
    return {"w": w_, "s1": s1_, "s2": s2_, "bias": b_, "bias_s1": bs1_, "bias_s2": bs2_,
            "w16": bits_to_f32(bf16_bits(w_.astype(f32))), "grad_out": gd, "bias_grad_out": gdb}


# ---- a whole step and a run, float64 ---------------------------------------------------------------------------------------
def probe_step(state, f, labels, opt, sc, rnd=bf16_rne):
    """One step of the probe in float64 with ``rnd`` at every place the contract rounds to bf16 (features, shadow weights,
    gradient rows).  ``state``: dict w (C, D), s1, s2, bias, bias_s1, bias_s2 -- replaced in place.  Returns (loss per row,
    pred per row) under the weights before the step."""
    f16 = rnd(f)
    logits = f16 @ rnd(state["w"]).T + state["bias"]
    g = rnd(p_minus_onehot(logits, labels))
    out = head_update(f16, g, labels, state["w"], state["s1"], state["s2"], state["bias"], state["bias_s1"], state["bias_s2"],
                      opt, sc, ft=f64)
    for k in ("w", "s1", "s2", "bias", "bias_s1", "bias_s2"):
        state[k] = out[k]
    return row_losses(logits, labels), logits.argmax(axis=1)


def new_state(kernel, bias):
    """float64 state from a Keras-layout kernel (D, C) and bias (C,), zero slots"""
    w = np.asarray(kernel, f64).T.copy()
    b = np.asarray(bias, f64).copy()
    return {"w": w, "s1": np.zeros_like(w), "s2": np.zeros_like(w), "bias": b, "bias_s1": np.zeros_like(b),
            "bias_s2": np.zeros_like(b)}


def run(kernel, bias, batches, opt, lr, betas, eps, weight_decay, rnd=bf16_rne):
    """``batches``: a sequence of (features, labels); returns the final state"""
    st = new_state(kernel, bias)
    for t, (f, y) in enumerate(batches, 1):
        probe_step(st, f, y, opt, scalars(opt, lr, betas, eps, weight_decay, t), rnd)
    return st

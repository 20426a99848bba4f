"""Restatement of the distillation of an embedding head -- the reference's ``DistillationProblem.train_step_inner``
(tfimm/train/problems/distillation.py) with a frozen student backbone, so that only the student's Dense head is trained --
in plain numpy (test helper): the single written rule that tfimm_hip_distill_grad (csrc/distill.hip) and
``tfimm.EmbeddingProbe`` are held to.  The update behind the gradient rows is tests/head_fit_ref.py's.

    student s = f16 . w16^T + bias            f16 = bf16(f), w16 = bf16(w); teacher t given, float32
    inv_s = 1 / sqrt(max(sum s^2, 1e-12)),  u = s * inv_s ;  inv_t, v from t alike       (tf.math.l2_normalize)
    c      = sum_e u_e v_e                    the cosine, in both modes
    normalised:     loss_b = sum_e (u_e - v_e)^2 ;  d loss_b / d s_e = 2 inv_s (c u_e - v_e)
                    [= 2 inv_s ((u - v) - u (u . (u - v))) with u . u = 1: the projection of 2 (u - v) off u, scaled]
        under the clamp (sum s^2 < 1e-12) inv_s is the constant 1e6 and the derivative is 2 inv_s (u_e - v_e)
    un-normalised:  loss_b = sum_e (s_e - t_e)^2 ;  d loss_b / d s_e = 2 (s_e - t_e)
    g[b]   = bf16(d loss_b / d s)             zeros, loss = cosine = 0 for a row with valid[b] = -1
    n      = number of rows with valid[b] = 0;  the head update divides by max(n, 1)            (reduce_mean over the batch)
    wd2    = 2 weight_decay / (D E + E)       d/dw of weight_decay * sum(w^2) / nb_variables, kernel and bias

The error bars of tests/test_gpu_distill.py (u = 2^-24, the unit roundoff of float32; L = E / 64):

  The device forms each sum per lane over its even and over its odd columns -- at most L / 2 + 2 terms each, one fma and so
  one rounding each --, adds the two and then the 64 partial sums in six butterfly steps: along the longest chain
  L / 2 + 9 <= L + 10 roundings.  To first order such a sum is off by at most (L + 10) u times the sum of the magnitudes
  of its terms.
    * sum s^2 (all terms positive): (L + 10) u relative.  inv_s = 1 / sqrt(.): half of it and two more roundings,
      (L / 2 + 7) u relative; u_e = s_e inv_s: (L / 2 + 8) u of |u_e| <= 1.  v_e alike.
    * c = ((sum s t) inv_s) inv_t: the sum is off by (L + 10) u sum |s t| and sum |s t| inv_s inv_t <= 1 (Cauchy-Schwarz);
      the two factors and the two products add 2 (L / 2 + 7) + 2.
    * gradient before its bf16 rounding: 2 inv_s fma(c, u_e, -v_e); every quantity inside is at most 1 in magnitude.
  The chain that dominates is the one sum of L + 10 roundings: (L + 10) u plus the "few operations" behind it is the
  (L + 8) * 2^-23 = (2 L + 16) u of the contract, per unit of 2 inv_s; the bf16 rounding adds half a unit in the last place
  of the 8 significant bits of bf16, h(g) = 2^(floor(log2 |g|) - 8) (``half_ulp_bf16``):
        |g - g64| <= h(g64) + 2 inv_s (L + 8) 2^-23              (inv_s = 1 for the un-normalised mode)
  h(g) lies between 2^-9 |g| (just below a power of two) and 2^-8 |g| (at one).  The bar was first written with 2^-9 |g64|
  for this term; that is half a unit of NINE significant bits, which no round-to-nearest bf16 value can keep: at
  (B, E) = (1, 1), normalize = 0, where g = 2 (s - t) is exact in float32 and the rounding is the only error, the device was
  1.48 times that bar away -- 0.74 of 2^-8 |g|, what nearest-even rounding of 8 bits gives.  tests/test_gpu_head_fit.py states
  the same rounding as 2^-8 relative; h(g) is the exact form and never wider.
  If EVERY rounding of all three sums, both inverse norms and the products erred in the same direction the total would be
  (3 L + 44) u, above that bar; they are independent and of either sign: N roundings of rms u / sqrt(12) each add up to
  sqrt(N / 12) u -- 4.4 u at L = 64 against a bar of 144 u, 1.9 u at L = 0 against 16 u.  The test prints the observed
  maximum of error / bar for every shape.
    * loss = sum (u - v)^2 and cosine = c: the same sums, values of magnitude <= 4 and <= 1:
        |loss - loss64|, |cosine - cosine64| <= (L + 8) 2^-23 max(1, |value|)
      (un-normalised: the terms are (s_e - t_e)^2, one rounding each; the scale is the loss itself.)

Deliberately independent of the engine: nothing here imports tfimm.
"""
import numpy as np

import head_fit_ref as hr
from head_fit_ref import ADAM, SGD, bf16_rne, bf16_trunc  # noqa: F401

f32, f64 = np.float32, np.float64
CLAMP = 1e-12


def half_ulp_bf16(g):
    """half a unit in the last place of bf16 (8 significant bits) at every element of g; 0 at 0"""
    a = np.abs(np.asarray(g, f64))
    return np.where(a > 0, 2.0 ** (np.floor(np.log2(np.where(a > 0, a, 1.0))) - 8), 0.0)


def trained(valid):
    """rows trained on: valid[b] == 0 (-1: ignored)"""
    return np.asarray(valid, np.int64) == 0


def l2_normalize(x):
    """(x * inv, inv, clamped) per row, float64"""
    x = np.asarray(x, f64)
    ss = (x * x).sum(axis=1)
    inv = 1.0 / np.sqrt(np.maximum(ss, CLAMP))
    return x * inv[:, None], inv, ss < CLAMP


def rows(s, t, valid=None, normalize=True):
    """(grad (B, E), loss (B,), cosine (B,)) in float64, nothing rounded: the row rule of tfimm_hip_distill_grad"""
    s, t = np.asarray(s, f64), np.asarray(t, f64)
    ok = np.ones(len(s), bool) if valid is None else trained(valid)
    u, inv_s, clamped = l2_normalize(s)
    v, _, _ = l2_normalize(t)
    c = (u * v).sum(axis=1)
    if normalize:
        k = np.where(clamped, 1.0, c)                         # under the clamp inv_s is a constant: 2 inv_s (u - v)
        grad = 2.0 * inv_s[:, None] * (k[:, None] * u - v)
        loss = ((u - v) ** 2).sum(axis=1)
    else:
        grad = 2.0 * (s - t)
        loss = ((s - t) ** 2).sum(axis=1)
    grad[~ok] = 0.0
    return grad, np.where(ok, loss, 0.0), np.where(ok, c, 0.0)


def wd2(D, E, weight_decay):
    """what the head update multiplies w by: the derivative of weight_decay * sum(w^2) / (D E + E)"""
    return 2.0 * float(weight_decay) / (D * E + E)


def scalars(opt, lr, betas, eps, weight_decay, t, D, E):
    """(lr, mom_or_one_minus_b1, one_minus_b2, eps, wd2) in float64 for step t (1-based)"""
    return hr.scalars(opt, lr, betas, eps, weight_decay, t)[:4] + (wd2(D, E, weight_decay),)


def total_loss(w, bias, f, t, valid, weight_decay, normalize=True):
    """mean row loss over the trained rows + weight_decay * (sum w^2 + sum bias^2) / nb_variables: train_step_inner's
    l2_loss + reg_loss, float64, nothing rounded.  w is (E, D)."""
    w, bias, f = np.asarray(w, f64), np.asarray(bias, f64), np.asarray(f, f64)
    n = max(int(trained(valid).sum()), 1)
    loss = rows(f @ w.T + bias, t, valid, normalize)[1].sum() / n
    return loss + weight_decay * ((w * w).sum() + (bias * bias).sum()) / (w.size + bias.size)


def labels_of(valid):
    """the `labels` tfimm_hip_head_update counts n from: the valid array itself (0 lies in [0, C), -1 does not)"""
    return np.asarray(valid, np.int64)


def probe_step(state, f, t, valid, opt, sc, normalize=True, rnd=bf16_rne):
    """One step of the probe in float64 with ``rnd`` at every place the contract rounds to bf16 (features, shadow weights,
    gradient rows).  ``state``: head_fit_ref's dict, w (E, D) -- replaced in place.  Returns (loss, cosine) per row under the
    weights before the step."""
    f16 = rnd(f)
    s = f16 @ rnd(state["w"]).T + state["bias"]
    grad, loss, cos = rows(s, t, valid, normalize)
    out = hr.head_update(f16, rnd(grad), labels_of(valid), state["w"], state["s1"], state["s2"], state["bias"], state["bias_s1"],
                         state["bias_s2"], opt, sc, ft=f64)
    for k in ("w", "s1", "s2", "bias", "bias_s1", "bias_s2"):
        state[k] = out[k]
    return loss, cos


def run(kernel, bias, batches, opt, lr, betas, eps, weight_decay, normalize=True, rnd=bf16_rne):
    """``batches``: a sequence of (features, teacher, valid); returns (the final state, the mean loss over the trained rows
    of every step)"""
    st = hr.new_state(kernel, bias)
    E, D = st["w"].shape
    means = []
    for i, (f, t, valid) in enumerate(batches, 1):
        loss, _ = probe_step(st, f, t, valid, opt, scalars(opt, lr, betas, eps, weight_decay, i, D, E), normalize, rnd)
        means.append(loss.sum() / max(int(trained(valid).sum()), 1))
    return st, means

"""pytest -m gpu: the LoRA path on the device.  tfimm_hip_lora_delta (csrc/lora.hip) and its float32 twin
against the float64 contract of tests/lora_ref.py; ``LoRAConvNeXt`` unmerged against the oracle run on the merged weights;
merged against the base model bit for bit; an adapter swap under a live recording.

Observed on MI355X (unmerged, rel-to-max error of the logits against the oracle; the bars are TOL_LOGITS = 5e-2 and 1e-3):
rank 4: bf16 1.38e-2, fp32 1.0e-6; rank 17: bf16 1.86e-2, fp32 2.0e-6.  Kernel cases: element-wise score 0.25 of the STAGED bar
(half an ulp: the one rounding of the output) at every shape but K = 8192, where it is 0.26 with and 0.59 without the residual;
slope and offset at most 5.0e-5 against BIAS_GEMM = 3e-4 (the 8-output case runs on exact data and measures 0).  float32 twin:
2.9e-7 rel-to-max where a bf16-rounded t would give 3e-3."""
import ctypes as C

import numpy as np
import pytest
import torch

import hip_checks as hc
import lora_ref as lr
import model_checks as mc
import oracle
from tfimm.architectures.convnext import ConvNeXtConfig
from tfimm.architectures.lora import (
    LORA_WEIGHT_NAMES,
    LoRAConvNeXt,
    LoRAConvNeXtConfig,
    convert_to_regular_model,
    merge_lora_weights,
    unmerge_lora_weights,
)
from tfimm.engine import ffi, precision
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = 0x5A5A
TOL_FP32 = 1e-3          # the float32 path's bar (tests/test_gpu_fp32.py)

#: (M, K, N, r): one row; K and N that are no multiple of the 32-deep k-step / the 64-column trip; more than one workgroup (128
#: rows) with a ragged last wave and a rank that is no multiple of 16; whole tiles; the full rank; the longest K with the full rank
SHAPES = [(1, 8, 8, 1), (37, 24, 152, 4), (333, 200, 152, 17), (64, 96, 384, 16), (130, 384, 96, 64), (37, 8192, 64, 64)]
#: fewer outputs than this: exact data (see ``inputs``)
FEW = 256


def inputs(M, K, N, r, residual=True, rounded=True):
    """x, A, B', residual with t and t . B' of unit scale, so that a dropped or mis-scaled low-rank term cannot pass.

    A correctly rounded result is itself off by up to half an ulp per element, which the slope and the offset over few
    elements do not average away (2^-9 / sqrt(8) = 7e-4 for the 8 outputs of the first shape, twice BIAS_GEMM): a shape with
    fewer than ``FEW`` outputs therefore gets small dyadic values for which t and the result are exact in bf16 -- the bars
    then ask for an error of exactly zero there.  Either way the REFERENCE ROUNDED TO bf16 must sit inside half the bias
    bar: asserted below, on the reference alone."""
    rng = np.random.default_rng(1000 + M + K + N + r)
    if M * N < FEW:
        assert K * r <= 8                                  # |t| <= 16 in halves, |t b + residual| <= 26 in quarters: 8 bits
        x = rng.integers(-2, 3, (M, K)).astype(f32)
        a = rng.choice([-1.0, -0.5, 0.5, 1.0], (K, r)).astype(f32)
        b = rng.choice([-1.5, -1.0, -0.5, 0.5, 1.0, 1.5], (r, N)).astype(f32)
        res = (rng.integers(-8, 9, (M, N)) / 4).astype(f32) if residual else None
    else:
        x = rng.standard_normal((M, K)).astype(f32)
        a = (rng.standard_normal((K, r)) / np.sqrt(K)).astype(f32)
        b = (rng.standard_normal((r, N)) / np.sqrt(r)).astype(f32)
        res = rng.standard_normal((M, N)).astype(f32) if residual else None
    if rounded:
        x, a, b, res = lr.bf16(x), lr.bf16(a), lr.bf16(b), None if res is None else lr.bf16(res)
        ref = lr.lora_delta(x, a, b, res)
        low_rank = lr.lora_delta(x, a, b, None)
        if res is not None:
            assert np.sqrt(np.mean(low_rank ** 2)) >= 0.25 * np.sqrt(np.mean(res.astype(np.float64) ** 2))
        slope, offset = hc._bias(hc._rne_bf16(ref), ref)
        assert max(slope, offset) <= hc.BIAS_GEMM / 2, (slope, offset)
    return x, a, b, res


class Launch:
    """Operands on the device in the descriptor's layout: pitches ``K + pad`` / ``N + pad``, NaN in every padding column of
    an input, ``guard`` rows of the sentinel in front of and behind ``out`` and the sentinel in its padding columns."""

    def __init__(self, x, a, b, res, pad=0, guard=0, fp32=False):
        (self.M, self.K), self.N = x.shape, b.shape[1]
        at, bt = lr.pack_operands(a, b)
        self.Rp, self.guard, self.fp32 = at.shape[0], guard, fp32
        self.lda, self.lda_a, self.ldr, self.ldc = self.K + pad, self.K + 2 * pad, self.N + 3 * pad, self.N + pad
        dt = torch.float32 if fp32 else torch.bfloat16

        def dev(arr, pitch):
            h = np.full((arr.shape[0], pitch), np.nan, f32)
            h[:, :arr.shape[1]] = arr
            t = torch.from_numpy(h).cuda().to(dt)
            assert t.data_ptr() % 16 == 0
            return t

        self.x, self.a, self.b = dev(x, self.lda), dev(at, self.lda_a), dev(bt, self.Rp)
        self.res = None if res is None else dev(res, self.ldr)
        # out as integers of the element's size, every one the sentinel (float32: the 16-bit pattern twice)
        self.sentinel = SENTINEL * 65537 if fp32 else SENTINEL
        self.out = torch.full(((2 * guard + self.M) * self.ldc,), self.sentinel, dtype=torch.int32 if fp32 else torch.int16,
                              device="cuda")
        self.desc = ffi.LoraDesc()
        d, es = self.desc, self.out.element_size()
        d.x, d.a, d.b = self.x.data_ptr(), self.a.data_ptr(), self.b.data_ptr()
        d.residual = None if self.res is None else self.res.data_ptr()
        d.out = self.out.data_ptr() + guard * self.ldc * es
        d.M, d.K, d.N, d.Rp = self.M, self.K, self.N, self.Rp
        d.lda, d.lda_a, d.ldr, d.ldc = self.lda, self.lda_a, self.ldr, self.ldc

    def run(self):
        fn = ffi.lib.tfimm_hip_ref_lora_delta if self.fp32 else ffi.lib.tfimm_hip_lora_delta
        rc = fn(C.byref(self.desc), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return bool((self.out == self.sentinel).all())

    def result(self):
        """the M x N result as float64, after checking that nothing but it was written"""
        rows = self.out.view(2 * self.guard + self.M, self.ldc)
        g, sent = self.guard, self.sentinel
        assert (rows[:g] == sent).all() and (rows[g + self.M:] == sent).all(), "a launch wrote into a guard row"
        assert (rows[g:g + self.M, self.N:] == sent).all(), "a launch wrote into the padding columns of out"
        body = rows[g:g + self.M, :self.N].contiguous()
        return body.view(torch.float32 if self.fp32 else torch.bfloat16).double().cpu().numpy()


# ---- the kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_meets_the_staged_bar(shape, residual):
    x, a, b, res = inputs(*shape, residual=residual)
    run = Launch(x, a, b, res, guard=1)
    assert run.run() == 0, ffi.lib.tfimm_hip_last_error().decode()
    e, stats = hc.tight_score(run.result(), lr.lora_delta(x, a, b, res), hc.STAGED, hc.BIAS_GEMM)
    print(f"lora_delta {shape} residual={residual}: score {e:.3f} (element-wise, slope, offset) = {stats}")
    assert e <= 1.0, (e, stats)


def test_kernel_with_pitches_larger_than_the_rows():
    x, a, b, res = inputs(333, 200, 152, 17)
    run = Launch(x, a, b, res, pad=8, guard=1)
    assert (run.lda, run.lda_a, run.ldr, run.ldc) == (208, 216, 176, 160)
    assert run.run() == 0, ffi.lib.tfimm_hip_last_error().decode()
    got = run.result()
    e, stats = hc.tight_score(got, lr.lora_delta(x, a, b, res), hc.STAGED, hc.BIAS_GEMM)
    assert e <= 1.0, (e, stats)
    dense = Launch(x, a, b, res)
    assert dense.run() == 0
    assert np.array_equal(dense.result(), got)            # the pitch moves no value


def test_kernel_leaves_guard_rows_alone():
    x, a, b, res = inputs(130, 384, 96, 64)
    run = Launch(x, a, b, res, pad=16, guard=3)
    assert run.run() == 0, ffi.lib.tfimm_hip_last_error().decode()
    got = run.result()                                      # (asserts the guard rows and the padding columns)
    assert not run.untouched() and np.isfinite(got).all()


def test_a_row_does_not_depend_on_m():
    x, a, b, res = inputs(333, 200, 152, 17)
    full = Launch(x, a, b, res)
    part = Launch(x[:130], a, b, res[:130])
    assert full.run() == 0 and part.run() == 0
    assert np.array_equal(full.result()[:130], part.result())


def _refusal(edit, K=16, N=16, r=4):
    x, a, b, res = inputs(20, K, N, r, rounded=False)
    run = Launch(lr.bf16(x), lr.bf16(a), lr.bf16(b), lr.bf16(res))
    edit(run.desc, run)
    rc = run.run()
    assert run.untouched(), "a refused call wrote its output"
    return rc, ffi.lib.tfimm_hip_last_error().decode()


def test_refusals_launch_nothing():
    def k12(d, run):
        d.K = 12

    def n12(d, run):
        d.N = 12

    def rp80(d, run):
        d.Rp = 80

    def k8200(d, run):
        d.K, d.lda, d.lda_a = 8200, 8200, 8200

    for edit, code, word in ((k12, ffi_code("EUNSUP"), "K=12"), (n12, ffi_code("EUNSUP"), "N=12"), (rp80, ffi_code("EUNSUP"), "Rp=80"),
                             (k8200, ffi_code("EUNSUP"), "K=8200")):
        rc, msg = _refusal(edit)
        assert rc == code and word in msg, (rc, msg)
    x, a, b, res = inputs(20, 16, 16, 4, rounded=False)
    run = Launch(lr.bf16(x), lr.bf16(a), lr.bf16(b), lr.bf16(res))
    before = run.x.clone()
    run.desc.out = run.desc.x
    assert run.run() == ffi_code("EINVAL") and "overlaps x" in ffi.lib.tfimm_hip_last_error().decode()
    assert torch.equal(run.x.view(torch.int16), before.view(torch.int16)) and run.untouched()


def ffi_code(name):
    return {"EINVAL": -1, "EUNSUP": -2}[name]          # include/tfimm_hip.h


@pytest.mark.parametrize("shape", [(37, 24, 152, 4), (130, 384, 96, 64)])
def test_fp32_twin_does_not_round_t(shape):
    x, a, b, res = inputs(*shape, rounded=False)
    run = Launch(x, a, b, res, pad=8, guard=1, fp32=True)
    assert run.run() == 0, ffi.lib.tfimm_hip_last_error().decode()
    ref = lr.lora_delta(x, a, b, res, round_t=False)
    err = mc.rel_err(run.result(), ref)
    rounded = mc.rel_err(lr.lora_delta(x, a, b, res), ref)
    print(f"ref_lora_delta {shape}: rel-to-max {err:.2e} (a bf16-rounded t would be {rounded:.2e})")
    assert err <= TOL_FP32


# ---- the model ------------------------------------------------------------------------------------------------------------------
MINI = dict(name="lora_mini", input_size=(32, 32), embed_dim=(16, 32, 64, 128), nb_blocks=(1, 1, 2, 1), nb_classes=12)
ALPHA = 8.0


def is_lora(name):
    return name.rsplit("/", 1)[1] in LORA_WEIGHT_NAMES


def adapter(model, seed):
    """seeded normal A and B of a size at which the low-rank terms move the logits by far more than the parity bar"""
    rng = np.random.default_rng(seed)
    out = {}
    for k, v in model.weights.items():
        if is_lora(k):
            fan = v.shape[0] if k.endswith("_a") else ALPHA
            out[k] = (rng.standard_normal(v.shape) / np.sqrt(fan)).astype(f32)
    return out


def merged_for_oracle(weights, scaling):
    """the base model's weights with W + scaling * A @ B in place of every adapted kernel, formed here in float64"""
    out = {}
    for k, v in weights.items():
        if is_lora(k):
            continue
        if k + "_lora_a" in weights:
            v = (v.astype(np.float64) + scaling * (weights[k + "_lora_a"].astype(np.float64) @ weights[k + "_lora_b"].astype(np.float64)))
        out[k] = np.asarray(v, f32)
    return out


_SETUPS = {}


def setup(rank):
    """model, its weights, the input and the oracle's logits with and without the adapter: built once per rank"""
    if rank not in _SETUPS:
        model = LoRAConvNeXt(LoRAConvNeXtConfig(**MINI, lora_rank=rank, lora_alpha=ALPHA))
        w = synthetic_weights(model, 2021)
        w.update(adapter(model, 11 + rank))
        model.set_weights(w)
        x = mc.make_input(model.cfg, 3)
        base_cfg = ConvNeXtConfig(**MINI)
        ref = oracle.forward(base_cfg, merged_for_oracle(w, ALPHA / rank), x)
        plain = oracle.forward(base_cfg, {k: v for k, v in w.items() if not is_lora(k)}, x)
        _SETUPS[rank] = (model, w, x, np.asarray(ref), np.asarray(plain))
    return _SETUPS[rank]


@pytest.mark.parametrize("rank", [4, 17])
def test_unmerged_model_against_the_oracle_on_merged_weights(rank):
    model, w, x, ref, plain = setup(rank)
    moved = mc.rel_err(plain, ref)
    assert moved > 10 * mc.TOL_LOGITS, f"the adapter moves the oracle's logits by {moved:.2e} only"
    assert not model.merged and "lora_delta" in [op.kind for op in model.program().ops]
    got = model(x).numpy()
    err = mc.rel_err(got, ref)
    print(f"LoRAConvNeXt rank {rank} unmerged, bf16: logits rel-to-max {err:.2e} (the adapter moves them by {moved:.2e})")
    assert err <= mc.TOL_LOGITS
    srt = np.sort(ref, -1)
    margin, row_abs = srt[:, -1] - srt[:, -2], np.abs(got - ref).max(-1)
    assert ((got.argmax(-1) == ref.argmax(-1)) | (margin < 2 * row_abs)).all()
    with precision.use("fp32"):
        got32 = model(x).numpy()
    err32 = mc.rel_err(got32, ref)
    print(f"LoRAConvNeXt rank {rank} unmerged, fp32: logits rel-to-max {err32:.2e}")
    assert err32 <= TOL_FP32


def test_merged_model_is_the_base_model_bit_for_bit():
    model, w, x, ref, _ = setup(4)
    unmerged = model(x).numpy()
    base = convert_to_regular_model(model)
    merge_lora_weights(model)
    try:
        assert "lora_delta" not in [op.kind for op in model.program().ops]
        merged = model(x).numpy()
        assert np.array_equal(merged, base(x).numpy())
        assert mc.rel_err(merged, ref) <= mc.TOL_LOGITS
    finally:
        unmerge_lora_weights(model)
    assert np.array_equal(model(x).numpy(), unmerged)


def test_adapter_swap_keeps_programs_plans_and_recordings():
    model, w, x, _, _ = setup(17)
    first = model(x).numpy()
    model(x)                                   # the second call records
    assert model._captured
    held = [dict(model._programs), dict(model._plans), dict(model._captured)]
    second = adapter(model, 99)
    try:
        model.set_lora_weights(second)
        for before, now in zip(held, (model._programs, model._plans, model._captured)):
            assert list(before) == list(now) and all(before[k] is now[k] for k in before)
        swapped = model(x).numpy()
        assert list(model._captured) == list(held[2])
        fresh = LoRAConvNeXt(LoRAConvNeXtConfig(**MINI, lora_rank=17, lora_alpha=ALPHA))
        fresh.set_weights({**w, **second})
        assert np.array_equal(swapped, fresh(x).numpy())
        assert not np.array_equal(swapped, first)
    finally:
        model.set_lora_weights({k: w[k] for k in second})
    assert np.array_equal(model(x).numpy(), first)


def test_branches_and_top_k():
    model, w, _, _, _ = setup(4)
    x = mc.make_input(model.cfg, 4, seed=5)
    one = model(x).numpy()
    model.branches = 2
    try:
        assert np.array_equal(model(x).numpy(), one)
    finally:
        model.branches = 1
    top = model.top_k(x, 3)
    order = np.argsort(-one, axis=-1, kind="stable")[:, :3]
    assert np.array_equal(top.indices.numpy(), order)

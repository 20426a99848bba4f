"""tfimm_hip_gemm refuses a malformed descriptor before anything touches a device (CPU): one case per refusal of validate().

validate() (csrc/gemm.hip) returns TFIMM_EINVAL through one TFIMM_FAIL per clause.  REFUSALS walks it top to bottom: each entry
takes a VALID baseline descriptor (hip_ops.gemm_baseline), breaks exactly one field and names the phrase of the clause's message,
so that a clause that stops firing, fires for the wrong reason or moves behind another is seen.  The first element of an entry is
the clause's number in source order; to recount, list the TFIMM_FAIL lines between ``int validate(`` and the ``// ---- step 2``
banner of csrc/gemm.hip (test_refusal_table_has_every_clause_of_validate does exactly that and fails when they disagree).
"""
import ctypes
import os
import re

import pytest

import hip_ops as H
from tfimm.engine import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _set(**fields):
    def mutate(d):
        for k, v in fields.items():
            setattr(d, k, v)
    return mutate


def _off(field, nbytes):
    """move a pointer by ``nbytes`` (misalign it)"""
    def mutate(d):
        setattr(d, field, getattr(d, field) + nbytes)
    return mutate


def _alias(dst, src):
    """point ``dst`` at what ``src`` points at (any valid, aligned tensor: nothing is launched)"""
    def mutate(d):
        setattr(d, dst, getattr(d, src))
    return mutate


def _both(*ms):
    def mutate(d):
        for m in ms:
            m(d)
    return mutate


# (clause, id, baseline, what to break, phrase of the message)
REFUSALS = [
    (1, "null_a", "dense", _set(a=None), "null a/wt/out pointer"),
    (1, "null_wt", "dense", _set(wt=None), "null a/wt/out pointer"),
    (1, "null_out", "conv", _set(out=None), "null a/wt/out pointer"),
    (2, "M_zero", "dense", _set(M=0), "M=0 N=40 K=72"),
    (2, "N_negative", "dense", _set(N=-1), "N=-1"),
    (2, "K_zero", "dense", _set(K=0), "K=0"),
    (3, "ldw_below_K", "dense", _set(ldw=64), "ldw=64 must be >= K=72"),
    (3, "ldw_not_multiple_of_8", "dense", _set(ldw=132), "ldw=132 must be >= K=72 and a multiple of 8"),
    (4, "wt_misaligned", "dense", _off("wt", 8), "wt must be 16-byte aligned"),
    (5, "ldc_below_N", "dense", _set(ldc=39), "ldc=39 < N=40"),
    (6, "mode_3", "dense", _set(mode=3), "mode=3"),
    (6, "mode_negative", "dense", _set(mode=-1), "mode=-1"),
    (7, "remap_in_negative", "dense", _set(remap_in=-1), "negative remap/res_mod"),
    (7, "res_mod_negative", "dense", _set(res_mod=-1), "negative remap/res_mod"),
    (8, "bias_misaligned", "dense", _off("bias", 4), "bias must be 16-byte aligned"),
    (9, "ln_stats_without_c1", "ln_fold", _set(ln_c1=None), "ln_stats and ln_c1 go together"),
    (9, "ln_c1_without_stats", "ln_fold", _set(ln_stats=None), "ln_stats and ln_c1 go together"),
    (10, "ln_with_residual", "ln_fold", _alias("residual", "a"), "LayerNorm folding needs a dense bf16 layer"),
    (10, "ln_with_f32_out", "ln_fold", _set(out_f32=1), "LayerNorm folding needs a dense bf16 layer"),
    (10, "ln_with_gate", "ln_fold", _both(_alias("a_scale", "bias"), _set(rows_per_image=36)), "LayerNorm folding needs a dense bf16 layer"),
    (10, "ln_stats_misaligned", "ln_fold", _off("ln_stats", 8), "16-byte aligned tables"),
    (10, "ln_c1_misaligned", "ln_fold", _off("ln_c1", 2), "16-byte aligned tables"),
    (11, "a2_with_residual", "dual_dense", _alias("residual", "a"), "a second A operand needs a bf16 layer"),
    (11, "a2_with_f32_out", "dual_dense", _set(out_f32=1), "a second A operand needs a bf16 layer"),
    (11, "a2_with_remap", "dual_dense", _set(remap_in=36, remap_out=36), "a second A operand needs a bf16 layer"),
    (11, "a2_with_res_mod", "dual_conv", _set(res_mod=36), "a second A operand needs a bf16 layer"),
    (11, "a2_in_c4_mode", "dual_conv", _set(mode=2), "a second A operand needs a bf16 layer"),
    (12, "a2_K2_zero", "dual_dense", _set(K2=0), "a2 needs K2=0"),
    (12, "a2_K2_not_multiple_of_8", "dual_dense", _set(K2=36), "a2 needs K2=36 % 8 == 0"),
    (12, "a2_lda2_below_K2", "dual_dense", _set(lda2=32), "lda2=32 >= K2"),
    (12, "a2_lda2_not_multiple_of_8", "dual_conv", _set(lda2=44), "lda2=44 >= K2 and % 8 == 0"),
    (12, "a2_misaligned", "dual_conv", _off("a2", 8), "a 16-byte aligned pointer"),
    (13, "a2_stride_zero", "dual_dense", _set(a2_stride=0), "a2_stride=0 a2_window=0"),
    (13, "a2_window_negative", "dual_dense", _set(a2_window=-1), "a2_window=-1"),
    (13, "a2_window_5", "dual_dense_window2", _set(a2_window=5), "a2_window=5"),
    (14, "a2_geometry_missing", "dual_dense", _set(a2_stride=2), "a2 geometry 0x0 -> 0x0 at stride 2, window 1"),
    (14, "a2_rows_not_whole_images", "dual_dense_window2", _set(a2_OH=5), "a2 geometry 12x12 -> 5x6"),
    (14, "a2_window_leaves_image", "dual_conv_window2", _set(a2_W=11), "a2 geometry 12x11 -> 6x6 at stride 2, window 2"),
    # the gap the header never allowed: the LAST tap of the second operand left unpadded (K2 = 40: 64 columns per tap)
    (15, "a2_last_tap_unpadded", "dual_dense", _set(ldw=128 + 40), "padded to whole 64-wide k-tiles (ldw >= 192)"),
    (15, "a2_last_of_four_taps_unpadded", "dual_dense_window2", _set(ldw=128 + 3 * 64 + 40), "4 taps of K2=40: wt holds K and every tap padded to whole 64-wide k-tiles (ldw >= 384)"),
    (15, "a2_conv_last_tap_unpadded", "dual_conv_window2", _set(ldw=128 + 3 * 64 + 40), "padded to whole 64-wide k-tiles"),
    (15, "a2_weights_of_first_operand_only", "dual_conv", _set(ldw=128), "ldw=128 too small for K=72 + 1 taps of K2=40"),
    (16, "lda_below_K", "dense", _set(lda=64), "lda=64 < K=72"),
    (17, "gate_on_unaligned_rows", "se_gate", _set(lda=76), "a_scale needs aligned K % 8 == 0 rows"),
    (17, "gate_on_misaligned_a", "se_gate", _off("a", 8), "a_scale needs aligned K % 8 == 0 rows"),
    (17, "gate_without_rows_per_image", "se_gate", _set(rows_per_image=0), "rows_per_image > 0"),
    (17, "gate_table_misaligned", "se_gate", _off("a_scale", 4), "a_scale needs aligned"),
    (18, "gate_on_conv", "conv", _both(_alias("a_scale", "bias"), _set(rows_per_image=36)), "a_scale only in dense mode"),
    (19, "conv_B_zero", "conv", _set(B=0), "bad conv geometry"),
    (19, "conv_H_zero", "conv", _set(H=0), "bad conv geometry"),
    (19, "conv_W_negative", "conv_c4", _set(W=-6), "bad conv geometry"),
    (19, "conv_KH_zero", "conv", _set(KH=0), "bad conv geometry"),
    (19, "conv_KW_zero", "conv_c4", _set(KW=0), "bad conv geometry"),
    (19, "conv_stride_zero", "conv", _set(stride=0), "bad conv geometry"),
    (19, "conv_OH_zero", "conv", _set(OH=0), "bad conv geometry"),
    (19, "conv_OW_zero", "conv", _set(OW=0), "bad conv geometry"),
    (20, "conv_M_not_B_OH_OW", "conv", _set(M=71), "M != B*OH*OW"),
    (20, "conv_c4_OW_off", "conv_c4", _set(OW=5), "M != B*OH*OW"),
    (21, "conv_input_misaligned", "conv", _off("a", 8), "conv input must be 16-byte aligned"),
    (22, "conv_K_not_KH_KW_Cin", "conv", _set(K=64), "K != KH*KW*Cin"),
    (23, "pix_pitch_negative", "conv", _set(pix_pitch=-8), "pix_pitch=-8 < Cin=8"),
    (23, "pix_pitch_below_Cin", "conv", _set(pix_pitch=4), "pix_pitch=4 < Cin=8"),
    (24, "c4_Cin_8", "conv_c4", _set(Cin=8), "C4 mode needs Cin == 4"),
    (24, "c4_pix_pitch_8", "conv_c4", _set(pix_pitch=8), "C4 mode needs Cin == 4 (and no pixel pitch)"),
    (25, "c4_K_of_unpadded_row", "conv_c4", _set(K=36), "K != KH*KWp*4 (K=36)"),
]


def _call(d):
    rc = ffi.lib.tfimm_hip_gemm(ctypes.byref(d), None)
    return rc, ffi.lib.tfimm_hip_last_error().decode()


@pytest.mark.parametrize("clause,name,kind,mutate,phrase", REFUSALS, ids=[f"{c:02d}_{n}" for c, n, *_ in REFUSALS])
def test_validate_refuses(clause, name, kind, mutate, phrase):
    d, out, keep = H.gemm_baseline(kind)
    mutate(d)
    rc, msg = _call(d)
    assert rc == EINVAL, (rc, msg)
    assert msg.startswith("gemm: ") and phrase in msg, msg


def _validate_source():
    src = open(os.path.join(ROOT, "tensorflow-image-models_amd", "csrc", "gemm.hip")).read()
    return src[src.index("int validate("):src.index("// ---- step 2")]


def test_refusal_table_has_every_clause_of_validate():
    n = len(re.findall(r"\bTFIMM_FAIL\(", _validate_source()))
    assert n == 25, f"validate() has {n} TFIMM_FAIL clauses now: walk it again and bring REFUSALS up to date"
    assert sorted({c for c, *_ in REFUSALS}) == list(range(1, n + 1))
    assert [c for c, *_ in REFUSALS] == sorted(c for c, *_ in REFUSALS), "REFUSALS follows the source order of validate()"
    assert len({name for _, name, *_ in REFUSALS}) == len(REFUSALS)
    assert set(re.findall(r"TFIMM_FAIL\((\w+)", _validate_source())) == {"TFIMM_EINVAL"}


@pytest.mark.parametrize("kind", H.BASELINES)
def test_baselines_pass_validate(kind):
    """every baseline gets past validate(): without a GPU what comes back is the first HIP call's error, never a refusal (with
    one, 0: tests/test_gpu_gemm_contract.py looks at the result)"""
    d, out, keep = H.gemm_baseline(kind)
    rc, msg = H.gemm_rc(d)
    H.sync()
    assert rc == 0 or (H.DEV == "cpu" and rc > 0 and not msg.startswith("gemm: ")), (rc, msg)


def test_second_operand_weights_padded_per_tap_is_the_smallest_pitch_accepted():
    """ldw = pad64(K) + taps * pad64(K2) exactly passes validate(); 8 columns fewer do not (K2 = 40: the last tap's pad)"""
    for kind, need in (("dual_dense", 192), ("dual_dense_window2", 384), ("dual_conv", 192), ("dual_conv_window2", 384)):
        d, out, keep = H.gemm_baseline(kind)
        assert d.ldw == need
        d.ldw = need - 8
        rc, msg = _call(d)
        assert rc == EINVAL and f"ldw >= {need}" in msg, (kind, rc, msg)


def test_device_info_of_a_device_that_does_not_exist():
    """a positive return is a CU count, so a failure is negative (the negated hipError_t), names the call and leaves name[] alone"""
    n, name = H.device_info(device=4096)
    assert n < 0, n
    assert b"hipGetDeviceProperties(device 4096)" in ffi.lib.tfimm_hip_last_error()
    assert name == "?" * 63
    assert ffi.lib.tfimm_hip_device_info(4096, None, 0) < 0            # no buffer: the same answer, nothing written

"""The contract of tfimm_hip_lora_delta (include/tfimm_hip.h, csrc/lora.hip) restated in float64 numpy:

    t   = bf16( x[M][K] . A[K][R] )                      one rounding, nearest even
    out =       residual[M][N] + t[M][R] . B'[R][N]      (the kernel rounds this once more, to bf16)

Inputs are rounded to bf16 first -- they are what the device holds -- so the only differences left between a correct kernel
and ``lora_delta`` are its fp32 accumulation order and the final rounding of the stored output.  ``round_t=False`` is the
float32 twin's contract (tfimm_hip_ref_lora_delta: float32 inputs as they are, t not rounded).
"""
import numpy as np

import hip_checks as hc
from tfimm.engine import pack


def bf16(a):
    """float32 array -> the bf16 values the device holds, as float32"""
    a = np.asarray(a, dtype=np.float32)
    return pack.bf16_bits_to_f32(pack.to_bf16_bits(a)).reshape(a.shape)


def lora_delta(x, a, b, residual=None, round_t=True):
    """x [M][K], a [K][R], b [R][N] (scaling and any output scale already folded into b), residual [M][N] or None ->
    float64 [M][N]"""
    if round_t:
        x, a, b = bf16(x), bf16(a), bf16(b)
        residual = None if residual is None else bf16(residual)
    t = np.asarray(x, np.float64) @ np.asarray(a, np.float64)
    if round_t:
        t = hc._rne_bf16(t)
    out = t @ np.asarray(b, np.float64)
    return out if residual is None else out + np.asarray(residual, np.float64)


def pack_operands(a, b):
    """a [K][R], b [R][N] float32 -> (a^T [Rp][K], b^T [N][Rp]) float32 with the rank zero padded to a multiple of 16: the
    layout of the descriptor's ``a`` and ``b``"""
    (K, R), N = a.shape, b.shape[1]
    Rp = -(-R // 16) * 16
    at, bt = np.zeros((Rp, K), np.float32), np.zeros((N, Rp), np.float32)
    at[:R], bt[:, :R] = a.T, b.T
    return at, bt

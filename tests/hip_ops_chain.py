"""tfimm_hip_conv_chain_next for the op-level tests (test helper, next to hip_ops.py): the launch wrapper, one random
stage-1 bottleneck tail with the following block's conv1 behind it, and the two-launch path of the same library it is
compared with.  ``python hip_ops_chain.py B H W seed`` prints the sha256 of both outputs of the fused launch (the chunking
test runs it in a process of its own: TFIMM_CHAIN_LIMIT is read once per process)."""
import ctypes as C
import hashlib
import math

import numpy as np
import torch

import hip_ops as H
from tfimm.engine import ffi, pack

lib = ffi.lib


def conv_chain_next(x, wt1, b1, wt2, b2, residual, wt3, b3, *, OH, OW, C1=64, N2=256, N3=64, act1="relu", act2="relu",
                    ds_x=None, ds_w=None, check=True):
    """(out [M][N2], out2 [M][N3], return code) of one tfimm_hip_conv_chain_next launch; 3x3 / stride 1 / pad 1"""
    B, Hh, Ww, Cin = x.shape
    d = ffi.ChainNextDesc()
    out = torch.empty(B * OH * OW, N2, dtype=torch.bfloat16, device=H.DEV)
    out2 = torch.empty(B * OH * OW, N3, dtype=torch.bfloat16, device=H.DEV)
    d.x, d.w1, d.b1, d.w2, d.b2, d.residual, d.out = (H.ptr(x), H.ptr(wt1), H.ptr(b1), H.ptr(wt2), H.ptr(b2), H.ptr(residual),
                                                      H.ptr(out))
    d.B, d.H, d.W, d.Cin, d.KH, d.KW, d.stride, d.pad_t, d.pad_l, d.OH, d.OW = B, Hh, Ww, Cin, 3, 3, 1, 1, 1, OH, OW
    d.C1, d.N2, d.ldw1, d.ldw2, d.ldr, d.ldc = C1, N2, wt1.shape[1], wt2.shape[1], N2, N2
    d.act1, d.act2 = ffi.ACT[act1], ffi.ACT[act2]
    if ds_x is not None:
        d.ds_x, d.ds_w, d.ds_cin = H.ptr(ds_x), H.ptr(ds_w), ds_x.shape[-1]
    d.w3, d.b3, d.out2 = H.ptr(wt3), H.ptr(b3), H.ptr(out2)
    d.N3, d.ldw3, d.ldc2 = N3, wt3.shape[1], N3
    rc = lib.tfimm_hip_conv_chain_next(C.byref(d), H.stream())
    if check:
        ffi.check(rc, "conv_chain_next")
    return out, out2, rc


def make_case(B, Hh, Ww, seed, C1=64, N2=256, N3=64):
    """Device operands of one tail (as hip_checks._chain_case draws them) and of the 1x1 convolution N2 -> N3 behind it"""
    r = np.random.default_rng(seed)
    x = r.standard_normal((B, Hh, Ww, C1)).astype(np.float32)
    k1 = (r.standard_normal((3, 3, C1, C1)) / math.sqrt(9 * C1)).astype(np.float32)
    s1, t1 = r.uniform(0.5, 1.5, C1).astype(np.float32), r.standard_normal(C1).astype(np.float32)
    k2 = (r.standard_normal((C1, N2)) / math.sqrt(C1)).astype(np.float32)
    s2, t2 = r.uniform(0.5, 1.5, N2).astype(np.float32), r.standard_normal(N2).astype(np.float32)
    k3 = (r.standard_normal((N2, N3)) / math.sqrt(N2)).astype(np.float32)
    s3, t3 = r.uniform(0.5, 1.5, N3).astype(np.float32), r.standard_normal(N3).astype(np.float32)
    res = r.standard_normal((B * Hh * Ww, N2)).astype(np.float32)
    wt1, b1, _, _ = pack.pack_conv(k1, s1, t1, C1)
    wt2, b2 = pack.pack_dense((k2 * s2.reshape(1, N2))[pack.chain_k_order(C1)], t2)
    wt3, b3 = pack.pack_dense(k3 * s3.reshape(1, N3), t3)
    return dict(x=H.dev_bf16(x), wt1=H.dev_bits(wt1), b1=H.dev_f32(b1), wt2=H.dev_bits(wt2), b2=H.dev_f32(b2),
                res=H.dev_bf16(res), wt3=H.dev_bits(wt3), b3=H.dev_f32(b3), OH=Hh, OW=Ww, N2=N2, N3=N3)


def run_next(c):
    out, out2, _ = conv_chain_next(c["x"], c["wt1"], c["b1"], c["wt2"], c["b2"], c["res"], c["wt3"], c["b3"], OH=c["OH"],
                                   OW=c["OW"], N2=c["N2"], N3=c["N3"])
    H.sync()
    return out, out2


def run_two_launches(c):
    """tfimm_hip_conv_chain, then tfimm_hip_gemm (bias, relu) on its result: what the program runs without the fold"""
    out = H.conv_chain(c["x"], c["wt1"], c["b1"], c["wt2"], c["b2"], c["res"], KH=3, KW=3, stride=1, pad=1, OH=c["OH"],
                       OW=c["OW"], C1=64, N2=c["N2"])
    out2 = H.gemm(out, c["wt3"], c["N3"], c["N2"], bias=c["b3"], act="relu")
    H.sync()
    return out, out2


def digest(t):
    return hashlib.sha256(t.view(torch.int16).cpu().numpy().tobytes()).hexdigest()


if __name__ == "__main__":
    import sys
    o, o2 = run_next(make_case(*(int(v) for v in sys.argv[1:5])))
    print("DIGEST", digest(o), digest(o2))

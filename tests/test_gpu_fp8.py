"""pytest -m gpu: the MXFP8 precision mode (engine/precision.py "fp8", csrc/mx.hip).

* tfimm_hip_quantize_mx is bit-exact against the shared numpy quantizer (engine/pack.py mx_quantize), with and without the
  LayerNorm it can apply first; with LayerNorm also against the fp64 LayerNorm on every row width class, exact except where
  provably ambiguous (tests/mx_checks.py);
* tfimm_hip_gemm_mx against an fp64 product of the DEQUANTIZED operands, every epilogue and output format, with a bar on
  fp32 accumulation only;
* models: ViT / DeiT against an MX-emulated oracle (oracle.common.W.dense wrapped here so that it quantizes x and the kernel
  with the same rule), Swin / CaiT / ConvNeXt against the plain fp32 oracle next to the bf16 path's own deviation; every
  bar, and every observed deviation from the fp32 oracle, is recorded in tests/golden/fp8_bars.json;
* every quant_mx / gemm_mx op of five fp8 programs, each against a reference built from its own read-back inputs;
* eager vs graph replay, branches=2 vs branches=1, ResNet-50 under fp8 == bf16, an exported fp8 plan through the C host."""
import contextlib
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import model_checks as mc
import mx_checks as mxc
import oracle
import oracle.common
import test_architectures  # noqa: F401
import tfimm
from tfimm.engine import ffi, pack, precision
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = os.path.join(ROOT, "tests", "golden", "fp8_bars.json")
HOST = os.path.join(ROOT, "tensorflow-image-models_amd", "csrc", "build", "plan_host")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bf16_bits(x):
    return pack.to_bf16_bits(x)


def _mixed_rows(rng, rows, c):
    """bf16-representable rows of mixed magnitude: per 32-block scales 2^-40 .. 2^40, zero blocks, bf16 subnormals,
    values near the bf16 maximum, negative values"""
    x = rng.standard_normal((rows, c)).astype(np.float32)
    x *= np.exp2(rng.integers(-40, 40, (rows, c // 32, 1))).repeat(32, -1).reshape(rows, c).astype(np.float32)
    x[rng.random((rows, c)) < 0.05] = 0.0
    blk = x.reshape(rows, c // 32, 32)
    blk[rng.random((rows, c // 32)) < 0.1] = 0.0                                      # zero blocks
    x[0, :32] = np.float32(2.0 ** -130) * np.arange(32)                               # bf16 subnormals
    x[-1, -32:] = np.float32(3.0e38) * np.where(np.arange(32) % 2, 1, -1)             # huge
    return pack.bf16_bits_to_f32(_bf16_bits(x))


def _quantize_dev(x_f32, ldq, gamma=None, beta=None, eps=0.0):
    rows, c = x_f32.shape
    x = torch.from_numpy(_bf16_bits(x_f32).view(np.int16)).cuda()
    q = torch.full((rows, ldq), 0x55, dtype=torch.uint8, device="cuda")
    s = torch.full((rows, ldq // 32), 0x55, dtype=torch.uint8, device="cuda")
    g = None if gamma is None else torch.from_numpy(gamma).cuda()
    b = None if beta is None else torch.from_numpy(beta).cuda()
    ffi.check(ffi.lib.tfimm_hip_quantize_mx(x.data_ptr(), rows, c, c, None if g is None else g.data_ptr(),
                                            None if b is None else b.data_ptr(), eps, q.data_ptr(), s.data_ptr(), ldq,
                                            _stream()), "quantize_mx")
    torch.cuda.synchronize()
    return q.cpu().numpy(), s.cpu().numpy()


@pytest.mark.parametrize("rows,c", [(37, 96), (5, 768), (130, 3072), (3, 4096)])
def test_quantize_mx_bit_exact(rows, c):
    x = _mixed_rows(np.random.default_rng(rows + c), rows, c)
    ldq = pack.ceil_to(c, 128)
    q, s = _quantize_dev(x, ldq)
    wq, ws = pack.mx_quantize(x)
    np.testing.assert_array_equal(q[:, :c], wq)
    np.testing.assert_array_equal(s[:, : c // 32], ws)
    assert not q[:, c:].any() and not s[:, c // 32:].any()       # zero K padding


@pytest.mark.parametrize("rows,c", [(19, 256), (4, 2048)])
def test_quantize_mx_with_layernorm_bit_exact(rows, c):
    """rows 3 +- 1 with balanced signs: mean 3 and variance 1 are exact in fp32 (C a power of two, eps = 0), so the
    normalised value is exactly +-1 and y = fma(+-1, gamma, beta) -- gamma / beta of mixed magnitude -- is reproducible
    on the host (one rounding of the exact fp64 sum)"""
    rng = np.random.default_rng(c)
    sgn = np.tile(np.r_[np.ones(c // 2), -np.ones(c // 2)], (rows, 1))
    sgn = rng.permuted(sgn, axis=1).astype(np.float32)
    x = (3.0 + sgn).astype(np.float32)
    gamma = (rng.standard_normal(c) * np.exp2(rng.integers(-20, 20, c))).astype(np.float32)
    gamma[:32] = 0.0
    beta = (rng.standard_normal(c) * np.exp2(rng.integers(-20, 5, c))).astype(np.float32)
    q, s = _quantize_dev(x, c, gamma, beta, 0.0)
    y = (sgn.astype(np.float64) * gamma + beta).astype(np.float32)
    wq, ws = pack.mx_quantize(y)
    np.testing.assert_array_equal(s, ws)
    np.testing.assert_array_equal(q, wq)


LN_GPU_CASES = [(rows, c, eps) for rows, c in [(37, 32), (130, 96), (19, 192), (66, 384), (5, 480), (43, 544), (130, 768),
                                                 (7, 1536), (9, 2560), (13, 4096)] for eps in (1e-5, 1e-6)]


@pytest.mark.parametrize("rows,c,eps", LN_GPU_CASES)
def test_quantize_mx_with_layernorm_against_fp64(rows, c, eps):
    """mixed-sigma, far-from-zero, constant and zero rows (test_fp8.ln_rows), rows not a multiple of 4, ldq > C: exact
    against the fp64 LayerNorm except where provably ambiguous (mx_checks.check_ln_quantize), y == beta on constant rows"""
    from test_fp8 import ln_rows
    x, g, b = ln_rows(rows, c, c + int(eps * 1e7))
    ldq = pack.ceil_to(c, 128) + 128
    q, s = _quantize_dev(x, ldq, g, b, eps)
    bad, exempt = mxc.check_ln_quantize(q, s, x, g, b, eps)
    assert bad == 0 and exempt <= mxc.LN_EXEMPT_CAP, (bad, exempt)
    want_c, want_s = pack.mx_quantize(np.tile(b, (2, 1)))
    np.testing.assert_array_equal(q[1:3, :c], want_c)                       # constant and all-zero rows: y == beta
    np.testing.assert_array_equal(s[1:3, : c // 32], want_s)
    assert (s[:, : c // 32][:, np.all(g.reshape(-1, 32) == 0, -1)] == 0).all()   # gamma = beta = 0: scale byte 0
    assert not q[:, c:].any() and not s[:, c // 32:].any()                  # zero padding up to ldq


def _gelu(v):
    from scipy.special import erf
    return 0.5 * v * (1.0 + erf(v / np.sqrt(2.0)))


def _act(v, act):
    return {"": v, "relu": np.maximum(v, 0), "gelu": _gelu(v), "swish": v / (1 + np.exp(-v)),
            "sigmoid": 1 / (1 + np.exp(-v)), "relu6": np.clip(v, 0, 6), "tanh": np.tanh(v)}[act]


def _spread_blocks(rng, x, lo=-20, hi=20):
    """every 32-block along the last axis of x with its own power-of-two scale in 2^lo .. 2^hi, and zero blocks in the
    middle of K: scale bytes far from 127 on both sides, and 0"""
    nb = x.shape[-1] // 32
    e = rng.integers(lo, hi + 1, x.shape[:-1] + (nb, 1)).astype(np.float64)
    e[rng.random(e.shape) < 0.05] = -np.inf
    e[..., nb // 2, :] = -np.inf                                            # a zero block in the middle of K
    return (x.reshape(x.shape[:-1] + (nb, 32)) * np.exp2(e)).reshape(x.shape).astype(np.float32)


def _gemm_case(M, N, K, *, bias=True, act="", residual=False, act_after_res=False, out_fmt=0, seed=0, spread=False):
    rng = np.random.default_rng(seed + M + N + K)
    kp = pack.ceil_to(K, 128)
    a_f = (rng.standard_normal((M, K)) * np.exp2(rng.integers(-3, 3, (M, 1)))).astype(np.float32)
    if spread:
        a_f = _spread_blocks(rng, a_f)
    a_q, a_s = pack.mx_quantize(a_f)
    a = np.zeros((M, kp), np.uint8); a[:, :K] = a_q
    a_sc = np.zeros((M, kp // 32), np.uint8); a_sc[:, : K // 32] = a_s
    # an asymmetric weight (columns of different magnitude) catches a row <-> column swap of the lane maps
    w_f = (rng.standard_normal((K, N)) * 0.05 * (1 + np.arange(N) / N)).astype(np.float32)
    if spread:
        w_f = np.ascontiguousarray(_spread_blocks(rng, np.ascontiguousarray(w_f.T)).T)
    w, w_sc = pack.pack_dense_mx(w_f)
    b = (rng.standard_normal(N)).astype(np.float32) if bias else None
    r = pack.bf16_bits_to_f32(_bf16_bits(rng.standard_normal((M, N)).astype(np.float32))) if residual else None
    A, Wd = pack.mx_dequantize(a[:, :K], a_sc), pack.mx_dequantize(w[:, :K], w_sc)
    acc = A @ Wd.T
    mag = np.abs(A) @ np.abs(Wd).T
    v = acc + (b if bias else 0)
    if not act_after_res:
        v = _act(v, act)
    if residual:
        v = v + r
    if act_after_res:
        v = _act(v, act)
    dev = {k: torch.from_numpy(np.ascontiguousarray(t)).cuda() for k, t in
           (("a", a), ("as", a_sc), ("w", w), ("ws", w_sc))}
    d = ffi.GemmMxDesc()
    d.a, d.a_scale, d.w, d.w_scale = dev["a"].data_ptr(), dev["as"].data_ptr(), dev["w"].data_ptr(), dev["ws"].data_ptr()
    keep = []
    if bias:
        keep.append(torch.from_numpy(b).cuda()); d.bias = keep[-1].data_ptr()
    if residual:
        keep.append(torch.from_numpy(_bf16_bits(r).view(np.int16)).cuda()); d.residual = keep[-1].data_ptr(); d.ldr = N
    if out_fmt == 2:
        out = torch.full((M, N), 0x55, dtype=torch.uint8, device="cuda")
        osc = torch.full((M, N // 32), 0x55, dtype=torch.uint8, device="cuda")
        d.out_scale = osc.data_ptr()
    else:
        out = torch.full((M, N), float("nan"), dtype=torch.float32 if out_fmt == 1 else torch.bfloat16, device="cuda")
    d.out = out.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldw, d.ldc = M, N, K, kp, kp, N
    d.out_fmt, d.act, d.act_after_res = out_fmt, ffi.ACT[act], int(act_after_res)
    ffi.check(ffi.lib.tfimm_hip_gemm_mx(C.byref(d), _stream()), "gemm_mx")
    torch.cuda.synchronize()
    tol = mxc.gemm_tol(mag, v, act, b, r)
    if out_fmt == 2:
        return out.cpu().numpy(), osc.cpu().numpy(), v, tol
    return out.float().cpu().numpy(), None, v, tol


@pytest.mark.parametrize("M,N,K", [(1, 32, 32), (300, 96, 96), (513, 288, 800), (64, 2304, 768), (700, 768, 3072)])
def test_gemm_mx_ragged_shapes(M, N, K):
    for out_fmt in (0, 1):
        got, _, ref, tol = _gemm_case(M, N, K, out_fmt=out_fmt)
        tol = mxc.bf16_tol(ref, tol) if out_fmt == 0 else tol
        bad = np.abs(got - ref) > tol
        assert not bad.any(), (out_fmt, int(bad.sum()), np.argwhere(bad)[:5], float((np.abs(got - ref) / tol).max()))


@pytest.mark.parametrize("M,N,K", [(256, 256, 256), (257, 288, 800), (300, 96, 1536)])
def test_gemm_mx_scales_spread_over_the_e8m0_range(M, N, K):
    """each 32-block of A and of W with its own scale, 2^-20 .. 2^20, and zero blocks in the middle of K"""
    got, _, ref, tol = _gemm_case(M, N, K, out_fmt=1, spread=True, seed=11)
    bad = np.abs(got - ref) > tol
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5], float((np.abs(got - ref) / tol).max()))


@pytest.mark.parametrize("M,N,K", [(256, 768, 768), (257, 768, 768), (3152, 3072, 768)])
def test_gemm_mx_tile_counts(M, N, K):
    """M = 256 / 257: one full row of tiles and one row more; 3152 x 3072 (ViT fc1 at batch 16): 156 tiles over the XCD
    remap, more than one per XCD slot with a remainder"""
    got, _, ref, tol = _gemm_case(M, N, K, act="gelu", residual=M != 3152, out_fmt=0, seed=5)
    bad = np.abs(got - ref) > mxc.bf16_tol(ref, tol)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5])


@pytest.mark.parametrize("act", ["relu", "gelu", "swish", "sigmoid", "relu6", "tanh"])
@pytest.mark.parametrize("residual,after", [(False, False), (True, False), (True, True)])
def test_gemm_mx_epilogues(act, residual, after):
    got, _, ref, tol = _gemm_case(200, 160, 224, act=act, residual=residual, act_after_res=after, out_fmt=1, seed=7)
    bad = np.abs(got - ref) > tol + (1e-6 if act in ("swish", "sigmoid", "tanh") else 0)
    assert not bad.any(), (int(bad.sum()), np.abs(got - ref).max())
    got16, _, _, _ = _gemm_case(200, 160, 224, act=act, residual=residual, act_after_res=after, out_fmt=0, seed=7)
    # bf16 output: the fp32 result rounded to nearest even (common.h pack_bf2) -- the fp32 kernel output, rounded here
    np.testing.assert_array_equal(_bf16_bits(got16.astype(np.float32)), _bf16_bits(got))


@pytest.mark.parametrize("M,N,K,act", [(333, 384, 96, "gelu"), (96, 3072, 768, "gelu"), (64, 256, 128, "")])
def test_gemm_mx_mxfp8_output(M, N, K, act):
    codes, scales, ref, tol = _gemm_case(M, N, K, act=act, out_fmt=2, seed=3)
    fails, _ = mxc.check_mxfp8_output(codes, scales, ref, tol)
    assert not fails, fails


def test_gemm_mx_refuses_bad_descriptors_before_launch():
    d = ffi.GemmMxDesc()
    assert ffi.lib.tfimm_hip_gemm_mx(C.byref(d), None) == -1
    assert ffi.lib.tfimm_hip_quantize_mx(None, 1, 32, 32, None, None, 0.0, None, None, 128, None) == -1


# ---- models --------------------------------------------------------------------------------------------------------------
HEADS = ("head", "head_dist", "pre_logits/fc")


@contextlib.contextmanager
def mx_emulated_oracle():
    """oracle.common.W.dense with both operands run through the shared MX rule (x per row along K, the kernel per output
    column along K); the classifier layers stay plain fp32, as in the engine"""
    from oracle import ops
    orig = oracle.common.W.dense

    def q(a, axis):
        a = np.moveaxis(np.asarray(a, np.float32), axis, -1)
        c, s = pack.mx_quantize(a)
        return np.moveaxis(pack.mx_dequantize(c, s).astype(np.float32), -1, axis)

    def dense(self, x, prefix, bias=True):
        if prefix.split("/")[-1] in HEADS or prefix in HEADS or prefix.endswith("pre_logits/fc"):
            return orig(self, x, prefix, bias)
        k = self(prefix + "/kernel")
        xq = torch.from_numpy(q(x.detach().numpy(), -1))
        kq = torch.from_numpy(q(k.detach().numpy(), 0))
        return ops.dense(xq, kq, self(prefix + "/bias") if bias else None)

    oracle.common.W.dense = dense
    try:
        yield
    finally:
        oracle.common.W.dense = orig


def model_devs(name, batch, emulate, features=False):
    """{"fp8_vs_emulated": ..., "fp8_vs_fp32": ..., "bf16_vs_fp32": ...} (rel-to-max, logits and, for ViT, features)"""
    model = tfimm.create_model(name)
    w = synthetic_weights(model, 2021)
    model.set_weights(w)
    x = mc.make_input(model.cfg, batch, 2021)
    ref = oracle.forward(model.cfg, w, x, return_features=features)
    out = {}
    with precision.use("fp8"):
        got = model(x, return_features=features)
    with precision.use("bf16"):
        got16 = model(x)
    r32 = ref[0] if features else ref
    g8 = got[0] if features else got
    out["fp8_vs_fp32"] = mc.rel_err(g8.numpy().reshape(r32.shape), r32)
    out["bf16_vs_fp32"] = mc.rel_err(got16.numpy().reshape(r32.shape), r32)
    if emulate:
        with mx_emulated_oracle():
            em = oracle.forward(model.cfg, w, x, return_features=features)
        e32 = em[0] if features else em
        out["fp8_vs_emulated"] = mc.rel_err(g8.numpy().reshape(e32.shape), e32)
        if features:
            out["features_vs_emulated"] = mc.rel_err(got[1]["features"].numpy().reshape(em[1]["features"].shape),
                                                     em[1]["features"])
    return out


def _bars():
    with open(BARS) as f:
        return json.load(f)


MODELS = [("vit_base_patch16_224", 2, True), ("deit_base_distilled_patch16_224", 2, True),
          ("swin_tiny_patch4_window7_224", 2, False), ("cait_xxs24_224", 2, False), ("convnext_tiny", 2, False)]


@pytest.mark.parametrize("name,batch,emulate", MODELS)
def test_model_fp8_against_bars(name, batch, emulate):
    bars = _bars()[name]
    got = model_devs(name, batch, emulate, features=emulate)
    for k, bar in bars["bars"].items():
        assert got[k] <= bar, (name, k, got[k], bar, bars["observed"])


def test_resnet50_fp8_is_bf16():
    model = tfimm.create_model("resnet50")
    model.set_weights(synthetic_weights(model, 2021))
    x = mc.make_input(model.cfg, 2, 2021)
    with precision.use("bf16"):
        a = model(x).numpy()
        p16 = model.program()
    with precision.use("fp8"):
        b = model(x).numpy()
        p8 = model.program()
    assert [o.kind for o in p8.ops] == [o.kind for o in p16.ops]
    np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


def test_fp8_graph_replay_and_branches_are_bit_equal():
    model = tfimm.create_model("vit_tiny_patch16_224")
    model.set_weights(synthetic_weights(model, 2021))
    x = torch.from_numpy(mc.make_input(model.cfg, 4, 2021)).cuda()
    with precision.use("fp8"):
        prog = model.program()
        assert any(o.kind == "gemm_mx" for o in prog.ops)
        eager = model(x).torch().float().cpu().numpy()          # first call: eager launches
        graph = model(x).torch().float().cpu().numpy()          # second: captured graph
        graph2 = model(x).torch().float().cpu().numpy()         # replay
        np.testing.assert_array_equal(eager, graph)
        np.testing.assert_array_equal(eager, graph2)
        model.branches = 2
        try:
            for _ in range(3):
                np.testing.assert_array_equal(model(x).torch().float().cpu().numpy(), eager)
        finally:
            model.branches = 1


def test_fp8_plan_through_c_host(tmp_path):
    model = tfimm.create_model("vit_tiny_patch16_224")
    model.set_weights(synthetic_weights(model, 2021))
    x = torch.from_numpy(mc.make_input(model.cfg, 3, 2021)).cuda()
    with precision.use("fp8"):
        want = model(x).torch().float().cpu().numpy()
        blob = model.program().make_plan(3).export()
    bp, xp, op = tmp_path / "plan.bin", tmp_path / "x.bin", tmp_path / "out.bin"
    bp.write_bytes(blob)
    xp.write_bytes(x.cpu().numpy().astype(np.float32).tobytes())
    r = subprocess.run([HOST, str(bp), str(xp), str(op)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.frombuffer(op.read_bytes(), dtype=np.float32).reshape(want.shape)
    np.testing.assert_array_equal(got, want)


# ---- every quant_mx / gemm_mx op of real fp8 programs, teacher-forced ------------------------------------------------------
# (quant_mx, of them with LayerNorm, gemm_mx, of them with MXFP8 output, of them whose packed weight is the named kernel's:
# the others carry a folded LayerScale or a kernel derived on the host)
PER_OP_COUNTS = {"vit_base_patch16_224": (36, 24, 48, 12, 48), "deit_base_distilled_patch16_224": (36, 24, 48, 12, 48),
                 "swin_tiny_patch4_window7_224": (39, 24, 51, 12, 51), "cait_xxs24_224": (76, 48, 100, 24, 50),
                 "convnext_tiny": (18, 18, 36, 18, 18)}


def _read_bf16(plan, t):
    return plan.tensor_view(t).float().cpu().numpy().reshape(plan.batch * t.rows, t.C).astype(np.float64)


def _read_mx(plan, t):
    """(codes [B rows, mx_ld], scale bytes [B rows, mx_ld / 32]): the scales follow the whole batch's elements"""
    n = plan.batch * t.rows
    slab = plan.slabs[plan.assign[t.id]]
    e = slab[: n * t.mx_ld].cpu().numpy().reshape(n, t.mx_ld)
    s = slab[n * t.mx_ld: n * t.mx_ld + n * (t.mx_ld // 32)].cpu().numpy().reshape(n, t.mx_ld // 32)
    return e, s


def _const(prog, cid):
    return prog._dev_consts[cid].cpu().numpy()


@pytest.mark.parametrize("name", list(PER_OP_COUNTS))
def test_fp8_program_op_by_op(name):
    """The fp8 program at batch 2 with every quant_mx / gemm_mx input and output kept (after lowering, so fuse_mx_outputs
    fused as in production); each op checked against a reference built from its own read-back inputs:
    quant_mx bit-exact (mx_checks.check_ln_quantize with LayerNorm, gamma / beta / eps from the model's weights and config),
    gemm_mx against the fp64 product of the dequantized read-back A and the device's packed W (mx_checks.gemm_tol, bf16 or
    MXFP8 output).  The instrumented plan's logits equal model(x) bit for bit."""
    model = tfimm.create_model(name)
    w = synthetic_weights(model, 2021)
    model.set_weights(w)
    x = mc.make_input(model.cfg, 2, 2021)
    eps = oracle.common.LN_EPS[model.cfg.norm_layer]
    with precision.use("fp8"):
        want = model(x).numpy()
        prog = model.program()
    ops = [op for op in prog.ops if op.kind in ("quant_mx", "gemm_mx")]
    qs = [op for op in ops if op.kind == "quant_mx"]
    gs = [op for op in ops if op.kind == "gemm_mx"]
    last_write = {}
    for i, op in enumerate(prog.ops):
        for t in ([op.output] if op.output is not None else []) + list(op.extra_outputs):
            last_write[t] = i
    for i, op in enumerate(prog.ops):
        if op.kind in ("quant_mx", "gemm_mx"):
            for t in op.inputs + [op.output]:
                prog.tensors[t].keep = True
                assert last_write[t] <= i, (name, op.kind, prog.tensors[t].name)   # read back = what the op saw
    plan = prog.make_plan(2)
    xd = torch.from_numpy(x).cuda()
    plan.run(xd)
    torch.cuda.synchronize()
    got = plan.tensor_view(prog.outputs["logits"]).float().cpu().numpy().reshape(want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))

    n_ln = n_mxo = n_packed = 0
    worst_g, worst_o, exempt = 0.0, 0.0, 0.0
    for op in qs:
        xin, (q, s) = _read_bf16(plan, prog.tensors[op.inputs[0]]), _read_mx(plan, prog.tensors[op.output])
        C = op.attrs["C"]
        assert not q[:, C:].any() and not s[:, C // 32:].any(), (name, "padding")
        if op.attrs["ln"]:
            n_ln += 1
            layer = prog.consts[op.consts["gamma"]].name.rsplit("/", 1)[0]
            g, b = np.asarray(w[layer + "/gamma"], np.float32), np.asarray(w[layer + "/beta"], np.float32)
            bad, ex = mxc.check_ln_quantize(q, s, xin, g, b, eps)
            assert bad == 0, (name, layer, bad)
            exempt = max(exempt, ex)
        else:
            wc, ws = pack.mx_quantize(xin.astype(np.float32))
            nbad = int((q[:, :C] != wc).sum() + (s[:, : C // 32] != ws).sum())
            assert nbad == 0, (name, op.cite, nbad)
    assert exempt <= mxc.LN_EXEMPT_CAP, (name, exempt)
    for op in gs:
        a = op.attrs
        K, N = a["K"], a["N"]
        ac, asc = _read_mx(plan, prog.tensors[op.inputs[0]])
        wc, wsc = _const(prog, op.consts["w"]), _const(prog, op.consts["w_scale"])
        kname = prog.consts[op.consts["w"]].name[: -len(":mx")]
        if kname in w:
            k = np.asarray(w[kname], np.float32)
            pw, pws = pack.pack_dense_mx(k[0, 0] if k.ndim == 4 else k)
            n_packed += int(np.array_equal(pw, wc) and np.array_equal(pws, wsc))
        A, Wd = pack.mx_dequantize(ac[:, :K], asc), pack.mx_dequantize(wc[:, :K], wsc)
        v = A @ Wd.T
        mag = np.abs(A) @ np.abs(Wd).T
        bias = _const(prog, op.consts["bias"]).astype(np.float64) if "bias" in op.consts else None
        if bias is not None:
            v = v + bias
        v = _act(v, a["act"])
        r = _read_bf16(plan, prog.tensors[op.inputs[1]]) if a["has_residual"] else None
        if r is not None:
            v = v + r
        tol = mxc.gemm_tol(mag, v, a["act"], bias, r)
        out_t = prog.tensors[op.output]
        if a["out_fmt"] == 2:
            n_mxo += 1
            oc, osc = _read_mx(plan, out_t)
            fails, ratio = mxc.check_mxfp8_output(oc, osc, v, tol)
            assert not fails, (name, kname, fails)
            worst_o = max(worst_o, ratio)
        else:
            assert a["out_fmt"] == 0
            o = _read_bf16(plan, out_t)
            lim = mxc.bf16_tol(v, tol)
            ratio = float((np.abs(o - v) / lim).max())
            assert ratio <= 1.0, (name, kname, ratio, int((np.abs(o - v) > lim).sum()))
            worst_g = max(worst_g, ratio)
    assert (len(qs), n_ln, len(gs), n_mxo, n_packed) == PER_OP_COUNTS[name]
    measured = {"ln_exempt_max": round(exempt, 6), "gemm_bf16_worst_ratio": round(worst_g, 4),
                "gemm_mxfp8_worst_ratio": round(worst_o, 4)}
    print("PER_OP", json.dumps({name: measured}))

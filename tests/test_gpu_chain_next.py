"""pytest -m gpu: tfimm_hip_conv_chain_next -- the stage-1 bottleneck tail with the following block's conv1 as a second
output of the launch -- against the two-launch path of the same library (tfimm_hip_conv_chain, then tfimm_hip_gemm).

The first output is the tail's and must be bit-equal.  The second is a 256-deep fp32 sum in another order with one rounding to
bf16: held to the STAGED bar of hip_checks (2 ulps + 2^-14 rms element-wise; at most 0.5 % of the elements beyond it, none
beyond 2 ulps + 2^-8 rms) against the GEMM launch, and against the float64 product of the stored bf16 first output."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hip_checks
import test_architectures  # noqa: F401

pytestmark = pytest.mark.gpu

# (B, H, W): less than one tile, rows >= M | ragged last tile, image borders inside tiles | the workload's row width |
# 515 tiles on 512 workgroup slots: some workgroups run a second tile (acc3 and the first-tile waits cross a tile boundary)
SHAPES = [(1, 7, 7), (3, 12, 12), (2, 56, 56), (21, 56, 56)]


@functools.lru_cache(maxsize=None)
def _case(B, Hh, Ww):
    import hip_ops_chain as HC
    c = HC.make_case(B, Hh, Ww, 4000 + B)
    ref = HC.run_two_launches(c)
    return c, tuple(t.clone() for t in ref)


def _f64_next(out, c):
    """relu(out . W3^T + b3) in float64 from the stored bf16 values"""
    w3 = c["wt3"].double()[:, :c["N2"]]
    return torch.relu(out.double() @ w3.t() + c["b3"].double()).cpu().numpy()


@pytest.mark.parametrize("B,Hh,Ww", SHAPES)
def test_both_outputs_against_the_two_launch_path(B, Hh, Ww):
    import hip_ops_chain as HC
    c, (ref, ref2) = _case(B, Hh, Ww)
    out, out2 = HC.run_next(c)
    assert out.shape == ref.shape and out2.shape == (B * Hh * Ww, 64)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), "the first output differs from tfimm_hip_conv_chain's"
    got2 = out2.float().cpu().numpy()
    vs_gemm, _ = hip_checks.tight_score(got2, ref2.float().cpu().numpy(), hip_checks.STAGED)
    vs_f64, _ = hip_checks.tight_score(got2, _f64_next(out, c), hip_checks.STAGED)
    gemm_f64, _ = hip_checks.tight_score(ref2.float().cpu().numpy(), _f64_next(ref, c), hip_checks.STAGED)
    print(f"chain_next {B}x{Hh}x{Ww}: vs gemm {vs_gemm:.3f}  vs float64 {vs_f64:.3f}  (gemm vs float64 {gemm_f64:.3f})")
    assert vs_gemm <= 1.0, f"second output vs tfimm_hip_gemm: {vs_gemm:.3f} of the STAGED bar"
    assert vs_f64 <= 1.0, f"second output vs float64: {vs_f64:.3f} of the STAGED bar"


@pytest.mark.parametrize("B,Hh,Ww", [(3, 12, 12), (21, 56, 56)])
def test_two_launches_give_the_same_bits(B, Hh, Ww):
    import hip_ops_chain as HC
    c, _ = _case(B, Hh, Ww)
    a, a2 = HC.run_next(c)
    b, b2 = HC.run_next(c)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(a2.view(torch.int16), b2.view(torch.int16))


def test_image_chunks_give_the_same_bits():
    """TFIMM_CHAIN_LIMIT (read once per process, hence the subprocess) at 2 MB: one 56 x 56 image per launch, the second
    output offset per chunk like the first"""
    import hip_ops_chain as HC
    c = HC.make_case(2, 56, 56, 4002)
    out, out2 = HC.run_next(c)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TFIMM_CHAIN_LIMIT=str(2 * 1000 * 1000),
               PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tensorflow-image-models_amd"), os.path.join(root, "tests")]))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "hip_ops_chain.py"), "2", "56", "56", "4002"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][-1].split()
    assert line[1:] == [HC.digest(out), HC.digest(out2)]


def test_shapes_that_are_not_built_are_refused():
    import hip_ops as H
    import hip_ops_chain as HC
    from tfimm.engine import pack
    c, _ = _case(1, 7, 7)
    kw = dict(OH=7, OW=7)
    args = (c["x"], c["wt1"], c["b1"], c["wt2"], c["b2"], c["res"], c["wt3"], c["b3"])
    assert HC.conv_chain_next(*args, act2="", check=False, **kw)[2] == -2                       # not relu
    assert HC.conv_chain_next(*args, N3=128, check=False, **kw)[2] == -2                        # a width that is not built
    ds_w = H.dev_bits(pack.pack_chain_ds(np.zeros((64, 256), np.float32)))
    no_res = args[:5] + (None,) + args[6:]
    assert HC.conv_chain_next(*no_res, ds_x=c["x"].reshape(-1, 64), ds_w=ds_w, check=False, **kw)[2] == -2   # shortcut flavour
    x128 = torch.zeros(1, 7, 7, 128, dtype=torch.bfloat16, device="cuda")
    w1 = torch.zeros(128, 1152, dtype=torch.bfloat16, device="cuda")
    w2 = torch.zeros(256, 128, dtype=torch.bfloat16, device="cuda")
    b128 = torch.zeros(128, dtype=torch.float32, device="cuda")
    assert HC.conv_chain_next(x128, w1, b128, w2, c["b2"], c["res"], c["wt3"], c["b3"], C1=128, check=False, **kw)[2] == -2


def _resnet50(seed=2021):
    import tfimm
    from tfimm.utils.init import synthetic_weights
    m = tfimm.create_model("resnet50")
    m.set_weights(synthetic_weights(m, seed))
    return m


def _logits(model, x):
    prog = model.program()
    plan = prog.make_plan(x.shape[0])
    plan.run(x)
    torch.cuda.synchronize()
    return prog, plan, plan.tensor_view(prog.outputs["logits"]).float().cpu().numpy().copy()


def test_resnet50_with_and_without_the_fold(monkeypatch):
    """batch 2: the logits of the plan that launches the pair once against today's call list within the model's bf16 bar; a
    graph replay, a two-branch recording and hybrid recordings cut in front of, between and behind the two ops give the
    eager run's bits"""
    import json
    import model_checks as mc
    from tfimm.engine.graph import CapturedBranches, CapturedHybrid
    bar = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bf16_bars.json")))["models"]["resnet50"]
    model = _resnet50()
    x = torch.from_numpy(mc.make_input(model.cfg, 2)).cuda().contiguous()
    prog, plan, eager = _logits(model, x)
    (pair,) = plan.fused_next
    assert prog.ops[pair].kind == "conv_chain" and prog.ops[pair + 1].kind == "gemm" and len(plan.calls) == len(prog.ops) - 1
    out_t = prog.outputs["logits"]
    rec = plan.capture(x)
    for _ in range(2):
        rec.replay()
    torch.cuda.synchronize()
    assert np.array_equal(plan.tensor_view(out_t).float().cpu().numpy(), eager)
    recs = [CapturedBranches(prog.make_branches(2, 2), x)] + [CapturedHybrid(prog, x, cut) for cut in (pair, pair + 1, pair + 2)]
    assert [r.full.fused_next == plan.fused_next for r in recs[1:]] == [True, False, True]
    for r in recs:
        for _ in range(2):
            r.replay()
        torch.cuda.synchronize()
        assert np.array_equal(r.output(out_t).float().cpu().numpy().reshape(eager.shape), eager)
    monkeypatch.setenv("TFIMM_NO_CHAIN_NEXT", "1")
    _, pplan, want = _logits(model, x)
    assert not pplan.fused_next and len(pplan.calls) == len(plan.calls) + 1
    err = mc.rel_err(eager, want)
    print(f"resnet50 logits, one launch vs two: rel-to-max {err:.3e} (bar {bar['logits_bar']})")
    assert err <= bar["logits_bar"]

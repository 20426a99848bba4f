"""The following block's conv1 computed by the plain stage-1 bottleneck tail's launch (tfimm_hip_conv_chain_next), checked
without a GPU.  The layer program keeps both ops -- the tail and the 1x1 convolution behind it; a PLAN launches the pair once
(engine/graph.py: Program.chain_next_pairs, Plan.fused_next) and places the convolution's output before the tail's inputs
are released."""
import ctypes

import test_architectures  # noqa: F401  (registers the miniature configs)
import tfimm
from tfimm.engine import ffi
from tfimm.utils.init import synthetic_weights


def _prog(name="resnet50", size=None, **kw):
    m = tfimm.create_model(name)
    m.set_weights(synthetic_weights(m))
    return m.program(*(size or m.cfg.input_size), **kw)


def _names(plan):
    return [fn if isinstance(fn, str) else getattr(fn, "__name__", "input") for fn, _ in plan.calls]


def test_resnet50_launches_exactly_one_gemm_fewer_and_the_switch_restores_the_call_list(monkeypatch):
    prog = _prog()
    kinds = [op.kind for op in prog.ops]
    # the program is today's: stem, conv1, tail (shortcut flavour), conv1, tail, conv1, tail, ...
    assert len(prog.ops) == 46 and kinds[:9] == ["cast_input", "stem_pool", "gemm", "conv_chain", "gemm", "conv_chain", "gemm",
                                                  "conv_chain", "gemm"]
    assert not any(op.extra_outputs for op in prog.ops) and abs(prog.flops_per_image() / 1e9 - 8.178) < 0.01
    # block 2's tail (plain flavour) and conv1 of block 3; not the first tail (shortcut convolution inside), not the last one
    # (its successor is conv1 of stage 2: 256 -> 128)
    assert prog.chain_next_pairs() == [5]
    gone = prog.ops[6]
    assert (gone.attrs["M"], gone.attrs["K"], gone.attrs["N"], gone.attrs["act"]) == (3136, 256, 64, "relu")
    plan = prog.make_plan(2, device="cpu")
    names = _names(plan)
    assert plan.fused_next == {5} and len(plan.calls) == 45 == plan.check_marshalling()
    assert names.count("tfimm_hip_conv_chain_next") == 1 and names.count("tfimm_hip_conv_chain") == 5
    # one entry per op, the paired convolution without a call of its own; everything else where it was
    assert plan.op_call_start == list(range(7)) + list(range(6, 45))
    assert names[3:8] == ["tfimm_hip_conv_chain", "tfimm_hip_gemm", "tfimm_hip_conv_chain_next", "tfimm_hip_conv_chain", "tfimm_hip_gemm"]
    monkeypatch.setenv("TFIMM_NO_CHAIN_NEXT", "1")
    assert prog.chain_next_pairs() == []
    plain = prog.make_plan(2, device="cpu")
    pnames = _names(plain)
    assert not plain.fused_next and len(plain.calls) == 46 and plain.op_call_start == list(range(46))
    assert pnames.count("tfimm_hip_gemm") == names.count("tfimm_hip_gemm") + 1 and "tfimm_hip_conv_chain_next" not in pnames
    assert pnames[:5] == names[:5] and pnames[7:] == names[6:]
    assert plain.assign == prog.plan_buffers()[0]


def test_the_paired_launch_takes_the_convolutions_own_operands():
    prog = _prog()
    plan = prog.make_plan(2, device="cpu")
    tail, conv1, nxt = prog.ops[5], prog.ops[6], prog.ops[7]
    assert conv1.inputs == [tail.output] and nxt.inputs == [conv1.output, tail.output]
    d = plan.calls[5][1][0]._obj
    assert isinstance(d, ffi.ChainNextDesc) and (d.N2, d.N3, d.ldw3, d.ldc2, d.C1, d.B) == (256, 64, 256, 64, 64, 2)
    assert d.w3 == plan.cptr(conv1.consts["wt"]) and d.b3 == plan.cptr(conv1.consts["bias"])
    assert d.out == plan.tptr(tail.output) and d.out2 == plan.tptr(conv1.output) and d.residual and not d.ds_x
    # the launch reads two tensors and writes two: four different slabs.  Placed op by op, the convolution's output would take
    # the slab of the tail's 64-channel input, which the tail's other workgroups are still reading
    assert len({plan.assign[t] for t in tail.inputs + [tail.output, conv1.output]}) == 4
    assert prog.plan_buffers()[0][conv1.output] in {prog.plan_buffers()[0][t] for t in tail.inputs}
    # the tail in front of the next pair of ops reads what that launch wrote
    d7 = plan.calls[6][1][0]._obj
    assert isinstance(d7, ffi.ChainDesc) and d7.x == d.out2 and d7.residual == d.out


def test_shapes_outside_the_kernel_keep_two_launches():
    assert _prog(size=(256, 256)).chain_next_pairs() == []          # rows of 64 pixels: no fused tail at all
    for name in ("resnet50_mini_test_model", "resnet18", "seresnet50", "resnet50_gn", "resnext50_32x4d", "wide_resnet50_2"):
        assert _prog(name).chain_next_pairs() == [], name
    assert _prog("resnet101").chain_next_pairs() == [5]             # the same stage 1
    assert _prog(want_features=True).chain_next_pairs() == [5]      # kept block outputs do not change the launch
    from tfimm.engine import precision
    with precision.use("fp32"):                                      # the verification path has no fusions
        assert _prog().chain_next_pairs() == []


def test_live_tensors_branches_and_a_cut_between_the_pair():
    prog = _prog()
    ops = prog.ops
    assert prog.supports_branches()
    written = set()
    for i, op in enumerate(ops):
        if i > 0:
            live = prog.live_across(i)
            assert live and set(live) <= written
            needed = {t for o in ops[i:] for t in o.inputs}
            assert all(t in needed or prog.tensors[t].keep for t in live)
        written.update(([op.output] if op.output is not None else []) + list(op.extra_outputs))
    # behind the pair: the block output (the next block's shortcut) and the next block's conv1 output
    assert set(prog.live_across(7)) == {ops[5].output, ops[6].output}
    # a recording cut between the two ops (CapturedHybrid passes its cut to every plan it builds) keeps them two launches,
    # so each part writes exactly what live_across says crosses the join; any other cut leaves the pair together
    assert prog.chain_next_pairs(split_at=6) == [] and prog.chain_next_pairs(split_at=5) == [5] == prog.chain_next_pairs(split_at=7)
    from tfimm.engine.graph import Plan
    cut = Plan(prog, 2, device="cpu", split_at=6)
    assert not cut.fused_next and cut.op_call_start == list(range(46))
    assert [p.fused_next for p in prog.make_branches(4, 2, device="cpu")] == [{5}, {5}]


def test_roctx_labels_name_both_ops_of_the_launch():
    plan = _prog().make_plan(2, device="cpu")
    labels = plan._roctx_labels()
    assert len(labels) == len(plan.calls)
    assert labels[5].startswith("5 conv_chain") and "+ gemm resnet.py:269-271" in labels[5] and labels[6].startswith("6 conv_chain")


def test_descriptor_layout_and_refusals_without_a_gpu():
    """tfimm_chain_next_desc = tfimm_chain_desc + (w3, b3, out2, N3, ldw3, ldc2); the ABI version stays: a new symbol, nothing
    that existed changed"""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfimm_hip.h")).read()
    body = hdr[hdr.index("typedef struct tfimm_chain_next_desc {"):hdr.index("} tfimm_chain_next_desc;")]
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body.split("{", 1)[1], flags=re.S))
    assert names == ["chain", "w3", "b3", "out2", "N3", "ldw3", "ldc2"]
    nchain = len(ffi.ChainDesc._fields_)
    assert ffi.ChainNextDesc._fields_[:nchain] == ffi.ChainDesc._fields_
    assert [f[0] for f in ffi.ChainNextDesc._fields_[nchain:]] == names[1:]
    assert ffi.ChainNextDesc.w3.offset == ctypes.sizeof(ffi.ChainDesc)        # the nested struct's size, tail padding included
    assert ctypes.sizeof(ffi.ChainNextDesc) == ctypes.sizeof(ffi.ChainDesc) + 3 * 8 + 3 * 4 + 4
    lib = ffi.lib
    assert lib.tfimm_hip_conv_chain_next(None, None) == -1
    d = ffi.ChainNextDesc()
    assert lib.tfimm_hip_conv_chain_next(ctypes.byref(d), None) == -1 and b"null" in lib.tfimm_hip_last_error()

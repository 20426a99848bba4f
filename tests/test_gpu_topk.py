"""pytest -m gpu: the output end on the device.  tfimm_hip_topk (csrc/topk.hip) against the written rule of
tests/topk_ref.py -- ``indices`` identical, ``values`` bit-equal, ``probs`` under a bar computed from the shape -- and
``Model.top_k`` through every input form ``Model.__call__`` takes, eager, recorded and replayed, and out of an exported plan."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import model_checks as mc
import test_architectures  # noqa: F401
import tfimm
import topk_ref as tr
from tfimm.engine import ffi
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 8          # elements behind every output buffer that a launch must leave alone


def launch(x, k, *, pad=0, shift=0, probs=True):
    """tfimm_hip_topk on the rows of ``x`` (float32 (B, N)) laid out with ``ld = N + pad`` from a base ``shift`` elements
    past a 16-byte boundary; the columns [N, ld) hold NaN -- a launch that read them would select them.  Returns
    (indices int32, values float32, probs float32 or None) as numpy arrays."""
    x = np.ascontiguousarray(x, f32)
    B, N = x.shape
    ld = N + pad
    host = np.full(shift + B * ld + 4, np.nan, f32)
    host[shift:shift + B * ld].reshape(B, ld)[:, :N] = x
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 16 == 0
    values = torch.full((B * k + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    indices = torch.full((B * k + GUARD,), -7, dtype=torch.int32, device="cuda")
    pr = torch.full((B * k + GUARD,), -7.0, dtype=torch.float32, device="cuda") if probs else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ffi.check(ffi.lib.tfimm_hip_topk(dev.data_ptr() + 4 * shift, ld, B, N, k, values.data_ptr(), indices.data_ptr(),
                                     pr.data_ptr() if probs else None, st), "tfimm_hip_topk")
    torch.cuda.synchronize()
    out = []
    for t in (indices, values, pr):
        if t is None:
            out.append(None)
            continue
        a = t.cpu().numpy()
        assert (a[B * k:] == -7).all(), "the launch wrote behind an output"
        out.append(a[:B * k].reshape(B, k))
    return tuple(out)


def check(x, k, **kw):
    """device == rule: indices identical, values bit-equal"""
    idx, values, pr = launch(x, k, **kw)
    want_idx, want_values, _ = tr.topk(x, k, probs=False)
    assert np.array_equal(idx, want_idx), (idx[idx != want_idx][:8], want_idx[idx != want_idx][:8])
    assert np.array_equal(tr.bits(values), tr.bits(want_values))
    return idx, values, pr


def _normal(seed, B, N):
    return np.random.default_rng(seed).standard_normal((B, N)).astype(f32)


# ---- op level: values and indices ------------------------------------------------------------------------------------------
SHAPES = {"common": (3, 1000, 5), "minimal": (1, 1, 1), "k_equals_n": (2, 37, 37), "ragged_last_round": (2, 257, 8),
          "21k_path": (2, 21843, 5), "limits": (1, 32768, 64)}


@pytest.mark.parametrize("case", list(SHAPES))
def test_shapes(case):
    B, N, k = SHAPES[case]
    check(_normal(len(case), B, N), k)
    check(_normal(len(case), B, N), k, probs=False)            # probs may be null


def test_all_equal_row_gives_the_first_columns():
    idx, _, _ = check(np.full((2, 300), -2.5, f32), 7)
    assert idx.tolist() == [list(range(7))] * 2


@pytest.mark.parametrize("c", [0, 63, 191, 255, 300, 743])
def test_equal_values_across_thread_wave_and_round_owners(c):
    """the same value at columns c, c + 1 (the next lane, or the next wave), c + 64 (another wave) and c + 256 (the same
    thread, its next column): as the row maximum and as a second tier below one larger entry"""
    x = np.random.default_rng(c).uniform(-1, 1, (2, 1100)).astype(f32)
    cols = [c, c + 1, c + 64, c + 256]
    x[0, cols] = 3.0
    x[1, cols] = 3.0
    x[1, 1050] = 4.0
    idx, _, _ = check(x, 6)
    assert idx[0, :4].tolist() == cols and idx[1, :5].tolist() == [1050] + cols


def test_signed_zeros_are_equal_and_keep_their_sign():
    rng = np.random.default_rng(5)
    x = -np.abs(rng.standard_normal((3, 600))).astype(f32) - f32(0.5)        # everything else is negative
    zeros = rng.choice(600, 40, replace=False)
    x[:, zeros[:20]] = 0.0
    x[:, zeros[20:]] = -0.0
    x[2] = np.where(np.arange(600) % 2 == 0, f32(-0.0), f32(0.0))           # nothing but zeros
    idx, values, _ = check(x, 45)
    assert idx[0, :40].tolist() == sorted(zeros.tolist())                   # by column, whatever the sign
    assert np.signbit(values[0, :40]).sum() == 20 and idx[2].tolist() == list(range(45))


def test_non_finite_rows_values_and_indices():
    """+inf, -inf, NaNs of either sign and any payload: values / indices follow the rule, probs may hold anything"""
    x = _normal(9, 4, 500)
    nans = np.array([0x7fc00000, 0xffc00001, 0x7f800123, 0xffffffff], np.uint32).view(f32)
    x[0, [7, 300, 301]] = [np.inf, np.inf, -np.inf]
    x[1, [499, 0, 256, 64]] = nans
    x[2, [100, 101, 102, 103, 104]] = [np.inf, nans[1], -np.inf, nans[3], np.inf]
    x[3, :] = -np.inf
    x[3, 250] = nans[2]
    idx, values, _ = check(x, 6)
    assert idx[0, :2].tolist() == [7, 300] and idx[1, :4].tolist() == [0, 64, 256, 499]
    assert idx[2, :4].tolist() == [101, 103, 100, 104] and idx[3].tolist() == [250, 0, 1, 2, 3, 4]
    assert tr.bits(values)[1, :4].tolist() == [0xffc00001, 0xffffffff, 0x7f800123, 0x7fc00000]
    check(x, 64)                                                            # the most rounds there are: deep into the -inf of row 3
    y = _normal(10, 2, 40)
    y[0, [3, 9]] = -np.inf
    y[1, [5, 6]] = [-np.inf, np.nan]
    idx, _, _ = check(y, 40)                                                # every column: -inf comes last, by column
    assert idx[0, -2:].tolist() == [3, 9] and idx[1, 0] == 6 and idx[1, -1] == 5


@pytest.mark.parametrize("pad, shift", [(3, 1), (0, 1), (1, 0), (2, 3), (5, 2)])
def test_padded_and_unaligned_rows(pad, shift):
    """ld = N + pad from a base 4 * shift bytes past a 16-byte boundary: rows start at every alignment, the 16-byte body
    moves, the columns behind N (NaN) are never read"""
    check(_normal(pad * 8 + shift, 5, 1000), 5, pad=pad, shift=shift)
    check(_normal(pad * 8 + shift + 1, 3, 6), 2, pad=pad, shift=shift)       # rows shorter than one 16-byte load and its head


def test_rows_are_independent_of_the_batch():
    x = np.random.default_rng(13).integers(-2, 3, (130, 10)).astype(f32)    # many ties
    idx, values, pr = check(x, 3)
    for b in range(130):
        i1, v1, p1 = launch(x[b:b + 1], 3)
        assert np.array_equal(i1[0], idx[b]) and np.array_equal(tr.bits(v1[0]), tr.bits(values[b]))
        assert np.array_equal(tr.bits(p1[0]), tr.bits(pr[b]))


def test_two_launches_are_bit_equal():
    x = np.random.default_rng(17).uniform(-8, 8, (3, 21843)).astype(f32)
    a, b = launch(x, 9), launch(x, 9)
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(tr.bits(a[1]), tr.bits(b[1])) and np.array_equal(tr.bits(a[2]), tr.bits(b[2]))


# ---- op level: probabilities -------------------------------------------------------------------------------------------------
T = 256            # threads per row: csrc/topk.hip kThreads
U = 2.0 ** -24     # unit roundoff of float32


def prob_bar(N):
    return (math.ceil(N / T) + math.log2(T) + 16 + 4) * U


@pytest.mark.parametrize("B, N, k", [(3, 1000, 5), (2, 37, 37), (2, 257, 8), (2, 21843, 5), (1, 32768, 64)])
def test_probabilities_within_the_bar_of_the_shape(B, N, k):
    """Rows with entries in [-8, 8], so that d = x - m lies in [-16, 0].  The device's float32 ``exp(v - m) / sum`` against the
    float64 softmax of tests/topk_ref.py, relative error at most

        (ceil(N / T) + log2 T + 16 + 4) u,        u = 2^-24, T = 256 threads per row:

    * ceil(N / T) + log2 T: the longest chain of additions a term of the sum passes through -- a thread adds its
      ceil(N / T) columns in ascending order, then six butterfly steps inside the wave and two levels over the four waves
      ((w0 + w1) + (w2 + w3)): log2 256 = 8.  All terms are positive, so each addition costs at most u of the sum;
    * 16 u = |d| u: the rounding of ``x - m`` moves the exponential by |d| u relative;
    * 2 u: expf;
    * 1 u: the division;
    * 1 u of slack.
    The summation order is the one the bar was written for (csrc/topk.hip); nothing measured enters it."""
    x = np.random.default_rng(N + k).uniform(-8, 8, (B, N)).astype(f32)
    idx, _, pr = check(x, k)
    want = tr.topk(x, k)[2]
    rel = np.abs(pr.astype(np.float64) - want) / want
    print(f"topk probs B={B} N={N} k={k}: max relative error {rel.max() / U:.2f} u, bar {prob_bar(N) / U:.0f} u")
    assert rel.max() <= prob_bar(N)
    assert (pr > 0).all() and (np.diff(pr, axis=1) <= 0).all()


# ---- model level ---------------------------------------------------------------------------------------------------------
MODELS = ["resnet_test_model_1", "vit_test_model"]      # one CNN, one transformer; 12 classes
BATCH, K = 4, 5


def _model(name):
    model = tfimm.create_model(name)
    model.set_weights(synthetic_weights(model, 2021))
    return model


def _same(a, b):
    return (np.array_equal(a.indices.numpy(), b.indices.numpy())
            and np.array_equal(tr.bits(a.values.numpy()), tr.bits(b.values.numpy()))
            and np.array_equal(tr.bits(a.probs.numpy()), tr.bits(b.probs.numpy())))


def _three_calls(model, make_x, logits):
    """eager, recording, replay: bit-equal to each other; indices and values = the rule applied to ``logits``; the
    probabilities = the kernel's own on those logits (its arithmetic is held to its bar at op level)"""
    got = [model.top_k(make_x(), K) for _ in range(3)]
    assert _same(got[0], got[1]) and _same(got[0], got[2])
    t = got[0]
    assert (t.indices.shape, t.values.shape, t.probs.shape) == ((BATCH, K),) * 3
    assert (t.indices.numpy().dtype, t.values.numpy().dtype, t.probs.numpy().dtype) == (np.int32, np.float32, np.float32)
    want_idx, want_values, _ = tr.topk(logits, K, probs=False)
    assert np.array_equal(t.indices.numpy(), want_idx)
    assert np.array_equal(tr.bits(t.values.numpy()), tr.bits(want_values))
    assert np.array_equal(tr.bits(t.probs.numpy()), tr.bits(launch(logits, K)[2]))
    return t


def _topk_keys(d):
    return [key for key in d if ("topk", K) in key]


@pytest.mark.parametrize("name", MODELS)
def test_model_top_k_eager_recorded_replayed_and_model_call_untouched(name):
    model = _model(name)
    x = mc.make_input(model.cfg, BATCH)
    before = model(x).numpy()
    plain_keys = (set(model._programs), set(model._plans))
    _three_calls(model, lambda: x, before)
    assert len(_topk_keys(model._programs)) == 1 and len(_topk_keys(model._plans)) == 1
    assert len(_topk_keys(model._captured)) == 1                               # one recording, made by the second call
    assert plain_keys[0] <= set(model._programs) and plain_keys[1] <= set(model._plans)
    assert model._plans[_topk_keys(model._plans)[0]].calls[-1][0].__name__ == "tfimm_hip_topk"
    for _ in range(3):                                                         # eager, recording, replay of the plain program
        assert np.array_equal(model(x).numpy(), before)
    assert _same(model.top_k(x.astype(np.float32), K), model.top_k(torch.from_numpy(x).cuda(), K))
    bf = torch.from_numpy(x).to(torch.bfloat16)
    assert np.array_equal(model.top_k(bf, K).indices.numpy(), tr.topk(model(bf).numpy(), K, probs=False)[0])


@pytest.mark.parametrize("name", MODELS)
def test_model_top_k_with_two_branches(name):
    model = _model(name)
    x = mc.make_input(model.cfg, BATCH)
    logits = model(x).numpy()
    one = model.top_k(x, K)
    model.branches = 2
    two = _three_calls(model, lambda: x, logits)
    assert _same(one, two) and any("branches" in key for key in _topk_keys(model._plans))
    assert np.array_equal(model(x).numpy(), logits)


@pytest.mark.parametrize("name", MODELS)
def test_model_top_k_through_deferred_uint8_resize(name):
    model = _model(name)
    pre = tfimm.create_preprocessing(name, defer=True, resize=True)
    u8 = np.random.default_rng(3).integers(0, 256, (BATCH, 40, 52, 3), dtype=np.uint8)
    logits = model(pre(u8)).numpy()
    _three_calls(model, lambda: pre(u8), logits)
    assert np.array_equal(model(pre(u8)).numpy(), logits)


@pytest.mark.parametrize("name, aa", [(MODELS[0], False), (MODELS[1], True)], ids=["resnet", "vit-antialias"])
def test_model_top_k_on_a_list_of_mixed_sizes(name, aa):
    model = _model(name)
    pre = tfimm.create_preprocessing(name, defer=True, resize=True, antialias=aa)
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(48, 56), (81, 35), (33, 90), (40, 40)]]
    logits = model(pre(imgs)).numpy()
    _three_calls(model, lambda: pre(imgs), logits)
    assert len([key for key in _topk_keys(model._captured) if ("src", "mixed") + (("antialias",) if aa else ()) in key]) == 1
    assert np.array_equal(model(pre(imgs)).numpy(), logits)


def test_distilled_model_answers_per_head():
    model = _model("deit_test_model")
    x = mc.make_input(model.cfg, BATCH)
    logits = model(x).numpy()
    assert logits.shape == (BATCH, 2, 12)
    t = model.top_k(x, 3)
    assert t.indices.shape == (BATCH, 2, 3)
    want_idx, want_values, _ = tr.topk(logits.reshape(BATCH * 2, 12), 3, probs=False)
    assert np.array_equal(t.indices.numpy().reshape(-1, 3), want_idx)
    assert np.array_equal(tr.bits(t.values.numpy()).reshape(-1, 3), tr.bits(want_values))


DTYPE_CODES = {0: (torch.bfloat16, 2), 1: (torch.float32, 4), 2: (torch.int32, 4)}      # tfimm_hip_plan_output


@pytest.mark.parametrize("name", MODELS)
def test_exported_top_k_plan_through_the_c_entry_points(name):
    """Plan.export() of a top_k plan, run by tfimm_hip_plan_create / _forward / _output with nothing of engine/graph.py
    involved: ``topk_indices`` comes back with dtype code 2 (int32) and the contents of ``Model.top_k``"""
    model = _model(name)
    x = torch.from_numpy(mc.make_input(model.cfg, BATCH)).cuda()
    want = model.top_k(x, K)
    blob = model.program(top_k=K).make_plan(BATCH).export()
    lib = ffi.lib
    info = ffi.PlanInfo()
    ffi.check(lib.tfimm_hip_plan_query(blob, len(blob), C.byref(info)), "plan_query")
    assert info.n_outputs == 5
    ws = torch.empty(int(info.workspace_bytes), dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h = C.c_void_p()
    ffi.check(lib.tfimm_hip_plan_create(blob, len(blob), ws.data_ptr(), st, C.byref(h)), "plan_create")
    try:
        ffi.check(lib.tfimm_hip_plan_forward(h, x.data_ptr(), 0, st), "plan_forward")
        torch.cuda.synchronize()
        got = {}
        for out, code in (("topk_indices", 2), ("topk_values", 1), ("topk_probs", 1), ("logits", 1)):
            ptr, rows, cols, dt = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int()
            ffi.check(lib.tfimm_hip_plan_output(h, out.encode(), C.byref(ptr), C.byref(rows), C.byref(cols), C.byref(dt)), out)
            assert dt.value == code and rows.value == BATCH, (out, dt.value, rows.value)
            dtype, size = DTYPE_CODES[dt.value]
            off = ptr.value - ws.data_ptr()
            got[out] = ws[off:off + rows.value * cols.value * size].view(dtype).cpu().numpy().reshape(rows.value, cols.value)
    finally:
        lib.tfimm_hip_plan_destroy(h)
    assert got["topk_indices"].dtype == np.int32 and got["topk_indices"].shape == (BATCH, K)
    assert np.array_equal(got["topk_indices"], want.indices.numpy())
    assert np.array_equal(tr.bits(got["topk_values"]), tr.bits(want.values.numpy()))
    assert np.array_equal(tr.bits(got["topk_probs"]), tr.bits(want.probs.numpy()))
    assert np.array_equal(got["logits"], model(x).numpy())

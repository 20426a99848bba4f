"""pytest -m gpu: the scoring end on the device.  tfimm_hip_score (csrc/score.hip) against the written rule of
tests/score_ref.py -- ``rank`` / ``pred`` identical, ``prob`` and ``loss`` under bars computed from the shape -- and against
tfimm_hip_topk on the same logits; the meter's integer state, exactly and whatever the split into batches; ``Model.evaluate``
through the input forms ``Model.__call__`` takes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import model_checks as mc
import score_ref as sr
import test_architectures  # noqa: F401
import tfimm
import topk_ref as tr
from tfimm.engine import ffi
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 8          # elements behind every output buffer that a launch must leave alone


def launch(x, labels, *, pad=0, shift=0, state=None, per_class=None, confusion=None):
    """tfimm_hip_score on the rows of ``x`` (float32 (B, N)) laid out with ``ld = N + pad`` from a base ``shift`` elements
    past a 16-byte boundary; the columns [N, ld) and the elements around the rows hold NaN -- a launch that read them would
    change ``rank`` or ``pred``.  ``state`` / ``per_class`` / ``confusion``: device tensors to accumulate into, or None."""
    x = np.ascontiguousarray(x, f32)
    B, N = x.shape
    ld = N + pad
    host = np.full(shift + B * ld + 4, np.nan, f32)
    host[shift:shift + B * ld].reshape(B, ld)[:, :N] = x
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 16 == 0
    y = torch.from_numpy(np.asarray(labels, np.int64).astype(np.int32)).cuda()
    assert y.shape == (B,)
    outs = [torch.full((B + GUARD,), -7, dtype=dt, device="cuda") for dt in (torch.float32, torch.int32, torch.int32, torch.float32)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    acc = [None if t is None else t.data_ptr() for t in (state, per_class, confusion)]
    ffi.check(ffi.lib.tfimm_hip_score(dev.data_ptr() + 4 * shift, ld, B, N, y.data_ptr(), *(t.data_ptr() for t in outs), *acc, st),
              "tfimm_hip_score")
    torch.cuda.synchronize()
    res = []
    for t in outs:
        a = t.cpu().numpy()
        assert (a[B:] == -7).all(), "the launch wrote behind an output"
        res.append(a[:B])
    return tuple(res)


def check(x, labels, **kw):
    """device == rule: rank and pred identical; ignored / invalid rows as specified"""
    loss, rank, pred, prob = launch(x, labels, **kw)
    _, want_rank, want_pred, _ = sr.score(x, labels)
    assert np.array_equal(rank, want_rank), (rank[rank != want_rank][:8], want_rank[rank != want_rank][:8])
    assert np.array_equal(pred, want_pred)
    off = want_rank < 0
    assert (tr.bits(loss[off]) == 0).all() and (tr.bits(prob[off]) == 0).all()      # +0.0, bit for bit
    return loss, rank, pred, prob


def _uniform(seed, B, N):
    return np.random.default_rng(seed).uniform(-8, 8, (B, N)).astype(f32)


def _placed_labels(x):
    """per row one of: column 0, 255, 256, N - 1 (clipped into the row) and the argmax, in turn -- every row of a small batch
    gets each of them through the offsets"""
    B, N = x.shape
    picks = [0, min(255, N - 1), min(256, N - 1), N - 1, None]
    return [[int(np.argmax(x[b])) if picks[(b + o) % 5] is None else picks[(b + o) % 5] for b in range(B)] for o in range(5)]


# ---- op level: rank, pred, prob, loss ------------------------------------------------------------------------------------
T = 256            # threads per row: csrc/topk_select.h kThreads
U = 2.0 ** -24     # unit roundoff of float32
SHAPES = {"common": (3, 1000), "minimal": (1, 1), "short": (2, 37), "ragged_last_round": (2, 257), "21k_path": (2, 21843),
          "limits": (1, 32768)}


def prob_bar(N):
    """tests/test_gpu_topk.py's bar, restated: the relative error of ``exp(v - m) / sum`` (the same arithmetic)"""
    return (math.ceil(N / T) + math.log2(T) + 16 + 4) * U


def loss_bar(N):
    """Absolute error of the float32 ``logf(sum) - (x_y - m)`` against float64 for entries in [-8, 8] (d = x - m in [-16, 0],
    1 <= sum <= N, so 0 <= log(sum) <= ln N):

        (ceil(N / T) + 8 + 16 + 2) u     relative error of ``sum`` -- the chain of additions a term passes through (a thread's
                                         ceil(N / T) columns, six butterfly steps, two levels over the waves), the rounding
                                         of ``x - m`` (|d| u <= 16 u relative on the exponential) and expf (2 u) -- which the
                                         logarithm turns into the same ABSOLUTE error
      + 2 u ln N                         logf: 2 u relative on a value of at most ln N
      + 16 u                             the rounding of ``x_y - m``: u relative on at most 16
      + (ln N + 16) u                    the final subtraction: u relative on a result of at most ln N + 16
      + 1 u                              slack.
    Nothing measured enters it."""
    ln = math.log(N)
    return ((math.ceil(N / T) + 8 + 16 + 2) + 2 * ln + 16 + (ln + 16) + 1) * U


@pytest.mark.parametrize("case", list(SHAPES))
def test_shapes_rank_pred_prob_and_loss(case):
    B, N = SHAPES[case]
    x = _uniform(len(case) + N, B, N)
    worst_p = worst_l = 0.0
    for labels in _placed_labels(x):
        loss, rank, pred, prob = check(x, labels)
        want_loss, _, _, want_prob = sr.score(x, labels)
        worst_p = max(worst_p, float((np.abs(prob.astype(np.float64) - want_prob) / want_prob).max()))
        worst_l = max(worst_l, float(np.abs(loss.astype(np.float64) - want_loss).max()))
        assert (loss >= 0).all() and not np.signbit(loss).any() and (prob > 0).all() and (prob <= 1).all()
        assert all(rank[b] == 0 for b in range(B) if labels[b] == pred[b])
    print(f"score B={B} N={N}: prob max relative error {worst_p / U:.2f} u, bar {prob_bar(N) / U:.0f} u; "
          f"loss max absolute error {worst_l / U:.2f} u, bar {loss_bar(N) / U:.1f} u")
    assert worst_p <= prob_bar(N)
    assert worst_l <= loss_bar(N)
    if N == 1:
        assert tr.bits(loss).tolist() == [0] and prob.tolist() == [1.0]            # exactly +0.0 and 1


def test_all_equal_row_ranks_every_label_by_its_column():
    N = 300
    x = np.full((N, N), -2.5, f32)
    _, rank, pred, _ = check(x, np.arange(N))
    assert rank.tolist() == list(range(N)) and pred.tolist() == [0] * N


@pytest.mark.parametrize("c", [0, 63, 191, 255, 300, 743])
def test_equal_values_across_thread_wave_and_round_owners(c):
    """the same value at columns c, c + 1 (the next lane, or the next wave), c + 64 (another wave) and c + 256 (the same
    thread, its next column): as the row maximum and as a second tier below one larger entry; every one of them as label"""
    cols = [c, c + 1, c + 64, c + 256]
    x = np.repeat(np.random.default_rng(c).uniform(-1, 1, (2, 1100)).astype(f32), 4, axis=0)      # rows 0-3 and 4-7
    x[:, cols] = 3.0
    x[4:, 1050] = 4.0
    _, rank, pred, _ = check(x, cols + cols)
    assert rank.tolist() == [0, 1, 2, 3, 1, 2, 3, 4] and pred.tolist() == [c] * 4 + [1050] * 4


def test_signed_zeros_are_equal():
    rng = np.random.default_rng(5)
    x = -np.abs(rng.standard_normal((3, 600))).astype(f32) - f32(0.5)        # everything else is negative
    zeros = np.sort(rng.choice(600, 40, replace=False))
    x[:, zeros[::2]] = 0.0
    x[:, zeros[1::2]] = -0.0
    x[2] = np.where(np.arange(600) % 2 == 0, f32(-0.0), f32(0.0))           # nothing but zeros
    loss, rank, pred, prob = check(x, [zeros[7], zeros[39], 599])
    assert rank.tolist() == [7, 39, 599] and pred.tolist() == [zeros[0], zeros[0], 0]
    assert abs(float(loss[2]) - math.log(600)) <= loss_bar(600) and abs(float(prob[2]) * 600 - 1) <= prob_bar(600)


def test_non_finite_rows_follow_the_rule_and_nothing_faults():
    """+inf, -inf, NaNs of either sign and any payload: rank / pred follow the rule, loss and prob may hold anything; the meter
    puts what is not below 1024 into loss_excluded and still counts the rank"""
    x = np.random.default_rng(9).standard_normal((5, 500)).astype(f32)
    nans = np.array([0x7fc00000, 0xffc00001, 0x7f800123, 0xffffffff], np.uint32).view(f32)
    x[0, [7, 300, 301]] = [np.inf, np.inf, -np.inf]
    x[1, [499, 0, 256, 64]] = nans
    x[2, [100, 101, 102, 103, 104]] = [np.inf, nans[1], -np.inf, nans[3], np.inf]
    x[3, :] = -np.inf
    x[3, 250] = nans[2]
    x[4, :] = -np.inf
    state = torch.zeros(sr.STATE_WORDS, dtype=torch.int64, device="cuda")
    for labels in ([300, 256, 104, 499, 3], [301, 5, 102, 250, 0], [7, 499, 101, 0, 499]):
        loss, rank, pred, _ = check(x, labels, state=state)
    assert rank.tolist() == [0, 3, 0, 1, 499] and pred.tolist() == [7, 0, 101, 250, 0]
    w = state.cpu().numpy()
    assert w[sr.SCORED] == 15 and w[sr.RANK_HIST:].sum() == 15
    assert w[sr.LOSS_EXCLUDED] >= 9 and w[sr.LOSS_Q] >= 0       # rows 1-3 hold a NaN: m is one, and so is every loss of theirs


def test_labels_outside_the_row_are_not_scored_and_read_nothing():
    x = _uniform(21, 6, 70)
    labels = [-1, -2, 70, 2 ** 31 - 1, -2 ** 31, 69]
    bufs = [torch.zeros(n, dtype=dt, device="cuda") for n, dt in ((sr.STATE_WORDS, torch.int64), (2 * 70, torch.int64), (70 * 70, torch.int32))]
    for pad, shift in ((0, 0), (3, 1)):
        loss, rank, pred, prob = check(x, labels, pad=pad, shift=shift, state=bufs[0], per_class=bufs[1], confusion=bufs[2])
        assert rank.tolist()[:5] == [-1, -2, -2, -2, -2] and rank[5] >= 0
        assert np.array_equal(pred, np.argmax(x, 1)) and loss[5] > 0 and prob[5] > 0          # pred is written for every row
    w = bufs[0].cpu().numpy()
    assert (w[sr.SCORED], w[sr.IGNORED], w[sr.INVALID]) == (2, 2, 8)
    pc, cm = bufs[1].cpu().numpy().reshape(2, 70), bufs[2].cpu().numpy().reshape(70, 70)
    assert pc[0].sum() == 2 and pc[0, 69] == 2 and cm.sum() == 2 and cm[69, int(np.argmax(x[5]))] == 2


@pytest.mark.parametrize("pad, shift", [(3, 1), (0, 1), (1, 0), (2, 3), (5, 2)])
def test_padded_and_unaligned_rows(pad, shift):
    """ld = N + pad from a base 4 * shift bytes past a 16-byte boundary: rows start at every alignment, the 16-byte body
    moves, the columns behind N (NaN) are never read"""
    x = _uniform(pad * 8 + shift, 5, 1000)
    plain = check(x, _placed_labels(x)[0])
    moved = check(x, _placed_labels(x)[0], pad=pad, shift=shift)
    assert all(np.array_equal(tr.bits(a), tr.bits(b)) if a.dtype == f32 else np.array_equal(a, b) for a, b in zip(plain, moved))
    y = _uniform(pad * 8 + shift + 1, 3, 6)                                  # rows shorter than one 16-byte load and its head
    check(y, [5, 0, 3], pad=pad, shift=shift)


def _same(a, b):
    return all(np.array_equal(tr.bits(u), tr.bits(v)) if u.dtype == f32 else np.array_equal(u, v) for u, v in zip(a, b))


def test_rows_are_independent_of_the_batch_and_two_launches_are_bit_equal():
    x = np.random.default_rng(13).integers(-2, 3, (130, 10)).astype(f32)    # many ties
    labels = np.random.default_rng(14).integers(0, 10, 130)
    whole = check(x, labels)
    assert _same(whole, launch(x, labels))
    for b in range(0, 130, 7):
        assert _same([a[b:b + 1] for a in whole], launch(x[b:b + 1], labels[b:b + 1]))
    big = _uniform(17, 3, 21843)
    assert _same(launch(big, [0, 21842, 256]), launch(big, [0, 21842, 256]))


def _topk(x, k):
    B, N = x.shape
    dev = torch.from_numpy(x).cuda()
    values = torch.empty((B, k), dtype=torch.float32, device="cuda")
    indices = torch.empty((B, k), dtype=torch.int32, device="cuda")
    probs = torch.empty((B, k), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ffi.check(ffi.lib.tfimm_hip_topk(dev.data_ptr(), N, B, N, k, values.data_ptr(), indices.data_ptr(), probs.data_ptr(), st),
              "tfimm_hip_topk")
    torch.cuda.synchronize()
    return indices.cpu().numpy(), probs.cpu().numpy()


@pytest.mark.parametrize("kind", ["uniform", "ties"])
def test_against_tfimm_hip_topk_on_the_same_logits(kind):
    """pred is the first index; the label is among the k indices exactly when rank < k, at position rank; prob has the bits
    of that kernel's probs[rank]"""
    rng = np.random.default_rng(23)
    B, N = 64, 1000
    x = _uniform(23, B, N) if kind == "uniform" else rng.integers(-3, 4, (B, N)).astype(f32)
    x[5, :] = np.where(np.arange(N) % 3 == 0, f32(0.0), f32(-0.0))          # zeros of both signs, m == 0
    order = np.stack([tr.order(r) for r in x])
    # labels at the ranks 0, 1, 4, 5, 63, 64, 999 and anywhere
    want = np.array([0, 1, 4, 5, 63, 64, 999, 500])[np.arange(B) % 8]
    labels = order[np.arange(B), want]
    loss, rank, pred, prob = check(x, labels)
    assert np.array_equal(rank, want)
    for k in (5, 64):
        idx, pr = _topk(x, k)
        assert np.array_equal(pred, idx[:, 0])
        hit = (idx == labels[:, None]).any(1)
        assert np.array_equal(rank < k, hit) and hit.any() and not hit.all()
        rows = np.nonzero(hit)[0]
        assert np.array_equal(idx[rows, rank[rows]], labels[rows])
        assert np.array_equal(tr.bits(prob[rows]), tr.bits(pr[rows, rank[rows]]))


# ---- the meter's state ---------------------------------------------------------------------------------------------------
def _meter_state(meter):
    s = meter.state()
    return [s.words] + [a for a in (s.per_class, s.confusion) if a is not None]


def _equal_states(a, b, but=()):
    a, b = [v.copy() for v in a], [v.copy() for v in b]
    for i in but:
        a[0][i] = b[0][i] = 0
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def test_state_after_one_launch_is_the_rule_applied_to_the_device_s_own_outputs():
    N = 37
    x = _uniform(31, 40, N)
    x[3, 5] = np.nan                                                         # a row whose loss is excluded
    x[4, :] = [2000.0 if c == 0 else 0.0 for c in range(N)]                  # a finite loss of 2000: excluded, too
    labels = np.random.default_rng(32).integers(0, N, 40)
    labels[[4, 7, 9, 11]] = [1, -1, N, -5]
    labels[20:30] = np.argmax(x[20:30], 1)
    meter = tfimm.Meter(N, per_class=True, confusion=True)
    s = meter.update(x, labels)
    loss, rank, pred, prob = (t.numpy() for t in s)
    assert loss.dtype == f32 and rank.dtype == np.int32 and pred.dtype == np.int32 and prob.dtype == f32
    assert _same((loss, rank, pred, prob), launch(x, labels))                # the Python path is the same launch
    words, per_class, confusion = sr.state(loss, rank, labels, N, pred)
    got = meter.state()
    assert np.array_equal(got.words, words) and got.words.shape == (70,)
    assert np.array_equal(got.per_class, per_class) and np.array_equal(got.confusion, confusion)
    assert (words[sr.SCORED], words[sr.IGNORED], words[sr.INVALID], words[sr.LOSS_EXCLUDED]) == (37, 1, 2, 2)
    r = meter.result()
    keep = (rank >= 0) & (loss < 1024)
    assert r.count == 37 and abs(r.loss - loss[keep].astype(np.float64).mean()) < 2.0 ** -32
    assert r.top1 == (rank == 0).sum() / 37 and r.accuracy(5) == ((rank >= 0) & (rank < 5)).sum() / 37
    assert np.array_equal(r.per_class_hits, per_class[1]) and r.top1 >= 10 / 37


def test_state_does_not_depend_on_the_split_the_order_or_ignored_padding():
    N = 21
    x = np.random.default_rng(41).integers(-2, 3, (12, N)).astype(f32) * f32(0.37)
    labels = np.random.default_rng(42).integers(0, N, 12)

    def run(parts):
        m = tfimm.Meter(N, per_class=True, confusion=True)
        for rows, lab in parts:
            m.update(rows, lab)
        return _meter_state(m)
    one = run([(x, labels)])
    assert one[0][sr.SCORED] == 12 and one[0][sr.LOSS_Q] > 0
    assert _equal_states(one, run([(x[:5], labels[:5]), (x[5:], labels[5:])]))
    assert _equal_states(one, run([(x[b:b + 1], labels[b:b + 1]) for b in range(12)]))
    assert _equal_states(one, run([(x[::-1].copy(), labels[::-1].copy())]))
    padded = run([(np.concatenate([x, x[:4]]), np.concatenate([labels, [-1] * 4]))])
    assert padded[0][sr.IGNORED] == 4 and one[0][sr.IGNORED] == 0
    assert _equal_states(one, padded, but=(sr.IGNORED,))
    # device-side labels and logits, int64 and int32, give the same state as host ones
    m = tfimm.Meter(N, per_class=True, confusion=True)
    m.update(torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda())
    assert _equal_states(one, _meter_state(m))
    m.reset()
    m.update(tfimm.Tensor(torch.from_numpy(x).cuda()), torch.from_numpy(labels.astype(np.int32)))
    assert _equal_states(one, _meter_state(m))


def test_contended_counters_are_exact():
    B, N = 4096, 8
    x = np.random.default_rng(51).uniform(-1, 1, (B, N)).astype(f32)
    x[:, 3] = 5.0                                                            # every argmax and every label: class 3
    meter = tfimm.Meter(N, per_class=True, confusion=True)
    s = meter.update(x, np.full(B, 3))
    got = meter.state()
    assert got.words[sr.SCORED] == B and got.words[sr.RANK_HIST] == B and got.words[sr.RANK_HIST:].sum() == B
    assert got.per_class[:, 3].tolist() == [B, B] and got.per_class.sum() == 2 * B
    assert got.confusion[3, 3] == B and got.confusion.sum() == B
    loss = s.loss.numpy()
    assert got.words[sr.LOSS_Q] == sum(int(np.rint(np.float64(v) * 2.0 ** 32)) for v in loss)
    assert got.words[[sr.IGNORED, sr.INVALID, sr.LOSS_EXCLUDED]].tolist() == [0, 0, 0]


def test_reset_zeroes_everything_and_merge_equals_one_meter_fed_both():
    N = 12
    x, labels = _uniform(61, 20, N), np.random.default_rng(62).integers(-1, N + 1, 20)
    a, b, both = (tfimm.Meter(N, per_class=True, confusion=True) for _ in range(3))
    a.update(x[:9], labels[:9])
    b.update(x[9:], labels[9:])
    both.update(x, labels)
    a.merge(b)
    assert _equal_states(_meter_state(a), _meter_state(both))
    once = _meter_state(b)
    b.merge(b.state())                                                       # the arrays of state(), too: b twice
    assert _equal_states(_meter_state(b), [2 * v for v in once])
    for m in (a, b):
        m.reset()
        assert not any(v.any() for v in _meter_state(m)) and m.result().count == 0
    a.update(x, labels)                                                      # and it counts again from zero
    assert _equal_states(_meter_state(a), _meter_state(both))


def test_score_without_a_meter_and_an_empty_batch():
    x, labels = _uniform(71, 5, 12), [0, 11, -1, 12, 3]
    s = tfimm.score(x, labels)
    assert _same([t.numpy() for t in s], launch(x, labels)) and s.loss.shape == (5,)
    e = tfimm.score(np.zeros((0, 12), f32), np.zeros(0, np.int64))
    assert e.loss.shape == (0,) and e.rank.numpy().dtype == np.int32
    wide = torch.from_numpy(_uniform(72, 4, 24)).cuda()[:, :12]              # a view with a row stride: made contiguous
    assert _same([t.numpy() for t in tfimm.score(wide, [1, 2, 3, 4])], launch(wide.cpu().numpy(), [1, 2, 3, 4]))


# ---- model level ---------------------------------------------------------------------------------------------------------
MODELS = ["resnet_test_model_1", "vit_test_model"]      # one CNN, one transformer; 12 classes
BATCH = 4
LABELS = [3, 11, -1, 0]


def _model(name):
    model = tfimm.create_model(name)
    model.set_weights(synthetic_weights(model, 2021))
    return model


def _np(s):
    return [t.numpy() for t in s]


def _evaluate_equals_score_of_the_logits(model, make_x):
    """eager, recording, replay: ``evaluate`` is bit-equal to ``tfimm.score(model(x), labels)`` every time, and adds no plan
    and no recording to what ``model(x)`` alone leaves"""
    logits = model(make_x())
    want = _np(tfimm.score(logits, LABELS))
    for _ in range(2):
        assert np.array_equal(model(make_x()).numpy(), logits.numpy())        # the recording and a replay exist now
    plans, captured = len(model._plans), len(model._captured)
    meter = tfimm.Meter(model.cfg.nb_classes)
    for i in range(3):
        got = model.evaluate(make_x(), LABELS, meter if i else None)
        assert _same(_np(got), want)
        assert got.loss.shape == (BATCH,) and got.rank.numpy()[2] == -1
    assert (len(model._plans), len(model._captured)) == (plans, captured)
    assert meter.result().count == 6 and meter.result().ignored == 2
    assert np.array_equal(model(make_x()).numpy(), logits.numpy())            # model(x) bits are unchanged afterwards
    return want


@pytest.mark.parametrize("name", MODELS)
def test_model_evaluate_float32_bf16_and_the_eager_first_call(name):
    model = _model(name)
    x = mc.make_input(model.cfg, BATCH)
    first = _np(model.evaluate(x, LABELS))                                    # eager: the model has run nothing yet
    assert _same(first, _evaluate_equals_score_of_the_logits(model, lambda: x))
    bf = torch.from_numpy(x).to(torch.bfloat16)
    _evaluate_equals_score_of_the_logits(model, lambda: bf)
    want_rank = sr.score(model(x).numpy(), LABELS)[1]
    assert np.array_equal(first[1], want_rank)


@pytest.mark.parametrize("name", MODELS)
def test_model_evaluate_with_two_branches_and_micro_batches(name):
    model = _model(name)
    x = mc.make_input(model.cfg, BATCH)
    plain = _np(model.evaluate(x, LABELS))
    model.branches = 2
    assert _same(plain, _evaluate_equals_score_of_the_logits(model, lambda: x))
    model.branches = 1
    model.micro_batch = 3
    assert _same(plain, _evaluate_equals_score_of_the_logits(model, lambda: x))


@pytest.mark.parametrize("name", MODELS)
def test_model_evaluate_through_deferred_resize_and_a_list_of_mixed_sizes(name):
    model = _model(name)
    pre = tfimm.create_preprocessing(name, defer=True, resize=True)
    u8 = np.random.default_rng(3).integers(0, 256, (BATCH, 40, 52, 3), dtype=np.uint8)
    _evaluate_equals_score_of_the_logits(model, lambda: pre(u8))
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(48, 56), (81, 35), (33, 90), (40, 40)]]
    _evaluate_equals_score_of_the_logits(model, lambda: pre(imgs))

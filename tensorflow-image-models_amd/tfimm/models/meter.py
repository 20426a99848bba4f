"""Scoring labelled batches on the device: ``tfimm.score``, ``tfimm.Meter`` and what they return (tfimm_hip_score,
csrc/score.hip).  The logits stay where ``model(x)`` left them; per sample four numbers come back, and a
``Meter`` accumulates accuracy@k, mean loss, per-class hits and a confusion matrix in device memory as integers, without
a host synchronisation per batch."""
import ctypes as C
from collections import namedtuple

import numpy as np

from .model import Tensor

#: what ``tfimm.score`` / ``Meter.update`` / ``Model.evaluate`` return: four ``Tensor`` of shape (B,) -- float32
#: cross-entropy, int32 rank of the true class (0 = it is the prediction; -1 ignored, -2 label out of range), int32 predicted
#: class, float32 softmax probability of the true class
Scores = namedtuple("Scores", ["loss", "rank", "pred", "prob"])

#: what ``Meter.state()`` returns and ``Meter.merge`` takes: numpy arrays -- int64 (SCORE_STATE_WORDS,), int64 (2, N) or None,
#: int64 (N, N) or None
MeterState = namedtuple("MeterState", ["words", "per_class", "confusion"])


def _consts():
    from ..engine import ffi
    return ffi


def _logits(x, nb_classes, what):
    """``x`` as a contiguous float32 device tensor (B, nb_classes): a ``Tensor`` or torch tensor on the GPU stays where it is,
    host data is uploaded (``Gallery._rows``).  Returns a callable that does the device part, so that every ``ValueError``
    comes first."""
    import torch
    if isinstance(x, Tensor):
        t = x.torch()
    elif isinstance(x, torch.Tensor):
        t = x
    else:
        t = np.asarray(x)
    if str(t.dtype).replace("torch.", "") != "float32":
        raise ValueError(f"{what}: logits: expected float32, got {t.dtype}")
    if t.ndim != 2 or (nb_classes is not None and t.shape[1] != nb_classes):
        raise ValueError(f"{what}: logits: expected shape (B, {'N' if nb_classes is None else nb_classes}), got {tuple(t.shape)}")
    n = int(t.shape[1])
    ffi = _consts()
    if not 1 <= n <= ffi.SCORE_MAX_N:
        raise ValueError(f"{what}: logits with {n} classes, must be in [1, TFIMM_SCORE_MAX_N = {ffi.SCORE_MAX_N}] "
                         f"(the row is held in LDS)")

    def upload():
        if isinstance(t, np.ndarray) or not t.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError("tfimm (MI355X engine) needs a ROCm GPU: no CPU execution path exists.")
            return (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t.contiguous()).to("cuda", non_blocking=True)
        return t.contiguous()
    return tuple(t.shape), upload


def _labels(y, batch, what):
    """``y`` -- a list, an integer numpy array, a torch int32 / int64 tensor on either side -- as (B,) int32.  Values are not
    looked at: int64 is saturated to [-2, 2^31 - 1] without a branch (below -1 and above every N stay what they were: out of
    range), so that host and device labels behave alike.  Returns a callable that does the device part."""
    import torch
    if isinstance(y, Tensor):
        y = y.torch()
    if isinstance(y, torch.Tensor):
        if y.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{what}: labels: expected int32 or int64, got {y.dtype}")
    else:
        y = np.asarray(y)
        if y.dtype.kind not in "iu":
            raise ValueError(f"{what}: labels: expected integers, got {y.dtype}")
    if y.ndim != 1:
        raise ValueError(f"{what}: labels: expected shape (B,), got {tuple(y.shape)}")
    if batch is not None and y.shape[0] != batch:
        raise ValueError(f"{what}: {y.shape[0]} labels for a batch of {batch}")
    top = 2 ** 31 - 1

    def upload():
        if isinstance(y, torch.Tensor):
            t = y if y.dtype == torch.int32 else y.clamp(-2, top).to(torch.int32)
        else:
            a = np.minimum(y.astype(np.uint64), top) if y.dtype.kind == "u" else np.clip(y.astype(np.int64), -2, top)
            t = torch.from_numpy(np.ascontiguousarray(a.astype(np.int32)))
        if not t.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError("tfimm (MI355X engine) needs a ROCm GPU: no CPU execution path exists.")
            t = t.to("cuda", non_blocking=True)
        return t.contiguous()
    return upload


def _launch(logits, labels, state=None, per_class=None, confusion=None) -> Scores:
    """tfimm_hip_score on the current stream, behind whatever produced ``logits`` there; no synchronisation"""
    import torch
    ffi = _consts()
    B, N = int(logits.shape[0]), int(logits.shape[1])
    dev = logits.device
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    rank = torch.empty(B, dtype=torch.int32, device=dev)
    pred = torch.empty(B, dtype=torch.int32, device=dev)
    prob = torch.empty(B, dtype=torch.float32, device=dev)
    if B:
        ptr = [None if t is None else t.data_ptr() for t in (state, per_class, confusion)]
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_score(logits.data_ptr(), N, B, N, labels.data_ptr(), loss.data_ptr(), rank.data_ptr(),
                                          pred.data_ptr(), prob.data_ptr(), ptr[0], ptr[1], ptr[2], st), "tfimm_hip_score")
    return Scores(Tensor(loss), Tensor(rank), Tensor(pred), Tensor(prob))


class MeterResult:
    """What a ``Meter`` has seen, on the host.  ``count`` rows were scored, ``ignored`` carried the label -1, ``invalid`` a
    label outside [0, nb_classes); ``loss`` is the mean cross-entropy (float64) over the scored rows but the ``loss_excluded``
    ones (NaN, inf or >= 1024); ``rank_hist[r]`` rows had the true class at rank ``r`` < 64, ``rank_hist[64]`` further down;
    ``per_class_support[c]`` / ``per_class_hits[c]``: rows of class ``c`` / those predicted right; ``confusion[label, pred]``.
    The last three are None when the meter did not keep them.  An empty meter gives NaN, it does not raise."""

    def __init__(self, count, ignored, invalid, loss, loss_excluded, rank_hist, per_class_support, per_class_hits, confusion):
        self.count, self.ignored, self.invalid = int(count), int(ignored), int(invalid)
        self.loss, self.loss_excluded = float(loss), int(loss_excluded)
        self.rank_hist = rank_hist
        self.per_class_support, self.per_class_hits, self.confusion = per_class_support, per_class_hits, confusion

    @classmethod
    def from_state(cls, words, per_class=None, confusion=None):
        """from the int64 words of tfimm_hip_score's state (include/tfimm_hip.h) and, optionally, the (2, N) per-class and
        (N, N) confusion counts: plain numpy, no device"""
        ffi = _consts()
        w = np.asarray(words)
        if w.shape != (ffi.SCORE_STATE_WORDS,) or w.dtype.kind not in "iu":
            raise ValueError(f"MeterResult.from_state: expected {ffi.SCORE_STATE_WORDS} integer words, got {w.dtype} {w.shape}")
        w = w.astype(np.int64)
        count, excluded = int(w[ffi.SCORE_SCORED]), int(w[ffi.SCORE_LOSS_EXCLUDED])
        summed = count - excluded
        # loss_q is a sum of rint(loss * 2^32): int -> float64 division, exact to 2^-53 relative
        loss = int(w[ffi.SCORE_LOSS_Q]) / 2.0 ** 32 / summed if summed > 0 else float("nan")
        hist = w[ffi.SCORE_RANK_HIST:ffi.SCORE_RANK_HIST + ffi.SCORE_RANK_BINS].copy()
        pc = None if per_class is None else np.asarray(per_class).astype(np.int64)
        if pc is not None and (pc.ndim != 2 or pc.shape[0] != 2):
            raise ValueError(f"MeterResult.from_state: per_class: expected shape (2, N), got {pc.shape}")
        cm = None if confusion is None else np.asarray(confusion).astype(np.int64)
        if cm is not None and (cm.ndim != 2 or cm.shape[0] != cm.shape[1]):
            raise ValueError(f"MeterResult.from_state: confusion: expected shape (N, N), got {cm.shape}")
        return cls(count, w[ffi.SCORE_IGNORED], w[ffi.SCORE_INVALID], loss, excluded, hist,
                   None if pc is None else pc[0].copy(), None if pc is None else pc[1].copy(), cm)

    def accuracy(self, k: int = 1) -> float:
        """the share of scored rows whose true class is among the ``k`` largest logits in ``tf.math.top_k``'s order (equal
        values by ascending class; ``tf.math.in_top_k`` would count every tie as a hit), 1 <= k <= 64"""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= len(self.rank_hist) - 1:
            raise ValueError(f"MeterResult.accuracy: k = {k!r}, must be an integer in [1, {len(self.rank_hist) - 1}]")
        return int(self.rank_hist[:k].sum()) / self.count if self.count else float("nan")

    @property
    def top1(self) -> float:
        return self.accuracy(1)

    def __repr__(self):
        return (f"MeterResult(count={self.count}, ignored={self.ignored}, invalid={self.invalid}, loss={self.loss:.6g}, "
                f"loss_excluded={self.loss_excluded}, top1={self.top1:.6g})")


class Meter:
    """``Meter(nb_classes, per_class=False, confusion=False)``: running accuracy@k for every k <= 64 and mean loss over the
    batches given to ``update`` (or to ``Model.evaluate(x, labels, meter)``), optionally per-class support / hits and the
    confusion matrix.  Everything is an integer in device memory, added to by the scoring launch itself; integer adds commute,
    so the state after a dataset is the same bits whatever the batch size or the order.  ``result()`` is the one copy to the
    host.  The buffers are allocated, zeroed, by the first ``update``; ``merge`` adds on the host."""

    def __init__(self, nb_classes: int, per_class: bool = False, confusion: bool = False):
        ffi = _consts()
        if isinstance(nb_classes, bool) or not isinstance(nb_classes, (int, np.integer)) or not 1 <= nb_classes <= ffi.SCORE_MAX_N:
            raise ValueError(f"Meter: nb_classes = {nb_classes!r}, must be an integer in [1, TFIMM_SCORE_MAX_N = {ffi.SCORE_MAX_N}]")
        if confusion and nb_classes > ffi.SCORE_MAX_CONFUSION_N:
            raise ValueError(f"Meter: a confusion matrix of {nb_classes} classes, more than TFIMM_SCORE_MAX_CONFUSION_N = "
                             f"{ffi.SCORE_MAX_CONFUSION_N} (64 MB)")
        self.nb_classes = int(nb_classes)
        self.per_class, self.confusion = bool(per_class), bool(confusion)
        self._buf = None            # one torch.int64 allocation: state words | per_class [2][N] | confusion [N][N] uint32
        self._merged = self._zeros()

    def _zeros(self) -> MeterState:
        n = self.nb_classes
        return MeterState(np.zeros(_consts().SCORE_STATE_WORDS, np.int64), np.zeros((2, n), np.int64) if self.per_class else None,
                          np.zeros((n, n), np.int64) if self.confusion else None)

    def _layout(self):
        """word offsets of the three parts in the one buffer, and its length"""
        n, words = self.nb_classes, _consts().SCORE_STATE_WORDS
        pc = words
        cm = pc + (2 * n if self.per_class else 0)
        return pc, cm, cm + ((n * n + 1) // 2 if self.confusion else 0)

    def _views(self):
        pc, cm, end = self._layout()
        return (self._buf[:pc], self._buf[pc:cm] if self.per_class else None,
                self._buf[cm:end] if self.confusion else None)

    def update(self, logits, labels) -> Scores:
        """Score a batch and add it: float32 ``logits`` (B, nb_classes) -- a ``Tensor`` or torch tensor on the GPU stays
        there, host arrays are uploaded -- and ``labels`` (B,), a list, an integer numpy array or a torch int32 / int64
        tensor on either side.  -1 marks a row that is not scored (the padding of a last batch); any other label outside
        [0, nb_classes) is counted in ``invalid``.  One launch on the current stream, no synchronisation."""
        return self._update(logits, labels, "Meter.update")

    def _update(self, logits, labels, what) -> Scores:
        import torch
        shape, up_logits = _logits(logits, self.nb_classes, what)
        up_labels = labels if callable(labels) else _labels(labels, shape[0], what)
        t, y = up_logits(), up_labels()
        if self._buf is None:
            self._buf = torch.zeros(self._layout()[2], dtype=torch.int64, device=t.device)
        return _launch(t, y, *self._views())

    def reset(self) -> None:
        """zero every counter"""
        if self._buf is not None:
            self._buf.zero_()
        self._merged = self._zeros()

    def state(self) -> MeterState:
        """the raw integers as numpy arrays (one device -> host copy): ``MeterState(words, per_class, confusion)``"""
        out = MeterState(*(None if a is None else a.copy() for a in self._merged))
        if self._buf is not None:
            host = self._buf.cpu().numpy()
            pc, cm, end = self._layout()
            n = self.nb_classes
            out.words[:] += host[:pc]
            if self.per_class:
                out.per_class[:] += host[pc:cm].reshape(2, n)
            if self.confusion:
                out.confusion[:] += host[cm:end].view(np.uint32)[:n * n].reshape(n, n)
        return out

    def merge(self, other) -> None:
        """add the counters of another ``Meter`` (or the arrays its ``state()`` gave: how the ranks of a data-parallel run
        combine) to this one's, on the host"""
        theirs = other.state() if isinstance(other, Meter) else MeterState(*other)
        mine = self._merged
        for name, a, b in zip(MeterState._fields, mine, theirs):
            if a is None:
                continue                       # this meter does not keep it
            if b is None:
                raise ValueError(f"Meter.merge: the other state has no {name}, this meter keeps it")
            b = np.asarray(b)
            if b.shape != a.shape or b.dtype.kind not in "iu":
                raise ValueError(f"Meter.merge: {name}: expected integers of shape {a.shape}, got {b.dtype} {b.shape}")
        for a, b in zip(mine, theirs):
            if a is not None:
                a += np.asarray(b).astype(np.int64)

    def result(self) -> MeterResult:
        return MeterResult.from_state(*self.state())


def score(logits, labels, meter: Meter = None) -> Scores:
    """``Scores(loss, rank, pred, prob)`` of float32 ``logits`` (B, N) against integer ``labels`` (B,): per sample the softmax
    cross-entropy (``tf.nn.sparse_softmax_cross_entropy_with_logits``), the number of classes ranked before the true one in
    ``tf.math.top_k``'s order, ``tf.argmax`` and the true class's softmax probability -- one launch (tfimm_hip_score) that
    reads every row once, on the current stream.  With ``meter`` the batch is also added to it (``Meter.update``)."""
    return _score(logits, labels, meter, "score")


def _score(logits, labels, meter, what) -> Scores:
    """``labels``: what ``score`` takes, or the callable ``_labels`` made of it (``Model.evaluate`` checks the labels before
    the forward pass runs)"""
    if meter is not None:
        return meter._update(logits, labels, what)
    shape, up_logits = _logits(logits, None, what)
    up_labels = labels if callable(labels) else _labels(labels, shape[0], what)
    return _launch(up_logits(), up_labels())

"""Base class of every tfimm model in this package.

Mirrors the parts of ``tf.keras.Model`` the reference's forward-path callers rely on
(SURVEY.md §8b): ``model(x, training=False, return_features=False)``,
``model.forward_features``, ``model.cfg``, ``model.name``, ``model.dummy_inputs``,
``model.feature_names``, ``model.weights`` -- but executes on MI355X through
libtfimm_hip.so.  Subclasses provide

  * ``weight_specs()``: ordered ``{tfimm weight name: WeightSpec}`` -- the variable
    inventory a Keras build would create, and
  * ``lower(b, H, W, features)``: trace the forward pass into a layer program.
"""
import os
from collections import OrderedDict, namedtuple
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from ..engine import precision
from ..engine.graph import Builder, Program
from ..utils import init as winit


@dataclass
class WeightSpec:
    shape: Tuple[int, ...]
    kind: str          # conv | dwconv | dense | bias | gamma | beta | mean | var | token | pos | table | scale
    init: str = ""     # keras-default initialiser override: "zeros" | "ones" | ""


#: what ``Model.top_k`` returns: three ``Tensor`` of shape (B, k) -- int32 class indices, float32 logits, float32 softmax
#: probabilities -- ordered by value descending, equal values by ascending class (``tf.math.top_k``)
TopK = namedtuple("TopK", ["indices", "values", "probs"])


class Tensor:
    """Result handle: device tensor with the ``.numpy()`` / ``.shape`` surface callers of the
    reference use on ``tf.Tensor`` results (tests/models/test_factory.py:47-49)."""

    def __init__(self, t):
        self._t = t

    @property
    def shape(self):
        return tuple(self._t.shape)

    @property
    def dtype(self):
        return self._t.dtype

    def torch(self):
        return self._t

    def numpy(self) -> np.ndarray:
        if not self._t.dtype.is_floating_point:
            return self._t.cpu().numpy()                     # class indices stay int32
        return self._t.float().cpu().numpy()

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a.astype(dtype) if dtype is not None else a

    def __repr__(self):
        return f"tfimm.Tensor(shape={self.shape}, dtype={self._t.dtype}, device={self._t.device})"


class DeferredInput:
    """uint8 pixels in [0, 255] plus the model's per-channel (mean, std): what
    ``create_preprocessing(name, defer=True)`` returns for uint8 images.  ``model(x)`` consumes it directly
    -- ``(v / 255 - mean) / std`` is evaluated by the kernel that converts the input to the engine's
    bf16 layout (tfimm_hip_preprocess_input), so no float image is ever materialised.  ``numpy()`` gives
    the float32 image the reference's preprocessing would have produced (models/factory.py:165-167).  With a ``resize``
    spec (``create_preprocessing(..., resize=True)``) the pixels may have any spatial size: resize, centre crop and
    normalisation run in one launch (tfimm_hip_preprocess_resize; with ``antialias=True`` tfimm_hip_preprocess_resize_aa) and
    ``numpy()`` is the same arithmetic on the CPU.  With ``boxes`` (``pre(frames, boxes=..., box_indices=...)``) ``data`` is a
    list of frames and every box ``(y0, x0, y1, x1)`` -- rows ``[y0, y1)``, columns ``[x0, x1)`` of frame ``box_indices[n]`` --
    is an image of its own: the batch is the boxes, each computed as the slice would be (tfimm_hip_preprocess_regions[_aa],
    DESIGN.md 3.22)."""

    def __init__(self, data, mean, std, resize=None, boxes=None, box_indices=None):
        self.data = data
        #: int32 (N, 4) corners and int32 (N,) frame indices of ``pre(frames, boxes=...)``, already checked against the
        #: frames (engine/ffi.py check_boxes); None for every other form
        self.boxes = boxes
        self.box_indices = box_indices
        self.mean = tuple(float(np.float32(v)) for v in mean)
        self.std = tuple(float(np.float32(v)) for v in std)
        #: ``create_preprocessing(..., resize=True)``: ``(interpolation, crop_pct, input_size)`` of the model config --
        #: the pixels may have any spatial size; they are resized to ``input_size / crop_pct``, centre-cropped
        #: (models/factory.py resize_geometry) and normalised in one launch (tfimm_hip_preprocess_resize)
        #: ``antialias=True`` appends ``True`` (tfimm_hip_preprocess_resize_aa); without it the spec has three entries
        self.resize = None if resize is None else (str(resize[0]), float(resize[1]), tuple(int(v) for v in resize[2]))
        if resize is not None and len(resize) > 3 and resize[3]:
            self.resize += (True,)

    @property
    def mixed(self) -> bool:
        """a list of images, each of a size of its own (``create_preprocessing(..., resize=True)`` on a list)"""
        return isinstance(self.data, (list, tuple)) and self.boxes is None

    @property
    def regions(self) -> bool:
        """boxes inside a list of frames (``pre(frames, boxes=...)``): the batch is the boxes"""
        return self.boxes is not None

    def slices(self) -> list:
        """the boxes as views into their frames, in box order: what the list form ``pre([...])`` would be handed"""
        return [self.data[int(f)][y0:y1, x0:x1] for (y0, x0, y1, x1), f in zip(self.boxes.tolist(), self.box_indices)]

    @property
    def shape(self):
        if self.regions:
            return (len(self.boxes), None, None, int(self.data[0].shape[2]))
        if self.mixed:
            return (len(self.data), None, None, int(self.data[0].shape[2]))
        return tuple(self.data.shape)

    def numpy(self) -> np.ndarray:
        """The float32 model input on the CPU.  With a resize spec this is the evaluation the device performs, operation
        for operation: the geometry of ``resize_geometry``, the tap tables of the library's host function
        (tfimm_hip_resize_taps), the sums of ``tf.image.resize(..., antialias=False)`` -- bicubic: vertical pass, then
        horizontal, each sum from 0.0 in tap order; bilinear: TensorFlow's compute_lerp -- then the three operations of
        the normalisation, all in float32.  Downscaling is not antialiased unless the spec says so: then the sums run
        over the span tables of tfimm_hip_resize_spans (``tf.image.resize(..., antialias=True)``), vertical pass first,
        each sum from 0.0 in tap order, for both methods.  A list of images: the stack of every image's own result; boxes:
        the stack of every slice's own result."""
        if self.regions:
            return np.stack([DeferredInput(im, self.mean, self.std, self.resize).numpy() for im in self.slices()])
        if self.mixed:
            return np.stack([DeferredInput(im, self.mean, self.std, self.resize).numpy() for im in self.data])
        d = self.data
        d = d.cpu().numpy() if hasattr(d, "cpu") else np.asarray(d)
        x = d.astype(np.float32)
        if self.resize is not None:
            x = x[None] if x.ndim == 3 else x
            x = _resize_crop_host(x, *self.resize)
            x = x[0] if d.ndim == 3 else x
        x = x / np.float32(255.0)
        return (x - np.asarray(self.mean, np.float32)) / np.asarray(self.std, np.float32)

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a.astype(dtype) if dtype is not None else a


def _resize_crop_host(x: np.ndarray, method: str, crop_pct: float, input_size, antialias: bool = False) -> np.ndarray:
    """(B, Hs, Ws, C) float32 -> the (B, H, W, C) crop window of the resized image, in plain numpy over the library's
    tap tables (a tap outside the image arrives as weight +0.0 at a clamped index: adding it is exact)."""
    from ..engine import ffi
    from .factory import resize_geometry
    H, W = input_size
    Hs, Ws = x.shape[1:3]
    Rh, Rw, top, left = resize_geometry((Hs, Ws), input_size, crop_pct)
    if antialias:
        # span tables: entries past a span's count weigh +0.0 (at an index clamped into the image), so every row and
        # column sums over the whole pitch
        (ys, _, wy), (xs, _, wx) = ffi.resize_spans(Hs, Rh, top, H, method), ffi.resize_spans(Ws, Rw, left, W, method)
        rows = np.zeros((x.shape[0], H, Ws, x.shape[3]), np.float32)
        for t in range(wy.shape[1]):
            rows = rows + wy[None, :, t, None, None] * x[:, np.minimum(ys + t, Hs - 1)]
        out = np.zeros((x.shape[0], H, W, x.shape[3]), np.float32)
        for t in range(wx.shape[1]):
            out = out + wx[None, None, :, t, None] * rows[:, :, np.minimum(xs + t, Ws - 1)]
        return out
    iy, wy = ffi.resize_taps(Hs, Rh, top, H, method)
    ix, wx = ffi.resize_taps(Ws, Rw, left, W, method)
    if method == "bicubic":
        rows = np.zeros((x.shape[0], H, Ws, x.shape[3]), np.float32)
        for t in range(4):
            rows = rows + wy[None, :, t, None, None] * x[:, iy[:, t]]
        out = np.zeros((x.shape[0], H, W, x.shape[3]), np.float32)
        for t in range(4):
            out = out + wx[None, None, :, t, None] * rows[:, :, ix[:, t]]
        return out
    xf, yf = wx[None, None, :, 1, None], wy[None, :, 1, None, None]
    r0, r1 = x[:, iy[:, 0]], x[:, iy[:, 1]]
    tl, tr, bl, br = r0[:, :, ix[:, 0]], r0[:, :, ix[:, 1]], r1[:, :, ix[:, 0]], r1[:, :, ix[:, 1]]
    upper = tl + (tr - tl) * xf
    lower = bl + (br - bl) * xf
    return upper + (lower - upper) * yf


class Model:
    cfg_class = None
    #: weights that exist in the reference as non-trainable build-time constants and are
    #: never loaded (e.g. swin attn_mask) -- accepted and ignored by ``set_weights``.
    keys_to_ignore_on_load = ()

    def __init__(self, cfg, name: Optional[str] = None, *, init: str = "keras", seed: int = 0):
        self.cfg = cfg
        self.name = name or cfg.name
        self._specs = self.weight_specs()
        self._weights: Dict[str, np.ndarray] = winit.initialize(self._specs, mode=init, seed=seed)
        self._programs: Dict[tuple, Program] = {}
        #: device copies of packed constants, shared by every program of this model (engine/graph.py Program.upload)
        self._const_cache: Dict[tuple, object] = {}
        self._plans: Dict[tuple, object] = {}
        #: hipGraph recordings of plans that have been used more than once: (plan key, input dtype) -> CapturedPlan
        self._captured: Dict[tuple, object] = {}
        self._plan_uses: Dict[tuple, int] = {}
        #: images per kernel launch sequence; larger batches are processed in chunks so
        #: producer->consumer activations stay inside the 256 MiB Infinity Cache.
        self.micro_batch: Optional[int] = None
        #: > 1: a batch runs as that many slices on parallel branches of one HIP graph (engine/graph.py CapturedBranches);
        #: pays for workloads whose launches leave compute units idle (ResNet-50 +6 %, Swin-B +12 % at batch 256), not for
        #: ViT-B.  TFIMM_BRANCHES sets the default.
        self.branches: int = int(os.environ.get("TFIMM_BRANCHES", "1") or "1")

    # -- to be provided by subclasses ------------------------------------------------------
    def weight_specs(self) -> "OrderedDict[str, WeightSpec]":
        raise NotImplementedError

    def lower(self, b: Builder, H: int, W: int, want_features: bool):
        """Build the program; must call ``b.p.mark_output`` for "logits" and "features"."""
        raise NotImplementedError

    @property
    def feature_names(self) -> List[str]:
        raise NotImplementedError

    # -- weights ----------------------------------------------------------------------------
    @property
    def weights(self) -> Dict[str, np.ndarray]:
        """``{name: fp32 array}`` keyed by the reference's variable names without the
        ``<model name>/`` prefix and ``:0`` suffix (models/factory.py:269-279)."""
        return self._weights

    def weight_names(self, with_prefix=False) -> List[str]:
        return [f"{self.name}/{k}:0" if with_prefix else k for k in self._specs]

    def set_weights(self, new: Dict[str, np.ndarray], strict: bool = True):
        """Replace weights by name.  ``strict`` (default): every variable of the model must be provided and no unknown
        name may appear (the build-time constants of ``keys_to_ignore_on_load`` excepted) -- a truncated or mismatched
        checkpoint fails loudly instead of leaving initialised values in place.  All names and shapes are validated
        before anything is committed, so a failed call leaves the model untouched."""
        staged: Dict[str, np.ndarray] = {}
        for k, v in new.items():
            if k.startswith(self.name + "/"):
                k = k[len(self.name) + 1:]
            if k.endswith(":0"):
                k = k[:-2]
            if k not in self._specs:
                if any(k.endswith(s) for s in self.keys_to_ignore_on_load):
                    continue
                if strict:
                    raise KeyError(f"{self.name}: unexpected weight '{k}'")
                continue
            v = np.asarray(v, dtype=np.float32)
            if tuple(v.shape) != tuple(self._specs[k].shape):
                raise ValueError(f"{self.name}: weight '{k}' has shape {v.shape}, expected {self._specs[k].shape}")
            staged[k] = v
        if strict:
            missing = [k for k in self._specs if k not in staged]
            if missing:
                raise KeyError(f"{self.name}: {len(missing)} weights missing from the provided set, e.g. {missing[:5]}")
        self._weights.update(staged)
        self._programs.clear()
        self._const_cache.clear()
        self._plans.clear()
        self._captured.clear()
        self._plan_uses.clear()

    def save_weights(self, path: str):
        np.savez(path, **self._weights)

    def load_weights(self, path: str):
        with np.load(path) as f:
            self.set_weights({k: f[k] for k in f.files})

    def count_params(self) -> int:
        return int(sum(int(np.prod(s.shape)) for s in self._specs.values()))

    # -- program cache -------------------------------------------------------------------------
    def program(self, H: Optional[int] = None, W: Optional[int] = None, want_features=False,
                top_k: Optional[int] = None) -> Program:
        """``top_k``: the program ends in one more op behind its logits (engine/graph.py Builder.topk) and has the outputs
        ``topk_values`` / ``topk_indices`` / ``topk_probs`` next to them -- a program of its own under a key of its own;
        without it keys and programs are what they were."""
        H = H or self.cfg.input_size[0]
        W = W or self.cfg.input_size[1]
        key = (H, W, bool(want_features), precision.get()) + self._topk_key(top_k)
        if key not in self._programs:
            if top_k:
                self._check_top_k(top_k)
            b = Builder(self._weights)
            b.p.const_cache = self._const_cache
            self.lower(b, H, W, want_features)
            if top_k:
                logits = b.p.outputs["logits"]
                # a tensor of several heads side by side (distilled DeiT: 2 x nb_classes columns): top-k per head
                b.topk(logits, top_k, heads=max(1, logits.C // self.cfg.nb_classes))
            self._programs[key] = b.finish()
        return self._programs[key]

    @staticmethod
    def _topk_key(top_k: Optional[int]) -> tuple:
        """the element ``top_k`` adds to the keys of programs, plans and recordings; nothing when it is not set"""
        return (("topk", int(top_k)),) if top_k else ()

    def _check_top_k(self, k) -> None:
        """``ValueError`` for what tfimm_hip_topk would refuse, before any device work"""
        from ..engine import ffi
        n = int(self.cfg.nb_classes)
        if n == 0:
            raise ValueError(f"{self.name}: top_k needs a classifier, this model has nb_classes == 0")
        if n > ffi.TOPK_MAX_N:
            raise ValueError(f"{self.name}: top_k holds a row of logits in LDS: nb_classes = {n} exceeds the limit "
                             f"TFIMM_TOPK_MAX_N = {ffi.TOPK_MAX_N}")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"{self.name}: top_k: k must be an integer, got {k!r}")
        if k < 1 or k > n or k > ffi.TOPK_MAX_K:
            raise ValueError(f"{self.name}: top_k: k = {k}, must be in [1, min(nb_classes = {n}, TFIMM_TOPK_MAX_K = "
                             f"{ffi.TOPK_MAX_K})]")

    # -- forward ---------------------------------------------------------------------------------
    @property
    def dummy_inputs(self) -> np.ndarray:
        return np.zeros((1, *self.cfg.input_size, self.cfg.in_channels), dtype=np.float32)

    def _to_device(self, x):
        import torch
        if isinstance(x, DeferredInput) and x.mixed:
            # a list of images of mixed sizes stays on the host: the plan packs it into its staging buffer per call
            imgs = [np.ascontiguousarray(im.cpu().numpy() if hasattr(im, "cpu") else im) for im in x.data]
            if x.resize is None or not imgs or len(x.mean) != self.cfg.in_channels or any(
                    im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != self.cfg.in_channels or im.size == 0 for im in imgs):
                raise ValueError(f"{self.name}: expected a non-empty list of uint8 images (Hs, Ws, {self.cfg.in_channels}) with "
                                 f"a resize spec, got shapes {[tuple(im.shape) for im in imgs]}")
            if not torch.cuda.is_available():
                raise RuntimeError("tfimm (MI355X engine) needs a ROCm GPU: no CPU execution path exists.")
            return imgs
        if isinstance(x, DeferredInput):
            # uint8 pixels + (mean, std): the normalisation runs inside the engine's input conversion
            u = x.data if isinstance(x.data, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x.data))
            if u.dim() != 4 or u.shape[-1] != self.cfg.in_channels or len(x.mean) != self.cfg.in_channels:
                raise ValueError(f"{self.name}: expected uint8 input (B, H, W, {self.cfg.in_channels}), got shape "
                                 f"{tuple(u.shape)} with {len(x.mean)} mean/std values")
            if not torch.cuda.is_available():
                raise RuntimeError("tfimm (MI355X engine) needs a ROCm GPU: no CPU execution path exists.")
            return u.to("cuda", non_blocking=True).contiguous()
        if isinstance(x, Tensor):
            x = x.torch()
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        if x.dim() != 4:
            raise ValueError(f"{self.name}: expected input (B, H, W, C), got shape {tuple(x.shape)}")
        if x.shape[-1] != self.cfg.in_channels:
            raise ValueError(f"{self.name}: expected {self.cfg.in_channels} input channels, got {x.shape[-1]}")
        if not torch.cuda.is_available():
            raise RuntimeError("tfimm (MI355X engine) needs a ROCm GPU: no CPU execution path exists.")
        return x.to("cuda", non_blocking=True).contiguous()

    def _run(self, x, want_features: bool, top_k: Optional[int] = None):
        import torch
        if isinstance(x, DeferredInput) and x.regions:
            return self._run_regions(x, want_features, top_k)
        xd = self._to_device(x)
        norm = (tuple(x.mean), tuple(x.std)) if isinstance(x, DeferredInput) else None
        if isinstance(xd, list):
            return self._run_mixed(xd, norm, x.resize, want_features, top_k)
        B, H, W, _ = xd.shape
        src = ()
        if norm is not None and x.resize is not None:
            # the program is the one of the MODEL's input size; the source size only selects the tap tables, so it joins the
            # plan / recording keys: a second source size makes a second recording instead of replaying the first one's tables
            method, crop_pct, (H, W) = x.resize[:3]
            # antialiased resampling is another input step over other tables: a plan and a recording of its own
            aa = len(x.resize) > 3
            norm = norm + ((method, crop_pct) + ((True,) if aa else ()),)
            src = (("src",) + tuple(xd.shape[1:3]) + (("antialias",) if aa else ()),)
        prog = self.program(H, W, want_features, top_k)
        src = src + self._topk_key(top_k)
        mb = self.micro_batch or B
        mb = min(mb, B)
        if self.branches > 1 and mb == B and B >= 2 * self.branches and prog.supports_branches():
            return self._run_branches(prog, xd, norm, want_features, (H, W), src)
        results: Dict[str, list] = {k: [] for k in prog.outputs}
        for start in range(0, B, mb):
            nb = min(mb, B - start)
            key = (H, W, bool(want_features), nb, precision.get()) + src
            plan = self._plans.get(key)
            if plan is None:
                plan = prog.make_plan(nb)
                self._plans[key] = plan
            chunk = xd[start:start + nb]
            # The first forward of a (shape, dtype) launches its ~100 kernels one ctypes call at a time; from the
            # second on the whole layer program is one hipGraphLaunch on a recording made then (TFIMM_NO_GRAPH=1
            # keeps launching eagerly).  The recording reads a private input buffer, refreshed by a device copy.
            gkey = key + (str(chunk.dtype), norm)
            cap = self._captured.get(gkey)
            if cap is None and self._plan_uses.get(gkey, 0) >= 1 and os.environ.get("TFIMM_NO_GRAPH", "0") != "1":
                cap = plan.capture(chunk.clone(), norm)
                self._captured[gkey] = cap
            self._plan_uses[gkey] = self._plan_uses.get(gkey, 0) + 1
            if cap is not None:
                cap.static_input.copy_(chunk)
                cap.replay()
            else:
                plan.run(chunk, norm=norm)
            for name, t in prog.outputs.items():
                # plans own their buffers and reuse them on the next call: hand out copies
                results[name].append(plan.tensor_view(t).clone())
        out = {}
        for name, parts in results.items():
            v = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
            t = prog.outputs[name]
            if t.H > 0:
                v = v.view(v.shape[0], t.H, t.W, t.C)
            elif t.rows == 1:
                v = v.view(v.shape[0], t.C)
            out[name] = v
        return out

    def _run_mixed(self, imgs, norm, resize, want_features: bool, top_k: Optional[int] = None):
        """A list of uint8 images, each of a size of its own.  The program is the one of the model's input
        size; the keys carry ``("src", "mixed")`` in place of a source size, so every mix of sizes meets the same plan and the
        same recording.  Per chunk: the plan builds records and tables on the host and uploads them with the packed pixels
        (``Plan.stage_mixed``), then the program is launched or replayed -- the recording reads the plan's buffers, whatever
        they hold.  Only a buffer that had to grow drops the recording.  ``branches`` is not used: a mixed batch runs on one
        branch (same bits, the engine's kernels never mix images)."""
        from ..engine.graph import MIXED
        return self._run_staged(len(imgs), lambda plan, lo, hi, norm: plan.stage_mixed(imgs[lo:hi], norm), MIXED, "mixed", norm,
                                resize, want_features, top_k)

    def _run_regions(self, x: "DeferredInput", want_features: bool, top_k: Optional[int] = None):
        """Boxes inside larger frames, ``pre(frames, boxes=...)``: ``_run_mixed`` with the boxes as the
        batch.  The keys carry ``("src", "regions")``, so every set of frames, frame sizes and boxes meets the same plan and
        the same recording per (model, N, precision); per chunk of boxes the plan uploads the frames the chunk names, once
        each, with records and tables (``Plan.stage_regions``).  Runs on one branch, as a mixed batch does."""
        import torch
        from ..engine.graph import REGIONS
        frames = [np.ascontiguousarray(f.cpu().numpy() if hasattr(f, "cpu") else f) for f in x.data]
        if x.resize is None or not frames or len(x.mean) != self.cfg.in_channels or any(
                f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != self.cfg.in_channels or f.size == 0 for f in frames):
            raise ValueError(f"{self.name}: expected uint8 frames (Hf, Wf, {self.cfg.in_channels}) with a resize spec, got "
                             f"shapes {[tuple(f.shape) for f in frames]}")
        if not torch.cuda.is_available():
            raise RuntimeError("tfimm (MI355X engine) needs a ROCm GPU: no CPU execution path exists.")
        boxes, idx = x.boxes, x.box_indices
        if len(x.resize) > 3 and (self.micro_batch or len(boxes)) < len(boxes):
            # several chunks: the antialias domain of EVERY box before the first chunk is staged or launched, by the box's own
            # number (a single chunk is refused by stage_regions itself, before it touches the plan)
            from ..engine import ffi
            from .factory import resize_geometry
            method, crop_pct, size = x.resize[:3]
            for n, (y0, x0, y1, x1) in enumerate(boxes.tolist()):
                Rh, Rw = resize_geometry((y1 - y0, x1 - x0), size, crop_pct)[:2]
                T = max(ffi.resize_span_taps(y1 - y0, Rh, method), ffi.resize_span_taps(x1 - x0, Rw, method))
                if T > ffi.RESIZE_AA_MAX_TAPS:
                    raise ValueError(f"{self.name}: antialiased {method} resize: box {n} ({y1 - y0} x {x1 - x0} -> {Rh} x {Rw}) "
                                     f"needs {T} taps per output pixel, more than TFIMM_RESIZE_AA_MAX_TAPS = "
                                     f"{ffi.RESIZE_AA_MAX_TAPS}: the box is too large for the device resize")
        return self._run_staged(len(boxes), lambda plan, lo, hi, norm: plan.stage_regions(frames, boxes[lo:hi], idx[lo:hi], norm),
                                REGIONS, "regions", (tuple(x.mean), tuple(x.std)), x.resize, want_features, top_k)

    def _run_staged(self, B, stage, marker, tag, norm, resize, want_features: bool, top_k: Optional[int] = None):
        """What ``_run_mixed`` and ``_run_regions`` share: a batch of ``B`` whose input step reads buffers the plan owns.
        ``stage(plan, lo, hi, norm)`` uploads members [lo, hi) and returns True when a buffer grew; ``marker`` is what
        ``Plan.run`` / ``Plan.capture`` take in place of an input tensor; ``tag`` names the form in the keys."""
        import torch
        method, crop_pct, (H, W) = resize[:3]
        aa = len(resize) > 3
        norm = norm + ((method, crop_pct) + ((True,) if aa else ()),)
        src = (("src", tag) + (("antialias",) if aa else ()),) + self._topk_key(top_k)
        prog = self.program(H, W, want_features, top_k)
        mb = min(self.micro_batch or B, B)
        results: Dict[str, list] = {k: [] for k in prog.outputs}
        for start in range(0, B, mb):
            nb = min(mb, B - start)
            key = (H, W, bool(want_features), nb, precision.get()) + src
            plan = self._plans.get(key)
            if plan is None:
                plan = self._plans[key] = prog.make_plan(nb)
            gkey = key + ("torch.uint8", norm)
            if stage(plan, start, start + nb, norm):
                self._captured.pop(gkey, None)        # a buffer grew: the recording points at the old one
            cap = self._captured.get(gkey)
            if cap is None and self._plan_uses.get(gkey, 0) >= 1 and os.environ.get("TFIMM_NO_GRAPH", "0") != "1":
                cap = self._captured[gkey] = plan.capture(marker, norm)
            self._plan_uses[gkey] = self._plan_uses.get(gkey, 0) + 1
            if cap is not None:
                cap.replay()
            else:
                plan.run(marker, norm=norm)
            for name, t in prog.outputs.items():
                results[name].append(plan.tensor_view(t).clone())
        out = {}
        for name, parts in results.items():
            v = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
            t = prog.outputs[name]
            if t.H > 0:
                v = v.view(v.shape[0], t.H, t.W, t.C)
            elif t.rows == 1:
                v = v.view(v.shape[0], t.C)
            out[name] = v
        return out

    def _run_branches(self, prog, xd, norm, want_features: bool, size, src=()):
        """The batch as ``self.branches`` slices on parallel branches of one HIP graph (engine/graph.py CapturedBranches):
        same kernels, same results, launches of different slices side by side."""
        import torch
        from ..engine.graph import CapturedBranches
        B, (H, W) = xd.shape[0], size
        key = (H, W, bool(want_features), B, precision.get(), "branches", self.branches) + src
        plans = self._plans.get(key)
        if plans is None:
            plans = prog.make_branches(B, self.branches)
            self._plans[key] = plans
        gkey = key + (str(xd.dtype), norm)
        cap = self._captured.get(gkey)
        if cap is None and self._plan_uses.get(gkey, 0) >= 1 and os.environ.get("TFIMM_NO_GRAPH", "0") != "1":
            cap = CapturedBranches(plans, xd.clone(), norm)
            self._captured[gkey] = cap
        self._plan_uses[gkey] = self._plan_uses.get(gkey, 0) + 1
        if cap is not None:
            cap.static_input.copy_(xd)
            cap.replay()
        else:
            lo = 0
            for p in plans:
                p.run(xd[lo:lo + p.batch], norm=norm)
                lo += p.batch
        out = {}
        for name, t in prog.outputs.items():
            v = torch.cat([p.tensor_view(t).clone() for p in plans], dim=0)
            if t.H > 0:
                v = v.view(v.shape[0], t.H, t.W, t.C)
            elif t.rows == 1:
                v = v.view(v.shape[0], t.C)
            out[name] = v
        return out

    def _finish(self, out: Dict[str, object], key: str, return_features: bool):
        y = self._shape_output(key, out[key])
        if not return_features:
            return Tensor(y)
        feats = OrderedDict()
        for name in self.feature_names:
            if name in out:
                feats[name] = Tensor(self._shape_output(name, out[name]))
            if name == key:
                break
        return Tensor(y), feats

    def _shape_output(self, name, v):
        return v

    def __call__(self, x, training: bool = False, return_features: bool = False):
        if training:
            raise NotImplementedError("This engine implements the inference forward path only (training=False).")
        out = self._run(x, return_features)
        return self._finish(out, "logits", return_features)

    def top_k(self, x, k: int = 5, training: bool = False) -> TopK:
        """Which classes, how sure: ``TopK(indices, values, probs)`` of ``model(x)`` -- each (B, k): int32 class indices,
        the float32 logits at them and their softmax probabilities over all classes -- by value descending, equal values by
        ascending class (``tf.nn.softmax`` + ``tf.math.top_k`` behind ``model(x)`` in a caller of the reference).  Takes
        everything ``__call__`` takes; the selection is the last launch of the same program (tfimm_hip_topk), from the
        second call on the last node of the same recording, so only ``3 * B * k`` numbers leave the device.  A model whose
        logits hold several heads (distilled DeiT: (B, 2, nb_classes)) answers per head: (B, 2, k)."""
        if training:
            raise NotImplementedError("This engine implements the inference forward path only (training=False).")
        self._check_top_k(k)
        out = self._run(x, False, top_k=int(k))
        return TopK(Tensor(out["topk_indices"]), Tensor(out["topk_values"]), Tensor(out["topk_probs"]))

    @staticmethod
    def _batch_of(x) -> int:
        """images in ``x``, whatever ``__call__`` takes: the members of a list, the BOXES of ``pre(frames, boxes=...)``"""
        if isinstance(x, DeferredInput):
            return int(x.shape[0])
        return len(x) if isinstance(x, (list, tuple)) else int(x.shape[0])

    def _check_evaluate(self, x, labels, meter):
        """``ValueError`` for what ``evaluate`` cannot score, before any device work; returns the checked labels as the
        callable that uploads them"""
        from ..engine import ffi
        n = int(self.cfg.nb_classes)
        if n == 0:
            raise ValueError(f"{self.name}: evaluate needs a classifier, this model has nb_classes == 0")
        if n > ffi.SCORE_MAX_N:
            raise ValueError(f"{self.name}: evaluate holds a row of logits in LDS: nb_classes = {n} exceeds the limit "
                             f"TFIMM_SCORE_MAX_N = {ffi.SCORE_MAX_N}")
        heads = self.program().outputs["logits"].C // n          # (lowering is host work)
        if heads != 1:
            raise ValueError(f"{self.name}: the logits hold {heads} heads per image; evaluate scores one (score a head's "
                             f"logits with tfimm.score)")
        if meter is not None and meter.nb_classes != n:
            raise ValueError(f"{self.name}: the meter counts {meter.nb_classes} classes, the model has nb_classes = {n}")
        from .meter import _labels
        batch = self._batch_of(x)
        return _labels(labels, int(batch), f"{self.name}: evaluate")

    def evaluate(self, x, labels, meter=None, training: bool = False):
        """How good on labelled data: ``tfimm.score(model(x), labels, meter)`` -- ``Scores(loss, rank, pred, prob)``, each
        (B,): the softmax cross-entropy, the rank of the true class among the logits, the predicted class and the true class's
        probability; with a ``tfimm.Meter`` the batch is added to its running accuracy@k and mean loss on the device.  Takes
        everything ``__call__`` takes.  The scoring launch (tfimm_hip_score) runs behind the model's program or recording on
        the same stream -- it is not part of them, labels being a second per-call input -- so the logits never leave the
        device and no program, plan or recording is added.  A label of -1 marks a padded row that is not scored."""
        if training:
            raise NotImplementedError("This engine implements the inference forward path only (training=False).")
        from .meter import _score
        labels = self._check_evaluate(x, labels, meter)
        return _score(self(x), labels, meter, f"{self.name}: evaluate")

    def _head_input(self, x, training: bool = False) -> Tensor:
        """What the classifier of ``model(x)`` reads, (B, D): ``forward_features(x)``, a feature map (B, H, W, D) averaged
        over H and W (tfimm_hip_mean_rows, as the model's own head does).  Takes everything ``__call__`` takes."""
        import ctypes as C
        import torch
        from ..engine import ffi
        f = self.forward_features(x, training=training).torch()
        if f.ndim == 2:
            return Tensor(f)
        if f.ndim != 4:
            raise ValueError(f"{self.name}: forward_features is {tuple(f.shape)}: several feature rows per image, no single "
                             f"classifier input")
        B, H, W, D = f.shape
        f = f.contiguous()
        pooled = torch.empty((B, D), dtype=f.dtype, device=f.device)
        if B:
            bf16 = f.dtype == torch.bfloat16
            mean = ffi.lib.tfimm_hip_mean_rows if bf16 else ffi.lib.tfimm_hip_ref_mean_rows
            ffi.check(mean(f.data_ptr(), pooled.data_ptr(), B, H * W, D, 0 if bf16 else 1,
                           C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tfimm_hip_mean_rows")
        return Tensor(pooled)

    def fit_head(self, x, labels, probe, training: bool = False):
        """One step of a ``tfimm.LinearProbe`` on this model's frozen features: ``probe.step(_head_input(x), labels)``.  Takes
        everything ``__call__`` takes; the model's weights, programs, plans and recordings are not touched
        (``probe.install(model)`` hands the fitted head over).  Returns ``StepResult(loss, pred)``, each (B,), without waiting
        for the device.  ``ValueError`` before any device work for a model whose logits hold several heads."""
        if training:
            raise NotImplementedError("This engine implements the inference forward path only (training=False).")
        from .meter import _labels
        n = int(self.cfg.nb_classes)
        if n > 0:
            heads = self.program().outputs["logits"].C // n          # (lowering is host work)
            if heads != 1:
                raise ValueError(f"{self.name}: the logits hold {heads} heads per image; fit_head fits one")
        batch = self._batch_of(x)
        labels = _labels(labels, int(batch), f"{self.name}: fit_head")
        return probe.step(self._head_input(x), labels)

    def distill_head(self, x, teacher, probe, valid=None, training: bool = False):
        """One step of a ``tfimm.EmbeddingProbe`` on this model's frozen features towards a teacher's embeddings:
        ``probe.step(_head_input(x), teacher, valid)``.  Takes everything ``__call__`` takes; ``teacher`` is (B, embed_dim),
        typically another model's output for the same images (``teacher_model(pre_t(img))``), and is checked against the
        batch of ``x`` before any device work.  The model's weights, programs, plans and recordings are not touched
        (``probe.install(embedding_model)`` hands the trained head over).  Returns ``DistillResult(loss, cosine)``, each (B,),
        without waiting for the device."""
        if training:
            raise NotImplementedError("This engine implements the inference forward path only (training=False).")
        targets = probe._targets(teacher, valid, int(self._batch_of(x)), f"{self.name}: distill_head")
        return probe.step(self._head_input(x), targets)

    def forward_features(self, x, training: bool = False, return_features: bool = False):
        if training:
            raise NotImplementedError("This engine implements the inference forward path only (training=False).")
        out = self._run(x, return_features)
        return self._finish(out, "features", return_features)

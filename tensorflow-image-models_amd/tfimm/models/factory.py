"""``create_model`` / ``create_preprocessing`` / ``transfer_weights``.

Same call signatures, keyword semantics and error behaviour as the reference's
tfimm/models/factory.py (create_model :18-125, create_preprocessing :128-171,
transfer_weights :174-250, _transform_first_conv :282-305); models are engine objects
(:class:`tfimm.models.model.Model`) instead of ``tf.keras.Model``.

Differences forced by the environment (documented in INTEGRATION.md):
  * ``model_path`` / the model cache hold ``.npz`` weight files written by
    ``model.save_weights`` (the reference stores Keras SavedModels).
  * ``pretrained=True`` with a ``[timm]`` / ``[pytorch]`` / ``[hf-pytorch]`` url needs
    network access + timm and raises ``NotImplementedError`` when the weights are not cached.
"""
import logging
import re
from copy import deepcopy
from typing import Callable, List, Optional

import numpy as np

from ..utils.cache import cached_model_path
from .registry import is_model, model_class, model_config


def create_model(
    model_name: str,
    pretrained: bool = False,
    model_path: str = "",
    *,
    in_channels: Optional[int] = None,
    nb_classes: Optional[int] = None,
    **kwargs,
):
    if not is_model(model_name):
        raise RuntimeError(f"Unknown model {model_name}.")
    cls = model_class(model_name)
    cfg = model_config(model_name)

    loaded_model = None
    if model_path or pretrained:
        path = model_path or cached_model_path(model_name)
        if not path:
            if cfg.url.startswith(("[timm]", "[pytorch]", "[hf-pytorch]")):
                raise NotImplementedError(
                    f"Pretrained weights for {model_name} ({cfg.url}) must be converted with timm/torch "
                    "and network access; neither is available. Put an .npz in the model cache instead.")
            raise NotImplementedError(
                "Model not found in cache. Download of weights only implemented for PyTorch models.")
        loaded_model = cls(deepcopy(cfg))
        loaded_model.load_weights(path)

    # config overrides: unknown keys are warned about and ignored (factory.py:92-103)
    cfg = deepcopy(cfg)
    for key, value in kwargs.items():
        if hasattr(cfg, key):
            setattr(cfg, key, value)
        else:
            logging.warning(f"Config for {model_name} does not have field `{key}`. Ignoring field.")
    if in_channels is not None:
        setattr(cfg, "in_channels", in_channels)
    if nb_classes is not None:
        setattr(cfg, "nb_classes", nb_classes)
    model_kwargs = {}
    if "name" in kwargs:
        model_kwargs["name"] = kwargs["name"]

    if loaded_model is not None and loaded_model.cfg == cfg:
        return loaded_model
    model = cls(cfg, **model_kwargs)
    if loaded_model is not None:
        transfer_weights(loaded_model, model)
    return model


def resize_geometry(src_hw, input_size, crop_pct: float):
    """``(Rh, Rw, top, left)``: the size a ``src_hw = (Hs, Ws)`` image is resized to and the corner of the
    ``input_size`` crop window inside it -- timm's evaluation transform, where ``crop_pct`` comes from.

    * square ``input_size`` (an int or ``(H, H)``): ``S = floor(H / crop_pct)``; the shorter source side becomes ``S``,
      the longer one ``int(S * long / short)`` (torchvision's ``Resize(int)``);
    * non-square ``(H, W)``: ``Rh = floor(H / crop_pct)``, ``Rw = floor(W / crop_pct)``, no aspect preservation;
    * centre crop: ``top = round((Rh - H) / 2)``, ``left = round((Rw - W) / 2)``, halves rounding to even."""
    import math
    if isinstance(input_size, (int, np.integer)):
        input_size = (int(input_size), int(input_size))
    H, W = int(input_size[0]), int(input_size[1])
    Hs, Ws = int(src_hw[0]), int(src_hw[1])
    if min(H, W, Hs, Ws) <= 0 or not 0.0 < crop_pct <= 1.0:
        raise ValueError(f"resize_geometry: bad arguments src={src_hw} input_size={input_size} crop_pct={crop_pct}")
    if H == W:
        S = int(math.floor(H / crop_pct))
        if Hs <= Ws:
            Rh, Rw = S, int(S * Ws / Hs)
        else:
            Rh, Rw = int(S * Hs / Ws), S
    else:
        Rh, Rw = int(math.floor(H / crop_pct)), int(math.floor(W / crop_pct))
    return Rh, Rw, int(round((Rh - H) / 2)), int(round((Rw - W) / 2))     # Python's round: half to even


def create_preprocessing(model_name: str, *, in_channels: Optional[int] = None,
                         dtype: Optional[str] = None, defer: bool = False, resize: bool = False,
                         antialias: bool = False, crop_pct: Optional[float] = None) -> Callable:
    """Function mapping [0, 255] images to model inputs: ``(img / 255 - mean) / std`` with
    mean/std tiled to ``in_channels`` (factory.py:153-169).  Works on numpy arrays and torch
    tensors, single images and batches; returns the input's array type.

    ``defer=True`` (not in the reference): a **uint8** image is not converted on the host but wrapped
    in a ``DeferredInput``; ``model(pre(img))`` then evaluates the same three float32 operations inside
    the kernel that converts the input to the engine's layout -- same bits as the host path, a quarter of
    the input bytes.  Anything that is not uint8 is preprocessed immediately as without the flag.

    ``resize=True`` (not in the reference; needs ``defer=True``): the uint8 image or batch may have ANY spatial size.  The
    ``DeferredInput`` then also carries the config's ``interpolation`` and ``crop_pct`` and the model's ``input_size``, and
    ``model(pre(img))`` resizes, centre-crops (``resize_geometry``) and normalises in one kernel launch
    (tfimm_hip_preprocess_resize).  Resampling is ``tf.image.resize(..., antialias=False)``: downscaling is NOT
    antialiased (TensorFlow's default; antialiasing is default off, see ``antialias`` below).  There is no host resize path: without
    ``defer``, or for input that is not uint8, ``ValueError`` is raised.  ``pre(img).numpy()`` evaluates the same
    arithmetic on the CPU, bit for bit what the device computes.  Every distinct source size makes a plan (with its
    activation buffers) and a recording of its own on the model, as every distinct float input size does: feed batches of
    few distinct sizes, device memory grows with their number.

    ``antialias=True`` (needs ``resize=True``): resampling is ``tf.image.resize(..., antialias=True)`` -- every output pixel
    sums a span of source pixels that grows with the scale, as PIL's resize does and as the pretrained weights were
    evaluated; without it a 480 x 640 frame going to 224 skips almost half of its source pixels.  One launch as before
    (tfimm_hip_preprocess_resize_aa), ``pre(img).numpy()`` again the same arithmetic bit for bit.  An axis
    may shrink to about 1/15 (bicubic) or 1/31 (bilinear) of its size; beyond that ``model(pre(img))`` raises
    ``ValueError`` (TFIMM_RESIZE_AA_MAX_TAPS).  Antialiased and plain input of the same source size use separate plans and
    recordings.

    A LIST (or tuple) of uint8 images ``(Hs_i, Ws_i, C)`` with ``resize=True``: every image may have a size of its own.  The
    ``DeferredInput`` holds the list (``shape`` is ``(B, None, None, C)``), ``numpy()`` is the stack of the per-image results,
    and ``model(pre(images))`` resizes the whole list in ONE launch whose arguments do not depend on the sizes
    (tfimm_hip_preprocess_resize_batch[_aa]): per model, batch size and precision there is one plan and one
    recording for every mix of sizes, so streaming a folder of photos does not grow device memory with the number of
    sizes.  Same arithmetic as for an array, image by image, bit for bit.  A list without ``resize=True``, an empty list, a
    member that is not uint8, not 3-D or of another channel count raises ``ValueError``.

    BOXES of frames, ``pre(frames, boxes=b, box_indices=i)`` with ``resize=True``: ``frames`` is one uint8 ``(Hf, Wf, C)`` frame,
    an ``(F, Hf, Wf, C)`` array or a list of frames of different sizes; ``boxes`` is an integer array-like ``(N, 4)`` of pixel
    corners ``(y0, x0, y1, x1)`` -- box ``n`` covers rows ``[y0, y1)`` and columns ``[x0, x1)`` of frame ``box_indices[n]``;
    ``box_indices`` ``(N,)`` may be in any order and repeat, and defaults to zeros for one frame.  The batch is the boxes
    (``shape`` is ``(N, None, None, C)``) and every box is an image of its own: ``model(pre(frames, boxes=b))`` computes, bit
    for bit, what ``model(pre([frames[i][y0:y1, x0:x1], ...]))`` computes -- taps beyond a box's edge clamp to the box -- but
    uploads every frame once, however many boxes lie in it, and slices nothing on the host (tfimm_hip_preprocess_regions[_aa],
    DESIGN.md 3.22); one plan and one recording per model, ``N`` and precision.  ``ValueError`` before anything is uploaded for
    boxes without ``resize=True``, float boxes (round them on purpose), ``N == 0``, a box that is empty or outside its frame,
    a frame index out of range, frames that are not uint8 or of another channel count.

    ``crop_pct`` (needs ``resize=True``; in (0, 1]): replaces the config's ``crop_pct`` in the resize spec of every form.  A
    detector's boxes usually want ``1.0``: the config's value (0.875 for most models) cuts their rim.  ``None`` keeps the
    config's value."""
    if not is_model(model_name):
        raise ValueError(f"Unknown model: {model_name}.")
    cfg = model_config(model_name)
    if resize and not defer:
        raise ValueError("create_preprocessing(resize=True) needs defer=True: the resize runs on the device, inside the "
                         "model's input conversion; there is no host resize path")
    if antialias and not resize:
        raise ValueError("create_preprocessing(antialias=True) needs resize=True: antialiasing is part of the device resize")
    if crop_pct is not None:
        if not resize:
            raise ValueError("create_preprocessing(crop_pct=...) needs resize=True: the crop is part of the device resize")
        if isinstance(crop_pct, bool) or not 0.0 < float(crop_pct) <= 1.0:
            raise ValueError(f"create_preprocessing: crop_pct = {crop_pct!r} must be in (0, 1]")
    if resize and cfg.interpolation not in ("bicubic", "bilinear"):
        raise ValueError(f"{model_name}: interpolation '{cfg.interpolation}' is not supported (bicubic, bilinear)")
    out_dtype = np.dtype(dtype or "float32")
    n = in_channels or cfg.in_channels

    def _adapt(v):
        v = np.asarray(v, dtype=np.float64)
        reps = n // v.shape[0] + 1
        return np.tile(v, reps)[:n]

    mean, std = _adapt(cfg.mean), _adapt(cfg.std)

    def _spec():
        """the resize spec of a DeferredInput: (interpolation, crop_pct, input_size[, True])"""
        pct = float(cfg.crop_pct if crop_pct is None else crop_pct)
        return (cfg.interpolation, pct, tuple(int(v) for v in cfg.input_size)) + ((True,) if antialias else ())

    def _regions(frames, boxes, box_indices):
        """boxes inside one frame, a stack of frames or a list of frames: one DeferredInput whose batch is the boxes"""
        from ..engine.ffi import check_boxes
        from .model import DeferredInput
        if not resize:
            raise ValueError("boxes need create_preprocessing(defer=True, resize=True): a box is cropped by the device resize")
        if isinstance(frames, (list, tuple)):
            frames = list(frames)
        elif len(getattr(frames, "shape", ())) == 3:
            frames = [frames]
        elif len(getattr(frames, "shape", ())) == 4:
            frames = [frames[i] for i in range(frames.shape[0])]
        else:
            raise ValueError(f"frames must be a uint8 (Hf, Wf, {n}) frame, an (F, Hf, Wf, {n}) array or a list of frames, got "
                             f"{getattr(frames, 'shape', type(frames).__name__)}")
        if len(frames) == 0:
            raise ValueError("create_preprocessing(resize=True): no frame")
        for i, f in enumerate(frames):
            if not str(getattr(f, "dtype", "")).endswith("uint8"):
                raise ValueError(f"create_preprocessing(resize=True) takes uint8 frames only, frame {i} is "
                                 f"{getattr(f, 'dtype', type(f).__name__)}: there is no host resize path")
            if len(f.shape) != 3 or int(f.shape[2]) != n or min(int(v) for v in f.shape) <= 0:
                raise ValueError(f"frame {i} has shape {tuple(f.shape)}, expected (Hf, Wf, {n})")
        boxes, box_indices = check_boxes([tuple(int(v) for v in f.shape[:2]) for f in frames], boxes, box_indices)
        return DeferredInput(frames, mean.astype(np.float32), std.astype(np.float32), resize=_spec(), boxes=boxes,
                             box_indices=box_indices)

    def _images(imgs):
        """a list / tuple of images, each of a size of its own: one DeferredInput over the list"""
        from .model import DeferredInput
        if not resize:
            raise ValueError("a list of images needs create_preprocessing(defer=True, resize=True): images of different "
                             "sizes only meet in the device resize; stack same-sized images into one array instead")
        if len(imgs) == 0:
            raise ValueError("create_preprocessing(resize=True): an empty list of images")
        for i, im in enumerate(imgs):
            if not str(getattr(im, "dtype", "")).endswith("uint8"):
                raise ValueError(f"create_preprocessing(resize=True) takes uint8 images only, image {i} of the list is "
                                 f"{getattr(im, 'dtype', type(im).__name__)}: there is no host resize path")
            if len(im.shape) != 3 or int(im.shape[2]) != n or min(int(v) for v in im.shape) <= 0:
                raise ValueError(f"image {i} of the list has shape {tuple(im.shape)}, expected (Hs, Ws, {n})")
        return DeferredInput(list(imgs), mean.astype(np.float32), std.astype(np.float32), resize=_spec())

    def _preprocess(img, boxes=None, box_indices=None):
        if boxes is not None:
            return _regions(img, boxes, box_indices)
        if box_indices is not None:
            raise ValueError("box_indices without boxes")
        if isinstance(img, (list, tuple)) and (len(img) == 0 or hasattr(img[0], "shape")):
            return _images(img)
        if defer and getattr(img, "dtype", None) is not None and str(img.dtype).endswith("uint8"):
            from .model import DeferredInput
            return DeferredInput(img, mean.astype(np.float32), std.astype(np.float32), resize=_spec() if resize else None)
        if resize:
            raise ValueError("create_preprocessing(resize=True) takes uint8 images only, got "
                             f"{getattr(img, 'dtype', type(img).__name__)}: there is no host resize path")
        try:
            import torch
            if isinstance(img, torch.Tensor):
                tdt = {"float16": torch.float16, "float32": torch.float32, "float64": torch.float64,
                       "bfloat16": torch.bfloat16}[str(dtype or "float32")]
                m = torch.as_tensor(mean, dtype=tdt, device=img.device)
                s = torch.as_tensor(std, dtype=tdt, device=img.device)
                return (img.to(tdt) / 255.0 - m) / s
        except ImportError:  # pragma: no cover
            pass
        x = np.asarray(img).astype(out_dtype) / out_dtype.type(255.0)
        return ((x - mean.astype(out_dtype)) / std.astype(out_dtype)).astype(out_dtype)

    return _preprocess


def _layer_name(w_name: str) -> str:
    """"remove/fc/kernel" -> "fc" (factory.py:253-266: drop auxiliary levels and the leaf)."""
    name = ("/" + w_name).replace("/remove/", "/")[1:]
    return name.rsplit("/", 1)[0] if "/" in name else name


def _transform_first_conv(weight: np.ndarray, in_channels: int) -> np.ndarray:
    """factory.py:282-305: sum over RGB for 1 channel, otherwise tile and rescale."""
    if weight.ndim != 4:
        return weight
    src = weight.shape[2]
    if in_channels == src:
        return weight
    if in_channels == 1:
        return weight.sum(axis=2, keepdims=True)
    reps = in_channels // src + 1
    w = np.tile(weight, (1, 1, reps, 1))[:, :, :in_channels, :]
    return w * np.float32(src / in_channels)


def transfer_weights(src_model, dst_model, weights_to_ignore: Optional[List[str]] = None):
    """Copy weights ``src_model`` -> ``dst_model`` (in place), adapting the first conv to
    ``dst.cfg.in_channels``, dropping the classifier when ``nb_classes`` differs, applying
    per-model transforms (e.g. pos-embed resize) and skipping ``weights_to_ignore`` patterns
    (factory.py:174-250)."""
    weights_to_ignore = list(weights_to_ignore or [])
    dst_first_conv = getattr(dst_model.cfg, "first_conv", None)
    if hasattr(src_model.cfg, "nb_classes") and hasattr(dst_model.cfg, "nb_classes"):
        keep_classifier = src_model.cfg.nb_classes == dst_model.cfg.nb_classes
    else:
        keep_classifier = True
    dst_classifier = getattr(dst_model.cfg, "classifier", [])
    if isinstance(dst_classifier, str):
        dst_classifier = [dst_classifier]
    transforms = getattr(src_model, "transform_weights", dict())
    weights_to_ignore += list(getattr(dst_model, "keys_to_ignore_on_load_missing", []))

    src = src_model.weights
    new = {}
    for w_name in dst_model.weights:
        layer = _layer_name(w_name)
        if any(re.search(pat, w_name) is not None for pat in weights_to_ignore):
            continue
        if layer in dst_classifier:
            if keep_classifier:
                new[w_name] = src[w_name]
        elif layer == dst_first_conv:
            new[w_name] = _transform_first_conv(src[w_name], dst_model.cfg.in_channels)
        elif w_name in transforms:
            new[w_name] = transforms[w_name](src_model, src[w_name], dst_model.cfg)
        else:
            new[w_name] = src[w_name]
    dst_model.set_weights(new, strict=False)

"""Time the mixed-size resize launches (tfimm_hip_preprocess_resize_batch[_aa]) against the uniform ones.

    python tools/time_resize_batch.py [--batch 256] [--out profiles/r10_resize_batch.txt]
HIP events around single launches, the median of 20 after 5 warm-ups, all in this one process and interleaved (uniform, mixed,
uniform, ...), into ResNet-50's zero-bordered four-channel input (229 x 230 x 4 bf16):
1. a UNIFORM batch, batch x 480 x 640 x 3 -> 224, both methods, plain and antialiased: the new launch against the existing
   uniform launch on the same pixels (the yardstick; bar: at most 1.25 x).  The antialiased launch is timed with the LDS size
   the plan picks (engine/graph.py Plan.stage_mixed: the batch's largest tile, doubling from 16 KiB) and with the full 64 KiB;
2. a MIXED batch of `batch` seeded sizes, heights 333 - 500 and widths 375 - 500, through one launch, against what a caller
   must do without it: `batch` uniform launches at B = 1, back to back;
3. the per-call host cost of that batch: building records and tables, and packing the pixels into the staging buffer."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tensorflow-image-models_amd"))

import tfimm  # noqa: E402,F401
from tfimm.engine import ffi  # noqa: E402
from tfimm.engine.graph import _grown  # noqa: E402
from tfimm.models.factory import resize_geometry  # noqa: E402

WARMUP, LAUNCHES = 5, 20
PAD = (3, 2, 3, 3)                      # the border of ResNet-50's fused stem: 224 x 224 -> 229 x 230
H = W = 224
MEAN, STD = (C.c_float * 3)(0.485, 0.456, 0.406), (C.c_float * 3)(0.229, 0.224, 0.225)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def interleaved(fns):
    """median ms of every callable: LAUNCHES rounds, each timing one call of each in turn, after WARMUP rounds"""
    for _ in range(WARMUP):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(LAUNCHES):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return [statistics.median(m) for m in ms]


def uniform_launch(x_ptr, B, src, out, method, aa):
    """the existing launch over B images of one size at x_ptr; returns (callable, keepalive)"""
    Hs, Ws = src
    geo = resize_geometry(src, (H, W), 0.875)
    if aa:
        ty, tx = ffi.resize_aa_tables(src, geo, (H, W), method)
        tabs = [torch.from_numpy(t).cuda() for t in ty + tx]
        d = ffi.ResizeAADesc()
        d.y_start, d.y_count, d.y_w, d.x_start, d.x_count, d.x_w = (t.data_ptr() for t in tabs)
        d.y_taps, d.x_taps = ty[2].shape[1], tx[2].shape[1]
        fn = ffi.lib.tfimm_hip_preprocess_resize_aa
    else:
        iy, wy = ffi.resize_taps(Hs, geo[0], geo[2], H, method)
        ix, wx = ffi.resize_taps(Ws, geo[1], geo[3], W, method)
        tabs = [torch.from_numpy(t).cuda() for t in (iy, wy, ix, wx)]
        d = ffi.ResizeDesc()
        d.y_idx, d.y_w, d.x_idx, d.x_w = (t.data_ptr() for t in tabs)
        d.taps = iy.shape[1]
        fn = ffi.lib.tfimm_hip_preprocess_resize
    d.in_, d.out = x_ptr, out
    d.mean_host, d.std_host = MEAN, STD
    d.B, d.Hs, d.Ws, d.c_in, d.H, d.W, d.c_out = B, Hs, Ws, 3, H, W, 4
    d.pad_t, d.pad_b, d.pad_l, d.pad_r = PAD
    return (lambda: ffi.check(fn(C.byref(d), stream()), fn.__name__)), (d, tabs)


def batch_launch(arena, sizes, out, method, aa, lds="plan"):
    """the new launch over the images packed in `arena`; returns (callable, keepalive, tables)"""
    t = ffi.resize_batch_tables(sizes, [resize_geometry(s, (H, W), 0.875) for s in sizes], (H, W), method, aa, c_in=3, pad=PAD)
    recs = torch.from_numpy(t["recs"].view(np.uint8)).cuda()
    w = torch.from_numpy(t["w"]).cuda()
    if aa:
        d = ffi.ResizeBatchAADesc()
        ta, tb = torch.from_numpy(t["start"]).cuda(), torch.from_numpy(t["count"]).cuda()
        d.start, d.count, d.w_floats = ta.data_ptr(), tb.data_ptr(), w.numel()
        d.taps_cap = min(_grown(t["max_taps"], 0, 16), ffi.RESIZE_AA_MAX_TAPS)
        d.lds_bytes = min(_grown(4 * t["lds_floats"], 0, 16 << 10), 64 << 10) if lds == "plan" else lds
        fn = ffi.lib.tfimm_hip_preprocess_resize_batch_aa
    else:
        d = ffi.ResizeBatchDesc()
        ta, tb = torch.from_numpy(t["idx"]).cuda(), None
        d.idx, d.taps = ta.data_ptr(), 4 if method == "bicubic" else 2
        fn = ffi.lib.tfimm_hip_preprocess_resize_batch
    d.in_, d.recs, d.out, d.w, d.in_bytes = arena.data_ptr(), recs.data_ptr(), out, w.data_ptr(), arena.numel()
    d.mean_host, d.std_host = MEAN, STD
    d.B, d.c_in, d.H, d.W, d.c_out = len(sizes), 3, H, W, 4
    d.pad_t, d.pad_b, d.pad_l, d.pad_r = PAD
    return (lambda: ffi.check(fn(C.byref(d), stream()), fn.__name__)), (d, recs, w, ta, tb), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    B = a.batch
    prop = torch.cuda.get_device_properties(0)
    lines = [f"device: {prop.name}, {prop.multi_processor_count} CUs, torch {torch.__version__}, HIP {torch.version.hip}",
             f"HIP events around single launches, median of {LAUNCHES} after {WARMUP} warm-ups, one process, interleaved",
             f"output {B} x 229 x 230 x 4 bf16 (224 x 224, crop_pct 0.875, ResNet-50's padded layout)"]
    out = torch.empty((B, H + PAD[0] + PAD[1], W + PAD[2] + PAD[3], 4), dtype=torch.bfloat16, device="cuda")
    rng = np.random.default_rng(0)
    # ---- 1. uniform batch
    src = (480, 640)
    x = torch.from_numpy(rng.integers(0, 256, (B, *src, 3), dtype=np.uint8)).cuda()
    lines.append(f"1. uniform batch {B} x {src[0]} x {src[1]} x 3: existing launch | mixed-size launch | ratio (bar 1.25)")
    for method in ("bicubic", "bilinear"):
        for aa in (False, True):
            uni, k0 = uniform_launch(x.data_ptr(), B, src, out.data_ptr(), method, aa)
            new, k1, t = batch_launch(x.view(-1), [src] * B, out.data_ptr(), method, aa)
            fns, extra = [uni, new], ""
            if aa:
                full, k2, _ = batch_launch(x.view(-1), [src] * B, out.data_ptr(), method, aa, lds=64 << 10)
                fns.append(full)
            ms = interleaved(fns)
            if aa:
                extra = f" (LDS {k1[0].lds_bytes} B; with 64 KiB: {ms[2] * 1e3:.1f} us, {ms[2] / ms[0]:.2f} x)"
            lines.append(f"   {method:8s} antialias={aa!s:5s}: {ms[0] * 1e3:8.1f} us | {ms[1] * 1e3:8.1f} us | {ms[1] / ms[0]:.2f} x"
                         f" {'ok' if ms[1] <= 1.25 * ms[0] else 'MISSES THE BAR'}{extra}")
    del x
    # ---- 2. mixed batch
    sizes = [(int(h), int(w)) for h, w in zip(rng.integers(333, 501, B), rng.integers(375, 501, B))]
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    arena = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).cuda()
    offs = np.cumsum([0] + [im.size for im in images])
    lines.append(f"2. mixed batch, {B} seeded sizes {min(s[0] for s in sizes)}-{max(s[0] for s in sizes)} x "
                 f"{min(s[1] for s in sizes)}-{max(s[1] for s in sizes)}, {len(set(sizes))} distinct, {arena.numel() / 2**20:.1f} MiB: "
                 f"{B} uniform launches at B = 1 | one mixed-size launch | ratio")
    step = out[0].numel() * 2
    for method in ("bicubic", "bilinear"):
        for aa in (False, True):
            singles = [uniform_launch(arena.data_ptr() + int(offs[i]), 1, sizes[i], out.data_ptr() + i * step, method, aa) for i in range(B)]

            def each(singles=singles):
                for fn, _ in singles:
                    fn()
            new, k1, t = batch_launch(arena, sizes, out.data_ptr(), method, aa)
            ms = interleaved([each, new])
            lines.append(f"   {method:8s} antialias={aa!s:5s}: {ms[0] * 1e3:8.1f} us | {ms[1] * 1e3:8.1f} us | {ms[0] / ms[1]:.1f} x faster")
    # ---- 3. host cost per call
    stage = torch.empty(arena.numel(), dtype=torch.uint8, pin_memory=True).numpy()
    lines.append("3. host cost per call of that batch (wall time, median of 20): records and tables | packing the pixels")
    for method in ("bicubic", "bilinear"):
        for aa in (False, True):
            tb, tp = [], []
            for _ in range(LAUNCHES):
                t0 = time.perf_counter()
                ffi.resize_batch_tables(sizes, [resize_geometry(s, (H, W), 0.875) for s in sizes], (H, W), method, aa, c_in=3, pad=PAD)
                t1 = time.perf_counter()
                pos = 0
                for im in images:
                    stage[pos:pos + im.size] = im.reshape(-1)
                    pos += im.size
                t2 = time.perf_counter()
                tb.append(t1 - t0)
                tp.append(t2 - t1)
            lines.append(f"   {method:8s} antialias={aa!s:5s}: {statistics.median(tb) * 1e3:7.2f} ms | {statistics.median(tp) * 1e3:7.2f} ms")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

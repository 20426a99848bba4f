"""What boxes of a frame cost against slices packed on the host, in ONE process:

    python tools/regions_probe.py [--rounds R] [--out FILE]

resnet50 and EmbeddingModel(resnet50, 512); N = 64 seeded boxes, sides 64 to 400 and overlapping, from one 1080 x 1920 frame;
plain and antialiased.
(a) ``model(pre(frame, boxes=b))`` against ``model(pre([slices]))``: the calls alternate, each timed with a host clock around a
    synchronised call, so slicing, staging and upload are inside; every shape is warmed up first (plan, recording, capacities).
(b) the bytes each path stages and uploads, computed from the shapes.
(c) the input-step kernels alone, tfimm_hip_preprocess_regions[_aa] against tfimm_hip_preprocess_resize_batch[_aa] on the same
    boxes: a captured graph of LAUNCHES launches per arm, replayed alternately, HIP events around each replay.
Not a bench.py line."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tensorflow-image-models_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tfimm  # noqa: E402
from tfimm.engine import ffi  # noqa: E402
from tfimm.models.factory import resize_geometry  # noqa: E402
from tfimm.utils.init import synthetic_weights  # noqa: E402

FRAME_HW = (1080, 1920)
N_BOXES = 64
SIDES = (64, 400)
LAUNCHES = 20          # launches per recorded graph of part (c)
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def seeded_input():
    rng = np.random.default_rng(2021)
    frame = rng.integers(0, 256, (*FRAME_HW, 3), dtype=np.uint8)
    h, w = rng.integers(SIDES[0], SIDES[1] + 1, N_BOXES), rng.integers(SIDES[0], SIDES[1] + 1, N_BOXES)
    y0, x0 = rng.integers(0, FRAME_HW[0] - h + 1), rng.integers(0, FRAME_HW[1] - w + 1)
    return frame, np.stack([y0, x0, y0 + h, x0 + w], axis=1).astype(np.int64)


def timed_replay(graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)          # ms


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def call_level(label, model, frame, boxes, aa, rounds):
    pre = tfimm.create_preprocessing("resnet50", defer=True, resize=True, antialias=aa)

    def slices():
        return [frame[y0:y1, x0:x1] for y0, x0, y1, x1 in boxes.tolist()]

    arms = {"pre(frame, boxes=b)": lambda: model(pre(frame, boxes=boxes)),
            "pre([slices])": lambda: model(pre(slices()))}
    outs = {}
    for _ in range(4):                                     # plan, recording, capacities: every shape has settled
        for name, fn in arms.items():
            outs[name] = wall(fn)[1].numpy()
    assert np.array_equal(outs["pre(frame, boxes=b)"], outs["pre([slices])"]), "the two paths disagree"
    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            times[name].append(wall(fn)[0])
    say(f"(a) {label}, {'antialiased' if aa else 'plain'}: {rounds} calls per arm, alternating, host clock around a synchronised call")
    med = {}
    for name, t in times.items():
        med[name] = float(np.median(t))
        say(f"    model({name:20s}) {med[name]:8.3f} ms/call (min {min(t):.3f}, max {max(t):.3f})")
    d = med["pre([slices])"] - med["pre(frame, boxes=b)"]
    say(f"    slices - boxes: {d:+.3f} ms per call ({d / med['pre([slices])'] * 100:+.1f} % of the list path)")


def bytes_level(frame, boxes):
    packed = int(sum((y1 - y0) * (x1 - x0) * 3 for y0, x0, y1, x1 in boxes.tolist()))
    say(f"(b) staged and uploaded per call, {N_BOXES} boxes of one {FRAME_HW[0]} x {FRAME_HW[1]} frame:")
    say(f"    pre(frame, boxes=b): {frame.size:10d} bytes of pixels (the frame once) + {N_BOXES * C.sizeof(ffi.ResizeRegionRec)} bytes of records")
    say(f"    pre([slices])      : {packed:10d} bytes of pixels (every slice)    + {N_BOXES * C.sizeof(ffi.ResizeBatchRec)} bytes of records")
    say(f"    ratio slices / frame: {packed / frame.size:.2f}; the tables are the same bytes on both paths")


def kernel_level(frame, boxes, method, aa, rounds):
    """the two launches on the same boxes into a (N, 224, 224, 4) bf16 tensor"""
    H = W = 224
    hw = [(int(b[2] - b[0]), int(b[3] - b[1])) for b in boxes]
    geos = [resize_geometry(s, (H, W), 0.875) for s in hw]
    mean, std = (C.c_float * 3)(0.485, 0.456, 0.406), (C.c_float * 3)(0.229, 0.224, 0.225)
    tabs = {"regions": ffi.resize_region_tables([FRAME_HW], boxes, np.zeros(N_BOXES, np.int32), geos, (H, W), method, aa),
            "batch": ffi.resize_batch_tables(hw, geos, (H, W), method, aa)}
    pixels = {"regions": frame.reshape(-1),
              "batch": np.concatenate([frame[y0:y1, x0:x1].reshape(-1) for y0, x0, y1, x1 in boxes.tolist()])}
    arms = {}
    for arm, t in tabs.items():
        dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda") for k, v in t.items() if isinstance(v, np.ndarray) and k != "recs"}
        dev["recs"] = torch.from_numpy(t["recs"].view(np.uint8)).to("cuda")
        dev["in"] = torch.from_numpy(pixels[arm]).to("cuda")
        out = torch.zeros((N_BOXES, H, W, 4), dtype=torch.bfloat16, device="cuda")
        if arm == "regions":
            d = ffi.ResizeRegionAADesc() if aa else ffi.ResizeRegionDesc()
        else:
            d = ffi.ResizeBatchAADesc() if aa else ffi.ResizeBatchDesc()
        d.in_, d.recs, d.out, d.w, d.in_bytes = dev["in"].data_ptr(), dev["recs"].data_ptr(), out.data_ptr(), dev["w"].data_ptr(), pixels[arm].size
        d.mean_host, d.std_host = mean, std
        d.B, d.c_in, d.H, d.W, d.c_out = N_BOXES, 3, H, W, 4
        if aa:
            d.start, d.count, d.w_floats = dev["start"].data_ptr(), dev["count"].data_ptr(), t["w"].size
            d.taps_cap, d.lds_bytes = ffi.RESIZE_AA_MAX_TAPS, 0
        else:
            d.idx, d.taps = dev["idx"].data_ptr(), 4 if method == "bicubic" else 2
        fn = getattr(ffi.lib, ("tfimm_hip_preprocess_regions" if arm == "regions" else "tfimm_hip_preprocess_resize_batch")
                     + ("_aa" if aa else ""))

        def launch(fn=fn, d=d):
            ffi.check(fn(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "input step")
        launch()                      # function attributes are set outside the recording
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            for _ in range(LAUNCHES):
                launch()
        graph.replay()
        torch.cuda.synchronize()
        arms[arm] = dict(graph=graph, out=out, times=[], keep=(dev, d, mean, std))
    assert torch.equal(arms["regions"]["out"], arms["batch"]["out"]), "the two launches disagree"
    for _ in range(3):
        for a in arms.values():
            timed_replay(a["graph"])
    for _ in range(rounds):
        for a in arms.values():
            a["times"].append(timed_replay(a["graph"]) / LAUNCHES * 1e3)
    say(f"(c) input step alone, {method} {'antialiased' if aa else 'plain'}, {N_BOXES} boxes -> {H} x {W}: graphs of {LAUNCHES} launches, "
        f"{rounds} replays per arm, alternating")
    med = {}
    for arm, a in arms.items():
        med[arm] = float(np.median(a["times"]))
        say(f"    {arm:8s} {med[arm]:9.2f} us/launch (min {min(a['times']):.2f}, max {max(a['times']):.2f}); {pixels[arm].size} source bytes")
    say(f"    regions / batch: {med['regions'] / med['batch']:.3f}")


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 30
    if not torch.cuda.is_available():
        sys.exit("regions_probe needs a GPU: nothing here can be measured without one")
    say(f"device: {torch.cuda.get_device_name(0)}")
    frame, boxes = seeded_input()
    say(f"{N_BOXES} boxes, sides {SIDES[0]}..{SIDES[1]}, of one {FRAME_HW[0]} x {FRAME_HW[1]} x 3 uint8 frame (seed 2021)")
    bytes_level(frame, boxes)
    for aa in (False, True):
        kernel_level(frame, boxes, "bicubic", aa, rounds)
    resnet = tfimm.create_model("resnet50")
    resnet.set_weights(synthetic_weights(resnet, 2021))
    emb = tfimm.EmbeddingModel(tfimm.create_model("resnet50"), 512)
    emb.set_weights(synthetic_weights(emb, 2021))
    for label, model in (("resnet50", resnet), ("EmbeddingModel(resnet50, 512)", emb)):
        for aa in (False, True):
            call_level(label, model, frame, boxes, aa, rounds)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

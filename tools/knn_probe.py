"""What the kNN end costs, in ONE process:

    python tools/knn_probe.py [--rounds R] [--out FILE]

(1) tfimm_hip_knn_vote alone on matches that are already there, at (B, k, top) = (256, 20, 5) and (4096, 64, 5), weighted
sum at temperature 0.07 over a gallery of 1 000 000 labels in 1000 classes: a captured graph of LAUNCHES launches against a
captured graph of LAUNCHES runs of the torch baseline -- label gather, ``exp``, ``scatter_add`` into a dense (B, classes)
matrix, ``topk`` (probe only, never on the product path) --, the two replayed alternately (R rounds after a warm-up, HIP events
around each replay); microseconds per launch against the bytes the kernel must move once (indices, scores, one label per
candidate, the four outputs) at 8 TB/s.
(2) ``Gallery.classify`` end to end (the two launches of the search + the vote) with k = 20 at (B, N, E) = (32, 1 000 000, 512)
and (256, 100 000, 512), against ``(q.bfloat16() @ g.T).float().topk(k)`` + the baseline of (1); the search alone is timed as
a third arm, so that the vote's share shows.
Shader clock and socket power over the timed regions come from tools/telemetry.py.  Not a bench.py line."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tensorflow-image-models_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tfimm  # noqa: E402
from tfimm.engine import ffi  # noqa: E402

VOTE_SHAPES = [(256, 20, 5), (4096, 64, 5)]
CLASSIFY_SHAPES = [(32, 1_000_000, 512), (256, 100_000, 512)]
K, TOP, CLASSES, TEMPERATURE = 20, 5, 1000, 0.07
N_LABELS = 1_000_000
LAUNCHES = 20          # runs per recorded graph
HBM_BYTES_PER_S = 8e12
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)
    if "--out" in sys.argv:                # rewritten as it grows: a run cut short leaves what it measured
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(LINES) + "\n")


def timed_replay(graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)          # ms


def telemetry():
    try:
        from telemetry import Telemetry
        t = Telemetry(device_index=0)
        t.__enter__()
        return t
    except Exception as e:  # noqa: BLE001  (telemetry is optional: a box without a source still measures)
        say(f"telemetry unavailable: {e}")
        return None


def telemetry_line(t):
    if t is None:
        return
    t.__exit__(None, None, None)
    s = t.summary()
    say("  telemetry: " + ", ".join(f"{k} {s.get(k)}" for k in ("sclk_mhz_mean", "sclk_mhz_min", "power_w_mean", "power_w_max",
                                                               "power_cap_w", "source")))


def record(fn):
    fn()                              # workspaces and torch's own set-up stay outside the recording
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for _ in range(LAUNCHES):
            fn()
    return graph


def race(arms, rounds):
    """``arms``: name -> function; each recorded, replayed alternately; returns name -> (median, min, max) in us per run"""
    graphs = {name: record(fn) for name, fn in arms.items()}
    for _ in range(3):
        for g in graphs.values():
            timed_replay(g)
    times = {name: [] for name in arms}
    t = telemetry()
    for _ in range(rounds):
        for name, g in graphs.items():
            times[name].append(timed_replay(g) / LAUNCHES * 1e3)
    return {name: (float(np.median(v)), min(v), max(v)) for name, v in times.items()}, t


def torch_vote(indices, scores, labels, inv_t):
    """the baseline behind the matches: what a caller of torch would write"""
    lab = labels[indices.long()].long()
    w = torch.exp((scores - scores[:, :1]) * inv_t)
    votes = torch.zeros(indices.shape[0], CLASSES, dtype=torch.float32, device=indices.device).scatter_add_(1, lab, w)
    return votes.topk(TOP)


def vote_level(shape, rounds):
    B, k, top = shape
    gen = torch.Generator().manual_seed(2021)
    labels = torch.randint(0, CLASSES, (N_LABELS,), generator=gen, dtype=torch.int32).to("cuda")
    indices = torch.randint(0, N_LABELS, (B, k), generator=gen, dtype=torch.int32).to("cuda")
    scores = torch.rand(B, k, generator=gen).sort(1, descending=True).values.to("cuda")
    inv_t = float(np.float32(1.0) / np.float32(TEMPERATURE))
    outs = [torch.empty((B, top), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.int32)]
    total = torch.empty(B, dtype=torch.float32, device="cuda")
    base = {}

    def vote():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_knn_vote(indices.data_ptr(), scores.data_ptr(), k, B, k, labels.data_ptr(), N_LABELS, None, inv_t,
                                             ffi.KNN_SUM, top, *(t.data_ptr() for t in outs), total.data_ptr(), st), "tfimm_hip_knn_vote")

    def baseline():
        base["out"] = torch_vote(indices, scores, labels, inv_t)

    res, t = race({"tfimm_hip_knn_vote": vote, "torch gather + scatter_add + topk": baseline}, rounds)
    torch.cuda.synchronize()
    agree = float((outs[0][:, 0].long() == base["out"].indices[:, 0]).float().mean())
    moved = B * k * 12 + B * (3 * top + 1) * 4
    floor = moved / HBM_BYTES_PER_S * 1e6
    say(f"vote B={B} k={k} top={top}: {moved} bytes to move once, {floor:.3f} us at 8 TB/s; first class equal to the baseline's "
        f"in {agree * 100:.2f} % of the rows")
    for name, (us, lo, hi) in res.items():
        say(f"  {name:36s} {us:9.2f} us/launch (min {lo:.2f}, max {hi:.2f}); {us / floor:9.1f} x floor")
    say(f"  vote / baseline: {res['tfimm_hip_knn_vote'][0] / res['torch gather + scatter_add + topk'][0]:.3f}")
    telemetry_line(t)


def classify_level(shape, rounds):
    B, N, E = shape
    gen = torch.Generator().manual_seed(2021)
    gallery = tfimm.Gallery(E, capacity=N)
    for lo in range(0, N, 100_000):                                      # filled in slices: no float32 copy of the whole gallery
        n = min(100_000, N - lo)
        gallery.add(torch.randn(n, E, generator=gen).to("cuda"),
                    torch.randint(0, CLASSES, (n,), generator=gen, dtype=torch.int32).to("cuda"))
    q = torch.randn(B, E, generator=gen).to("cuda")
    g, labels = gallery._buf[:N], gallery._lab[:N]
    inv_t = float(np.float32(1.0) / np.float32(TEMPERATURE))
    out = {}

    def classify():
        out["votes"] = gallery.classify(q, K, TEMPERATURE, TOP)

    def search():
        out["matches"] = gallery.search(q, K)

    def baseline():
        s, i = (q.bfloat16() @ g.T).float().topk(K)
        out["base"] = torch_vote(i, s, labels, inv_t)

    res, t = race({"Gallery.classify": classify, "Gallery.search alone": search,
                   "torch matmul + topk + gather + scatter_add": baseline}, rounds)
    torch.cuda.synchronize()
    agree = float((out["votes"].classes.torch()[:, 0].long() == out["base"].indices[:, 0]).float().mean())
    floor = N * E * 2 / HBM_BYTES_PER_S * 1e6
    say(f"classify B={B} N={N} E={E} k={K} top={TOP}: one-read floor of the gallery {floor:.1f} us; first class equal to the "
        f"baseline's in {agree * 100:.2f} % of the rows (the baseline rounds its scores to bf16)")
    for name, (us, lo, hi) in res.items():
        say(f"  {name:44s} {us:10.1f} us/call (min {lo:.1f}, max {hi:.1f}); {us / floor:7.1f} x floor")
    say(f"  vote's share of classify: {res['Gallery.classify'][0] - res['Gallery.search alone'][0]:+.1f} us; classify / baseline: "
        f"{res['Gallery.classify'][0] / res['torch matmul + topk + gather + scatter_add'][0]:.2f}")
    telemetry_line(t)
    del gallery, g, labels, out
    torch.cuda.empty_cache()


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 30
    if not torch.cuda.is_available():
        sys.exit("knn_probe needs a GPU: nothing here can be measured without one")
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"graphs of {LAUNCHES} runs, the arms replayed alternately, {rounds} rounds after 3 warm-up rounds; {CLASSES} classes, "
        f"temperature {TEMPERATURE}")
    for shape in VOTE_SHAPES:
        vote_level(shape, rounds)
    for shape in CLASSIFY_SHAPES:
        classify_level(shape, rounds)


if __name__ == "__main__":
    main()

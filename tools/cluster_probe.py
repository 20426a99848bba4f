"""What the cluster end costs, in ONE process:

    python tools/cluster_probe.py [--rounds R] [--out FILE]

(1) tfimm_hip_cluster_assign at (N, C, E) = (1 000 000, 1024, 512) and (100 000, 256, 128) against the larger of its byte floor
(2 N E + 2 C E + 8 N bytes once, at 8 TB/s) and its flop floor (2 N C E at 2.5 PFLOP/s), and against ``torch``'s bf16 ``matmul``
+ ``max`` over the (N, C) matrix it materialises (probe only, never on the product path).
(2) tfimm_hip_segment_mean at (M, E) = (1 000 000, 512), C = 1024, once with balanced segments and once with one segment
holding half the rows, against its byte floor (2 M E + 4 M read once, 4 C E written) and against ``torch``'s ``index_add_`` into
float32 + the division.  The CSR form is built before the clock starts on both sides.
(3) one k-means iteration end to end -- assign, the CSR form (``torch`` sort + searchsorted), the means, the normalisation,
bf16, empty clusters kept -- at both shapes of (1), against the same loop in ``torch``.
Every arm is a captured graph of LAUNCHES runs; the arms are replayed alternately (R rounds after a warm-up, HIP events around
each replay) and the median of the rounds is reported.  Shader clock and socket power over the timed regions come from
tools/telemetry.py.  Not a bench.py line."""
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

SHAPES = [(1_000_000, 1024, 512), (100_000, 256, 128)]
SEGMENT_SHAPE = (1_000_000, 1024, 512)
LAUNCHES = 5           # runs per recorded graph
HBM_BYTES_PER_S = 8e12
MFMA_FLOP_PER_S = 2.5e15
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


def report(res, floor, ours, base):
    for name, (us, lo, hi) in res.items():
        say(f"  {name:44s} {us:10.1f} us/call (min {lo:.1f}, max {hi:.1f}); {us / floor:7.2f} x floor")
    say(f"  {ours} / {base}: {res[ours][0] / res[base][0]:.2f}")


def filled_gallery(N, E, gen):
    gallery = tfimm.Gallery(E, capacity=N)
    for lo in range(0, N, 100_000):                                      # filled in slices: no float32 copy of the whole gallery
        n = min(100_000, N - lo)
        x = torch.randn(n, E, generator=gen).to("cuda")
        gallery.add(x / x.norm(dim=1, keepdim=True))
    return gallery


def centroids_of(gallery, nc, gen):
    """nc distinct rows of the gallery as a bf16 matrix with the gallery's pitch"""
    pick = torch.randperm(len(gallery), generator=gen)[:nc].to("cuda")
    return gallery._buf[pick].contiguous()


def assign_level(gallery, cen, rounds):
    N, E, nc = len(gallery), gallery.dim, cen.shape[0]
    g = gallery._buf[:N]
    out = {}

    def ours():
        out["ours"] = gallery._launch_assign(cen, gallery.pitch, nc)

    def baseline():
        out["base"] = (g @ cen.T).max(1)

    res, t = race({"tfimm_hip_cluster_assign": ours, "torch bf16 matmul + max": baseline}, rounds)
    torch.cuda.synchronize()
    agree = float((out["ours"][0].long() == out["base"].indices).float().mean())
    bytes_floor = (2 * N * E + 2 * nc * E + 8 * N) / HBM_BYTES_PER_S * 1e6
    flop_floor = 2 * N * nc * E / MFMA_FLOP_PER_S * 1e6
    floor = max(bytes_floor, flop_floor)
    say(f"assign N={N} C={nc} E={E}: byte floor {bytes_floor:.1f} us at 8 TB/s, flop floor {flop_floor:.1f} us at 2.5 PFLOP/s; same "
        f"centroid as the baseline in {agree * 100:.2f} % of the rows (the baseline rounds its scores to bf16)")
    report(res, floor, "tfimm_hip_cluster_assign", "torch bf16 matmul + max")
    ours_us = res["tfimm_hip_cluster_assign"][0]
    say(f"  tfimm_hip_cluster_assign: {2 * N * nc * E / ours_us / 1e6:.0f} TFLOP/s")
    telemetry_line(t)
    del out
    torch.cuda.empty_cache()


def segment_level(gallery, nc, skewed, rounds):
    M, E = len(gallery), gallery.dim
    gen = torch.Generator().manual_seed(7)
    groups = torch.randint(0, nc, (M,), generator=gen, dtype=torch.int32)
    if skewed:
        groups[torch.randperm(M, generator=gen)[:M // 2]] = 0           # one segment holds half the rows (and its share)
    groups = groups.to("cuda")
    g = gallery._buf[:M, :E]
    ordered, order = torch.sort(groups, stable=True)
    offsets = torch.searchsorted(ordered, torch.arange(nc + 1, dtype=torch.int32, device="cuda"), out_int32=True).contiguous()
    rows = order.to(torch.int32).contiguous()
    need = ffi.lib.tfimm_hip_segment_mean_workspace(M, nc, E)
    work = torch.empty(int(need), dtype=torch.uint8, device="cuda")
    mean = torch.empty((nc, E), dtype=torch.float32, device="cuda")
    counts = torch.empty(nc, dtype=torch.int32, device="cuda")
    sizes = torch.zeros(nc, dtype=torch.float32, device="cuda").scatter_add_(0, groups.long(), torch.ones(M, device="cuda"))
    which = groups.long()
    out = {}

    def ours():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_segment_mean(gallery._buf.data_ptr(), gallery.pitch, M, E, rows.data_ptr(), M, offsets.data_ptr(),
                                                 nc, mean.data_ptr(), E, counts.data_ptr(), work.data_ptr(), work.numel(), st),
                  "tfimm_hip_segment_mean")

    def baseline():
        sums = torch.zeros((nc, E), dtype=torch.float32, device="cuda").index_add_(0, which, g.float())
        out["base"] = sums / sizes.clamp(min=1)[:, None]

    res, t = race({"tfimm_hip_segment_mean": ours, "torch index_add_ + division": baseline}, rounds)
    torch.cuda.synchronize()
    err = float((mean - out["base"]).abs().max())
    floor = (2 * M * E + 4 * M + 4 * nc * E) / HBM_BYTES_PER_S * 1e6
    say(f"segment_mean M={M} E={E} C={nc}, {'one segment holds half the rows' if skewed else 'balanced segments'} (largest "
        f"{int(sizes.max())}): byte floor {floor:.1f} us at 8 TB/s; max |mean - baseline| {err:.2e}")
    report(res, floor, "tfimm_hip_segment_mean", "torch index_add_ + division")
    telemetry_line(t)
    del out
    torch.cuda.empty_cache()


def iteration_level(gallery, cen0, rounds):
    N, E, nc = len(gallery), gallery.dim, cen0.shape[0]
    g = gallery._buf[:N, :E]
    cen = cen0.clone()
    tcen = cen0[:, :E].clone()
    ones = torch.ones(N, device="cuda")

    def ours():
        a, _ = gallery._launch_assign(cen, gallery.pitch, nc)
        mean, counts = gallery._segment_means(a, nc)
        new = gallery._normalize(mean).to(torch.bfloat16)
        cen[:, :E] = torch.where((counts > 0)[:, None], new, cen[:, :E])

    def baseline():
        a = (g @ tcen.T).argmax(1)
        sums = torch.zeros((nc, E), dtype=torch.float32, device="cuda").index_add_(0, a, g.float())
        counts = torch.zeros(nc, dtype=torch.float32, device="cuda").scatter_add_(0, a, ones)
        mean = sums / counts.clamp(min=1)[:, None]
        new = (mean / mean.norm(dim=1, keepdim=True).clamp(min=1e-6)).to(torch.bfloat16)
        tcen.copy_(torch.where((counts > 0)[:, None], new, tcen))

    res, t = race({"assign + CSR + segment_mean + normalise": ours, "torch matmul + argmax + index_add_ + normalise": baseline},
                  rounds)
    floor = max(2 * N * E * 2 / HBM_BYTES_PER_S, 2 * N * nc * E / MFMA_FLOP_PER_S) * 1e6
    say(f"one k-means iteration N={N} C={nc} E={E} (the centroids move on from run to run on both sides); floor: the gallery read "
        f"twice or the flops of the assignment, {floor:.1f} us")
    report(res, floor, "assign + CSR + segment_mean + normalise", "torch matmul + argmax + index_add_ + normalise")
    telemetry_line(t)
    torch.cuda.empty_cache()


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 20
    if not torch.cuda.is_available():
        sys.exit("cluster_probe needs a GPU: nothing here can be measured without one")
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"graphs of {LAUNCHES} runs, the arms replayed alternately, median of {rounds} rounds after 3 warm-up rounds; L2-normalised "
        f"standard normal rows, the centroids are rows of the gallery")
    for N, nc, E in SHAPES:
        gen = torch.Generator().manual_seed(2021)
        gallery = filled_gallery(N, E, gen)
        cen = centroids_of(gallery, nc, gen)
        assign_level(gallery, cen, rounds)
        if (N, nc, E) == SEGMENT_SHAPE:
            segment_level(gallery, nc, False, rounds)
            segment_level(gallery, nc, True, rounds)
        iteration_level(gallery, cen, rounds)
        del gallery, cen
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

"""What the coarse-to-fine gallery search costs and finds, in ONE process:

    python tools/search_coarse_probe.py [--rounds R] [--out FILE]

Per shape (B, N, E, k) -- the seven of tools/search_wide_probe.py -- up to five arms: the LIST path (tfimm_hip_embed_search,
k <= 64 only), the BUFFER path (tfimm_hip_embed_search_wide), COARSE (tfimm_hip_embed_search_coarse) with the default
``candidates = min(max(4 k, 32), 256)`` and with ``candidates = 256``, and the torch baseline
``(q.bfloat16() @ g.T).float().topk(k)`` (probe only, never on the product path).  Each arm is a captured graph of LAUNCHES
searches; the arms are replayed alternately (R rounds after a warm-up, HIP events around each replay); microseconds per search
as median (min - max).  Floors at 8 TB/s: N * E * 2 bytes for the exact paths, N * (E + 1) for the fp8 scan.  The three passes
of a coarse search are timed apart in a run of their own outside the timed rounds: ten eager searches under ``torch.profiler``,
kernel time by kernel name.  Recall: the share of the exact path's indices that the coarse result holds, per query, on the
probe's data (standard normal rows); the bits of the outputs are compared as well.  The row quantisation is timed once per
gallery.  Shader clock and socket power over the timed regions come from tools/telemetry.py.  Not a bench.py line."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tensorflow-image-models_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tfimm.engine import ffi  # noqa: E402

SHAPES = [(32, 1_000_000, 512, 5), (32, 1_000_000, 512, 20), (32, 1_000_000, 512, 64), (32, 1_000_000, 512, 200),
          (32, 1_000_000, 128, 64), (256, 100_000, 512, 20), (256, 100_000, 512, 200)]
LAUNCHES = 10          # searches per recorded graph
HBM_BYTES_PER_S = 8e12
LIST, BUFFER, TORCH = "list   tfimm_hip_embed_search", "buffer tfimm_hip_embed_search_wide", "torch  matmul + topk"
COARSE = "coarse tfimm_hip_embed_search_coarse"
PASSES = ("embed_coarse_pass1", "embed_coarse_pass2", "embed_coarse_rerank")
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
    fn()                              # function attributes, workspaces and torch's own set-up stay outside the recording
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for _ in range(LAUNCHES):
            fn()
    return graph


_GALLERY = {}


def gallery(N, E):
    """(bf16 rows, e4m3 codes, int8 exponents) of a (N, E), seeded; one gallery at a time on the device"""
    if (N, E) not in _GALLERY:
        _GALLERY.clear()
        torch.cuda.empty_cache()
        gen = torch.Generator().manual_seed(2021)
        g = torch.empty(N, E, dtype=torch.bfloat16, device="cuda")
        for lo in range(0, N, 100_000):                                  # filled in slices: no float32 copy of the gallery
            g[lo:lo + 100_000] = torch.randn(min(100_000, N - lo), E, generator=gen).to("cuda")
        codes = torch.empty(N, E, dtype=torch.uint8, device="cuda")
        exps = torch.empty(N, dtype=torch.int8, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        times = []
        for _ in range(4):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ffi.check(ffi.lib.tfimm_hip_embed_quantize_rows(g.data_ptr(), E, N, E, codes.data_ptr(), E, exps.data_ptr(), st),
                      "tfimm_hip_embed_quantize_rows")
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        say(f"gallery N={N} E={E}: tfimm_hip_embed_quantize_rows {min(times[1:]):.1f} us (best of 3 after one; "
            f"{N * E * 3 / HBM_BYTES_PER_S * 1e6:.1f} us for {N * E * 3} bytes read and written at 8 TB/s)")
        _GALLERY[(N, E)] = (g, codes, exps)
    return _GALLERY[(N, E)]


def exact(entry, q, g, B, N, E, k):
    need = getattr(ffi.lib, entry + "_workspace")(B, N, E, k, 0)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    scores = torch.empty(B, k, dtype=torch.float32, device="cuda")
    indices = torch.empty(B, k, dtype=torch.int32, device="cuda")

    def search():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(getattr(ffi.lib, entry)(q.data_ptr(), E, B, g.data_ptr(), E, N, E, k, 0, scores.data_ptr(), indices.data_ptr(),
                                          work.data_ptr(), need, st), entry)
    # the graph holds the workspace's address, not the tensor: it stays referenced for as long as the graph is replayed
    return dict(graph=record(search), times=[], scores=scores, indices=indices, workspace=work)


def coarse(q, g, codes, exps, B, N, E, k, c):
    need = ffi.lib.tfimm_hip_embed_search_coarse_workspace(B, N, E, k, c, 0)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    scores = torch.empty(B, k, dtype=torch.float32, device="cuda")
    indices = torch.empty(B, k, dtype=torch.int32, device="cuda")

    def search():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_embed_search_coarse(q.data_ptr(), E, B, g.data_ptr(), E, codes.data_ptr(), E, exps.data_ptr(), N, E,
                                                        k, c, 0, scores.data_ptr(), indices.data_ptr(), work.data_ptr(), need, st),
                  "tfimm_hip_embed_search_coarse")
    return dict(graph=record(search), times=[], scores=scores, indices=indices, search=search, c=c)


def passes(search):
    """microseconds of kernel time per search for each of the three passes: ten eager searches under torch.profiler"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(10):
                search()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for name in PASSES:
                if name in ev.key:
                    total = getattr(ev, "device_time_total", None)
                    out[name] = out.get(name, 0.0) + (ev.cuda_time_total if total is None else total) / 10
        return out if len(out) == len(PASSES) else f"the profiler named {sorted(out)} of the three kernels"
    except Exception as e:  # noqa: BLE001  (a box without a tracer still measures the whole)
        return f"unavailable ({type(e).__name__}: {e})"


def recall(got, want):
    """the mean share of a query's exact indices that the coarse result holds"""
    hit = (got.long()[:, :, None] == want.long()[:, None, :]).any(1).float().mean()
    return float(hit)


def shape_level(shape, rounds):
    B, N, E, k = shape
    g, codes, exps = gallery(N, E)
    q = torch.randn(B, E, generator=torch.Generator().manual_seed(B + k)).to("cuda")
    base = {}

    def baseline():
        base["out"] = (q.bfloat16() @ g.T).float().topk(k)

    most = ffi.lib.tfimm_hip_embed_search_coarse_max_candidates(E)
    default = min(max(4 * k, 32), most, N)
    arms = {}
    if k <= ffi.EMBED_MAX_K:
        arms[LIST] = exact("tfimm_hip_embed_search", q, g, B, N, E, k)
    arms[BUFFER] = exact("tfimm_hip_embed_search_wide", q, g, B, N, E, k)
    names = []
    for c in sorted({default, min(most, N)}):
        if c >= k:
            names.append(f"{COARSE} c={c}")
            arms[names[-1]] = coarse(q, g, codes, exps, B, N, E, k, c)
    arms[TORCH] = dict(graph=record(baseline), times=[])
    for a in arms.values():
        a["graph"].replay()
    torch.cuda.synchronize()
    for _ in range(3):
        for a in arms.values():
            timed_replay(a["graph"])
    t = telemetry()
    for _ in range(rounds):
        for a in arms.values():
            a["times"].append(timed_replay(a["graph"]) / LAUNCHES * 1e3)
    floor, scan = N * E * 2 / HBM_BYTES_PER_S * 1e6, N * (E + 1) / HBM_BYTES_PER_S * 1e6
    say(f"B={B} N={N} E={E} k={k}: one-read floor of the exact paths {floor:.1f} us, stream floor of the fp8 scan "
        f"(N * (E + 1) bytes) {scan:.1f} us")
    for name, a in arms.items():
        a["us"], a["min"] = float(np.median(a["times"])), min(a["times"])
        say(f"  {name:42s} {a['us']:10.1f} us/search (min {a['min']:.1f}, max {max(a['times']):.1f}); "
            f"{a['us'] / (scan if name in names else floor):7.1f} x its floor")
    telemetry_line(t)
    best_exact = min(arms[n]["us"] for n in (LIST, BUFFER) if n in arms)
    for name in names:
        a, want = arms[name], arms[BUFFER]
        same = torch.equal(a["indices"], want["indices"]) and torch.equal(a["scores"].view(torch.int32), want["scores"].view(torch.int32))
        say(f"  {name}: recall against the exact path {recall(a['indices'], want['indices']) * 100:.3f} %, outputs "
            f"{'bit-equal to' if same else 'DIFFERENT from'} the exact path's; coarse / best exact path {a['us'] / best_exact:.2f}, "
            f"coarse / torch {a['us'] / arms[TORCH]['us']:.2f}")
        p = passes(a["search"])
        if isinstance(p, dict):
            whole = sum(p.values())
            say("    kernel time per search: " + ", ".join(f"{n} {p[n]:.1f} us ({p[n] / whole * 100:.0f} %)" for n in PASSES) +
                f"; pass 1 is {p[PASSES[0]] / scan:.1f} x the scan's stream floor")
        else:
            say(f"    kernel time per pass: {p}")
    return {n: arms[n]["us"] for n in arms}


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 30
    if not torch.cuda.is_available():
        sys.exit("search_coarse_probe needs a GPU: nothing here can be measured without one")
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"graphs of {LAUNCHES} launches, the arms replayed alternately, {rounds} rounds after 3 warm-up rounds")
    rows = []
    for shape in SHAPES:
        us = shape_level(shape, rounds)
        first = next(n for n in us if n.startswith(COARSE))
        rows.append((shape, us[first], min(us[n] for n in (LIST, BUFFER) if n in us), us[TORCH]))
    say("coarse (default candidates) against the better exact path and against torch, medians:")
    for (B, N, E, k), c, e, t in rows:
        say(f"  B={B} N={N} E={E} k={k}: coarse {c:.1f} us, exact {e:.1f} us ({c / e:.2f}), torch {t:.1f} us ({c / t:.2f})")


if __name__ == "__main__":
    main()

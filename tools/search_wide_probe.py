"""What the two selections of the gallery search cost, in ONE process:

    python tools/search_wide_probe.py [--rounds R] [--out FILE]

Per shape (B, N, E, k) three arms: the LIST path (tfimm_hip_embed_search, k <= 64 only), the BUFFER path
(tfimm_hip_embed_search_wide) and the torch baseline ``(q.bfloat16() @ g.T).float().topk(k)`` (probe only, never on the product
path).  Each arm is a captured graph of LAUNCHES searches; the arms are replayed alternately (R rounds after a warm-up, HIP
events around each replay); microseconds per search as median (min - max), against the one-read floor N * E * 2 bytes / 8 TB/s.
Shapes: (32, 1 000 000, 512, k) for k in 5, 20, 64, 200; (32, 1 000 000, 128, 64), the bold row of DESIGN.md 3.18;
(256, 100 000, 512, k) for k in 20, 200.  Where both of our paths run, their outputs are compared bit for bit.  The last lines
name the switch-over of ``Gallery.search`` (``search_with(method="auto")``): the smallest k from which the buffer path's median lies below the
list path's minimum at every probed shape of that k.  Shader clock and socket power over the timed regions come from
tools/telemetry.py.  Not a bench.py line."""
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
    """the bf16 gallery of a (N, E), seeded; one at a time on the device"""
    if (N, E) not in _GALLERY:
        _GALLERY.clear()
        torch.cuda.empty_cache()
        gen = torch.Generator().manual_seed(2021)
        g = torch.empty(N, E, dtype=torch.bfloat16, device="cuda")
        for lo in range(0, N, 100_000):                                  # filled in slices: no float32 copy of the gallery
            g[lo:lo + 100_000] = torch.randn(min(100_000, N - lo), E, generator=gen).to("cuda")
        _GALLERY[(N, E)] = g
    return _GALLERY[(N, E)]


def ours(entry, q, g, B, N, E, k):
    need = getattr(ffi.lib, entry + "_workspace")(B, N, E, k, 0)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    scores = torch.empty(B, k, dtype=torch.float32, device="cuda")
    indices = torch.empty(B, k, dtype=torch.int32, device="cuda")

    def search():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(getattr(ffi.lib, entry)(q.data_ptr(), E, B, g.data_ptr(), E, N, E, k, 0, scores.data_ptr(), indices.data_ptr(),
                                          work.data_ptr(), need, st), entry)
    return dict(graph=record(search), times=[], scores=scores, indices=indices, workspace=need)


def shape_level(shape, rounds):
    B, N, E, k = shape
    g = gallery(N, E)
    q = torch.randn(B, E, generator=torch.Generator().manual_seed(B + k)).to("cuda")
    base = {}

    def baseline():
        base["out"] = (q.bfloat16() @ g.T).float().topk(k)

    arms = {}
    if k <= ffi.EMBED_MAX_K:
        arms[LIST] = ours("tfimm_hip_embed_search", q, g, B, N, E, k)
    arms[BUFFER] = ours("tfimm_hip_embed_search_wide", q, g, B, N, E, k)
    arms[TORCH] = dict(graph=record(baseline), times=[])
    for a in arms.values():
        a["graph"].replay()
    torch.cuda.synchronize()
    same = "not compared (k > 64: the list path refuses)"
    if LIST in arms:
        same = "bit-equal" if torch.equal(arms[LIST]["indices"], arms[BUFFER]["indices"]) and \
            torch.equal(arms[LIST]["scores"].view(torch.int32), arms[BUFFER]["scores"].view(torch.int32)) else "DIFFERENT"
    agree = float((arms[BUFFER]["indices"].long() == base["out"].indices).float().mean())
    for _ in range(3):
        for a in arms.values():
            timed_replay(a["graph"])
    t = telemetry()
    for _ in range(rounds):
        for a in arms.values():
            a["times"].append(timed_replay(a["graph"]) / LAUNCHES * 1e3)
    floor = N * E * 2 / HBM_BYTES_PER_S * 1e6
    say(f"B={B} N={N} E={E} k={k}: one-read floor {floor:.1f} us; buffer workspace {arms[BUFFER]['workspace']} bytes; list and "
        f"buffer outputs: {same}; buffer indices equal to torch's at {agree * 100:.2f} % of the positions (torch rounds its scores "
        f"to bf16)")
    for name, a in arms.items():
        a["us"], a["min"] = float(np.median(a["times"])), min(a["times"])
        say(f"  {name:34s} {a['us']:10.1f} us/search (min {a['min']:.1f}, max {max(a['times']):.1f}); {a['us'] / floor:7.1f} x floor")
    if LIST in arms:
        say(f"  buffer / list: {arms[BUFFER]['us'] / arms[LIST]['us']:.2f}   (buffer median {arms[BUFFER]['us']:.1f} against list minimum "
            f"{arms[LIST]['min']:.1f}: {'below' if arms[BUFFER]['us'] < arms[LIST]['min'] else 'NOT below'})")
    say(f"  buffer / torch: {arms[BUFFER]['us'] / arms[TORCH]['us']:.2f}")
    telemetry_line(t)
    return None if LIST not in arms else arms[BUFFER]["us"] < arms[LIST]["min"]


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 30
    if not torch.cuda.is_available():
        sys.exit("search_wide_probe needs a GPU: nothing here can be measured without one")
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"graphs of {LAUNCHES} launches, the arms replayed alternately, {rounds} rounds after 3 warm-up rounds")
    wins = {}
    for shape in SHAPES:
        won = shape_level(shape, rounds)
        if won is not None:
            wins.setdefault(shape[3], []).append(won)
    ks = sorted(wins)
    say("buffer median below list minimum at every probed shape of k: " + ", ".join(f"k={k}: {'yes' if all(wins[k]) else 'no'}" for k in ks))
    first = next((k for i, k in enumerate(ks) if all(all(wins[j]) for j in ks[i:])), None)
    say(f"switch-over of method=\"auto\": " + (f"k = {first} (the smallest probed k from which the buffer path wins at every shape)"
                                              if first is not None else "none: the list path keeps every k <= 64"))


if __name__ == "__main__":
    main()

"""What the embedding end costs, in ONE process:

    python tools/embed_probe.py [--rounds R] [--out FILE] [--skip-models]

(1) tfimm_hip_embed_search (both passes) at (B, N, E, k) = (1, 100 000, 512, 5), (32, 1 000 000, 512, 5),
(256, 1 000 000, 512, 5), (32, 1 000 000, 128, 64): per shape a captured graph of LAUNCHES searches and a captured graph of
LAUNCHES runs of the torch baseline ``(q.bfloat16() @ g.T).float().topk(k)`` (probe only, never on the product path), the two
replayed alternately (R rounds after a warm-up, HIP events around each replay); microseconds per search against the one-read
floor N * E * 2 bytes / 8 TB/s.  Re-reads of the gallery for further query tiles are the kernel's own choice and count
against it.
(2) resnet50 at batch 256: the recording of ``EmbeddingModel(resnet50, 512, normalize=True)`` against the recording of the
backbone's ``forward_features`` program (same seeded weights and input), replayed alternately, ms per replay.
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
from tfimm.utils.init import synthetic_weights  # noqa: E402

SHAPES = [(1, 100_000, 512, 5), (32, 1_000_000, 512, 5), (256, 1_000_000, 512, 5), (32, 1_000_000, 128, 64)]
MODEL, BATCH, EMBED = "resnet50", 256, 512
LAUNCHES = 20          # searches per recorded graph of part (1)
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
    fn()                              # function attributes, workspaces and torch's own set-up stay outside the recording
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for _ in range(LAUNCHES):
            fn()
    return graph


def op_level(shape, rounds):
    B, N, E, k = shape
    gen = torch.Generator().manual_seed(2021)
    q = torch.randn(B, E, generator=gen).to("cuda")
    g = torch.empty(N, E, dtype=torch.bfloat16, device="cuda")
    for lo in range(0, N, 100_000):                                      # filled in slices: no second float32 copy of the gallery
        g[lo:lo + 100_000] = torch.randn(min(100_000, N - lo), E, generator=gen).to("cuda")
    need = ffi.lib.tfimm_hip_embed_search_workspace(B, N, E, k, 0)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    scores = torch.empty(B, k, dtype=torch.float32, device="cuda")
    indices = torch.empty(B, k, dtype=torch.int32, device="cuda")
    base = {}

    def search():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_embed_search(q.data_ptr(), E, B, g.data_ptr(), E, N, E, k, 0, scores.data_ptr(),
                                                 indices.data_ptr(), work.data_ptr(), need, st), "tfimm_hip_embed_search")

    def baseline():
        base["out"] = (q.bfloat16() @ g.T).float().topk(k)

    arms = {"tfimm_hip_embed_search": dict(graph=record(search), times=[]),
            "torch matmul + topk": dict(graph=record(baseline), times=[])}
    for a in arms.values():
        a["graph"].replay()
    torch.cuda.synchronize()
    agree = float((indices.long() == base["out"].indices).float().mean())
    for _ in range(3):
        for a in arms.values():
            timed_replay(a["graph"])
    t = telemetry()
    for _ in range(rounds):
        for a in arms.values():
            a["times"].append(timed_replay(a["graph"]) / LAUNCHES * 1e3)
    floor = N * E * 2 / HBM_BYTES_PER_S * 1e6
    say(f"B={B} N={N} E={E} k={k}: one-read floor {floor:.1f} us; workspace {need} bytes; indices equal to the baseline's at "
        f"{agree * 100:.2f} % of the positions (the baseline rounds its scores to bf16)")
    for name, a in arms.items():
        us = float(np.median(a["times"]))
        a["us"] = us
        say(f"  {name:24s} {us:10.1f} us/search (min {min(a['times']):.1f}, max {max(a['times']):.1f}); {us / floor:7.1f} x floor")
    say(f"  search / baseline: {arms['tfimm_hip_embed_search']['us'] / arms['torch matmul + topk']['us']:.2f}")
    telemetry_line(t)
    del g, base
    torch.cuda.empty_cache()


def model_level(rounds):
    bb = tfimm.create_model(MODEL)
    bb.set_weights(synthetic_weights(bb, 2021))
    m = tfimm.EmbeddingModel(bb, EMBED, normalize=True)
    gen = torch.Generator().manual_seed(2021)
    x = torch.randn(BATCH, *bb.cfg.input_size, bb.cfg.in_channels, generator=gen).to("cuda", torch.bfloat16)
    bare = tfimm.create_model(MODEL, nb_classes=0)                       # the forward_features program: no classifier
    bare.set_weights({k: v for k, v in bb.weights.items() if k in bare.weights})
    arms = {}
    for arm, model in (("forward_features", bare), ("EmbeddingModel", m)):
        prog = model.program()
        plan = prog.make_plan(BATCH)
        cap = plan.capture(x)
        cap.replay()
        torch.cuda.synchronize()
        arms[arm] = dict(cap=cap, plan=plan, prog=prog, times=[])
    for _ in range(5):
        for a in arms.values():
            timed_replay(a["cap"].graph)
    t = telemetry()
    for _ in range(rounds):
        for a in arms.values():
            a["times"].append(timed_replay(a["cap"].graph))
    e = arms["EmbeddingModel"]["prog"].outputs["embeddings"]
    say(f"{MODEL} batch {BATCH}, embed_dim {EMBED}, normalize=True (embeddings per image: {e.rows} x {e.C}): {rounds} replays per "
        f"arm, alternating")
    for arm, a in arms.items():
        a["ms"] = float(np.median(a["times"]))
        say(f"  {arm:18s} {a['ms']:9.4f} ms/replay (min {min(a['times']):.4f}, max {max(a['times']):.4f}; {len(a['prog'].ops)} ops)")
    d = arms["EmbeddingModel"]["ms"] - arms["forward_features"]["ms"]
    say(f"  EmbeddingModel - forward_features: {d * 1e3:+.1f} us per replay ({d / arms['forward_features']['ms'] * 100:+.3f} %)")
    telemetry_line(t)


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 30
    if not torch.cuda.is_available():
        sys.exit("embed_probe needs a GPU: nothing here can be measured without one")
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"graphs of {LAUNCHES} launches, the two arms replayed alternately, {rounds} rounds after 3 warm-up rounds")
    for shape in SHAPES:
        op_level(shape, rounds)
    if "--skip-models" not in sys.argv:
        model_level(rounds)


if __name__ == "__main__":
    main()

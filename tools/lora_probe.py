"""What the unmerged LoRA path costs, in ONE process:

    python tools/lora_probe.py [--rounds R] [--out FILE] [--skip-models]

(1) tfimm_hip_lora_delta alone at the fc1 / fc2 shapes of convnext_tiny's first and third stage at batch 256, rank 4 and rank 64:
a captured graph of LAUNCHES launches per shape, replayed R times after a warm-up (HIP events around each replay); microseconds
per launch against the one-read floor -- x and the residual read once, out written once: M * (K + N [+ N]) * 2 bytes / 8 TB/s.
What the kernel re-reads of A and B' (L2 resident) is its own choice and counts against it.
(2) convnext_tiny at batch 256: the recording of the unmerged program at rank 4 and at rank 64 against the recording of the
merged program (= the base model's program), same seeded weights and input, replayed alternately, ms per replay.
Shader clock and socket power over the timed regions come from tools/telemetry.py.  Not a bench.py line."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tensorflow-image-models_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tfimm  # noqa: F401,E402
from tfimm.architectures.lora import create_model, merge_lora_weights  # noqa: E402
from tfimm.engine import ffi  # noqa: E402
from tfimm.utils.init import synthetic_weights  # noqa: E402

MODEL, BATCH = "convnext_tiny", 256
# (rows per image, K, N, residual): fc1 and fc2 of stage 0 (56 x 56, D = 96) and of stage 2 (14 x 14, D = 384)
LAYERS = [(3136, 96, 384, False), (3136, 384, 96, True), (196, 384, 1536, False), (196, 1536, 384, True)]
RANKS = (4, 64)
LAUNCHES = 20
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


def op_level(layer, rank, rounds):
    rows, K, N, residual = layer
    M, Rp = BATCH * rows, -(-rank // 16) * 16
    gen = torch.Generator().manual_seed(2021)
    x = torch.randn(M, K, generator=gen).to("cuda", torch.bfloat16)
    a = torch.zeros(Rp, K)
    a[:rank] = torch.randn(rank, K, generator=gen) / K ** 0.5
    b = torch.zeros(N, Rp)
    b[:, :rank] = torch.randn(N, rank, generator=gen) / rank ** 0.5
    a, b = a.to("cuda", torch.bfloat16), b.to("cuda", torch.bfloat16)
    res = torch.randn(M, N, generator=gen).to("cuda", torch.bfloat16) if residual else None
    out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    d = ffi.LoraDesc()
    d.x, d.a, d.b, d.out = x.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr()
    d.residual = res.data_ptr() if residual else None
    d.M, d.K, d.N, d.Rp, d.lda, d.lda_a, d.ldr, d.ldc = M, K, N, Rp, K, K, N, N

    def launch():
        ffi.check(ffi.lib.tfimm_hip_lora_delta(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tfimm_hip_lora_delta")

    launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for _ in range(LAUNCHES):
            launch()
    for _ in range(3):
        timed_replay(graph)
    times = [timed_replay(graph) / LAUNCHES * 1e3 for _ in range(rounds)]
    nbytes = M * (K + N * (2 if residual else 1)) * 2
    floor = nbytes / HBM_BYTES_PER_S * 1e6
    us = float(np.median(times))
    say(f"M={M} K={K} N={N} rank={rank} (Rp={Rp}) residual={'yes' if residual else 'no'}: {nbytes / 1e6:.1f} MB, one-read floor "
        f"{floor:.1f} us; {us:.1f} us/launch (min {min(times):.1f}, max {max(times):.1f}); {us / floor:.2f} x floor, "
        f"{nbytes / us / 1e6:.2f} TB/s")
    del x, out, res
    torch.cuda.empty_cache()


def model_level(rounds):
    gen = torch.Generator().manual_seed(2021)
    arms = {}
    x = None
    for arm, rank, merged in (("merged (base program)", 4, True), ("unmerged rank 4", 4, False), ("unmerged rank 64", 64, False)):
        model = create_model(MODEL, lora_rank=rank, lora_alpha=float(rank))
        model.set_weights(synthetic_weights(model, 2021))          # (synthetic B is not zero)
        if merged:
            merge_lora_weights(model)
        if x is None:
            x = torch.randn(BATCH, *model.cfg.input_size, model.cfg.in_channels, generator=gen).to("cuda", torch.bfloat16)
        prog = model.program()
        plan = prog.make_plan(BATCH)
        cap = plan.capture(x)
        cap.replay()
        torch.cuda.synchronize()
        arms[arm] = dict(cap=cap, plan=plan, prog=prog, model=model, times=[])
    for _ in range(5):
        for a in arms.values():
            timed_replay(a["cap"].graph)
    t = telemetry()
    for _ in range(rounds):
        for a in arms.values():
            a["times"].append(timed_replay(a["cap"].graph))
    say(f"{MODEL} batch {BATCH}: {rounds} replays per arm, alternating")
    for arm, a in arms.items():
        a["ms"] = float(np.median(a["times"]))
        kinds = [op.kind for op in a["prog"].ops]
        say(f"  {arm:22s} {a['ms']:9.4f} ms/replay (min {min(a['times']):.4f}, max {max(a['times']):.4f}; {len(kinds)} ops, "
            f"{kinds.count('lora_delta')} lora_delta, {kinds.count('gemm')} gemm, {kinds.count('mlp_fused')} mlp_fused)")
    base = arms["merged (base program)"]["ms"]
    for arm in ("unmerged rank 4", "unmerged rank 64"):
        say(f"  {arm} / merged: {arms[arm]['ms'] / base:.3f}")
    telemetry_line(t)


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 30
    if not torch.cuda.is_available():
        sys.exit("lora_probe needs a GPU: nothing here can be measured without one")
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"graphs of {LAUNCHES} launches, {rounds} rounds after 3 warm-up rounds")
    for layer in LAYERS:
        for rank in RANKS:
            op_level(layer, rank, rounds)
    if "--skip-models" not in sys.argv:
        model_level(rounds)


if __name__ == "__main__":
    main()

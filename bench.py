#!/usr/bin/env python3
"""Forward-throughput benchmark of the tfimm hot path on MI355X (contract: see task brief).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--workload resnet50|vit_base_patch16_224|...] [--full]
                  [--dump-outputs DIR]

A plain run does only what its headline figure needs: set-up (including the choice of launch mode under --branches auto),
W warm-up steps, the K timed steps and the result line.  ``--full`` adds everything listed under "Printed JSON" below that
is not that figure: per-step medians, the sustained window and telemetry, per-kernel rooflines, the CPU baseline and parity
statements, the other BASELINE configurations (``also``) and the bit-equality checks of the launch modes and the exchange.
``--dump-outputs DIR`` writes the logits of the main workload's last timed step (and, N > 1, the gathered logits of all
ranks) as float32 ``DIR/logits.npy`` / ``DIR/gathered_logits.npy``; weights and inputs are seeded, so two builds run with the
same arguments can be compared output for output.

A "step" is one forward pass of the workload's model over one synthetic, already preprocessed bf16
batch that is resident in HBM before the timed region starts.  Weak scaling: every rank processes
its own fixed-size batch (``per_gpu_batch``) and the only exchange is an RCCL all-gather of the fp32
logits, inside the timed region: asynchronous and double-buffered, step i's ring pass runs
under step i + 1's kernels (tfimm/engine/dp.py PipelinedGather) and the last ones are drained before the clock stops.  ``value`` = images of all ranks / max-over-ranks
time of the MAIN workload (``--workload``, default resnet50 @224 B=256 = BASELINE.json configs[1]).

``--gpus N`` with N > 1 starts its own N ranks (``python -m torch.distributed.run``, one process per
GPU, rendezvous on 127.0.0.1) unless it already runs under a launcher (WORLD_SIZE set).

Printed JSON (one line, rank 0): metric / value / unit / ... plus
  roofline      achieved vs peak of the main workload's dominant kernel family: HIP events recorded
                around those launches on the launch stream over K eagerly launched steps,
  cpu_baseline  the fp32 CPU oracle (torch-CPU restatement of the reference, pinned to the reference's
                own code by tests/test_golden.py; TensorFlow itself is not installable) timed on a
                bounded sample of the same workload,
  parity_vs_oracle   top-1 match over 64 images + how many mismatches the oracle's own top-1 / top-2
                margin explains,
  parity        top level: per model the rel-to-max error and the top-1 figures (bf16 random head / calibrated head /
                float32 path) -- ResNet-50 AND ViT-B/16, the two models the metric names,
  energy        joules per step (mean socket power of the sustained window x its time per step) against the floor this part's
                energy per MFMA flop and per HBM byte set at its 1400-W cap,
  sclk_mhz_mean / power_w_mean / power_cap_w / telemetry / sustained
                shader clock and socket power of this box over the timed region (side-thread samples of the amdsmi
                gpu_metrics table, tfimm/utils/telemetry.py) and over >= 0.6 s of back-to-back replays; every workload
                under `also` carries the same fields,
  also          every other BASELINE.json configuration (ViT-B/16 B=512, Swin-B B=256,
                EfficientNet-B4 @380 B=256 per GPU), same protocol, each with its own roofline.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "tensorflow-image-models_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))       # telemetry.py: measurement tooling, not part of the product package

# What is inside the timed region, by number (frozen since round 5; see README "bench protocol"):
#   2 = K hipGraph replays (logits written by the recording's last node), the asynchronous double-buffered all-gather submitted per
#       step and drained before the clock stops; per-step event records in a pass of their own.  (1 = rounds 1-4: an event record and
#       a logits copy launch per step inside the region, the all-gather on the launch stream.)
PROTOCOL_VERSION = 2
LINE_LIMIT = 4096          # bytes of the ONE stdout line (the driver's parser lost round 5's 21-KB line); everything else -> detail file

# BASELINE.json configs -> (model, per-GPU batch, roofline bound, kernel family the roofline is quoted on)
#   mfma: achieved = FLOPs of the GEMM launches / their time
#   hbm:  achieved = algorithmic bytes (every conv / linear / attention output written once and read once
#         per consumer in bf16, input once, weights once per step) / time of the kernels that produce those outputs
WORKLOADS = {
    "resnet50": dict(model="resnet50", batch=256, bound="hbm", family=("gemm",)),
    "vit_base_patch16_224": dict(model="vit_base_patch16_224", batch=512, bound="mfma", family=("gemm",)),
    # HBM-bound under the layer-boundary byte convention (the MLP hidden tensor is written and read), MFMA-bound
    # if fc1 -> GELU -> fc2 were one kernel -- both bounds are reported (roofline.second_bound)
    "swin_base_patch4_window7_224": dict(model="swin_base_patch4_window7_224", batch=256, bound="hbm", second_bound="mfma",
                                         family=("gemm", "attention")),
    "efficientnet_b4": dict(model="efficientnet_b4", batch=256, bound="hbm", family=("gemm", "dwconv")),
    "vit_tiny_patch16_224": dict(model="vit_tiny_patch16_224", batch=1, bound="mfma", family=("gemm",)),
    "convnext_tiny": dict(model="convnext_tiny", batch=256, bound="hbm", family=("gemm", "dwconv")),
    "convnext_base": dict(model="convnext_base", batch=256, bound="hbm", family=("gemm", "dwconv")),
    "cait_xxs24_224": dict(model="cait_xxs24_224", batch=256, bound="mfma", family=("gemm",)),
}
DEFAULT_EXTRA = "vit_base_patch16_224,swin_base_patch4_window7_224,efficientnet_b4"
PEAK = {"hbm": (8000.0, "GB/s"), "mfma": (2500.0, "TFLOP/s")}   # MI355X_MICROARCH.md chip table (spec HBM, dense bf16)
# algorithmic activation bytes per image -- the HBM-roofline numerator
ALG_BYTES_PER_IMAGE = {"resnet50": 56.8e6, "swin_base_patch4_window7_224": 140.1e6, "efficientnet_b4": 205.2e6,
                       "vit_base_patch16_224": 80.8e6, "vit_tiny_patch16_224": 20.4e6}
# Energy coefficients of this part, measured with one resource busy at a time (profiles/r05_power.md, tools/probes/energy_probe.hip):
# joules above the idle floor per bf16 MFMA flop on random operands and per byte of HBM traffic (reads 0.14, writes 0.17 nJ/B on
# random data).  Every workload here runs at 0.88 .. 0.97 of the 1400-W socket cap, so a step cannot take less than
# (flops x E_MFMA + algorithmic bytes x E_HBM) / (cap - idle): the `energy` object of a workload states that floor next to the
# joules the step really took (mean socket power of the sustained window x its time per step).
E_MFMA_PJ_PER_FLOP, E_HBM_NJ_PER_BYTE, P_IDLE_W = 0.62, 0.15, 255.0
FAMILY_KERNELS = {"gemm": "tfimm_gemm::* (all GEMM / conv flavours) + stem_pool_kernel",
                  "attention": "attn_*_kernel", "dwconv": "dwconv_*_kernel + expand_dw_kernel"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default=os.environ.get("TFIMM_BENCH_WORKLOAD", "resnet50"), choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0, help="override per-GPU batch of the main workload")
    ap.add_argument("--branches", default=os.environ.get("TFIMM_BENCH_BRANCHES", "auto"),
                    help="'auto' (default): the batch is also recorded as two half-batch slices on parallel branches of one HIP "
                         "graph, both recordings are timed and the faster one runs in the timed region; 1 / 2: fixed")
    ap.add_argument("--micro-batch", type=int, default=int(os.environ.get("TFIMM_MICRO_BATCH", "0")))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-events", action="store_true")
    ap.add_argument("--no-graph", action="store_true", help="launch every op eagerly instead of replaying a hipGraph")
    ap.add_argument("--extra", default=os.environ.get("TFIMM_BENCH_EXTRA"),
                    help="comma separated further workloads measured after the main one (reported under 'also'); "
                         f"default: {DEFAULT_EXTRA} on one GPU, vit_base_patch16_224,efficientnet_b4 on several")
    ap.add_argument("--spawn", action="store_true", help="go through the rank launcher even for --gpus 1")
    ap.add_argument("--backend", default=os.environ.get("TFIMM_BENCH_BACKEND", "nccl"), choices=["nccl", "gloo"],
                    help="torch.distributed backend of the logits exchange: nccl (= RCCL over xGMI, one rank per GPU) or gloo "
                         "(host sockets; lets several ranks share one GPU -- how the N > 1 path is exercised on a 1-GPU box)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline figure (medians, telemetry, rooflines, CPU "
                         "baseline, parity, the other BASELINE configurations)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the main workload's logits of the last timed step to DIR/logits.npy (float32)")
    return ap.parse_args()


# ------------------------------------------------------------------------------------------------------------------
# rank launcher
# ------------------------------------------------------------------------------------------------------------------
def spawn_ranks(n: int) -> int:
    """Start ``n`` ranks of this script (one process per GPU) and relay rank 0's JSON line."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: RCCL needs it on this driver
    env["TFIMM_BENCH_SPAWNED"] = "1"
    argv = [a for a in sys.argv[1:] if a != "--spawn"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    return subprocess.run(cmd, env=env).returncode


# ------------------------------------------------------------------------------------------------------------------
# measurement
# ------------------------------------------------------------------------------------------------------------------
def measured_traffic(workload, batch):
    """HBM bytes per launch of the workload's roofline family from the rocprofv3 PMC passes COMMITTED under profiles/
    (FETCH_SIZE / WRITE_SIZE need their own profiler passes and cannot be collected from inside this process):
    tools/gpu_traffic.sh.  Returns (bytes per launch, source) -- a constant from that profile, not a counter of this run;
    None when no profile of this workload / batch exists."""
    for rel in ("r06_traffic.json", "r05_traffic.json", "r04_traffic.json"):            # the newest committed profile
        path = os.path.join(ROOT, "profiles", rel)
        if batch == WORKLOADS.get(workload, {}).get("batch") and os.path.exists(path):
            with open(path) as f:
                t = json.load(f).get("workloads", {}).get(workload)
            if t and "hbm_bytes_per_launch" in t:
                return (round(t["hbm_bytes_per_launch"]),
                        f"from committed profile profiles/{rel} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, "
                        "eager launches; not measured in this run)")
    return None, None


def build_model(name):
    import tfimm
    from tfimm.utils.init import synthetic_weights
    model = tfimm.create_model(name)
    model.set_weights(synthetic_weights(model, seed=2021))   # random-init weights of that architecture
    return model


def synthetic_batch(cfg, batch, seed):
    """default_rng-style [0, 1) pixels + the model's preprocessing, bf16, generated on the device."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(batch, *cfg.input_size, cfg.in_channels, device="cuda", generator=g)
    mean = torch.tensor(cfg.mean, device="cuda")
    std = torch.tensor([s if s else 1.0 for s in cfg.std], device="cuda")
    return ((x - mean) / std).to(torch.bfloat16).contiguous()


_CAPI = {}     # the C-ABI communicator of this process (one per run: RCCL communicators are not cheap)


def measure(model, batch, micro_batch, steps, warmup, world, kernel_events, dist, graph=True, branches="auto", full=True):
    """Timed region: barrier + sync, K steps, sync + barrier.  Returns seconds, per-kind kernel time, handles.
    ``full=False`` (a plain bench run): set-up, warm-up and the timed region only -- no telemetry, no bit-equality checks,
    no median / other-mode / sustained passes (their fields are None)."""
    import torch
    cfg = model.cfg
    x = synthetic_batch(cfg, batch, 2021 + (dist.get_rank() if dist is not None else 0))
    prog = model.program()
    mb = micro_batch or batch
    plans = {}
    for s in range(0, batch, mb):
        nb = min(mb, batch - s)
        if nb not in plans:
            plans[nb] = prog.make_plan(nb)
    out_t = prog.outputs["logits"]
    logits = torch.empty(batch, out_t.C, dtype=torch.float32, device="cuda")
    # the one exchange step: double-buffered and asynchronous -- the all-gather of step i runs on the
    # communicator's stream under the kernels of step i + 1 (tfimm/engine/dp.py PipelinedGather); TFIMM_BENCH_SYNC_GATHER=1
    # issues it the round-4 way (on the launch stream, between two replays) for the A/B under profiles/
    from tfimm.engine.dp import PipelinedGather
    from telemetry import Telemetry
    sync_gather = os.environ.get("TFIMM_BENCH_SYNC_GATHER") == "1"
    # TFIMM_DP_EXCHANGE=capi: the same pipelined exchange, the collective issued through the C ABI (include/tfimm_hip_dp.h:
    # a direct ncclAllGather call site, tfimm/engine/dp.py CapiComm) instead of torch.distributed -- opt-in
    comm = None
    if dist is not None and not sync_gather and os.environ.get("TFIMM_DP_EXCHANGE") == "capi" and dist.get_backend() == "nccl":
        from tfimm.engine.dp import CapiComm
        comm = _CAPI.get("comm") or _CAPI.setdefault("comm", CapiComm(dist))
    pipe = PipelinedGather(batch, out_t.C, torch.float32, "cuda", dist, comm=comm) if (dist is not None and not sync_gather) else None
    gathered = torch.empty(world * batch, out_t.C, dtype=torch.float32, device="cuda") if (dist is not None and sync_gather) else None
    tele = Telemetry(torch.cuda.current_device()) if full else None

    host_gather = dist is not None and dist.get_backend() == "gloo"
    use_graph = graph and mb == batch
    captured = None
    if use_graph:
        try:
            # `sink`: the recording's last node writes the fp32 logits into `logits` -- a step is ONE hipGraphLaunch
            captured = plans[batch].capture(x, sink=(out_t, logits))
        except RuntimeError as e:      # same launches one by one instead of one hipGraphLaunch; reported in config.launch
            print(f"warning: hipGraph recording failed ({e}); launching eagerly", file=sys.stderr)
            torch.cuda.synchronize()

    # The batch as two slices on PARALLEL branches of one HIP graph (engine/graph.py CapturedBranches: same kernels, bit-equal
    # results, launches of the two slices side by side).  "auto": both recordings are timed before the warm-up and the faster
    # one runs in the timed region; the choice and the other mode's time are reported (config.launch, single_branch_ms_per_step).
    forked, single_ms, forked_ms, hybrid_cut = None, None, None, None
    n_br = 2 if branches == "auto" else int(branches)
    if captured is not None and n_br > 1 and batch >= 2 * n_br and prog.supports_branches():
        from tfimm.engine.graph import CapturedBranches
        try:
            forked = CapturedBranches(prog.make_branches(batch, n_br), x, sink=(out_t, logits))
        except Exception as e:      # a recording that cannot be made must not cost the measurement: one branch
            print(f"warning: branch recording failed ({type(e).__name__}: {e}); one branch", file=sys.stderr)
            forked = None
            torch.cuda.synchronize()
        if forked is not None:
            def _time(g, n=5, rounds=3):
                """ms per replay of a recording: the best of `rounds` groups of `n` replays (one group of 5 picked among six
                recordings on what is partly clock noise: VERDICT r05 weak 8)"""
                for _ in range(2):
                    g.replay()
                best = float("inf")
                for _ in range(rounds):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for _ in range(n):
                        g.replay()
                    torch.cuda.synchronize()
                    best = min(best, (time.perf_counter() - t) / n * 1e3)
                return best
            single_ms, forked_ms = _time(captured), _time(forked)
            if branches == "auto":
                # ... and hybrids: branches for the first part of the program, the full batch for the rest (CapturedHybrid:
                # ResNet-50's 14 x 14 / 7 x 7 stages are too small to split).  A few cut positions, the fastest recording wins.
                from tfimm.engine.graph import CapturedHybrid
                n_ops = len(prog.ops)
                for frac in (0.5, 0.65, 0.8, 0.9):
                    try:
                        hyb = CapturedHybrid(prog, x, max(1, int(round(frac * n_ops))), sink=(out_t, logits))
                    except Exception as e:
                        print(f"warning: hybrid recording failed ({type(e).__name__}: {e})", file=sys.stderr)
                        torch.cuda.synchronize()
                        break
                    t_h = _time(hyb)
                    if t_h < 0.995 * forked_ms:          # (a recording replaces the incumbent only by more than the repeatability of _time)
                        forked, forked_ms, hybrid_cut = hyb, t_h, hyb.cut_op
                    else:
                        del hyb
                if forked_ms >= 0.995 * single_ms:
                    forked = None
    # the recording that will be timed must give the bits of the single-branch recording (checked once, before the warm-up)
    forked_bit_equal = None
    if forked is not None and full:
        captured.replay()
        one = logits.clone()
        assert torch.equal(one, plans[batch].tensor_view(out_t).view(batch, out_t.C).float()), "recorded sink differs from the plan's output"
        forked.replay()
        forked_bit_equal = bool(torch.equal(one, logits) and torch.equal(one, forked.output(out_t).view(batch, out_t.C).float()))
        torch.cuda.synchronize()

    def step(events=None):
        if forked is not None and events is None:
            forked.replay()                                # one hipGraphLaunch: both branches + the logits into `logits`
        elif captured is not None and events is None:
            captured.replay()                              # one hipGraphLaunch: the whole layer program + the logits into `logits`
        else:
            for s in range(0, batch, mb):
                nb = min(mb, batch - s)
                plan = plans[nb]
                if events is None:
                    plan.run(x[s:s + nb])
                else:
                    run_with_events(plan, x[s:s + nb], events)
                logits[s:s + nb].copy_(plan.tensor_view(out_t).view(nb, out_t.C))
        if pipe is not None:
            pipe.submit(logits)                            # copy into a send slot + asynchronous all-gather (RCCL / gloo)
        elif dist is not None:
            if host_gather:                                # gloo: through pinned host memory (ranks sharing a GPU)
                lh = logits.cpu()
                gh = torch.empty(world * batch, out_t.C, dtype=torch.float32)
                dist.all_gather_into_tensor(gh, lh)
                gathered.copy_(gh)
            else:
                dist.all_gather_into_tensor(gathered, logits)  # on the launch stream: the next replay waits for the ring pass

    for _ in range(warmup):
        step()
    if tele is not None:
        tele.start()          # (sampler process: shader clock / socket power) -- started in front of the barrier, so that its
    torch.cuda.synchronize()  # round trip is not idle GPU time between the warm-up and the first timed step
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):    # exactly K steps and nothing else between the two synchronisations
        step()
    if pipe is not None:
        pipe.drain()                                       # the last steps' exchanges are inside the timed region
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    telemetry = tele.stop().summary() if tele is not None else {}
    if pipe is not None:
        gathered = pipe.last()
    # what a caller of the timed path receives from its last step (the passes below write the same buffers again)
    last_logits = logits.clone()
    last_gathered = None if gathered is None else gathered.clone()
    torch.cuda.synchronize()
    # per-step durations for the median: the same K steps once more with an event on the launch stream between them -- a pass
    # of its own (an event record between two graph launches costs a step of ResNet-50 about 50 us: it stays out of `value`)
    median_ms = None
    if full:
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        marks[0].record()
        for i in range(steps):
            step()
            marks[i + 1].record()
        if pipe is not None:
            pipe.drain()
        torch.cuda.synchronize()
        per_step = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
        median_ms = per_step[steps // 2] if steps % 2 else 0.5 * (per_step[steps // 2 - 1] + per_step[steps // 2])
    # the exchange step really delivered this rank's logits (and, world = 1, nothing else): bit for bit
    gather_bit_equal = None
    if dist is not None and full:
        rk = dist.get_rank()
        gather_bit_equal = bool(torch.equal(gathered[rk * batch:(rk + 1) * batch], logits))
    # the other launch mode under the SAME protocol (warm-up, K steps between synchronisations), so that kernel changes stay
    # visible round over round whichever mode wins on a box
    if forked is not None and captured is not None and full:
        for _ in range(warmup):
            captured.replay()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for _ in range(steps):
            captured.replay()
        torch.cuda.synchronize()
        single_ms = (time.perf_counter() - t2) / steps * 1e3
    # a SUSTAINED window of the timed recording (>= 0.6 s of back-to-back replays, no exchange): the timed region of a 3.6-ms
    # step is 70 ms -- a handful of telemetry samples -- and a part that has not reached its steady clock / power state yet
    sustained = None
    best = forked if forked is not None else captured
    if best is not None and full:
        n_s = max(steps, int(0.6 / max(dt / steps, 1e-4)) + 1)
        torch.cuda.synchronize()
        tele.start()
        t3 = time.perf_counter()
        for _ in range(n_s):
            best.replay()
        torch.cuda.synchronize()
        dt3 = time.perf_counter() - t3
        sustained = dict(steps=n_s, ms_per_step=round(dt3 / n_s * 1e3, 4), telemetry=tele.stop().summary())
    # per-kernel durations: the same K steps again, launched eagerly with a HIP event pair (on the launch stream)
    # around every launch of the conv / linear / attention families -- events cannot be read back from a graph replay
    events = [] if kernel_events else None
    eager_dt = None
    if events is not None:
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(steps):
            step(events)
        torch.cuda.synchronize()
        eager_dt = time.perf_counter() - t1
    stats = {}
    if events:
        for kind, flops, e0, e1 in events:
            s_ = stats.setdefault(kind, dict(ms=0.0, n=0, flops=0.0))
            s_["ms"] += e0.elapsed_time(e1)
            s_["n"] += 1
            s_["flops"] += flops
    return dict(seconds=dt, ms_per_step=dt / steps * 1e3, median_ms_per_step=median_ms, gather_bit_equal=gather_bit_equal,
                forked_bit_equal=forked_bit_equal, kernels=stats, logits=last_logits, x=x, prog=prog, telemetry=telemetry,
                sustained=sustained, exchange_mode=(None if dist is None else "synchronous on the launch stream" if pipe is None else
                                                    "asynchronous, double-buffered (dp.PipelinedGather): step i's all-gather under step i + 1"
                                                    + (", ncclAllGather through the C ABI (tfimm_hip_dp_all_gather_logits)" if comm is not None else "")),
                graph=captured is not None, gathered=last_gathered, branches=(n_br if forked is not None else 1),
                hybrid_cut=(hybrid_cut if forked is not None and hybrid_cut is not None and getattr(forked, "cut_op", None) == hybrid_cut else None),
                n_ops=len(prog.ops),
                single_branch_ms=single_ms, forked_ms=forked_ms,
                eager_ms_per_step=None if eager_dt is None else eager_dt / steps * 1e3)


_EVENT_KINDS = {"gemm": "gemm", "stem_pool": "gemm", "conv_chain": "gemm", "mlp_fused": "gemm", "grouped_conv": "gemm", "dwconv": "dwconv",
                "expand_dwconv": "dwconv", "attention": "attention", "talking_heads_attention": "attention"}


def run_with_events(plan, x_dev, events):
    """plan.run with a HIP event pair (torch's current stream == the launch stream) around every launch of a
    conv / linear / attention kernel."""
    import ctypes as C

    import torch
    ffi = plan.ffi
    lib = ffi.lib
    stream_ptr = torch.cuda.current_stream().cuda_stream
    st = C.c_void_p(stream_ptr)
    idx = plan._input_patch[0]
    from tfimm.engine.graph import _hip_memset_async
    B = plan.batch
    by_fn = {id(lib.tfimm_hip_gemm): "gemm", id(lib.tfimm_hip_stem_conv_pool): "stem_pool",
             id(lib.tfimm_hip_conv_chain): "conv_chain", id(lib.tfimm_hip_grouped_conv3x3): "grouped_conv",
             id(lib.tfimm_hip_expand_dwconv): "expand_dwconv", id(lib.tfimm_hip_mlp_fused): "mlp_fused",
             id(lib.tfimm_hip_dwconv): "dwconv", id(lib.tfimm_hip_attention): "attention",
             id(lib.tfimm_hip_talking_heads_attention): "talking_heads_attention"}     # ctypes functions are not hashable
    cache = plan.__dict__.setdefault("_timed_ops", {})
    if not cache:
        for k in set(by_fn.values()):
            cache[k] = [op for op in plan.prog.ops if op.kind == k]
    cursor = {k: 0 for k in cache}
    for i, (fn, args) in enumerate(plan.calls):
        kind = by_fn.get(id(fn)) if not isinstance(fn, str) else None
        if i == idx:
            rc = plan.launch_input(x_dev, st)
        elif fn == "memset":
            rc = _hip_memset_async(args[0], args[1], stream_ptr)
        elif kind is not None:
            a = cache[kind][cursor[kind]].attrs
            cursor[kind] += 1
            if kind in ("gemm", "stem_pool"):
                flops = 2.0 * a["M"] * B * a["N"] * a["K_true"]
            elif kind == "dwconv":
                flops = 2.0 * B * a["OH"] * a["OW"] * a["C"] * a["k"] * a["k"]
            else:
                flops = float(a["flops"]) * B
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args, st)
            e1.record()
            events.append((_EVENT_KINDS[kind], flops, e0, e1))
        else:
            rc = fn(*args, st)
        if rc != 0:
            ffi.check(rc, f"op {i}")


def roofline_of(name, wl, r, steps, batch):
    """The roofline object of one measured workload (None without kernel events)."""
    ks = r["kernels"]
    fam = [ks[k] for k in wl["family"] if k in ks and ks[k]["n"]]
    if not fam:
        return None
    bound = wl["bound"]
    peak, punit = PEAK[bound]
    fam_ms = sum(k["ms"] for k in fam)
    fam_n = sum(k["n"] for k in fam)
    launches_per_step = fam_n / steps
    prog = r["prog"]
    alg = None
    if bound == "mfma":
        achieved = sum(k["flops"] for k in fam) / (fam_ms * 1e-3) / 1e12
    else:
        alg = ALG_BYTES_PER_IMAGE.get(name, 0.0) * batch + prog.weight_bytes()
        achieved = alg * steps / (fam_ms * 1e-3) / 1e9
    traffic, traffic_src = measured_traffic(name, batch)
    eager = r["eager_ms_per_step"]
    second = None
    if wl.get("second_bound") == "mfma":
        tf_s = sum(k["flops"] for k in fam) / (fam_ms * 1e-3) / 1e12
        n_fused = sum(1 for op in prog.ops if op.kind == "mlp_fused")
        n_split = sum(1 for op in prog.ops if op.kind == "gemm" and op.attrs.get("act") == "gelu")
        second = dict(bound="mfma", achieved=round(tf_s, 2), peak=PEAK["mfma"][0], unit=PEAK["mfma"][1],
                      frac=round(tf_s / PEAK["mfma"][0], 4),
                      mlp_blocks_in_one_kernel=f"{n_fused} of {n_fused + n_split}",
                      note="the same family's FLOPs over the same time against the dense bf16 MFMA peak: the bound that "
                           "applies once the MLP (fc1 -> GELU -> fc2) is a single kernel (SURVEY.md 8d); today only the "
                           "128-channel stage runs it as one launch (mlp_blocks_in_one_kernel), the others write and re-read "
                           "the hidden tensor, so the HBM bound above is the one that applies to them.  Wider fused MLPs were "
                           "priced on the measured op times and rejected (profiles/NOTES_r04.md 8: C = 256 would gain 8 us per "
                           "block, C = 512 is compute-bound as two launches)")
    return dict(bound=bound, achieved=round(achieved, 2), peak=peak, unit=punit, frac=round(achieved / peak, 4),
                second_bound=second,
                traffic=traffic, traffic_unit="HBM bytes per launch (PMC)", traffic_source=traffic_src,
                traffic_measured_in_run=False,
                algorithmic_bytes_per_launch=None if alg is None else round(alg / launches_per_step),
                algorithmic_bytes_per_step=None if alg is None else round(alg),
                kernel=" + ".join(FAMILY_KERNELS[k] for k in wl["family"]),
                launches_per_step=launches_per_step, avg_launch_ms=round(fam_ms / fam_n, 5),
                family_ms_per_step=round(fam_ms / steps, 4),
                share_of_eager_step=None if not eager else round(fam_ms / steps / eager, 3),
                launches_measured=("one branch, full batch, launched one by one with a HIP event pair on the launch stream: the "
                                   "kernels by themselves" + ("; the timed region ran the batch as parallel branches, where "
                                   "launches overlap and a per-launch duration is not defined" if r.get("branches", 1) > 1 else "")),
                per_kind={k: dict(ms_per_step=round(v["ms"] / steps, 4), launches_per_step=v["n"] / steps,
                                  tflops=round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1)) for k, v in ks.items()},
                timing="HIP event pair around every launch of the family, on the launch stream, over K eagerly launched "
                       "steps run right after the timed region (which replays a hipGraph of the same launches); "
                       "share_of_eager_step compares with the wall time of those eager steps")


def energy_of(name, flops_img, batch, weight_bytes, sustained):
    """Joules per step against the floor the part's energy coefficients set (None without telemetry or byte count)."""
    tl = (sustained or {}).get("telemetry") or {}
    pw = tl.get("energy_power_w") or tl.get("power_w_mean")
    cap = tl.get("power_cap_w")
    alg = ALG_BYTES_PER_IMAGE.get(name)
    if not pw or not cap or not alg:
        return None
    ms = sustained["ms_per_step"]
    flops, byts = flops_img * batch, alg * batch + weight_bytes
    floor_j = flops * E_MFMA_PJ_PER_FLOP * 1e-12 + byts * E_HBM_NJ_PER_BYTE * 1e-9
    dyn_j = (pw - P_IDLE_W) * ms * 1e-3
    floor_ms = floor_j / (cap - P_IDLE_W) * 1e3
    return dict(joules_per_step=round(pw * ms * 1e-3, 3), joules_per_image=round(pw * ms * 1e-3 / batch, 5),
                dynamic_joules_per_step=round(dyn_j, 3), floor_dynamic_joules=round(floor_j, 3), frac=round(floor_j / dyn_j, 4),
                floor_ms_per_step_at_the_cap=round(floor_ms, 3), floor_images_per_sec_at_the_cap=round(batch / floor_ms * 1e3, 1),
                power_w=pw, power_cap_w=cap, share_of_cap=round(pw / cap, 3),
                model=f"floor = matmul flops x {E_MFMA_PJ_PER_FLOP} pJ + algorithmic bytes x {E_HBM_NJ_PER_BYTE} nJ (single-resource probes of "
                      f"profiles/r05_power.md; VALU work -- depthwise multiply-adds, activations, softmax -- not counted, so it is a "
                      f"lower bound); dynamic = above the {P_IDLE_W:.0f}-W idle floor; measured over the sustained window of the timed recording")


def usable_cores():
    """CPU threads this process may really use: affinity mask capped by the cgroup quota
    (a GPU box reports 256 logical CPUs but the container gets far fewer)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:  # noqa: BLE001
        pass
    return max(1, min(n, 64))


def cpu_baseline(model, name, target_seconds=20.0, parity_images=1024):
    """fp32 CPU oracle on a bounded sample of the same workload (non-target number), and its logits on
    ``parity_images`` distinct synthetic images (every timed forward runs a fresh batch) for the top-1 statement."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import oracle
    cores = usable_cores()
    torch.set_num_threads(cores)
    cfg = model.cfg
    b = 8 if cfg.input_size[0] <= 256 else 4
    rng = np.random.default_rng(2021)
    mean = np.asarray(cfg.mean, np.float32)
    std = np.asarray([s if s else 1.0 for s in cfg.std], np.float32)

    def batch_():
        return ((rng.random((b, *cfg.input_size, cfg.in_channels), dtype=np.float32) - mean) / std).astype(np.float32)

    w = model.weights
    poolable = type(model).__name__ in ("ResNet", "EfficientNet", "ViT", "SwinTransformer", "CaiT")   # classifier input = pooled "features"

    def fwd(x):
        """logits (+ the classifier's input: the pooled "features" entry of the reference's feature dictionary)"""
        if not poolable:
            return oracle.forward(cfg, w, x), None
        y, feats = oracle.forward(cfg, w, x, return_features=True)
        f = np.asarray(feats["features"], dtype=np.float32)
        return y, (f if f.ndim == 2 else f.reshape(f.shape[0], -1, f.shape[-1]).mean(1))

    xs, ys, fs = [batch_()], [], []
    t0 = time.perf_counter()
    y0, f0 = fwd(xs[0])                                # warm-up, also the first parity batch
    ys.append(y0)
    fs.append(f0)
    first = time.perf_counter() - t0
    need = -(-parity_images // b) - 1                 # forwards that fill the parity sample ...
    n = max(7, min(need, int(target_seconds / max(first, 1e-3)) - 1))      # ... bounded by the time budget (>= 64 images)
    dt = 0.0
    for _ in range(n):
        x = batch_()
        t0 = time.perf_counter()
        y, f = fwd(x)
        dt += time.perf_counter() - t0
        if len(xs) * b < parity_images:
            xs.append(x)
            ys.append(y)
            fs.append(f)
    feats = None if (not poolable or any(f is None for f in fs)) else np.concatenate(fs)
    return (dict(value=round(b * n / dt, 2), unit="images/sec", cores=cores, kind="port",
                 sample=f"{n} forwards of batch {b}, {name}, fp32 torch-CPU oracle"),
            np.concatenate(xs), np.concatenate(ys), feats)


def calibrated_head(model, feats, nb_classes):
    """A classifier head with NON-TRIVIAL MARGINS for the parity images.  With random-init weights on
    uniform-noise images the 1000 logits of every image are nearly the same near-Gaussian vector, so "top-1 match" with the
    random head says little.  Here the first n_anchor = min(images, classes, feature width / 2) parity images become the
    prototypes of classes 0 .. n_anchor-1: W^T (f_i - mean f) ~ e_i by ridge regression on the ORACLE's classifier-input
    features (lambda = 1e-3 of the mean eigenvalue), remaining classes get zero weights and bias -1.  Returns
    (kernel [D][classes], bias [classes], n_anchor) or None when the model's classifier does not read the pooled features."""
    import numpy as np
    if feats is None or not hasattr(model.cfg, "classifier") or isinstance(model.cfg.classifier, (list, tuple)):
        return None
    w = model.weights
    kname = next((k for k in w if k.endswith(f"{model.cfg.classifier}/kernel")), None)
    if kname is None or w[kname].ndim != 2 or w[kname].shape[0] != feats.shape[1]:
        return None
    d = feats.shape[1]
    n = int(min(feats.shape[0], nb_classes, d // 2))
    f64 = feats.astype(np.float64)
    fbar = f64.mean(0)
    fc = f64[:n] - fbar
    g = fc @ fc.T
    wt = np.linalg.solve(g + 1e-3 * np.trace(g) / n * np.eye(n), fc)       # [n][D]: row i = the weights of class i
    kernel = np.zeros((d, nb_classes), np.float32)
    kernel[:, :n] = wt.T
    bias = np.full(nb_classes, -1.0, np.float32)
    bias[:n] = -(wt @ fbar)
    return kname, kernel, bias, n


def parity_statement(model, xs, ys, feats=None):
    """Engine vs oracle on the parity images (every forward the CPU baseline timed, up to 1024 distinct synthetic images):
    * the bf16 product path: rel-to-max error, top-1 match, and the match restricted to images whose ORACLE top-1 / top-2
      margin is at least 10x that image's own error (where an argmax is decided by the kernels rather than by rounding);
    * the float32 verification path (tfimm/engine/precision.py, csrc/ref32.hip) on the same images: the same lowering with
      float32 storage must agree with the float32 oracle at the reference's 1e-3 bar and reproduce its top-1."""
    import numpy as np
    import torch
    from tfimm.engine import precision

    def run(x):
        out = []
        for s in range(0, x.shape[0], 32):
            out.append(model(torch.from_numpy(x[s:s + 32])).numpy())
        return np.concatenate(out).reshape(ys.shape)

    def stats(got):
        flat_y, flat_g = ys.reshape(-1, ys.shape[-1]), got.reshape(-1, ys.shape[-1])
        err = np.abs(flat_g - flat_y).max(-1)                       # per image, absolute
        top = np.sort(flat_y, -1)
        margin = top[:, -1] - top[:, -2]
        miss = flat_g.argmax(-1) != flat_y.argmax(-1)
        clear = margin >= 10 * err
        return flat_y, err, margin, miss, clear

    got = run(xs)
    flat_y, err, margin, miss, clear = stats(got)
    out = dict(images=int(flat_y.shape[0]), top1_match=float(1.0 - miss.mean()), mismatches=int(miss.sum()),
               images_with_margin_ge_10x_own_err=int(clear.sum()),
               top1_match_where_margin_ge_10x_own_err=(float(1.0 - miss[clear].mean()) if clear.any() else None),
               mismatches_with_oracle_margin_below_2x_own_err=int((miss & (margin < 2 * err)).sum()),
               rel_to_max_err=float(np.abs(got - ys).max() / (np.abs(ys).max() + 1e-6)),
               max_abs_err=float(err.max()), median_oracle_top1_top2_margin=float(np.median(margin)),
               max_abs_logit=float(np.abs(ys).max()),
               note="random-init weights on uniform-noise images: all images produce nearly the same 1000 near-Gaussian logits, "
                    "whose top-1 / top-2 gap is a few percent of the logit range -- a bf16 forward flips an argmax whenever that gap "
                    "is inside its error band; the float32 path below shows the flips are rounding, not arithmetic")
    try:
        with precision.use("fp32"):
            got32 = run(xs)
        _, err32, _, miss32, _ = stats(got32)
        out["fp32_path"] = dict(images=int(flat_y.shape[0]), rel_to_max_err=float(np.abs(got32 - ys).max() / (np.abs(ys).max() + 1e-6)),
                                top1_match=float(1.0 - miss32.mean()), max_abs_err=float(err32.max()),
                                what="same layer program, float32 storage and kernels (TFIMM_PRECISION=fp32), vs the same oracle logits; "
                                     "the reference's own bar is 1e-3 (tests/test_timm.py:71)")
    except Exception as e:  # noqa: BLE001
        out["fp32_path"] = {"error": f"{type(e).__name__}: {e}"}
    # the same images through a head with real margins: each anchor image is its own class
    try:
        cal = calibrated_head(model, feats, ys.shape[-1])
        if cal is not None:
            kname, kernel, bias, n_anchor = cal
            bname = kname[:-len("kernel")] + "bias"
            orig = {kname: model.weights[kname].copy(), bname: model.weights[bname].copy()}
            ref = feats.astype(np.float32) @ kernel + bias                    # the oracle's logits with that head (Dense: x @ W + b)
            model.set_weights({kname: kernel, bname: bias}, strict=False)
            try:
                got_c = run(xs).reshape(ref.shape)
            finally:
                model.set_weights(orig, strict=False)
            a = slice(0, n_anchor)                                            # anchors: own class by construction
            err_c = np.abs(got_c - ref).max(-1)
            top = np.sort(ref, -1)
            margin_c = top[:, -1] - top[:, -2]
            miss_c = got_c.argmax(-1) != ref.argmax(-1)
            out["calibrated_head"] = dict(
                images=int(ref.shape[0]), anchors=int(n_anchor),
                oracle_top1_is_own_class=float((ref[a].argmax(-1) == np.arange(n_anchor)).mean()),
                top1_match=float(1.0 - miss_c.mean()), top1_match_anchors=float(1.0 - miss_c[a].mean()),
                median_margin_over_own_err_anchors=float(np.median(margin_c[a] / np.maximum(err_c[a], 1e-30))),
                min_margin_over_own_err_anchors=float((margin_c[a] / np.maximum(err_c[a], 1e-30)).min()),
                rel_to_max_err=float(np.abs(got_c - ref).max() / (np.abs(ref).max() + 1e-6)),
                what="classifier replaced by a ridge-regression prototype head fitted on the oracle's pooled features (anchor image i "
                     "= class i), same backbone weights, same images: the engine must single out every image among the anchors")
    except Exception as e:  # noqa: BLE001
        out["calibrated_head"] = {"error": f"{type(e).__name__}: {e}"}
    return out


def parity_summary(results):
    """Top level of the bench line: what "top-1 match" means here and the three figures per model that carry it
    (BASELINE.md 3.4 asks for >= 99 %; that statement holds for the float32 path and the calibrated head, NOT for the bf16
    path on the random-init head, whose near-degenerate logits flip inside the bf16 error band)."""
    models = {}
    for name, r in results:
        pv = (r or {}).get("parity_vs_oracle")
        if not pv:
            continue
        cal, f32 = pv.get("calibrated_head") or {}, pv.get("fp32_path") or {}
        models[name] = dict(images=pv.get("images"),
                            bf16_rel_to_max_err=pv.get("rel_to_max_err"),
                            bf16_top1_match_random_head=pv.get("top1_match"),
                            bf16_top1_match_where_margin_ge_10x_own_err=pv.get("top1_match_where_margin_ge_10x_own_err"),
                            bf16_top1_match_calibrated_head=cal.get("top1_match"),
                            bf16_top1_match_calibrated_head_anchors=cal.get("top1_match_anchors"),
                            fp32_path_top1_match=f32.get("top1_match"), fp32_path_rel_to_max_err=f32.get("rel_to_max_err"))
    if not models:
        return None
    return dict(oracle="fp32 torch-CPU restatement of the reference's forward (oracle/), pinned to the reference's own model code "
                       "(tests/test_golden.py); identical synthetic weights and images on both sides",
                bars="logits rel-to-max <= 5e-2 (bf16 path), <= 1e-3 (float32 path: the reference's own bar, tests/test_timm.py:71)",
                ge_99_percent_top1_holds_for="fp32_path_top1_match and bf16_top1_match_calibrated_head (a head with real margins: "
                                             "anchor image i = class i); the random-init head's figure is reported as measured",
                models=models)


def run_workload(name, args, world, rank, dist, steps, warmup, batch=0, micro_batch=0, with_cpu=False, with_parity=False,
                 cpu_seconds=20.0, parity_images=1024):
    import torch
    wl = WORKLOADS[name]
    batch = batch or wl["batch"]
    model = build_model(wl["model"])
    torch.cuda.empty_cache()
    r = measure(model, batch, micro_batch, steps, warmup, world, args.full and not args.no_kernel_events, dist, graph=not args.no_graph,
                branches=args.branches, full=args.full)
    ms = r["ms_per_step"]
    per_rank = [ms]
    if dist is not None:
        dev = "cpu" if dist.get_backend() == "gloo" else "cuda"
        t = torch.tensor([ms], device=dev)
        allms = torch.empty(world, device=dev)
        dist.all_gather_into_tensor(allms, t)
        per_rank = [round(float(v), 4) for v in allms.tolist()]
        ms = max(per_rank)                                   # max over ranks
    out = None
    if rank == 0:
        prog = r["prog"]
        flops_img = prog.flops_per_image()
        total = batch * world
        rl = roofline_of(name, wl, r, steps, batch)
        if rl is not None and rl.get("algorithmic_bytes_per_step"):
            # the timed region's own figure: algorithmic bytes of a step over ms_per_step (parallel branches included) --
            # `frac` is the kernels by themselves (one branch, launch by launch)
            rl["frac_timed_mode"] = round(rl["algorithmic_bytes_per_step"] / (ms * 1e-3) / 1e9 / rl["peak"], 4)
        out = dict(value=round(total / ms * 1e3, 1), unit="images/sec", ms_per_step=round(ms, 4),
                   median_ms_per_step=_r(r["median_ms_per_step"], 4), gather_bit_equal=r["gather_bit_equal"],
                   forked_bit_equal_to_single=r["forked_bit_equal"], per_gpu_batch=batch,
                   global_batch=total, per_rank_ms=per_rank, model=wl["model"], input_size=int(model.cfg.input_size[0]),
                   launch=("eager" if not r["graph"] else "hipGraph replay" if r["branches"] == 1 else
                           f"hipGraph replay, {r['branches']} parallel branches of " +
                           (f"{batch // r['branches']}" if batch % r['branches'] == 0 else
                            f"{batch // r['branches']}-{-(-batch // r['branches'])}") + " images" +
                           (f" for ops 0..{r['hybrid_cut'] - 1} of {r['n_ops']}, the full batch for the rest" if r["hybrid_cut"] else "")),
                   branches=r["branches"],
                   single_branch_ms_per_step=None if r["single_branch_ms"] is None else round(r["single_branch_ms"], 4),
                   forked_ms_per_step=None if r["forked_ms"] is None else round(r["forked_ms"], 4),
                   gflops_per_image=round(flops_img / 1e9, 3),
                   model_tflops=round(flops_img * total / ms / 1e9, 1),
                   mfma_frac_whole_step=round(flops_img * batch / ms / 1e9 / 2500.0, 4),
                   # clock / power state of THIS box over the timed region (side-thread samples; energy_power_w = the firmware's
                   # energy accumulator over the same window) and over a sustained window of the same recording
                   # (power: from the firmware's energy counter over the window when it is there -- the sampled socket power is a
                   #  filtered value that lags by ~100 ms, far too slow for a 70-ms region; the samples stay in `telemetry`)
                   sclk_mhz_mean=r["telemetry"].get("sclk_mhz_mean"),
                   power_w_mean=r["telemetry"].get("energy_power_w") or r["telemetry"].get("power_w_mean"),
                   power_cap_w=r["telemetry"].get("power_cap_w"), telemetry=r["telemetry"], sustained=r["sustained"],
                   exchange_mode=r["exchange_mode"],
                   roofline=rl, outputs=dict(logits=r["logits"], gathered_logits=r["gathered"]))
        out["energy"] = energy_of(name, flops_img, batch, prog.weight_bytes(), r["sustained"])
        if with_cpu:
            cpu, xs, ys, fs = cpu_baseline(model, wl["model"], target_seconds=cpu_seconds, parity_images=parity_images)
            out["cpu_baseline"] = cpu
            out["parity_vs_oracle"] = parity_statement(model, xs, ys, fs)
        elif with_parity:
            # N > 1: the CPU baseline is an N = 1 figure, but rank 0 still states parity of what it just ran
            _, xs, ys, fs = cpu_baseline(model, wl["model"], target_seconds=1.0)
            out["parity_vs_oracle"] = parity_statement(model, xs, ys, fs)
    del r, model
    torch.cuda.empty_cache()
    return out


def detail_record(args, m, also, world, distributed, launched):
    """Everything the run measured (the round-5 line): goes to the detail file and stderr, never to stdout."""
    return {
        "metric": "images/sec (fwd, bf16)", "value": m["value"], "unit": "images/sec", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": m["ms_per_step"],
        "median_ms_per_step": m["median_ms_per_step"], "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic", "protocol_version": PROTOCOL_VERSION,
        "config": {"workload": f"{m['model']} @{m['input_size']} fwd", "per_gpu_batch": m["per_gpu_batch"],
                   "global_batch": m["global_batch"], "micro_batch": args.micro_batch or m["per_gpu_batch"],
                   "parallelism": f"dp{world}", "exchange": ("none" if not distributed else "RCCL all-gather of fp32 logits" if args.backend == "nccl"
                                else "gloo all-gather of fp32 logits (host)"),
                   "exchange_mode": m.get("exchange_mode"),
                   "ranks": world, "launcher": ("bench.py spawn" if os.environ.get("TFIMM_BENCH_SPAWNED") else
                                                "external" if launched else "in-process"),
                   "weights": "random-init (synthetic generator, seed 2021)", "launch": m["launch"],
                   "branches": m["branches"], "single_branch_ms_per_step": m["single_branch_ms_per_step"],
                   "forked_ms_per_step": m["forked_ms_per_step"], "gflops_per_image": m["gflops_per_image"],
                   "forked_bit_equal_to_single": m["forked_bit_equal_to_single"],
                   "gathered_logits_bit_equal_to_local": m["gather_bit_equal"]},
        "per_rank_ms": m["per_rank_ms"], "model_tflops": m["model_tflops"],
        "roofline": m["roofline"], "cpu_baseline": m.get("cpu_baseline"), "parity_vs_oracle": m.get("parity_vs_oracle"),
        "parity": parity_summary([(args.workload, m)] + list(also.items())),
        "sclk_mhz_mean": m.get("sclk_mhz_mean"), "power_w_mean": m.get("power_w_mean"), "power_cap_w": m.get("power_cap_w"),
        "telemetry": m.get("telemetry"), "sustained": m.get("sustained"), "energy": m.get("energy"),
        "headline": {k: (v["value"] if v and "value" in v else None)
                     for k, v in [(args.workload, m)] + list(also.items())},
        "also": also,
    }


_ROOFLINE_KEYS = ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_step",
                  "algorithmic_bytes_per_launch", "kernel", "launches_per_step", "avg_launch_ms", "frac_timed_mode")


def _short(s, n):
    return s if s is None or len(s) <= n else s[:n - 1] + "~"


def _compact_roofline(rl):
    if not rl:
        return None
    out = {k: rl.get(k) for k in _ROOFLINE_KEYS if k in rl}
    out["kernel"] = _short(out.get("kernel"), 96)
    return out


def compact_line(d):
    """The ONE stdout line: the contract's fields + roofline + cpu_baseline + one parity figure per model + the four headline
    numbers, always below LINE_LIMIT bytes -- the optional groups are dropped last-first if a run ever grows past it."""
    cfg = d["config"]
    line = {k: d[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "median_ms_per_step",
                              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "protocol_version")}
    line["config"] = {k: cfg[k] for k in ("workload", "per_gpu_batch", "global_batch", "parallelism", "exchange", "ranks",
                                          "launcher", "launch", "branches", "gathered_logits_bit_equal_to_local")}
    line["config"]["launch"] = _short(cfg["launch"], 120)
    line["per_rank_ms"] = [round(float(v), 4) for v in d["per_rank_ms"]]
    line["roofline"] = _compact_roofline(d.get("roofline"))
    cb = d.get("cpu_baseline")
    line["cpu_baseline"] = None if not cb else dict(value=cb["value"], unit=cb["unit"], cores=cb["cores"], kind=cb["kind"],
                                                    sample=_short(cb.get("sample"), 72))
    par = (d.get("parity") or {}).get("models") or {}
    line["parity"] = {name: dict(images=p.get("images"), rel_to_max=_r(p.get("bf16_rel_to_max_err"), 5),
                                 top1=_r(p.get("bf16_top1_match_random_head"), 4),
                                 top1_calibrated_head=_r(p.get("bf16_top1_match_calibrated_head"), 4),
                                 top1_fp32_path=_r(p.get("fp32_path_top1_match"), 4),
                                 rel_to_max_fp32_path=_r(p.get("fp32_path_rel_to_max_err"), 8))
                      for name, p in par.items()} or None
    line["headline"] = d["headline"]
    line["clock_power"] = dict(sclk_mhz_mean=d.get("sclk_mhz_mean"), power_w_mean=d.get("power_w_mean"), power_cap_w=d.get("power_cap_w"))
    # the other BASELINE configurations: value / time / roofline fraction each (their full objects are in the detail file)
    line["also"] = {}
    for name, v in (d.get("also") or {}).items():
        if not v or "value" not in v:
            line["also"][name] = {"error": _short((v or {}).get("error", "no result"), 80)}
            continue
        rl = v.get("roofline") or {}
        line["also"][name] = dict(value=v["value"], ms_per_step=v["ms_per_step"], per_gpu_batch=v["per_gpu_batch"], branches=v.get("branches"),
                                  bound=rl.get("bound"), frac=rl.get("frac"), achieved=rl.get("achieved"), unit=rl.get("unit"))
    line["detail"] = "bench_detail.json (+ stderr)"
    for drop in (None, "clock_power", "also", "parity"):
        if drop is not None:
            line.pop(drop, None)
        text = json.dumps(line, separators=(",", ":"))
        if len(text) < LINE_LIMIT:
            return text
    raise RuntimeError(f"bench line is {len(text)} bytes even without its optional groups (limit {LINE_LIMIT})")


def _r(v, n):
    return None if v is None else round(float(v), n)


def write_detail(detail):
    """The full record: bench_detail.json next to bench.py (or $TFIMM_BENCH_DETAIL) and, as one line, on stderr."""
    text = json.dumps(detail)
    print("bench detail: " + text, file=sys.stderr)
    path = os.environ.get("TFIMM_BENCH_DETAIL") or os.path.join(ROOT, "bench_detail.json")
    try:
        with open(path, "w") as f:
            f.write(text + "\n")
    except OSError as e:
        print(f"warning: could not write {path}: {e}", file=sys.stderr)


def dump_outputs(directory, outputs):
    """What the timed path handed its caller in the last timed step, as float32 .npy files (logits: batch x classes, 1 MB for
    ResNet-50 at 256; the gathered logits of all ranks when N > 1)."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    for name, t in outputs.items():
        if t is not None:
            np.save(os.path.join(directory, f"{name}.npy"), t.detach().float().cpu().numpy().astype(np.float32))


def main():
    args = parse()
    launched = "WORLD_SIZE" in os.environ
    if not launched and (args.gpus > 1 or args.spawn):
        sys.exit(spawn_ranks(args.gpus))
    # ONE JSON line on stdout, nothing else: RCCL prints a version banner to fd 1 when its first communicator comes up (and
    # other libraries may follow), so fd 1 points at stderr while the work runs and the line goes to the saved descriptor
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if launched:
        # under a launcher (the driver's torchrun, or spawn_ranks above): one process per GPU, RCCL over xGMI
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            torch.cuda.set_device(local_rank % torch.cuda.device_count())   # ranks may share a GPU
            dist.init_process_group("gloo", rank=rank, world_size=world)
    else:
        torch.cuda.set_device(0)
    if args.gpus != world and rank == 0:
        print(f"warning: --gpus {args.gpus} but WORLD_SIZE={world}; reporting n_gpus={world}", file=sys.stderr)

    cpu = args.full and not args.no_cpu_baseline
    main_r = run_workload(args.workload, args, world, rank, dist, args.steps, args.warmup, batch=args.batch,
                          micro_batch=args.micro_batch, with_cpu=(world == 1 and cpu), with_parity=(world > 1 and cpu))
    if rank == 0:
        outputs = main_r.pop("outputs")
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, outputs)
        del outputs
    # N > 1: ViT-B/16 (the other half of the headline metric) and EfficientNet-B4 -- BASELINE.json configs[4] is B4 at
    # 256 per GPU x 8 GPUs = 2048 global, so `bench.py --gpus 8 --full` measures it; a plain run measures the main workload only
    extra = args.extra if args.extra is not None else (
        "" if not args.full else DEFAULT_EXTRA if world == 1 else "vit_base_patch16_224,efficientnet_b4")
    also = {}
    for name in [n for n in extra.split(",") if n and n != args.workload]:
        try:
            if name not in WORKLOADS:
                raise KeyError(f"unknown workload {name}")
            # the metric names ViT-B/16 next to ResNet-50: it gets the full protocol (K steps, W warm-ups) and, on one GPU, its own
            # CPU baseline and parity statement (bounded: ~6 s of CPU, >= 64 images); the other configurations half the steps
            vit = name == "vit_base_patch16_224"
            # (every BASELINE configuration carries parity next to its throughput: 128 images each on one GPU)
            also[name] = run_workload(name, args, world, rank, dist, args.steps if vit else max(3, args.steps // 2),
                                      args.warmup if vit else max(2, args.warmup // 2),
                                      with_cpu=(world == 1 and cpu), cpu_seconds=6.0, parity_images=128)
            if also[name] is not None:
                also[name].pop("outputs", None)
        except Exception as e:  # noqa: BLE001
            if dist is not None:
                raise                     # a rank that skips a collective would hang the others
            also[name] = {"error": f"{type(e).__name__}: {e}"}
    if rank == 0:
        detail = detail_record(args, main_r, also, world, dist is not None, launched)
        line = compact_line(detail)
        write_detail(detail)
        sys.stdout.flush()
        os.write(saved_stdout, (line + "\n").encode())
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

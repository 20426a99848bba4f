"""bf16 vs fp8 (MXFP8 Dense layers, tfimm/engine/precision.py) of one model in ONE process:

    python tools/fp8_ab.py MODEL BATCH [rounds]

Captured graphs of the same seeded model and input under both precisions, replayed alternately (rounds x 20 replays each,
so that clock / power drift hits both arms alike).  Prints ms/step and img/s of each arm, the fp8 / bf16 speed ratio, the
shader clock and socket power over the timed region (tools/telemetry.py) and the fp8-vs-bf16 logits deviation
(rel-to-max).  Not a bench.py line: bench.py measures the default precision only."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tensorflow-image-models_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tfimm  # noqa: E402
from tfimm.engine import precision  # noqa: E402
from tfimm.utils.init import synthetic_weights  # noqa: E402


def main():
    name, batch = sys.argv[1], int(sys.argv[2])
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    reps = 20
    m = tfimm.create_model(name)
    m.set_weights(synthetic_weights(m, 2021))
    g = torch.Generator().manual_seed(2021)
    x = torch.randn(batch, *m.cfg.input_size, m.cfg.in_channels, generator=g).to("cuda", torch.bfloat16)
    arms = {}
    for prec in ("bf16", "fp8"):
        with precision.use(prec):
            prog = m.program()
            plan = prog.make_plan(batch)
            plan.run(x)
            cap = plan.capture(x)
            cap.replay()
            torch.cuda.synchronize()
            logits = plan.tensor_view(prog.outputs["logits"]).float().cpu().numpy().copy()
            arms[prec] = dict(cap=cap, plan=plan, logits=logits, times=[], ops=len(prog.ops),
                              mx=sum(o.kind == "gemm_mx" for o in prog.ops))
    for a in arms.values():
        for _ in range(5):
            a["cap"].replay()
    torch.cuda.synchronize()
    tele = None
    try:
        from telemetry import Telemetry
        tele = Telemetry(device_index=0)
        tele.__enter__()
    except Exception as e:  # noqa: BLE001  (telemetry is optional: a box without a source still measures)
        print("telemetry unavailable:", e)
        tele = None
    for _ in range(rounds):
        for prec, a in arms.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                a["cap"].replay()
            torch.cuda.synchronize()
            a["times"].append((time.perf_counter() - t) / reps * 1e3)
    summ = {}
    if tele is not None:
        tele.__exit__(None, None, None)
        summ = tele.summary()
    print(f"{name} batch {batch}: {rounds} rounds x {reps} replays per arm, alternating")
    for prec, a in arms.items():
        ms = float(np.median(a["times"]))
        a["ms"] = ms
        print(f"  {prec:5s} {ms:8.3f} ms/step  {batch / ms * 1e3:9.1f} img/s  (min {min(a['times']):.3f}, max "
              f"{max(a['times']):.3f}; {a['ops']} ops, {a['mx']} gemm_mx)")
    print(f"  fp8 / bf16 img/s: {arms['bf16']['ms'] / arms['fp8']['ms']:.3f}x")
    l8, l16 = arms["fp8"]["logits"], arms["bf16"]["logits"]
    dev = float(np.abs(l8 - l16).max() / (np.abs(l16).max() + 1e-6))
    agree = float((l8.argmax(-1) == l16.argmax(-1)).mean())
    print(f"  fp8 vs bf16 logits: rel-to-max {dev:.4e}, top-1 agreement {agree:.4f}")
    if summ:
        print("  telemetry: " + ", ".join(f"{k} {summ.get(k)}" for k in
                                          ("sclk_mhz_mean", "sclk_mhz_min", "power_w_mean", "power_w_max", "power_cap_w",
                                           "source")))


if __name__ == "__main__":
    main()

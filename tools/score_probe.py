"""What the scoring end costs, in ONE process:

    python tools/score_probe.py [--rounds R] [--out FILE] [--skip-models]

(1) tfimm_hip_score alone at (B, N) = (256, 1000) and (512, 21843), without the meter buffers and with all three of them
(state, per_class, confusion -- the last only where N <= TFIMM_SCORE_MAX_CONFUSION_N): a captured graph of LAUNCHES launches per
arm, the graphs replayed alternately (R rounds after a warm-up, HIP events around each replay), microseconds per launch against
the one-read floor B * N * 4 bytes / 8 TB/s.
(2) resnet50 at batch 256: ``model.evaluate(x, labels, meter)`` against ``model(x)`` followed by
``torch.nn.functional.cross_entropy(reduction="none")`` + ``torch.topk(logits, 5)``, both as a caller would run them (the model's
recording, then eager launches), alternately, HIP events around each call, ms per call; and the model's recording alone.
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

SHAPES = [(256, 1000), (512, 21843)]
MODELS = [("resnet50", 256)]
LAUNCHES = 20          # launches per recorded graph of part (1)
HBM_BYTES_PER_S = 8e12
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
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


def op_level(rounds):
    say(f"tfimm_hip_score alone: graphs of {LAUNCHES} launches, replayed alternately, {rounds} rounds after 3 warm-up rounds")
    g = torch.Generator().manual_seed(2021)
    arms = []
    for B, N in SHAPES:
        x = (torch.randn(B, N, generator=g) * 3).to("cuda")
        labels = torch.randint(0, N, (B,), generator=g, dtype=torch.int32).to("cuda")
        want_loss = torch.nn.functional.cross_entropy(x, labels.long(), reduction="none")
        for with_meter in (False, True):
            outs = [torch.empty(B, dtype=dt, device="cuda") for dt in (torch.float32, torch.int32, torch.int32, torch.float32)]
            acc = [None, None, None]
            if with_meter:
                acc = [torch.zeros(ffi.SCORE_STATE_WORDS, dtype=torch.int64, device="cuda"),
                       torch.zeros(2 * N, dtype=torch.int64, device="cuda"),
                       torch.zeros(N * N, dtype=torch.int32, device="cuda") if N <= ffi.SCORE_MAX_CONFUSION_N else None]

            def launch(x=x, B=B, N=N, labels=labels, outs=outs, acc=acc):
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                ffi.check(ffi.lib.tfimm_hip_score(x.data_ptr(), N, B, N, labels.data_ptr(), *(t.data_ptr() for t in outs),
                                                  *(None if t is None else t.data_ptr() for t in acc), st), "tfimm_hip_score")
            launch()                      # function attributes are set outside the recording
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                for _ in range(LAUNCHES):
                    launch()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(outs[2].long(), x.argmax(1)), "the probe's launch disagrees with torch.argmax on tie-free rows"
            assert torch.allclose(outs[0], want_loss, rtol=1e-4, atol=1e-4), "the probe's launch disagrees with torch's cross-entropy"
            what = "no meter" if not with_meter else "state + per_class" + (" + confusion" if acc[2] is not None else "")
            arms.append(dict(shape=(B, N), what=what, graph=graph, times=[], keep=(x, labels, outs, acc)))
    for _ in range(3):
        for a in arms:
            timed(a["graph"].replay)
    t = telemetry()
    for _ in range(rounds):
        for a in arms:
            a["times"].append(timed(a["graph"].replay) / LAUNCHES * 1e3)
    for a in arms:
        B, N = a["shape"]
        us = float(np.median(a["times"]))
        floor = B * N * 4 / HBM_BYTES_PER_S * 1e6
        say(f"  B={B:4d} N={N:6d} {a['what']:30s}: {us:8.2f} us/launch (min {min(a['times']):.2f}, max {max(a['times']):.2f}); "
            f"one-read floor {floor:6.2f} us; {us / floor:6.1f} x floor; {B * N * 4 / us / 1e6:7.3f} TB/s of logits")
    telemetry_line(t)


def model_level(name, batch, rounds):
    m = tfimm.create_model(name)
    m.set_weights(synthetic_weights(m, 2021))
    g = torch.Generator().manual_seed(2021)
    x = torch.randn(batch, *m.cfg.input_size, m.cfg.in_channels, generator=g).to("cuda", torch.bfloat16)
    labels = torch.randint(0, m.cfg.nb_classes, (batch,), generator=g).to("cuda")
    meter = tfimm.Meter(m.cfg.nb_classes)
    keep = {}

    def plain():
        keep["plain"] = m(x)

    def evaluate():
        keep["evaluate"] = m.evaluate(x, labels, meter)

    def torch_way():
        logits = m(x).torch()
        keep["torch"] = (torch.nn.functional.cross_entropy(logits, labels, reduction="none"), torch.topk(logits, 5, dim=1))
    arms = {"model(x)": plain, "model.evaluate(x, labels, meter)": evaluate, "model(x) + torch cross_entropy + topk(5)": torch_way}
    for _ in range(5):                    # the first call is eager, the second records
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ours, theirs = keep["evaluate"], keep["torch"]
    assert torch.allclose(ours.loss.torch(), theirs[0], rtol=1e-4, atol=1e-4), "evaluate disagrees with torch's cross-entropy"
    times = {arm: [] for arm in arms}
    t = telemetry()
    for _ in range(rounds):
        for arm, fn in arms.items():
            times[arm].append(timed(fn))
    say(f"{name} batch {batch} ({m.cfg.nb_classes} classes): {rounds} calls per arm, alternating, HIP events around each call")
    ms = {}
    for arm in arms:
        ms[arm] = float(np.median(times[arm]))
        say(f"  {arm:42s} {ms[arm]:9.4f} ms/call (min {min(times[arm]):.4f}, max {max(times[arm]):.4f})")
    base = ms["model(x)"]
    for arm in list(arms)[1:]:
        say(f"  {arm} - model(x): {(ms[arm] - base) * 1e3:+.1f} us per call ({(ms[arm] - base) / base * 100:+.3f} %)")
    telemetry_line(t)
    r = meter.result()
    say(f"  the meter after {r.count} rows: top1 {r.top1:.4f}, top5 {r.accuracy(5):.4f}, mean loss {r.loss:.4f}")


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 30
    if not torch.cuda.is_available():
        sys.exit("score_probe needs a GPU: nothing here can be measured without one")
    say(f"device: {torch.cuda.get_device_name(0)}")
    op_level(rounds)
    if "--skip-models" not in sys.argv:
        for name, batch in MODELS:
            model_level(name, batch, rounds)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

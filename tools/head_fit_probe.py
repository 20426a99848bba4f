"""What fitting a head on the device costs, in ONE process:

    python tools/head_fit_probe.py [--rounds R] [--out FILE] [--skip-models]

(1) tfimm_hip_head_update alone at (B, D, C) = (256, 2048, 1000), (256, 768, 5) and (4096, 768, 100), sgd and adam: a captured
graph of LAUNCHES launches per arm, the graphs replayed alternately (R rounds after a warm-up, HIP events around each replay),
microseconds per launch against the bytes the step must move once -- w and the slots read and written, w16 written, f and g
read -- at 8 TB/s.
(2) the three-launch step (``LinearProbe.step``) against torch's linear + cross-entropy + backward + ``torch.optim`` step on the
same features (float32 parameters, eager, as a caller would run it), called alternately, HIP events around each call.
(3) resnet50 at batch 256: ``model.fit_head(x, labels, probe)`` against ``model.evaluate(x, labels)``, alternately.
Not a bench.py line."""
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
from tfimm.train.linear_probe import step_scalars  # noqa: E402
from tfimm.utils.init import synthetic_weights  # noqa: E402

SHAPES = [(256, 2048, 1000), (256, 768, 5), (4096, 768, 100)]
MODELS = [("resnet50", 256)]
LAUNCHES = 20
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


def step_bytes(B, D, Cn, adam):
    """w and the slots in and out, w16 out, f and g in"""
    return Cn * D * 4 * 2 * (3 if adam else 2) + Cn * D * 2 + B * D * 2 + B * ((Cn + 7) // 8 * 8) * 2


def op_level(rounds):
    say(f"tfimm_hip_head_update alone: graphs of {LAUNCHES} launches, replayed alternately, {rounds} rounds after 3 warm-up rounds")
    g = torch.Generator().manual_seed(2021)
    arms = []
    for B, D, Cn in SHAPES:
        ldg = (Cn + 7) // 8 * 8
        f = torch.randn(B, D, generator=g).to("cuda", torch.bfloat16)
        gr = ((torch.rand(B, ldg, generator=g) - 0.5) * 0.1).to("cuda", torch.bfloat16)
        labels = torch.randint(0, Cn, (B,), generator=g, dtype=torch.int32).to("cuda")
        for name in ("sgd", "adam"):
            w = (torch.randn(Cn, D, generator=g) * 0.05).to("cuda")
            bufs = [w, torch.zeros_like(w), torch.zeros_like(w), torch.zeros(Cn, device="cuda"), torch.zeros(Cn, device="cuda"),
                    torch.zeros(Cn, device="cuda"), w.to(torch.bfloat16)]
            d = ffi.HeadUpdateDesc()
            d.f, d.g, d.labels = f.data_ptr(), gr.data_ptr(), labels.data_ptr()
            d.w, d.s1, d.s2, d.bias, d.bias_s1, d.bias_s2, d.w16 = (t.data_ptr() for t in bufs)
            d.B, d.D, d.C = B, D, Cn
            d.ldf, d.ldg, d.ldw, d.ldw16 = D, ldg, D, D
            d.opt = ffi.HEAD_ADAM if name == "adam" else ffi.HEAD_SGD
            d.lr, d.mom_or_one_minus_b1, d.one_minus_b2, d.eps, d.wd2 = step_scalars(name, 1e-3, (0.9, 0.999), 1e-7, 1e-4, 10)

            def launch(d=d):
                ffi.check(ffi.lib.tfimm_hip_head_update(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                          "tfimm_hip_head_update")
            w0 = w.clone()
            launch()
            torch.cuda.synchronize()
            # one sgd step from zero momentum is w - lr * (g^T f / n + wd2 * w): the probe times what it can check
            if name == "sgd":
                want = w0 - 1e-3 * (gr[:, :Cn].float().T @ f.float() / B + 2e-4 * w0)
                assert torch.allclose(w, want, rtol=1e-4, atol=1e-6), "the probe's launch disagrees with torch"
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                for _ in range(LAUNCHES):
                    launch()
            arms.append(dict(shape=(B, D, Cn), what=name, graph=graph, times=[], keep=(f, gr, labels, bufs, d)))
    for _ in range(3):
        for a in arms:
            timed(a["graph"].replay)
    for _ in range(rounds):
        for a in arms:
            a["times"].append(timed(a["graph"].replay) / LAUNCHES * 1e3)
    for a in arms:
        B, D, Cn = a["shape"]
        us = float(np.median(a["times"]))
        nbytes = step_bytes(B, D, Cn, a["what"] == "adam")
        floor = nbytes / HBM_BYTES_PER_S * 1e6
        say(f"  B={B:4d} D={D:4d} C={Cn:4d} {a['what']:4s}: {us:8.2f} us/launch (min {min(a['times']):.2f}, max {max(a['times']):.2f}); "
            f"{nbytes / 1e6:7.2f} MB once, floor {floor:6.2f} us; {us / floor:6.1f} x floor; {nbytes / us / 1e6:6.3f} TB/s")


def step_level(rounds):
    say(f"LinearProbe.step (3 launches) against torch linear + cross_entropy + backward + optim.step: {rounds} calls per arm, "
        f"alternating, HIP events around each call")
    g = torch.Generator().manual_seed(7)
    for B, D, Cn in SHAPES:
        f = torch.randn(B, D, generator=g).to("cuda")
        f16 = f.to(torch.bfloat16)
        labels = torch.randint(0, Cn, (B,), generator=g).to("cuda")
        labels32 = labels.to(torch.int32)
        for name in ("sgd", "adam"):
            probe = tfimm.LinearProbe(D, Cn, optimizer=name, lr=1e-3, weight_decay=0.0)
            lin = torch.nn.Linear(D, Cn).to("cuda")
            opt = (torch.optim.SGD(lin.parameters(), lr=1e-3, momentum=0.9) if name == "sgd"
                   else torch.optim.Adam(lin.parameters(), lr=1e-3, eps=1e-7))
            keep = {}

            def ours():
                keep["ours"] = probe.step(f16, labels32)

            def theirs():
                opt.zero_grad(set_to_none=True)
                loss = torch.nn.functional.cross_entropy(lin(f), labels)
                loss.backward()
                opt.step()
                keep["theirs"] = loss
            arms = {"LinearProbe.step": ours, "torch": theirs}
            for _ in range(5):
                for fn in arms.values():
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in arms}
            for _ in range(rounds):
                for k, fn in arms.items():
                    times[k].append(timed(fn) * 1e3)
            us = {k: float(np.median(v)) for k, v in times.items()}
            say(f"  B={B:4d} D={D:4d} C={Cn:4d} {name:4s}: step {us['LinearProbe.step']:8.1f} us (min {min(times['LinearProbe.step']):.1f}), "
                f"torch {us['torch']:8.1f} us (min {min(times['torch']):.1f}); torch / step {us['torch'] / us['LinearProbe.step']:.2f}")


def model_level(name, batch, rounds):
    m = tfimm.create_model(name)
    m.set_weights(synthetic_weights(m, 2021))
    g = torch.Generator().manual_seed(2021)
    x = torch.randn(batch, *m.cfg.input_size, m.cfg.in_channels, generator=g).to("cuda", torch.bfloat16)
    labels = torch.randint(0, m.cfg.nb_classes, (batch,), generator=g).to("cuda")
    probe = tfimm.LinearProbe.for_model(m, optimizer="sgd", lr=1e-3)
    keep = {}

    def evaluate():
        keep["evaluate"] = m.evaluate(x, labels)

    def fit():
        keep["fit"] = m.fit_head(x, labels, probe)
    arms = {"model.evaluate(x, labels)": evaluate, "model.fit_head(x, labels, probe)": fit}
    for _ in range(5):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times = {arm: [] for arm in arms}
    for _ in range(rounds):
        for arm, fn in arms.items():
            times[arm].append(timed(fn))
    say(f"{name} batch {batch} ({m.cfg.nb_classes} classes): {rounds} calls per arm, alternating, HIP events around each call")
    ms = {arm: float(np.median(times[arm])) for arm in arms}
    for arm in arms:
        say(f"  {arm:36s} {ms[arm]:9.4f} ms/call (min {min(times[arm]):.4f}, max {max(times[arm]):.4f})")
    a, b = list(arms)
    say(f"  fit_head - evaluate: {(ms[b] - ms[a]) * 1e3:+.1f} us per call ({(ms[b] - ms[a]) / ms[a] * 100:+.3f} %)")


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 30
    if not torch.cuda.is_available():
        sys.exit("head_fit_probe needs a GPU: nothing here can be measured without one")
    say(f"device: {torch.cuda.get_device_name(0)}")
    op_level(rounds)
    step_level(rounds)
    if "--skip-models" not in sys.argv:
        for name, batch in MODELS:
            model_level(name, batch, rounds)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

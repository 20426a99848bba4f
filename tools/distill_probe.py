"""What distilling an embedding head on the device costs, in ONE process:

    python tools/distill_probe.py [--rounds R] [--out FILE]

(1) tfimm_hip_distill_grad alone at (B, E) = (256, 128), (256, 512), (4096, 512) and (256, 2048), both modes: a captured graph
of LAUNCHES launches per arm, the graphs replayed alternately (R rounds after a warm-up, HIP events around each replay),
microseconds per launch against the bytes the launch must move once -- s and t read, the bf16 gradient written, valid read,
loss and cosine written: 10 B E + 12 B -- at 8 TB/s.
(2) the three-launch step (``EmbeddingProbe.step``) against torch's linear + ``normalize`` + squared error + backward +
``torch.optim`` step on the same features (float32 parameters, eager, as a caller would run it), called alternately, HIP
events around each call.
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

SHAPES = [(256, 128), (256, 512), (4096, 512), (256, 2048)]
STEP_SHAPES = [(256, 768, 128), (256, 2048, 512), (4096, 768, 512)]       # (B, D, E)
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


def op_level(rounds):
    say(f"tfimm_hip_distill_grad alone: graphs of {LAUNCHES} launches, replayed alternately, {rounds} rounds after 3 warm-up rounds")
    g = torch.Generator().manual_seed(2021)
    arms = []
    for B, E in SHAPES:
        s = torch.randn(B, E, generator=g).to("cuda")
        t = torch.randn(B, E, generator=g).to("cuda")
        valid = torch.zeros(B, dtype=torch.int32, device="cuda")
        for normalize in (1, 0):
            grad = torch.zeros(B, E, dtype=torch.bfloat16, device="cuda")
            loss, cosine = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")

            def launch(s=s, t=t, valid=valid, grad=grad, loss=loss, cosine=cosine, B=B, E=E, normalize=normalize):
                ffi.check(ffi.lib.tfimm_hip_distill_grad(s.data_ptr(), E, t.data_ptr(), E, B, E, valid.data_ptr(), normalize,
                                                         grad.data_ptr(), E, loss.data_ptr(), cosine.data_ptr(),
                                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tfimm_hip_distill_grad")
            launch()
            torch.cuda.synchronize()
            # the probe times what it can check: the loss against torch's on the same rows
            if normalize:
                want = ((torch.nn.functional.normalize(s, dim=1) - torch.nn.functional.normalize(t, dim=1)) ** 2).sum(dim=1)
            else:
                want = ((s - t) ** 2).sum(dim=1)
            assert torch.allclose(loss, want, rtol=1e-4, atol=1e-5), "the probe's launch disagrees with torch"
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                for _ in range(LAUNCHES):
                    launch()
            arms.append(dict(shape=(B, E), normalize=normalize, graph=graph, times=[], keep=(s, t, valid, grad, loss, cosine)))
    for _ in range(3):
        for a in arms:
            timed(a["graph"].replay)
    for _ in range(rounds):
        for a in arms:
            a["times"].append(timed(a["graph"].replay) / LAUNCHES * 1e3)
    for a in arms:
        B, E = a["shape"]
        us = float(np.median(a["times"]))
        nbytes = 10 * B * E + 12 * B
        floor = nbytes / HBM_BYTES_PER_S * 1e6
        say(f"  B={B:4d} E={E:4d} normalize={a['normalize']}: {us:8.2f} us/launch (min {min(a['times']):.2f}, max {max(a['times']):.2f}); "
            f"{nbytes / 1e6:7.3f} MB once, floor {floor:6.3f} us; {us / floor:7.1f} x floor; {nbytes / us / 1e6:6.3f} TB/s")


def step_level(rounds):
    say(f"EmbeddingProbe.step (3 launches) against torch linear + normalize + squared error + backward + optim.step: {rounds} calls "
        f"per arm, alternating, HIP events around each call")
    g = torch.Generator().manual_seed(7)
    for B, D, E in STEP_SHAPES:
        f = torch.randn(B, D, generator=g).to("cuda")
        f16 = f.to(torch.bfloat16)
        teacher = torch.randn(B, E, generator=g).to("cuda")
        valid = torch.ones(B, dtype=torch.bool, device="cuda")
        for name in ("sgd", "adam"):
            probe = tfimm.EmbeddingProbe(D, E, optimizer=name, lr=1e-3, weight_decay=0.0)
            lin = torch.nn.Linear(D, E).to("cuda")
            opt = (torch.optim.SGD(lin.parameters(), lr=1e-3, momentum=0.9) if name == "sgd"
                   else torch.optim.Adam(lin.parameters(), lr=1e-3, eps=1e-7))
            keep = {}

            def ours():
                keep["ours"] = probe.step(f16, teacher, valid)

            def theirs():
                opt.zero_grad(set_to_none=True)
                u = torch.nn.functional.normalize(lin(f), dim=1)
                v = torch.nn.functional.normalize(teacher, dim=1)
                loss = ((u - v) ** 2).sum(dim=1).mean()
                loss.backward()
                opt.step()
                keep["theirs"] = loss
            arms = {"EmbeddingProbe.step": ours, "torch": theirs}
            for _ in range(5):
                for fn in arms.values():
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in arms}
            for _ in range(rounds):
                for k, fn in arms.items():
                    times[k].append(timed(fn) * 1e3)
            us = {k: float(np.median(v)) for k, v in times.items()}
            say(f"  B={B:4d} D={D:4d} E={E:4d} {name:4s}: step {us['EmbeddingProbe.step']:8.1f} us (min {min(times['EmbeddingProbe.step']):.1f}), "
                f"torch {us['torch']:8.1f} us (min {min(times['torch']):.1f}); torch / step {us['torch'] / us['EmbeddingProbe.step']:.2f}")


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 30
    if not torch.cuda.is_available():
        sys.exit("distill_probe needs a GPU: nothing here can be measured without one")
    say(f"device: {torch.cuda.get_device_name(0)}")
    op_level(rounds)
    step_level(rounds)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

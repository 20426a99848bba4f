"""What the inverted-list gallery search costs and finds, in ONE process:

    python tools/search_index_probe.py [--rounds R] [--out FILE] [--shapes 0,1,2,3]

Data: clustered unit rows -- CENTRES random unit centres, a row is its centre plus NOISE times a unit-scale normal vector,
normalised; the queries are drawn the same way.  Per shape (B, N, E, n_lists) a ``tfimm.Gallery`` is filled on the device,
clustered (``kmeans``, 10 iterations) and indexed (``build_index``); both are timed once, wall clock around a synchronise.
Per (shape, k) the arms are: INDEX at nprobe 1, 8 and 32 (the probe of the centroids plus tfimm_hip_embed_search_lists), the
exact LIST path (tfimm_hip_embed_search, k <= 64) and BUFFER path (tfimm_hip_embed_search_wide) -- the faster one is what the
index is held against -- and the torch baseline ``(q.bfloat16() @ g.T).float().topk(k)`` (probe only, never on the product
path).  Each arm is a captured graph of LAUNCHES searches; the arms are replayed alternately (R rounds after a warm-up, HIP
events around each replay); microseconds per search as median (min - max).  Pass 1's floor: the bytes of the lists the batch
probes (every query's lists counted, shared or not) at 8 TB/s.  The probe, pass 1 and pass 2 of an index search are timed apart
in a run of their own outside the timed rounds: ten eager searches under ``torch.profiler``, kernel time by kernel name.
Recall: the share of the exact path's indices that the index result holds, per query.  Not a bench.py line."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tensorflow-image-models_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tfimm  # noqa: E402
from tfimm.engine import ffi  # noqa: E402

#: (B, N, E, n_lists); None: what build_index derives, round(sqrt(N))
SHAPES = [(32, 1_000_000, 512, 1024), (256, 100_000, 512, 256), (32, 1_000_000, 128, None), (1024, 1_000_000, 512, 1024)]
NPROBES, KS = (1, 8, 32), (5, 20, 64, 200)
CENTRES, NOISE = 4096, 1.0
HBM_BYTES_PER_S = 8e12
LIST, BUFFER, TORCH, INDEX = "list   tfimm_hip_embed_search", "buffer tfimm_hip_embed_search_wide", "torch  matmul + topk", "index  nprobe="
PASSES = ("embed_lists_pass1", "embed_lists_pass2")
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


def record(fn, launches):
    fn()                              # workspaces and torch's own set-up stay outside the recording
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for _ in range(launches):
            fn()
    return graph


def clustered(gen, centres, n, E):
    """``n`` unit rows (float32, on the device) around the unit ``centres``"""
    at = torch.randint(0, centres.shape[0], (n,), generator=gen, device="cuda")
    x = centres[at] + NOISE * torch.randn(n, E, generator=gen, device="cuda") / E ** 0.5
    return x / x.norm(dim=1, keepdim=True)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


_BUILT = {}


def built(N, E, L):
    """(gallery, index, centres, generator) for (N, E, L), seeded; one gallery at a time on the device"""
    if (N, E, L) not in _BUILT:
        _BUILT.clear()
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(2021)
        centres = torch.randn(CENTRES, E, generator=gen, device="cuda")
        centres /= centres.norm(dim=1, keepdim=True)
        gallery = tfimm.Gallery(E, capacity=N)
        for lo in range(0, N, 100_000):
            gallery.add(clustered(gen, centres, min(100_000, N - lo), E))
        n_lists = L if L is not None else min(max(int(round(N ** 0.5)), 1), ffi.CLUSTER_MAX_C)
        clusters, t_kmeans = wall(lambda: gallery.kmeans(n_lists, iters=10))
        index, t_lists = wall(lambda: gallery.build_index(clusters=clusters))
        counts = index.counts.numpy()
        say(f"gallery N={N} E={E}: n_lists {index.n_lists}, kmeans (10 iterations) {t_kmeans * 1e3:.0f} ms, lists (sort, offsets, the "
            f"list-ordered copy of {N * E * 2 / 1e6:.0f} MB, one synchronisation) {t_lists * 1e3:.1f} ms; list length mean "
            f"{counts.mean():.0f}, largest {counts.max()}, empty lists {(counts == 0).sum()}; parts {index.parts}")
        _BUILT[(N, E, L)] = (gallery, index, centres, gen)
    return _BUILT[(N, E, L)]


def outputs(B, k):
    return torch.empty(B, k, dtype=torch.float32, device="cuda"), torch.empty(B, k, dtype=torch.int32, device="cuda")


def exact(entry, q, gallery, B, k, launches):
    N, E = len(gallery), gallery.dim
    need = getattr(ffi.lib, entry + "_workspace")(B, N, E, k, 0)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    scores, indices = outputs(B, k)

    def search():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(getattr(ffi.lib, entry)(q.data_ptr(), E, B, gallery._buf.data_ptr(), gallery.pitch, N, E, k, 0, scores.data_ptr(),
                                          indices.data_ptr(), work.data_ptr(), need, st), entry)
    # the graph holds the workspace's address, not the tensor: it stays referenced for as long as the graph is replayed
    return dict(graph=record(search, launches), times=[], scores=scores, indices=indices, workspace=work)


def indexed(q, index, B, k, nprobe, launches):
    """the two entry points of ``GalleryIndex.search`` over buffers allocated once"""
    E, cen = index.dim, index.centroids
    probe = "tfimm_hip_embed_search" if cen._route(nprobe) == "list" else "tfimm_hip_embed_search_wide"
    need_p = getattr(ffi.lib, probe + "_workspace")(B, len(cen), E, nprobe, 0)
    need = ffi.lib.tfimm_hip_embed_search_lists_workspace(B, index.size, E, index.n_lists, nprobe, k, index.parts)
    work_p, work = torch.empty(need_p, dtype=torch.uint8, device="cuda"), torch.empty(need, dtype=torch.uint8, device="cuda")
    pscores, probes = outputs(B, nprobe)
    scores, indices = outputs(B, k)

    def search():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(getattr(ffi.lib, probe)(q.data_ptr(), E, B, cen._buf.data_ptr(), cen.pitch, len(cen), E, nprobe, 0, pscores.data_ptr(),
                                          probes.data_ptr(), work_p.data_ptr(), need_p, st), probe)
        ffi.check(ffi.lib.tfimm_hip_embed_search_lists(q.data_ptr(), E, B, index._rows.data_ptr(), index.pitch, index.size, E,
                                                       index._ids.data_ptr(), index._offsets.data_ptr(), index.n_lists, probes.data_ptr(),
                                                       nprobe, nprobe, k, index.parts, scores.data_ptr(), indices.data_ptr(),
                                                       work.data_ptr(), need, st), "tfimm_hip_embed_search_lists")
    return dict(graph=record(search, launches), times=[], scores=scores, indices=indices, probes=probes, search=search,
                keep=(work_p, work, pscores))


def passes(search):
    """microseconds of kernel time per search: the probe (every other kernel), pass 1, pass 2; ten eager searches under
    torch.profiler"""
    try:
        from torch.profiler import ProfilerActivity, profile
    except ImportError as e:                  # a torch without the profiler still measures the whole; a failing search is not caught
        return f"unavailable ({type(e).__name__}: {e})"
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(10):
            search()
        torch.cuda.synchronize()
    out = {"probe": 0.0}
    for ev in prof.key_averages():
        total = getattr(ev, "device_time_total", None)
        us = (ev.cuda_time_total if total is None else total) / 10
        name = next((n for n in PASSES if n in ev.key), "probe")
        out[name] = out.get(name, 0.0) + us
    return out if all(n in out for n in PASSES) else f"the profiler named {sorted(out)}"


def recall(got, want):
    """the mean share of a query's exact indices that the index result holds"""
    return float((got.long()[:, :, None] == want.long()[:, None, :]).any(1).float().mean())


def level(shape, k, rounds):
    B, N, E, L = shape
    gallery, index, centres, _ = built(N, E, L)
    launches = 10 if B < 1024 else 2
    q = clustered(torch.Generator(device="cuda").manual_seed(B + k), centres, B, E).contiguous()
    g = gallery._buf[:N, :E]
    base = {}

    def baseline():
        base["out"] = (q.bfloat16() @ g.T).float().topk(k)

    arms = {}
    if k <= ffi.EMBED_MAX_K:
        arms[LIST] = exact("tfimm_hip_embed_search", q, gallery, B, k, launches)
    arms[BUFFER] = exact("tfimm_hip_embed_search_wide", q, gallery, B, k, launches)
    names = []
    for nprobe in NPROBES:
        if nprobe <= index.n_lists:
            names.append(f"{INDEX}{nprobe}")
            arms[names[-1]] = indexed(q, index, B, k, nprobe, launches)
    arms[TORCH] = dict(graph=record(baseline, launches), times=[])
    for _ in range(3):
        for a in arms.values():
            timed_replay(a["graph"])
    for _ in range(rounds):
        for a in arms.values():
            a["times"].append(timed_replay(a["graph"]) / launches * 1e3)
    say(f"B={B} N={N} E={E} n_lists={index.n_lists} k={k}: one read of the gallery {N * E * 2 / HBM_BYTES_PER_S * 1e6:.1f} us "
        f"(graphs of {launches} searches)")
    for name, a in arms.items():
        a["us"] = float(np.median(a["times"]))
        say(f"  {name:36s} {a['us']:10.1f} us/search (min {min(a['times']):.1f}, max {max(a['times']):.1f})")
    best = min((n for n in (LIST, BUFFER) if n in arms), key=lambda n: arms[n]["us"])
    out = {"exact": arms[best]["us"], "torch": arms[TORCH]["us"]}
    counts = index.counts.torch().long()
    for name in names:
        a, want = arms[name], arms[BUFFER]
        rows = int(counts[a["probes"].long().clamp(0, index.n_lists - 1)].sum())
        floor = rows * E * 2 / HBM_BYTES_PER_S * 1e6
        short = int((a["indices"] < 0).sum())
        say(f"  {name}: recall against the exact path {recall(a['indices'], want['indices']) * 100:.2f} %, {short} empty slots; "
            f"{rows / B:.0f} rows probed per query, {rows * E * 2} bytes: pass 1's floor {floor:.2f} us; "
            f"index / {best.split()[0]} {a['us'] / out['exact']:.2f}, index / torch {a['us'] / out['torch']:.2f}")
        p = passes(a["search"])
        if isinstance(p, dict):
            say(f"    kernel time per search: probe {p['probe']:.1f} us, pass 1 {p[PASSES[0]]:.1f} us "
                f"({p[PASSES[0]] / max(floor, 1e-9):.1f} x its floor), pass 2 {p[PASSES[1]]:.1f} us")
        else:
            say(f"    kernel time per pass: {p}")
        out[name] = (a["us"], recall(a["indices"], want["indices"]))
    return out


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 20
    which = [int(s) for s in sys.argv[sys.argv.index("--shapes") + 1].split(",")] if "--shapes" in sys.argv else range(len(SHAPES))
    if not torch.cuda.is_available():
        sys.exit("search_index_probe needs a GPU: nothing here can be measured without one")
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"data: unit rows around {CENTRES} unit centres, noise {NOISE}; the arms replayed alternately, {rounds} rounds after 3 warm-up rounds")
    table = []
    for i in which:
        for k in KS:
            table.append((SHAPES[i], k, level(SHAPES[i], k, rounds)))
    say("index against the faster exact path and against torch, medians (us/search; recall in %):")
    for (B, N, E, _), k, r in table:
        cells = ", ".join(f"nprobe {n[len(INDEX):]}: {r[n][0]:.1f} ({r[n][0] / r['exact']:.2f} x exact, {r[n][0] / r['torch']:.2f} x torch, "
                          f"recall {r[n][1] * 100:.1f})" for n in r if n.startswith(INDEX))
        say(f"  B={B} N={N} E={E} k={k}: exact {r['exact']:.1f}, torch {r['torch']:.1f}; {cells}")


if __name__ == "__main__":
    main()

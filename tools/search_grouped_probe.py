"""What grouping the queries of a probed list into MFMA tiles buys and costs, in ONE process:

    python tools/search_grouped_probe.py [--rounds R] [--out FILE] [--shapes 0,1,2,3] [--no-neighbours]

Data, galleries and indexes are tools/search_index_probe.py's (clustered unit rows, ``kmeans`` of 10 iterations, ``build_index``).
Per (shape, nprobe, k) the arms are: GROUPED (the probe of the centroids plus tfimm_hip_embed_search_lists_grouped), SINGLE (the
same probe plus tfimm_hip_embed_search_lists: ``GalleryIndex.search``), the exact LIST path (tfimm_hip_embed_search, k <= 64)
and BUFFER path (tfimm_hip_embed_search_wide) -- the faster one is reported -- and the torch baseline
``(q.bfloat16() @ g.T).float().topk(k)``, 1024 queries at a time (probe only, never on the product path).  Each arm is a
captured graph of LAUNCHES searches; the arms are replayed alternately (R rounds after a warm-up, HIP events around each replay); microseconds per search
as median (min - max).  The two exact arms and torch do not depend on nprobe: they are measured once per (shape, k), next to the
index arms of every nprobe.  Of a grouped search the grouping (fill, rank, scan, place), pass 1 and pass 2 are timed apart in a
run of their own: eager searches under ``torch.profiler``, kernel time by kernel name.  The tables of the last search say how
many tiles it used against the bound the grid is launched with, and how many lanes of a tile hold a query; pass 1's floor is
the bytes of (tiles x the rows of their lists) at 8 TB/s.  The two results are compared bit for bit.  Last, the kNN graph of the
million-row index (``neighbours(k = 20, nprobe = 8)``) end to end by both methods, wall clock.  Not a bench.py line."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tensorflow-image-models_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import search_index_probe as sip  # noqa: E402
from search_index_probe import BUFFER, HBM_BYTES_PER_S, LIST, TORCH, built, clustered, exact, outputs, record, say, timed_replay, wall  # noqa: E402
from tfimm.engine import ffi  # noqa: E402

#: (B, N, E, n_lists)
SHAPES = [(32, 1_000_000, 512, 1024), (256, 100_000, 512, 256), (1024, 1_000_000, 512, 1024), (8192, 1_000_000, 512, 1024)]
NPROBES, KS = (1, 8, 32), (5, 20, 200)
GROUPED, SINGLE = "grouped nprobe=", "single  nprobe="
GROUPING = ("grouped_fill", "grouped_rank", "grouped_scan", "grouped_place")
PASS1, PASS2 = "embed_lists_grouped_pass1", "embed_lists_grouped_pass2"


def grouped(q, index, B, k, nprobe, launches):
    """the probe and tfimm_hip_embed_search_lists_grouped over buffers allocated once, as ``sip.indexed`` has the single entry"""
    E, cen = index.dim, index.centroids
    probe = "tfimm_hip_embed_search" if cen._route(nprobe) == "list" else "tfimm_hip_embed_search_wide"
    need_p = getattr(ffi.lib, probe + "_workspace")(B, len(cen), E, nprobe, 0)
    need = ffi.lib.tfimm_hip_embed_search_lists_grouped_workspace(B, index.size, E, index.n_lists, nprobe, k, index.parts)
    work_p, work = torch.empty(need_p, dtype=torch.uint8, device="cuda"), torch.empty(need, dtype=torch.uint8, device="cuda")
    pscores, probes = outputs(B, nprobe)
    scores, indices = outputs(B, k)

    def search():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(getattr(ffi.lib, probe)(q.data_ptr(), E, B, cen._buf.data_ptr(), cen.pitch, len(cen), E, nprobe, 0, pscores.data_ptr(),
                                          probes.data_ptr(), work_p.data_ptr(), need_p, st), probe)
        ffi.check(ffi.lib.tfimm_hip_embed_search_lists_grouped(q.data_ptr(), E, B, index._rows.data_ptr(), index.pitch, index.size, E,
                                                               index._ids.data_ptr(), index._offsets.data_ptr(), index.n_lists,
                                                               probes.data_ptr(), nprobe, nprobe, k, index.parts, scores.data_ptr(),
                                                               indices.data_ptr(), work.data_ptr(), need, st),
                  "tfimm_hip_embed_search_lists_grouped")
    return dict(graph=record(search, launches), times=[], scores=scores, indices=indices, probes=probes, search=search, work=work,
                keep=(work_p, pscores))


def tables(a, index, B, k, nprobe):
    """(tiles used, live pairs, gallery rows read by pass 1) from the tables the last search left in its workspace: count [L]
    and first [L + 1] stand behind the pair arrays"""
    L = index.n_lists
    words = a["work"].view(torch.int32)
    at = B * nprobe * index.parts * k * 2
    count, total = words[at:at + L].long(), int(words[at + 2 * L])
    tiles = (count + 31) // 32
    assert int(tiles.sum()) == total
    return total, int(count.sum()), int((tiles * index.counts.torch().long()).sum())


def passes(search, times):
    """microseconds of kernel time per search: the probe (every other kernel), the grouping, pass 1, pass 2"""
    try:
        from torch.profiler import ProfilerActivity, profile
    except ImportError as e:
        return f"unavailable ({type(e).__name__}: {e})"
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(times):
            search()
        torch.cuda.synchronize()
    out = {"probe": 0.0, "grouping": 0.0}
    for ev in prof.key_averages():
        total = getattr(ev, "device_time_total", None)
        us = (ev.cuda_time_total if total is None else total) / times
        name = "grouping" if any(n in ev.key for n in GROUPING) else next((n for n in (PASS1, PASS2) if n in ev.key), "probe")
        out[name] = out.get(name, 0.0) + us
    return out if PASS1 in out and PASS2 in out else f"the profiler named {sorted(out)}"


def level(shape, k, rounds):
    B, N, E, L = shape
    gallery, index, centres, _ = built(N, E, L)
    launches = 10 if B < 1024 else (2 if B < 8192 else 1)
    q = clustered(torch.Generator(device="cuda").manual_seed(B + k), centres, B, E).contiguous()
    g = gallery._buf[:N, :E]
    base = {}

    def baseline():
        base["out"] = [(q[lo:lo + 1024].bfloat16() @ g.T).float().topk(k) for lo in range(0, B, 1024)]      # 4 GB of scores at a time

    arms = {}
    if k <= ffi.EMBED_MAX_K:
        arms[LIST] = exact("tfimm_hip_embed_search", q, gallery, B, k, launches)
    arms[BUFFER] = exact("tfimm_hip_embed_search_wide", q, gallery, B, k, launches)
    for nprobe in NPROBES:
        arms[f"{GROUPED}{nprobe}"] = grouped(q, index, B, k, nprobe, launches)
        arms[f"{SINGLE}{nprobe}"] = sip.indexed(q, index, B, k, nprobe, launches)
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
    for nprobe in NPROBES:
        a, s = arms[f"{GROUPED}{nprobe}"], arms[f"{SINGLE}{nprobe}"]
        equal = bool(torch.equal(a["indices"], s["indices"]) and torch.equal(a["scores"].view(torch.int32), s["scores"].view(torch.int32)))
        tiles, live, rows = tables(a, index, B, k, nprobe)
        bound = ffi.lib.tfimm_hip_embed_search_lists_grouped_tiles(B, index.n_lists, nprobe)
        floor = rows * E * 2 / HBM_BYTES_PER_S * 1e6
        say(f"  nprobe={nprobe}: grouped / single {a['us'] / s['us']:.2f}, grouped / {best.split()[0]} {a['us'] / out['exact']:.2f}, grouped / "
            f"torch {a['us'] / out['torch']:.2f}; bit-equal to single: {equal}; tiles {tiles} of T_max {bound} x parts {index.parts}, "
            f"{live / max(tiles, 1):.1f} of 32 lanes occupied; pass 1 reads {rows * E * 2} bytes: floor {floor:.2f} us")
        p = passes(a["search"], 10 if B < 1024 else 3)
        if isinstance(p, dict):
            say(f"    kernel time per search: probe {p['probe']:.1f} us, grouping {p['grouping']:.1f} us, pass 1 {p[PASS1]:.1f} us "
                f"({p[PASS1] / max(floor, 1e-9):.1f} x its floor), pass 2 {p[PASS2]:.1f} us")
        else:
            say(f"    kernel time per pass: {p}")
        out[nprobe] = (a["us"], s["us"], equal, live / max(tiles, 1))
    return out


def neighbours(N, E, L):
    _, index, _, _ = built(N, E, L)
    got = {}
    for method in ("grouped", "single"):
        index.neighbours(20, 8, 8192, method)                                # workspaces and torch's own set-up
        got[method], t = wall(lambda: index.neighbours(20, 8, 8192, method))
        say(f"neighbours(k=20, nprobe=8, batch=8192, method={method!r}) of N={N} E={E} n_lists={index.n_lists}: {t * 1e3:.0f} ms end to "
            f"end ({-(-N // 8192)} batches of a probe, a search for 21 and the drop), {t / N * 1e6:.2f} us per row")
    a, b = got["grouped"], got["single"]
    say(f"  the two graphs bit-equal: {bool(torch.equal(a.indices.torch(), b.indices.torch()) and torch.equal(a.scores.torch().view(torch.int32), b.scores.torch().view(torch.int32)))}; "
        f"rows that are their own neighbour: {int((a.indices.torch() == torch.arange(N, device='cuda', dtype=torch.int32)[:, None]).sum())}; "
        f"empty slots {int((a.indices.torch() < 0).sum())}")


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 10
    which = [int(s) for s in sys.argv[sys.argv.index("--shapes") + 1].split(",")] if "--shapes" in sys.argv else range(len(SHAPES))
    if not torch.cuda.is_available():
        sys.exit("search_grouped_probe needs a GPU: nothing here can be measured without one")
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"data: unit rows around {sip.CENTRES} unit centres, noise {sip.NOISE}; the arms replayed alternately, {rounds} rounds after 3 warm-up rounds")
    table = []
    for i in which:
        for k in KS:
            table.append((SHAPES[i], k, level(SHAPES[i], k, rounds)))
    say("grouped against single, the faster exact path and torch, medians (us/search):")
    for (B, N, E, _), k, r in table:
        cells = ", ".join(f"nprobe {n}: grouped {r[n][0]:.1f} / single {r[n][1]:.1f} = {r[n][0] / r[n][1]:.2f} ({r[n][0] / r['exact']:.2f} x "
                          f"exact, {r[n][0] / r['torch']:.2f} x torch, {r[n][3]:.1f} lanes{'' if r[n][2] else ', BITS DIFFER'})" for n in NPROBES)
        say(f"  B={B} N={N} E={E} k={k}: exact {r['exact']:.1f}, torch {r['torch']:.1f}; {cells}")
    if "--no-neighbours" not in sys.argv:
        neighbours(1_000_000, 512, 1024)


if __name__ == "__main__":
    main()

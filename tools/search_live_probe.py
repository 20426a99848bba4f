"""What an index that follows its gallery costs, in ONE process:

    python tools/search_live_probe.py [--rounds R] [--out FILE]

Data and method are those of tools/search_index_probe.py: clustered unit rows, a million rows of 512 in 1024 lists; every arm is
a captured graph of LAUNCHES calls, the arms of a shape are replayed alternately (R rounds after 3 warm-up rounds, HIP events
around each replay); microseconds per call as median (min - max).

  MERGE alone: tfimm_hip_matches_merge of S sets of 64 columns into 64, against the bytes it must move once -- 8 (sum k_s + k) B,
  at 8 TB/s -- and against ``torch``: cat, a sort by (score, row), gather.
  LIVE: the gallery grows behind the snapshot by FRESH rows; per (fresh, queries, k) at nprobe = 8 the arms are
  ``index.search_live`` (method "single"), ``index.search_with`` on the snapshot (what the tail costs is the difference),
  ``gallery.search`` over all rows, ``torch`` matmul + topk over all rows, and -- apart -- the tail's exact search of the fresh
  rows and the merge of the two results.
  ABSORB: ``index.absorb()`` of the fresh rows (on a shallow copy: the snapshot stays) against ``build_index(clusters=...)`` over
  the same assignment and a full ``build_index()`` (k-means, 10 iterations), wall clock around a synchronise.
  RECALL: after growth by 10 % and by 100 % from the same distribution, the absorbed index (the old centroids) next to a fresh
  build, each against the exact search (1024 queries, k = 20, nprobe = 8).
Not a bench.py line."""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tensorflow-image-models_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import search_index_probe as sip  # noqa: E402
import tfimm  # noqa: E402
from tfimm.models.gallery import _merge_launch  # noqa: E402
from tfimm.models.model import Tensor  # noqa: E402

N, E, L, NPROBE = 1_000_000, 512, 1024, 8
FRESH, QUERIES, KS = (0, 1_000, 10_000, 100_000), (32, 1024), (5, 20, 200)
say = sip.say


def run(arms, rounds, launches):
    """the arms (name -> callable) as graphs of ``launches`` calls, replayed alternately -> name -> (median, min, max) us/call"""
    for fn in arms.values():              # every workspace reaches its size before any graph holds its address: an arm that
        fn()                              # outgrew a cached workspace behind another arm's capture would free what that graph uses
    torch.cuda.synchronize()
    graphs = {n: sip.record(fn, launches) for n, fn in arms.items()}
    times = {n: [] for n in arms}
    for r in range(3 + rounds):
        for n, g in graphs.items():
            t = sip.timed_replay(g) / launches * 1e3
            if r >= 3:
                times[n].append(t)
    return {n: (float(np.median(t)), min(t), max(t)) for n, t in times.items()}


def show(res, indent="  "):
    for n, (med, lo, hi) in res.items():
        say(f"{indent}{n:44s} {med:10.1f} us (min {lo:.1f}, max {hi:.1f})")


def merge_alone(rounds):
    say("MERGE alone: S sets of 64 columns into k = 64 (random scores, distinct rows)")
    gen = torch.Generator(device="cuda").manual_seed(5)
    for S in (2, 8):
        for B in (32, 8192):
            sets = []
            for s in range(S):
                sc = torch.randn(B, 64, generator=gen, device="cuda").sort(1, descending=True).values.contiguous()
                idx = torch.rand(B, 1000, generator=gen, device="cuda").argsort(1)[:, :64].int().contiguous()
                sets.append((idx, sc, 1000 * s))

            def baseline():
                sc = torch.cat([s for _, s, _ in sets], 1)
                rows = torch.cat([i + b for i, _, b in sets], 1)
                by_row = rows.argsort(dim=1, stable=True)
                sc2 = sc.gather(1, by_row)
                best = sc2.argsort(dim=1, descending=True, stable=True)[:, :64]
                return sc2.gather(1, best), rows.gather(1, by_row).gather(1, best)

            got, want = _merge_launch(sets, 64), baseline()
            assert torch.equal(got[0].long(), want[1].long()) and torch.equal(got[1], want[0])
            res = run({"tfimm_hip_matches_merge": lambda: _merge_launch(sets, 64), "torch cat + sort (score, row) + gather": baseline},
                      rounds, 20)
            moved = 8 * (64 * S + 64) * B
            say(f" S={S} B={B}: {moved} bytes once, {moved / sip.HBM_BYTES_PER_S * 1e6:.3f} us at 8 TB/s")
            show(res)


def live(gallery, index, centres, rounds, fresh):
    n = len(gallery)
    g = gallery._buf[:n, :E]
    for B in QUERIES:
        launches = 10 if B < 1024 else 2
        q = sip.clustered(torch.Generator(device="cuda").manual_seed(B + fresh), centres, B, E).contiguous()
        for k in KS:
            arms = {"index.search_live (single)": lambda: index.search_live(q, k, NPROBE),
                    "index.search_with on the snapshot (single)": lambda: index.search_with(q, k, NPROBE, 0, "single"),
                    "gallery.search over all rows": lambda: gallery.search(q, k),
                    "torch matmul + topk over all rows": lambda: (q.bfloat16() @ g.T).float().topk(k)}
            if fresh:
                start, rows, ks, path = gallery._range_args(k, index.size, n, "auto")
                head = index.search_with(q, k, NPROBE, 0, "single")
                hi, hs = head.indices.torch(), head.scores.torch()
                ti, ts = gallery._range_launch(q, ks, start, rows, path)
                arms[f"  the tail alone: exact search of the fresh rows ({path}, k = {ks})"] = lambda: gallery._range_launch(q, ks, start, rows, path)
                arms["  the merge alone"] = lambda: _merge_launch([(hi, hs, 0), (ti, ts, start)], k)
            res = run(arms, rounds, launches)
            say(f" fresh={fresh} B={B} k={k} nprobe={NPROBE} (graphs of {launches} calls)")
            show(res)
            names = list(arms)
            live_us, others = res[names[0]][0], {m: res[m][0] for m in names[1:4]}
            lost = [m.strip() for m, us in others.items() if m != names[1] and us < live_us]
            say(f"  search_live / snapshot {live_us / others[names[1]]:.2f}, / gallery.search {live_us / others[names[2]]:.2f}, "
                f"/ torch {live_us / others[names[3]]:.2f}" + (f"  ** LOSES to: {', '.join(lost)} **" if lost else ""))


def recall_of(index, gallery, q, live_too=False):
    want = gallery.search(q, 20).indices.torch()
    got = (index.search_live(q, 20, NPROBE) if live_too else index.search_with(q, 20, NPROBE, 0, "single")).indices.torch()
    return sip.recall(got, want) * 100


def absorb_and_recall(gallery, index, centres, gen, label):
    fresh = index.fresh
    absorbed = copy.copy(index)                       # absorb re-lays into new tensors: the snapshot keeps its own
    n_abs, t_abs = sip.wall(absorbed.absorb)
    assert n_abs == fresh and not absorbed.stale and index.fresh == fresh
    clusters = tfimm.Clusters(index.centroids, Tensor(absorbed._assignment()), None, None, None)
    _, t_lists = sip.wall(lambda: gallery.build_index(clusters=clusters))
    rebuilt, t_full = sip.wall(lambda: gallery.build_index(L))
    say(f"ABSORB {label}: {fresh} fresh rows into {index.size}: absorb() {t_abs * 1e3:.1f} ms; build_index(clusters=...) over the same "
        f"assignment {t_lists * 1e3:.1f} ms; a full build_index({L}) (k-means, 10 iterations) {t_full * 1e3:.0f} ms")
    q = sip.clustered(gen, centres, 1024, E).contiguous()
    say(f"RECALL {label} (1024 queries, k = 20, nprobe = {NPROBE}, against gallery.search): absorbed index {recall_of(absorbed, gallery, q):.2f} %, "
        f"fresh build {recall_of(rebuilt, gallery, q):.2f} %, the snapshot through search_live {recall_of(index, gallery, q, True):.2f} %, "
        f"the snapshot alone {recall_of(index, gallery, q):.2f} %; longest list {absorbed.longest} (absorbed) / {rebuilt.longest} (rebuilt)")
    return absorbed


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 10
    if not torch.cuda.is_available():
        sys.exit("search_live_probe needs a GPU: nothing here can be measured without one")
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"data: unit rows around {sip.CENTRES} unit centres, noise {sip.NOISE}; the arms replayed alternately, {rounds} rounds after 3 warm-up rounds")
    merge_alone(rounds)
    gallery, index, centres, gen = sip.built(N, E, L)
    for fresh in FRESH:
        while index.fresh < fresh:
            gallery.add(sip.clustered(gen, centres, min(100_000, fresh - index.fresh), E))
        say(f"LIVE: {index.fresh} fresh rows behind a snapshot of {index.size}")
        live(gallery, index, centres, rounds, fresh)
        if fresh == 10_000:
            absorb_and_recall(gallery, index, centres, gen, "10 000 rows (1 %)")
    absorbed = absorb_and_recall(gallery, index, centres, gen, "100 000 rows (10 %)")
    del index
    while len(gallery) < 2 * N:                       # growth by 100 %: the lists double, the centroids are those of the first million
        gallery.add(sip.clustered(gen, centres, 100_000, E))
    absorb_and_recall(gallery, absorbed, centres, gen, "to 2 000 000 rows (100 %; the index had absorbed the first 10 %)")


if __name__ == "__main__":
    main()

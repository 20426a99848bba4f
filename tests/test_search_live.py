"""The index that follows its gallery without a device: the written rules of tests/live_ref.py -- with every list
probed a live search is the exact search over all rows, a fresh row is found whatever is probed, short results fill with
-1 / -inf, and ``merge`` with bases, widths, empty sets and the special values --, the refusals of tfimm_hip_matches_merge before
any launch and its struct, the signatures of everything new, every ``ValueError`` before any device work, and ``absorb`` on an
index whose plumbing ran on the host."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import coarse_ref as cr
import embed_ref as er
import index_ref as ir
import live_ref as lr
import tfimm
from tfimm.engine import ffi
from tfimm.models.model import Tensor

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
grid = cr.grid
NINF, QNAN = 0xff800000, 0x7fffffff           # -inf; what bits_of gives for the key of every NaN


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(er.bits(a[1]), er.bits(b[1]))


# ---- the rules -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, size, L, k", [(300, 200, 7, 20), (1000, 997, 37, 64), (260, 10, 3, 200), (64, 40, 1, 5)])
def test_probing_every_list_with_a_live_tail_is_the_exact_search(N, size, L, k):
    """grid data: ties are frequent, and duplicated rows sit on BOTH sides of the snapshot boundary, so that equal scores are
    decided by the row across the two halves of the merge"""
    rng = np.random.default_rng(N + L)
    q, g, cen = grid(N, (6, 32)), grid(N + 1, (N, 32)), grid(N + 2, (L, 32))
    assignment = rng.integers(0, L, size)
    dup = np.concatenate([rng.choice(size, 6, replace=False), size + rng.choice(N - size, min(6, N - size), replace=False)])
    g[dup] = g[dup[0]]
    got = lr.search_live(q, g, cen, assignment, L, k)
    assert same(got, er.search(q, g, k))
    assert ((got[0] < size).any(1) & (got[0] >= size).any(1)).any()          # results that take rows from both halves


def test_a_fresh_row_is_found_although_its_list_is_not_probed():
    """the construction of test_search_index.py::test_a_row_in_an_unprobed_list_is_absent with the best row added AFTER the
    build: an index over all rows does not find it with one probe (its list's centroid is the negated query), the live search
    of the snapshot does"""
    q = grid(5, (1, 32))
    q[0, 0] = 0.5
    g = np.concatenate([q / 2, q / 4, -q, q])                    # row 3, the last, is the query itself
    cen = np.concatenate([-q, q])
    assert er.search(q, g, 1)[0].tolist() == [[3]]
    idx, _ = ir.search_index(q, g, cen, np.array([1, 1, 1, 0]), 1, 2)
    assert idx.tolist() == [[0, 1]] and 3 not in idx
    idx, sc = lr.search_live(q, g, cen, np.array([1, 1, 1]), 1, 2)
    assert idx.tolist() == [[3, 0]]
    assert np.array_equal(er.bits(sc), er.bits(er.search(q, g, 2)[1]))


def test_short_results_fill_with_none():
    q, g, cen = grid(1, (3, 16)), grid(2, (53, 16)), grid(3, (5, 16))
    assignment = np.arange(50) % 5
    idx, sc = lr.search_live(q, g, cen, assignment, 1, 25)      # one list of 10 rows and 3 fresh rows
    assert (idx[:, :13] >= 0).all() and (idx[:, 13:] == -1).all() and (er.bits(sc[:, 13:]) == NINF).all()
    for b in range(3):
        assert set(range(50, 53)) <= set(idx[b].tolist()) and len(set((idx[b, :13] % 5)[idx[b, :13] < 50].tolist())) == 1


def _m(idx, sc):
    return np.asarray(idx, np.int32).reshape(1, -1), np.asarray(sc, f32).reshape(1, -1)


def test_merge_bases_widths_and_empty_sets():
    a = _m([4, 0, 2, -1], [9, 7, 7, -np.inf])
    b = _m([1, 3], [8, 7])
    none = _m([-1, -1, -1], [-np.inf] * 3)
    idx, sc = lr.merge([a, b, none], [0, 0, 100])
    assert idx.tolist() == [[4, 1, 0, 2]] and sc.tolist() == [[9, 8, 7, 7]]              # k: the widest part; row 3 is cut
    idx, sc = lr.merge([a, b, none], [10, 0, 100], 7)
    assert idx.tolist() == [[14, 1, 3, 10, 12, -1, -1]] and sc[0, :5].tolist() == [9, 8, 7, 7, 7]
    assert (er.bits(sc[0, 5:]) == NINF).all()
    idx, sc = lr.merge([a, b], [0, 1], 2)                                                    # rows 2 and 2 + 0 never meet: bases keep them apart
    assert idx.tolist() == [[4, 2]] and sc.tolist() == [[9, 8]]
    idx, sc = lr.merge([none, none], None, 2)
    assert idx.tolist() == [[-1, -1]] and (er.bits(sc) == NINF).all()
    assert same(lr.merge([a]), (np.array([[4, 0, 2, -1]], np.int32), a[1]))                  # one set: a copy


def test_merge_special_values():
    nan_neg = np.array([0xffc12345], np.uint32).view(f32)[0]
    a = _m([5, 6, 7, 8], [np.inf, -0.0, -1.0, -np.inf])
    b = _m([0, 1, 2], [nan_neg, 0.0, -np.inf])
    idx, sc = lr.merge([a, b], [0, 0], 8)
    # NaN first, above +inf; the two zeros are equal and decided by row; -inf with a valid index before the fill, by row
    assert idx.tolist() == [[0, 5, 1, 6, 7, 2, 8, -1]]
    assert er.bits(sc)[0].tolist() == [QNAN, 0x7f800000, 0, 0, 0xbf800000, NINF, NINF, NINF]
    idx, sc = lr.merge([a, b], [0, 10], 4)                                                  # with a base the zero of row 6 comes first
    assert idx.tolist() == [[10, 5, 6, 11]] and er.bits(sc)[0].tolist() == [QNAN, 0x7f800000, 0, 0]
    assert lr.key_of(er.bits(f32(-np.inf))) == 0x007fffff and lr.key_of(np.uint32(0x80000000)) == lr.key_of(np.uint32(0)) == 0x80000000
    x = np.random.default_rng(0).standard_normal(100).astype(f32)
    assert np.array_equal(lr.bits_of(lr.key_of(er.bits(x))), er.bits(x))                    # the bits of a search pass through
    assert (np.diff(lr.key_of(er.bits(np.sort(x))).astype(np.int64)) >= 0).all()


# ---- the C entry point ----------------------------------------------------------------------------------------------------------------
def _aligned(nbytes, align=64):
    raw = np.zeros(nbytes + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + nbytes]


def _merge(sets=True, S=2, B=2, k=5, scores=True, indices=True, ld_out=8, s_off=0, i_off=0, per_set=None):
    """tfimm_hip_matches_merge over host buffers (every call is refused, or has B == 0): ``per_set`` maps a set's number to
    overrides of its fields -- scores / indices False: null, scores_off / indices_off: bytes, k, ld, base"""
    bufs = [_aligned(1 << 12) for _ in range(2 * ffi.MERGE_MAX_SETS + 2)]
    arr = (ffi.MatchSet * (ffi.MERGE_MAX_SETS + 1))()
    for s in range(ffi.MERGE_MAX_SETS):
        kw = (per_set or {}).get(s, {})
        arr[s].scores = bufs[2 * s].ctypes.data + kw.get("scores_off", 0) if kw.get("scores", True) else None
        arr[s].indices = bufs[2 * s + 1].ctypes.data + kw.get("indices_off", 0) if kw.get("indices", True) else None
        arr[s].ld, arr[s].k, arr[s].base = kw.get("ld", 8), kw.get("k", 5), kw.get("base", 0)
    out = [C.c_void_p(b.ctypes.data + o) if f else None for b, f, o in zip(bufs[-2:], (scores, indices), (s_off, i_off))]
    rc = ffi.lib.tfimm_hip_matches_merge(arr if sets else None, S, B, k, out[0], out[1], ld_out, None)
    return rc, ffi.lib.tfimm_hip_last_error().decode()


@pytest.mark.parametrize("kw, names", [
    (dict(sets=False), "sets is null"), (dict(scores=False), "scores is null"), (dict(indices=False), "indices is null"),
    (dict(per_set={1: dict(indices=False)}), "sets[1].indices is null"), (dict(per_set={0: dict(scores=False)}), "sets[0].scores is null"),
    (dict(S=8, per_set={7: dict(scores=False)}), "sets[7].scores is null"),
    (dict(s_off=2), "4-byte aligned"), (dict(i_off=1), "4-byte aligned"), (dict(s_off=2), "scores"),
    (dict(per_set={0: dict(scores_off=2)}), "sets[0].scores"), (dict(per_set={1: dict(indices_off=3)}), "sets[1].indices"),
    (dict(per_set={1: dict(indices_off=3)}), "4-byte aligned"),
    (dict(S=0), "S=0"), (dict(S=9), "S=9"), (dict(S=-1), "S=-1"), (dict(S=9), "TFIMM_MERGE_MAX_SETS = 8"),
    (dict(k=0), "k=0"), (dict(k=257, ld_out=300), "k=257"), (dict(k=257, ld_out=300), "TFIMM_EMBED_WIDE_MAX_K = 256"),
    (dict(per_set={1: dict(k=0)}), "sets[1].k=0"), (dict(per_set={0: dict(k=257, ld=300)}), "sets[0].k=257"),
    (dict(per_set={1: dict(ld=4)}), "sets[1].ld=4"), (dict(ld_out=4), "ld_out=4"),
    (dict(per_set={0: dict(base=-1)}), "sets[0].base=-1"), (dict(S=3, per_set={2: dict(base=-2 ** 31)}), "sets[2].base=-2147483648"),
    (dict(B=-1), "B=-1"), (dict(B=65535 * 32 + 1), "B=2097121"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_merge_refusals_name_the_argument(kw, names):
    rc, msg = _merge(**kw)
    assert rc == -1 and msg.startswith("matches_merge:") and names in msg, (rc, msg)


def test_the_empty_call_the_struct_and_the_constants():
    assert _merge(B=0)[0] == 0                                              # no queries: returns before any launch
    assert _merge(B=0, S=8)[0] == 0
    assert _merge(B=0, k=0)[0] == -1                                        # but not before the checks
    assert _merge(B=0, per_set={1: dict(ld=4)})[0] == -1
    assert _merge(B=0, per_set={5: dict(indices=False, k=0, base=-1)})[0] == 0     # sets behind S are not looked at
    hdr = open(os.path.join(ROOT, "include", "tfimm_hip.h")).read()
    body = re.search(r"typedef struct tfimm_match_set \{(.*?)\} tfimm_match_set;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(const float\*|const int32_t\*|int64_t|int32_t)\s+(\w+);", body, re.M)
    assert fields == [("const float*", "scores"), ("const int32_t*", "indices"), ("int64_t", "ld"), ("int32_t", "k"), ("int32_t", "base")]
    assert [name for name, _ in ffi.MatchSet._fields_] == [name for _, name in fields]
    assert C.sizeof(ffi.MatchSet) == 32
    assert [getattr(ffi.MatchSet, n).offset for n in ("scores", "indices", "ld", "k", "base")] == [0, 8, 16, 24, 28]
    assert int(re.search(r"#define TFIMM_MERGE_MAX_SETS (\d+)", hdr).group(1)) == ffi.MERGE_MAX_SETS == 8
    assert " tfimm_hip_matches_merge(" in hdr and "tfimm_hip_matches_merge" in ffi.SYMBOLS and hasattr(ffi.lib, "tfimm_hip_matches_merge")
    assert ffi.lib.tfimm_hip_abi_version() == 4                             # the change is additive
    assert int(re.search(r"#define TFIMM_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 4


# ---- signatures ------------------------------------------------------------------------------------------------------------------------
def test_signatures_of_everything_new():
    assert tfimm.merge_matches is tfimm.models.merge_matches is tfimm.models.gallery.merge_matches
    sig = inspect.signature(tfimm.merge_matches).parameters
    assert list(sig) == ["parts", "bases", "k"] and [sig[n].default for n in ("bases", "k")] == [None, None]
    sig = inspect.signature(tfimm.Gallery.search_range).parameters
    assert list(sig) == ["self", "q", "k", "start", "stop", "method"]
    assert [sig[n].default for n in list(sig)[2:]] == [5, 0, None, "auto"]
    sig = inspect.signature(tfimm.GalleryIndex.search_live).parameters
    assert list(sig) == ["self", "q", "k", "nprobe", "method"] and [sig[n].default for n in list(sig)[2:]] == [5, 8, "single"]
    sig = inspect.signature(tfimm.GalleryIndex.classify_live).parameters
    assert list(sig) == ["self", "q", "k", "nprobe", "temperature", "top", "reduce", "exclude"]
    assert [sig[n].default for n in list(sig)[2:]] == [20, 8, 0.07, 5, "sum", None]
    sig = inspect.signature(tfimm.GalleryIndex.absorb).parameters
    assert list(sig) == ["self", "assignment"] and sig["assignment"].default is None
    sig = inspect.signature(tfimm.EmbeddingModel.search_live).parameters
    assert list(sig) == ["self", "x", "index", "k", "nprobe"] and (sig["k"].default, sig["nprobe"].default) == (5, 8)
    assert isinstance(tfimm.GalleryIndex.fresh, property) and isinstance(tfimm.GalleryIndex.stale, property)


# ---- host-only behaviour (the helpers of tests/test_search_index.py) ------------------------------------------------------------------
@pytest.fixture
def hostless(monkeypatch):
    """``Gallery._store`` replaced by the bookkeeping alone (tests/test_search_wide.py): nothing is uploaded"""
    def store(self, t, up_labels, n):
        self._labelled = self._labelled or up_labels is not None
        first, self._n = self._n, self._n + n
        return range(first, self._n)
    monkeypatch.setattr(tfimm.Gallery, "_store", store)


def _gallery(n, dim=32, labels=True):
    g = tfimm.Gallery(dim)
    g.add(np.zeros((n, dim), f32), np.arange(n) % 7 if labels else None)
    return g


def _host_index(n=1000, L=10, dim=32, labels=True):
    """an index whose plumbing ran in ``torch`` on the host: the rows, the centroids and the assignment are host tensors, so
    everything up to the first launch can be looked at without a device"""
    g = _gallery(n, dim, labels)
    g._buf = torch.zeros((n, g.pitch), dtype=torch.bfloat16)
    g._buf[:, 0] = torch.arange(n) % 128                                    # exact in bf16: a row knows where it came from
    if labels:
        g._lab = (torch.arange(n) % 7).to(torch.int32)
    assignment = torch.from_numpy(((np.arange(n) * 7) % L).astype(np.int32))
    cen = tfimm.Gallery._of_rows(dim, torch.zeros((L, dim)), torch.arange(L, dtype=torch.int32))
    counts = torch.bincount(assignment.long(), minlength=L).to(torch.int32)
    clusters = tfimm.Clusters(cen, Tensor(assignment), None, Tensor(counts), None)
    return g, clusters, g.build_index(clusters=clusters)


def _grow(g, n):
    """``n`` more rows: the bookkeeping of ``add`` (hostless) and the host buffer by hand"""
    first = len(g)
    g.add(np.zeros((n, g.dim), f32), np.zeros(n, np.int64) if g.labelled else None)
    more = torch.zeros((n, g.pitch), dtype=torch.bfloat16)
    more[:, 0] = torch.arange(first, first + n) % 128
    g._buf = torch.cat([g._buf, more])


def _host_matches(B=2, k=5, idx=torch.int32, sc=torch.float32):
    return tfimm.Matches(Tensor(torch.zeros((B, k), dtype=idx)), Tensor(torch.zeros((B, k), dtype=sc)))


def test_merge_matches_value_errors_come_before_device_work():
    m = _host_matches()
    with pytest.raises(ValueError, match="merge_matches: parts: 0 Matches, must be 1 to TFIMM_MERGE_MAX_SETS = 8"):
        tfimm.merge_matches([])
    with pytest.raises(ValueError, match="merge_matches: parts: 9 Matches"):
        tfimm.merge_matches([m] * 9)
    with pytest.raises(ValueError, match="merge_matches: parts must be a sequence of Matches, got Matches"):
        tfimm.merge_matches(m)
    with pytest.raises(ValueError, match=r"merge_matches: parts\[1\] must be the Matches"):
        tfimm.merge_matches([m, 3])
    with pytest.raises(ValueError, match=r"merge_matches: parts\[1\] holds 3 queries, parts\[0\] holds B = 2"):
        tfimm.merge_matches([m, _host_matches(3)])
    with pytest.raises(ValueError, match=r"merge_matches: parts\[0\]: expected int32 indices and float32 scores"):
        tfimm.merge_matches([_host_matches(sc=torch.float64), m])
    with pytest.raises(ValueError, match=r"merge_matches: parts\[1\]: expected int32 indices"):
        tfimm.merge_matches([m, _host_matches(idx=torch.int64)])
    with pytest.raises(ValueError, match=r"merge_matches: parts\[1\]: expected .* one shape"):
        tfimm.merge_matches([m, tfimm.Matches(m.indices, _host_matches(2, 6).scores)])
    with pytest.raises(ValueError, match=r"merge_matches: parts\[0\] with k = 257"):
        tfimm.merge_matches([_host_matches(2, 257)])
    with pytest.raises(ValueError, match="merge_matches: bases: 1 offsets for 2 parts"):
        tfimm.merge_matches([m, m], [0])
    with pytest.raises(ValueError, match=r"merge_matches: bases\[1\] = -1"):
        tfimm.merge_matches([m, m], [0, -1])
    with pytest.raises(ValueError, match=r"merge_matches: bases\[0\] = 1.5"):
        tfimm.merge_matches([m, m], [1.5, 0])
    with pytest.raises(ValueError, match="merge_matches: k = 0"):
        tfimm.merge_matches([m, m], k=0)
    with pytest.raises(ValueError, match=r"merge_matches: k = 257, must be in \[1, TFIMM_EMBED_WIDE_MAX_K = 256\]"):
        tfimm.merge_matches([m, m], k=257)
    with pytest.raises(ValueError, match="merge_matches: k must be an integer"):
        tfimm.merge_matches([m, m], k=2.0)
    with pytest.raises(ValueError, match=r"merge_matches: parts\[0\] must be on the device"):       # the last check: these are host tensors
        tfimm.merge_matches([m, m], [0, 5], 7)


def test_search_range_value_errors_come_before_device_work(hostless):
    g, _, index = _host_index(1000, 10)
    q = np.zeros((2, 32), f32)
    what = "Gallery.search_range: "
    with pytest.raises(ValueError, match=what + r"k = 0, must be in \[1, TFIMM_EMBED_WIDE_MAX_K = 256\]"):
        g.search_range(q, 0)
    with pytest.raises(ValueError, match=what + "k = 257"):
        g.search_range(q, 257)
    with pytest.raises(ValueError, match=what + "k must be an integer"):
        g.search_range(q, 5.0)
    with pytest.raises(ValueError, match=what + r"rows \[-1, 1000\): 0 <= start <= stop <= len = 1000"):
        g.search_range(q, 5, -1)
    with pytest.raises(ValueError, match=what + r"rows \[0, 1001\)"):
        g.search_range(q, 5, 0, 1001)
    with pytest.raises(ValueError, match=what + r"rows \[700, 500\)"):
        g.search_range(q, 5, 700, 500)
    with pytest.raises(ValueError, match=what + "start and stop must be integers"):
        g.search_range(q, 5, 0.0)
    with pytest.raises(ValueError, match=what + "method = 'fast'"):
        g.search_range(q, 5, method="fast")
    with pytest.raises(ValueError, match=what + "method = 'fast'"):
        g.search_range(q, 5, 37, 37, method="fast")                         # an empty range checks as well
    with pytest.raises(ValueError, match=what + "k = 65 with method='list', whose limit is TFIMM_EMBED_MAX_K = 64"):
        g.search_range(q, 65, method="list")
    with pytest.raises(ValueError, match=what + "expected float32"):
        g.search_range(q.astype(np.float64))
    with pytest.raises(ValueError, match=what + r"expected shape \(n, 32\)"):
        g.search_range(np.zeros((2, 48), f32))
    wide = _host_index(1000, 100, 2048)[0]
    with pytest.raises(ValueError, match=what + "k = 65: rows of dim 2048 allow k <= 64"):
        wide.search_range(np.zeros((2, 2048), f32), 65)
    with pytest.raises(ValueError, match=what + "k = 5 with method='buffer': rows of dim 2048 allow no k"):
        wide.search_range(np.zeros((2, 2048), f32), 5, method="buffer")
    # the limits apply to min(k, rows): what the search runs for
    assert g._range_args(65, 10, 30, "list") == (10, 20, 20, "list") and g._range_args(256, 0, None, "auto") == (0, 1000, 256, "buffer")
    assert g._range_args(5, 37, 37, "auto") == (37, 0, 0, None) and wide._range_args(200, 0, 64, "auto") == (0, 64, 64, "list")
    assert not g._work and not wide._work


def test_live_value_errors_come_before_device_work(hostless):
    g, _, index = _host_index(1000, 10)
    q = np.zeros((2, 32), f32)
    for grown in (False, True):                                             # without and with fresh rows
        if grown:
            _grow(g, 100)
        assert index.fresh == (100 if grown else 0) and index.stale == grown
        for call in (index.search_live, index.classify_live):
            name = "GalleryIndex." + call.__name__
            with pytest.raises(ValueError, match=name + r": k = 0, must be in \[1"):
                call(q, 0)
            with pytest.raises(ValueError, match=name + ": k must be an integer"):
                call(q, 5.0)
            with pytest.raises(ValueError, match=name + r": nprobe = 11, must be in \[1, min\(n_lists = 10, TFIMM_EMBED_LISTS_MAX_PROBE = 256\)\]"):
                call(q, 5, 11)
            with pytest.raises(ValueError, match=name + ": nprobe must be an integer"):
                call(q, 5, 2.0)
            with pytest.raises(ValueError, match=name + ": expected float32"):
                call(q.astype(np.float64), 5, 2)
            with pytest.raises(ValueError, match=name + r": expected shape \(n, 32\)"):
                call(np.zeros((2, 48), f32), 5, 2)
        with pytest.raises(ValueError, match=r"search_live: k = 257, must be in \[1, TFIMM_EMBED_WIDE_MAX_K = 256\]"):
            index.search_live(q, 257)
        with pytest.raises(ValueError, match="search_live: method = 'auto', must be one of 'grouped', 'single'"):
            index.search_live(q, 5, 2, "auto")
        with pytest.raises(ValueError, match=r"search_live: 65536 queries, at most 65535"):
            index.search_live(np.zeros((65536, 32), f32), 5, 2)
        with pytest.raises(ValueError, match=r"classify_live: k = 65, must be in \[1, TFIMM_KNN_MAX_K = 64\]"):
            index.classify_live(q, 65)
        with pytest.raises(ValueError, match=r"classify_live: k = 64 \(\+ 1 for the excluded row\)"):
            index.classify_live(q, 64, exclude=[0, 1])
        with pytest.raises(ValueError, match="classify_live: top = 0"):
            index.classify_live(q, 5, 2, top=0)
        with pytest.raises(ValueError, match="classify_live: temperature = 0"):
            index.classify_live(q, 5, 2, temperature=0)
        with pytest.raises(ValueError, match="classify_live: reduce = 'mean'"):
            index.classify_live(q, 5, 2, reduce="mean")
    with pytest.raises(ValueError, match="classify_live: this gallery has no labels"):
        _host_index(100, 4, labels=False)[2].classify_live(q, 5, 2)
    # k must be acceptable to both halves, and the error says which one refused
    gw, _, wide = _host_index(1000, 100, 2048)
    qw = np.zeros((2, 2048), f32)
    with pytest.raises(ValueError, match=r"search_live: the index half refused: k = 5 with method='grouped': rows of dim 2048 allow no k"):
        wide.search_live(qw, 5, 8, "grouped")
    assert wide._live_args(200, 8, "single", "w") == (1, None)              # nothing fresh: the index's limits alone
    _grow(gw, 100)
    with pytest.raises(ValueError, match=r"search_live: the exact half \(the 100 fresh rows\) refused: k = 65: rows of dim 2048 allow k <= 64"):
        wide.search_live(qw, 65, 8)
    assert wide._live_args(64, 8, "single", "w") == (1, (1000, 100, 64, "list"))
    _, _, few = _host_index(1000, 100, 2048)
    _grow(few._gallery, 5)
    assert few._live_args(200, 8, "single", "w") == (1, (1000, 5, 5, "list"))        # the tail runs for min(k, fresh)
    assert index._live_args(256, 10, "grouped", "w") == (1, (1000, 100, 100, "buffer"))
    assert not index._work and not g._work and not index.centroids._work and not gw._work     # nothing was launched or allocated

    class Model:
        name, embed_dim = "m", 32

        def _embeddings_for(self, x, index):
            raise AssertionError("the forward pass ran")
    with pytest.raises(ValueError, match="m: embeddings have 32 columns, the index holds rows of 2048"):
        tfimm.EmbeddingModel.search_live(Model(), None, wide)
    with pytest.raises(ValueError, match="search_live: nprobe = 11"):
        tfimm.EmbeddingModel.search_live(Model(), None, index, 5, 11)
    with pytest.raises(ValueError, match="search_live: k = 257"):
        tfimm.EmbeddingModel.search_live(Model(), None, index, 257)


def test_absorb_value_errors_come_before_device_work(hostless):
    g, _, index = _host_index(1000, 10)
    _grow(g, 5)
    rows = index._rows
    with pytest.raises(ValueError, match="absorb: assignment: expected integers, got float64"):
        index.absorb(np.zeros(5))
    with pytest.raises(ValueError, match=r"absorb: assignment: expected shape \(5,\) -- one list per fresh row --, got \(4,\)"):
        index.absorb(np.zeros(4, np.int32))
    with pytest.raises(ValueError, match=r"absorb: assignment: expected shape \(5,\)"):
        index.absorb(torch.zeros((5, 1), dtype=torch.int64))
    with pytest.raises(ValueError, match=r"absorb: assignment: lists must be in \[0, n_lists = 10\), got values in \[0, 10\]"):
        index.absorb(np.array([0, 1, 10, 3, 4]))
    with pytest.raises(ValueError, match=r"absorb: assignment: lists must be in .* got values in \[-1, 4\]"):
        index.absorb(Tensor(torch.tensor([0, 1, -1, 3, 4], dtype=torch.int32)))
    assert index._rows is rows and index.fresh == 5 and index.size == 1000


def _same_index(a, b):
    ia, oa = a.lists()
    ib, ob = b.lists()
    assert np.array_equal(ia, ib) and np.array_equal(oa, ob) and ia.dtype == ib.dtype == np.int32
    assert torch.equal(a._rows, b._rows) and a._rows.dtype == torch.bfloat16
    assert np.array_equal(a.counts.numpy(), b.counts.numpy())
    assert (a.size, a.longest, a.parts, a.n_lists, a.stale, a.fresh) == (b.size, b.longest, b.parts, b.n_lists, False, 0)


def test_absorb_takes_the_fresh_rows_into_the_lists(hostless):
    g, clusters, index = _host_index(1000, 10)
    old = clusters.assignment.torch()
    assert torch.equal(index._assignment(), old) and index._assignment().dtype == torch.int32      # re-derived from ids / offsets
    assert index.fresh == 0 and not index.stale
    rows = index._rows
    assert index.absorb() == 0 and index.absorb(np.zeros(0, np.int64)) == 0 and index._rows is rows   # nothing fresh: nothing done
    index._work["kept"] = 1
    _grow(g, 5)
    assert index.fresh == 5 and index.stale and index.size == 1000
    first = np.array([3, 3, 0, 9, 3], np.int64)                             # a routing of the caller's choice
    assert index.absorb(first) == 5
    assert index.fresh == 0 and not index.stale and index.size == 1005 and not index._work          # the workspace cache is dropped
    both = torch.cat([old, torch.from_numpy(first).int()])
    _same_index(index, g.build_index(clusters=tfimm.Clusters(clusters.centroids, Tensor(both), None, None, None)))
    ids, offsets = index.lists()
    assert offsets.tolist() == [0, 101, 201, 301, 404, 504, 604, 704, 804, 904, 1005]
    assert ids[offsets[3]:offsets[4]][-3:].tolist() == [1000, 1001, 1004] and ids[offsets[0]:offsets[1]][-1] == 1002     # rows ascend inside a list
    assert np.array_equal(index._rows[:, 0].float().numpy(), ids % 128)     # the list-ordered copy follows
    _grow(g, 130)
    assert index.fresh == 130 and index.stale
    second = torch.full((130,), 7, dtype=torch.int32)                       # two lists share them: the longest list grows
    second[::2] = 1
    assert index.absorb(Tensor(second)) == 130
    assert index.fresh == 0 and index.size == 1135 and index.longest == 165
    every = torch.cat([both, second])
    _same_index(index, g.build_index(clusters=tfimm.Clusters(clusters.centroids, Tensor(every), None, None, None)))
    assert torch.equal(index._assignment(), every)                          # old rows keep their list
    rows = index._rows
    assert index.absorb() == 0 and index._rows is rows

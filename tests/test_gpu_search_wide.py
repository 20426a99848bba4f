"""pytest -m gpu: the gallery search for up to 256 neighbours (tfimm_hip_embed_search_wide, csrc/embed_wide.hip; DESIGN.md
3.26) against the written rule of tests/embed_ref.py: bit-equal on exact data over the shapes at which the buffers, the prunes
and the chunks meet their edges; bit-equal to the list path (tfimm_hip_embed_search) on random data; independent of batch,
chunk and replay; within the float32 band of DESIGN.md 3.18 at k = 200; and through ``EmbeddingModel.search``."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import embed_ref as er
import model_checks as mc
import test_architectures  # noqa: F401
import tfimm
from tfimm.engine import ffi
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 8          # elements behind every output buffer that a launch must leave alone


class Device:
    """queries and gallery uploaded once: q float32 [B][E + pad_q], g bf16 [N][E + pad_g], NaN in every padding column -- a
    launch that read them would show it"""

    def __init__(self, q, g, pad_q=0, pad_g=0):
        q, g = np.ascontiguousarray(q, f32), np.ascontiguousarray(g, f32)
        assert np.array_equal(er.bf16_round(g), g) and pad_g % 8 == 0
        (self.B, self.E), self.N = q.shape, g.shape[0]
        self.ld_q, self.ld_g = self.E + pad_q, self.E + pad_g
        hq = np.full((self.B, self.ld_q), np.nan, f32)
        hq[:, :self.E] = q
        hg = np.full((self.N, self.ld_g), np.nan, f32)
        hg[:, :self.E] = g
        self.q, self.g = torch.from_numpy(hq).cuda(), torch.from_numpy(hg).cuda().bfloat16()
        assert self.g.data_ptr() % 16 == 0

    def search(self, k, chunk=0, rows=None, sync=True):
        """tfimm_hip_embed_search_wide for the queries ``rows`` (a slice; default all) -> (indices, scores) as numpy arrays,
        or the device buffers if not ``sync``"""
        lo, hi = (0, self.B) if rows is None else rows
        B = hi - lo
        need = ffi.lib.tfimm_hip_embed_search_wide_workspace(B, self.N, self.E, k, chunk)
        assert need > 0, ffi.lib.tfimm_hip_last_error().decode()
        work = torch.empty(need + 4 * GUARD, dtype=torch.uint8, device="cuda")
        work[need:] = 0x5a
        scores = torch.full((B * k + GUARD,), -7.0, dtype=torch.float32, device="cuda")
        indices = torch.full((B * k + GUARD,), -7, dtype=torch.int32, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_embed_search_wide(self.q.data_ptr() + 4 * lo * self.ld_q, self.ld_q, B, self.g.data_ptr(),
                                                      self.ld_g, self.N, self.E, k, chunk, scores.data_ptr(), indices.data_ptr(),
                                                      work.data_ptr(), need, st), "tfimm_hip_embed_search_wide")
        if not sync:
            return indices, scores, work
        torch.cuda.synchronize()
        i, s = indices.cpu().numpy(), scores.cpu().numpy()
        assert (i[B * k:] == -7).all() and (s[B * k:] == -7).all() and (work[need:] == 0x5a).all(), "a launch wrote behind a buffer"
        return i[:B * k].reshape(B, k), s[:B * k].reshape(B, k)


def grid(seed, shape):
    """entries from {-4, ..., 4} / 8: exact in bf16, products multiples of 1/64, every partial sum exact in float32 for
    E <= 2048: scores are bit-equal to the rule in any summation order, and ties are plentiful"""
    return (np.random.default_rng(seed).integers(-4, 5, shape) / 8).astype(f32)


def check_exact(q, g, k, chunk=0, **pads):
    idx, sc = Device(q, g, **pads).search(k, chunk)
    want_idx, want_sc = er.search(q, g, k)
    assert np.array_equal(idx, want_idx), (idx[idx != want_idx][:8], want_idx[idx != want_idx][:8])
    assert np.array_equal(er.bits(sc), er.bits(want_sc))
    return idx, sc


# ---- exact data: a covering set -------------------------------------------------------------------------------------------------
KS, N_KINDS, BS, ES, CHUNK_KINDS = (1, 5, 64, 65, 200, 256), ("k", "k+1", 257, 5000, 40000), (1, 33, 70), (16, 48, 512, 768), \
    ("0", "4k", 4096)


def _covering():
    """every pair of values of two different axes occurs: the cases are picked greedily, in a fixed order, by the number of
    pairs each still adds"""
    axes = (KS, N_KINDS, BS, ES, CHUNK_KINDS)
    cases = list(itertools.product(*axes))
    missing = {(a, va, b, vb) for a, b in itertools.combinations(range(5), 2) for va in axes[a] for vb in axes[b]}
    out = []
    while missing:
        def gain(c):
            return sum((a, c[a], b, c[b]) in missing for a, b in itertools.combinations(range(5), 2))
        best = max(cases, key=gain)                      # the first of equal gains: deterministic
        missing -= {(a, best[a], b, best[b]) for a, b in itertools.combinations(range(5), 2)}
        out.append(best)
    return out


def _resolve(k, n_kind, chunk_kind):
    N = {"k": k, "k+1": k + 1}.get(n_kind, n_kind)
    chunk = {"0": 0, "4k": 32 * -(-4 * k // 32)}.get(chunk_kind, chunk_kind)
    return N, chunk


def test_covering_set_covers():
    c = _covering()
    assert len(c) <= 48
    for axis, values in enumerate((KS, N_KINDS, BS, ES, CHUNK_KINDS)):
        assert {x[axis] for x in c} == set(values)
    for a, b in itertools.combinations(range(5), 2):
        assert {(x[a], x[b]) for x in c} == set(itertools.product((KS, N_KINDS, BS, ES, CHUNK_KINDS)[a], (KS, N_KINDS, BS, ES, CHUNK_KINDS)[b]))


@pytest.mark.parametrize("k, n_kind, B, E, chunk_kind", _covering())
def test_wide_search_is_bit_equal_to_the_rule_on_exact_data(k, n_kind, B, E, chunk_kind):
    N, chunk = _resolve(k, n_kind, chunk_kind)
    check_exact(grid(E + N, (B, E)), grid(B + k, (N, E)), k, chunk)


def test_the_widest_rows_with_their_largest_k():
    """E = 1024: the buffers hold exactly k + 128 pairs, and LDS is full to the byte"""
    k = ffi.lib.tfimm_hip_embed_search_wide_max_k(1024)
    assert k == 254
    check_exact(grid(1, (33, 1024)), grid(2, (700, 1024)), k, 0)
    check_exact(grid(1, (33, 1024)), grid(2, (700, 1024)), k, 160)


def test_padded_rows_are_never_read():
    q, g = grid(7, (33, 48)), grid(8, (5000, 48))
    check_exact(q, g, 200, 800, pad_q=3, pad_g=8)
    check_exact(q, g, 65, 0, pad_q=1, pad_g=24)


# ---- orders that stress the buffers -------------------------------------------------------------------------------------------------
N_STRESS = 40000


def _counting_gallery():
    """row n scores exactly (n + 1) / 256 against query 0 = (1, 1/256, 0, ...), -(n + 1) / 256 against query 1 = -query 0:
    ascending for the one -- every row beats every threshold, the most prunes possible --, descending for the other -- no row
    after the first prune is accepted.  n + 1 = 256 hi + lo with hi < 157, lo < 256: integers that bf16 holds exactly."""
    n = np.arange(N_STRESS) + 1
    g = grid(30, (N_STRESS, 16))
    g[:, 0], g[:, 1] = n // 256, n % 256
    q = grid(31, (3, 16))
    q[0] = 0
    q[0, 0], q[0, 1] = 1, 1 / 256
    q[1] = -q[0]
    q[2, :2] = 0                                         # query 2 sees the random columns alone: plenty of ties
    return q, g


@pytest.mark.parametrize("k", [64, 256])
def test_ascending_and_descending_rows(k):
    q, g = _counting_gallery()
    for chunk in (0, 4096):
        idx, sc = check_exact(q, g, k, chunk)
        assert idx[0].tolist() == list(range(N_STRESS - 1, N_STRESS - 1 - k, -1)) and idx[1].tolist() == list(range(k))
        assert sc[0, 0] == N_STRESS / 256 and sc[1, 0] == -1 / 256


@pytest.mark.parametrize("k", [64, 256])
def test_equal_rows_keep_the_lowest(k):
    """all rows equal: every key is the same, so a threshold that compared keys alone would accept or refuse them all"""
    q = grid(32, (5, 48))
    for chunk in (0, 32 * -(-4 * k // 32)):
        idx, _ = check_exact(q, np.tile(grid(33, (1, 48)), (N_STRESS, 1)), k, chunk)
        assert idx.tolist() == [list(range(k))] * 5


def _liked_row(q):
    best = np.sign(q[0]).astype(f32) / 2                 # the row that query 0 likes best: score = sum |q| / 2 > 4
    assert float(er.scores64(q[:1], best[None])[0, 0]) > 4
    return best


@pytest.mark.parametrize("k", [64, 256])
def test_one_row_repeated_600_times(k):
    g = grid(34, (N_STRESS, 64)) / 4                     # |score| <= 64 * 0.125 * 0.5 = 4
    q = grid(35, (3, 64))
    q[:, 0] = 0.5
    at = np.sort(np.random.default_rng(36).choice(N_STRESS, 600, replace=False))
    g[at] = _liked_row(q)
    idx, _ = check_exact(q, g, k)
    assert idx[0].tolist() == at[:k].tolist()


@pytest.mark.parametrize("k", [64, 256])
def test_equal_rows_on_both_sides_of_a_chunk_border(k):
    g = grid(37, (N_STRESS, 64)) / 4
    q = grid(38, (3, 64))
    q[:, 0] = 0.5
    chunk = 32 * -(-4 * k // 32)                         # 256 / 1024: borders at its multiples, with chunk = 0 as well
    rows = [chunk - 1, chunk, 2 * chunk - 2, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1, 5 * chunk - 1, 7 * chunk]
    g[rows] = _liked_row(q)
    for c in (chunk, 0, 32):
        idx, _ = check_exact(q, g, k, c)
        assert idx[0, :len(rows)].tolist() == rows


@pytest.mark.parametrize("k", [64, 256])
def test_a_chunk_with_fewer_than_k_rows_and_a_last_chunk_of_one_row(k):
    q, g = grid(39, (33, 16)), grid(40, (N_STRESS + 1, 16))
    check_exact(q, g[:N_STRESS], k, 39968)               # 40000 = 39968 + 32: the last chunk holds 32 rows, empty entries behind
    # no multiple of 32 leaves one row of 40000 (39999 is odd), so this one case runs over 40001 rows: 25 chunks of 1600 and one row
    g[N_STRESS] = 0.5 * np.sign(q[0]) + (q[0] == 0) * 0.5
    idx, _ = check_exact(q, g, k, 1600)
    assert idx[0, 0] == N_STRESS


# ---- the same bits as the list path ---------------------------------------------------------------------------------------------------
_RANDOM = {}


def _random(E, B):
    """(queries, gallery rows rounded to bf16), standard normal, computed once and never changed"""
    if (E, B) not in _RANDOM:
        rng = np.random.default_rng(E)
        q = rng.standard_normal((B, E)).astype(f32)
        g = er.bf16_round(rng.standard_normal((20000, E)).astype(f32))
        q.setflags(write=False)
        g.setflags(write=False)
        _RANDOM[(E, B)] = (q, g)
    return _RANDOM[(E, B)]


@pytest.mark.parametrize("E", [64, 768])
def test_buffer_and_list_paths_give_the_same_bits(E):
    q, g = _random(E, 33)
    gallery = tfimm.Gallery(E)
    gallery.add(g.copy())
    for k in (1, 20, 64):
        a, b = gallery.search_with(q.copy(), k, method="buffer"), gallery.search_with(q.copy(), k, method="list")
        assert np.array_equal(a.indices.numpy(), b.indices.numpy()), k
        assert np.array_equal(er.bits(a.scores.numpy()), er.bits(b.scores.numpy())), k
        auto = gallery.search(q.copy(), k)
        assert np.array_equal(auto.indices.numpy(), b.indices.numpy()) and np.array_equal(er.bits(auto.scores.numpy()), er.bits(b.scores.numpy()))
    assert {key[2] for key in gallery._work} == {"buffer", "list"} and all(key[0] == 33 for key in gallery._work)
    assert ffi.lib.tfimm_hip_embed_search_workspace(33, 20000, E, 65, 0) < 0      # the list kernel keeps its limit
    assert "k=65" in ffi.lib.tfimm_hip_last_error().decode()


# ---- independence ---------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_batch_chunk_or_replay():
    k = 200
    d = Device(grid(9, (70, 48)), grid(10, (5000, 48)))
    idx, sc = d.search(k, 0)
    for b in range(70):                                                     # the same queries one at a time
        i1, s1 = d.search(k, 0, rows=(b, b + 1))
        assert np.array_equal(i1[0], idx[b]) and np.array_equal(er.bits(s1[0]), er.bits(sc[b])), b
    i2, s2 = d.search(k, 4096)
    assert np.array_equal(i2, idx) and np.array_equal(er.bits(s2), er.bits(sc))
    for _ in range(3):
        i, s = d.search(k, 0)
        assert np.array_equal(i, idx) and np.array_equal(er.bits(s), er.bits(sc))
    # a captured graph of the two launches, replayed three times
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d.search(k, 0, sync=False)                                         # one-time setup outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            indices, scores, _work = d.search(k, 0, sync=False)
    for _ in range(3):
        indices.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(indices.cpu().numpy()[:70 * k].reshape(70, k), idx)
        assert np.array_equal(er.bits(scores.cpu().numpy()[:70 * k].reshape(70, k)), er.bits(sc))


# ---- random data: scores within the float32 band ----------------------------------------------------------------------------------------
def check_band(q, g, idx, sc, k):
    """The band and the four conditions of DESIGN.md 3.18.  ``band = E * 2^-23 * sum_e |q_e g_e|`` per (query, row): E exact
    products and at most E float32 additions at up to one ulp each (the matrix unit may truncate); nothing measured enters it"""
    E = q.shape[1]
    q16 = er.bf16_round(q).astype(np.float64)
    g64 = g.astype(np.float64)
    ref = q16 @ g64.T
    band = E * 2.0 ** -23 * (np.abs(q16) @ np.abs(g64).T)
    rows = np.arange(q.shape[0])[:, None]
    own, own_band = ref[rows, idx], band[rows, idx]
    assert (np.abs(sc - own) <= own_band).all(), float((np.abs(sc - own) / own_band).max())
    assert all(len(set(r)) == k for r in idx.tolist())                      # distinct
    assert (np.diff(sc, axis=1) <= 0).all()                                 # non-increasing
    assert ((np.diff(sc, axis=1) < 0) | (np.diff(idx, axis=1) > 0)).all()   # equal scores by ascending index
    kth = -np.sort(-ref, axis=1)[:, k - 1:k]
    assert (own >= kth - 2 * band.max(1, keepdims=True)).all()             # (the widest band of the query: the displaced row is unknown)


@pytest.mark.parametrize("E", [64, 768])
def test_wide_search_on_random_data(E):
    q, g = _random(E, 33)
    idx, sc = Device(q, g).search(200)
    check_band(q, g, idx, sc, 200)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_model_search_for_a_hundred_neighbours():
    bb = tfimm.create_model("vit_test_model")
    m = tfimm.EmbeddingModel(bb, 48, normalize=True)
    m.set_weights(synthetic_weights(m, 2021))
    x = mc.make_input(m.cfg, 4)
    gallery = tfimm.Gallery(48)
    gallery.add(m(x))
    gallery.add((np.random.default_rng(3).standard_normal((300, 48)) / 7).astype(f32))
    got = m.search(x, gallery, k=100)
    want = gallery.search(m(x), 100)
    assert got.indices.shape == got.scores.shape == (4, 100)
    assert np.array_equal(got.indices.numpy(), want.indices.numpy())
    assert np.array_equal(er.bits(got.scores.numpy()), er.bits(want.scores.numpy()))
    check_band(m(x).numpy(), gallery.numpy(), got.indices.numpy(), got.scores.numpy(), 100)

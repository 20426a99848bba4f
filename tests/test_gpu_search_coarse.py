"""pytest -m gpu: the coarse-to-fine gallery search (tfimm_hip_embed_quantize_rows / tfimm_hip_embed_search_coarse,
csrc/embed_coarse.hip) against the written rule of tests/coarse_ref.py: the quantiser bit-equal to it; on
exact data, where fp8 loses nothing, the search bit-equal to the exact rule of tests/embed_ref.py over the shapes at which
buffers, prunes, chunks and candidate tiles meet their edges; on random data bit-equal to ``Gallery.search`` (what
tests/test_search_coarse.py proves from the bands); in the lossy case exactly the rule's loss; independent of batch, chunk and
replay; and through ``Gallery`` / ``EmbeddingModel``.  Every launch runs over buffers with guards and NaN padding columns."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import coarse_ref as cr
import embed_ref as er
import model_checks as mc
import test_architectures  # noqa: F401
import tfimm
from tfimm.engine import ffi
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 8          # elements behind every output buffer that a launch must leave alone
grid = cr.grid


class Device:
    """queries and gallery uploaded once: q float32 [B][E + pad_q], g bf16 [N][E + pad_g], NaN in every padding column -- a
    launch that read them would show it --, and the rows quantised on the device into codes uint8 [N][E + pad_c] and exps int8
    [N], both pre-filled with 0x5a: what the quantiser must not write stays 0x5a"""

    def __init__(self, q, g, pad_q=0, pad_g=0, pad_c=0):
        q, g = np.ascontiguousarray(q, f32), np.ascontiguousarray(g, f32)
        assert np.array_equal(er.bf16_round(g), g, equal_nan=True) and pad_g % 8 == 0 and pad_c % 16 == 0
        (self.B, self.E), self.N = q.shape, g.shape[0]
        self.ld_q, self.ld_g, self.ld_c = self.E + pad_q, self.E + pad_g, self.E + pad_c
        hq = np.full((self.B, self.ld_q), np.nan, f32)
        hq[:, :self.E] = q
        hg = np.full((self.N, self.ld_g), np.nan, f32)
        hg[:, :self.E] = g
        self.q, self.g = torch.from_numpy(hq).cuda(), torch.from_numpy(hg).cuda().bfloat16()
        self.codes = torch.full((self.N * self.ld_c + 16 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda")
        self.exps = torch.full((self.N + 4 * GUARD,), 0x5a, dtype=torch.int8, device="cuda")
        assert self.g.data_ptr() % 16 == 0 and self.codes.data_ptr() % 16 == 0 and self.exps.data_ptr() % 4 == 0
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_embed_quantize_rows(self.g.data_ptr(), self.ld_g, self.N, self.E, self.codes.data_ptr(), self.ld_c,
                                                        self.exps.data_ptr(), st), "tfimm_hip_embed_quantize_rows")

    def quantised(self):
        """(codes (N, E), exps (N,)) as numpy arrays, after checking that nothing else was written"""
        torch.cuda.synchronize()
        c, e = self.codes.cpu().numpy(), self.exps.cpu().numpy()
        rows = c[:self.N * self.ld_c].reshape(self.N, self.ld_c)
        assert (rows[:, self.E:] == 0x5a).all() and (c[self.N * self.ld_c:] == 0x5a).all() and (e[self.N:] == 0x5a).all(), \
            "the quantiser wrote behind a row or a buffer"
        return rows[:, :self.E], e[:self.N]

    def search(self, k, c, chunk=0, rows=None, sync=True):
        """tfimm_hip_embed_search_coarse for the queries ``rows`` (a slice; default all) -> (indices, scores) as numpy arrays,
        or the device buffers if not ``sync``"""
        lo, hi = (0, self.B) if rows is None else rows
        B = hi - lo
        need = ffi.lib.tfimm_hip_embed_search_coarse_workspace(B, self.N, self.E, k, c, chunk)
        assert need > 0, ffi.lib.tfimm_hip_last_error().decode()
        work = torch.empty(need + 4 * GUARD, dtype=torch.uint8, device="cuda")
        work[need:] = 0x5a
        scores = torch.full((B * k + GUARD,), -7.0, dtype=torch.float32, device="cuda")
        indices = torch.full((B * k + GUARD,), -7, dtype=torch.int32, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_embed_search_coarse(self.q.data_ptr() + 4 * lo * self.ld_q, self.ld_q, B, self.g.data_ptr(),
                                                        self.ld_g, self.codes.data_ptr(), self.ld_c, self.exps.data_ptr(), self.N,
                                                        self.E, k, c, chunk, scores.data_ptr(), indices.data_ptr(), work.data_ptr(),
                                                        need, st), "tfimm_hip_embed_search_coarse")
        if not sync:
            return indices, scores, work
        torch.cuda.synchronize()
        i, s = indices.cpu().numpy(), scores.cpu().numpy()
        assert (i[B * k:] == -7).all() and (s[B * k:] == -7).all() and (work[need:] == 0x5a).all(), "a launch wrote behind a buffer"
        return i[:B * k].reshape(B, k), s[:B * k].reshape(B, k)

    def exact(self, k):
        """tfimm_hip_embed_search_wide over the same buffers -> (indices, scores)"""
        need = ffi.lib.tfimm_hip_embed_search_wide_workspace(self.B, self.N, self.E, k, 0)
        work = torch.empty(need, dtype=torch.uint8, device="cuda")
        scores = torch.empty((self.B, k), dtype=torch.float32, device="cuda")
        indices = torch.empty((self.B, k), dtype=torch.int32, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_embed_search_wide(self.q.data_ptr(), self.ld_q, self.B, self.g.data_ptr(), self.ld_g, self.N,
                                                      self.E, k, 0, scores.data_ptr(), indices.data_ptr(), work.data_ptr(), need, st),
                  "tfimm_hip_embed_search_wide")
        torch.cuda.synchronize()
        return indices.cpu().numpy(), scores.cpu().numpy()


# ---- the quantiser ---------------------------------------------------------------------------------------------------------------------
def _quantiser_rows(N, E, seed):
    """grid rows, normal rows over many magnitudes, a zero row, rows whose amax is exactly 448 * 2^j, bf16 subnormals"""
    rng = np.random.default_rng(seed)
    g = er.bf16_round((rng.standard_normal((N, E)) * np.exp2(rng.integers(-30, 30, (N, 1)))).astype(f32))
    g[::3] = grid(seed + 1, g[::3].shape)
    if N > 4:
        g[1] = 0
        g[2, 5] = -0.0
        for j, row in zip((0, -7, 9, 100, -110), range(4, N, 7)):
            g[row] = er.bf16_round((rng.uniform(-1, 1, E) * 448).astype(f32)) * f32(2.0) ** j
            g[row, rng.integers(E)] = f32(448) * f32(2.0) ** j * (-1) ** row
        sub = (rng.integers(0, 128, (len(g[3::11]), E)).astype(np.uint32) << 16).view(f32)     # bf16 subnormals: exponent field 0
        g[3::11] = sub * (-1) ** rng.integers(0, 2, sub.shape)
    return g


@pytest.mark.parametrize("E", [16, 48, 512, 2048])
@pytest.mark.parametrize("N", [1, 33, 5000])
def test_quantiser_is_bit_equal_to_the_rule(N, E):
    if N == 5000 and E == 2048:
        N = 1500                                              # the same paths; the reference is the slow part
    g = _quantiser_rows(N, E, 100 * N + E)
    for pads in (dict(), dict(pad_g=8, pad_c=16), dict(pad_g=24, pad_c=48)):
        codes, exps = Device(np.zeros((1, E), f32), g, **pads).quantised()
        want_codes, want_exps = cr.quantize_rows(g)
        assert np.array_equal(exps, want_exps), (exps[exps != want_exps][:8], want_exps[exps != want_exps][:8])
        assert np.array_equal(codes, want_codes), np.argwhere(codes != want_codes)[:8]
    if N > 4:
        assert exps[1] == 0 and not codes[1].any() and (np.abs(g).max(1) < 2.0 ** -126).any() and (codes == 0x7e).any()


# ---- exact data: a covering set -------------------------------------------------------------------------------------------------------
KS, C_KINDS, N_KINDS, BS, ES, CHUNK_KINDS = (1, 5, 64), ("k", "4k", 256), ("c", "c+1", 257, 5000, 40000), (1, 33, 70), \
    (16, 48, 512, 768), ("0", "4c", 4096)
AXES = (KS, C_KINDS, N_KINDS, BS, ES, CHUNK_KINDS)


def _covering():
    """every pair of values of two different axes occurs: the cases are picked greedily, in a fixed order, by the number of
    pairs each still adds"""
    pairs = list(itertools.combinations(range(len(AXES)), 2))
    cases = list(itertools.product(*AXES))
    missing = {(a, va, b, vb) for a, b in pairs for va in AXES[a] for vb in AXES[b]}
    out = []
    while missing:
        def gain(c):
            return sum((a, c[a], b, c[b]) in missing for a, b in pairs)
        best = max(cases, key=gain)                      # the first of equal gains: deterministic
        missing -= {(a, best[a], b, best[b]) for a, b in pairs}
        out.append(best)
    return out


def _resolve(k, c_kind, n_kind, chunk_kind):
    c = {"k": k, "4k": 4 * k}.get(c_kind, c_kind)
    N = {"c": c, "c+1": c + 1}.get(n_kind, n_kind)
    chunk = {"0": 0, "4c": 32 * -(-4 * c // 32)}.get(chunk_kind, chunk_kind)
    return c, N, chunk


def test_covering_set_covers():
    cases = _covering()
    assert len(cases) <= 40
    for a, b in itertools.combinations(range(len(AXES)), 2):
        assert {(x[a], x[b]) for x in cases} == set(itertools.product(AXES[a], AXES[b]))


def check_exact(q, g, k, c, chunk=0, **pads):
    idx, sc = Device(q, g, **pads).search(k, c, chunk)
    want_idx, want_sc = er.search(q, g, k)
    assert np.array_equal(idx, want_idx), (idx[idx != want_idx][:8], want_idx[idx != want_idx][:8])
    assert np.array_equal(er.bits(sc), er.bits(want_sc))
    return idx, sc


@pytest.mark.parametrize("k, c_kind, n_kind, B, E, chunk_kind", _covering())
def test_coarse_search_is_bit_equal_to_the_exact_rule_on_exact_data(k, c_kind, n_kind, B, E, chunk_kind):
    c, N, chunk = _resolve(k, c_kind, n_kind, chunk_kind)
    check_exact(grid(E + N, (B, E)), grid(B + k, (N, E)), k, c, chunk)


def test_every_k_up_to_the_candidates():
    d = Device(grid(1, (5, 48)), grid(2, (700, 48)))
    want_idx, want_sc = er.search(grid(1, (5, 48)), grid(2, (700, 48)), 40)
    for k in range(1, 41):
        idx, sc = d.search(k, 40)
        assert np.array_equal(idx, want_idx[:, :k]) and np.array_equal(er.bits(sc), er.bits(want_sc[:, :k])), k


def test_the_widest_rows_with_their_most_candidates():
    """E = 2048: the buffers hold exactly candidates + 128 pairs, and LDS is full to the byte"""
    c = ffi.lib.tfimm_hip_embed_search_coarse_max_candidates(2048)
    assert c == 254
    q, g = grid(1, (33, 2048)), grid(2, (700, 2048))
    check_exact(q, g, 64, c, 0)
    check_exact(q, g, c, c, 512)


def test_padded_rows_are_never_read():
    q, g = grid(7, (33, 48)), grid(8, (5000, 48))
    check_exact(q, g, 64, 200, 800, pad_q=3, pad_g=8, pad_c=16)
    check_exact(q, g, 5, 20, 0, pad_q=1, pad_g=24, pad_c=48)


def test_ascending_keys_force_a_prune_on_every_other_step():
    """Row n is (8 + n % 8) * 2^(n // 8 - 60) in column 0 and zero elsewhere: every row quantises exactly, so for the query +e0
    the coarse keys rise strictly with the row -- every row of the scan beats the threshold, each step fills 128 slots of every
    buffer, and a prune is due on every other step -- and for -e0 they fall strictly: nothing is appended after the first
    prune.  The result is the rule's, and the rule's is known: the last rows downwards, the first rows upwards."""
    N, E = 896, 16
    n = np.arange(N)
    g = np.zeros((N, E), f32)
    g[:, 0] = np.ldexp((8 + n % 8).astype(f32), n // 8 - 60)
    q = np.zeros((2, E), f32)
    q[0, 0], q[1, 0] = 1, -1
    codes, exps = cr.quantize_rows(g)
    assert (int(exps.min()), int(exps.max())) == (-65, 47)
    assert np.array_equal(np.ldexp(cr.e4m3_decode(codes), exps.astype(np.int64)[:, None]), g.astype(np.float64))
    keys = cr.keys64(q, g)[0]
    assert (np.diff(keys[0]) > 0).all() and (np.diff(keys[1]) < 0).all()
    d = Device(q, g)
    for c, k in ((64, 64), (256, 256), (256, 5)):
        want_idx, want_sc, _ = cr.search_coarse(q, g, k, c)
        assert want_idx.tolist() == [list(range(N - 1, N - 1 - k, -1)), list(range(k))]
        for chunk in (896, 0):
            idx, sc = d.search(k, c, chunk)
            assert np.array_equal(idx, want_idx), (c, k, chunk, idx[idx != want_idx][:8], want_idx[idx != want_idx][:8])
            assert np.array_equal(er.bits(sc), er.bits(want_sc)), (c, k, chunk)


N_STRESS = 40000


@pytest.mark.parametrize("k, c", [(5, 20), (64, 256)])
def test_equal_rows_keep_the_lowest(k, c):
    """all rows equal: every key and every score is the same, so only the row decides, in the scan and in the rerank"""
    q = grid(32, (5, 48))
    for chunk in (0, 32 * -(-4 * c // 32)):
        idx, _ = check_exact(q, np.tile(grid(33, (1, 48)), (N_STRESS, 1)), k, c, chunk)
        assert idx.tolist() == [list(range(k))] * 5


@pytest.mark.parametrize("k, c", [(5, 20), (64, 256)])
def test_equal_rows_on_both_sides_of_a_chunk_border(k, c):
    g = grid(37, (N_STRESS, 64)) / 4                     # |score| <= 64 * 0.125 * 0.5 = 4
    q = grid(38, (3, 64))
    q[:, 0] = 0.5
    best = np.sign(q[0]).astype(f32) / 2                 # the row that query 0 likes best: score = sum |q| / 2 > 4
    assert float(er.scores64(q[:1], best[None])[0, 0]) > 4
    chunk = 32 * -(-4 * c // 32)
    rows = [chunk - 1, chunk, 2 * chunk - 2, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1, 5 * chunk - 1, 7 * chunk][:k]
    g[rows] = best
    for ch in (chunk, 0, 32):
        idx, _ = check_exact(q, g, k, c, ch)
        assert idx[0, :len(rows)].tolist() == rows


# ---- random data: the bits of the exact search -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [64, 768])
def test_random_data_gives_the_bits_of_the_exact_search(E):
    """tests/test_search_coarse.py proves from the bands that every exact top-k row is a candidate here"""
    q, g = cr.random_case(E)
    gallery = tfimm.Gallery(E)
    gallery.add(g.copy())
    gallery.build_coarse()
    for k, c in cr.RANDOM_PAIRS:
        got, want = gallery.search_coarse(q.copy(), k, candidates=c), gallery.search(q.copy(), k)
        assert np.array_equal(got.indices.numpy(), want.indices.numpy()), (k, c)
        assert np.array_equal(er.bits(got.scores.numpy()), er.bits(want.scores.numpy())), (k, c)
    assert set(gallery._work_coarse) == {(33, k, c) for k, c in cr.RANDOM_PAIRS}


# ---- the lossy case ------------------------------------------------------------------------------------------------------------------------
def test_the_lossy_case_loses_what_the_rule_loses():
    seed, E, centres, noise, N, B, k, c = cr.LOSSY
    q, g = cr.clustered(seed, E, centres, noise, N, B)
    _, missed, sure, top, cand = cr.margins(q, g, k, c)
    d = Device(q, g)
    idx, sc = d.search(k, c)
    all_idx, all_sc = d.exact(N)                                            # N = 256: the exact score of every row
    table = np.empty((B, N), np.uint32)
    np.put_along_axis(table, all_idx.astype(np.int64), er.bits(all_sc), 1)
    # the scores are the exact search's for the same rows, bit for bit; the order is strict by (score, row)
    assert np.array_equal(er.bits(sc), np.take_along_axis(table, idx.astype(np.int64), 1))
    assert ((np.diff(sc, axis=1) < 0) | ((np.diff(sc, axis=1) == 0) & (np.diff(idx, axis=1) > 0))).all()
    # where the candidate set is sure, the result is the exact top k of it
    value = table.view(f32)
    for b in np.flatnonzero(sure):
        want = sorted(cand[b].tolist(), key=lambda n: (-value[b, n], n))[:k]
        assert idx[b].tolist() == want, b
    # and the rows that are surely outside are absent: the exact search would have returned them
    assert (missed.any(1) & sure).sum() == 29
    for b in np.flatnonzero(missed.any(1)):
        assert not set(top[b][missed[b]].tolist()) & set(idx[b].tolist()), b
    assert (idx != all_idx[:, :k]).any(1).sum() >= 30


# ---- independence ----------------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_batch_chunk_or_replay():
    k, c = 20, 80
    d = Device(grid(9, (70, 48)), grid(10, (5000, 48)))
    idx, sc = d.search(k, c, 0)
    for b in range(70):                                                     # the same queries one at a time
        i1, s1 = d.search(k, c, 0, rows=(b, b + 1))
        assert np.array_equal(i1[0], idx[b]) and np.array_equal(er.bits(s1[0]), er.bits(sc[b])), b
    for chunk in (320, 4096):
        i2, s2 = d.search(k, c, chunk)
        assert np.array_equal(i2, idx) and np.array_equal(er.bits(s2), er.bits(sc))
    for _ in range(3):
        i, s = d.search(k, c, 0)
        assert np.array_equal(i, idx) and np.array_equal(er.bits(s), er.bits(sc))
    # a captured graph of the three launches, replayed three times
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d.search(k, c, 0, sync=False)                                      # one-time setup outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            indices, scores, _work = d.search(k, c, 0, sync=False)
    for _ in range(3):
        indices.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(indices.cpu().numpy()[:70 * k].reshape(70, k), idx)
        assert np.array_equal(er.bits(scores.cpu().numpy()[:70 * k].reshape(70, k)), er.bits(sc))


def test_random_data_does_not_depend_on_batch_or_chunk():
    q, g = cr.random_case(64)
    d = Device(q, g[:5000])
    idx, sc = d.search(20, 80)
    i2, s2 = d.search(20, 80, 512)
    assert np.array_equal(i2, idx) and np.array_equal(er.bits(s2), er.bits(sc))
    for b in (0, 17, 32):
        i1, s1 = d.search(20, 80, 0, rows=(b, b + 1))
        assert np.array_equal(i1[0], idx[b]) and np.array_equal(er.bits(s1[0]), er.bits(sc[b])), b


# ---- the gallery's life cycle ------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(a.indices.numpy(), b.indices.numpy()) and np.array_equal(er.bits(a.scores.numpy()), er.bits(b.scores.numpy()))


def test_gallery_life_cycle():
    rows, q = grid(50, (700, 48)), grid(51, (9, 48))
    labels = np.arange(700) % 11
    gallery = tfimm.Gallery(48, capacity=300)
    gallery.add(rows[:300], labels[:300])
    before = gallery.search(q, 20)
    assert gallery.coarse is False
    gallery.build_coarse()
    assert gallery.coarse is True and _same(gallery.search(q, 20), before)            # search is untouched by the copy
    want = er.search(q, rows[:300], 20)
    got = gallery.search_coarse(q, 20)
    assert np.array_equal(got.indices.numpy(), want[0]) and np.array_equal(er.bits(got.scores.numpy()), er.bits(want[1]))
    gallery.build_coarse()                                                            # again: a rebuild
    assert _same(gallery.search_coarse(q, 20), got)
    gallery.add(rows[300:], labels[300:])                                             # a regrow: codes and exponents move with the rows
    assert gallery.capacity >= 700 and gallery._codes.shape[0] == gallery.capacity == gallery._exps.shape[0]
    codes, exps = cr.quantize_rows(rows)
    assert np.array_equal(gallery._codes[:700].cpu().numpy(), codes) and np.array_equal(gallery._exps[:700].cpu().numpy(), exps)
    want = er.search(q, rows, 20)
    got = gallery.search_coarse(q, 20, candidates=64, chunk=128)
    assert np.array_equal(got.indices.numpy(), want[0]) and np.array_equal(er.bits(got.scores.numpy()), er.bits(want[1]))
    assert _same(gallery.search(q, 20), got)
    # vote takes the matches as it takes those of search
    a, b = gallery.vote(got), gallery.vote(gallery.search(q, 20))
    for x, y in zip(a, b):
        assert np.array_equal(x.numpy().view(np.uint32), y.numpy().view(np.uint32))
    # a gallery that starts empty with a coarse copy quantises from its first add on
    late = tfimm.Gallery(48)
    late.build_coarse()
    late.add(rows)
    assert _same(late.search_coarse(q, 20, candidates=64), got)
    assert gallery.prototypes(11).coarse is False


def test_model_search_coarse():
    bb = tfimm.create_model("vit_test_model")
    m = tfimm.EmbeddingModel(bb, 48, normalize=True)
    m.set_weights(synthetic_weights(m, 2021))
    x = mc.make_input(m.cfg, 4)
    gallery = tfimm.Gallery(48)
    gallery.add(m(x))
    gallery.add((np.random.default_rng(3).standard_normal((300, 48)) / 7).astype(f32))
    with pytest.raises(ValueError, match="build_coarse"):
        m.search_coarse(x, gallery)
    gallery.build_coarse()
    got = m.search_coarse(x, gallery, k=10, candidates=40)
    want = gallery.search_coarse(m(x), 10, candidates=40)
    assert got.indices.shape == got.scores.shape == (4, 10) and _same(got, want)
    assert got.indices.numpy()[:, 0].tolist() == [0, 1, 2, 3]                         # every image finds itself

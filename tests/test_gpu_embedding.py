"""pytest -m gpu: the embedding end on the device.  tfimm_hip_embed_search and tfimm_hip_l2_normalize
(csrc/embed.hip) against the written rules of tests/embed_ref.py, ``tfimm.EmbeddingModel`` against the oracle's features
through the float64 head, and model -> ``tfimm.Gallery`` -> search end to end."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import embed_ref as er
import model_checks as mc
import oracle
import test_architectures  # noqa: F401
import tfimm
from tfimm.engine import ffi, precision
from tfimm.utils.init import synthetic_weights

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 8          # elements behind every output buffer that a launch must leave alone


# ---- op level: the search ---------------------------------------------------------------------------------------------------
class Device:
    """queries and gallery uploaded once: q float32 [B][E + pad_q], g bf16 [N][E + pad_g], NaN in every padding column --
    a launch that read them would show it"""

    def __init__(self, q, g, pad_q=0, pad_g=0):
        q, g = np.ascontiguousarray(q, f32), np.ascontiguousarray(g, f32)
        assert np.array_equal(er.bf16_round(g), g, equal_nan=True) and pad_g % 8 == 0
        (self.B, self.E), self.N = q.shape, g.shape[0]
        self.ld_q, self.ld_g = self.E + pad_q, self.E + pad_g
        hq = np.full((self.B, self.ld_q), np.nan, f32)
        hq[:, :self.E] = q
        hg = np.full((self.N, self.ld_g), np.nan, f32)
        hg[:, :self.E] = g
        self.q, self.g = torch.from_numpy(hq).cuda(), torch.from_numpy(hg).cuda().bfloat16()
        assert self.g.data_ptr() % 16 == 0

    def search(self, k, chunk=0, rows=None, sync=True):
        """tfimm_hip_embed_search for the queries ``rows`` (a slice; default all) -> (indices, scores) as numpy arrays, or
        the device buffers if not ``sync``"""
        lo, hi = (0, self.B) if rows is None else rows
        B = hi - lo
        need = ffi.lib.tfimm_hip_embed_search_workspace(B, self.N, self.E, k, chunk)
        assert need > 0, ffi.lib.tfimm_hip_last_error().decode()
        work = torch.empty(need + 4 * GUARD, dtype=torch.uint8, device="cuda")
        work[need:] = 0x5a
        scores = torch.full((B * k + GUARD,), -7.0, dtype=torch.float32, device="cuda")
        indices = torch.full((B * k + GUARD,), -7, dtype=torch.int32, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ffi.check(ffi.lib.tfimm_hip_embed_search(self.q.data_ptr() + 4 * lo * self.ld_q, self.ld_q, B, self.g.data_ptr(), self.ld_g,
                                                 self.N, self.E, k, chunk, scores.data_ptr(), indices.data_ptr(), work.data_ptr(),
                                                 need, st), "tfimm_hip_embed_search")
        if not sync:
            return indices, scores, work
        torch.cuda.synchronize()
        i, s = indices.cpu().numpy(), scores.cpu().numpy()
        assert (i[B * k:] == -7).all() and (s[B * k:] == -7).all() and (work[need:] == 0x5a).all(), "a launch wrote behind a buffer"
        return i[:B * k].reshape(B, k), s[:B * k].reshape(B, k)


def grid(seed, shape):
    """entries from {-4, ..., 4} / 8: exact in bf16, products multiples of 1/64, every partial sum exact in float32 for
    E <= 2048 (|sum| <= 512 = 2^15 / 64): scores are bit-equal to the rule in any summation order, and ties are plentiful"""
    return (np.random.default_rng(seed).integers(-4, 5, shape) / 8).astype(f32)


def check_exact(q, g, k, chunk=0, **pads):
    idx, sc = Device(q, g, **pads).search(k, chunk)
    want_idx, want_sc = er.search(q, g, k)
    assert np.array_equal(idx, want_idx), (idx[idx != want_idx][:8], want_idx[idx != want_idx][:8])
    assert np.array_equal(er.bits(sc), er.bits(want_sc))
    return idx, sc


def _covering():
    """40 of the 720 combinations: i runs over the residues of 3, 5 and 4 at once, so every pair of (E, N, B) values occurs;
    k and chunk cycle at other rates; k is cut to the largest listed value that N allows"""
    Es, Ns, Bs, ks, cs = (16, 48, 512), (1, 31, 33, 129, 5000), (1, 31, 33, 70), (1, 5, 64), (0, 32, 160, 4096)
    out = []
    for i in range(40):
        N = Ns[i % 5]
        k = max(v for v in ks[:(i // 2) % 3 + 1] if v <= N)
        out.append((Es[i % 3], N, Bs[i % 4], k, cs[(i + i // 4) % 4]))
    return out


@pytest.mark.parametrize("E, N, B, k, chunk", _covering())
def test_search_is_bit_equal_to_the_rule_on_exact_data(E, N, B, k, chunk):
    check_exact(grid(E + N, (B, E)), grid(B + k, (N, E)), k, chunk)


def test_covering_set_covers():
    c = _covering()
    for axis, values in enumerate([(16, 48, 512), (1, 31, 33, 129, 5000), (1, 31, 33, 70), (1, 5, 64), (0, 32, 160, 4096)]):
        assert {x[axis] for x in c} == set(values), axis
    assert {(x[0], x[1]) for x in c} == {(e, n) for e in (16, 48, 512) for n in (1, 31, 33, 129, 5000)}
    assert {(x[1], x[2]) for x in c} == {(n, b) for n in (1, 31, 33, 129, 5000) for b in (1, 31, 33, 70)}
    assert any(x[1] == 5000 and x[3] == 64 and x[4] == 32 for x in c)      # the most chunks with the longest lists


@pytest.mark.parametrize("E, k", [(2048, 64), (2048, 5), (1536, 64), (1024, 64)])
def test_search_at_the_limits_of_e_and_k(E, k):
    """the largest query tile next to the longest lists: the shapes at which fewer waves keep lists"""
    check_exact(grid(1, (33, E)), grid(2, (700, E)), k, 160)


def test_one_row_repeated_gives_the_first_rows():
    q = grid(3, (5, 48))
    for k in (1, 5, 64):
        idx, _ = check_exact(q, np.tile(grid(4, (1, 48)), (300, 1)), k, chunk=32)
        assert idx.tolist() == [list(range(k))] * 5


def test_duplicated_rows_on_either_side_of_a_chunk_border():
    g = grid(5, (256, 64)) / 4                       # |score| <= 64 * 0.125 * 0.5 = 4
    q = grid(6, (3, 64))
    q[:, 0] = 0.5
    best = np.sign(q[0]).astype(f32) / 2             # the row that query 0 likes best: score = sum |q| / 2
    assert float(er.scores64(q[:1], best[None])[0, 0]) > 4
    for rows in ([31, 32], [63, 64, 65], [30, 33, 95, 96, 160]):       # chunk = 32: borders at 32, 64, 96, ...
        h = g.copy()
        h[rows] = best
        idx, _ = check_exact(q, h, 6, chunk=32)
        assert idx[0, :len(rows)].tolist() == rows
        check_exact(q, h, 6, chunk=64)


def test_padded_rows_are_never_read():
    q, g = grid(7, (33, 48)), grid(8, (129, 48))
    check_exact(q, g, 5, 32, pad_q=3, pad_g=8)
    check_exact(q, g, 5, 0, pad_q=1, pad_g=24)


# ---- independence -----------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_batch_chunk_or_replay():
    d = Device(grid(9, (70, 48)), grid(10, (5000, 48)))
    idx, sc = d.search(5, 0)
    for b in range(70):                                                     # the same queries one at a time
        i1, s1 = d.search(5, 0, rows=(b, b + 1))
        assert np.array_equal(i1[0], idx[b]) and np.array_equal(er.bits(s1[0]), er.bits(sc[b])), b
    i32, s32 = d.search(5, 32)
    assert np.array_equal(i32, idx) and np.array_equal(er.bits(s32), er.bits(sc))
    for _ in range(3):
        i, s = d.search(5, 0)
        assert np.array_equal(i, idx) and np.array_equal(er.bits(s), er.bits(sc))
    # a captured graph of the two launches, replayed three times
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d.search(5, 0, sync=False)                                         # one-time setup outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            indices, scores, _work = d.search(5, 0, sync=False)
    for _ in range(3):
        indices.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(indices.cpu().numpy()[:350].reshape(70, 5), idx)
        assert np.array_equal(er.bits(scores.cpu().numpy()[:350].reshape(70, 5)), er.bits(sc))


# ---- random data: scores within the float32 band -----------------------------------------------------------------------------
def check_band(q, g, idx, sc, k):
    """``band = E * 2^-23 * sum_e |q_e g_e|`` per (query, row): E exact products and at most E float32 additions at up to one
    ulp each (the matrix unit may truncate); nothing measured enters it"""
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
def test_search_on_random_data(E):
    rng = np.random.default_rng(E)
    q = rng.standard_normal((40, E)).astype(f32)
    g = er.bf16_round(rng.standard_normal((20000, E)).astype(f32))
    idx, sc = Device(q, g).search(10)
    check_band(q, g, idx, sc, 10)


def test_non_finite_inputs_do_not_fault():
    q, g = grid(11, (3, 32)), grid(12, (200, 32))
    q[1, 3], q[2, 5] = np.inf, np.nan
    g[7, 3], g[9, 0] = -np.inf, np.nan
    idx, _ = Device(q, g).search(5, 32)                                     # the rule says nothing about such scores
    assert ((idx >= 0) & (idx < 200)).all()


# ---- op level: normalise ------------------------------------------------------------------------------------------------------
def normalize(x, pad=0):
    B, E = x.shape
    host = np.full((B, E + pad), np.nan, f32)
    host[:, :E] = x
    dx = torch.from_numpy(host).cuda()
    dy = torch.full((B * (E + pad) + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ffi.check(ffi.lib.tfimm_hip_l2_normalize(dx.data_ptr(), E + pad, B, E, dy.data_ptr(), E + pad, st), "tfimm_hip_l2_normalize")
    torch.cuda.synchronize()
    y = dy.cpu().numpy()
    assert (y[B * (E + pad):] == -7).all()
    y = y[:B * (E + pad)].reshape(B, E + pad)
    assert (y[:, E:] == -7).all()
    return y[:, :E]


@pytest.mark.parametrize("E", [1, 63, 64, 65, 512, 2048])
def test_normalize_against_float64(E):
    """relative error per element <= (ceil(E / 64) + 10) * 2^-24: the longest addition chain of the positive sum is
    ceil(E / 64) + 6 half-ulps, the square root halves its relative error; one half-ulp each for the square, the root, the
    division and the product, plus slack"""
    rng = np.random.default_rng(E)
    norms = 10.0 ** rng.uniform(-3, 3, (9, 1))
    x = rng.standard_normal((9, E))
    x = (x / np.sqrt((x * x).sum(-1, keepdims=True)) * norms).astype(f32)
    x[4] = 0.0
    x = x[:, :E]
    y = normalize(x, pad=3)
    ref = er.l2_normalize(x)
    ok = ref != 0
    rel = np.abs(y[ok] - ref[ok]) / np.abs(ref[ok])
    bar = (math.ceil(E / 64) + 10) * 2.0 ** -24
    print(f"E={E}: max rel {rel.max():.3e} bar {bar:.3e}")
    assert rel.max() <= bar
    assert not y[4].any() and not np.signbit(y[4]).any()                    # an all-zero row gives zeros
    for b in (0, 4, 8):                                                     # independent of B
        assert np.array_equal(er.bits(normalize(x[b:b + 1])), er.bits(y[b:b + 1]))


def test_normalize_in_place_gives_the_same_bits():
    """the header allows y == x: every lane has read its columns (the sum needs them) before any is written"""
    x = np.random.default_rng(2).standard_normal((7, 200)).astype(f32)
    want = normalize(x)
    d = torch.from_numpy(x).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ffi.check(ffi.lib.tfimm_hip_l2_normalize(d.data_ptr(), 200, 7, 200, d.data_ptr(), 200, st), "tfimm_hip_l2_normalize")
    torch.cuda.synchronize()
    assert np.array_equal(er.bits(d.cpu().numpy()), er.bits(want))


def test_gallery_uploads_host_tensors_and_a_map_cannot_be_searched():
    g = tfimm.Gallery(32)
    rows = grid(20, (40, 32))
    assert g.add(torch.from_numpy(rows[:10])) == range(0, 10)              # a torch tensor on the CPU: uploaded, as arrays are
    assert g.add(rows[10:]) == range(10, 40) and g._buf.is_cuda and np.array_equal(g.numpy(), rows)
    m = g.search(torch.from_numpy(rows[:3]), 4)
    want_idx, want_sc = er.search(rows[:3], rows, 4)
    assert m.indices.torch().is_cuda and np.array_equal(m.indices.numpy(), want_idx)
    assert np.array_equal(er.bits(m.scores.numpy()), er.bits(want_sc))
    model = _embedding_model("resnet50_mini_test_model")                    # features are a map: (B, 2, 2, EMBED)
    gal = tfimm.Gallery(EMBED)
    gal.add(grid(21, (4, EMBED)))
    with pytest.raises(ValueError, match="map"):
        model.search(mc.make_input(model.cfg, 2), gal, 2)


# ---- the model ----------------------------------------------------------------------------------------------------------------
FAMILIES = ["resnet50_mini_test_model", "vit_test_model", "swin_test_model", "efficientnet_test_model", "convnext_test_model",
            "cait_test_model"]
TOL_FP32 = 1e-3
EMBED = 48


def _embedding_model(name, normalize=False, seed=2021):
    bb = tfimm.create_model(name)
    m = tfimm.EmbeddingModel(bb, EMBED, normalize=normalize)
    m.set_weights(synthetic_weights(m, seed))
    return m


_REF = {}


def _reference(name, batch):
    """(input, weights, oracle features through the float64 head): computed once per (model, batch), never changed"""
    if (name, batch) not in _REF:
        m = _embedding_model(name)
        w = dict(m.weights)
        x = mc.make_input(m.cfg, batch)
        _, feats = oracle.forward(m.cfg, {k: v for k, v in w.items() if not k.startswith("emb/")}, x, return_features=True)
        ref = er.head(feats["features"], w)
        ref.setflags(write=False)
        _REF[(name, batch)] = (x, w, ref, list(feats))
    return _REF[(name, batch)]


@pytest.mark.parametrize("batch", [2, 3])
@pytest.mark.parametrize("name", FAMILIES)
def test_embeddings_against_the_oracle_features_through_the_float64_head(name, batch):
    x, w, ref, oracle_names = _reference(name, batch)
    m = _embedding_model(name)
    emb = m(x)
    assert emb.torch().dtype == torch.float32 and emb.shape[0] == batch and emb.shape[-1] == EMBED
    assert emb.numpy().size == ref.size
    if name != "resnet50_mini_test_model":
        assert emb.shape == (batch, EMBED)
    err = mc.rel_err(emb.numpy().reshape(ref.shape), ref)
    print(f"{name} B={batch}: embeddings rel-to-max {err:.3e}")
    assert err <= mc.TOL_LOGITS
    # three consecutive calls (eager, then replays): the same bits
    again = [m(x).numpy() for _ in range(3)]
    assert all(np.array_equal(er.bits(a), er.bits(emb.numpy())) for a in again) and m._captured
    # the features dictionary: the backbone's keys up to `features`, then `embeddings`; `features` bit-equal to the backbone's
    got, feats = m(x, return_features=True)
    assert list(feats) == m.feature_names and list(feats)[-2:] == ["features", "embeddings"]
    assert list(feats)[:-1] == oracle_names[:oracle_names.index("features") + 1]
    assert np.array_equal(er.bits(got.numpy()), er.bits(emb.numpy()))
    assert np.array_equal(er.bits(feats["embeddings"].numpy()), er.bits(emb.numpy()))
    bb = tfimm.create_model(name)
    bb.set_weights({k: v for k, v in w.items() if not k.startswith("emb/")})
    own, own_feats = bb.forward_features(x, return_features=True)
    same = {"features": own_feats.get("features", own)}
    if name == "convnext_test_model":
        # ConvNeXt's forward_features is the map in front of pooling and norm (convnext.py:383-411), its `features` entry what
        # lies behind them (convnext.py:431-436) and what the head reads: each is compared with the backbone's own
        same = {"features": bb(x, return_features=True)[1]["features"], "conv_features": own}
    else:
        assert own_feats["features"].shape == own.shape and np.array_equal(er.bits(own_feats["features"].numpy()), er.bits(own.numpy()))
    for key, want in same.items():
        assert feats[key].shape == want.shape and np.array_equal(er.bits(feats[key].numpy()), er.bits(want.numpy())), key
    # normalize=True: rows of norm 1
    n = _embedding_model(name, normalize=True)(x).numpy().astype(np.float64)
    assert np.abs(np.sqrt((n * n).sum(-1)) - 1).max() <= 1e-6
    assert mc.rel_err(n.reshape(ref.shape), er.l2_normalize(ref)) <= mc.TOL_LOGITS


@pytest.mark.parametrize("name", FAMILIES)
def test_embeddings_under_fp32_precision(name):
    x, w, ref, _ = _reference(name, 2)
    with precision.use("fp32"):
        m = _embedding_model(name, normalize=True)
        n = m(x).numpy()
        m2 = _embedding_model(name)
        err = mc.rel_err(m2(x).numpy().reshape(ref.shape), ref)
    print(f"{name}: fp32 embeddings rel-to-max {err:.3e}")
    assert err <= TOL_FP32
    assert mc.rel_err(n.reshape(ref.shape), er.l2_normalize(ref)) <= TOL_FP32


def test_preprocessed_uint8_input_and_branches():
    name = "vit_test_model"
    m = _embedding_model(name, normalize=True)
    pre = tfimm.create_preprocessing(name, defer=True, resize=True)
    u8 = np.random.default_rng(3).integers(0, 256, (4, 40, 52, 3), dtype=np.uint8)
    one = [m(pre(u8)).numpy() for _ in range(3)]
    assert one[0].shape == (4, EMBED) and all(np.array_equal(er.bits(a), er.bits(one[0])) for a in one)
    imgs = [u8[i, :30 + 3 * i, :40 + i] for i in range(4)]
    mixed = m(pre(imgs)).numpy()
    assert mixed.shape == (4, EMBED) and np.isfinite(mixed).all()
    x = mc.make_input(m.cfg, 4)
    base = m(x).numpy()
    m.branches = 2
    two = [m(x).numpy() for _ in range(3)]
    assert all(np.array_equal(er.bits(a), er.bits(base)) for a in two) and any("branches" in key for key in m._plans)


def test_exported_plan_without_the_normalise_op_gives_the_same_embeddings():
    m = _embedding_model("vit_test_model")
    x = torch.from_numpy(mc.make_input(m.cfg, 2)).cuda()
    want = m(x).numpy()
    blob = m.program().make_plan(2).export()
    lib, info = ffi.lib, ffi.PlanInfo()
    ffi.check(lib.tfimm_hip_plan_query(blob, len(blob), C.byref(info)), "plan_query")
    ws = torch.empty(int(info.workspace_bytes), dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h = C.c_void_p()
    ffi.check(lib.tfimm_hip_plan_create(blob, len(blob), ws.data_ptr(), st, C.byref(h)), "plan_create")
    try:
        ffi.check(lib.tfimm_hip_plan_forward(h, x.data_ptr(), 0, st), "plan_forward")
        torch.cuda.synchronize()
        ptr, rows, cols, dt = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int()
        ffi.check(lib.tfimm_hip_plan_output(h, b"embeddings", C.byref(ptr), C.byref(rows), C.byref(cols), C.byref(dt)), "output")
        assert (dt.value, rows.value, cols.value) == (1, 2, EMBED)
        off = ptr.value - ws.data_ptr()
        got = ws[off:off + 2 * EMBED * 4].view(torch.float32).cpu().numpy().reshape(2, EMBED)
    finally:
        lib.tfimm_hip_plan_destroy(h)
    assert np.array_equal(er.bits(got), er.bits(want))
    with pytest.raises(NotImplementedError, match="l2_normalize"):
        _embedding_model("vit_test_model", normalize=True).program().make_plan(2).export()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_model_gallery_search_end_to_end(tmp_path):
    name = "swin_test_model"
    m = _embedding_model(name, normalize=True)
    x = mc.make_input(m.cfg, 8)
    gallery = tfimm.Gallery(EMBED, capacity=8)
    emb = m(x)
    assert gallery.add(emb) == range(0, 8) and len(gallery) == 8 and gallery.dim == EMBED
    e = emb.numpy()
    assert np.array_equal(gallery.numpy(), er.bf16_round(e))                # rounded to nearest even, on the device

    def check(matches, queries, k):
        idx, sc = matches.indices.numpy(), matches.scores.numpy()
        assert idx.dtype == np.int32 and sc.dtype == np.float32 and idx.shape == sc.shape == (len(queries), k)
        check_band(queries, gallery.numpy(), idx, sc, k)
        return idx

    idx = check(m.search(x, gallery, 3), e, 3)
    # past the capacity: the buffer doubles, the old rows answer as before
    old = gallery.numpy()
    rng = np.random.default_rng(1)
    far = (rng.standard_normal((100, EMBED)) * 0.01).astype(f32)
    assert gallery.add(far) == range(8, 108) and gallery.capacity >= 108
    assert np.array_equal(gallery.numpy()[:8], old) and np.array_equal(gallery.numpy()[8:], er.bf16_round(far))
    idx2 = check(m.search(x, gallery, 3), e, 3)
    assert np.array_equal(idx2[:, 0], idx[:, 0])
    check(gallery.search(far[:5], 64), far[:5], 64)                        # an array as the query
    with pytest.raises(ValueError, match="k = 109"):
        gallery.search(e, 109)
    # save_weights -> load_weights: bit-identical embeddings (the reference's test_save_load_model, without Keras)
    path = str(tmp_path / "emb.npz")
    m.save_weights(path)
    fresh = tfimm.EmbeddingModel(tfimm.create_model(name), EMBED, normalize=True)
    fresh.load_weights(path)
    assert np.array_equal(er.bits(fresh(x).numpy()), er.bits(e))

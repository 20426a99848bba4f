"""tfimm_hip_gemm's dispatcher on the GPU: what route() refuses, the fall-back routes behind the A/B switches, the row chunking.

In-process tests run in the default environment.  The switches (TFIMM_GEMM_NO_STREAM, TFIMM_GEMM_NO_DMA, TFIMM_STRIP_CONV,
TFIMM_GEMM_LIMIT) are read once per process: each gets ONE child process that runs the child_* function of this module, one
child at a time, no retry.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hip_checks as hc
import hip_ops as H
from tfimm.engine import pack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUNSUP = -2
CONTROL = "tight_gemm_tile21_ragged_333x200x150_gelu_res"        # the valid GEMM issued behind every refusal
# a horizontal stride of its own on a valid geometry: 6 x 6 -> 6 x 3 (only the stream family has the kernel)
STRIDE_W = dict(mode=1, Cin=8, B=2, H=6, W=6, KH=3, KW=3, stride=1, stride_w=2, pad_t=1, pad_l=1, OH=6, OW=3)


def _sentinel_out(n):
    return torch.full((n,), hc.LAYOUT_SENTINEL, dtype=torch.int16, device=H.DEV)


def _spare_a():
    """A large enough for rows at a pitch of 76 (were a refusal missing, the launch would still read its own buffer)"""
    return H.dev_bf16(np.ones((80, 76), np.float32))


def _refusal(name):
    """(descriptor, its sentinel-filled output, phrase of the message, keep-alive)"""
    out = _sentinel_out(72 * 40 + 16)
    if name == "a2_n_not_multiple_of_8":
        d, _, keep = H.gemm_baseline("dual_dense", N=36, out=out.view(torch.bfloat16))
        return d, out, "a second A operand needs N % 8 == 0", keep
    if name == "a2_out_misaligned":
        d, _, keep = H.gemm_baseline("dual_conv", out=out.view(torch.bfloat16), out_byte_offset=2)
        return d, out, "16-byte aligned bf16 output rows", keep
    if name == "ln_n_not_multiple_of_8":
        d, _, keep = H.gemm_baseline("ln_fold", N=36, out=out.view(torch.bfloat16))
        return d, out, "LayerNorm folding needs dense bf16 rows, N % 8 == 0", keep
    if name == "ln_weights_not_k_padded":
        d, _, keep = H.gemm_baseline("ln_fold", out=out.view(torch.bfloat16), ldw=72)
        return d, out, "LayerNorm folding needs the persistent LDS-DMA family", keep
    if name == "stride_w_cin_not_multiple_of_8":
        d, _, keep = H.gemm_baseline("conv", out=out.view(torch.bfloat16), conv=dict(STRIDE_W, Cin=6), residual=None)
        d.K = 54
        return d, out, "stride_w != stride needs the persistent LDS-DMA family", keep
    if name == "a2_rows_not_16_byte_aligned":
        d, _, keep = H.gemm_baseline("dual_dense", out=out.view(torch.bfloat16))
        a = _spare_a()
        d.a, d.lda = a.data_ptr(), 76
        return d, out, "a second A operand needs the persistent LDS-DMA family", keep + (a,)
    raise KeyError(name)


ROUTE_REFUSALS = ("a2_n_not_multiple_of_8", "a2_out_misaligned", "ln_n_not_multiple_of_8", "ln_weights_not_k_padded",
                  "stride_w_cin_not_multiple_of_8", "a2_rows_not_16_byte_aligned")


def _check_refused(d, out, phrase):
    rc, msg = H.gemm_rc(d)
    H.sync()
    assert rc == EUNSUP and phrase in msg, (rc, msg)
    assert bool((out == hc.LAYOUT_SENTINEL).all()), "a refused GEMM wrote to its output"


def _check_control():
    err, tol = hc.run_case(CONTROL)
    assert err <= tol, (CONTROL, err)


@pytest.mark.parametrize("name", ROUTE_REFUSALS)
def test_route_refuses_and_leaves_no_state(name):
    d, out, phrase, keep = _refusal(name)
    _check_refused(d, out, phrase)
    _check_control()


@pytest.mark.parametrize("kind", H.BASELINES + ("stride_w",))
def test_baselines_run(kind):
    """the valid descriptors the refusal table (tests/test_gemm_contract.py) starts from return 0 and write finite values"""
    if kind == "stride_w":
        d, out, keep = H.gemm_baseline("conv", conv=STRIDE_W, residual=None)
    else:
        d, out, keep = H.gemm_baseline(kind)
    rc, msg = H.gemm_rc(d)
    H.sync()
    assert rc == 0, (rc, msg)
    assert bool(torch.isfinite(out.float()).all())


def test_device_info_is_the_runtime_s():
    n, name = H.device_info(torch.cuda.current_device())
    assert n == torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    assert name.startswith("gfx")
    n4, short = H.device_info(torch.cuda.current_device(), length=4)          # cut to the buffer, terminated
    assert n4 == n and short == "gfx"
    assert H.device_info(torch.cuda.current_device(), length=0) == (n, "")


# ---- pick_tile, the register-staged heuristic, at hint 0: reached only when both LDS-DMA families refuse the operands
def pick_tile_mirror(M, N, cus):
    """pick_tile of csrc/gemm.hip for vector-loaded operands and no hint"""
    def blocks(bm, bn):
        return -(-M // bm) * -(-N // bn)
    if N > 64 and blocks(128, 128) >= 2 * cus:
        return 0
    if N <= 64 and blocks(128, 64) >= 2 * cus:
        return 1
    if N > 64 and blocks(64, 128) >= cus:
        return 5
    if blocks(128, 64) >= 2 * cus:
        return 1
    return 2


def pick_tile_shapes(cus):
    """one (M, N) per return of the heuristic at K = 72; on 256 CUs: 4096 x 2048, 65536 x 64, 2048 x 1024, 333 x 150"""
    return {0: (128 * -(-2 * cus // 16), 2048), 1: (128 * 2 * cus, 64), 5: (64 * -(-cus // 8), 1024), 2: (333, 150)}


def test_pick_tile_mirror_on_256_cus():
    assert pick_tile_shapes(256) == {0: (4096, 2048), 1: (65536, 64), 5: (2048, 1024), 2: (333, 150)}


@pytest.mark.parametrize("want", [0, 1, 5, 2])
def test_pick_tile_at_hint_0_with_unpadded_weights(want):
    cus, _ = H.device_info(torch.cuda.current_device())
    shapes = pick_tile_shapes(cus)
    assert sorted(pick_tile_mirror(M, N, cus) for M, N in shapes.values()) == [0, 1, 2, 5], (cus, shapes)   # four different tiles
    M, N = shapes[want]
    assert pick_tile_mirror(M, N, cus) == want
    run = hc._tg(lambda: hc._gemm_layout_case(M, 72, N, ldw=72, tile=0, seed=2400 + want))
    err, tol = run()
    assert err <= tol, (want, M, N, err, run.stats)


# ---- children
def _run_cases(names):
    for n in names:
        e, t = hc.run_case(n)
        print(n, e, t, getattr(hc.CASES[n], "stats", None), flush=True)
        assert e <= t, (n, e, t)


_STREAM_HINTS = (21, 22, 23, 24, 25, 26, 27, 28, 29, 30)
SWITCH_CASES = (
    [f"tight_gemm_tile{t:02d}_ragged_333x200x150_gelu_res" for t in (0,) + _STREAM_HINTS]
    + [f"tight_gemm_tile{t:02d}_600x320x520_relu_after_res_f32" for t in (0, 21, 28, 30)]
    + ["conv3x3_s1_p1_64to64_relu", "conv3x3_s2_p1_128to128_relu", "conv1x1_s2_256to512"]
    + [f"conv3x3_tile{t:02d}" for t in _STREAM_HINTS] + [f"conv3x3_s2_res_tile{t:02d}" for t in _STREAM_HINTS]
    + ["gemm_se_scale_prologue", "gemm_se_scale_t21_r4_falls_back"] + [f"gemm_se_scale_tile{t:02d}_r144_k200" for t in (1, 21, 23, 25, 29)]
    + sorted(n for n in hc.CASES if n.startswith("tight_gemm_layout_")))
DMA_HINT_CASES = ([f"tight_gemm_tile{t:02d}_ragged_333x200x150_gelu_res" for t in range(11, 17)]
                  + [f"conv3x3_tile{t:02d}" for t in range(11, 17)] + [f"conv3x3_s2_res_tile{t:02d}" for t in range(11, 17)])


def _only_stream_descriptors():
    """valid descriptors only the stream family has a kernel for: (descriptor, sentinel output, phrase, keep-alive)"""
    for kind, over, phrase in (("dual_dense", {}, "a second A operand needs the persistent LDS-DMA family"),
                               ("dual_conv_window2", {}, "a second A operand needs the persistent LDS-DMA family"),
                               ("ln_fold", {}, "LayerNorm folding needs the persistent LDS-DMA family"),
                               ("conv", dict(conv=STRIDE_W, residual=None), "stride_w != stride needs the persistent LDS-DMA family")):
        out = _sentinel_out(72 * 40 + 16)
        d, _, keep = H.gemm_baseline(kind, out=out.view(torch.bfloat16), **over)
        yield d, out, phrase, keep


def child_no_stream():
    """TFIMM_GEMM_NO_STREAM=1: every hint 0 / 21-30 layer falls back to the one-tile LDS-DMA family (SE gate: register-staged)"""
    assert os.environ["TFIMM_GEMM_NO_STREAM"] == "1"
    _run_cases(SWITCH_CASES)
    for d, out, phrase, keep in _only_stream_descriptors():
        _check_refused(d, out, phrase)
    _run_cases([CONTROL])


def child_no_dma():
    """TFIMM_GEMM_NO_DMA=1: everything on the register-staged family, hints 11-16 included"""
    assert os.environ["TFIMM_GEMM_NO_DMA"] == "1"
    _run_cases(SWITCH_CASES + DMA_HINT_CASES)
    for d, out, phrase, keep in _only_stream_descriptors():
        _check_refused(d, out, phrase)
    _run_cases([CONTROL])


def child_no_strip():
    """TFIMM_STRIP_CONV=0: the strip shape at hint 0 stays on the implicit-GEMM tiles -- right, and bit-equal to hint 24's result
    (_strip_conv_case compares the two)"""
    assert os.environ["TFIMM_STRIP_CONV"] == "0"
    e, t = hc._strip_conv_case(130, 28, 28, 405, hint=0)
    print("strip_conv_multiround_b130 at hint 0", e, t, flush=True)
    assert e <= t, e


CHUNK_M, CHUNK_K, CHUNK_N, CHUNK_LDA = 5000, 200, 152, 328          # 656-byte rows: 1536 rows per chunk at 1 MiB -> 1536 x 3 + 392
CHUNK_KINDS = ("plain", "residual_ldr_n8", "out_f32", "ln_fold", "ldc_n8_sentinel")


def _chunk_case(kind):
    """M = 5000 rows through the row chunking (and, pieces of 1250 rows, without it), hint 21: (tight score vs float64, equal bits)"""
    import math
    M, K, N, lda = CHUNK_M, CHUNK_K, CHUNK_N, CHUNK_LDA
    r = np.random.default_rng(2500 + CHUNK_KINDS.index(kind))
    a = hc._bf(r.standard_normal((M, K)) + (0.5 if kind == "ln_fold" else 0.0))
    w = hc._bf(r.standard_normal((K, N)) / math.sqrt(K))
    b = r.standard_normal(N).astype(np.float32)
    f32, ldr, ldc = kind == "out_f32", N + 8, (N + 8 if kind == "ldc_n8_sentinel" else N)
    res = hc._bf(r.standard_normal((M, N))) if kind == "residual_ldr_n8" else None
    wt, _ = pack.pack_dense(w, None)
    a64 = a.astype(np.float64)
    ad = torch.from_numpy(hc._layout_strided(a, lda, 0).view(np.int16)).to(H.DEV).view(torch.bfloat16)
    kw = dict(bias=H.dev_f32(b), act="gelu", out_f32=f32, tile_hint=21, lda=lda, ldc=ldc)
    if kind == "ln_fold":
        st = H.row_stats(ad, 1e-6, rows=M, d=K, xs=lda)
        kw.update(ln_c1=H.dev_bits(pack.pack_ln_c1(wt, N, K)))
        wr = pack.bf16_bits_to_f32(wt).astype(np.float64)[:N, :K]
        a64 = (a64 - a64.mean(1, keepdims=True)) / np.sqrt(a64.var(1, keepdims=True) + 1e-6)
        ref = a64 @ wr.T + b
    else:
        ref = a64 @ w.astype(np.float64) + b
    ref = hc.O.activation(torch.from_numpy(ref), "gelu").numpy()
    if res is not None:
        ref = ref + res
        rd = torch.from_numpy(hc._layout_strided(res, ldr, 0).view(np.int16)).to(H.DEV).view(torch.bfloat16)
        kw.update(residual=rd, ldr=ldr)
    es = 4 if f32 else 2
    wd = H.dev_bits(wt)

    def launch(m0, m1):
        buf, first = hc._layout_out(M, N, ldc, 0, f32)
        od = torch.from_numpy(buf).to(H.DEV)
        extra = dict(ln_stats=st[m0:]) if kind == "ln_fold" else {}
        H.gemm(ad, wd, N, K, M=m1 - m0, out=od, a_byte_offset=m0 * lda * 2, out_byte_offset=(first + m0 * ldc) * es,
               res_byte_offset=m0 * ldr * 2 if res is not None else 0, **extra, **kw)
        H.sync()
        return od.cpu().numpy(), first
    full, first = launch(0, M)
    run = hc._tg(lambda: (hc._layout_score(full, first, ref, ldc, f32), 1.0))
    score = run()[0]
    pieces = np.full_like(full, full[0])                       # the sentinel
    for m0 in range(0, M, 1250):                               # 1250 x 656 bytes < 1 MiB: runs as it is
        part, _ = launch(m0, m0 + 1250)
        lo, hi = first + m0 * ldc, first + (m0 + 1250) * ldc
        assert np.all(part[:lo] == full[0]) and np.all(part[hi:] == full[0])
        pieces[lo:hi] = part[lo:hi]
    return score, run.stats, bool(np.array_equal(pieces, full))


def child_chunks():
    """TFIMM_GEMM_LIMIT = 1 MiB: chunk_rows / run_chunks on a small tensor"""
    assert os.environ["TFIMM_GEMM_LIMIT"] == str(1 << 20)
    for kind in CHUNK_KINDS:
        score, stats, same = _chunk_case(kind)
        print("chunked", kind, score, stats, same, flush=True)
        assert score <= 1.0, (kind, score, stats)
        assert same, f"{kind}: the chunked launch differs from the same rows launched in pieces"
    # what chunk_rows leaves alone (SE gate, a2, row remap + res_mod), each over 1 MiB: unchunked and right
    _run_cases(["gemm_se_scale_t24_r2304_k960", "tight_dual_resnet50_stage2_s2", "tight_dual_conv3x3_resnet18_stage2",
                "gemm_t21_resmod_remap_19600x192x768", "gemm_resmod_remap_392x64x96"])


def _child(fn, env, timeout):
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_gemm_contract as T; T.%s()\n"
            % (ROOT, os.path.join(ROOT, "tensorflow-image-models_amd"), os.path.join(ROOT, "tests"), fn))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_no_stream_switch_falls_back_and_refuses():
    _child("child_no_stream", {"TFIMM_GEMM_NO_STREAM": "1"}, 300)


def test_no_dma_switch_runs_everything_register_staged():
    _child("child_no_dma", {"TFIMM_GEMM_NO_DMA": "1"}, 300)


def test_strip_conv_switch_keeps_the_implicit_gemm_tiles():
    _child("child_no_strip", {"TFIMM_STRIP_CONV": "0"}, 120)


def test_gemm_limit_chunks_rows_bit_equal_to_unchunked_launches():
    _child("child_chunks", {"TFIMM_GEMM_LIMIT": str(1 << 20)}, 240)

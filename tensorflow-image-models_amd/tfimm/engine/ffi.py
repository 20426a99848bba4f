"""ctypes binding of libtfimm_hip.so (C ABI: include/tfimm_hip.h).

The library is the ONLY compute path of this package: if it cannot be loaded the import of
this module raises -- there is deliberately no CPU or PyTorch fallback.
"""
import ctypes as C
import os

# torch ships its own libamdhip64/libhsa-runtime64.  It must be loaded FIRST so that
# libtfimm_hip.so's DT_NEEDED libamdhip64.so.7 resolves to that already-loaded runtime: two HIP
# runtimes in one process do not share devices/streams (launches fail with hipErrorNoDevice).
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# TFIMM_HIP_LIB: another build of the same library (kernel A/B comparisons); there is no non-HIP fallback
LIB_PATH = os.environ.get("TFIMM_HIP_LIB") or os.path.join(_HERE, "libtfimm_hip.so")

ACT = {
    "": 0, "linear": 0, "none": 0, None: 0,
    "relu": 1, "gelu": 2, "swish": 3, "sigmoid": 4, "relu6": 5, "tanh": 6,
}
A_DENSE, A_CONV, A_CONV_C4 = 0, 1, 2


class GemmDesc(C.Structure):
    _fields_ = [
        ("a", C.c_void_p), ("wt", C.c_void_p), ("bias", C.c_void_p), ("residual", C.c_void_p),
        ("out", C.c_void_p), ("a_scale", C.c_void_p),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("lda", C.c_int32), ("ldw", C.c_int32), ("ldr", C.c_int32), ("ldc", C.c_int32),
        ("out_f32", C.c_int32), ("act", C.c_int32), ("act_after_res", C.c_int32),
        ("res_mod", C.c_int32),
        ("remap_in", C.c_int32), ("remap_out", C.c_int32), ("remap_off", C.c_int32),
        ("mode", C.c_int32),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32),
        ("KH", C.c_int32), ("KW", C.c_int32), ("stride", C.c_int32),
        ("pad_t", C.c_int32), ("pad_l", C.c_int32), ("OH", C.c_int32), ("OW", C.c_int32),
        ("rows_per_image", C.c_int32), ("tile_hint", C.c_int32), ("stride_w", C.c_int32),
        ("pix_pitch", C.c_int32),
        ("ln_stats", C.c_void_p), ("ln_c1", C.c_void_p),
        # ABI v4: a second A operand (the shortcut convolution of a residual block folded into its last 1x1 convolution)
        ("a2", C.c_void_p), ("K2", C.c_int32), ("lda2", C.c_int32),
        ("a2_stride", C.c_int32), ("a2_H", C.c_int32), ("a2_W", C.c_int32), ("a2_OH", C.c_int32), ("a2_OW", C.c_int32),
        ("a2_window", C.c_int32),
    ]


class AttnDesc(C.Structure):
    _fields_ = [
        ("qkv", C.c_void_p), ("out", C.c_void_p), ("rel_bias", C.c_void_p),
        ("batch", C.c_int32), ("n_tokens", C.c_int32), ("heads", C.c_int32), ("hd", C.c_int32),
        ("scale", C.c_float),
        ("window", C.c_int32), ("shift", C.c_int32), ("res_h", C.c_int32), ("res_w", C.c_int32),
        ("bias_log2", C.c_void_p),
    ]


class ThaDesc(C.Structure):
    _fields_ = [
        ("qkv", C.c_void_p), ("out", C.c_void_p),
        ("proj_l_w", C.c_void_p), ("proj_l_b", C.c_void_p), ("proj_w_w", C.c_void_p), ("proj_w_b", C.c_void_p),
        ("batch", C.c_int32), ("n_tokens", C.c_int32), ("heads", C.c_int32), ("hd", C.c_int32),
        ("scale", C.c_float), ("proj_dev", C.c_void_p),
    ]


class StemDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("wt", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
        ("batch", C.c_int32), ("Hp", C.c_int32), ("Wp2", C.c_int32), ("OH", C.c_int32), ("OW", C.c_int32),
        ("ldw", C.c_int32),
        ("in_dtype", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pad_t", C.c_int32), ("pad_l", C.c_int32),
    ]


class ChainDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
        ("residual", C.c_void_p), ("out", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32), ("KH", C.c_int32), ("KW", C.c_int32),
        ("stride", C.c_int32), ("pad_t", C.c_int32), ("pad_l", C.c_int32), ("OH", C.c_int32), ("OW", C.c_int32),
        ("C1", C.c_int32), ("N2", C.c_int32),
        ("ldw1", C.c_int32), ("ldw2", C.c_int32), ("ldr", C.c_int32), ("ldc", C.c_int32),
        ("act1", C.c_int32), ("act2", C.c_int32),
        ("ds_x", C.c_void_p), ("ds_w", C.c_void_p), ("ds_cin", C.c_int32),
    ]


class ChainNextDesc(C.Structure):
    """tfimm_chain_next_desc: the fields of tfimm_chain_desc (its first member ``chain``, written flat here so that
    Plan.export finds every pointer), then the following block's conv1 as a second output of the launch"""
    _fields_ = ChainDesc._fields_ + [
        ("w3", C.c_void_p), ("b3", C.c_void_p), ("out2", C.c_void_p),
        ("N3", C.c_int32), ("ldw3", C.c_int32), ("ldc2", C.c_int32),
    ]


class ExpandDwDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p), ("wdw", C.c_void_p), ("b2", C.c_void_p),
        ("y", C.c_void_p), ("sum_out", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32), ("C", C.c_int32), ("Cpad", C.c_int32),
        ("k", C.c_int32), ("stride", C.c_int32), ("pad_t", C.c_int32), ("pad_l", C.c_int32), ("OH", C.c_int32),
        ("OW", C.c_int32), ("act1", C.c_int32), ("act2", C.c_int32),
        ("stem", C.c_int32), ("img_h", C.c_int32), ("img_w", C.c_int32),
    ]


class MlpDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p),
                ("b2", C.c_void_p), ("residual", C.c_void_p), ("out", C.c_void_p), ("M", C.c_int64),
                ("C", C.c_int32), ("hidden", C.c_int32), ("act", C.c_int32), ("eps", C.c_float)]


class GemmMxDesc(C.Structure):
    """tfimm_gemm_mx_desc: the MXFP8 GEMM of the fp8 precision mode (csrc/mx.hip)"""
    _fields_ = [("a", C.c_void_p), ("a_scale", C.c_void_p), ("w", C.c_void_p), ("w_scale", C.c_void_p),
                ("bias", C.c_void_p), ("residual", C.c_void_p), ("out", C.c_void_p), ("out_scale", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("lda", C.c_int32), ("ldw", C.c_int32), ("ldr", C.c_int32), ("ldc", C.c_int32),
                ("out_fmt", C.c_int32), ("act", C.c_int32), ("act_after_res", C.c_int32)]


class LoraDesc(C.Structure):
    """tfimm_lora_desc: the low-rank term of a LoRA Dense layer (csrc/lora.hip)"""
    _fields_ = [("x", C.c_void_p), ("a", C.c_void_p), ("b", C.c_void_p), ("residual", C.c_void_p), ("out", C.c_void_p),
                ("M", C.c_int64), ("K", C.c_int32), ("N", C.c_int32), ("Rp", C.c_int32),
                ("lda", C.c_int32), ("lda_a", C.c_int32), ("ldr", C.c_int32), ("ldc", C.c_int32)]


class HeadUpdateDesc(C.Structure):
    """tfimm_head_update_desc: the weight gradient of a Dense head and the optimizer step on it (csrc/head_fit.hip)"""
    _fields_ = [("f", C.c_void_p), ("g", C.c_void_p), ("labels", C.c_void_p),
                ("w", C.c_void_p), ("w16", C.c_void_p), ("s1", C.c_void_p), ("s2", C.c_void_p),
                ("bias", C.c_void_p), ("bias_s1", C.c_void_p), ("bias_s2", C.c_void_p),
                ("grad_out", C.c_void_p), ("bias_grad_out", C.c_void_p),
                ("B", C.c_int32), ("D", C.c_int32), ("C", C.c_int32),
                ("ldf", C.c_int32), ("ldg", C.c_int32), ("ldw", C.c_int32), ("ldw16", C.c_int32),
                ("opt", C.c_int32),
                ("lr", C.c_float), ("mom_or_one_minus_b1", C.c_float), ("one_minus_b2", C.c_float), ("eps", C.c_float),
                ("wd2", C.c_float)]


class ResizeDesc(C.Structure):
    """tfimm_resize_desc: resize + centre crop + normalise of a uint8 batch (csrc/resize.hip)"""
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p),
                ("y_idx", C.c_void_p), ("y_w", C.c_void_p), ("x_idx", C.c_void_p), ("x_w", C.c_void_p),
                ("mean_host", C.POINTER(C.c_float)), ("std_host", C.POINTER(C.c_float)),
                ("B", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32), ("c_in", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32), ("c_out", C.c_int32),
                ("pad_t", C.c_int32), ("pad_b", C.c_int32), ("pad_l", C.c_int32), ("pad_r", C.c_int32),
                ("taps", C.c_int32)]


class ResizeAADesc(C.Structure):
    """tfimm_resize_aa_desc: the antialiased resize + centre crop + normalise of a uint8 batch (csrc/resize_aa.hip)"""
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p),
                ("y_start", C.c_void_p), ("y_count", C.c_void_p), ("y_w", C.c_void_p),
                ("x_start", C.c_void_p), ("x_count", C.c_void_p), ("x_w", C.c_void_p),
                ("mean_host", C.POINTER(C.c_float)), ("std_host", C.POINTER(C.c_float)),
                ("B", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32), ("c_in", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32), ("c_out", C.c_int32),
                ("pad_t", C.c_int32), ("pad_b", C.c_int32), ("pad_l", C.c_int32), ("pad_r", C.c_int32),
                ("y_taps", C.c_int32), ("x_taps", C.c_int32)]


class ResizeBatchRec(C.Structure):
    """tfimm_resize_batch_rec: where one image of a mixed-size batch and its tables live (csrc/resize_batch.hip)"""
    _fields_ = [("in_offset", C.c_int64), ("Hs", C.c_int32), ("Ws", C.c_int32),
                ("y_tab", C.c_int32), ("x_tab", C.c_int32), ("y_w", C.c_int32), ("x_w", C.c_int32),
                ("y_taps", C.c_int32), ("x_taps", C.c_int32),
                ("tile_rows", C.c_int32), ("cols_max", C.c_int32), ("tile0", C.c_int32), ("n_tiles", C.c_int32)]


class ResizeBatchDesc(C.Structure):
    """tfimm_resize_batch_desc: resize + centre crop + normalise of a uint8 batch of mixed sizes (csrc/resize_batch.hip)"""
    _fields_ = [("in_", C.c_void_p), ("recs", C.c_void_p), ("out", C.c_void_p),
                ("idx", C.c_void_p), ("w", C.c_void_p),
                ("mean_host", C.POINTER(C.c_float)), ("std_host", C.POINTER(C.c_float)),
                ("in_bytes", C.c_int64),
                ("B", C.c_int32), ("c_in", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("c_out", C.c_int32),
                ("pad_t", C.c_int32), ("pad_b", C.c_int32), ("pad_l", C.c_int32), ("pad_r", C.c_int32),
                ("taps", C.c_int32)]


class ResizeBatchAADesc(C.Structure):
    """tfimm_resize_batch_aa_desc: the antialiased launch over a batch of mixed sizes (csrc/resize_batch.hip)"""
    _fields_ = [("in_", C.c_void_p), ("recs", C.c_void_p), ("out", C.c_void_p),
                ("start", C.c_void_p), ("count", C.c_void_p), ("w", C.c_void_p),
                ("mean_host", C.POINTER(C.c_float)), ("std_host", C.POINTER(C.c_float)),
                ("in_bytes", C.c_int64), ("w_floats", C.c_int64),
                ("B", C.c_int32), ("c_in", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("c_out", C.c_int32),
                ("pad_t", C.c_int32), ("pad_b", C.c_int32), ("pad_l", C.c_int32), ("pad_r", C.c_int32),
                ("taps_cap", C.c_int32), ("lds_bytes", C.c_int32)]


class ResizeRegionRec(C.Structure):
    """tfimm_resize_region_rec: where one box inside a larger frame and its tables live (csrc/resize_regions.hip)"""
    _fields_ = [("in_offset", C.c_int64), ("row_pitch", C.c_int64)] + ResizeBatchRec._fields_[1:]


class ResizeRegionDesc(C.Structure):
    """tfimm_resize_region_desc: resize + centre crop + normalise of boxes inside uint8 frames (csrc/resize_regions.hip)"""
    _fields_ = ResizeBatchDesc._fields_


class ResizeRegionAADesc(C.Structure):
    """tfimm_resize_region_aa_desc: the antialiased launch over boxes inside uint8 frames (csrc/resize_regions.hip)"""
    _fields_ = ResizeBatchAADesc._fields_


class ResizeBatchSizes(C.Structure):
    """tfimm_resize_batch_sizes: what tfimm_hip_resize_batch_tables reports"""
    _fields_ = [("in_bytes", C.c_int64), ("tab_elems", C.c_int64), ("w_floats", C.c_int64), ("n_tiles", C.c_int64),
                ("max_taps", C.c_int32), ("lds_floats", C.c_int32), ("bad_image", C.c_int32), ("reserved", C.c_int32)]


class MatchSet(C.Structure):
    """tfimm_match_set: one set of matches for tfimm_hip_matches_merge (csrc/embed_merge.hip) -- 32 bytes"""
    _fields_ = [("scores", C.c_void_p), ("indices", C.c_void_p), ("ld", C.c_int64), ("k", C.c_int32), ("base", C.c_int32)]


# name -> (restype, argtypes); every symbol declared in include/tfimm_hip.h
_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
SYMBOLS = {
    "tfimm_hip_abi_version": (_i, []),
    "tfimm_hip_last_error": (C.c_char_p, []),
    "tfimm_hip_device_info": (_i, [_i, C.c_char_p, _i]),
    "tfimm_hip_gemm": (_i, [C.POINTER(GemmDesc), _vp]),
    "tfimm_hip_conv_chain": (_i, [C.POINTER(ChainDesc), _vp]),
    "tfimm_hip_conv_chain_next": (_i, [C.POINTER(ChainNextDesc), _vp]),
    "tfimm_hip_mlp_fused": (_i, [C.POINTER(MlpDesc), _vp]),
    "tfimm_hip_gemm_mx": (_i, [C.POINTER(GemmMxDesc), _vp]),
    "tfimm_hip_quantize_mx": (_i, [_vp, _i64, _i, _i64, _vp, _vp, _f, _vp, _vp, _i, _vp]),
    "tfimm_hip_expand_dwconv": (_i, [C.POINTER(ExpandDwDesc), _vp]),
    "tfimm_hip_stem_conv_pool": (_i, [C.POINTER(StemDesc), _vp]),
    "tfimm_hip_cast_input": (_i, [_vp, _i, _vp, _i64, _i, _i, _vp]),
    "tfimm_hip_cast_input_pad": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tfimm_hip_preprocess_input": (_i, [_vp, _vp, _i64, _i, _i, C.POINTER(C.c_float), C.POINTER(C.c_float), _vp]),
    "tfimm_hip_preprocess_input_pad": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_float),
                                            C.POINTER(C.c_float), _vp]),
    "tfimm_hip_resize_taps": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "tfimm_hip_preprocess_resize": (_i, [C.POINTER(ResizeDesc), _vp]),
    "tfimm_hip_resize_span_taps": (_i, [_i, _i, _i]),
    "tfimm_hip_resize_spans": (_i, [_i, _i, _i, _i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "tfimm_hip_preprocess_resize_aa": (_i, [C.POINTER(ResizeAADesc), _vp]),
    "tfimm_hip_resize_batch_tables": (_i, [_i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i, _i, _i, C.POINTER(C.c_int32), _i, _i,
                                           C.POINTER(ResizeBatchSizes), _vp, _vp, _vp, _vp]),
    "tfimm_hip_preprocess_resize_batch": (_i, [C.POINTER(ResizeBatchDesc), _vp]),
    "tfimm_hip_preprocess_resize_batch_aa": (_i, [C.POINTER(ResizeBatchAADesc), _vp]),
    "tfimm_hip_resize_region_tables": (_i, [_i, C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32), _i, _i, _i, C.POINTER(C.c_int32), _i, _i,
                                            C.POINTER(ResizeBatchSizes), _vp, _vp, _vp, _vp]),
    "tfimm_hip_preprocess_regions": (_i, [C.POINTER(ResizeRegionDesc), _vp]),
    "tfimm_hip_preprocess_regions_aa": (_i, [C.POINTER(ResizeRegionAADesc), _vp]),
    "tfimm_hip_row_stats": (_i, [_vp, _vp, _i64, _i, _i64, _f, _vp]),
    "tfimm_hip_layernorm": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i64, _i64, _f, _vp]),
    "tfimm_hip_attention": (_i, [C.POINTER(AttnDesc), _vp]),
    "tfimm_hip_talking_heads_attention": (_i, [C.POINTER(ThaDesc), _vp]),
    "tfimm_hip_class_attention": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tfimm_hip_copy_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "tfimm_hip_maxpool": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tfimm_hip_mean_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "tfimm_hip_bcast_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "tfimm_hip_dwconv": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tfimm_hip_se_gate": (_i, [_vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "tfimm_hip_scale_channels": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "tfimm_hip_patch_merge_ln": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "tfimm_hip_attention_probs": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "tfimm_hip_group_norm": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _i, _vp]),
    "tfimm_hip_blur_pool": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "tfimm_hip_avg_pool": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "tfimm_hip_eca_gate": (_i, [_vp, _f, _vp, _vp, _i, _i, _i, _i, _vp]),
    "tfimm_hip_grouped_conv3x3": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "tfimm_hip_bias_act": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp]),
    # the output end (csrc/topk.hip): logits, ld, B, N, k, values, indices, probs
    "tfimm_hip_topk": (_i, [_vp, _i64, _i, _i, _i, _vp, _vp, _vp, _vp]),
    # the scoring end (csrc/score.hip): logits, ld, B, N, labels, loss, rank, pred, prob, state, per_class, confusion
    "tfimm_hip_score": (_i, [_vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # the head fit (csrc/head_fit.hip): logits, ld, B, N, labels, grad, ldg, loss, pred | descriptor
    "tfimm_hip_softmax_grad": (_i, [_vp, _i64, _i, _i, _vp, _vp, _i64, _vp, _vp, _vp]),
    "tfimm_hip_head_update": (_i, [C.POINTER(HeadUpdateDesc), _vp]),
    # the distillation gradient (csrc/distill.hip): s, ld_s, t, ld_t, B, E, valid, normalize, grad, ldg, loss, cosine
    "tfimm_hip_distill_grad": (_i, [_vp, _i64, _vp, _i64, _i, _i, _vp, _i, _vp, _i64, _vp, _vp, _vp]),
    # the embedding end (csrc/embed.hip): x, ld_x, B, E, y, ld_y | B, N, E, k, chunk |
    # q, ld_q, B, g, ld_g, N, E, k, chunk, scores, indices, workspace, workspace_bytes
    "tfimm_hip_l2_normalize": (_i, [_vp, _i64, _i, _i, _vp, _i64, _vp]),
    "tfimm_hip_embed_search_workspace": (_i64, [_i, _i, _i, _i, _i]),
    "tfimm_hip_embed_search": (_i, [_vp, _i64, _i, _vp, _i64, _i, _i, _i, _i, _vp, _vp, _vp, _i64, _vp]),
    # the search for up to 256 neighbours (csrc/embed_wide.hip): E | then as tfimm_hip_embed_search
    "tfimm_hip_embed_search_wide_max_k": (_i, [_i]),
    "tfimm_hip_embed_search_wide_workspace": (_i64, [_i, _i, _i, _i, _i]),
    "tfimm_hip_embed_search_wide": (_i, [_vp, _i64, _i, _vp, _i64, _i, _i, _i, _i, _vp, _vp, _vp, _i64, _vp]),
    # the coarse-to-fine search (csrc/embed_coarse.hip): g, ld_g, N, E, codes, ld_c, exps | E | B, N, E, k, candidates, chunk |
    # q, ld_q, B, g, ld_g, codes, ld_c, exps, N, E, k, candidates, chunk, scores, indices, workspace, workspace_bytes
    "tfimm_hip_embed_quantize_rows": (_i, [_vp, _i64, _i, _i, _vp, _i64, _vp, _vp]),
    "tfimm_hip_embed_search_coarse_max_candidates": (_i, [_i]),
    "tfimm_hip_embed_search_coarse_workspace": (_i64, [_i, _i, _i, _i, _i, _i]),
    "tfimm_hip_embed_search_coarse": (_i, [_vp, _i64, _i, _vp, _i64, _vp, _i64, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i64, _vp]),
    # the search over inverted lists (csrc/embed_lists.hip): B, N, E, L, nprobe, k, parts |
    # q, ld_q, B, g, ld_g, N, E, ids, offsets, L, probes, ld_p, nprobe, k, parts, scores, indices, workspace, workspace_bytes
    "tfimm_hip_embed_search_lists_workspace": (_i64, [_i, _i, _i, _i, _i, _i, _i]),
    "tfimm_hip_embed_search_lists": (_i, [_vp, _i64, _i, _vp, _i64, _i, _i, _vp, _vp, _i, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _i64, _vp]),
    # the same with the queries of a list grouped into MFMA tiles (csrc/embed_lists_grouped.hip): B, L, nprobe | then as above
    "tfimm_hip_embed_search_lists_grouped_tiles": (_i64, [_i, _i, _i]),
    "tfimm_hip_embed_search_lists_grouped_workspace": (_i64, [_i, _i, _i, _i, _i, _i, _i]),
    "tfimm_hip_embed_search_lists_grouped": (_i, [_vp, _i64, _i, _vp, _i64, _i, _i, _vp, _vp, _i, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _i64,
                                                  _vp]),
    # the join of up to MERGE_MAX_SETS sets of matches (csrc/embed_merge.hip): sets, S, B, k, scores, indices, ld_out
    "tfimm_hip_matches_merge": (_i, [C.POINTER(MatchSet), _i, _i, _i, _vp, _vp, _i64, _vp]),
    # the kNN end (csrc/knn.hip): indices, scores, ld, B, k, glabels, N, exclude, inv_temperature, then
    # reduce, top, classes, values, counts, total | nb_classes, labels, loss, rank, pred, prob, state, per_class, confusion
    "tfimm_hip_knn_vote": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i, _vp, _f, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "tfimm_hip_knn_score": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i, _vp, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # the cluster end (csrc/cluster.hip): g, ld_g, N, c, ld_c, C, E, assign, score | M, C, E |
    # g, ld_g, N, E, rows, M, offsets, C, mean, ld_m, counts, workspace, workspace_bytes
    "tfimm_hip_cluster_assign": (_i, [_vp, _i64, _i, _vp, _i64, _i, _i, _vp, _vp, _vp]),
    "tfimm_hip_segment_mean_workspace": (_i64, [_i, _i, _i]),
    "tfimm_hip_segment_mean": (_i, [_vp, _i64, _i, _i, _vp, _i, _vp, _i, _vp, _i64, _vp, _vp, _i64, _vp]),
    # the low-rank adapter term (csrc/lora.hip)
    "tfimm_hip_lora_delta": (_i, [C.POINTER(LoraDesc), _vp]),
    # program-level entry points (csrc/plan.hip): a serialised plan (graph.Plan.export) run without Python host logic
    "tfimm_hip_plan_query": (_i, [_vp, C.c_size_t, _vp]),
    "tfimm_hip_plan_create": (_i, [_vp, C.c_size_t, _vp, _vp, C.POINTER(_vp)]),
    "tfimm_hip_plan_forward": (_i, [_vp, _vp, _i, _vp]),
    "tfimm_hip_plan_output": (_i, [_vp, C.c_char_p, C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i)]),
    "tfimm_hip_plan_destroy": (_i, [_vp]),
    # float32 verification path (csrc/ref32.hip): the bf16 signatures with float tensors
    "tfimm_hip_ref_gemm": (_i, [C.POINTER(GemmDesc), _vp]),
    "tfimm_hip_ref_cast_input": (_i, [_vp, _i, _vp, _i64, _i, _i, C.POINTER(C.c_float), C.POINTER(C.c_float), _vp]),
    "tfimm_hip_ref_preprocess_resize": (_i, [C.POINTER(ResizeDesc), _vp]),
    "tfimm_hip_ref_preprocess_resize_aa": (_i, [C.POINTER(ResizeAADesc), _vp]),
    "tfimm_hip_ref_preprocess_resize_batch": (_i, [C.POINTER(ResizeBatchDesc), _vp]),
    "tfimm_hip_ref_preprocess_resize_batch_aa": (_i, [C.POINTER(ResizeBatchAADesc), _vp]),
    "tfimm_hip_ref_preprocess_regions": (_i, [C.POINTER(ResizeRegionDesc), _vp]),
    "tfimm_hip_ref_preprocess_regions_aa": (_i, [C.POINTER(ResizeRegionAADesc), _vp]),
    "tfimm_hip_ref_layernorm": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i64, _i64, _f, _vp]),
    "tfimm_hip_ref_patch_merge_ln": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "tfimm_hip_ref_copy_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "tfimm_hip_ref_bcast_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "tfimm_hip_ref_mean_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "tfimm_hip_ref_scale_channels": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "tfimm_hip_ref_maxpool": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tfimm_hip_ref_avg_pool": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "tfimm_hip_ref_blur_pool": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "tfimm_hip_ref_dwconv": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tfimm_hip_ref_group_norm": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _i, _vp]),
    "tfimm_hip_ref_attention": (_i, [C.POINTER(AttnDesc), _vp]),
    "tfimm_hip_ref_attention_probs": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "tfimm_hip_ref_talking_heads_attention": (_i, [C.POINTER(ThaDesc), _vp]),
    "tfimm_hip_ref_class_attention": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "tfimm_hip_ref_lora_delta": (_i, [C.POINTER(LoraDesc), _vp]),
    "tfimm_hip_memset_async": (_i, [_vp, _i, C.c_size_t, _vp]),
}


class PlanInfo(C.Structure):
    _fields_ = [("workspace_bytes", C.c_uint64), ("batch", C.c_int32), ("in_h", C.c_int32), ("in_w", C.c_int32),
                ("in_c", C.c_int32), ("n_calls", C.c_int32), ("n_outputs", C.c_int32)]


class HipError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C tensorflow-image-models_amd/csrc -j8` "
            "(or __graft_entry__.build()). tfimm has no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the ABI drifted
        fn.restype = res
        fn.argtypes = args
    # 4 = this tree.  3 (tfimm_gemm_desc without the second A operand) is accepted ONLY for a library named by TFIMM_HIP_LIB --
    # an older build in a kernel A/B; the lowering then does not emit what that build cannot run (ABI below)
    v = lib.tfimm_hip_abi_version()
    if v != 4 and not (v == 3 and os.environ.get("TFIMM_HIP_LIB")):
        raise ImportError("libtfimm_hip.so ABI version mismatch")
    return lib


lib = _load()
ABI = lib.tfimm_hip_abi_version()


_dp_lib = None


def dp_lib():
    """libtfimm_hip_dp.so (include/tfimm_hip_dp.h: the data-parallel exchange behind a C ABI), loaded on first use -- it
    links RCCL, which a single-GPU forward never needs."""
    global _dp_lib
    if _dp_lib is None:
        path = os.environ.get("TFIMM_HIP_DP_LIB") or os.path.join(_HERE, "libtfimm_hip_dp.so")
        if not os.path.exists(path):
            raise HipError(f"{path} not found: build it with `make -C tensorflow-image-models_amd/csrc`")
        L = C.CDLL(path)
        L.tfimm_hip_dp_abi_version.restype = C.c_int
        L.tfimm_hip_dp_last_error.restype = C.c_char_p
        L.tfimm_hip_dp_shard_bounds.argtypes = [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.tfimm_hip_dp_unique_id.argtypes = [C.c_void_p, C.c_size_t]
        L.tfimm_hip_dp_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int]
        L.tfimm_hip_dp_world.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.tfimm_hip_dp_all_gather_logits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        L.tfimm_hip_dp_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.tfimm_hip_dp_destroy.argtypes = [C.c_void_p]
        for f in ("shard_bounds", "unique_id", "create", "world", "all_gather_logits", "forward", "destroy"):
            getattr(L, "tfimm_hip_dp_" + f).restype = C.c_int
        assert L.tfimm_hip_dp_abi_version() == 1
        _dp_lib = L
    return _dp_lib


RESIZE_METHODS = {"bilinear": 0, "bicubic": 1}


def resize_taps(n_in: int, n_resized: int, first: int, n_out: int, method: str):
    """tfimm_hip_resize_taps as numpy arrays: (idx int32 [n_out][taps], w float32 [n_out][taps]) of the output positions
    [first, first + n_out) of an axis resized from ``n_in`` to ``n_resized`` -- a host function, no GPU involved."""
    import numpy as np
    taps = 4 if method == "bicubic" else 2
    idx = np.zeros((n_out, taps), np.int32)
    w = np.zeros((n_out, taps), np.float32)
    check(lib.tfimm_hip_resize_taps(n_in, n_resized, first, n_out, RESIZE_METHODS[method],
                                    idx.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(C.POINTER(C.c_float))),
          "tfimm_hip_resize_taps")
    return idx, w


# include/tfimm_hip.h: the domain and the tiling of tfimm_hip_preprocess_resize_aa
RESIZE_AA_MAX_TAPS = 64
RESIZE_AA_TILE_ROWS, RESIZE_AA_TILE_COLS, RESIZE_AA_MAX_BLOCKS = 16, 32, 1024


# include/tfimm_hip.h: the domain of tfimm_hip_topk (k selection rounds over a row held in LDS)
TOPK_MAX_K, TOPK_MAX_N = 64, 32768

# include/tfimm_hip.h: the domain of tfimm_hip_score (a row held in LDS; a confusion matrix of at most 64 MB), the label of a row
# that is not scored, and the layout of the meter state (int64 words)
SCORE_MAX_N, SCORE_MAX_CONFUSION_N, SCORE_IGNORE = TOPK_MAX_N, 4096, -1
SCORE_SCORED, SCORE_IGNORED, SCORE_INVALID, SCORE_LOSS_EXCLUDED, SCORE_LOSS_Q, SCORE_RANK_HIST = 0, 1, 2, 3, 4, 5
SCORE_RANK_BINS, SCORE_STATE_WORDS = 65, 70

# include/tfimm_hip.h: the optimizers and the domain of tfimm_hip_head_update
HEAD_SGD, HEAD_ADAM = 0, 1
HEAD_MAX_D, HEAD_MAX_C, HEAD_MAX_B = 8192, 32768, 65535
DISTILL_MAX_E = 4096              # tfimm_hip_distill_grad: columns of an embedding row

# include/tfimm_hip.h: the domain of tfimm_hip_embed_search (E a multiple of 16; the gallery row pitch a multiple of 8 elements)
EMBED_MIN_E, EMBED_MAX_E, EMBED_MAX_K = 16, 2048, 64
EMBED_MAX_B = 65535 * 32          # queries per call: tiles of 32 are one grid dimension
EMBED_WIDE_MAX_K = 256            # tfimm_hip_embed_search_wide; what a width E allows: tfimm_hip_embed_search_wide_max_k(E)
EMBED_COARSE_MAX_CANDIDATES = 256 # tfimm_hip_embed_search_coarse; per width: tfimm_hip_embed_search_coarse_max_candidates(E)
EMBED_LISTS_MAX_PROBE = 256       # tfimm_hip_embed_search_lists: lists per query
EMBED_LISTS_MAX_PARTS = 64        # ... and cuts of a list, one workgroup each
EMBED_LISTS_MAX_B = 65535         # ... and queries per call: one grid dimension
EMBED_LISTS_GROUPED_TILE = 32     # tfimm_hip_embed_search_lists_grouped: queries of one list per workgroup of the first pass;
                                  # its k obeys tfimm_hip_embed_search_wide_max_k(E) as well
MERGE_MAX_SETS = 8                # tfimm_hip_matches_merge: sets of matches per call
# include/tfimm_hip.h: the domain of tfimm_hip_knn_vote / tfimm_hip_knn_score (one lane per candidate and per slot of the list)
KNN_MAX_K, KNN_MAX_TOP, KNN_SUM, KNN_MAX = EMBED_MAX_K, 64, 0, 1
# include/tfimm_hip.h: centroids per tfimm_hip_cluster_assign; entries per run of tfimm_hip_segment_mean's summation rule
CLUSTER_MAX_C, SEGMENT_RUN = 65536, 256


def resize_span_taps(n_in: int, n_resized: int, method: str) -> int:
    """tfimm_hip_resize_span_taps: the span pitch T of an axis resized from ``n_in`` to ``n_resized`` with antialiasing"""
    t = lib.tfimm_hip_resize_span_taps(n_in, n_resized, RESIZE_METHODS[method])
    if t <= 0:
        check(t or -1, "tfimm_hip_resize_span_taps")
    return t


def resize_spans(n_in: int, n_resized: int, first: int, n_out: int, method: str):
    """tfimm_hip_resize_spans as numpy arrays: (start int32 [n_out], count int32 [n_out], w float32 [n_out][T]) of the output
    positions [first, first + n_out) of an axis resized from ``n_in`` to ``n_resized`` with antialiasing; entries of ``w`` past
    ``count`` are +0.0 -- a host function, no GPU involved."""
    import numpy as np
    if n_out <= 0:
        raise HipError(f"tfimm_hip_resize_spans: n_out={n_out}")
    T = resize_span_taps(n_in, n_resized, method)
    start, count = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    w = np.zeros((n_out, T), np.float32)
    check(lib.tfimm_hip_resize_spans(n_in, n_resized, first, n_out, RESIZE_METHODS[method],
                                     start.ctypes.data_as(C.POINTER(C.c_int32)), count.ctypes.data_as(C.POINTER(C.c_int32)),
                                     w.ctypes.data_as(C.POINTER(C.c_float))),
          "tfimm_hip_resize_spans")
    return start, count, w


def resize_aa_tables(src_hw, geometry, size, method: str):
    """The span tables of tfimm_hip_preprocess_resize_aa for a ``src_hw`` image resized to ``geometry = (Rh, Rw, top, left)``
    and cropped to ``size``: ``((y_start, y_count, y_w), (x_start, x_count, x_w))``.  ``ValueError`` when an axis shrinks
    further than the launch supports -- checked here, on the host, before anything is uploaded."""
    (Hs, Ws), (Rh, Rw, top, left), (H, W) = src_hw, geometry, size
    for axis, n_in, n_res in (("height", Hs, Rh), ("width", Ws, Rw)):
        T = resize_span_taps(n_in, n_res, method)
        if T > RESIZE_AA_MAX_TAPS:
            raise ValueError(f"antialiased {method} resize of the {axis} {n_in} -> {n_res} needs {T} taps per output pixel, "
                             f"more than TFIMM_RESIZE_AA_MAX_TAPS = {RESIZE_AA_MAX_TAPS}: the source is too large for the "
                             "device resize, shrink it on the host first")
    return resize_spans(Hs, Rh, top, H, method), resize_spans(Ws, Rw, left, W, method)


#: numpy view of tfimm_resize_batch_rec
RESIZE_BATCH_REC = [("in_offset", "<i8")] + [(n, "<i4") for n in (
    "Hs", "Ws", "y_tab", "x_tab", "y_w", "x_w", "y_taps", "x_taps", "tile_rows", "cols_max", "tile0", "n_tiles")]


def resize_batch_tables(sizes, geometries, size, method: str, antialias: bool = False, *, c_in: int = 3, pad=(0, 0, 0, 0)):
    """tfimm_hip_resize_batch_tables as numpy arrays -- records and table arenas of a batch whose images each have a size of
    their own (``sizes[i] = (Hs, Ws)``, ``geometries[i] = (Rh, Rw, top, left)``), all going to the crop window ``size``; a host
    function, no GPU involved.  Returns a dict: ``recs`` (structured, ``RESIZE_BATCH_REC``), ``idx`` and ``w`` (plain) or
    ``start``, ``count`` and ``w`` (antialiased), each exactly as long as the library asked for, and the reported ``in_bytes``,
    ``max_taps``, ``lds_floats`` and ``n_tiles``.  ``c_in`` and ``pad`` (the output layout's border) enter the byte offsets
    and the tile bookkeeping only.  ``ValueError`` naming the image when one lies outside the antialias domain."""
    import numpy as np
    src = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(-1, 2))
    geo = np.ascontiguousarray(np.asarray(geometries, np.int32).reshape(-1, 4))
    B = src.shape[0]
    if B == 0 or geo.shape[0] != B:
        raise ValueError(f"resize_batch_tables: {B} sizes and {geo.shape[0]} geometries")
    pads = (C.c_int32 * 4)(*[int(v) for v in pad])
    i32p = C.POINTER(C.c_int32)
    args = (B, src.ctypes.data_as(i32p), geo.ctypes.data_as(i32p), int(size[0]), int(size[1]), int(c_in), pads,
            RESIZE_METHODS[method], 1 if antialias else 0)
    need = ResizeBatchSizes()
    rc = lib.tfimm_hip_resize_batch_tables(*args, C.byref(need), None, None, None, None)
    if rc != 0 and need.bad_image >= 0:
        i = need.bad_image
        raise ValueError(f"antialiased {method} resize: image {i} of the batch ({src[i, 0]} x {src[i, 1]} -> {geo[i, 0]} x "
                         f"{geo[i, 1]}) needs more than TFIMM_RESIZE_AA_MAX_TAPS = {RESIZE_AA_MAX_TAPS} taps per output pixel: "
                         "the source is too large for the device resize, shrink it on the host first")
    check(rc, "tfimm_hip_resize_batch_tables")
    recs = np.zeros(B, np.dtype(RESIZE_BATCH_REC))
    assert recs.itemsize == C.sizeof(ResizeBatchRec)
    tab_a = np.zeros(need.tab_elems, np.int32)
    tab_b = np.zeros(need.tab_elems if antialias else 0, np.int32)
    w = np.zeros(need.w_floats, np.float32)
    check(lib.tfimm_hip_resize_batch_tables(*args, C.byref(need), recs.ctypes.data, tab_a.ctypes.data,
                                            tab_b.ctypes.data if antialias else None, w.ctypes.data),
          "tfimm_hip_resize_batch_tables")
    out = {"recs": recs, "w": w, "in_bytes": int(need.in_bytes), "max_taps": int(need.max_taps),
           "lds_floats": int(need.lds_floats), "n_tiles": int(need.n_tiles)}
    if antialias:
        out["start"], out["count"] = tab_a, tab_b
    else:
        out["idx"] = tab_a
    return out


#: numpy view of tfimm_resize_region_rec
RESIZE_REGION_REC = [("in_offset", "<i8"), ("row_pitch", "<i8")] + RESIZE_BATCH_REC[1:]


def check_boxes(frames_hw, boxes, box_indices=None):
    """The boxes of ``pre(frames, boxes=..., box_indices=...)`` as ``(boxes int32 (N, 4), box_indices int32 (N,))`` --
    ``boxes[n] = (y0, x0, y1, x1)`` covers rows ``[y0, y1)`` and columns ``[x0, x1)`` of frame ``box_indices[n]``.
    ``ValueError`` naming the box for float coordinates (the caller rounds on purpose), a wrong shape, no box at all, an
    empty box, a box outside its frame and a frame index out of range; ``box_indices`` defaults to zeros for ONE frame."""
    import numpy as np
    hw = np.asarray(frames_hw, np.int64).reshape(-1, 2)
    b = np.asarray(boxes)
    if b.dtype.kind not in "iu":
        raise ValueError(f"boxes must be integer pixel corners (y0, x0, y1, x1), got dtype {b.dtype}: round them on purpose")
    if b.ndim != 2 or b.shape[1] != 4 or b.shape[0] == 0:
        raise ValueError(f"boxes must have shape (N, 4) with N >= 1, got {b.shape}")
    if box_indices is None:
        if hw.shape[0] != 1:
            raise ValueError(f"box_indices is required with {hw.shape[0]} frames: it says which frame every box lies in")
        idx = np.zeros(b.shape[0], np.int64)
    else:
        idx = np.asarray(box_indices)
        if idx.dtype.kind not in "iu" or idx.shape != (b.shape[0],):
            raise ValueError(f"box_indices must be {b.shape[0]} integers, got shape {idx.shape}, dtype {idx.dtype}")
    b, idx = b.astype(np.int64), idx.astype(np.int64)
    no_frame = (idx < 0) | (idx >= hw.shape[0])
    Hf, Wf = hw[np.where(no_frame, 0, idx)].T
    empty = (b[:, 2] <= b[:, 0]) | (b[:, 3] <= b[:, 1])
    outside = (b[:, 0] < 0) | (b[:, 1] < 0) | (b[:, 2] > Hf) | (b[:, 3] > Wf)
    bad = no_frame | empty | outside
    if bad.any():                                        # the first bad box, by what is wrong with it
        n = int(np.argmax(bad))
        y0, x0, y1, x1 = (int(v) for v in b[n])
        if no_frame[n]:
            raise ValueError(f"box {n} names frame {int(idx[n])} of {hw.shape[0]}")
        if empty[n]:
            raise ValueError(f"box {n} ({y0}, {x0}, {y1}, {x1}) is empty")
        raise ValueError(f"box {n} ({y0}, {x0}, {y1}, {x1}) lies outside its frame {int(idx[n])} ({int(Hf[n])} x {int(Wf[n])})")
    return np.ascontiguousarray(b, np.int32), np.ascontiguousarray(idx, np.int32)


def resize_region_tables(frames_hw, boxes, box_indices, geometries, size, method: str, antialias: bool = False, *,
                         c_in: int = 3, pad=(0, 0, 0, 0)):
    """tfimm_hip_resize_region_tables as numpy arrays -- records and table arenas of boxes inside larger frames
    (``frames_hw[f] = (Hf, Wf)``, ``boxes[n] = (y0, x0, y1, x1)`` in frame ``box_indices[n]``, ``geometries[n] = (Rh, Rw, top,
    left)`` of the box's own size), all going to the crop window ``size``; a host function, no GPU involved.  Returns the dict
    of ``resize_batch_tables`` with ``recs`` structured as ``RESIZE_REGION_REC``; ``in_bytes`` is the sum of the FRAMES'
    bytes, each frame packed once.  ``ValueError`` naming the box for a box that is empty, outside its frame, names no frame
    or lies outside the antialias domain."""
    import numpy as np
    hw = np.ascontiguousarray(np.asarray(frames_hw, np.int32).reshape(-1, 2))
    bx, idx = check_boxes(hw, boxes, box_indices)
    geo = np.ascontiguousarray(np.asarray(geometries, np.int32).reshape(-1, 4))
    N = bx.shape[0]
    if geo.shape[0] != N:
        raise ValueError(f"resize_region_tables: {N} boxes and {geo.shape[0]} geometries")
    pads = (C.c_int32 * 4)(*[int(v) for v in pad])
    i32p = C.POINTER(C.c_int32)
    args = (hw.shape[0], hw.ctypes.data_as(i32p), N, bx.ctypes.data_as(i32p), idx.ctypes.data_as(i32p), geo.ctypes.data_as(i32p),
            int(size[0]), int(size[1]), int(c_in), pads, RESIZE_METHODS[method], 1 if antialias else 0)
    need = ResizeBatchSizes()
    need.bad_image = -1
    rc = lib.tfimm_hip_resize_region_tables(*args, C.byref(need), None, None, None, None)
    if rc != 0 and need.bad_image >= 0:
        i = need.bad_image
        raise ValueError(f"antialiased {method} resize: box {i} ({bx[i, 2] - bx[i, 0]} x {bx[i, 3] - bx[i, 1]} -> {geo[i, 0]} x "
                         f"{geo[i, 1]}) needs more than TFIMM_RESIZE_AA_MAX_TAPS = {RESIZE_AA_MAX_TAPS} taps per output pixel: "
                         "the box is too large for the device resize, shrink the frame on the host first")
    check(rc, "tfimm_hip_resize_region_tables")
    recs = np.zeros(N, np.dtype(RESIZE_REGION_REC))
    assert recs.itemsize == C.sizeof(ResizeRegionRec)
    tab_a = np.zeros(need.tab_elems, np.int32)
    tab_b = np.zeros(need.tab_elems if antialias else 0, np.int32)
    w = np.zeros(need.w_floats, np.float32)
    check(lib.tfimm_hip_resize_region_tables(*args, C.byref(need), recs.ctypes.data, tab_a.ctypes.data,
                                             tab_b.ctypes.data if antialias else None, w.ctypes.data),
          "tfimm_hip_resize_region_tables")
    out = {"recs": recs, "w": w, "in_bytes": int(need.in_bytes), "max_taps": int(need.max_taps),
           "lds_floats": int(need.lds_floats), "n_tiles": int(need.n_tiles)}
    if antialias:
        out["start"], out["count"] = tab_a, tab_b
    else:
        out["idx"] = tab_a
    return out


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib.tfimm_hip_last_error().decode("utf-8", "replace")
        raise HipError(f"{what or 'tfimm_hip call'} failed (rc={rc}): {msg}")


# ---- roctx markers (TFIMM_ROCTX=1, graph.Plan.run): libroctx64 ships with ROCm; absent library = no markers, never an error
_roctx = None


def _roctx_lib():
    global _roctx
    if _roctx is None:
        _roctx = False
        # rocprofv3 (rocprofiler-sdk) traces its own roctx library; libroctx64 is the roctracer-era one
        for name in ("librocprofiler-sdk-roctx.so", "libroctx64.so"):
            try:
                cand = C.CDLL(name)
                cand.roctxRangePushA.argtypes = [C.c_char_p]
                cand.roctxRangePushA.restype = C.c_int
                cand.roctxRangePop.restype = C.c_int
                _roctx = cand
                break
            except (OSError, AttributeError):
                continue
    return _roctx


def roctx_push(label: str) -> None:
    lib_ = _roctx_lib()
    if lib_:
        lib_.roctxRangePushA(label.encode("utf-8", "replace"))


def roctx_pop() -> None:
    lib_ = _roctx_lib()
    if lib_:
        lib_.roctxRangePop()

"""ctypes binding of libxmh.so (the C ABI declared in include/xmh.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C
clip-based-cross-modal-hash_amd`` with ``hipcc --offload-arch=gfx950``.  If it
is missing this module raises at import: the product path never falls back to
PyTorch/CPU arithmetic.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("XMH_LIB", os.path.join(_HERE, "libxmh.so"))

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libxmh.so not found at %s -- build it first (python -c 'import __graft_entry__ as g; g.build()' "
        "or make -C clip-based-cross-modal-hash_amd). There is no CPU fallback." % LIB_PATH)

# PyTorch first: it ships its own HIP runtime, and the process must end up with ONE.  Loaded after torch, libxmh.so binds to the runtime
# torch already brought in (same soname); loaded before it, the library initialises /opt/rocm's copy, torch then initialises its own, and
# the first caller of the second one finds "no ROCm-capable device" (seen with build() and smoke() in one process).  Every caller of this
# module hands it torch tensors anyway.
import torch  # noqa: E402,F401

lib = C.CDLL(LIB_PATH)

vp, i64, i32, sz = C.c_void_p, C.c_int64, C.c_int, C.c_size_t


class ScanPlan(C.Structure):
    _fields_ = [("chunk", i64), ("nchunk", i64), ("nqtile", i64), ("qpad", i64), ("nbuckets", i64), ("ws_bytes", sz)]


class Linear(C.Structure):                     # xmh_linear
    _fields_ = [("w_f32", vp), ("w_hi", vp), ("w_lo", vp), ("bias", vp), ("n", i64), ("k", i64)]


class ClipBlock(C.Structure):                  # xmh_clip_block
    _fields_ = [("ln1_w", vp), ("ln1_b", vp), ("ln2_w", vp), ("ln2_b", vp),
                ("qkv", Linear), ("out", Linear), ("fc", Linear), ("proj", Linear)]


class VitWeights(C.Structure):                 # xmh_vit_weights
    _fields_ = [("resolution", i32), ("patch", i32), ("width", i32), ("heads", i32), ("layers", i32), ("out_dim", i32),
                ("conv1", Linear), ("cls", vp), ("pos", vp), ("ln_pre_w", vp), ("ln_pre_b", vp), ("ln_post_w", vp),
                ("ln_post_b", vp), ("proj", Linear), ("blocks", C.POINTER(ClipBlock))]


class TextWeights(C.Structure):                # xmh_text_weights
    _fields_ = [("vocab", i32), ("context", i32), ("width", i32), ("heads", i32), ("layers", i32), ("out_dim", i32),
                ("tok_emb", vp), ("pos", vp), ("ln_final_w", vp), ("ln_final_b", vp), ("proj", Linear),
                ("blocks", C.POINTER(ClipBlock))]


class DcmhtHead(C.Structure):                  # xmh_dcmht_head
    _fields_ = [("v_proj", Linear), ("out_proj", Linear), ("norm_is_batchnorm", i32), ("norm_eps", C.c_float),
                ("norm_w", vp), ("norm_b", vp), ("bn_mean", vp), ("bn_var", vp), ("fc2", Linear)]


class MithMlp(C.Structure):                    # xmh_mith_mlp
    _fields_ = [("ln_w", vp), ("ln_b", vp), ("ln_eps", C.c_float), ("fc1", Linear), ("fc2", Linear)]


class MithHead(C.Structure):                   # xmh_mith_head
    _fields_ = [("width", i32), ("k_bits", i32), ("top_k", i32), ("res_layers", i32), ("layers", i32), ("heads", i32),
                ("mlps", C.POINTER(MithMlp)), ("concept", Linear), ("pos_enc", vp), ("blocks", C.POINTER(ClipBlock)),
                ("hash_w", vp), ("hash_b", vp)]


class MithLossArgs(C.Structure):               # xmh_mith_loss_args
    _fields_ = [("N", i64), ("B", i32), ("K", i32), ("D", i32), ("res_img_cls", vp), ("res_txt_cls", vp), ("img_cls_hash", vp),
                ("txt_cls_hash", vp), ("tokens_hash_i", vp), ("tokens_hash_t", vp), ("trans_tokens_i", vp), ("trans_tokens_t", vp),
                ("buffer", vp), ("label_sim", vp), ("hyper_tokens_intra", C.c_double), ("hyper_distill", C.c_double),
                ("hyper_info_nce", C.c_double), ("hyper_cls_inter", C.c_double), ("hyper_quan", C.c_double), ("hyper_alpha", C.c_double),
                ("hyper_lambda", C.c_double), ("temperature", C.c_double)]


class MithTrain(C.Structure):                  # xmh_mith_train
    _fields_ = [("head", MithHead), ("proj", Linear)]


class MithMlpGrads(C.Structure):               # xmh_mith_mlp_grads
    _fields_ = [(n, vp) for n in ("ln_w", "ln_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")]


class DcmhtTrain(C.Structure):                 # xmh_dcmht_train
    _fields_ = [("wv", vp), ("bv", vp), ("wo", vp), ("bo", vp), ("norm_w", vp), ("norm_b", vp), ("running_mean", vp),
                ("running_var", vp), ("w2", vp), ("b2", vp), ("norm_is_batchnorm", i32), ("eps", C.c_float), ("momentum", C.c_float)]


class DcmhtGrads(C.Structure):                 # xmh_dcmht_grads
    _fields_ = [("d_wv", vp), ("d_bv", vp), ("d_wo", vp), ("d_bo", vp), ("d_norm_w", vp), ("d_norm_b", vp), ("d_w2", vp),
                ("d_b2", vp), ("d_x", vp)]


class ClipBlockGrads(C.Structure):             # xmh_clip_block_grads
    _fields_ = [(n, vp) for n in ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_w", "ln2_b", "fc_w", "fc_b", "proj_w", "proj_b")]


class VitGrads(C.Structure):                   # xmh_vit_grads
    _fields_ = [(n, vp) for n in ("proj", "ln_post_w", "ln_post_b", "ln_pre_w", "ln_pre_b", "pos", "cls", "conv1")] + [("blocks", C.POINTER(ClipBlockGrads))]


class TextGrads(C.Structure):                  # xmh_text_grads
    _fields_ = [(n, vp) for n in ("proj", "ln_final_w", "ln_final_b", "pos", "tok")] + [("blocks", C.POINTER(ClipBlockGrads))]


class MithGrads(C.Structure):                  # xmh_mith_grads
    _fields_ = [("mlps", C.POINTER(MithMlpGrads)), ("concept", vp), ("blocks", C.POINTER(ClipBlockGrads))] + \
               [(n, vp) for n in ("hash_w", "hash_b", "proj_w", "proj_b", "d_cls", "d_tokens")]


class TwdhStreams(C.Structure):                # xmh_twdh_streams
    MAX = 8                                    # XMH_TWDH_MAX_STREAMS
    _fields_ = [("n", i32), ("bit", i32 * 8), ("K", i32 * 8)]


# name -> (restype, argtypes); mirrors include/xmh.h one to one
class DimchHead(C.Structure):                  # xmh_dimch_head
    _fields_ = [(k, vp) for k in ("conv_w", "conv_b", "w1", "b1", "w2", "b2")] + [(k, i32) for k in ("T", "E", "H", "M", "K", "hash_func")]


class DimchHeadGrads(C.Structure):             # xmh_dimch_head_grads
    _fields_ = [(k, vp) for k in ("d_conv_w", "d_conv_b", "d_w1", "d_b1", "d_w2", "d_b2", "d_tokens")]


class UmoedLayer(C.Structure):                 # xmh_umoed_layer
    NAMES = ("ln1_g", "ln1_b", "sa_in_w", "sa_in_b", "sa_out_w", "sa_out_b", "ln2_g", "ln2_b", "ca_in_w", "ca_in_b", "ca_out_w", "ca_out_b",
             "ln3_g", "ln3_b", "lin_w", "lin_b", "phi", "exp_w", "exp_b", "lin2_w", "lin2_b")
    _fields_ = [(k, vp) for k in NAMES]


class UmoedHead(C.Structure):                  # xmh_umoed_head
    _fields_ = [("layers", C.POINTER(UmoedLayer)), ("n_layers", i32)] + [(k, vp) for k in ("first_w", "first_b", "queries", "cls_w", "cls_b")] + \
               [(k, i32) for k in ("E", "d", "heads", "F", "M", "V", "n_experts", "slots", "moe", "hash_func", "merge")] + [("ln_eps", C.c_float)]


class UmoedLayerGrads(C.Structure):            # xmh_umoed_layer_grads: the MoE layer's 19 parameters, in UmoedLayer's order
    NAMES = UmoedLayer.NAMES[:19]
    _fields_ = [(k, vp) for k in NAMES]


class UmoedHeadGrads(C.Structure):             # xmh_umoed_head_grads
    _fields_ = [("layers", C.POINTER(UmoedLayerGrads))] + [(k, vp) for k in ("d_queries", "d_cls_w", "d_cls_b", "d_tokens")]


class UmoedConsts(C.Structure):                # xmh_umoed_consts
    _fields_ = [("extreme", i32)] + [(k, C.c_float) for k in ("extreme_T", "token_triplet_margin", "triplet_alpha", "unif_alpha")]


PROTOTYPES = {
    "xmh_version": (i32, []),
    "xmh_build_id": (C.c_char_p, []),
    "xmh_last_error": (C.c_char_p, []),
    "xmh_prof_enable": (i32, [i32]),
    "xmh_range_push": (i32, [C.c_char_p]),
    "xmh_range_pop": (i32, []),
    "xmh_scan_verify": (i32, [i32]),
    "xmh_prof_read": (i32, [C.c_char_p, C.POINTER(C.c_double), C.POINTER(i64)]),
    "xmh_pack_sign": (i32, [vp, i64, i32, vp, vp, vp, vp, vp]),
    "xmh_pack_pair_argmax": (i32, [vp, i64, i32, vp, vp, vp]),
    "xmh_unpack_pm1": (i32, [vp, vp, i64, i32, vp, vp]),
    "xmh_pack_labels": (i32, [vp, i32, i64, i32, vp, vp]),
    "xmh_hamming_dist": (i32, [vp, vp, vp, vp, i64, i64, i32, vp, vp, vp]),
    "xmh_label_sim": (i32, [vp, vp, i64, i64, i32, vp, vp]),
    "xmh_scan_plan_make": (i32, [i64, i64, i32, i32, C.POINTER(ScanPlan)]),
    "xmh_scan_pair_cache_bytes": (sz, [i64, i64, i32, i32]),
    "xmh_scan_pair_cache_offset": (sz, [i64, i64, i32, i32]),
    "xmh_scan_ws_bytes_nocache": (sz, [i64, i64, i32, i32]),
    "xmh_scan_describe": (i32, [i64, i64, i32, i32, i32, C.c_char_p, sz]),
    "xmh_scan_tables_packed": (i32, [i64, i64, i32, i32, i32, i32]),
    "xmh_scan_gate_offset": (sz, [i64, i64, i32, i32]),
    "xmh_hamming_hist": (i32, [vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, sz, vp, vp, vp]),
    "xmh_hamming_hist_for": (i32, [vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, sz, vp, vp, i32, vp]),
    "xmh_hamming_ap": (i32, [vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, sz, vp, vp, vp, i64, vp, vp, vp]),
    "xmh_hamming_map": (i32, [vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, sz, i64, vp, vp, vp, vp]),
    "xmh_scan_totals_offset": (sz, [i64, i64, i32, i32, C.POINTER(C.c_size_t)]),
    "xmh_hamming_map_sharded": (i32, [vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, sz, vp, i32, i32, i64, vp, vp, vp, vp]),
    "xmh_shard_slice_offsets": (i32, [vp, i32, i32, i32, vp, vp]),
    "xmh_hamming_map_sharded_offsets": (i32, [vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, sz, vp, i32, i64, vp, vp, vp, vp]),
    "xmh_calc_map_k_ws_bytes": (sz, [i64, i64, i32, i32]),
    "xmh_calc_map_k": (i32, [vp, vp, vp, vp, i64, i64, i32, i32, i64, vp, sz, C.POINTER(C.c_double), C.POINTER(i32), vp]),
    "xmh_map_finalize": (i32, [vp, vp, i64, vp, vp]),
    "xmh_shard_offsets": (i32, [vp, i32, i32, i64, i32, vp, vp, vp, vp]),
    "xmh_gemm_nt_f32": (i32, [vp, i64, vp, i64, vp, vp, i64, vp, i64, i64, i64, i64, i32, i32, vp]),
    "xmh_gemm_nt_h16": (i32, [vp, i64, vp, i64, vp, vp, i64, vp, i64, i64, i64, i64, i32, vp]),
    "xmh_gemm_nt_split16": (i32, [vp, i64, vp, vp, i64, vp, vp, i64, vp, i64, i64, i64, i64, i32, vp]),
    "xmh_cast_f32_to_f16": (i32, [vp, vp, i64, vp]),
    "xmh_layernorm_f32": (i32, [vp, i64, vp, vp, C.c_float, vp, i64, i64, i32, vp]),
    "xmh_attention_f32": (i32, [vp, i64, i32, i32, i32, i32, vp, vp, vp]),
    "xmh_attention_split16": (i32, [vp, i64, i32, i32, i32, i32, vp, vp, vp]),
    "xmh_image_preprocess_u8": (i32, [vp, i64, i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
    "xmh_image_preprocess_train_ws_bytes": (sz, [i64, i32, i32, i32]),
    "xmh_image_preprocess_train_u8": (i32, [vp, i64, vp, i64, i32, i32, i32, vp, vp, vp, sz, vp, vp, vp]),
    "xmh_im2col_patch": (i32, [vp, i64, i32, i32, i32, vp, vp]),
    "xmh_vit_assemble": (i32, [vp, vp, vp, vp, vp, C.c_float, vp, i64, i32, i32, vp]),
    "xmh_text_embed": (i32, [vp, vp, vp, vp, vp, i64, i32, i32, i32, vp]),
    "xmh_gather_rows": (i32, [vp, i64, vp, i32, i32, vp, i64, i32, vp]),
    "xmh_affine_cols": (i32, [vp, vp, vp, vp, vp, C.c_float, vp, i64, i32, vp]),
    "xmh_pair_softmax": (i32, [vp, vp, i64, i32, vp]),
    "xmh_lta_aggregate": (i32, [vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp]),
    "xmh_bitwise_hash": (i32, [vp, vp, vp, vp, vp, i64, i32, i32, vp]),
    "xmh_clip_workspace_bytes": (sz, [i64, i32, i32, i32, i32, i32]),
    "xmh_clip_blocks_forward": (i32, [C.POINTER(ClipBlock), i32, i32, i32, vp, i64, i32, i32, vp, i32, vp, sz, vp]),
    "xmh_clip_saved_bytes": (sz, [i64, i32, i32, i32]),
    "xmh_clip_blocks_forward_saved": (i32, [C.POINTER(ClipBlock), i32, i32, i32, vp, i64, i32, i32, vp, i32, vp, sz, vp, sz, vp]),
    "xmh_clip_blocks_backward_ws_bytes": (sz, [i64, i32, i32]),
    "xmh_clip_blocks_backward": (i32, [C.POINTER(ClipBlock), i32, i32, i32, i64, i32, i32, vp, vp, sz, vp, i32, C.POINTER(ClipBlockGrads), i32,
                                       vp, sz, vp]),
    "xmh_vit_b32_forward": (i32, [C.POINTER(VitWeights), vp, i64, i32, vp, vp, vp, sz, vp]),
    "xmh_text_forward": (i32, [C.POINTER(TextWeights), vp, vp, i64, i32, i32, vp, vp, vp, vp, sz, vp]),
    "xmh_text_forward_packed": (i32, [C.POINTER(TextWeights), vp, vp, i64, i64, i32, i32, vp, vp, sz, vp]),
    "xmh_text_forward_packed_dev": (i32, [C.POINTER(TextWeights), vp, vp, i64, i32, i32, vp, vp, vp, sz, vp]),
    "xmh_vit_train_saved_bytes": (sz, [i64, i32, i32, i32]),
    "xmh_vit_train_ws_bytes": (sz, [i64, i32, i32, i32, i32]),
    "xmh_vit_train_forward": (i32, [C.POINTER(VitWeights), vp, i64, vp, vp, sz, vp, sz, vp]),
    "xmh_vit_backward": (i32, [C.POINTER(VitWeights), vp, i64, vp, sz, vp, C.POINTER(VitGrads), i32, vp, sz, vp]),
    "xmh_text_train_saved_bytes": (sz, [i64, i32, i32, i32]),
    "xmh_text_train_ws_bytes": (sz, [i64, i32, i32, i32]),
    "xmh_text_train_forward": (i32, [C.POINTER(TextWeights), vp, vp, i64, i32, vp, vp, vp, sz, vp, sz, vp]),
    "xmh_text_backward": (i32, [C.POINTER(TextWeights), vp, vp, vp, i64, i32, vp, sz, vp, C.POINTER(TextGrads), i32, vp, sz, vp]),
    "xmh_vit_train_tokens_saved_bytes": (sz, [i64, i32, i32, i32]),
    "xmh_vit_train_tokens_ws_bytes": (sz, [i64, i32, i32, i32, i32]),
    "xmh_vit_train_forward_tokens": (i32, [C.POINTER(VitWeights), vp, i64, vp, vp, vp, sz, vp, sz, vp]),
    "xmh_vit_backward_tokens": (i32, [C.POINTER(VitWeights), vp, i64, vp, sz, vp, vp, C.POINTER(VitGrads), i32, vp, sz, vp]),
    "xmh_text_train_tokens_saved_bytes": (sz, [i64, i32, i32, i32]),
    "xmh_text_train_tokens_ws_bytes": (sz, [i64, i32, i32, i32]),
    "xmh_text_train_forward_tokens": (i32, [C.POINTER(TextWeights), vp, vp, i64, i32, vp, vp, vp, vp, sz, vp, sz, vp]),
    "xmh_text_backward_tokens": (i32, [C.POINTER(TextWeights), vp, vp, vp, i64, i32, vp, sz, vp, vp, C.POINTER(TextGrads), i32, vp, sz, vp]),
    "xmh_head_workspace_bytes": (sz, [i64, i32, i32]),
    "xmh_head_dcmht": (i32, [C.POINTER(DcmhtHead), vp, i64, i32, vp, vp, vp, vp, sz, vp]),
    "xmh_head_dsph": (i32, [C.POINTER(Linear), vp, i64, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    "xmh_head_mith_workspace_bytes": (sz, [i64, i32, i32, i32, i32]),
    "xmh_head_mith": (i32, [C.POINTER(MithHead), vp, vp, vp, i64, i32, i32, vp, vp, vp, sz, vp]),
    "xmh_row_l2normalize": (i32, [vp, i64, i32, vp, vp, vp]),
    "xmh_pairwise_l2_from_gram": (i32, [vp, vp, vp, i64, i64, vp]),
    "xmh_affine_inplace": (i32, [vp, i64, C.c_float, C.c_float, vp]),
    "xmh_gemm_f32_sort_ws_bytes": (sz, [i64, i64]),
    "xmh_gemm_f32_sort_map": (i32, [vp, vp, vp, vp, i64, i64, i32, i32, i64, vp, sz, vp, vp, vp, vp]),
    "xmh_float_sort_ap": (i32, [vp, vp, vp, i64, i64, i32, i64, vp, sz, vp, vp, vp]),
    "xmh_pair_similarity_loss": (i32, [vp, vp, i64, i32, vp, i32, i32, C.c_float, C.c_float, vp, vp]),
    "xmh_quant_loss": (i32, [vp, i64, vp, vp]),
    "xmh_pair_similarity_loss_grad": (i32, [vp, vp, i64, i32, vp, i32, i32, C.c_float, C.c_float, C.c_float, vp, vp, i32, vp]),
    "xmh_quant_loss_grad": (i32, [vp, i64, C.c_float, vp, vp, i32, vp]),
    "xmh_twdh_targets": (i32, [vp, i32, vp, vp, i64, i32, vp, vp]),
    "xmh_twdh_loss_ws_bytes": (sz, [i64, i32]),
    "xmh_twdh_loss": (i32, [C.POINTER(TwdhStreams), vp, vp, vp, vp, vp, i64, C.c_double, C.c_double, vp, vp, sz, vp]),
    "xmh_twdh_loss_grad": (i32, [C.POINTER(TwdhStreams), vp, vp, vp, i64, C.c_double, C.c_double, vp, vp, vp, vp]),
    "xmh_twdh_short_forward": (i32, [vp, vp, i64, i32, i32, vp, vp]),
    "xmh_twdh_short_backward": (i32, [vp, vp, vp, i64, i32, i32, vp, i32, vp, sz, vp]),
    "xmh_twdh_trans_ws_bytes": (sz, [i64, i32, i32]),
    "xmh_twdh_trans_loss": (i32, [vp, vp, i64, i32, i32, C.c_double, vp, sz, vp, vp]),
    "xmh_twdh_trans_grad": (i32, [vp, vp, i64, i32, i32, C.c_double, vp, vp, i32, vp, sz, vp]),
    "xmh_twdh_trans_check": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "xmh_hyp_loss_ws_bytes": (sz, [i64, i32, i32]),
    "xmh_hyp_loss": (i32, [vp, vp, vp, i64, i32, i32, vp, C.c_float, C.c_float, vp, sz, vp, vp]),
    "xmh_hyp_loss_grad": (i32, [vp, vp, vp, i64, i32, i32, vp, C.c_float, C.c_float, vp, vp, vp, vp, i32, vp, sz, vp]),
    "xmh_mith_loss_ws_bytes": (sz, [i64, i32, i32, i32]),
    "xmh_mith_loss": (i32, [C.POINTER(MithLossArgs), vp, sz, vp, vp]),
    "xmh_mith_loss_grad": (i32, [C.POINTER(MithLossArgs), vp, C.POINTER(vp), i32, vp, sz, vp]),
    "xmh_head_dcmht_train_bytes": (sz, [i64, i32, i32, C.POINTER(C.c_size_t)]),
    "xmh_head_dcmht_train_forward": (i32, [C.POINTER(DcmhtTrain), vp, i64, i32, i32, vp, vp, sz, vp, sz, vp]),
    "xmh_head_dcmht_backward": (i32, [C.POINTER(DcmhtTrain), vp, vp, i64, i32, i32, vp, sz, C.POINTER(DcmhtGrads), i32, vp, sz, vp]),
    "xmh_head_dcmht_stats_len": (i64, [i32]),
    "xmh_head_dcmht_train_forward_stats": (i32, [C.POINTER(DcmhtTrain), vp, i64, i32, i32, vp, sz, vp, sz, vp, vp]),
    "xmh_head_dcmht_train_forward_apply": (i32, [C.POINTER(DcmhtTrain), vp, i64, i32, i32, vp, i32, vp, vp, sz, vp, sz, vp]),
    "xmh_head_dcmht_backward_stats": (i32, [C.POINTER(DcmhtTrain), vp, vp, i64, i32, i32, vp, sz, C.POINTER(DcmhtGrads), i32, vp, sz, vp, vp]),
    "xmh_head_dcmht_backward_apply": (i32, [C.POINTER(DcmhtTrain), vp, i64, i32, i32, vp, i32, i32, vp, sz, C.POINTER(DcmhtGrads), i32, vp, sz,
                                            vp]),
    "xmh_head_dsph_train_forward": (i32, [vp, vp, vp, vp, C.c_float, i64, i32, i32, vp, vp]),
    "xmh_head_dsph_backward": (i32, [vp, vp, vp, vp, C.c_float, vp, i64, i32, i32, vp, vp, vp, i32, vp, sz, vp]),
    "xmh_mith_train_saved_bytes": (sz, [i64, i32, i32, i32, i32, i32]),
    "xmh_mith_train_ws_bytes": (sz, [i64, i32, i32, i32, i32]),
    "xmh_mith_train_forward": (i32, [C.POINTER(MithTrain), vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, sz, vp, sz, vp]),
    "xmh_mith_train_backward": (i32, [C.POINTER(MithTrain), vp, i64, i32, vp, vp, vp, vp, vp, sz, C.POINTER(MithGrads), i32, vp, sz, vp]),
    "xmh_bertadam_chunk": (i64, []),
    "xmh_bertadam_ws_bytes": (sz, [i64, i64]),
    "xmh_bertadam_step": (i32, [vp, i64, vp, i64, vp, sz, vp]),
    "xmh_bucket_pack": (i32, [vp, i64, vp, i64, C.c_float, vp, vp]),
    "xmh_bucket_unpack": (i32, [vp, i64, vp, i64, vp, vp]),
    "xmh_topk_ws_bytes": (sz, [i64, i64, i32, i32]),
    "xmh_hamming_topk": (i32, [vp, vp, i64, i64, i32, i32, i64, vp, sz, vp, vp, vp]),
    "xmh_topk_ws_init": (i32, [i64, i64, i32, i32, vp, sz, vp]),
    "xmh_hamming_topk_prepared": (i32, [vp, vp, i64, i64, i32, i32, i64, vp, sz, vp, vp, vp]),
    "xmh_topk_ternary_ws_bytes": (sz, [i64, i64, i32, i32]),
    "xmh_topk_ternary_ws_init": (i32, [i64, i64, i32, i32, vp, sz, vp]),
    "xmh_hamming_topk_ternary": (i32, [vp, vp, vp, vp, i64, i64, i32, i32, i64, vp, sz, i32, vp, vp, vp]),
    "xmh_topk_describe": (i32, [i64, i64, i32, i32, C.c_char_p, sz]),
    "xmh_topk_record_bytes": (sz, [i64, i32]),
    "xmh_topk_merge_host": (i32, [vp, i32, i64, i32, vp, vp]),
    "xmh_dnph_loss_ws_bytes": (sz, [i64, i32, i32, i32]),
    "xmh_dnph_loss": (i32, [vp, vp, vp, vp, vp, i64, i32, i32, i32, vp, C.c_float, C.c_float, vp, vp, vp, sz, vp, vp]),
    "xmh_dnph_loss_grad": (i32, [vp, vp, vp, vp, vp, i64, i32, i32, i32, vp, C.c_float, C.c_float, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp,
                                 sz, vp]),
    "xmh_assign_min_cost": (i32, [vp, i32, vp]),
    "xmh_linear_backward": (i32, [vp, vp, vp, i64, i32, i32, vp, vp, vp, i32, vp, sz, vp]),
    "xmh_dimch_loss_ws_bytes": (sz, [i64, i32, i32, i32]),
    "xmh_dimch_loss": (i32, [vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, vp, sz, vp, vp]),
    "xmh_dimch_loss_grad": (i32, [vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, sz, vp]),
    "xmh_head_dimch_bytes": (sz, [i64, i32, i32, i32, i32, i32, C.POINTER(sz)]),
    "xmh_head_dimch": (i32, [C.POINTER(DimchHead), vp, i64, vp, vp, vp, sz, vp]),
    "xmh_head_dimch_train_forward": (i32, [C.POINTER(DimchHead), vp, vp, C.c_float, i64, vp, vp, vp, sz, vp]),
    "xmh_head_dimch_backward": (i32, [C.POINTER(DimchHead), vp, i32, C.c_float, vp, vp, i64, vp, sz, C.POINTER(DimchHeadGrads), i32, vp, sz, vp]),
    "xmh_head_umoed_bytes": (sz, [i64, i32, C.POINTER(UmoedHead)]),
    "xmh_head_umoed": (i32, [C.POINTER(UmoedHead), vp, i64, i32, vp, vp, vp, sz, vp]),
    "xmh_head_umoed_train_bytes": (sz, [i64, i32, C.POINTER(UmoedHead), C.POINTER(sz)]),
    "xmh_umoed_keep_bytes": (sz, [i64, i32, C.POINTER(UmoedHead)]),
    "xmh_head_umoed_train_forward": (i32, [C.POINTER(UmoedHead), vp, vp, C.c_float, i64, i32, vp, vp, vp, sz, vp, sz, vp]),
    "xmh_head_umoed_backward": (i32, [C.POINTER(UmoedHead), vp, vp, C.c_float, vp, i64, i32, vp, sz, C.POINTER(UmoedHeadGrads), i32, vp, sz, vp]),
    "xmh_umoed_loss_ws_bytes": (sz, [i64, i32, i32, i32]),
    "xmh_umoed_loss": (i32, [vp, vp, i64, i32, i32, i32, vp, C.POINTER(UmoedConsts), vp, sz, vp, vp]),
    "xmh_umoed_loss_grad": (i32, [vp, vp, i64, i32, i32, i32, vp, C.POINTER(UmoedConsts), vp, vp, vp, i32, vp, sz, vp]),
}

for _name, (_res, _args) in PROTOTYPES.items():
    _fn = getattr(lib, _name)          # AttributeError here == header and library out of sync
    _fn.restype = _res
    _fn.argtypes = _args


class XmhError(RuntimeError):
    pass


def check(rc: int, what: str = "") -> None:
    """Map a non-zero C status to RuntimeError(xmh_last_error()) (SURVEY 8b 'Errors')."""
    if rc != 0:
        msg = lib.xmh_last_error().decode("utf-8", "replace")
        raise XmhError("%s failed (%d): %s" % (what or "libxmh call", rc, msg))


def ptr(t):
    """Device (or host) pointer of a torch tensor / None -> c_void_p."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(nbytes: int, device):
    """Scratch bytes for one call, from torch's stream-aware caching allocator: the runner drives several forwards of ONE model on
    different streams at a time, a workspace owned by the module would be shared between them."""
    import torch
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def prof_enable(on=True) -> None:
    """True / 1: HIP events around the dominant kernels (prof_read); 2: roctx ranges around every phase of the path (a
    `rocprofv3 --marker-trace` timeline gets phase markers); 3: both; False / 0: off."""
    check(lib.xmh_prof_enable(int(on)), "xmh_prof_enable")


def scan_verify(on: bool = True) -> None:
    """debug mode: every unsharded ranking call is re-derived with the masked VALU kernels and compared (xmh_scan_verify); a
    disagreement raises RuntimeError from the call.  About 3x the cost of an evaluation plus a stream synchronisation."""
    check(lib.xmh_scan_verify(int(bool(on))), "xmh_scan_verify")


class prof_range:
    """roctx range from the host layer (collectives of the sharded evaluation, the encode loop): ``with prof_range("name"):``.
    A no-op -- two foreign calls that return at once -- while ranges are off (prof_enable(2))."""

    def __init__(self, name: str):
        self.name = name.encode()

    def __enter__(self):
        lib.xmh_range_push(self.name)
        return self

    def __exit__(self, *exc):
        lib.xmh_range_pop()
        return False


def prof_read(name: str):
    """-> (mean launch ms, launches) of the named kernel since prof_enable(True)."""
    ms, n = C.c_double(0.0), i64(0)
    check(lib.xmh_prof_read(name.encode(), C.byref(ms), C.byref(n)), "xmh_prof_read")
    return ms.value, n.value

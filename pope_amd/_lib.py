"""ctypes binding of libpope_hip.so (C ABI: include/pope_hip.h).

The product path has NO fallback: if the library is missing or fails to load the import of
``lib()`` raises, and every op raises on a non-zero status.
"""
import ctypes as C
import os
import subprocess

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# POPE_LIB_PATH: dev override used by the lab scripts (stamped / ablated builds live outside the tree)
LIB_PATH = os.environ.get("POPE_LIB_PATH") or os.path.join(_CSRC, "libpope_hip.so")

c_float_p = C.POINTER(C.c_float)
c_int_p = C.POINTER(C.c_int)
c_ll_p = C.POINTER(C.c_longlong)


class VitBlockWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1",
        "norm2_w", "norm2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ls2", "qkv_wp", "fc1_wp", "fc2_wp", "proj_wp")]


class VitWeights(C.Structure):
    _fields_ = [("dim", C.c_int), ("depth", C.c_int), ("heads", C.c_int), ("patch", C.c_int),
                ("hidden", C.c_int), ("patch_w", C.c_void_p), ("norm_w", C.c_void_p),
                ("norm_b", C.c_void_p), ("blocks_host", C.POINTER(VitBlockWeights)), ("precision", C.c_int),
                ("patch_wp", C.c_void_p)]


class LoftrLayerWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("q_wp", "kv_wp", "merge_wp", "mlp0_wp", "mlp1_wp", "norm1_w", "norm1_b", "norm2_w",
                                           "norm2_b")]


class ResnetFpnWeights(C.Structure):
    _fields_ = [("w", C.c_void_p * 22), ("b", C.c_void_p * 22)]


class ConvLayerArgs(C.Structure):
    """pope_conv_layer_args: one convolution layer on the caller's buffers (pope_conv_layer_f32)."""
    _fields_ = [("form", C.c_int), ("precision", C.c_int), ("n", C.c_int), ("H", C.c_int), ("W", C.c_int), ("cch", C.c_int),
                ("taps", C.c_int), ("a", C.c_void_p), ("a_rows", C.c_size_t), ("w", C.c_void_p), ("bias", C.c_void_p), ("N", C.c_int),
                ("ldc", C.c_int), ("slope", C.c_float), ("out_planes", C.c_void_p), ("out_f32", C.c_void_p), ("zero_border", C.c_int),
                ("res", C.c_void_p), ("ldres", C.c_int), ("up_src", C.c_void_p), ("up_lds", C.c_int), ("scratch", C.c_void_p),
                ("scratch_bytes", C.c_size_t), ("range_flag", C.c_void_p)]


class DenseMatchArgs(C.Structure):
    """pope_dense_match_args: everything one dense-matcher call takes (pope_dense_match_workspace_bytes, pope_dense_match_f32)."""
    _fields_ = [("feat0", C.c_void_p), ("stride0", C.c_longlong), ("feat1", C.c_void_p), ("stride1", C.c_longlong)] + [
        (n, C.c_int) for n in ("n", "L", "S", "C", "h0", "w0", "h1", "w1")] + [
        ("thr", C.c_float), ("border_rm", C.c_int), ("temperature", C.c_float), ("scale", C.c_float), ("match_type", C.c_int),
        ("bin_score", C.c_void_p), ("skh_iters", C.c_int), ("skh_prefilter", C.c_int)] + [
        (n, C.c_void_p) for n in ("fill_mask0", "fill_mask1", "border_mask0", "border_mask1", "scale0", "scale1", "conf_matrix",
                                  "b_ids", "i_ids", "j_ids", "mconf", "mkpts0_c", "mkpts1_c", "counts", "workspace")] + [
        ("workspace_bytes", C.c_size_t), ("precision", C.c_int), ("range_flag", C.c_void_p)]


class SamBlockWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("norm1_w", "norm1_b", "qkv_wp", "qkv_b", "proj_wp", "proj_b", "rel_h", "rel_w",
                                           "norm2_w", "norm2_b", "fc1_wp", "fc1_b", "fc2_wp", "fc2_b")] + [("global_attn", C.c_int)]


class SamEncoderWeights(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("img", "patch", "dim", "depth", "heads", "hidden", "out_chans", "window", "precision")] + [
        ("patch_wp", C.c_void_p), ("patch_b", C.c_void_p), ("pos", C.c_void_p), ("ones", C.c_void_p),
        ("blocks_host", C.POINTER(SamBlockWeights)), ("neck0_wp", C.c_void_p), ("neck1_w", C.c_void_p), ("neck1_b", C.c_void_p),
        ("neck2_wp", C.c_void_p), ("neck3_w", C.c_void_p), ("neck3_b", C.c_void_p), ("block_eps", C.c_float), ("neck_eps", C.c_float)]


class SamDecoderLayerWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "sa_qkv_w", "sa_qkv_b", "sa_o_w", "sa_o_b", "norm1_w", "norm1_b", "t2i_q_w", "t2i_q_b", "t2i_o_w", "t2i_o_b", "norm2_w",
        "norm2_b", "mlp1_w", "mlp1_b", "mlp2_w", "mlp2_b", "norm3_w", "norm3_b", "i2t_kv_w", "i2t_kv_b", "img_qk_wp", "img_qk_b",
        "img_v_wp", "img_v_b", "i2t_o_wp", "i2t_o_b", "norm4_w", "norm4_b")]


class SamDecoderWeights(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("dim", "heads", "mlp_dim", "depth", "grid", "num_mask_tokens", "iou_hidden", "iou_depth",
                                       "precision")] + [
        ("token_eps", C.c_float), ("up_eps", C.c_float), ("tokens", C.c_void_p), ("layers_host", C.POINTER(SamDecoderLayerWeights))] + [
        (n, C.c_void_p) for n in ("fin_q_w", "fin_q_b", "fin_k_wp", "fin_k_b", "fin_v_wp", "fin_v_b", "fin_o_w", "fin_o_b",
                                  "norm_final_w", "norm_final_b", "up1_wp", "up1_b", "up_ln_w", "up_ln_b", "up2_w", "up2_b")] + [
        ("hyper_w", C.c_void_p * 12), ("hyper_b", C.c_void_p * 12), ("iou_w", C.c_void_p * 3), ("iou_b", C.c_void_p * 3)]


class SamMaskEmbedWeights(C.Structure):
    _fields_ = [("mask_in_chans", C.c_int), ("embed_dim", C.c_int), ("grid", C.c_int), ("ln1_eps", C.c_float), ("ln2_eps", C.c_float)] + [
        (n, C.c_void_p) for n in ("conv1_w", "conv1_b", "ln1_w", "ln1_b", "conv2_w", "conv2_b", "ln2_w", "ln2_b", "conv3_w", "conv3_b")]


class PoseRegressorLayer(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "linear1_w", "linear1_b", "linear2_w",
                                           "linear2_b", "norm1_w", "norm1_b", "norm2_w", "norm2_b")]


class PoseRegressorWeights(C.Structure):
    _fields_ = [("num_sample", C.c_int), ("mode", C.c_int), ("layers", PoseRegressorLayer * 4), ("mlp_w", C.c_void_p * 7),
                ("mlp_b", C.c_void_p * 7)] + [(n, C.c_void_p) for n in ("trans_w", "trans_b", "rot_w", "rot_b")]


class MocopeEncoderLayer(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "linear1_w", "linear1_b", "linear2_w",
                                           "linear2_b", "norm1_w", "norm1_b", "norm2_w", "norm2_b")]


class MocopeDecoderLayer(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "cross_in_proj_w", "cross_in_proj_b",
                                           "cross_out_proj_w", "cross_out_proj_b", "linear1_w", "linear1_b", "linear2_w", "linear2_b",
                                           "norm1_w", "norm1_b", "norm2_w", "norm2_b", "norm3_w", "norm3_b")]


class MocopeTransformer(C.Structure):
    _fields_ = [("enc", MocopeEncoderLayer * 6), ("enc_norm_w", C.c_void_p), ("enc_norm_b", C.c_void_p),
                ("dec", MocopeDecoderLayer * 6), ("dec_norm_w", C.c_void_p), ("dec_norm_b", C.c_void_p)]


class MocopeWeights(C.Structure):
    _fields_ = [("num_sample", C.c_int), ("mode", C.c_int), ("transformer_mkpts", MocopeTransformer), ("mkpts_as_q", MocopeTransformer),
                ("cnn_as_q", MocopeTransformer), ("mlp1_w", C.c_void_p * 2), ("mlp1_b", C.c_void_p * 2), ("mlp_img_w", C.c_void_p),
                ("mlp_img_b", C.c_void_p), ("mlp2_w", C.c_void_p * 7), ("mlp2_b", C.c_void_p * 7)] + [
        (n, C.c_void_p) for n in ("trans_w", "trans_b", "rot_w", "rot_b")]


class ConvNextBlockWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("dw_w", "dw_b", "norm_w", "norm_b", "pw1_w", "pw1_b", "grn_gamma", "grn_beta", "pw2_w",
                                           "pw2_b", "pw1_wp", "pw2_wp")]


class ConvNextWeights(C.Structure):
    _fields_ = [("depths", C.c_int * 4), ("dims", C.c_int * 4), ("num_classes", C.c_int)] + [
        (n, C.c_void_p) for n in ("stem_w", "stem_b", "stem_ln_w", "stem_ln_b")] + [
        (n, C.c_void_p * 3) for n in ("ds_ln_w", "ds_ln_b", "ds_w", "ds_b", "ds_wp")] + [
        ("blocks_host", C.POINTER(ConvNextBlockWeights))] + [(n, C.c_void_p) for n in ("norm_w", "norm_b", "head_w", "head_b", "ones")]


class VimDirWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("conv_w", "conv_b", "x_proj_w", "dt_w", "dt_b", "A_log", "D")]


class VimLayerWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("norm_w", "in_proj_w", "out_proj_w", "in_proj_wp", "out_proj_wp")] + [("dir", VimDirWeights * 2)]


class VimWeights(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("img", "stride", "dim", "depth", "num_classes")] + [("eps", C.c_float)] + [
        (n, C.c_void_p) for n in ("patch_w", "patch_b", "cls", "pos", "patch_wp")] + [("layers_host", C.POINTER(VimLayerWeights))] + [
        (n, C.c_void_p) for n in ("norm_f_w", "head_w", "head_b")]


# name -> (restype, argtypes); every symbol declared in include/pope_hip.h
PREC_F32_MFMA, PREC_F16X3, PREC_F16 = 0, 1, 2
PLANES_ACT_SCALE, PLANES_W_SCALE = 8.0, 256.0
PRECISIONS = {"f32": PREC_F32_MFMA, "f16x3": PREC_F16X3, "f16": PREC_F16}
FFN_KINDS = {"mlp": 0, "swiglu": 1}    # POPE_FFN_*
MATCH_TYPES = {"dual_softmax": 0, "sinkhorn": 1}   # POPE_MATCH_*
LOFTR_ATTENTIONS = {"linear": 0, "full": 1}        # POPE_LOFTR_ATTN_*
EPI_BIAS_SWIGLU = 11                   # POPE_EPI_BIAS_SWIGLU
EPI_QKV_F16 = 8                        # POPE_EPI_QKV_F16 (pope_linear_f16 only)
CONV3, CONV_S2, CONV1_UP, CONV_STEM = 0, 1, 2, 3   # POPE_CONV_* forms of pope_conv_layer_f32
c_uint_p = C.POINTER(C.c_uint)
F16_MAX = 65504.0
# bits of an f16x3 range-guard word (pope_hip.h POPE_RANGE_*)
RANGE_BITS = {1: "patch embed input", 2: "LayerNorm output", 4: "q/k/v", 8: "MLP hidden (GELU / SwiGLU output)",
              16: "matcher features", 32: "op-level operand"}

PROTOTYPES = {
    "pope_abi_version": (C.c_int, []),
    "pope_error_string": (C.c_char_p, [C.c_int]),
    "pope_layernorm_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "pope_linear_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p] * 2 + [C.c_int, C.c_void_p, C.c_void_p]),
    "pope_split_planes_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "pope_linear_planes_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p] * 4),
    "pope_layernorm_planes_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "pope_linear_rowln_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int]
                              + [C.c_void_p] * 3 + [C.c_float] + [C.c_void_p] * 4),
    "pope_layernorm_rowln_order_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "pope_layernorm_f16": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "pope_to_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]),
    "pope_linear_f16": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "pope_div_planes_f32": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                      C.c_void_p, C.c_void_p]),
    "pope_patch_embed_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p]),
    "pope_attention_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pope_patch_embed_planes_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pope_attention_planes_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pope_attention_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pope_attention_planes_diag_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, c_ll_p, C.c_void_p]),
    "pope_cls_cosine_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "pope_vit_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "pope_vit_forward_f32": (C.c_int, [C.POINTER(VitWeights), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int, c_int_p, C.POINTER(C.c_void_p),
                                       C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pope_vit_forward_profiled_f32": (C.c_int, [C.POINTER(VitWeights), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, c_int_p,
                                                c_int_p, C.c_uint]),
    "pope_vit_launch_count": (C.c_int, [C.c_int]),
    "pope_event_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "pope_event_destroy": (C.c_int, [C.c_void_p]),
    "pope_event_elapsed_ms": (C.c_int, [C.c_void_p, C.c_void_p, c_float_p]),
    "pope_dense_match_workspace_bytes": (C.c_size_t, [C.POINTER(DenseMatchArgs)]),
    "pope_dense_match_f32": (C.c_int, [C.POINTER(DenseMatchArgs), C.c_void_p]),
    "pope_loftr_layer_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "pope_loftr_encoder_layer_f32": (C.c_int, [C.POINTER(LoftrLayerWeights)] + [C.c_void_p] * 4 + [C.c_int] * 5
                                     + [C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pope_loftr_full_attention_f32": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pope_loftr_linear_attention_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "pope_loftr_linear_attention_seams": (None, [c_int_p, c_int_p]),
    "pope_loftr_linear_attention_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p, C.c_void_p]),
    "pope_resnetfpn_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "pope_resnetfpn_forward_f32": (C.c_int, [C.POINTER(ResnetFpnWeights), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pope_conv_layer_scratch_bytes": (C.c_size_t, [C.c_int] * 6),
    "pope_conv_layer_f32": (C.c_int, [C.POINTER(ConvLayerArgs), C.c_void_p]),
    "pope_conv_layer_f16": (C.c_int, [C.POINTER(ConvLayerArgs), C.c_void_p]),
    "pope_fine_preprocess_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "pope_fine_preprocess_f32": (C.c_int, [C.c_void_p, c_ll_p, C.c_int, C.c_int, C.c_int, C.c_void_p, c_ll_p, C.c_int, C.c_int,
                                           C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int] * 3
                                 + [C.c_void_p] * 4 + [C.c_int, C.c_void_p] + [C.c_void_p, C.c_size_t, C.c_void_p]
                                 + [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "pope_fine_match_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pope_sam_encoder_workspace_bytes": (C.c_size_t, [C.POINTER(SamEncoderWeights), C.c_int]),
    "pope_sam_encoder_forward_f32": (C.c_int, [C.POINTER(SamEncoderWeights), C.c_void_p, C.c_int, C.c_void_p, C.c_int, c_int_p,
                                               C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pope_sam_decoder_workspace_bytes": (C.c_size_t, [C.POINTER(SamDecoderWeights), C.c_int, C.c_int, C.c_int]),
    "pope_sam_decoder_forward_f32": (C.c_int, [C.POINTER(SamDecoderWeights)] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p,
                                                                                                  C.c_longlong, C.c_int]
                                     + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p, C.c_void_p]),
    "pope_sam_decoder_images_workspace_bytes": (C.c_size_t, [C.POINTER(SamDecoderWeights), C.c_int, c_int_p, C.c_int, C.c_int,
                                                             C.c_longlong]),
    "pope_sam_decoder_forward_images_f32": (C.c_int, [C.POINTER(SamDecoderWeights), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                      c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_int]
                                            + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p, C.c_void_p]),
    "pope_sam_decoder_seams": (None, [c_int_p] * 4),
    "pope_sam_decoder_token_linear_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 5
                                          + [C.c_void_p]),
    "pope_sam_decoder_self_attention_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "pope_sam_decoder_t2i_attention_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_longlong, c_int_p,
                                                     C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "pope_sam_decoder_i2t_attention_f32": (C.c_int, [C.c_void_p, C.c_longlong, c_int_p, C.c_void_p, C.c_int, C.c_int]
                                           + [C.c_void_p] * 4),
    "pope_sam_decoder_residual_norm_f32": (C.c_int, [C.c_void_p, C.c_longlong, c_int_p] + [C.c_void_p] * 3 + [C.c_float]
                                           + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pope_sam_decoder_prepare_keys_f32": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int]
                                          + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3),
    "pope_sam_decoder_upscale_tail_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_float] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p,
                                                                                                         C.c_void_p]),
    "pope_sam_mask_embed_f32": (C.c_int, [C.POINTER(SamMaskEmbedWeights), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "pope_sam_postprocess_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "pope_sam_postprocess_f32": (C.c_int, [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 6 + [C.c_double, C.c_double]
                                 + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "pope_sam_nms_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pope_sam_nms_segments_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pope_sam_rle_u32": (C.c_int, [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_longlong, C.c_void_p]),
    "pope_sam_small_regions_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "pope_sam_small_regions_u32": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]),
    "pope_preprocess_u8_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3
                               + [C.c_int] * 7 + [c_float_p, c_float_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pope_resize_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3
                       + [C.c_int] * 3 + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pope_sam_preprocess_u8_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3
                                   + [C.c_int] * 5 + [c_float_p, c_float_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "pope_crop_normalize_u8_f32": (C.c_int, [C.c_void_p] + [C.c_int] * 7 + [c_float_p, c_float_p, C.c_void_p, C.c_void_p]),
    "pope_gray_u8_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pope_pose_images_u8_f32": (C.c_int, [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 3
                                + [C.c_void_p, C.c_void_p]),
    "pope_crop_warp_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p]),
    "pope_estimate_pose_workspace_bytes": (C.c_size_t, [C.c_int, C.c_longlong]),
    "pope_estimate_pose_f64": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_longlong, C.c_double, C.c_double, C.c_int, C.c_ulonglong]
                               + [C.c_void_p] * 5 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "pope_pose_regressor_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "pope_pose_regressor_forward_f32": (C.c_int, [C.POINTER(PoseRegressorWeights)] + [C.c_void_p] * 7 + [C.c_int] * 3 + [C.c_longlong]
                                        + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "pope_pose_regressor_embedding_f32": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_longlong] + [C.c_void_p] * 4),
    "pope_pose_regressor_encoder_f32": (C.c_int, [C.POINTER(PoseRegressorWeights)] + [C.c_void_p] * 7 + [C.c_int] * 3 + [C.c_longlong]
                                        + [C.c_void_p] * 4),
    "pope_pose_regressor_layer_f32": (C.c_int, [C.POINTER(PoseRegressorLayer), C.c_void_p] + [C.c_int] * 3 + [C.c_void_p]),
    "pope_pose_regressor_stream_linear_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_longlong, C.c_int, C.c_void_p]),
    "pope_pose_regressor_tail_f32": (C.c_int, [C.POINTER(PoseRegressorWeights), C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3),
    "pope_mocope_linear_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]),
    "pope_mocope_attention_f32": (C.c_int, [C.c_void_p, C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]),
    "pope_mocope_add_ln_f32": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]),
    "pope_mocope_ffn76_f32": (C.c_int, [C.c_void_p] * 9 + [C.c_int, C.c_void_p]),
    "pope_mocope_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "pope_mocope_forward_f32": (C.c_int, [C.POINTER(MocopeWeights)] + [C.c_void_p] * 9 + [C.c_int] * 3 + [C.c_longlong, C.c_int]
                                + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "pope_mocope_tap_f32": (C.c_int, [C.POINTER(MocopeWeights)] + [C.c_void_p] * 9 + [C.c_int] * 3 + [C.c_longlong, C.c_int, C.c_int]
                            + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "pope_convnext_workspace_bytes": (C.c_size_t, [C.POINTER(ConvNextWeights), C.c_int, C.c_int, C.c_int]),
    "pope_convnext_forward_f32": (C.c_int, [C.POINTER(ConvNextWeights), C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_void_p,
                                                                                                     C.POINTER(C.c_void_p), C.c_void_p,
                                                                                                     C.c_size_t, C.c_void_p, C.c_void_p]),
    "pope_convnext_dwconv_f32": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]),
    "pope_convnext_grn_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "pope_convnext_grn_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p, C.c_void_p]),
    "pope_convnext_pose_heads_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p] * 3),
    "pope_vim_workspace_bytes": (C.c_size_t, [C.POINTER(VimWeights), C.c_int]),
    "pope_vim_forward_f32": (C.c_int, [C.POINTER(VimWeights), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]),
    "pope_vim_scan_chunk": (C.c_int, []),
    "pope_vim_scan_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "pope_vim_scan_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(VimDirWeights)] + [C.c_int] * 4
                          + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pope_vim_conv1d_silu_f32": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(VimDirWeights), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pope_vim_add_rmsnorm_f32": (C.c_int, [C.c_void_p] * 6 + [C.c_longlong, C.c_int, C.c_float, C.c_longlong, C.c_longlong, C.c_void_p,
                                                              C.c_void_p]),
    "pope_five_point_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pope_streaming_top3_host": (C.c_int, [c_float_p, C.c_int, c_float_p, c_ll_p]),
    "pope_vote_top3_batch_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_float] + [C.c_void_p] * 5 + [C.c_void_p]),
    "pope_vote_top3_shared_f32": (C.c_int, [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int] * 3 + [C.c_float]
                                  + [C.c_void_p] * 5 + [C.c_void_p]),
    "pope_slot_tally_f32": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_longlong, C.c_float] + [C.c_void_p] * 7 + [C.c_void_p]),
}

_lib = None


def build(force=False):
    """Compile libpope_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-C", _CSRC, "clean"], check=True, capture_output=True)
    res = subprocess.run(["make", "-C", _CSRC, "-j4"], capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building libpope_hip.so failed:\n" + res.stdout + res.stderr)
    return LIB_PATH


def code_object_archs(path=None):
    """GPU architectures of the code objects bundled in the library, read from the offload-bundle entry ids in the
    file itself (no extraction: `llvm-objdump --offloading` drops one file per code object next to its input)."""
    import re
    with open(path or LIB_PATH, "rb") as f:
        data = f.read()
    return sorted({m.decode() for m in re.findall(rb"hipv4-amdgcn-amd-amdhsa--(gfx[0-9a-z]+)", data)})


def lib():
    """Load the shared library (once).  Raises if it is missing — there is no CPU fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(pope_amd has no fallback path)")
        # torch FIRST: it ships its own HIP runtime (torch/lib/libamdhip64.so).  If libpope_hip.so is the first to
        # pull in a libamdhip64 (the system one), the process ends up with two runtimes and every launch of ours on a
        # torch stream fails — `build()` followed by `smoke()` in one process did exactly that
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(handle, name)  # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        if handle.pope_abi_version() != 10:
            raise RuntimeError("libpope_hip.so ABI version mismatch")
        _lib = handle
    return _lib


class PopeHipError(RuntimeError):
    pass


class PopeRangeError(PopeHipError):
    """An f16x3 operand left the f16 range (|activation| * 8 or |weight| * 256 >= 65504): results of that call are not
    valid; raised when the model's `on_overflow` policy is "raise" (the default policy re-runs on the fp32 MFMA)."""


def describe_range_bits(bits):
    return ", ".join(name for bit, name in RANGE_BITS.items() if bits & bit) or "none"


def check(status, what):
    if status != 0:
        raise PopeHipError(f"{what}: {lib().pope_error_string(status).decode()} (status {status})")


def to_planes(t, scale):
    """torch restatement of the planes layout (pope_hip.h): [rows, cols] fp32 -> f16 [rows, cols/32, 2, 32]
    with t*scale = hi + lo, hi = RNE f16."""
    ts = t.detach().float() * scale
    hi = ts.half()
    lo = (ts - hi.float()).half()
    r, c = t.shape
    import torch
    return torch.stack([hi.view(r, c // 32, 32), lo.view(r, c // 32, 32)], dim=2).contiguous()


def from_planes(pl, scale):
    """inverse of to_planes (fp32)."""
    r = pl.shape[0]
    return (pl[:, :, 0].float() + pl[:, :, 1].float()).reshape(r, -1) / scale


def params_key(tensors):
    """Cache key of everything derived from `tensors` (weight planes, folded BatchNorm, gathered tables): storage address AND
    torch's in-place modification counter of every source tensor, so `p.copy_()`, an optimizer / EMA step or `w[0, 0] = x`
    invalidates the derived data like a reallocation does."""
    return tuple((t.data_ptr(), t._version) for t in tensors)


def param_slots(module, buffers=False):
    """Where a module tree keeps its parameters (and buffers): [(the owning submodule's `_parameters` / `_buffers` dict, name)].
    Cached by the models as the source list of their derived data; the TENSORS are looked up through it on every call
    (`slots_key`), so a replaced Parameter object — `load_state_dict(..., assign=True)`, `m.weight = nn.Parameter(..)`,
    `.to()` — is seen like an in-place edit, at the price of one dict lookup per tensor instead of a walk over the module
    tree (0.35 ms for ViT-S/14).  Adding or removing SUBMODULES after the first call is not tracked."""
    slots = []
    for m in module.modules():
        slots += [(m._parameters, n) for n in m._parameters]
        if buffers:
            slots += [(m._buffers, n) for n in m._buffers]
    return slots


def slots_key(slots):
    """`params_key` of the tensors currently sitting in `slots` (None entries, e.g. `bias=None`, keyed as such)."""
    return tuple((t.data_ptr(), t._version) if t is not None else None for t in (d.get(n) for d, n in slots))


def param_ptr(t, keep, who):
    """Device pointer of an fp32 parameter (or a tensor derived from parameters) for a weights struct: detached, on a GPU, made
    contiguous and appended to `keep`, the list that keeps a struct's tensors alive."""
    import torch
    t = t.detach()
    if t.dtype != torch.float32:
        raise TypeError("pope_amd kernels take fp32 parameters")
    require_cuda(t, who)
    t = t.contiguous()
    keep.append(t)
    return C.c_void_p(t.data_ptr())


def grow_workspace(owner, need, device):
    """The grow-only byte workspace a module keeps in `owner._ws`, at least `need` bytes on `device`.  The old buffer is dropped
    before the new one is allocated (which is why this takes the owner and not the buffer: a caller's reference would keep the
    old one alive through the allocation)."""
    import torch
    ws = owner._ws
    if ws is None or ws.numel() < need or ws.device != device:
        ws = owner._ws = None
        ws = owner._ws = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def range_event(module, msg, note):
    """A range-guard event of a module with `overflow_events` and `on_overflow`: counted, then `PopeRangeError(msg)` under
    "raise", else a warning `msg + note` (the caller then re-runs in f32)."""
    module.overflow_events += 1
    if module.on_overflow == "raise":
        raise PopeRangeError(msg)
    import warnings
    warnings.warn(msg + note, stacklevel=2)   # reported at the caller's line, as when the caller warned itself


def ptr(t):
    """Device pointer of a contiguous fp32/int tensor (or None)."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError("pope_amd expects contiguous tensors")
    return C.c_void_p(t.data_ptr())


def padding_mask(m, shape, device, what):
    """A padding mask (bool, or 0 / 1 in an integer or float dtype) of exactly `shape`, as the contiguous fp32 0 / 1 tensor on
    `device` the kernels read; None stays None.  Anything else raises ValueError."""
    if m is None:
        return None
    import torch
    if not isinstance(m, torch.Tensor) or tuple(m.shape) != tuple(shape):
        raise ValueError(f"{what}: expected a padding mask of shape {tuple(shape)}, got {tuple(getattr(m, 'shape', ())) or type(m).__name__}")
    m = m.to(device)
    if m.dtype != torch.bool and (m.is_complex() or bool(((m != 0) & (m != 1)).any())):
        raise ValueError(f"{what}: padding masks are binary (bool, or 0 / 1)")
    return m.to(torch.float32).contiguous()


def pair_scale(s, n, device, what):
    """Per-pair (x, y) resize factors [n, 2] as a contiguous fp32 tensor on `device`; None stays None."""
    if s is None:
        return None
    import torch
    if not isinstance(s, torch.Tensor) or tuple(s.shape) != (n, 2) or s.is_complex():
        raise ValueError(f"{what}: expected per-pair (x, y) factors of shape ({n}, 2), got {tuple(getattr(s, 'shape', ())) or type(s).__name__}")
    return s.to(device=device, dtype=torch.float32).contiguous()


def stream_of(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def on_device_of(t):
    """Context manager: make `t`'s GPU the current HIP device around a C-ABI call.  torch hands out the NULL handle
    for every device's default stream, so the stream alone does not name the device (the reference keeps its matcher
    on cuda:1 while cuda:0 is current, pope_model_api.py:181-184); non-default streams are additionally resolved on
    the C side (stream_device.h:StreamDevice)."""
    import torch
    return torch.cuda.device(t.device)


def require_cuda(t, what):
    if not t.is_cuda:
        raise PopeHipError(
            f"{what}: tensor is on {t.device}; the pope_amd product path runs on the MI355X HIP kernels only "
            "(no CPU fallback) — move the model/inputs to 'cuda'")

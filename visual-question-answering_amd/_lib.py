"""ctypes binding of ``libcoattn_hip.so`` (C-ABI declared in ``include/coattn.h``, after 0.22.0 in ``include/coattn_ext.h``, the
recurrent entry points after 0.24.0 in ``include/coattn_rnn.h``, the fusion head of 0.26.0 in ``include/coattn_fusion.h``)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# COATTN_LIB_PATH: developer override for A/B timing of two builds; the product loads the in-tree library
LIB_PATH = os.environ.get("COATTN_LIB_PATH") or os.path.join(_HERE, "libcoattn_hip.so")
CSRC = os.path.join(_HERE, "csrc")

F32 = 0
IDS_I32, IDS_I64 = 0, 1   # ids_dtype of the word embedding calls (v0.18.0: COATTN_IDS_*)
BF16 = 1                  # storage type of coattn_features_native's input and of a bf16 feature table (coattn_features_gather)
IMPL_AUTO, IMPL_GENERAL, IMPL_FUSED = 0, 1, 2
FLAG_BF16_PROJ = 4
FLAG_BF16_IN = 8          # linear entry points: x (dy) stored as bf16
FLAG_EXACT3 = 16          # coattn_forward / coattn_backward: every contraction on the exact three-piece split (= flags 0: the default)
FLAG_SPLIT2 = 32          # linear entry points: the two-piece width (hi + mid, three partial products)
FLAG_F16PAIR = 64        # coattn_linear_forward: two FP16 pieces (the form the tolerance mode runs its projections in)
FLAG_FAST16 = 128        # coattn_forward / coattn_backward / coattn_phrase_*: the tolerance mode (forward products on two FP16
                         # pieces = 22 bits, backward on two bf16 pieces = 16 bits; range report: coattn_status)
OVERLAY_HEAT, OVERLAY_MASK = 0, 1   # mode of coattn_overlay_render (v0.21.0: COATTN_OVERLAY_*)
LOSS_SOFT_CE, LOSS_BCE = 1, 2   # loss kinds of the soft-answer-target calls (v0.12.0: COATTN_LOSS_*)
MAX_ANSWERS = 16         # answer slots per sample the soft-target kernels take
LOSS_KINDS = {"soft_ce": LOSS_SOFT_CE, "bce": LOSS_BCE}
FLAG_BILINEAR = 256      # every co-attention entry point: the affinity tanh((Q W_b^T + b_b) V^T) (v0.10.0; reads Params.W_b / b_b,
                         # writes ParamGrads.dW_b / db_b)


def precision_flag(fast: bool) -> int:
    return FLAG_FAST16 if fast else 0


def default_fast() -> bool:
    """The modules' default precision: exact fp32 products (the reference's arithmetic) unless VQA_PRECISION=fast;
    train.Trainer opts into the tolerance mode itself (precision="fast")."""
    return os.environ.get("VQA_PRECISION", "exact") == "fast"


class Params(C.Structure):
    # (W_b, b_b: appended in v0.10.0, read only under FLAG_BILINEAR; an 8-pointer Params(...) leaves them NULL)
    _fields_ = [(n, C.c_void_p) for n in ("W_v", "b_v", "W_q", "b_q", "w_v", "c_v", "w_q", "c_q", "W_b", "b_b")]


class ParamGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("dW_v", "db_v", "dW_q", "db_q", "dw_v", "dc_v", "dw_q", "dc_q", "dW_b", "db_b")]


# alternating co-attention (v0.11.0): the three guided-attention steps' parameters, in the header's order
ALT_PARAM_NAMES = ("W_x1", "b_x1", "w_h1", "c_h1", "W_x2", "b_x2", "W_g2", "b_g2", "w_h2", "c_h2",
                   "W_x3", "b_x3", "W_g3", "b_g3", "w_h3", "c_h3")


class AltParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ALT_PARAM_NAMES]


class AltParamGrads(C.Structure):
    _fields_ = [("d" + n, C.c_void_p) for n in ALT_PARAM_NAMES]


class PhraseParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("W1", "b1", "W2", "b2", "W3", "b3")]


class PhraseParamGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("dW1", "db1", "dW2", "db2", "dW3", "db3")]


class HeadParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("W_w", "b_w", "W_p", "b_p", "W_s", "b_s", "W_h", "b_h")]


class HeadParamGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("dW_w", "db_w", "dW_p", "db_p", "dW_s", "db_s", "dW_h", "db_h")]


class AdamTensor(C.Structure):
    # one entry of the optimiser step's list (v0.13.0): parameter, gradient, exp_avg, exp_avg_sq, elements
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64)]


class LstmParams(C.Structure):
    # the sentence LSTM (v0.17.0): nn.LSTM's weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0
    _fields_ = [(n, C.c_void_p) for n in ("w_ih", "w_hh", "b_ih", "b_hh")]


class LstmParamGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w_ih", "w_hh", "b_ih", "b_hh")]


class GruParams(C.Structure):
    # the question GRU of the baseline model (v0.25.0): nn.GRU's weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0
    _fields_ = [(n, C.c_void_p) for n in ("w_ih", "w_hh", "b_ih", "b_hh")]


class GruParamGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("w_ih", "w_hh", "b_ih", "b_hh")]


FUSION_PARAM_NAMES = ("W_i", "b_i", "W_q", "b_q", "W_m", "b_m", "W_f", "b_f")


class FusionParams(C.Structure):
    # the fusion head of the baseline model (v0.26.0): image_embedding, embedding_layer, mlp and fc_final as nn.Linear stores them
    _fields_ = [(n, C.c_void_p) for n in FUSION_PARAM_NAMES]


class FusionParamGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in FUSION_PARAM_NAMES]


class OverlayParams(C.Structure):
    # the attention overlays (v0.21.0): the image's normalisation, the two blend weights, the device pointer of the colour table
    _fields_ = [("mean", C.c_float * 3), ("std", C.c_float * 3), ("alpha", C.c_float), ("floor", C.c_float), ("lut", C.c_void_p)]


class GemmDesc(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("A", "B", "Cin", "C", "bias_n", "bias_m")]
                + [(n, C.c_int) for n in ("M", "N", "K", "batch", "inner", "inner_total", "ksplit", "act")]
                + [("beta", C.c_float)]
                + [(n, C.c_int64) for n in ("a_sm", "a_sk", "a_sz", "a_si", "a_mdiv", "a_sdiv",
                                            "b_sk", "b_sn", "b_sz", "b_si",
                                            "c_sm", "c_sn", "c_sz", "c_mdiv", "c_sdiv",
                                            "cin_sm", "cin_sn", "cin_sz", "cin_mdiv", "cin_sdiv")]
                + [("a_ptrs", C.c_void_p * 8), ("b_ptrs", C.c_void_p * 8), ("c_ptrs", C.c_void_p * 8),
                   ("cin_ptrs", C.c_void_p * 8), ("ptr_by_inner", C.c_int), ("b_imod", C.c_int),
                   ("kband_n", C.c_int), ("kband_lo", C.c_int * 3), ("kband_hi", C.c_int * 3),
                   ("out_scale", C.c_float)])

# ---- the C-ABI, argument by argument --------------------------------------------------------------------------------------
# SIGNATURES[symbol] = ((argument name, ctype), ...) for every function include/coattn.h declares, with its names and order
# (tests/test_call_layer_cpu.py holds every row against the header); RESTYPES the return types that are not int.  load() takes
# argtypes and restype from here, bind() turns keyword arguments into the positional tuple.  A new entry point is one row.
def _of(ctype):
    return lambda names: tuple((n, ctype) for n in names.split())


_void, _i64, _int, _ptrs = _of(C.c_void_p), _of(C.c_int64), _of(C.c_int), _of(C.POINTER(C.c_void_p))
_f64, _f32, _sizes, _floats = _of(C.c_double), _of(C.c_float), _of(C.POINTER(C.c_size_t)), _of(C.POINTER(C.c_float))


def _to(struct, name="p"):
    return ((name, C.POINTER(struct)),)


_V_Q = _void("V") + _i64("v_sB v_sN v_sD") + _ptrs("Q")
_LEN, _MAPS, _MAP_GRADS = _void("q_len"), _void("av_out aq_out"), _void("g_av g_aq")
_DIMS = _int("B N T d L dtype flags") + _void("stream")
_HEAD = _ptrs("v q") + _to(HeadParams)
_HEAD_DIMS = _int("B d mlp K dtype flags") + _void("stream")
_PHRASE_DIMS = _int("B T E dtype flags") + _void("stream")
_LSTM_DIMS = _int("B T E H dtype flags") + _void("stream")
_EMB_DIMS = _i64("n V") + _int("E") + _i64("padding_idx")
_BN_DIMS = _int("B H W C pool relu dtype") + _void("stream")
_THREE_SIZES = _sizes("saved ws_fwd ws_bwd")
CONV1_RECOMPUTE_CHUNK = 8   # COATTN_CONV1_RECOMPUTE_CHUNK: samples per workgroup of the recompute form's third kernel


def _forward(lens=(), maps=(), saved=_void("saved"), params=Params):
    return _V_Q + lens + _to(params) + _void("v_out q_out") + maps + saved + _void("ws") + _DIMS


def _backward(lens=(), maps=(), params=Params, grads=ParamGrads):
    return (_V_Q + lens + _to(params) + _void("saved gv gq") + maps + _void("dV") + _i64("dv_sB dv_sN dv_sD")
            + _ptrs("dQ") + _to(grads, "pg") + _int("accumulate") + _void("ws") + _DIMS)


def _conv1(outputs):
    return (_void("image weight gamma beta running_mean running_var") + _f64("momentum eps") + _void(outputs)
            + _void("save_mean save_invstd ws") + _int("B H W Cin Cout pool dtype") + _void("stream"))


SIGNATURES = {
    "coattn_version": (), "coattn_last_error": (),
    "coattn_profile_begin": _void("stream"),
    "coattn_profile_end": _floats("us") + _of(C.c_char_p)("names") + _int("names_bytes max_marks"),
    "coattn_features_native": _void("x") + _int("x_dtype") + _i64("sB sN sD") + _void("out") + _int("B N d") + _void("stream"),
    # the parallel and the alternating co-attention
    "coattn_fused_supported": _int("B N T d L dtype"),
    "coattn_workspace_bytes": _int("B N T d L dtype flags") + _THREE_SIZES,
    "coattn_alt_workspace_bytes": _int("B N T d L dtype flags") + _THREE_SIZES,
    "coattn_forward": _forward(), "coattn_forward_len": _forward(_LEN),
    "coattn_attention_forward": _forward(), "coattn_attention_forward_len": _forward(_LEN),
    "coattn_forward_maps": _forward(maps=_MAPS), "coattn_forward_maps_len": _forward(_LEN, _MAPS),
    "coattn_infer": _forward(maps=_MAPS, saved=()), "coattn_infer_len": _forward(_LEN, _MAPS, saved=()),
    "coattn_backward": _backward(), "coattn_backward_len": _backward(_LEN),
    "coattn_backward_maps": _backward(maps=_MAP_GRADS), "coattn_backward_maps_len": _backward(_LEN, _MAP_GRADS),
    "coattn_alt_forward": _forward(_LEN, _MAPS, params=AltParams),
    "coattn_alt_backward": _backward(_LEN, _MAP_GRADS, AltParams, AltParamGrads),
    "coattn_status": _void("saved") + _int("B N T d L dtype") + _void("stream") + _floats("amax"),
    "coattn_status_accumulate": _void("saved") + _int("B N T d L dtype") + _void("acc stream"),
    # the phrase level
    "coattn_phrase_workspace_bytes": _int("B T E dtype") + _THREE_SIZES,
    "coattn_phrase_forward": _void("X") + _to(PhraseParams) + _void("out saved ws") + _PHRASE_DIMS,
    "coattn_phrase_backward": (_void("X") + _to(PhraseParams) + _void("out saved g_out dX") + _to(PhraseParamGrads, "pg")
                               + _int("accumulate") + _void("ws") + _PHRASE_DIMS),
    "coattn_phrase_status": _void("saved") + _int("B T E") + _void("stream") + _floats("amax"),
    "coattn_phrase_status_accumulate": _void("saved") + _int("B T E") + _void("acc stream"),
    # the losses and the answer head
    "coattn_ce_workspace_bytes": _int("B K dtype") + _sizes("ws"),
    "coattn_ce_forward": _void("logits labels loss dlogits ws") + _int("B K dtype") + _void("stream"),
    "coattn_ce_status": _void("ws") + _int("B") + _void("stream"),
    "coattn_soft_loss_forward": (_void("logits ans_idx ans_score") + _int("A kind") + _void("loss dlogits ws") + _int("B K dtype")
                                 + _void("stream")),
    "coattn_vqa_score": (_void("logits ans_idx ans_score") + _int("A") + _void("pred row_score score_sum ws") + _int("B K dtype")
                         + _void("stream")),
    "coattn_head_workspace_bytes": _int("B d mlp K dtype") + _sizes("saved ws_bwd"),
    "coattn_head_forward": _HEAD + _void("labels logits loss saved") + _HEAD_DIMS,
    "coattn_head_forward_soft": (_HEAD + _void("ans_idx ans_score") + _int("A kind") + _void("logits loss saved")
                                 + _HEAD_DIMS),
    "coattn_head_backward": (_HEAD + _void("saved g_loss g_logits") + _ptrs("dv dq") + _to(HeadParamGrads, "pg")
                             + _int("accumulate") + _void("ws") + _HEAD_DIMS),
    "coattn_head_status": _void("saved") + _int("B d mlp K") + _void("stream"),
    # the optimiser step
    "coattn_adam_workspace_bytes": _to(AdamTensor, "t") + _int("n_tensors"),
    "coattn_adam_step": (_to(AdamTensor, "t") + _int("n_tensors step") + _f64("lr beta1 beta2 eps weight_decay max_grad_norm")
                         + _void("norm_out ws") + _of(C.c_size_t)("ws_bytes") + _void("stream")),
    # the frozen encoder
    "coattn_bn_supported": _int("B H W C pool dtype"),
    "coattn_bn_workspace_bytes": _int("B H W C"),
    "coattn_bn_relu_pool_forward": (_void("x gamma beta conv_bias running_mean running_var") + _f64("momentum eps")
                                    + _void("y stats_out ws") + _BN_DIMS),
    "coattn_relu_pool_forward": _void("x y") + _int("B H W C dtype") + _void("stream"),
    "coattn_bn_exact_geometry": _int("B H W C dtype") + _of(C.POINTER(C.c_int))("out"),
    "coattn_bn_exact_workspace_bytes": _int("B H W C"),
    "coattn_bn_exact_forward": (_void("x gamma beta running_mean running_var") + _f64("momentum eps")
                                + _void("y save_mean save_invstd ws") + _BN_DIMS),
    "coattn_conv1_bn_exact_supported": _int("B H W Cin Cout pool dtype"),
    "coattn_conv1_bn_exact_workspace_bytes": _int("B H W with_x"),
    "coattn_conv1_bn_exact_forward": _conv1("x_out y"),
    "coattn_conv1_probe": _void("image weight x ws") + _int("B H W order step halves skip") + _void("stream"),
    "coattn_conv1_bn_recompute_workspace_bytes": _int("B H W"),
    "coattn_conv1_bn_recompute_forward": _conv1("y"),
    # the sentence LSTM, the word embedding, feature dropout, cached features, overlays
    "coattn_lstm_supported": _int("B T E H dtype"),
    "coattn_lstm_workspace_bytes": _int("B T E H dtype") + _THREE_SIZES,
    "coattn_lstm_forward": _void("X len") + _to(LstmParams) + _void("out x_masked saved ws") + _LSTM_DIMS,
    "coattn_lstm_backward": (_void("X len") + _to(LstmParams) + _void("out saved g_out g_xmasked dX") + _to(LstmParamGrads, "pg")
                             + _int("accumulate") + _void("ws") + _LSTM_DIMS),
    "coattn_embedding_supported": _i64("n V") + _int("E dtype"),
    "coattn_embedding_workspace_bytes": _i64("n V") + _int("E dtype") + _sizes("ws_bwd"),
    "coattn_embedding_forward": (_void("ids") + _int("ids_dtype") + _void("W out bad_ids") + _EMB_DIMS + _int("dtype flags")
                                 + _void("stream")),
    "coattn_embedding_backward": (_void("ids") + _int("ids_dtype") + _void("g_out dW ws") + _EMB_DIMS
                                  + _int("accumulate dtype flags") + _void("stream")),
    "coattn_dropout_supported": _i64("n"),
    "coattn_dropout_forward": _void("x0 y0 x1 y1") + _i64("n") + _f32("p") + _void("state") + _int("advance") + _void("stream"),
    "coattn_dropout_backward": _void("g dx") + _i64("n") + _f32("p") + _void("state stream"),
    "coattn_features_gather_supported": _i64("S B") + _int("N d table_dtype flags"),
    "coattn_features_gather": (_void("table") + _int("table_dtype") + _void("idx") + _int("idx_dtype") + _void("out bad_idx")
                               + _i64("S B") + _int("N d flags") + _void("stream")),
    "coattn_overlay_supported": _int("B L H W Gh Gw T strip_h mode"),
    "coattn_overlay_render": (_void("image") + _i64("sB sC sH sW") + _void("a_v a_q q_len") + _to(OverlayParams)
                              + _void("out bad_maps") + _int("B L H W Gh Gw T strip_h mode") + _void("stream")),
    # the GEMM and linear building blocks, the peer-to-peer exchange
    "coattn_gemm_f32": _to(GemmDesc, "g") + _void("stream"), "coattn_gemm_bf16": _to(GemmDesc, "g") + _void("stream"),
    "coattn_linear_workspace_bytes": _int("N K"),
    "coattn_linear_forward": (_void("x") + _i64("ld_x") + _void("W bias y wimg") + _int("M N K") + _f32("out_scale") + _int("flags")
                              + _void("stream")),
    "coattn_linear_wgrad_workspace_bytes": _int("n_out n_in"),
    "coattn_linear_weight_grad": (_void("dy") + _i64("ld_dy") + _void("x") + _i64("ld_x") + _void("dW ws")
                                  + _int("M n_out n_in accumulate") + _void("stream")),
    "coattn_p2p_enable_peer": _int("peer_device"),
    "coattn_p2p_reduce_scatter": _ptrs("peer_bufs") + _int("world rank") + _i64("shard_elems") + _f32("scale") + _void("stream"),
    "coattn_p2p_all_gather": _ptrs("peer_bufs") + _int("world rank") + _i64("shard_elems") + _void("stream"),
}
RESTYPES = {"coattn_last_error": C.c_char_p}
RESTYPES.update(dict.fromkeys(("coattn_adam_workspace_bytes", "coattn_bn_workspace_bytes", "coattn_bn_exact_workspace_bytes",
                               "coattn_conv1_bn_exact_workspace_bytes", "coattn_conv1_bn_recompute_workspace_bytes",
                               "coattn_linear_workspace_bytes", "coattn_linear_wgrad_workspace_bytes"), C.c_size_t))
EXPORTS = tuple(SIGNATURES)   # every symbol include/coattn.h declares


class PreprocessDesc(C.Structure):
    # one image of coattn_preprocess_images (v0.23.0): where its pixels start, its size, where its two coefficient tables start
    _fields_ = [("offset", C.c_int64)] + [(n, C.c_int) for n in ("h", "w", "tab_x", "tab_y", "taps_x", "taps_y")]


PREPROCESS_ROWS, PREPROCESS_MAX_TAPS = 16, 1024   # COATTN_PREPROCESS_ROWS, COATTN_PREPROCESS_MAX_TAPS
# The entry points after 0.22.0, declared in include/coattn_ext.h: a second table of the same form (tests/test_preprocess_cpu.py
# holds it against that header).  SIGNATURES, RESTYPES and EXPORTS stay the 78 functions of include/coattn.h; load(), bind() and
# Call.replace() serve both tables.
EXT_SIGNATURES = {
    "coattn_preprocess_supported": _int("B S max_h max_w"),
    "coattn_preprocess_images": (_void("pixels") + _i64("pixel_bytes") + _void("desc coef") + _i64("coef_count") + _void("lut out")
                                 + _i64("sB sC sH sW") + _void("bad_images") + _int("B S max_h max_w") + _void("stream")),
    # the frozen encoder in eval mode (v0.24.0)
    "coattn_bn_eval_supported": _int("B H W C pool dtype"),
    "coattn_bn_eval_forward": (_void("x conv_bias gamma beta running_mean running_var") + _f64("eps") + _void("y") + _BN_DIMS),
    "coattn_conv1_bn_eval_supported": _int("B H W Cin Cout pool dtype"),
    "coattn_conv1_bn_eval_forward": (_void("image weight conv_bias gamma beta running_mean running_var") + _f64("eps") + _void("y")
                                     + _int("B H W Cin Cout pool dtype") + _void("stream")),
    "coattn_bn_eval_probe": (_void("x gamma beta running_mean running_var") + _f64("eps") + _void("y")
                             + _int("B H W C rsqrt step eps_mode") + _void("stream")),
}
EXT_RESTYPES = {}
EXT_EXPORTS = tuple(EXT_SIGNATURES)
# The recurrent entry points after 0.24.0, declared in include/coattn_rnn.h: a third table of the same form (tests/test_gru_cpu.py
# holds it against that header).  The two tables above keep their contents and order.
RNN_SIGNATURES = {
    # the question GRU of the baseline model (v0.25.0)
    "coattn_gru_supported": _int("B T E H dtype"),
    "coattn_gru_workspace_bytes": _int("B T E H dtype") + _THREE_SIZES,
    "coattn_gru_forward": _void("X len") + _to(GruParams) + _void("seq_out h_last saved ws") + _LSTM_DIMS,
    "coattn_gru_backward": (_void("X len") + _to(GruParams) + _void("saved g_seq g_last dX") + _to(GruParamGrads, "pg")
                            + _int("accumulate") + _void("ws") + _LSTM_DIMS),
}
RNN_RESTYPES = {}
RNN_EXPORTS = tuple(RNN_SIGNATURES)
# The fusion head of the baseline model (v0.26.0), declared in include/coattn_fusion.h: a fourth table of the same form
# (tests/test_fusion_cpu.py holds it against that header).  The three tables above keep their contents and order.
_FUSION_IN = _void("f") + _i64("ld_f") + _void("h") + _i64("ld_h") + _to(FusionParams)
_FUSION_DIMS = _int("B Di H J Mh K dtype flags") + _void("stream")
FUSION_SIGNATURES = {
    "coattn_fusion_supported": _int("B Di H J Mh K dtype"),
    "coattn_fusion_workspace_bytes": _int("B Di H J Mh K dtype") + _sizes("saved ws_bwd"),
    "coattn_fusion_forward": _FUSION_IN + _void("logits saved") + _f32("p_drop") + _void("drop_state") + _FUSION_DIMS,
    "coattn_fusion_backward": (_FUSION_IN + _void("saved g_logits dh") + _to(FusionParamGrads, "pg") + _int("accumulate")
                               + _f32("p_drop") + _void("drop_state ws") + _FUSION_DIMS),
}
FUSION_RESTYPES = {}
FUSION_EXPORTS = tuple(FUSION_SIGNATURES)
_ALL_SIGNATURES = {**SIGNATURES, **EXT_SIGNATURES, **RNN_SIGNATURES, **FUSION_SIGNATURES}
_ALL_RESTYPES = {**RESTYPES, **EXT_RESTYPES, **RNN_RESTYPES, **FUSION_RESTYPES}
_INDEX = {name: {n: i for i, (n, _) in enumerate(sig)} for name, sig in _ALL_SIGNATURES.items()}
# what bind() fills in for an argument it is not given: NULL for the pointers the header lets be NULL, 0 for dV's strides
_DEFAULTS = dict.fromkeys(("q_len av_out aq_out saved g_av g_aq dV labels loss g_loss g_logits dv dq bad_ids bad_idx x1 y1 bad_maps "
                           "conv_bias stats_out x_out dlogits x_masked g_xmasked dX bad_images h_last g_seq g_last dh drop_state").split())
_DEFAULTS.update(dv_sB=0, dv_sN=0, dv_sD=0)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def ptr_array(tensors):
    """Host array of the tensors' device pointers (`Q`, `dQ`)."""
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def rows(t):
    """Host array of the three [B,d] row-block pointers of a contiguous [3,B,d] tensor (the head's `v`, `q`, `dv`)."""
    step = t.stride(0) * t.element_size()
    return (C.c_void_p * 3)(*[t.data_ptr() + l * step for l in range(3)])


def stream_ptr(dev) -> int:
    """The hipStream_t of torch's current stream on `dev`."""
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


def _as_arg(value, ctype):
    if hasattr(value, "data_ptr"):                       # a tensor: its device pointer
        return C.c_void_p(value.data_ptr())
    if isinstance(value, C.Structure):                   # (the byref object keeps the structure alive)
        return C.byref(value)
    if ctype is C.c_void_p and isinstance(value, int):
        return C.c_void_p(value)
    return value


class Call(tuple):
    """The positional arguments of the entry point `name`, as bind() lays them out.  call() issues it and raises on an error
    code, call.code() issues it and returns the code (the status calls: -2 is theirs to interpret); a call bound without
    `stream` (always the last argument) takes it then: call(stream).  The tuple keeps the host arrays and structures it points
    to alive."""

    def code(self, *stream) -> int:
        return self.fn(*self, *stream)

    def __call__(self, *stream):
        check(self.code(*stream), self.name)

    def replace(self, **kw):
        """The same call with the given arguments replaced (one list copy: cheap enough for every step)."""
        sig, index, vals = _ALL_SIGNATURES[self.name], _INDEX[self.name], list(self)
        for n, v in kw.items():
            if n not in index:
                raise TypeError("%s has no argument %r" % (self.name, n))
            i = index[n]
            vals[i:i + 1] = [_as_arg(v, sig[i][1])]          # (i == len(vals): a `stream` left out so far)
        return _call(self.name, vals)


def _call(name, vals):
    call = Call(vals)
    call.name, call.fn = name, getattr(load(), name)
    return call


def bind(name: str, **kw) -> Call:
    """The call of SIGNATURES[name] (or EXT_SIGNATURES[name], RNN_SIGNATURES[name], FUSION_SIGNATURES[name]) with its arguments given by name: tensors go in as their device
    pointers, ctypes structures by reference, None as NULL; an omitted nullable pointer is NULL, an omitted dV stride 0, `stream` may be left
    for the call itself.  Raises TypeError on a name the entry point does not have and on a missing required one."""
    unknown = kw.keys() - _INDEX[name].keys()
    if unknown:
        raise TypeError("%s has no argument %s" % (name, ", ".join(sorted(unknown))))
    vals = []
    for n, ctype in _ALL_SIGNATURES[name]:
        if n in kw:
            vals.append(_as_arg(kw[n], ctype))
        elif n in _DEFAULTS:
            vals.append(_DEFAULTS[n])
        elif n != "stream":
            raise TypeError("%s: missing argument %r" % (name, n))
    return _call(name, vals)


def build(verbose: bool = False) -> str:
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", CSRC, "-j", "4"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout)
    if r.returncode != 0:
        raise RuntimeError("building libcoattn_hip.so failed")
    return LIB_PATH


_lib = None


def load() -> C.CDLL:
    """Load the library (after torch, so that the HIP runtime torch ships is the one bound)."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  -- must be imported first: one HIP runtime per process

    if not os.path.isfile(LIB_PATH):
        raise RuntimeError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the co-attention path)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, sig in _ALL_SIGNATURES.items():
        if not hasattr(lib, name):
            raise RuntimeError("libcoattn_hip.so lacks symbol %s" % name)
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = [ctype for _, ctype in sig], _ALL_RESTYPES.get(name, C.c_int)
    _lib = lib
    return lib


class RangeError(FloatingPointError):
    """An operand of the tolerance mode (FLAG_FAST16) left the exact range of its two FP16 pieces: the call's results are
    clamped, not within tolerance of the reference.  Use the exact mode (the modules' default; Trainer(precision="exact"))."""


F16_EXACT = 65504.0

# Range report of the tolerance mode, sticky: every tolerance-mode forward notes where its status words are (note_status),
# and the note is folded -- asynchronously, one tiny launch on the stream the forward ran on -- into a two-float accumulator
# per device (include/coattn.h coattn_status_accumulate); check_range() reads the accumulators back (synchronising), clears
# them and raises if ANY forward since the last check left the FP16-piece range.  A later forward, a validate() pass or a
# second model cannot overwrite an earlier call's report: the accumulator only grows until it is read.
_pending = []                 # (kind, tensor holding the status words, dims, device, stream pointer)
_range_acc = {}               # device index -> float32[2] accumulator


def note_status(kind: str, buf, dims, dev) -> None:
    import torch
    _pending.append((kind, buf, dims, dev, torch.cuda.current_stream(dev).cuda_stream))
    # folded right away, behind the forward on its own stream: the holder may be a static buffer (graph.py) or the
    # per-stream scratch (forward without `saved`), which the next call rewrites -- except while the stream is being
    # captured into a graph (the note then waits for the first fold outside the capture)
    if not torch.cuda.is_current_stream_capturing():
        fold_range()


def _acc(dev):
    import torch
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    a = _range_acc.get(key)
    if a is None:
        a = _range_acc[key] = torch.zeros(2, device=dev, dtype=torch.float32)
    return a


def fold_range() -> None:
    """Fold the status words of every tolerance-mode forward noted since the last fold into the per-device accumulators.
    Asynchronous (one 256-thread launch per call, on the stream the call ran on)."""
    while _pending:
        kind, buf, dims, dev, st = _pending.pop(0)
        with on_device(dev):
            status_accumulate(kind, buf, dims, _acc(dev), st)()


def status_accumulate(kind, saved, dims, acc, stream) -> Call:
    """The fold of one forward's status words into `acc`: coattn_status_accumulate over dims (B, N, T, d, L) for kind "coattn",
    coattn_phrase_status_accumulate over (B, T, E) otherwise."""
    if kind == "coattn":
        B, N, T, d, L = dims
        return bind("coattn_status_accumulate", saved=saved, B=B, N=N, T=T, d=d, L=L, dtype=F32, acc=acc, stream=stream)
    B, T, E = dims
    return bind("coattn_phrase_status_accumulate", saved=saved, B=B, T=T, E=E, acc=acc, stream=stream)


def range_maxima(reset: bool = True):
    """(largest out-of-range |activation|, largest |256 W|) over every tolerance-mode forward since the last reset, over
    all devices of this process.  Synchronises."""
    fold_range()
    act = wgt = 0.0
    for a in _range_acc.values():
        h = a.cpu()                                      # (synchronises the device)
        x, w = float(h[0]), float(h[1])
        act = x if (x > act or x != x) else act
        wgt = w if (w > wgt or w != w) else wgt
        if reset:
            a.zero_()
    return act, wgt


def check_range(stream=None) -> None:
    """Raise RangeError if ANY tolerance-mode co-attention / phrase forward since the last check met an operand outside the
    FP16-piece range (include/coattn.h, coattn_status_accumulate).  Synchronises -- call it where the host reads the loss.
    (`stream` is accepted for compatibility with v0.6.0 callers and ignored: every note is folded on the stream of its own
    forward.)"""
    del stream
    act, wgt = range_maxima()
    bad_a, bad_w = not (act <= F16_EXACT), not (wgt <= F16_EXACT)
    if bad_a or bad_w:
        raise RangeError("FP16-piece range exceeded in a tolerance-mode forward (COATTN_FLAG_FAST16): %s%s%s -- pieces were "
                         "clamped; use the exact mode (largest activation beyond the range %.4g, largest 256*|W| %.4g)"
                         % ("an activation (feature or stored projection) of magnitude > 65504" if bad_a else "",
                            " and " if bad_a and bad_w else "",
                            "a projection weight of magnitude > 255.87" if bad_w else "", act, wgt))


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, load().coattn_last_error().decode()))


def check_label_status(call: Call) -> None:
    """Issue a bound coattn_ce_status / coattn_head_status (they synchronise the stream): IndexError with the library's message
    for -2, a label or answer index out of range; any other code as check()."""
    rc = call.code()
    if rc == -2:
        raise IndexError(load().coattn_last_error().decode())
    check(rc, call.name)


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NO_GUARD = _NoGuard()


def on_device(dev):
    """Context manager that makes `dev` the current device for the C-ABI call inside (per-device one-time kernel
    attributes are keyed by it) -- a no-op object when it already is: ``torch.cuda.device`` costs ~10 us of host time per
    entry, the hot path enters it four times per step."""
    import torch
    return _NO_GUARD if dev.index is None or dev.index == torch.cuda.current_device() else torch.cuda.device(dev)


_bytes_cache = {}


def _bytes(symbol, n_out, *dims):
    """The n_out byte counts the *_workspace_bytes entry point `symbol` reports for `dims`; cached (the plan is a pure
    function of the shape)."""
    key = (symbol, *dims)
    hit = _bytes_cache.get(key)
    if hit is None:
        out = [C.c_size_t() for _ in range(n_out)]
        check(getattr(load(), symbol)(*dims, *[C.byref(o) for o in out]), symbol)
        hit = _bytes_cache[key] = tuple(o.value for o in out)
    return hit


def size_bytes(symbol, *args) -> int:
    """The byte count of a *_workspace_bytes entry point that returns size_t; 0 for a shape or list it does not take."""
    return getattr(load(), symbol)(*args)


def phrase_workspace_bytes(B, T, E):
    """(saved, ws_fwd, ws_bwd) in bytes of the phrase level."""
    return _bytes("coattn_phrase_workspace_bytes", 3, B, T, E, F32)


def ce_workspace_bytes(B, K):
    """ws in bytes of the cross entropy, the soft-target losses and the score."""
    return _bytes("coattn_ce_workspace_bytes", 1, B, K, F32)[0]


def workspace_bytes(B, N, T, d, L, flags=0):
    """(saved, ws_fwd, ws_bwd) in bytes of the parallel co-attention."""
    return _bytes("coattn_workspace_bytes", 3, B, N, T, d, L, F32, flags)


def alt_workspace_bytes(B, N, T, d, L):
    """(saved, ws_fwd, ws_bwd) in bytes of the alternating co-attention (exact mode)."""
    return _bytes("coattn_alt_workspace_bytes", 3, B, N, T, d, L, F32, 0)


def lstm_workspace_bytes(B, T, E, H):
    """(saved, ws_fwd, ws_bwd) in bytes of the sentence LSTM."""
    return _bytes("coattn_lstm_workspace_bytes", 3, B, T, E, H, F32)


def gru_workspace_bytes(B, T, E, H):
    """(saved, ws_fwd, ws_bwd) in bytes of the question GRU."""
    return _bytes("coattn_gru_workspace_bytes", 3, B, T, E, H, F32)


def fusion_workspace_bytes(B, Di, H, J, Mh, K):
    """(saved, ws_bwd) in bytes of the baseline model's fusion head."""
    return _bytes("coattn_fusion_workspace_bytes", 2, B, Di, H, J, Mh, K, F32)


def embedding_workspace_bytes(n, V, E):
    """ws_bwd in bytes of the word embedding's backward (no term in V E)."""
    return _bytes("coattn_embedding_workspace_bytes", 1, n, V, E, F32)[0]


def head_workspace_bytes(B, d, mlp, K):
    """(saved, ws_bwd) in bytes of the answer head."""
    return _bytes("coattn_head_workspace_bytes", 2, B, d, mlp, K, F32)


_scratch = {}
_SCRATCH_MAX_STREAMS = 8


def scratch(nbytes: int, device, stream_ptr: int):
    """Scratch workspace (contents undefined after a call) kept per (device, stream): calls on one stream run in
    order, so they can share it; grown on demand.  At most _SCRATCH_MAX_STREAMS buffers are kept (least recently used
    dropped: a process that touches many short-lived streams does not pile up workspaces), and nothing is cached while
    the stream is capturing a graph (the allocation then belongs to the graph's private pool)."""
    import torch
    if torch.cuda.is_current_stream_capturing():
        return torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)
    key = (device.index if device.index is not None else torch.cuda.current_device(), stream_ptr)
    buf = _scratch.pop(key, None)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)
    _scratch[key] = buf                                  # (re-inserted last: dict order = recency)
    while len(_scratch) > _SCRATCH_MAX_STREAMS:
        _scratch.pop(next(iter(_scratch)))
    return buf

"""What vqa_amd._lib.load() declares to ctypes for every function of include/coattn.h: the argtypes and the restype, held against
a literal record of what load() set before its hand-counted argtypes lists became rows of _lib.SIGNATURES.  bench.py, the tools
and many tests call the library positionally: a row that changes a type changes their calls."""
import ctypes as C

import pytest

import vqa_amd  # noqa: F401
from vqa_amd import _lib

NAMES = {C.c_int: "int", C.c_int64: "i64", C.c_size_t: "size_t", C.c_double: "double", C.c_float: "float", C.c_void_p: "void_p",
         C.c_char_p: "char_p"}
NAMES.update({C.POINTER(t): n + "*" for t, n in list(NAMES.items())})
NAMES.update({C.POINTER(t): t.__name__ + "*" for t in (_lib.Params, _lib.ParamGrads, _lib.AltParams, _lib.AltParamGrads,
                                                       _lib.PhraseParams, _lib.PhraseParamGrads, _lib.HeadParams,
                                                       _lib.HeadParamGrads, _lib.AdamTensor, _lib.LstmParams, _lib.LstmParamGrads,
                                                       _lib.OverlayParams, _lib.GemmDesc)})
# symbol: (restype, argtypes) as load() set them before; argtypes None: none were set (the two functions without parameters,
# which now get the empty list).  No restype differs: every size_t function already had its c_size_t.
BEFORE = {
    "coattn_version": ("int", None),
    "coattn_last_error": ("char_p", None),
    "coattn_fused_supported": ("int", "int int int int int int"),
    "coattn_workspace_bytes": ("int", "int int int int int int int size_t* size_t* size_t*"),
    "coattn_forward": ("int", "void_p i64 i64 i64 void_p* Params* void_p void_p void_p void_p int int int int int int int void_p"),
    "coattn_attention_forward": ("int", "void_p i64 i64 i64 void_p* Params* void_p void_p void_p void_p int int int int int int int void_p"),
    "coattn_backward": ("int", "void_p i64 i64 i64 void_p* Params* void_p void_p void_p void_p i64 i64 i64 void_p* ParamGrads* int void_p int int int int int int int void_p"),
    "coattn_gemm_f32": ("int", "GemmDesc* void_p"),
    "coattn_gemm_bf16": ("int", "GemmDesc* void_p"),
    "coattn_phrase_workspace_bytes": ("int", "int int int int size_t* size_t* size_t*"),
    "coattn_phrase_forward": ("int", "void_p PhraseParams* void_p void_p void_p int int int int int void_p"),
    "coattn_phrase_backward": ("int", "void_p PhraseParams* void_p void_p void_p void_p PhraseParamGrads* int void_p int int int int int void_p"),
    "coattn_ce_workspace_bytes": ("int", "int int int size_t*"),
    "coattn_ce_forward": ("int", "void_p void_p void_p void_p void_p int int int void_p"),
    "coattn_linear_workspace_bytes": ("size_t", "int int"),
    "coattn_linear_forward": ("int", "void_p i64 void_p void_p void_p void_p int int int float int void_p"),
    "coattn_linear_wgrad_workspace_bytes": ("size_t", "int int"),
    "coattn_linear_weight_grad": ("int", "void_p i64 void_p i64 void_p void_p int int int int void_p"),
    "coattn_head_workspace_bytes": ("int", "int int int int int size_t* size_t*"),
    "coattn_head_forward": ("int", "void_p* void_p* HeadParams* void_p void_p void_p void_p int int int int int int void_p"),
    "coattn_head_backward": ("int", "void_p* void_p* HeadParams* void_p void_p void_p void_p* void_p* HeadParamGrads* int void_p int int int int int int void_p"),
    "coattn_head_status": ("int", "void_p int int int int void_p"),
    "coattn_ce_status": ("int", "void_p int void_p"),
    "coattn_p2p_enable_peer": ("int", "int"),
    "coattn_p2p_reduce_scatter": ("int", "void_p* int int i64 float void_p"),
    "coattn_p2p_all_gather": ("int", "void_p* int int i64 void_p"),
    "coattn_profile_begin": ("int", "void_p"),
    "coattn_profile_end": ("int", "float* char_p int int"),
    "coattn_features_native": ("int", "void_p int i64 i64 i64 void_p int int int void_p"),
    "coattn_status": ("int", "void_p int int int int int int void_p float*"),
    "coattn_phrase_status": ("int", "void_p int int int void_p float*"),
    "coattn_status_accumulate": ("int", "void_p int int int int int int void_p void_p"),
    "coattn_phrase_status_accumulate": ("int", "void_p int int int void_p void_p"),
    "coattn_infer": ("int", "void_p i64 i64 i64 void_p* Params* void_p void_p void_p void_p void_p int int int int int int int void_p"),
    "coattn_forward_len": ("int", "void_p i64 i64 i64 void_p* void_p Params* void_p void_p void_p void_p int int int int int int int void_p"),
    "coattn_infer_len": ("int", "void_p i64 i64 i64 void_p* void_p Params* void_p void_p void_p void_p void_p int int int int int int int void_p"),
    "coattn_attention_forward_len": ("int", "void_p i64 i64 i64 void_p* void_p Params* void_p void_p void_p void_p int int int int int int int void_p"),
    "coattn_backward_len": ("int", "void_p i64 i64 i64 void_p* void_p Params* void_p void_p void_p void_p i64 i64 i64 void_p* ParamGrads* int void_p int int int int int int int void_p"),
    "coattn_forward_maps": ("int", "void_p i64 i64 i64 void_p* Params* void_p void_p void_p void_p void_p void_p int int int int int int int void_p"),
    "coattn_forward_maps_len": ("int", "void_p i64 i64 i64 void_p* void_p Params* void_p void_p void_p void_p void_p void_p int int int int int int int void_p"),
    "coattn_backward_maps": ("int", "void_p i64 i64 i64 void_p* Params* void_p void_p void_p void_p void_p void_p i64 i64 i64 void_p* ParamGrads* int void_p int int int int int int int void_p"),
    "coattn_backward_maps_len": ("int", "void_p i64 i64 i64 void_p* void_p Params* void_p void_p void_p void_p void_p void_p i64 i64 i64 void_p* ParamGrads* int void_p int int int int int int int void_p"),
    "coattn_alt_workspace_bytes": ("int", "int int int int int int int size_t* size_t* size_t*"),
    "coattn_alt_forward": ("int", "void_p i64 i64 i64 void_p* void_p AltParams* void_p void_p void_p void_p void_p void_p int int int int int int int void_p"),
    "coattn_alt_backward": ("int", "void_p i64 i64 i64 void_p* void_p AltParams* void_p void_p void_p void_p void_p void_p i64 i64 i64 void_p* AltParamGrads* int void_p int int int int int int int void_p"),
    "coattn_soft_loss_forward": ("int", "void_p void_p void_p int int void_p void_p void_p int int int void_p"),
    "coattn_vqa_score": ("int", "void_p void_p void_p int void_p void_p void_p void_p int int int void_p"),
    "coattn_head_forward_soft": ("int", "void_p* void_p* HeadParams* void_p void_p int int void_p void_p void_p int int int int int int void_p"),
    "coattn_adam_workspace_bytes": ("size_t", "AdamTensor* int"),
    "coattn_adam_step": ("int", "AdamTensor* int int double double double double double double void_p void_p size_t void_p"),
    "coattn_bn_supported": ("int", "int int int int int int"),
    "coattn_bn_workspace_bytes": ("size_t", "int int int int"),
    "coattn_bn_relu_pool_forward": ("int", "void_p void_p void_p void_p void_p void_p double double void_p void_p void_p int int int int int int int void_p"),
    "coattn_relu_pool_forward": ("int", "void_p void_p int int int int int void_p"),
    "coattn_bn_exact_geometry": ("int", "int int int int int int*"),
    "coattn_bn_exact_workspace_bytes": ("size_t", "int int int int"),
    "coattn_bn_exact_forward": ("int", "void_p void_p void_p void_p void_p double double void_p void_p void_p void_p int int int int int int int void_p"),
    "coattn_conv1_bn_exact_supported": ("int", "int int int int int int int"),
    "coattn_conv1_bn_exact_workspace_bytes": ("size_t", "int int int int"),
    "coattn_conv1_bn_exact_forward": ("int", "void_p void_p void_p void_p void_p void_p double double void_p void_p void_p void_p void_p int int int int int int int void_p"),
    "coattn_conv1_probe": ("int", "void_p void_p void_p void_p int int int int int int int void_p"),
    "coattn_conv1_bn_recompute_workspace_bytes": ("size_t", "int int int"),
    "coattn_conv1_bn_recompute_forward": ("int", "void_p void_p void_p void_p void_p void_p double double void_p void_p void_p void_p int int int int int int int void_p"),
    "coattn_lstm_supported": ("int", "int int int int int"),
    "coattn_lstm_workspace_bytes": ("int", "int int int int int size_t* size_t* size_t*"),
    "coattn_lstm_forward": ("int", "void_p void_p LstmParams* void_p void_p void_p void_p int int int int int int void_p"),
    "coattn_lstm_backward": ("int", "void_p void_p LstmParams* void_p void_p void_p void_p void_p LstmParamGrads* int void_p int int int int int int void_p"),
    "coattn_embedding_supported": ("int", "i64 i64 int int"),
    "coattn_embedding_workspace_bytes": ("int", "i64 i64 int int size_t*"),
    "coattn_embedding_forward": ("int", "void_p int void_p void_p void_p i64 i64 int i64 int int void_p"),
    "coattn_embedding_backward": ("int", "void_p int void_p void_p void_p i64 i64 int i64 int int int void_p"),
    "coattn_dropout_supported": ("int", "i64"),
    "coattn_dropout_forward": ("int", "void_p void_p void_p void_p i64 float void_p int void_p"),
    "coattn_dropout_backward": ("int", "void_p void_p i64 float void_p void_p"),
    "coattn_features_gather_supported": ("int", "i64 i64 int int int int"),
    "coattn_features_gather": ("int", "void_p int void_p int void_p void_p i64 i64 int int int void_p"),
    "coattn_overlay_supported": ("int", "int int int int int int int int int"),
    "coattn_overlay_render": ("int", "void_p i64 i64 i64 i64 void_p void_p void_p OverlayParams* void_p void_p int int int int int int int int int void_p"),
}


def test_the_record_covers_every_export():
    assert set(BEFORE) == set(_lib.EXPORTS) and len(BEFORE) == 78


@pytest.mark.parametrize("name", sorted(BEFORE))
def test_load_sets_the_argtypes_and_restype_it_set_before(name):
    restype, argtypes = BEFORE[name]
    fn = getattr(_lib.load(), name)
    assert [NAMES[t] for t in fn.argtypes] == (argtypes or "").split(), name
    assert NAMES[fn.restype] == restype, name
    if argtypes is None:
        assert fn.argtypes == [] and name in ("coattn_version", "coattn_last_error")

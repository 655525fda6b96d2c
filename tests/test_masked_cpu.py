"""Length-masked question attention (C-ABI 0.8.0, the *_len entry points), on the CPU: declarations and exports, the
command line flag, the model plumbing and the refusals that need no GPU."""
import ctypes
import os
import re

import pytest
import torch

NEW = ("coattn_forward_len", "coattn_infer_len", "coattn_attention_forward_len", "coattn_backward_len")


def test_masked_entry_points_declared_exported_and_versioned():
    from vqa_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib.CSRC.rstrip("/")), "..", "include", "coattn.h")).read()
    declared = set(re.findall(r"\b(coattn_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.coattn_version() >= 800
    # every masked form takes the lengths right after Q, and the header says that NULL means unmasked
    for name in NEW:
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, hdr).group(1)
        args = [a.strip() for a in decl.split(",")]
        assert args[4].endswith("Q") and args[5] == "const int32_t* q_len", (name, args[4:6])
    assert "NULL = unmasked" in hdr and "CLAMPED" in hdr


def test_question_mask_flag_parses_with_default_false():
    from vqa_amd import predict as Pr
    from vqa_amd import train as T
    assert T.build_parser().parse_args([]).question_mask is False
    assert T.build_parser().parse_args(["--question_mask", "true"]).question_mask is True
    assert T.build_parser().parse_args(["--question_mask", "false"]).question_mask is False
    assert Pr.build_parser().parse_args(["--question_mask", "true"]).question_mask is True     # predict inherits it
    assert "state_dict" in T.build_parser().format_help().replace("\n", " ")


def test_build_model_sets_the_module_flag_and_keeps_the_state_dict_keys():
    from vqa_amd import train as T
    torch.manual_seed(0)
    plain = T.build_model("attention", 50, 4)
    masked = T.build_model("attention", 50, 4, question_mask=True)
    assert plain.co_attention.question_mask is False and masked.co_attention.question_mask is True
    assert list(plain.state_dict()) == list(masked.state_dict())
    args = T.build_parser().parse_args(["--question_mask", "true", "--vocab_size", "50", "--num_cls", "4"])
    model, _ = T.model_from_args(args)
    assert model.co_attention.question_mask is True
    with pytest.raises(ValueError, match="question_mask"):
        T.build_model("baseline", 50, 4, question_mask=True)
    assert not hasattr(T.build_model("baseline", 50, 4), "co_attention")


def test_question_mask_requires_lengths_and_checks_them():
    import vqa_amd
    from vqa_amd.coattention import question_lengths
    m = vqa_amd.ParallelCoAttention(64, question_mask=True)
    assert m.question_mask is True and vqa_amd.ParallelCoAttention(64).question_mask is False
    assert list(m.state_dict()) == list(vqa_amd.ParallelCoAttention(64).state_dict())
    x = torch.zeros(2, 5, 64)
    qs = [torch.zeros(2, 4, 64)] * 3
    with pytest.raises(ValueError, match="x_ques_lens"):
        m(x, qs)
    with pytest.raises(ValueError, match="shape"):
        question_lengths([3, 4, 1], 2, "cpu")
    with pytest.raises(TypeError, match="integers"):
        question_lengths(torch.tensor([1.0, 2.0]), 2, "cpu")
    t = question_lengths(torch.tensor([4, 2]), 2, "cpu")
    assert t.dtype == torch.int32 and t.tolist() == [4, 2]
    assert question_lengths([0, 9], 2, "cpu").tolist() == [0, 9]          # (values are clamped by the kernels, not here)


def test_masked_entry_points_reject_bad_shapes():
    from vqa_amd import _lib
    lib = _lib.load()
    L = 3
    q = (ctypes.c_void_p * L)(*([0] * L))
    p = _lib.Params()
    pg = _lib.ParamGrads()
    null = ctypes.c_void_p(0)
    for B, N, T, d, what in ((0, 49, 26, 512, b"batch"), (4, 49, 0, 512, b"T="), (4, 49, 26, 0, b"hidden")):
        rc = lib.coattn_forward_len(null, 0, 0, 0, q, null, ctypes.byref(p), null, null, null, null,
                                    B, N, T, d, L, _lib.F32, 0, null)
        assert rc < 0 and what in lib.coattn_last_error(), (rc, lib.coattn_last_error())
        rc = lib.coattn_infer_len(null, 0, 0, 0, q, null, ctypes.byref(p), null, null, null, null, null,
                                  B, N, T, d, L, _lib.F32, 0, null)
        assert rc < 0 and what in lib.coattn_last_error()
        rc = lib.coattn_attention_forward_len(null, 0, 0, 0, q, null, ctypes.byref(p), null, null, ctypes.c_void_p(16),
                                              null, B, N, T, d, L, _lib.F32, 0, null)
        assert rc < 0 and what in lib.coattn_last_error()
        rc = lib.coattn_backward_len(null, 0, 0, 0, q, null, ctypes.byref(p), null, null, null, null, 0, 0, 0, q,
                                     ctypes.byref(pg), 0, null, B, N, T, d, L, _lib.F32, 0, null)
        assert rc < 0 and what in lib.coattn_last_error()
    # null operands with a good shape: refused before anything is enqueued
    rc = lib.coattn_forward_len(null, 0, 0, 0, q, null, ctypes.byref(p), null, null, null, null,
                                4, 49, 26, 512, L, _lib.F32, 0, null)
    assert rc < 0 and b"null" in lib.coattn_last_error()
    rc = lib.coattn_attention_forward_len(null, 0, 0, 0, q, null, ctypes.byref(p), null, null, null, null,
                                          4, 49, 26, 512, L, _lib.F32, 0, null)
    assert rc < 0 and b"saved" in lib.coattn_last_error()

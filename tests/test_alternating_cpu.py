"""The alternating co-attention's surface without a GPU: the C-ABI declarations (include/coattn.h v0.11.0) and their ctypes
mirrors, the module's parameters, the CLI switch and its refusals, and the refusal of CPU tensors."""
import os
import re

import pytest
import torch

import vqa_amd
from vqa_amd import _lib
from vqa_amd import train as T

from tests import _alternating as AL

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "coattn.h")


def _struct_fields(hdr, name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S)
    assert m, name
    return re.findall(r"\*\s*(\w+);", m.group(1))


def test_header_declares_the_calls_and_structs():
    hdr = open(HDR).read()
    for fn in ("coattn_alt_workspace_bytes", "coattn_alt_forward", "coattn_alt_backward"):
        assert re.search(r"\bint %s\(" % fn, hdr), fn
        assert fn in _lib.EXPORTS
    assert _struct_fields(hdr, "coattn_alt_params") == list(AL.NAMES)
    assert _struct_fields(hdr, "coattn_alt_param_grads") == ["d" + n for n in AL.NAMES]


def test_ctypes_structs_follow_the_header():
    hdr = open(HDR).read()
    assert [f for f, _ in _lib.AltParams._fields_] == _struct_fields(hdr, "coattn_alt_params")
    assert [f for f, _ in _lib.AltParamGrads._fields_] == _struct_fields(hdr, "coattn_alt_param_grads")
    assert len(_lib.AltParams._fields_) == 16
    # the parallel form's structs are untouched
    assert len(_lib.Params._fields_) == 10 and len(_lib.ParamGrads._fields_) == 10


def test_version_and_workspace_sizes():
    lib = _lib.load()
    assert lib.coattn_version() >= 1100
    s, f, b = _lib.alt_workspace_bytes(160, 196, 26, 512, 3)
    assert s > 0 and f > s and b > 0
    import ctypes as C
    z = C.c_size_t()
    for flags in (_lib.FLAG_FAST16, _lib.FLAG_BF16_PROJ, _lib.FLAG_BILINEAR):
        assert lib.coattn_alt_workspace_bytes(4, 7, 5, 64, 3, 0, flags, C.byref(z), None, None) < 0
        assert b"flags" in lib.coattn_last_error()


def test_module_state_dict_keys_and_shapes():
    d = 24
    m = vqa_amd.AlternatingCoAttention(d)
    sd = m.state_dict()
    assert [AL.state_key(n) for n in AL.NAMES] == list(sd.keys())
    for k, t in sd.items():
        if k.startswith("W_"):
            assert tuple(t.shape) == ((d, d) if k.endswith("weight") else (d,)), k
        else:
            assert tuple(t.shape) == ((1, d) if k.endswith("weight") else (1,)), k
    # a parallel checkpoint does not load into the alternating form (nor the other way round)
    with pytest.raises(RuntimeError):
        m.load_state_dict(vqa_amd.ParallelCoAttention(d).state_dict())
    assert m.fast_products is False and m.bf16_projections is False


def test_cpu_tensors_raise():
    m = vqa_amd.AlternatingCoAttention(16)
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.randn(2, 5, 16), [torch.randn(2, 4, 16)] * 3)
    with pytest.raises(RuntimeError, match="GPU"):
        m.forward_with_attention(torch.randn(2, 5, 16), [torch.randn(2, 4, 16)] * 3)


def test_cli_default_and_refusals():
    ap = T.build_parser()
    assert ap.parse_args([]).co_attention == "parallel"
    assert ap.parse_args(["--co_attention", "alternating"]).co_attention == "alternating"
    T.check_co_attention("attention", "alternating")
    T.check_co_attention("baseline", "parallel")
    with pytest.raises(ValueError, match="co-attention models"):
        T.check_co_attention("baseline", "alternating")
    with pytest.raises(ValueError, match="affinity"):
        T.check_co_attention("attention", "alternating", affinity="bilinear")
    with pytest.raises(ValueError, match="opt_lvl"):
        T.check_co_attention("attention", "alternating", opt_lvl=1)
    with pytest.raises(ValueError, match="precision"):
        T.check_co_attention("attention", "alternating", precision="fast")
    for argv in (["--model", "baseline"], ["--affinity", "bilinear"], ["--opt_lvl", "1"], ["--precision", "fast"]):
        args = ap.parse_args(["--model", "attention", "--co_attention", "alternating"] + argv)
        with pytest.raises(ValueError):
            T.model_from_args(args)


def test_net_builds_the_alternating_form():
    net = T.build_model("attention", 50, 5, co_attention="alternating", question_mask=True)
    assert isinstance(net.co_attention, vqa_amd.AlternatingCoAttention) and net.co_attention.question_mask
    assert net.co_attention_form == "alternating"
    assert isinstance(T.build_model("attention", 50, 5).co_attention, vqa_amd.ParallelCoAttention)
    from vqa_amd import predict as Pr
    assert Pr.build_parser().parse_args(["--co_attention", "alternating"]).co_attention == "alternating"

"""CPU checks of the bilinear affinity (include/coattn.h, COATTN_FLAG_BILINEAR): the C-ABI declarations, the ctypes
structs, the module / CLI surface, and the float64 oracle the GPU tests use (tests/_bilinear.py)."""
import os
import re

import pytest
import torch

import vqa_amd
from vqa_amd import _lib
from vqa_amd import train as T
from oracle import coattn_oracle as O

from tests import _bilinear as BL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "coattn.h")
API = os.path.join(ROOT, "visual-question-answering_amd", "csrc", "api.hip")


def _struct_fields(name):
    src = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"\*\s*(\w+)\s*;", body)


def test_header_declares_the_flag_and_the_version_is_0_10():
    src = open(HEADER).read()
    assert re.search(r"#define COATTN_FLAG_BILINEAR 256\b", src)
    assert _lib.FLAG_BILINEAR == 256
    for m in re.finditer(r"#define (COATTN_FLAG_\w+) (\d+)", src):   # flags bit 8 is no other flag's
        if m.group(1) != "COATTN_FLAG_BILINEAR":
            assert int(m.group(2)) != 256
    ver = int(re.search(r'coattn_version\(void\) \{ return (\d+); \}', open(API).read()).group(1))
    assert ver >= 1000


def test_param_structs_match_the_header_with_the_new_fields_last():
    for cls, name, last in ((_lib.Params, "coattn_params", ["W_b", "b_b"]),
                            (_lib.ParamGrads, "coattn_param_grads", ["dW_b", "db_b"])):
        fields = [f for f, _ in cls._fields_]
        assert fields == _struct_fields(name)
        assert fields[-2:] == last and len(fields) == 10
    p = _lib.Params(*range(1, 9))                    # callers of 0.9 pass eight pointers: the appended fields stay NULL
    assert p.W_b is None and p.b_b is None


def test_cli_default_and_refusals():
    ap = T.build_parser()
    assert ap.parse_args([]).affinity == "reference"
    assert ap.parse_args(["--affinity", "bilinear"]).affinity == "bilinear"
    with pytest.raises(SystemExit):
        ap.parse_args(["--affinity", "other"])
    T.check_affinity("attention", "bilinear", 0)
    T.check_affinity("baseline", "reference", 3)
    with pytest.raises(ValueError, match="co-attention models"):
        T.check_affinity("baseline", "bilinear", 0)
    with pytest.raises(ValueError, match="opt_lvl"):
        T.check_affinity("attention", "bilinear", 1)
    with pytest.raises(ValueError, match="co-attention models"):
        T.model_from_args(ap.parse_args(["--model", "baseline", "--affinity", "bilinear"]))
    with pytest.raises(ValueError, match="opt_lvl"):
        T.model_from_args(ap.parse_args(["--affinity", "bilinear", "--opt_lvl", "1"]))
    from vqa_amd import predict as Pr                # predict.py takes the flag from the training parser
    assert Pr.build_parser().parse_args(["--affinity", "bilinear"]).affinity == "bilinear"


def test_module_attribute_and_state_dict_keys():
    ref = vqa_amd.ParallelCoAttention(64)
    bil = vqa_amd.ParallelCoAttention(64, affinity="bilinear")
    assert ref.affinity == "reference" and bil.affinity == "bilinear"
    assert list(ref.state_dict().keys()) == list(bil.state_dict().keys())
    bil.load_state_dict(ref.state_dict())            # a reference checkpoint loads unchanged
    with pytest.raises(ValueError):
        vqa_amd.ParallelCoAttention(64, affinity="Bilinear")
    with pytest.raises(ValueError):
        vqa_amd.ParallelCoAttention(64, affinity=None)


def test_build_model_sets_the_attribute():
    torch.manual_seed(0)
    m_ref = T.build_model("attention", 100, 10)
    torch.manual_seed(0)
    m_bil = T.build_model("attention", 100, 10, affinity="bilinear")
    assert m_ref.co_attention.affinity == "reference" and m_bil.co_attention.affinity == "bilinear"
    assert list(m_ref.state_dict().keys()) == list(m_bil.state_dict().keys())
    with pytest.raises(ValueError):
        T.build_model("baseline", 100, 10, affinity="bilinear")
    with pytest.raises(ValueError):
        T.build_model("attention", 100, 10, affinity="nope")


def test_functional_form_needs_both_W_b_and_b_b():
    x = torch.zeros(1, 4, 8)
    with pytest.raises(ValueError):
        vqa_amd.coattention(x, [torch.zeros(1, 3, 8)], *[torch.zeros(1)] * 8, W_b=torch.zeros(8, 8))


def test_oracle_with_identity_W_b_is_the_reference_oracle():
    B, N, T_, d = 3, 7, 5, 16
    P = O.make_params(d, 4, dtype=torch.float64)
    P["W_b.weight"] = torch.eye(d, dtype=torch.float64)
    P["W_b.bias"] = torch.zeros(d, dtype=torch.float64)
    V, Qs = O.make_inputs(B, N, T_, d, 9, lens=[5, 2, 1], dtype=torch.float64)
    gv = torch.from_numpy(O.hash_normal((3, B, d), 11))
    gq = torch.from_numpy(O.hash_normal((3, B, d), 12))
    r = BL.forward_backward(V, Qs, P, gv, gq, bilinear=True)
    f = O.coattn_forward(V, Qs, P)
    g = O.coattn_backward(V, Qs, P, gv, gq)
    for k in ("v", "q", "a_v", "a_q"):
        torch.testing.assert_close(r[k], f[k], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["dV_phys"], g["dV_phys"], rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(r["dQ"], torch.stack(list(g["dQ"])), rtol=1e-10, atol=1e-12)
    for k in ("W_v.weight", "W_v.bias", "W_q.weight", "W_q.bias", "w_v.weight", "w_v.bias", "w_q.weight", "w_q.bias"):
        torch.testing.assert_close(r["d" + k], g["d" + k].reshape(r["d" + k].shape), rtol=1e-10, atol=1e-12)
    r0 = BL.forward_backward(V, Qs, P, gv, gq, bilinear=False)   # the reference form leaves W_b without a gradient
    assert r0["dW_b.weight"] is None and r["dW_b.weight"].abs().max() > 0

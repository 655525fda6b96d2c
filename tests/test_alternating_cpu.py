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


# ---- coattn_alt_workspace_bytes at its limits ------------------------------------------------------------------------------
def _sizes(B, N, T, d, L, dtype=0, flags=0):
    import ctypes as C
    lib = _lib.load()
    s, f, b = C.c_size_t(), C.c_size_t(), C.c_size_t()
    rc = lib.coattn_alt_workspace_bytes(B, N, T, d, L, dtype, flags, C.byref(s), C.byref(f), C.byref(b))
    return rc, (s.value, f.value, b.value), lib.coattn_last_error()


@pytest.mark.parametrize("arg,bad,name", [
    ("L", 0, b"L=0"), ("L", 5, b"L=5"), ("d", 0, b"d=0"), ("d", 1025, b"d=1025"), ("N", 0, b"N=0"), ("N", 513, b"N=513"),
    ("T", 0, b"T=0"), ("T", 513, b"T=513"), ("B", 0, b"B=0"), ("B", 65536, b"B=65536"), ("dtype", 1, b"dtype 1"),
])
def test_workspace_bytes_refuses_past_the_limits(arg, bad, name):
    shape = dict(B=4, N=7, T=5, d=64, L=3, dtype=0)
    shape[arg] = bad
    rc, _, msg = _sizes(**shape)
    assert rc < 0 and name in msg, (rc, msg)


def test_workspace_bytes_accepts_the_limits():
    for shape in (dict(B=4, N=7, T=5, d=64, L=4), dict(B=4, N=7, T=5, d=1024, L=3), dict(B=4, N=512, T=512, d=64, L=3),
                  dict(B=65535, N=7, T=5, d=64, L=3), dict(B=1, N=1, T=1, d=1, L=1)):
        rc, sizes, msg = _sizes(**shape)
        assert rc == 0 and all(x > 0 for x in sizes), (shape, rc, msg)


def test_workspace_sizes_are_aligned_and_monotone():
    base = dict(B=5, N=9, T=7, d=72, L=2)
    grow = dict(B=(6, 33, 160), N=(10, 49, 512), T=(8, 26, 512), d=(73, 128, 1024), L=(3, 4))
    rc, s0, _ = _sizes(**base)
    assert rc == 0
    for arg, values in grow.items():
        prev = s0
        for v in values:
            rc, s, _ = _sizes(**dict(base, **{arg: v}))
            assert rc == 0
            assert all(x % 256 == 0 for x in s), (arg, v, s)
            assert all(a >= b for a, b in zip(s, prev)), (arg, v, s, prev)   # non-decreasing in every argument
            assert s[1] >= s[0]                                             # ws_fwd holds the state when saved is NULL
            prev = s
    assert all(x % 256 == 0 for x in s0) and s0[1] >= s0[0]


# ---- paths(): the dispatch rules of csrc/coattn_alt.hip, pinned at every threshold the GPU sweep relies on -----------------
def test_paths_projection_thresholds():
    p = AL.paths
    # 127 / 128 rows (B T = B: T = 1), K = d = 64
    assert p(127, 4, 1, 64, 3)["x13"] == "general" and p(128, 4, 1, 64, 3)["x13"] == "gemm_w"
    assert p(127, 1, 4, 64, 3)["x2"] == "general" and p(128, 1, 4, 64, 3)["x2"] == "gemm_w"
    assert p(127, 1, 4, 64, 3)["dv"] == "general" and p(128, 1, 4, 64, 3)["dv"] == "gemm_w"
    for k in ("g2", "g3", "dvt", "dsh"):                   # L B rows
        assert p(42, 4, 4, 64, 3)[k] == "general" and p(43, 4, 4, 64, 3)[k] == "gemm_w"
        assert p(127, 4, 4, 64, 1)[k] == "general" and p(128, 4, 4, 64, 1)[k] == "gemm_w"
    # K = d for the projections, 2d for dQ: 31 / 32 / 48 / 64
    for d, proj, dq in ((15, "general", "general"), (16, "general", "gemm_w"), (31, "general", "general"),
                        (32, "gemm_w", "gemm_w"), (48, "general", "gemm_w"), (64, "gemm_w", "gemm_w"), (80, "general", "gemm_w")):
        r = p(64, 4, 4, d, 3)
        assert (r["x13"], r["x2"], r["g2"], r["dv"], r["dq"]) == (proj, proj, proj, proj, dq), (d, r)
    assert p(2, 7, 5, 1024, 3)["dq"] == "general"             # K qualifies, 10 rows do not


def test_paths_weight_gradient_thresholds():
    p = AL.paths
    # rows 15 / 16 at d = 128 (B T with T = 1; B N with N = 1; L B with L = 1)
    a, b = p(15, 1, 1, 128, 1), p(16, 1, 1, 128, 1)
    assert (a["dw_x13"], a["dw_x2"], a["dw_g"]) == ("splitk",) * 3 and (b["dw_x13"], b["dw_x2"], b["dw_g"]) == ("gemm_tn",) * 3
    # d 127 / 128 (and a multiple of 64 that is none of 128)
    assert p(16, 1, 1, 127, 1)["dw_x13"] == "splitk" and p(16, 1, 1, 192, 1)["dw_x13"] == "splitk"
    assert p(16, 1, 1, 256, 1)["dw_g"] == "gemm_tn"
    # part counts: the split-K's per = 32 / L, ks = ceil16(ceil(rows / per)); gemm_tn_plan with 32 parts at most
    assert p(3, 7, 5, 64, 3)["parts"]["dw_x13"] == 3 and p(43, 3, 3, 64, 3)["parts"]["dw_x13"] == 27
    assert p(160, 49, 26, 64, 3)["parts"]["dw_x13"] == 30      # per = 10, ks = 416, S = 10
    assert p(6, 7, 5, 128, 4)["parts"] == dict(dw_x13=8, dw_x2=3, dw_g=2, steps13=24, step2=6)
    # config 2: 8 x 4 tiles -> 16 / 3 = 5 parts per level of ceil16(4160 / 5) = 832 rows; 4 x 4 tiles -> 32 parts wanted,
    # ceil16(7840 / 32) = 256 rows each: 31 parts
    assert p(160, 49, 26, 512, 3)["parts"]["dw_x13"] == 15 and p(160, 49, 26, 512, 3)["parts"]["dw_x2"] == 31


def test_paths_feature_layouts():
    p = AL.paths
    # channel-major: the a_sk form needs N % 4 == 0 (then sD and sB are multiples of 4 too), B N >= 128, d % 32 == 0
    assert p(32, 4, 3, 64, 3, "cm")["x2"] == "gemm_w_ask" and p(31, 4, 3, 64, 3, "cm")["x2"] == "general_mdiv"
    assert p(64, 3, 3, 64, 3, "cm")["x2"] == "general_mdiv" and p(64, 6, 3, 64, 3, "cm")["x2"] == "general_mdiv"
    assert p(32, 4, 3, 48, 3, "cm")["x2"] == "general_mdiv"
    assert p(26, 8, 5, 64, 3, "cmpad")["x2"] == "general_mdiv"     # sD = 11
    assert p(26, 8, 5, 64, 3, "pad")["x2"] == "general_mdiv" and p(26, 8, 5, 64, 3, "col2")["x2"] == "general"
    # dV follows its own layout, not V's
    assert p(26, 8, 5, 64, 3, "cm", "lm")["dv"] == "gemm_w" and p(26, 8, 5, 64, 3, "lm", "cm")["dv"] == "general_mdiv"
    assert p(26, 8, 5, 64, 3, "lm", "pad")["dv"] == "general_mdiv" and p(26, 8, 5, 64, 3, "lm", "col2")["dv"] == "general"
    assert p(26, 8, 5, 64, 3, "cm", None)["dv"] is None
    # any V that is not location-major: the grouped dW_x2, G = ceil(B / 32) samples per part, S = ceil(B / G) parts
    for B, G, S in ((32, 1, 32), (33, 2, 17), (64, 2, 32), (65, 3, 22), (70, 3, 24)):
        for layout in ("cm", "pad", "cmpad", "col2"):
            r = p(B, 4, 3, 64, 3, layout)
            assert r["dw_x2"] == "grouped" and (r["parts"]["group"], r["parts"]["dw_x2"]) == (G, S), (B, layout, r)
    assert p(33, 4, 3, 64, 3, "lm")["dw_x2"] == "splitk"


def test_layout_geometry_matches_torch_views():
    B, N, d = 3, 5, 8
    views = {
        "lm": lambda: torch.empty(B, N, d),
        "cm": lambda: torch.empty(B, d, N).permute(0, 2, 1),
        "pad": lambda: torch.empty(B, N + 2, d + 5)[:, 1:1 + N, 2:2 + d],
        "cmpad": lambda: torch.empty(B, d + 1, N + 3)[:, 1:, 2:2 + N].permute(0, 2, 1),
        "col2": lambda: torch.empty(B, N, 2 * d)[:, :, ::2],
    }
    assert set(views) == set(AL.LAYOUTS)
    for name, make in views.items():
        v = make()
        shape, off, strides = AL.layout_geometry(B, N, d, name)
        assert tuple(v.shape) == (B, N, d) and tuple(v.stride()) == strides and v.storage_offset() == off, name
        assert shape[0] * shape[1] * shape[2] == v.untyped_storage().nbytes() // 4, name

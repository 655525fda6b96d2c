"""Differentiable attention maps (C-ABI 0.9.0: coattn_forward_maps(_len), coattn_backward_maps(_len)), on the CPU:
declarations, exports, argument order, refusals and the Python surface's refusal of CPU tensors."""
import ctypes
import re

import pytest
import torch

from tests._header import args as _args, header as _header

NEW = ("coattn_forward_maps", "coattn_forward_maps_len", "coattn_backward_maps", "coattn_backward_maps_len")


def test_map_entry_points_declared_exported_and_versioned():
    from vqa_amd import _lib
    hdr = _header()
    declared = set(re.findall(r"\b(coattn_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.coattn_version() >= 900
    loaded = _lib.load()
    for name in NEW:
        assert getattr(loaded, name).argtypes is not None, name


def test_map_entry_points_argument_order():
    hdr = _header()
    # the _len forms: q_len right after Q, as in every *_len entry point
    for name in ("coattn_forward_maps_len", "coattn_backward_maps_len"):
        a = _args(hdr, name)
        assert a[4].endswith("Q") and a[5] == "const int32_t* q_len", (name, a[4:6])
    # forward: the map buffers, then `saved` and `ws`, and otherwise coattn_forward's arguments
    fwd, plain = _args(hdr, "coattn_forward_maps"), _args(hdr, "coattn_forward")
    assert fwd[6:10] == ["void* v_out", "void* q_out", "void* av_out", "void* aq_out"], fwd[6:10]
    assert fwd[10:] == plain[8:] and fwd[:8] == plain[:8]
    assert _args(hdr, "coattn_forward_maps_len") == fwd[:5] + ["const int32_t* q_len"] + fwd[5:]
    # backward: g_av / g_aq right after gq, and otherwise coattn_backward's arguments
    bwd, plain = _args(hdr, "coattn_backward_maps"), _args(hdr, "coattn_backward")
    i = bwd.index("const void* gq")
    assert bwd[i + 1:i + 3] == ["const void* g_av", "const void* g_aq"], bwd[i:i + 3]
    assert bwd[:i + 1] + bwd[i + 3:] == plain
    assert _args(hdr, "coattn_backward_maps_len") == bwd[:5] + ["const int32_t* q_len"] + bwd[5:]
    # the header documents the semantics: NULL map gradients, the formulas, the masked read, where `saved` comes from
    assert "or NULL (= 0)" in hdr and "da_v = V g_v + G_av" in hdr and "da_q = Q g_q + G_aq" in hdr
    assert "READ AS 0" in hdr and "must come from a coattn_forward_maps(_len) or a coattn_forward(_len)" in hdr


def test_map_entry_points_reject_bad_shapes_and_null_buffers():
    from vqa_amd import _lib
    lib = _lib.load()
    L = 3
    q = (ctypes.c_void_p * L)(*([0] * L))
    p = _lib.Params()
    pg = _lib.ParamGrads()
    null = ctypes.c_void_p(0)
    some = ctypes.c_void_p(256)                     # (never dereferenced: every call below is refused on the host)
    for B, N, T, d, what in ((0, 49, 26, 512, b"batch"), (4, 49, 0, 512, b"T="), (4, 49, 26, 0, b"hidden"),
                             (4, 49, 26, 512 * 32, b"hidden")):
        rc = lib.coattn_forward_maps(null, 0, 0, 0, q, ctypes.byref(p), null, null, some, some, some, null,
                                     B, N, T, d, L, _lib.F32, 0, null)
        assert rc < 0 and what in lib.coattn_last_error(), (rc, lib.coattn_last_error())
        rc = lib.coattn_forward_maps_len(null, 0, 0, 0, q, null, ctypes.byref(p), null, null, some, some, some, null,
                                         B, N, T, d, L, _lib.F32, 0, null)
        assert rc < 0 and what in lib.coattn_last_error()
        rc = lib.coattn_backward_maps(null, 0, 0, 0, q, ctypes.byref(p), null, null, null, null, null, null, 0, 0, 0, q,
                                      ctypes.byref(pg), 0, null, B, N, T, d, L, _lib.F32, 0, null)
        assert rc < 0 and what in lib.coattn_last_error()
        rc = lib.coattn_backward_maps_len(null, 0, 0, 0, q, null, ctypes.byref(p), null, null, null, null, null, null,
                                          0, 0, 0, q, ctypes.byref(pg), 0, null, B, N, T, d, L, _lib.F32, 0, null)
        assert rc < 0 and what in lib.coattn_last_error()
    rc = lib.coattn_forward_maps(null, 0, 0, 0, q, ctypes.byref(p), null, null, some, some, null, null,
                                 4, 49, 26, 512, L, _lib.F32, 0, null)
    assert rc < 0 and b"saved" in lib.coattn_last_error()
    rc = lib.coattn_forward_maps_len(null, 0, 0, 0, q, null, ctypes.byref(p), null, null, some, some, null, null,
                                     4, 49, 26, 512, L, _lib.F32, 0, null)
    assert rc < 0 and b"saved" in lib.coattn_last_error()
    for av, aq in ((null, some), (some, null), (null, null)):
        rc = lib.coattn_forward_maps(null, 0, 0, 0, q, ctypes.byref(p), null, null, av, aq, some, null,
                                     4, 49, 26, 512, L, _lib.F32, 0, null)
        assert rc < 0 and b"map buffer" in lib.coattn_last_error()
        rc = lib.coattn_forward_maps_len(null, 0, 0, 0, q, null, ctypes.byref(p), null, null, av, aq, some, null,
                                         4, 49, 26, 512, L, _lib.F32, 0, null)
        assert rc < 0 and b"map buffer" in lib.coattn_last_error()
    # null operands with a good shape (`saved` among them): refused before anything is enqueued
    rc = lib.coattn_backward_maps(null, 0, 0, 0, q, ctypes.byref(p), null, null, null, some, some, null, 0, 0, 0, q,
                                  ctypes.byref(pg), 0, null, 4, 49, 26, 512, L, _lib.F32, 0, null)
    assert rc < 0 and b"null" in lib.coattn_last_error()
    rc = lib.coattn_backward_maps_len(null, 0, 0, 0, q, null, ctypes.byref(p), null, null, null, some, some, null,
                                      0, 0, 0, q, ctypes.byref(pg), 0, null, 4, 49, 26, 512, L, _lib.F32, 0, null)
    assert rc < 0 and b"null" in lib.coattn_last_error()


def test_return_attention_on_cpu_tensors_raises():
    import vqa_amd
    from vqa_amd.coattention import coattention
    torch.manual_seed(0)
    m = vqa_amd.ParallelCoAttention(64)
    x = torch.randn(2, 5, 64)
    qs = [torch.randn(2, 4, 64) for _ in range(3)]
    with pytest.raises(RuntimeError, match="GPU"):
        m(x, qs, return_attention=True)                        # (parameters need a gradient: the autograd path)
    with pytest.raises(RuntimeError, match="GPU"):
        m(x.requires_grad_(True), qs, return_attention=True)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
        m(x, qs, return_attention=True)                        # (the inference path)
    with pytest.raises(RuntimeError, match="GPU"):
        coattention(x, qs, m.W_v.weight, m.W_v.bias, m.W_q.weight, m.W_q.bias, m.w_v.weight, m.w_v.bias, m.w_q.weight,
                    m.w_q.bias, return_attention=True)
    # the existing inference entry point keeps its refusal under grad
    with pytest.raises(RuntimeError, match="forward only"):
        m.forward_with_attention(x, qs)


def test_network_return_attention_on_cpu_raises():
    from vqa_amd import train as T
    torch.manual_seed(0)
    net = T.build_model("attention", 50, 4)
    feats = torch.randn(2, 49, 512)
    qu = torch.randint(1, 50, (2, 6))
    ln = torch.tensor([6, 4])
    with pytest.raises(RuntimeError, match="GPU"):
        net.forward_features(feats, qu, ln, labels=torch.tensor([0, 1]), return_attention=True)

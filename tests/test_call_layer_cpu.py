"""The named-argument call layer of vqa_amd._lib (SIGNATURES, bind, Call.replace), on the CPU: every tabled signature
against include/coattn.h, and the positional tuples the binder lays out against the positional expressions the package
used before it -- restated here literally, so that a shifted position shows without a GPU."""
import ctypes as C

import pytest
import torch

import vqa_amd  # noqa: F401
from tests._header import args as header_args, header
from vqa_amd import _lib
from vqa_amd.coattention import _strides

TABLED = ("coattn_forward", "coattn_forward_len", "coattn_forward_maps", "coattn_forward_maps_len", "coattn_infer",
          "coattn_infer_len", "coattn_attention_forward", "coattn_attention_forward_len", "coattn_backward",
          "coattn_backward_len", "coattn_backward_maps", "coattn_backward_maps_len", "coattn_alt_forward", "coattn_alt_backward",
          "coattn_head_forward", "coattn_head_forward_soft", "coattn_head_backward")
STRUCTS = {"coattn_params": _lib.Params, "coattn_param_grads": _lib.ParamGrads, "coattn_alt_params": _lib.AltParams,
           "coattn_alt_param_grads": _lib.AltParamGrads, "coattn_head_params": _lib.HeadParams,
           "coattn_head_param_grads": _lib.HeadParamGrads}


def test_the_table_covers_the_seventeen_entry_points():
    assert sorted(_lib.SIGNATURES) == sorted(TABLED) and len(TABLED) == 17


@pytest.mark.parametrize("name", TABLED)
def test_signature_matches_the_header(name):
    declared = [a.rsplit(" ", 1) for a in header_args(header(), name)]          # [C type, argument name]
    sig = _lib.SIGNATURES[name]
    assert [n for n, _ in sig] == [n for _, n in declared]
    for (n, ctype), (ctext, _) in zip(sig, declared):
        base = ctext.replace("const", "").replace("*", "").strip()
        if "*" in ctext:
            assert ctype is C.c_void_p or issubclass(ctype, C._Pointer), (name, n, ctext, ctype)
            if base in STRUCTS:
                assert ctype is C.POINTER(STRUCTS[base]), (name, n, ctext, ctype)
            if ctext.count("*") == 2:                                            # a host array of device pointers
                assert ctype is C.POINTER(C.c_void_p), (name, n, ctext, ctype)
        elif base == "int64_t":
            assert ctype is C.c_int64, (name, n, ctext, ctype)
        else:
            assert base == "int" and ctype is C.c_int, (name, n, ctext, ctype)
    assert list(getattr(_lib.load(), name).argtypes) == [t for _, t in sig]


def _norm(args):
    """A positional tuple in comparable form: pointers as integers (NULL = 0 however it is spelled), host arrays as lists,
    byref(x) as the address of x."""
    out = []
    for a in args:
        if a is None:
            a = 0
        elif isinstance(a, C.c_void_p):
            a = a.value or 0
        elif isinstance(a, C.Array):
            a = [v or 0 for v in a]
        elif type(a).__name__ == "CArgObject":
            a = ("byref", C.addressof(a._obj))
        out.append(a)
    return tuple(out)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


B, N, T, d, L = 2, 5, 4, 8, 3


@pytest.mark.parametrize("dv", ("location-major", "channel-major", None))
@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("maps", ("both", "no g_av", "no g_aq", "neither"))
def test_backward_binding_is_the_positional_expression_it_replaces(dv, masked, maps):
    V = torch.randn(B, d, N).permute(0, 2, 1)                                    # (a channel-major view: three distinct strides)
    Qs = [torch.randn(B, T, d) for _ in range(L)]
    params = [torch.randn(4) for _ in range(10)]
    grads = [torch.randn(4) for _ in range(10)]
    saved, ws, g_v, g_q = torch.randn(16), torch.randn(16), torch.randn(L, B, d), torch.randn(L, B, d)
    g_av = torch.randn(L, B, N) if maps in ("both", "no g_aq") else None
    g_aq = torch.randn(L, B, T) if maps in ("both", "no g_av") else None
    q_len = torch.tensor([T, 1], dtype=torch.int32) if masked else None
    dQs = [torch.empty_like(q) for q in Qs]
    need_dv = dv is not None
    dV = {"location-major": torch.empty(B, N, d), "channel-major": torch.empty(B, d, N).permute(0, 2, 1), None: None}[dv]
    impl, stream = _lib.IMPL_GENERAL | _lib.FLAG_BILINEAR, 0x7f00
    pg = _lib.ParamGrads(*[t.data_ptr() for t in grads])
    p = _lib.Params(*[t.data_ptr() for t in params])
    qptr = (C.c_void_p * L)(*[q.data_ptr() for q in Qs])
    dqptr = (C.c_void_p * L)(*[q.data_ptr() for q in dQs])
    # the expression of _CoAttentionMapsFn.backward before the call layer, for coattn_backward_maps_len
    args = (C.byref(p), _ptr(saved), _ptr(g_v), _ptr(g_q), _ptr(g_av), _ptr(g_aq), _ptr(dV),
            *(_strides(dV) if need_dv else (0, 0, 0)), dqptr, C.byref(pg), 0, _ptr(ws), B, N, T, d, L, _lib.F32, impl,
            C.c_void_p(stream))
    before = (_ptr(V), *_strides(V), qptr, _ptr(q_len), *args)

    sB, sN, sD = _strides(V)
    kw = dict(V=V, v_sB=sB, v_sN=sN, v_sD=sD, Q=_lib.ptr_array(Qs), p=p, saved=saved, gv=g_v, gq=g_q, dQ=_lib.ptr_array(dQs),
              pg=pg, accumulate=0, ws=ws, B=B, N=N, T=T, d=d, L=L, dtype=_lib.F32, flags=impl, stream=stream)
    if masked:
        kw["q_len"] = q_len
    if g_av is not None:
        kw["g_av"] = g_av
    if g_aq is not None:
        kw["g_aq"] = g_aq
    if need_dv:
        kw.update(zip(("dV", "dv_sB", "dv_sN", "dv_sD"), (dV, *_strides(dV))))
    bound = _lib.bind("coattn_backward_maps_len", **kw)
    assert bound.name == "coattn_backward_maps_len" and len(bound) == len(_lib.SIGNATURES[bound.name]) == len(before)
    assert _norm(bound) == _norm(before)
    assert len(set(_norm(before)[:4])) == 4 and _norm(before)[5] == (q_len.data_ptr() if masked else 0)
    # None spelled out is the omitted argument
    spelled = _lib.bind("coattn_backward_maps_len", **{"q_len": None, "g_av": None, "g_aq": None, "dV": None, **kw})
    assert _norm(spelled) == _norm(before)
    # ... and so are the arguments the package's own calls share (coattention._shared_args)
    from vqa_amd.coattention import _shared_args
    assert _norm(_lib.bind("coattn_backward_maps_len", **{**kw, **_shared_args(V, Qs, q_len, p, ws, impl)})) == _norm(before)


@pytest.mark.parametrize("replaced", ("nothing", "g_logits", "g_loss", "accumulate", "all three"))
def test_head_backward_rebinding_is_the_slicing_it_replaces(replaced):
    Bh, dh, mlp, K, flags = 8, 16, 12, 11, _lib.FLAG_BF16_PROJ
    v, q, dx = torch.randn(3, Bh, dh), torch.randn(3, Bh, dh), torch.randn(3, Bh, dh)
    hsaved, hws, static_g_loss = torch.randn(8), torch.randn(8), torch.ones(1)
    hp = _lib.HeadParams(*[torch.randn(4).data_ptr() for _ in range(8)])
    hg = _lib.HeadParamGrads(*[torch.randn(4).data_ptr() for _ in range(8)])
    rows = lambda t: (C.c_void_p * 3)(*[t[l].data_ptr() for l in range(3)])      # noqa: E731
    rv, rq, rdx = rows(v), rows(q), rows(dx)
    # HotPathGraph._plan's "head_bwd" and its "head_bwd_args" before the call layer
    head_bwd = (rv, rq, C.byref(hp), _ptr(hsaved), _ptr(static_g_loss), None, rdx, None, C.byref(hg), 0,
                _ptr(hws), Bh, dh, mlp, K, _lib.F32, flags)
    head_bwd_args = lambda g_logits, acc, g_loss=None: (head_bwd[:4] + (_ptr(static_g_loss if g_loss is None else g_loss), _ptr(g_logits))   # noqa: E731
                                                        + head_bwd[6:9] + (acc,) + head_bwd[10:])
    assert head_bwd[9] == 0 and head_bwd[5] is None

    bound = _lib.bind("coattn_head_backward", v=_lib.rows(v), q=_lib.rows(q), p=hp, saved=hsaved, g_loss=static_g_loss,
                      dv=_lib.rows(dx), pg=hg, accumulate=0, ws=hws, B=Bh, d=dh, mlp=mlp, K=K, dtype=_lib.F32, flags=flags)
    assert len(bound) == len(_lib.SIGNATURES["coattn_head_backward"]) - 1           # (the stream is left for the call)
    assert _norm(bound) == _norm(head_bwd)
    g_logits, g_loss = torch.randn(Bh, K), torch.full((1,), 3.0)
    if replaced == "nothing":
        assert _norm(bound.replace()) == _norm(head_bwd_args(None, 0))
    elif replaced == "g_logits":
        assert _norm(bound.replace(g_logits=g_logits)) == _norm(head_bwd_args(g_logits, 0))
        assert _norm(bound.replace(g_logits=g_logits))[5] == g_logits.data_ptr()
    elif replaced == "g_loss":
        assert _norm(bound.replace(g_loss=g_loss)) == _norm(head_bwd_args(None, 0, g_loss))
        assert _norm(bound.replace(g_loss=g_loss))[4] == g_loss.data_ptr()
    elif replaced == "accumulate":
        assert _norm(bound.replace(accumulate=1)) == _norm(head_bwd_args(None, 1))
        assert _norm(bound.replace(accumulate=1))[9] == 1
    else:
        again = bound.replace(g_loss=g_loss, g_logits=g_logits, accumulate=1)
        assert _norm(again) == _norm(head_bwd_args(g_logits, 1, g_loss)) and again.name == bound.name
        assert _norm(again.replace(g_loss=static_g_loss, g_logits=None, accumulate=0)) == _norm(head_bwd)
    assert _norm(bound) == _norm(head_bwd)                                        # (replace leaves the bound call as it was)
    with_stream = bound.replace(stream=0x7f00)
    assert _norm(with_stream) == _norm(head_bwd) + (0x7f00,)


def test_unknown_and_missing_names_raise():
    t = torch.zeros(4)
    good = dict(v=_lib.rows(torch.zeros(3, 2, 2)), q=_lib.rows(torch.zeros(3, 2, 2)), p=_lib.HeadParams(), logits=t, saved=t,
                B=2, d=2, mlp=2, K=2, dtype=_lib.F32, flags=0)
    bound = _lib.bind("coattn_head_forward", **good)                               # labels, loss: nullable; stream: later
    assert _norm(bound)[3] == 0 and _norm(bound)[5] == 0
    with pytest.raises(TypeError, match="g_logits"):
        _lib.bind("coattn_head_forward", g_logits=t, **good)
    for name in ("v", "p", "logits", "K", "dtype", "flags"):
        with pytest.raises(TypeError, match="missing argument %r" % name):
            _lib.bind("coattn_head_forward", **{k: a for k, a in good.items() if k != name})
    with pytest.raises(TypeError, match="labelz"):
        bound.replace(labelz=t)
    with pytest.raises(KeyError):
        _lib.bind("coattn_head_sideways", **good)
    # the strides of V are required, those of an absent dV are not
    with pytest.raises(TypeError, match="v_sN"):
        _lib.bind("coattn_infer_len", V=t, v_sB=1, v_sD=1, Q=_lib.ptr_array([t]), p=_lib.Params(), v_out=t, q_out=t, ws=t,
                  B=1, N=1, T=1, d=1, L=1, dtype=_lib.F32, flags=0)
    with pytest.raises(TypeError, match="saved"):                                  # (coattn_infer_len keeps no state)
        _lib.bind("coattn_infer_len", V=t, v_sB=1, v_sN=1, v_sD=1, Q=_lib.ptr_array([t]), p=_lib.Params(), v_out=t, q_out=t,
                  ws=t, saved=t, B=1, N=1, T=1, d=1, L=1, dtype=_lib.F32, flags=0)

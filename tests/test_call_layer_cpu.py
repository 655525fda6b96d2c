"""The named-argument call layer of vqa_amd._lib (SIGNATURES, bind, Call.replace), on the CPU: every tabled signature
against include/coattn.h, and the positional tuples the binder lays out against the positional expressions the package
used before it -- restated here literally, so that a shifted position shows without a GPU."""
import ctypes as C
import re

import pytest
import torch

import vqa_amd  # noqa: F401
from tests._header import args as header_args, declared, header
from vqa_amd import _lib
from vqa_amd.coattention import _strides

HEADER = header()
DECLARED = declared(HEADER)                                                       # {function: return type}
STRUCTS = {"coattn_params": _lib.Params, "coattn_param_grads": _lib.ParamGrads, "coattn_alt_params": _lib.AltParams,
           "coattn_alt_param_grads": _lib.AltParamGrads, "coattn_head_params": _lib.HeadParams,
           "coattn_head_param_grads": _lib.HeadParamGrads, "coattn_phrase_params": _lib.PhraseParams,
           "coattn_phrase_param_grads": _lib.PhraseParamGrads, "coattn_lstm_params": _lib.LstmParams,
           "coattn_lstm_param_grads": _lib.LstmParamGrads, "coattn_adam_tensor": _lib.AdamTensor,
           "coattn_overlay_params": _lib.OverlayParams, "coattn_gemm_desc": _lib.GemmDesc}
SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "long long": C.c_int64, "double": C.c_double, "float": C.c_float,
           "size_t": C.c_size_t}
# what a `T*` is bound as: device memory (void*, and the int32_t* lengths and counters) by address, host memory by its type
POINTERS = {"void": C.c_void_p, "int32_t": C.c_void_p, "size_t": C.POINTER(C.c_size_t), "float": C.POINTER(C.c_float),
            "int": C.POINTER(C.c_int), "char": C.c_char_p}
POINTERS.update({text: C.POINTER(struct) for text, struct in STRUCTS.items()})
RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}


def test_the_table_covers_every_declared_function():
    assert set(_lib.SIGNATURES) == set(DECLARED) == set(_lib.EXPORTS)
    # (no declaration escapes the return types tests/_header.py knows: every line that opens one, whatever it returns)
    assert set(re.findall(r"^[a-z][^\n(]*\b(coattn_\w+)\(", HEADER, re.M)) == set(DECLARED)
    assert set(_lib.RESTYPES) == {n for n, ret in DECLARED.items() if ret != "int"}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_signature_matches_the_header(name):
    declared_args = [a.rsplit(" ", 1) for a in header_args(HEADER, name)]          # [C type, argument name]
    sig = _lib.SIGNATURES[name]
    assert [n for n, _ in sig] == [n for _, n in declared_args]
    for (n, ctype), (ctext, _) in zip(sig, declared_args):
        base = ctext.replace("const", "").replace("*", "").strip()
        if ctext.count("*") == 2:                                                # a host array of device pointers
            assert base == "void" and ctype is C.POINTER(C.c_void_p), (name, n, ctext, ctype)
        elif "*" in ctext:
            assert ctype is POINTERS[base], (name, n, ctext, ctype)
        else:
            assert ctype is SCALARS[base], (name, n, ctext, ctype)
    fn = getattr(_lib.load(), name)
    assert list(fn.argtypes) == [t for _, t in sig]
    assert fn.restype is RETURNS[DECLARED[name]] is _lib.RESTYPES.get(name, C.c_int)


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


# ---- the calls that took hand-counted positional lists until every entry point got a row -----------------------------------
# One test per call: `before` restates, literally, the positional expression the package's call site spelled out; the bound
# call comes from the helper that call site uses now, on CPU tensors (nothing is launched).
STREAM = 0x7f00


def _t(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


@pytest.mark.parametrize("keep", (True, False))
def test_phrase_forward_binding(keep):
    from vqa_amd import phrase
    Bp, Tp, E, flags = 2, 5, 8, _lib.FLAG_FAST16
    X, out, ws, saved = _t(Bp, Tp, E), _t(Bp, Tp, E), _t(16), (_t(16) if keep else None)
    p = _lib.PhraseParams(*[_t(4).data_ptr() for _ in range(6)])
    stream = C.c_void_p(STREAM)
    before = (_ptr(X), C.byref(p), _ptr(out), _ptr(saved), _ptr(ws), Bp, Tp, E, _lib.F32, flags, stream)
    bound = phrase._forward_call(X, p, out, saved, ws, flags, STREAM)
    assert bound.name == "coattn_phrase_forward" and _norm(bound) == _norm(before)
    assert _norm(before)[3] == (saved.data_ptr() if keep else 0)


@pytest.mark.parametrize("need_dx", (True, False))
def test_phrase_backward_binding(need_dx):
    from vqa_amd import phrase
    Bp, Tp, E, flags = 2, 5, 8, _lib.FLAG_BF16_PROJ
    X, out, saved, g, ws = _t(Bp, Tp, E), _t(Bp, Tp, E), _t(16), _t(Bp, Tp, E), _t(16)
    dX = _t(Bp, Tp, E) if need_dx else None
    p = _lib.PhraseParams(*[_t(4).data_ptr() for _ in range(6)])
    pg = _lib.PhraseParamGrads(*[_t(4).data_ptr() for _ in range(6)])
    stream = C.c_void_p(STREAM)
    before = (_ptr(X), C.byref(p), _ptr(out), _ptr(saved), _ptr(g), _ptr(dX),
              C.byref(pg), 0, _ptr(ws), Bp, Tp, E, _lib.F32, flags, stream)
    bound = phrase._backward_call(X, p, out, saved, g, dX, pg, ws, flags, STREAM)
    assert bound.name == "coattn_phrase_backward" and _norm(bound) == _norm(before)
    assert _norm(before)[5] == (dX.data_ptr() if need_dx else 0) and len(set(_norm(before)[:5])) == 5


@pytest.mark.parametrize("keep", (True, False))
@pytest.mark.parametrize("masked_out", (True, False))
def test_lstm_forward_binding(keep, masked_out):
    from vqa_amd import lstm
    Bl, Tl, E, H = 2, 5, 8, 16
    X, lens, out, ws = _t(Bl, Tl, E), _t(Bl, dtype=torch.int32), _t(Bl, Tl, H), _t(16)
    x_masked, saved = (_t(Bl, Tl, E) if masked_out else None), (_t(16) if keep else None)
    p = _lib.LstmParams(*[_t(4).data_ptr() for _ in range(4)])
    stream = C.c_void_p(STREAM)
    before = (_ptr(X), _ptr(lens), C.byref(p), _ptr(out), _ptr(x_masked), _ptr(saved),
              _ptr(ws), Bl, Tl, E, H, _lib.F32, 0, stream)
    bound = lstm._forward_call(X, lens, p, out, x_masked, saved, ws, STREAM)
    assert bound.name == "coattn_lstm_forward" and _norm(bound) == _norm(before)
    assert _norm(before)[4:6] == (x_masked.data_ptr() if masked_out else 0, saved.data_ptr() if keep else 0)


@pytest.mark.parametrize("need_dx", (True, False))
@pytest.mark.parametrize("with_g_xm", (True, False))
def test_lstm_backward_binding(need_dx, with_g_xm):
    from vqa_amd import lstm
    Bl, Tl, E, H = 2, 5, 8, 16
    X, lens, saved, g_out, ws = _t(Bl, Tl, E), _t(Bl, dtype=torch.int32), _t(16), _t(Bl, Tl, H), _t(16)
    g_xm, dX = (_t(Bl, Tl, E) if with_g_xm else None), (_t(Bl, Tl, E) if need_dx else None)
    p = _lib.LstmParams(*[_t(4).data_ptr() for _ in range(4)])
    pg = _lib.LstmParamGrads(*[_t(4).data_ptr() for _ in range(4)])
    stream = C.c_void_p(STREAM)
    before = (_ptr(X), _ptr(lens), C.byref(p), None, _ptr(saved), _ptr(g_out),
              _ptr(g_xm), _ptr(dX), C.byref(pg), 0, _ptr(ws), Bl, Tl, E, H, _lib.F32, 0,
              stream)
    bound = lstm._backward_call(X, lens, p, saved, g_out, g_xm, dX, pg, ws, H, STREAM)
    assert bound.name == "coattn_lstm_backward" and _norm(bound) == _norm(before)
    assert _norm(before)[6:8] == (g_xm.data_ptr() if with_g_xm else 0, dX.data_ptr() if need_dx else 0)


@pytest.mark.parametrize("need", (True, False))
def test_loss_bindings(need):
    from vqa_amd import loss as loss_mod
    Bc, K, A, kind = 3, 7, 4, _lib.LOSS_BCE
    z, lab, loss, ws = _t(Bc, K), _t(Bc, dtype=torch.int64), _t(1), _t(16)
    ai, sc = _t(Bc, A, dtype=torch.int32), _t(Bc, A)
    dz = _t(Bc, K) if need else None
    stream = C.c_void_p(STREAM)
    before = (_ptr(z), _ptr(lab), _ptr(loss), _ptr(dz), _ptr(ws), Bc, K, _lib.F32,
              stream)
    bound = loss_mod._ce_call(z, lab, loss, dz, ws, STREAM)
    assert bound.name == "coattn_ce_forward" and _norm(bound) == _norm(before)
    assert _norm(before)[3] == (dz.data_ptr() if need else 0)
    before = (_ptr(z), _ptr(ai), _ptr(sc), A, kind, _ptr(loss), _ptr(dz), _ptr(ws),
              Bc, K, _lib.F32, stream)
    bound = loss_mod._soft_loss_call(z, ai, sc, kind, loss, dz, ws, STREAM)
    assert bound.name == "coattn_soft_loss_forward" and _norm(bound) == _norm(before)
    assert _norm(before)[6] == (dz.data_ptr() if need else 0)


@pytest.mark.parametrize("row_score", (True, False))
def test_vqa_score_binding(row_score):
    from vqa_amd import loss as loss_mod
    Bc, K, A = 3, 7, 4
    z, ai, sc, ws = _t(Bc, K), _t(Bc, A, dtype=torch.int32), _t(Bc, A), _t(16)
    pred, rows, total = _t(Bc, dtype=torch.int32), (_t(Bc) if row_score else None), _t(1)
    before = (_ptr(z), _ptr(ai), _ptr(sc), ai.shape[1], _ptr(pred), _ptr(rows), _ptr(total), _ptr(ws),
              Bc, K, _lib.F32, C.c_void_p(STREAM))
    bound = loss_mod._score_call(z, ai, sc, pred, rows, total, ws, STREAM)
    assert bound.name == "coattn_vqa_score" and _norm(bound) == _norm(before)
    assert _norm(before)[5] == (rows.data_ptr() if row_score else 0)


def test_status_bindings():
    ws, saved, acc = _t(16), _t(16), _t(2)
    Bc, dh, mlp, K = 3, 16, 12, 11
    before = (_ptr(ws), Bc, C.c_void_p(STREAM))                                    # loss.check_labels
    assert _norm(_lib.bind("coattn_ce_status", ws=ws, B=Bc, stream=STREAM)) == _norm(before)
    before = (_lib.ptr(saved), Bc, dh, mlp, K, C.c_void_p(STREAM))                 # head.check_labels
    assert _norm(_lib.bind("coattn_head_status", saved=saved, B=Bc, d=dh, mlp=mlp, K=K, stream=STREAM)) == _norm(before)
    # _lib.fold_range
    dims = (B, N, T, d, L)
    before = (C.c_void_p(saved.data_ptr()), *dims, _lib.F32, C.c_void_p(acc.data_ptr()), C.c_void_p(STREAM))
    bound = _lib.status_accumulate("coattn", saved, dims, acc, STREAM)
    assert bound.name == "coattn_status_accumulate" and _norm(bound) == _norm(before)
    dims = (2, 5, 8)
    before = (C.c_void_p(saved.data_ptr()), *dims, C.c_void_p(acc.data_ptr()), C.c_void_p(STREAM))
    bound = _lib.status_accumulate("phrase", saved, dims, acc, STREAM)
    assert bound.name == "coattn_phrase_status_accumulate" and _norm(bound) == _norm(before)


def test_a_status_call_hands_back_its_code(monkeypatch):
    """Call.code() returns what the entry point returns; check_label_status turns -2 into IndexError with the library's
    message, any other failure into check()'s RuntimeError."""
    call = _lib.bind("coattn_ce_status", ws=_t(4), B=1, stream=0)
    for rc in (0, -2, -1):
        call.fn = lambda *a, rc=rc: rc
        assert call.code() == rc
        if rc == 0:
            _lib.check_label_status(call)
        else:
            with pytest.raises(IndexError if rc == -2 else RuntimeError) as e:
                _lib.check_label_status(call)
            assert rc == -1 or str(e.value) == _lib.load().coattn_last_error().decode()


@pytest.mark.parametrize("clipped", (True, False))
def test_adam_step_binding(clipped):
    from vqa_amd import optim
    entries = [(_t(6), _t(6), _t(6), _t(6)), (_t(3), _t(3), _t(3), _t(3))]
    arr = (_lib.AdamTensor * len(entries))()
    for e, (p, g, m, v) in zip(arr, entries):
        e.p, e.g, e.m, e.v, e.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
    group = {"lr": 1e-3, "eps": 1e-8}
    beta1, beta2, wd, step, stream_ptr = 0.9, 0.999, 0.01, 3, STREAM
    clip, nbytes = (2.0, 512) if clipped else (0.0, 0)
    norm, ws = (_t(1), _t(128)) if clipped else (None, None)
    before = (arr, len(entries), step, float(group["lr"]), float(beta1), float(beta2),
              float(group["eps"]), wd, clip,
              C.c_void_p(norm.data_ptr() if norm is not None else 0),
              C.c_void_p(ws.data_ptr() if ws is not None else 0), nbytes,
              C.c_void_p(stream_ptr))
    bound = optim._step_call(arr, step, float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), wd, clip, norm, ws,
                             nbytes, stream_ptr)
    assert bound.name == "coattn_adam_step" and bound[0] is arr and _norm(bound[1:]) == _norm(before[1:])
    assert _norm(before)[9:12] == ((norm.data_ptr(), ws.data_ptr(), 512) if clipped else (0, 0, 0))


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_features_native_binding(dtype):
    from vqa_amd.coattention import _features_native_call
    x_img, out = torch.zeros(B, d, N, dtype=dtype).permute(0, 2, 1), _t(B, N, d)
    sB, sN, sD = _strides(x_img)
    before = (_ptr(x_img), _lib.BF16 if x_img.dtype == torch.bfloat16 else _lib.F32,
              sB, sN, sD, _ptr(out), B, N, d, C.c_void_p(STREAM))
    bound = _features_native_call(x_img, out, STREAM)
    assert bound.name == "coattn_features_native" and _norm(bound) == _norm(before)
    assert _norm(before)[1:5] == (int(dtype == torch.bfloat16), d * N, 1, N)


def _bn(Ch):
    return torch.nn.BatchNorm2d(Ch, momentum=0.25, eps=3e-5)


@pytest.mark.parametrize("pool", (True, False))
@pytest.mark.parametrize("with_bias", (True, False))
@pytest.mark.parametrize("with_stats", (True, False))
def test_encoder_pool_bindings(pool, with_bias, with_stats):
    from vqa_amd import encoder
    Be, Ch, H, W = 2, 16, 4, 6
    x, y, ws, bn = _t(Be, Ch, H, W), _t(Be, Ch, H // 2, W // 2), _t(16), _bn(Ch)
    conv_bias, stats_out = (_t(Ch) if with_bias else None), (_t(2, Ch) if with_stats else None)
    before = (_lib.ptr(x), _lib.ptr(bn.weight), _lib.ptr(bn.bias), _lib.ptr(conv_bias),
              _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var), float(bn.momentum),
              float(bn.eps), _lib.ptr(y), _lib.ptr(stats_out), _lib.ptr(ws), Be, H, W, Ch,
              int(pool), 1, _lib.F32, C.c_void_p(STREAM))
    bound = encoder._bn_relu_pool_call(x, bn, conv_bias, y, stats_out, ws, pool, STREAM)
    assert bound.name == "coattn_bn_relu_pool_forward" and _norm(bound) == _norm(before)
    assert _norm(before)[3] == (conv_bias.data_ptr() if with_bias else 0)
    assert _norm(before)[9] == (stats_out.data_ptr() if with_stats else 0) and _norm(before)[6:8] == (0.25, 3e-5)
    before = (_lib.ptr(x), _lib.ptr(y), Be, H, W, Ch, _lib.F32,
              C.c_void_p(STREAM))
    bound = encoder._relu_pool_call(x, y, STREAM)
    assert bound.name == "coattn_relu_pool_forward" and _norm(bound) == _norm(before)


@pytest.mark.parametrize("pool", (True, False))
def test_encoder_bn_exact_binding(pool):
    from vqa_amd import encoder
    Be, Ch, H, W = 2, 64, 4, 6
    x, y, save, ws, bn = _t(Be, Ch, H, W), _t(Be, Ch, H, W), _t(2, Ch), _t(16), _bn(Ch)
    weight, bias, running_mean, running_var, momentum, eps = bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps
    before = (_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(running_mean),
              _lib.ptr(running_var), float(momentum), float(eps), _lib.ptr(y), _lib.ptr(save[0]),
              _lib.ptr(save[1]), _lib.ptr(ws), Be, H, W, Ch, int(pool), 1, _lib.F32,
              C.c_void_p(STREAM))
    bound = encoder._bn_exact_call(x, weight, bias, running_mean, running_var, momentum, eps, y, save, ws, pool, STREAM)
    assert bound.name == "coattn_bn_exact_forward" and _norm(bound) == _norm(before)
    assert _norm(before)[9] == _norm(before)[8] + 4 * Ch and _norm(before)[15] == int(pool)


@pytest.mark.parametrize("pool", (True, False))
@pytest.mark.parametrize("form", ("x_out", "x in ws", "recompute"))
def test_encoder_conv1_bindings(pool, form):
    from vqa_amd import encoder
    Be, H, W = 2, 8, 6
    image, weight, y, save, ws, bn = _t(Be, 3, H, W), _t(64, 3, 3, 3), _t(Be, 64, H, W), _t(2, 64), _t(16), _bn(64)
    gamma, beta, running_mean, running_var, momentum, eps = bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps
    x = _t(Be, 64, H, W) if form == "x_out" else None
    args = (image, weight, gamma, beta, running_mean, running_var, momentum, eps, y, save, ws, pool, STREAM)
    if form == "recompute":
        # (this call was bound by name already: its positional form is the stored form's without x_out)
        before = (_lib.ptr(image), _lib.ptr(weight), _lib.ptr(gamma), _lib.ptr(beta),
                  _lib.ptr(running_mean), _lib.ptr(running_var), float(momentum), float(eps),
                  _lib.ptr(y), _lib.ptr(save[0]), _lib.ptr(save[1]), _lib.ptr(ws), Be, H, W,
                  3, 64, int(pool), _lib.F32, C.c_void_p(STREAM))
        bound = encoder._conv1_call(*args)
        assert bound.name == "coattn_conv1_bn_recompute_forward"
    else:
        before = (_lib.ptr(image), _lib.ptr(weight), _lib.ptr(gamma), _lib.ptr(beta),
                  _lib.ptr(running_mean), _lib.ptr(running_var), float(momentum), float(eps),
                  _lib.ptr(x), _lib.ptr(y), _lib.ptr(save[0]), _lib.ptr(save[1]), _lib.ptr(ws), Be, H, W,
                  3, 64, int(pool), _lib.F32, C.c_void_p(STREAM))
        bound = encoder._conv1_call(*args, x_out=x)
        assert bound.name == "coattn_conv1_bn_exact_forward" and _norm(before)[8] == (x.data_ptr() if x is not None else 0)
    assert _norm(bound) == _norm(before) and len(bound) == len(_lib.SIGNATURES[bound.name])


def test_p2p_bindings():
    from types import SimpleNamespace
    from vqa_amd.dist import GradReducer
    world = 4
    peers = [_t(8 * world) for _ in range(world)]
    b = SimpleNamespace(flat=peers[1], peer_ptrs=(C.c_void_p * world)(*[t.data_ptr() for t in peers]))
    self = SimpleNamespace(world=world, rank=1)
    stream = STREAM
    before = (b.peer_ptrs, self.world, self.rank, b.flat.numel() // self.world,
              1.0 / self.world, stream)
    bound = GradReducer._p2p_call(self, "coattn_p2p_reduce_scatter", b, stream, scale=1.0 / self.world)
    assert bound.name == "coattn_p2p_reduce_scatter" and _norm(bound) == _norm(before)
    before = (b.peer_ptrs, self.world, self.rank, b.flat.numel() // self.world,
              stream)
    bound = GradReducer._p2p_call(self, "coattn_p2p_all_gather", b, stream)
    assert bound.name == "coattn_p2p_all_gather" and _norm(bound) == _norm(before)
    assert _norm(_lib.ptr_array(peers)) == _norm(b.peer_ptrs)


@pytest.mark.parametrize("labels", (True, False))
def test_head_forward_binding_with_and_without_labels(labels):
    Bh, dh, mlp, K = 8, 16, 12, 11
    v, q, logits, saved = _t(3, Bh, dh), _t(3, Bh, dh), _t(Bh, K), _t(16)
    lab, loss = (_t(Bh, dtype=torch.int64), _t(1)) if labels else (None, None)
    hp = _lib.HeadParams(*[_t(4).data_ptr() for _ in range(8)])
    rv, rq = _lib.rows(v), _lib.rows(q)
    before = (rv, rq, C.byref(hp), _ptr(lab), _ptr(logits), _ptr(loss), _ptr(saved), Bh, dh, mlp, K, _lib.F32, 0, C.c_void_p(STREAM))
    kw = dict(v=rv, q=rq, p=hp, logits=logits, saved=saved, B=Bh, d=dh, mlp=mlp, K=K, dtype=_lib.F32, flags=0, stream=STREAM)
    assert _norm(_lib.bind("coattn_head_forward", labels=lab, loss=loss, **kw)) == _norm(before)
    if not labels:
        assert _norm(_lib.bind("coattn_head_forward", **kw)) == _norm(before) and _norm(before)[3] == _norm(before)[5] == 0

"""Differentiable attention maps (C-ABI 0.9.0: coattn_forward_maps(_len) / coattn_backward_maps(_len);
ParallelCoAttention.forward(..., return_attention=True); HierarchicalCoAttentionNet.forward_features(..., return_attention=True))
on the GPU.

The reference for every gradient is autograd of oracle.coattn_oracle.coattn_forward in float64 on the loss
    sum <R_v, v> + sum <R_q, q> + sum <G_av, a_v> + sum <G_aq, a_q>,
so R_v / R_q are the upstream gradients g_v / g_q and G_av / G_aq those of the maps.  Under the length mask the oracle is the
reference's computation on Q[b, :len_b] alone (as tests/test_gpu_masked.py builds it)."""
import ctypes as C

import pytest
import torch

import vqa_amd
from oracle import coattn_oracle as O
from tests._hip import saved_views
from vqa_amd import _lib

pytestmark = pytest.mark.gpu

NAMES = ("W_v.weight", "W_v.bias", "W_q.weight", "W_q.bias", "w_v.weight", "w_v.bias", "w_q.weight", "w_q.bias")
GRADS = ["dV_phys", "dQ"] + ["d" + k for k in NAMES]
DEV = "cuda:0"


def _flags(mode, impl):
    f = {"general": _lib.IMPL_GENERAL, "fused": _lib.IMPL_FUSED, "auto": _lib.IMPL_AUTO}[impl]
    return f | {"exact": 0, "fast16": _lib.FLAG_FAST16, "bf16": _lib.FLAG_BF16_PROJ}[mode]


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def call(V, Qs, P, lens=None, gv=None, gq=None, g_av=None, g_aq=None, mode="exact", impl="fused", layout="lm",
         api="maps", accumulate=0, grads_init=None, api_bwd=None, Qs_bwd=None, saved=None):
    """One forward (+ backward) through the C-ABI.  api: "maps" (coattn_forward_maps / coattn_backward_maps), "maps_zero"
    (the same with g_av / g_aq given as zero tensors where they are None), "plain" (coattn_forward / coattn_backward) or
    "infer" (coattn_infer).  lens: None (the unmasked entry points) or host ints (the *_len ones).  V [B,d,N] values, handed
    over in the physical `layout`.  Every output buffer is NaN-filled first.
    api_bwd: the backward's family when it differs from the forward's ("plain" / "maps"); Qs_bwd: other device tensors (same
    values) as the backward's Q; saved: a caller-owned state buffer, used as it is (not refilled).  Device tensors in Qs /
    Qs_bwd that are contiguous are handed over at their own addresses (views at an offset included)."""
    lib = _lib.load()
    V = V.to(DEV).contiguous()
    B, d, N = V.shape
    Vbuf, vstr = (V.permute(0, 2, 1).contiguous(), (N * d, d, 1)) if layout == "lm" else (V, (d * N, 1, N))
    Qs = [q.to(DEV).contiguous() for q in Qs]
    L, T = len(Qs), Qs[0].shape[1]
    ps = [P[k].to(DEV).contiguous() for k in NAMES]
    flag = _flags(mode, impl)
    sb, fb, bb = _lib.workspace_bytes(B, N, T, d, L, flag)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)   # noqa: E731
    v, q, a_v, a_q = nan(L, B, d), nan(L, B, d), nan(L, B, N), nan(L, B, T)
    ql = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    qa = () if ql is None else (C.c_void_p(ql.data_ptr()),)
    sfx = "" if ql is None else "_len"
    qptr = (C.c_void_p * L)(*[t.data_ptr() for t in Qs])
    p = _lib.Params(*[t.data_ptr() for t in ps])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = nan(fb // 4)
    if api == "infer":
        _lib.check(getattr(lib, "coattn_infer" + sfx)(Vbuf.data_ptr(), *vstr, qptr, *qa, C.byref(p), v.data_ptr(),
                                                      q.data_ptr(), a_v.data_ptr(), a_q.data_ptr(), ws.data_ptr(), B, N, T,
                                                      d, L, _lib.F32, flag, st), "infer")
        torch.cuda.synchronize()
        return {"v": v, "q": q, "a_v": a_v, "a_q": a_q}
    saved = nan(sb // 4) if saved is None else saved
    if api == "plain":
        _lib.check(getattr(lib, "coattn_forward" + sfx)(Vbuf.data_ptr(), *vstr, qptr, *qa, C.byref(p), v.data_ptr(),
                                                        q.data_ptr(), saved.data_ptr(), ws.data_ptr(), B, N, T, d, L,
                                                        _lib.F32, flag, st), "forward")
        out = {"v": v, "q": q}
    else:
        _lib.check(getattr(lib, "coattn_forward_maps" + sfx)(Vbuf.data_ptr(), *vstr, qptr, *qa, C.byref(p), v.data_ptr(),
                                                             q.data_ptr(), a_v.data_ptr(), a_q.data_ptr(), saved.data_ptr(),
                                                             ws.data_ptr(), B, N, T, d, L, _lib.F32, flag, st),
                   "forward_maps")
        out = {"v": v, "q": q, "a_v": a_v, "a_q": a_q}
    torch.cuda.synchronize()
    out["saved"] = saved
    out["saved_views"] = saved_views(saved, B, N, T, d, L)
    if gv is None:
        return out
    gv, gq = gv.to(DEV).contiguous(), gq.to(DEV).contiguous()
    if api == "maps_zero":
        g_av = torch.zeros(L, B, N) if g_av is None else g_av
        g_aq = torch.zeros(L, B, T) if g_aq is None else g_aq
    g_av = None if g_av is None else g_av.to(DEV).contiguous()
    g_aq = None if g_aq is None else g_aq.to(DEV).contiguous()
    ws2 = nan(bb // 4)
    dV = torch.full_like(Vbuf, float("nan"))
    dQs = [torch.full_like(t, float("nan")) for t in Qs]
    grads = [torch.full_like(t, float("nan")) for t in ps] if grads_init is None else [g.to(DEV).clone() for g in grads_init]
    pg = _lib.ParamGrads(*[t.data_ptr() for t in grads])
    dqptr = (C.c_void_p * L)(*[t.data_ptr() for t in dQs])
    tail = (dV.data_ptr(), *vstr, dqptr, C.byref(pg), accumulate, ws2.data_ptr(), B, N, T, d, L, _lib.F32, flag, st)
    if Qs_bwd is not None:
        qptr = (C.c_void_p * L)(*[t.data_ptr() for t in Qs_bwd])
    if (api_bwd or api) == "plain":
        _lib.check(getattr(lib, "coattn_backward" + sfx)(Vbuf.data_ptr(), *vstr, qptr, *qa, C.byref(p), saved.data_ptr(),
                                                         gv.data_ptr(), gq.data_ptr(), *tail), "backward")
    else:
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        _lib.check(getattr(lib, "coattn_backward_maps" + sfx)(Vbuf.data_ptr(), *vstr, qptr, *qa, C.byref(p),
                                                              saved.data_ptr(), gv.data_ptr(), gq.data_ptr(), ptr(g_av),
                                                              ptr(g_aq), *tail), "backward_maps")
    torch.cuda.synchronize()
    out["dV_phys"] = dV.permute(0, 2, 1).contiguous() if layout == "lm" else dV
    out["dQ"] = torch.stack(dQs)
    for k, g in zip(NAMES, grads):
        out["d" + k] = g
    return out


def oracle(V, Qs, P, lens, Rv, Rq, Gav, Gaq):
    """float64 autograd of the oracle forward on sum <R_v,v> + <R_q,q> + <G_av,a_v> + <G_aq,a_q>; lens (or None): per group
    of equal (clamped) lengths, the reference on the truncated questions, a_q zero-padded."""
    L, B, T = len(Qs), V.shape[0], Qs[0].shape[1]
    P64 = {k: t.detach().double().requires_grad_(True) for k, t in P.items()}
    V64 = V.detach().double().requires_grad_(True)
    Q64 = [q.detach().double().requires_grad_(True) for q in Qs]
    ln = [T] * B if lens is None else [min(max(int(x), 1), T) for x in lens]
    o = {"v": torch.zeros(L, B, V.shape[1], dtype=torch.float64), "q": torch.zeros(L, B, V.shape[1], dtype=torch.float64),
         "a_v": torch.zeros(L, B, V.shape[2], dtype=torch.float64), "a_q": torch.zeros(L, B, T, dtype=torch.float64)}
    loss = 0.
    for t in sorted(set(ln)):
        idx = torch.tensor([b for b in range(B) if ln[b] == t])
        f = O.coattn_forward(V64[idx], [q[idx, :t] for q in Q64], P64)
        loss = loss + (Rv.double()[:, idx] * f["v"]).sum() + (Rq.double()[:, idx] * f["q"]).sum()
        loss = loss + (Gav.double()[:, idx] * f["a_v"]).sum() + (Gaq.double()[:, idx, :t] * f["a_q"]).sum()
        o["v"][:, idx], o["q"][:, idx], o["a_v"][:, idx] = f["v"].detach(), f["q"].detach(), f["a_v"].detach()
        o["a_q"][:, idx, :t] = f["a_q"].detach()
    loss.backward()
    o["dV_phys"] = V64.grad
    o["dQ"] = torch.stack([q.grad for q in Q64])
    for k in NAMES:
        o["d" + k] = P64[k].grad
    return o


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def err(r, o, k):
    """max|err| / max|ref|; absolute for dc_v / dc_q, which are 0 analytically (softmax shift invariance)."""
    if k in ("dw_v.bias", "dw_q.bias"):
        return float((r[k].detach().double().cpu() - o[k]).abs().max())
    return rel(r[k], o[k])


def case(B, N, T, d, lens=None, seed=3, maps_only=False, gscale=4.0):
    """Inputs (question rows past each length are zeros, the reference's pad tokens), upstream gradients R of v / q (zero
    for a maps-only loss) and G of the maps."""
    P = O.make_params(d, seed)
    V, Qs = O.make_inputs(B, N, T, d, seed + 10, lens=lens, scale_q=(2.0 / d) ** 0.5)
    L = len(Qs)
    gv = torch.from_numpy(O.hash_normal((L, B, d), seed + 5)).float()
    gq = torch.from_numpy(O.hash_normal((L, B, d), seed + 6)).float()
    if maps_only:
        gv, gq = torch.zeros_like(gv), torch.zeros_like(gq)
    g_av = torch.from_numpy(O.hash_normal((L, B, N), seed + 7, gscale)).float()
    g_aq = torch.from_numpy(O.hash_normal((L, B, T), seed + 8, gscale)).float()
    return V, Qs, P, gv, gq, g_av, g_aq


def mixed_lens(B, T):
    return [[1, T, 2, T - 1, 3, T // 2][b % 6] if b < 6 else 1 + (b * 7) % T for b in range(B)]


# ---- 1. forward identity ------------------------------------------------------------------------------------------------
# (B, N, T, d, impl); the general path: d = 64 / 96 (no fused kernel below d % 256) and T > 28
SHAPES = {"n49": (6, 49, 26, 512, "fused"), "n196": (4, 196, 26, 512, "fused"), "general_d64_t32": (4, 49, 32, 64, "auto"),
          "general_d96": (5, 49, 12, 96, "auto"), "cfg4_d2048": (4, 49, 26, 2048, "fused")}
MODES = ("exact", "fast16", "bf16")
FWD_CASES = [(s, m) for s in SHAPES for m in MODES
             if (m != "bf16" or SHAPES[s][3] % 512 == 0) and (s != "cfg4_d2048" or m != "fast16")]


@pytest.mark.parametrize("shape,mode", FWD_CASES, ids=["%s-%s" % c for c in FWD_CASES])
@pytest.mark.parametrize("layout", ["lm", "cm"])
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_forward_maps_is_the_saving_forward_plus_the_inference_maps(shape, mode, layout, masked):
    B, N, T, d, impl = SHAPES[shape]
    if impl == "auto":
        assert not _lib.load().coattn_fused_supported(B, N, T, d, 3, 0)
    lens = mixed_lens(B, T) if masked else None
    V, Qs, P, *_ = case(B, N, T, d, lens, seed=11)
    m = call(V, Qs, P, lens, mode=mode, impl=impl, layout=layout, api="maps")
    f = call(V, Qs, P, lens, mode=mode, impl=impl, layout=layout, api="plain")
    i = call(V, Qs, P, lens, mode=mode, impl=impl, layout=layout, api="infer")
    assert same_bits(m["v"], f["v"]) and same_bits(m["q"], f["q"])
    assert same_bits(m["saved"], f["saved"])                   # (every word: NaN-filled alike, written alike)
    assert same_bits(m["a_v"], i["a_v"]) and same_bits(m["a_q"], i["a_q"])
    assert same_bits(m["a_v"], m["saved_views"]["a_v"]) and same_bits(m["a_q"], m["saved_views"]["a_q"])
    assert not torch.isnan(m["a_v"]).any() and not torch.isnan(m["a_q"]).any()


# ---- 2. backward without map gradients ----------------------------------------------------------------------------------
BWD_CASES = [(s, m) for s in ("n49", "n196", "general_d96", "cfg4_d2048") for m in MODES
             if (m != "bf16" or SHAPES[s][3] % 512 == 0) and (s != "cfg4_d2048" or m == "bf16")]


@pytest.mark.parametrize("shape,mode", BWD_CASES, ids=["%s-%s" % c for c in BWD_CASES])
@pytest.mark.parametrize("layout", ["lm", "cm"])
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_backward_maps_without_map_gradients_is_the_plain_backward(shape, mode, layout, masked):
    B, N, T, d, impl = SHAPES[shape]
    lens = mixed_lens(B, T) if masked else None
    V, Qs, P, gv, gq, _, _ = case(B, N, T, d, lens, seed=13)
    kw = dict(mode=mode, impl=impl, layout=layout)
    ref = call(V, Qs, P, lens, gv, gq, api="plain", **kw)
    for api in ("maps", "maps_zero"):                          # NULL map gradients, and zero tensors
        r = call(V, Qs, P, lens, gv, gq, api=api, **kw)
        for k in GRADS:
            assert same_bits(r[k], ref[k]), (api, k)
    # accumulate = 1 adds onto the caller's parameter gradients in the same way
    init = [torch.from_numpy(O.hash_normal(tuple(P[k].shape), 90 + i)).float() for i, k in enumerate(NAMES)]
    ref = call(V, Qs, P, lens, gv, gq, api="plain", accumulate=1, grads_init=init, **kw)
    r = call(V, Qs, P, lens, gv, gq, api="maps", accumulate=1, grads_init=init, **kw)
    for k in GRADS:
        assert same_bits(r[k], ref[k]), ("accumulate", k)


# ---- 3. gradients against float64 -----------------------------------------------------------------------------------------
SMALL = {"n49_d256": (6, 49, 12, 256, "fused"), "n64_d512": (5, 64, 7, 512, "fused"), "n100_d256": (4, 100, 26, 256, "fused"),
         "general_t40": (4, 49, 40, 256, "auto"), "general_d96": (5, 49, 12, 96, "auto")}
TOL = {"exact": 2e-5, "fast16": 1e-4}


@pytest.mark.parametrize("shape", list(SMALL))
@pytest.mark.parametrize("layout", ["lm", "cm"])
@pytest.mark.parametrize("mode", ["exact", "fast16"])
@pytest.mark.parametrize("maps_only", [False, True], ids=["full_loss", "maps_only"])
def test_small_shapes_vs_float64(shape, layout, mode, maps_only):
    B, N, T, d, impl = SMALL[shape]
    V, Qs, P, gv, gq, g_av, g_aq = case(B, N, T, d, mixed_lens(B, T), seed=17, maps_only=maps_only)
    r = call(V, Qs, P, None, gv, gq, g_av, g_aq, mode=mode, impl=impl, layout=layout)
    o = oracle(V, Qs, P, None, gv, gq, g_av, g_aq)
    for k in ("v", "q", "a_v", "a_q") + tuple(GRADS):
        assert err(r, o, k) < TOL[mode], (k, err(r, o, k))


_ORACLE_CACHE = {}


def _cfg2(N, masked):
    B, T, d = 160, 26, 512
    lens = mixed_lens(B, T)
    key = (N, masked)
    V, Qs, P, gv, gq, g_av, g_aq = case(B, N, T, d, lens, seed=19)
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE[key] = oracle(V, Qs, P, lens if masked else None, gv, gq, g_av, g_aq)
    return (V, Qs, P, gv, gq, g_av, g_aq), (lens if masked else None), _ORACLE_CACHE[key]


@pytest.mark.parametrize("N", [49, 196])
@pytest.mark.parametrize("layout", ["lm", "cm"])
@pytest.mark.parametrize("mode", ["exact", "fast16"])
def test_cfg2_vs_float64(N, layout, mode):
    (V, Qs, P, gv, gq, g_av, g_aq), _, o = _cfg2(N, False)
    r = call(V, Qs, P, None, gv, gq, g_av, g_aq, mode=mode, layout=layout)
    for k in ("v", "q", "a_v", "a_q") + tuple(GRADS):
        assert err(r, o, k) < TOL[mode], (k, err(r, o, k))


def test_reduced_precision_cfg4_shape_vs_float64():
    """cfg 4's width on the single-product (bf16) instantiations, at the bounds of the unmasked bf16 tests (3e-2 absolute
    on v / q, 5e-2 of max|.| on the gradients), masked and not."""
    B, N, T, d = 8, 49, 26, 2048
    for lens in (None, mixed_lens(B, T)):
        V, Qs, P, gv, gq, g_av, g_aq = case(B, N, T, d, mixed_lens(B, T), seed=29)
        o = oracle(V, Qs, P, lens, gv, gq, g_av, g_aq)
        for layout in ("lm", "cm"):
            r = call(V, Qs, P, lens, gv, gq, g_av, g_aq, mode="bf16", layout=layout)
            for k in ("v", "q"):
                assert float((r[k].double().cpu() - o[k]).abs().max()) < 3e-2, (layout, k)
            for k in GRADS:
                assert err(r, o, k) < 5e-2, (lens is None, layout, k, err(r, o, k))


# ---- 4. the length mask ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["n49_d256", "n64_d512", "general_t40", "general_d96"])
@pytest.mark.parametrize("layout", ["lm", "cm"])
@pytest.mark.parametrize("mode", ["exact", "fast16"])
def test_masked_small_shapes_vs_truncated_float64(shape, layout, mode):
    B, N, T, d, impl = SMALL[shape]
    lens = mixed_lens(B, T)
    V, Qs, P, gv, gq, g_av, g_aq = case(B, N, T, d, lens, seed=23)
    r = call(V, Qs, P, lens, gv, gq, g_av, g_aq, mode=mode, impl=impl, layout=layout)
    o = oracle(V, Qs, P, lens, gv, gq, g_av, g_aq)
    for k in ("v", "q", "a_v", "a_q") + tuple(GRADS):
        assert err(r, o, k) < TOL[mode], (k, err(r, o, k))
    for b, n in enumerate(lens):
        assert (r["a_q"][:, b, n:] == 0).all() and (r["dQ"][:, b, n:] == 0).all()


@pytest.mark.parametrize("N", [49, 196])
@pytest.mark.parametrize("mode", ["exact", "fast16"])
def test_masked_cfg2_vs_truncated_float64(N, mode):
    (V, Qs, P, gv, gq, g_av, g_aq), lens, o = _cfg2(N, True)
    r = call(V, Qs, P, lens, gv, gq, g_av, g_aq, mode=mode, layout="lm")
    for k in ("v", "q", "a_v", "a_q") + tuple(GRADS):
        assert err(r, o, k) < TOL[mode], (k, err(r, o, k))


@pytest.mark.parametrize("shape", ["n49", "n196", "general_d96"])
@pytest.mark.parametrize("layout", ["lm", "cm"])
@pytest.mark.parametrize("mode", ["exact", "fast16"])
def test_pad_slots_of_the_question_map_gradient_are_not_read(shape, layout, mode):
    B, N, T, d, impl = SHAPES[shape]
    lens = mixed_lens(B, T)
    V, Qs, P, gv, gq, g_av, g_aq = case(B, N, T, d, lens, seed=31)
    junk = g_aq.clone()
    for b, n in enumerate(lens):
        junk[:, b, n:] = torch.tensor([float("nan"), float("inf"), -float("inf"), 1e30])[torch.arange(T - n) % 4]
        g_aq[:, b, n:] = 0.
    assert torch.isnan(junk).any()
    z = call(V, Qs, P, lens, gv, gq, g_av, g_aq, mode=mode, impl=impl, layout=layout)
    j = call(V, Qs, P, lens, gv, gq, g_av, junk, mode=mode, impl=impl, layout=layout)
    for k in GRADS:
        assert same_bits(z[k], j[k]), k
        assert torch.isfinite(j[k]).all(), k


@pytest.mark.parametrize("shape,mode", [("n49", "exact"), ("n196", "fast16"), ("general_d96", "exact")])
@pytest.mark.parametrize("layout", ["lm", "cm"])
def test_lengths_at_T_are_the_unmasked_maps_calls_bit_for_bit(shape, mode, layout):
    B, N, T, d, impl = SHAPES[shape]
    V, Qs, P, gv, gq, g_av, g_aq = case(B, N, T, d, [3, 1, T, 5, 2, T][:B], seed=37)
    a = call(V, Qs, P, None, gv, gq, g_av, g_aq, mode=mode, impl=impl, layout=layout)
    b = call(V, Qs, P, [T] * B, gv, gq, g_av, g_aq, mode=mode, impl=impl, layout=layout)
    for k in ("v", "q", "a_v", "a_q") + tuple(GRADS):
        assert same_bits(a[k], b[k]), k


# ---- 5. the module ----------------------------------------------------------------------------------------------------------
def _kl(target, a):
    """sum over levels of the batch-mean KL(target || a) over the last axis"""
    return (target * (target.clamp_min(1e-30).log() - a.clamp_min(1e-30).log())).sum(-1).mean(-1).sum()


def _module_case(B=6, N=49, T=12, d=512, seed=41):
    P = O.make_params(d, seed)
    V, Qs = O.make_inputs(B, N, T, d, seed + 10, lens=mixed_lens(B, T), scale_q=(2.0 / d) ** 0.5)
    Rv = torch.from_numpy(O.hash_normal((3, B, d), seed + 5)).float()
    Rq = torch.from_numpy(O.hash_normal((3, B, d), seed + 6)).float()
    tv = torch.softmax(torch.from_numpy(O.hash_normal((3, B, N), seed + 7, 2.0)).float(), -1)
    tq = torch.softmax(torch.from_numpy(O.hash_normal((3, B, T), seed + 8, 2.0)).float(), -1)
    return P, V, Qs, Rv, Rq, tv, tq


def _module(P, d, fast):
    m = vqa_amd.ParallelCoAttention(d)
    m.load_state_dict({k: v.clone() for k, v in P.items()}, strict=False)
    m.fast_products = fast
    return m.to(DEV)


@pytest.mark.parametrize("layout", ["lm", "cm"])
@pytest.mark.parametrize("mode", ["exact", "fast16"])
def test_module_attention_kl_vs_float64(layout, mode):
    P, V, Qs, Rv, Rq, tv, tq = _module_case()
    d = V.shape[1]
    m = _module(P, d, mode == "fast16")
    Vd = V.to(DEV) if layout == "cm" else V.permute(0, 2, 1).contiguous().to(DEV)
    Vd.requires_grad_(True)
    x = Vd.permute(0, 2, 1) if layout == "cm" else Vd           # x_img [B,N,d], dV flows (--vgg_train)
    Qg = [q.to(DEV).requires_grad_(True) for q in Qs]
    vs, qs, a_v, a_q = m(x, Qg, return_attention=True)
    assert a_v.requires_grad and a_q.requires_grad
    loss = (sum((vs[l] * Rv[l].to(DEV)).sum() + (qs[l] * Rq[l].to(DEV)).sum() for l in range(3))
            + _kl(tv.to(DEV), a_v) + 0.5 * _kl(tq.to(DEV), a_q))
    loss.backward()
    # float64 reference
    P64 = {k: t.double().requires_grad_(True) for k, t in P.items()}
    V64 = V.double().requires_grad_(True)
    Q64 = [q.double().requires_grad_(True) for q in Qs]
    f = O.coattn_forward(V64, Q64, P64)
    loss64 = ((Rv.double() * f["v"]).sum() + (Rq.double() * f["q"]).sum() + _kl(tv.double(), f["a_v"])
              + 0.5 * _kl(tq.double(), f["a_q"]))
    loss64.backward()
    assert abs(float(loss.detach()) - float(loss64.detach())) < 1e-5 * abs(float(loss64.detach()))
    dV = Vd.grad if layout == "cm" else Vd.grad.permute(0, 2, 1)
    assert rel(dV, V64.grad) < TOL[mode]
    for l in range(3):
        assert rel(Qg[l].grad, Q64[l].grad) < TOL[mode], l
    mp = dict(m.named_parameters())
    for k in NAMES:
        e = (float((mp[k].grad.double().cpu() - P64[k].grad).abs().max()) if k in ("w_v.bias", "w_q.bias")
             else rel(mp[k].grad, P64[k].grad))
        assert e < TOL[mode], (k, e)
    assert mp["W_b.weight"].grad is None


@pytest.mark.parametrize("mode", ["exact", "fast16"])
def test_module_with_unused_maps_has_the_plain_gradients_bit_for_bit(mode):
    P, V, Qs, Rv, Rq, _, _ = _module_case(seed=43)
    d = V.shape[1]
    res = []
    for ret in (False, True):
        m = _module(P, d, mode == "fast16")
        Vd = V.permute(0, 2, 1).contiguous().to(DEV).requires_grad_(True)
        Qg = [q.to(DEV).requires_grad_(True) for q in Qs]
        out = m(Vd, Qg, return_attention=ret)
        vs, qs = out[0], out[1]
        (sum((vs[l] * Rv[l].to(DEV)).sum() + (qs[l] * Rq[l].to(DEV)).sum() for l in range(3))).backward()
        assert m.W_b.weight.grad is None and m.W_b.bias.grad is None          # (dead in the reference's forward)
        res.append(([*vs, *qs], [Vd.grad, *[q.grad for q in Qg]] + [m.get_parameter(k).grad for k in NAMES]))
    for a, b in zip(res[0][0] + res[0][1], res[1][0] + res[1][1]):
        assert same_bits(a, b)


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_module_under_no_grad_is_forward_with_attention(masked):
    P, V, Qs, *_ = _module_case(seed=47)
    B, d, N = V.shape
    T = Qs[0].shape[1]
    m = _module(P, d, False)
    m.question_mask = masked
    lens = mixed_lens(B, T) if masked else None
    x = V.permute(0, 2, 1).contiguous().to(DEV)
    Qg = [q.to(DEV) for q in Qs]
    with torch.no_grad():
        a = m(x, Qg, lens, return_attention=True)
        b = m.forward_with_attention(x, Qg, lens)
    assert len(a) == 4
    for u, w in zip([*a[0], *a[1], a[2], a[3]], [*b[0], *b[1], b[2], b[3]]):
        assert same_bits(u, w)
    if masked:
        for bi, n in enumerate(lens):
            assert (a[3][:, bi, n:] == 0).all()


# ---- 6. the network ---------------------------------------------------------------------------------------------------------
class _OracleMapsCoAttention(O.OracleParallelCoAttention):
    """The oracle co-attention as a module under CPU autograd, with the maps; under question_mask per sample the reference
    on Q[b, :len_b] (a_q zero-padded)."""

    def __init__(self, hidden_dim, question_mask):
        super().__init__(hidden_dim)
        self.question_mask = question_mask

    def forward(self, x_img, x_ques_hierarchy, x_ques_lens=None, return_attention=False):
        P = {k: v for k, v in self.named_parameters()}
        qs = list(x_ques_hierarchy)
        B, T = x_img.shape[0], qs[0].shape[1]
        lens = [int(x) for x in x_ques_lens] if self.question_mask else [T] * B
        vs, qv, avs, aqs = [], [], [], []
        for b, n in enumerate(lens):
            r = O.coattn_forward(x_img[b:b + 1].permute(0, 2, 1), [q[b:b + 1, :n] for q in qs], P)
            vs.append(r["v"]); qv.append(r["q"]); avs.append(r["a_v"])
            aqs.append(torch.nn.functional.pad(r["a_q"], (0, T - n)))
        v, q = torch.cat(vs, 1), torch.cat(qv, 1)
        out = [v[l] for l in range(v.shape[0])], [q[l] for l in range(q.shape[0])]
        return (*out, torch.cat(avs, 1), torch.cat(aqs, 1)) if return_attention else out


@pytest.mark.parametrize("question_mask", [False, True], ids=["unmasked", "masked"])
def test_net_attention_supervision_matches_the_float64_composition(question_mask):
    """HierarchicalCoAttentionNet.forward_features(..., labels, return_attention=True) and the loss CE + lambda KL(target || a_v)
    over the three levels on the GPU, against the same net in float64 on the CPU with the oracle co-attention swapped in: loss
    and every non-encoder gradient, from the same image features."""
    from vqa_amd import train as T
    dev = torch.device(DEV)
    b = T.synthetic_batch(8, (64, 64), 26, 100, 11, seed=1)
    im, qu, la, ln = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
    torch.manual_seed(0)
    net = T.build_model("attention", 100, 10, question_mask=question_mask)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        feats = net.image_encoder(im).detach()                    # one set of features for both sides
    N = feats.shape[1]
    target = torch.softmax(torch.from_numpy(O.hash_normal((3, 8, N), 5, 2.0)).float(), -1)
    lam = 0.7
    gpu = net.to(dev)
    gpu.hot_path_static = True                                    # (ignored with return_attention: the per-module path)
    logits, ce, a_v, a_q = gpu.forward_features(feats.to(dev), qu.to(dev), ln, labels=la.to(dev), return_attention=True)
    assert not gpu._graphs
    loss = ce + lam * _kl(target.to(dev), a_v)
    loss.backward()
    ref = T.build_model("attention", 100, 10)
    ref.co_attention = _OracleMapsCoAttention(ref.hidden_dim, question_mask)
    ref.load_state_dict(sd)
    ref = ref.double()
    _, ce64, a_v64, a_q64 = ref.forward_features(feats.double(), qu, ln, labels=la, return_attention=True)
    loss64 = ce64 + lam * _kl(target.double(), a_v64)
    loss64.backward()
    assert abs(float(loss.detach()) - float(loss64.detach())) < 1e-5 * abs(float(loss64.detach()))
    assert rel(a_v, a_v64) < 1e-5 and rel(a_q, a_q64) < 1e-5
    if question_mask:
        for bi, n in enumerate(ln.tolist()):
            assert (a_q[:, bi, n:] == 0).all()
    gp = dict(gpu.named_parameters())
    checked = 0
    for n, p in ref.named_parameters():
        if p.grad is None or n.startswith("image_encoder"):
            continue
        assert gp[n].grad is not None, n
        if n.endswith("w_v.bias") or n.endswith("w_q.bias"):    # 0 analytically (softmax shift invariance): absolute
            e = float((gp[n].grad.double().cpu() - p.grad).abs().max())
        else:
            e = rel(gp[n].grad, p.grad)
        assert e < 1e-4, (n, e)
        checked += 1
    assert checked >= 20 and gp["co_attention.W_b.weight"].grad is None

"""The bilinear affinity (include/coattn.h, COATTN_FLAG_BILINEAR) on the GPU: C-ABI outputs and every gradient against the
float64 oracle of tests/_bilinear.py, in both arithmetic modes, both feature layouts, masked and with map gradients; the
identities it must keep; the refusals; and the module / hot-path / Trainer surface."""
import ctypes as C

import pytest
import torch

import vqa_amd
from vqa_amd import _lib
from oracle import coattn_oracle as O

from tests import _bilinear as BL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PNAMES = BL.NAMES
GRADS = ("dV_phys", "dQ") + tuple("d" + k for k in PNAMES)
MODES = (("exact", 0), ("fast16", _lib.FLAG_FAST16))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def case(B, N, T, d, lens=None, seed=3, L=3):
    P = O.make_params(d, seed)
    V, Qs = O.make_inputs(B, N, T, d, seed + 10, lens=lens, scale_q=(2.0 / d) ** 0.5, L=L)
    gv = torch.from_numpy(O.hash_normal((L, B, d), seed + 20)).float()
    gq = torch.from_numpy(O.hash_normal((L, B, d), seed + 21)).float()
    return V, Qs, P, gv, gq


def run(V, Qs, P, gv=None, gq=None, flags=0, layout="lm", lens=None, g_av=None, g_aq=None, accumulate=0, grads_init=None,
        null_wb=False, null_dwb=False, infer=False, maps=False, expect_rc=0):
    """One C-ABI forward (+ backward with gv / gq) under flags | COATTN_FLAG_BILINEAR.  V [B,d,N] values; layout "lm" hands
    a [B,N,d] buffer, "cm" the [B,d,N] one.  Returns v, q (, a_v, a_q) and the gradients, dV as [B,d,N] values."""
    lib = _lib.load()
    flags |= _lib.FLAG_BILINEAR
    B, d, N = V.shape
    L, T = len(Qs), Qs[0].shape[1]
    if layout == "lm":
        Vbuf, vstr = V.permute(0, 2, 1).contiguous().to(DEV), (N * d, d, 1)
    else:
        Vbuf, vstr = V.contiguous().to(DEV), (d * N, 1, N)
    Qd = [q.to(DEV).contiguous() for q in Qs]
    ps = [P[k].to(DEV).contiguous() for k in PNAMES]
    p = _lib.Params(*[t.data_ptr() for t in ps[:8]], None if null_wb else ps[8].data_ptr(), ps[9].data_ptr())
    sb, fb, bb = _lib.workspace_bytes(B, N, T, d, L, flags)
    saved = torch.zeros(sb // 4, device=DEV)
    ws = torch.full((max(fb, bb) // 4,), float("nan"), device=DEV)
    v = torch.full((L, B, d), float("nan"), device=DEV)
    q = torch.full((L, B, d), float("nan"), device=DEV)
    av = torch.full((L, B, N), float("nan"), device=DEV)
    aq = torch.full((L, B, T), float("nan"), device=DEV)
    qlen = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens is not None else None
    qptr = (C.c_void_p * L)(*[t.data_ptr() for t in Qd])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dims = (B, N, T, d, L, _lib.F32, flags, st)
    with_len = () if lens is None else (_ptr(qlen),)
    sfx = "" if lens is None else "_len"
    if infer:
        rc = getattr(lib, "coattn_infer" + sfx)(_ptr(Vbuf), *vstr, qptr, *with_len, C.byref(p), _ptr(v), _ptr(q), _ptr(av),
                                                _ptr(aq), _ptr(ws), *dims)
    elif maps:
        rc = getattr(lib, "coattn_forward_maps" + sfx)(_ptr(Vbuf), *vstr, qptr, *with_len, C.byref(p), _ptr(v), _ptr(q),
                                                       _ptr(av), _ptr(aq), _ptr(saved), _ptr(ws), *dims)
    else:
        rc = getattr(lib, "coattn_forward" + sfx)(_ptr(Vbuf), *vstr, qptr, *with_len, C.byref(p), _ptr(v), _ptr(q),
                                                  _ptr(saved), _ptr(ws), *dims)
    if expect_rc and rc != 0:
        return {"rc": rc}
    assert rc == 0, lib.coattn_last_error().decode()
    out = {"v": v, "q": q, "a_v": av, "a_q": aq, "saved": saved, "ws": ws, "rc": rc}
    if gv is None:
        return out
    dV = torch.full_like(Vbuf, float("nan"))
    dQ = [torch.full_like(t, float("nan")) for t in Qd]
    grads = [torch.full_like(t, float("nan")) for t in ps] if grads_init is None else [g.clone().to(DEV) for g in grads_init]
    pg = _lib.ParamGrads(*[g.data_ptr() for g in grads[:8]], None if null_dwb else grads[8].data_ptr(), grads[9].data_ptr())
    dqptr = (C.c_void_p * L)(*[t.data_ptr() for t in dQ])
    gvd, gqd = gv.to(DEV).contiguous(), gq.to(DEV).contiguous()
    tail = (_ptr(dV), *vstr, dqptr, C.byref(pg), accumulate, _ptr(ws), *dims)
    if maps:
        gav = g_av.to(DEV).contiguous() if g_av is not None else None
        gaq = g_aq.to(DEV).contiguous() if g_aq is not None else None
        rc = getattr(lib, "coattn_backward_maps" + sfx)(_ptr(Vbuf), *vstr, qptr, *with_len, C.byref(p), _ptr(saved), _ptr(gvd),
                                                        _ptr(gqd), _ptr(gav), _ptr(gaq), *tail)
    else:
        rc = getattr(lib, "coattn_backward" + sfx)(_ptr(Vbuf), *vstr, qptr, *with_len, C.byref(p), _ptr(saved), _ptr(gvd),
                                                   _ptr(gqd), *tail)
    if expect_rc:
        return {"rc": rc}
    assert rc == 0, lib.coattn_last_error().decode()
    torch.cuda.synchronize()
    out["dV_phys"] = dV.permute(0, 2, 1) if layout == "lm" else dV
    out["dQ"] = torch.stack(dQ)
    for k, g in zip(PNAMES, grads):
        out["d" + k] = g
    return out


def rel(a, b, floor=1e-30):
    a, b = a.double().cpu(), b.double().cpu().reshape(a.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(floor))


# The gradients of the score biases c_v, c_q are zero in exact arithmetic (a softmax does not see a shift): they are compared
# as absolute errors
ABS = ("dw_v.bias", "dw_q.bias")


def check(r, ref, tol, keys):
    for k in keys:
        e = rel(r[k], ref[k], 1.0 if k in ABS else 1e-30)
        assert e < tol, (k, e)


def oracle(V, Qs, P, gv, gq, lens=None, g_av=None, g_aq=None):
    return BL.forward_backward(V, Qs, P, gv, gq, bilinear=True, lens=lens, g_av=g_av, g_aq=g_aq, device=DEV)


SMALL = {"n49_d256": (4, 49, 8, 256), "n64_d512": (3, 64, 7, 512), "n100_d256": (3, 100, 9, 256), "d96": (2, 20, 6, 96)}


@pytest.mark.parametrize("mode,flag", MODES, ids=[m for m, _ in MODES])
@pytest.mark.parametrize("layout", ("lm", "cm"))
@pytest.mark.parametrize("shape", list(SMALL))
@pytest.mark.parametrize("impl", ("auto", "general"))
def test_small_shapes_vs_oracle(shape, layout, mode, flag, impl):
    B, N, T, d = SMALL[shape]
    lens = [T - b % 3 for b in range(B)]             # pad rows present: K = b_b there
    V, Qs, P, gv, gq = case(B, N, T, d, lens)
    r = run(V, Qs, P, gv, gq, flags=flag | (_lib.IMPL_GENERAL if impl == "general" else 0), layout=layout, maps=True)
    ref = oracle(V, Qs, P, gv, gq)
    tol = 1e-5 if mode == "exact" else 5e-5
    check(r, ref, tol, ("v", "q", "a_v", "a_q") + GRADS)


@pytest.mark.parametrize("mode,flag", MODES, ids=[m for m, _ in MODES])
@pytest.mark.parametrize("N", (49, 196))
def test_cfg2_padded_questions_vs_oracle(N, mode, flag):
    B, T, d = 160, 26, 512
    lens = [3 + (7 * b) % 24 for b in range(B)]
    V, Qs, P, gv, gq = case(B, N, T, d, lens, seed=5)
    r = run(V, Qs, P, gv, gq, flags=flag, layout="lm")
    ref = oracle(V, Qs, P, gv, gq)
    # Exact mode: 2e-5 for everything but dQ at N = 196, held to 5e-5 -- measured 3.7e-5 of max|dQ|, the same on the fused and the
    # general path (where K's larger magnitude saturates C, dA = dC (1 - C^2) is formed from the fp32 tanh)
    for k in ("v", "q") + GRADS:
        floor = 1.0 if k in ABS else 1e-30
        tol = (5e-5 if (k == "dQ" and N == 196) else 2e-5) if mode == "exact" else 1e-4
        assert rel(r[k], ref[k], floor) < tol, (k, rel(r[k], ref[k], floor), tol)
    assert rel(r["dW_b.bias"], ref["dW_b.bias"]) < 2e-5       # db_b: the pad rows' K = b_b terms included


@pytest.mark.parametrize("mode,flag", MODES, ids=[m for m, _ in MODES])
@pytest.mark.parametrize("layout", ("lm", "cm"))
def test_masked_vs_truncated_oracle_and_pad_rows_do_not_matter(layout, mode, flag):
    B, N, T, d = 4, 49, 10, 256
    lens = [10, 6, 3, 1]
    V, Qs, P, gv, gq = case(B, N, T, d, lens)
    r = run(V, Qs, P, gv, gq, flags=flag, layout=layout, lens=lens, maps=True)
    ref = oracle(V, Qs, P, gv, gq, lens=lens)
    check(r, ref, 1e-5 if mode == "exact" else 5e-5, ("v", "q", "a_v", "a_q") + GRADS)
    junk = [q.clone() for q in Qs]
    for b, n in enumerate(lens):
        for l, q in enumerate(junk):
            q[b, n:] = torch.from_numpy(O.hash_normal(tuple(q[b, n:].shape), 99 + 7 * b + l)).float() * 3.0
    r2 = run(V, junk, P, gv, gq, flags=flag, layout=layout, lens=lens, maps=True)
    for k in ("v", "q", "a_v", "a_q", "dV_phys", "dW_v.weight", "dW_q.weight", "dW_b.weight", "dW_b.bias", "dW_q.bias"):
        assert torch.equal(r[k], r2[k]), k
    for b, n in enumerate(lens):
        assert torch.equal(r["dQ"][:, b, :n], r2["dQ"][:, b, :n]) and (r2["dQ"][:, b, n:] == 0).all()


@pytest.mark.parametrize("mode,flag", MODES, ids=[m for m, _ in MODES])
def test_map_gradients_vs_oracle(mode, flag):
    B, N, T, d = 3, 49, 8, 256
    V, Qs, P, gv, gq = case(B, N, T, d, [8, 5, 2])
    g_av = torch.from_numpy(O.hash_normal((3, B, N), 41)).float()
    g_aq = torch.from_numpy(O.hash_normal((3, B, T), 42)).float()
    r = run(V, Qs, P, gv, gq, flags=flag, maps=True, g_av=g_av, g_aq=g_aq)
    ref = oracle(V, Qs, P, gv, gq, g_av=g_av, g_aq=g_aq)
    check(r, ref, 1e-5 if mode == "exact" else 5e-5, GRADS)


@pytest.mark.parametrize("mode,flag", MODES, ids=[m for m, _ in MODES])
@pytest.mark.parametrize("masked", (False, True))
def test_infer_equals_the_saving_forward(masked, mode, flag):
    B, N, T, d = 8, 49, 26, 512
    lens = [26 - 3 * b for b in range(B)]
    V, Qs, P, _, _ = case(B, N, T, d, lens)
    a = run(V, Qs, P, flags=flag, maps=True, lens=lens if masked else None)
    b = run(V, Qs, P, flags=flag, infer=True, lens=lens if masked else None)
    for k in ("v", "q", "a_v", "a_q"):
        assert torch.equal(a[k], b[k]), k


def _identity(P):
    P = dict(P)
    d = P["W_q.weight"].shape[0]
    P["W_b.weight"] = torch.eye(d)
    P["W_b.bias"] = torch.zeros(d)
    return P


def _reference_call(V, Qs, P, gv, gq, flags):
    """The same C-ABI call without the flag (tests/_hip.py style), returning v, q, dV, dQ."""
    lib = _lib.load()
    B, d, N = V.shape
    L, T = len(Qs), Qs[0].shape[1]
    Vbuf = V.permute(0, 2, 1).contiguous().to(DEV)
    Qd = [q.to(DEV).contiguous() for q in Qs]
    ps = [P[k].to(DEV).contiguous() for k in PNAMES[:8]]
    p = _lib.Params(*[t.data_ptr() for t in ps])
    sb, fb, bb = _lib.workspace_bytes(B, N, T, d, L, flags)
    saved, ws = torch.zeros(sb // 4, device=DEV), torch.zeros(max(fb, bb) // 4, device=DEV)
    v, q = torch.empty((L, B, d), device=DEV), torch.empty((L, B, d), device=DEV)
    qptr = (C.c_void_p * L)(*[t.data_ptr() for t in Qd])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dims = (B, N, T, d, L, _lib.F32, flags, st)
    assert lib.coattn_forward(_ptr(Vbuf), N * d, d, 1, qptr, C.byref(p), _ptr(v), _ptr(q), _ptr(saved), _ptr(ws), *dims) == 0
    dV = torch.empty_like(Vbuf)
    dQ = [torch.empty_like(t) for t in Qd]
    grads = [torch.empty_like(t) for t in ps]
    pg = _lib.ParamGrads(*[g.data_ptr() for g in grads])
    dqptr = (C.c_void_p * L)(*[t.data_ptr() for t in dQ])
    assert lib.coattn_backward(_ptr(Vbuf), N * d, d, 1, qptr, C.byref(p), _ptr(saved), _ptr(gv.to(DEV).contiguous()),
                               _ptr(gq.to(DEV).contiguous()), _ptr(dV), N * d, d, 1, dqptr, C.byref(pg), 0, _ptr(ws),
                               *dims) == 0
    torch.cuda.synchronize()
    return {"v": v, "q": q, "dV_phys": dV.permute(0, 2, 1), "dQ": torch.stack(dQ)}


@pytest.mark.parametrize("mode,flag", MODES, ids=[m for m, _ in MODES])
@pytest.mark.parametrize("impl", ("auto", "general"))
def test_identity_W_b_is_the_reference_affinity(impl, mode, flag):
    """W_b = I, b_b = 0: the reference's call.  Exact mode: K = Q bit for bit, so the forward is the reference's bit for bit on
    either path; the backward's dQ projection adds dP_q W_q and dK I in one contraction, so dQ / dV agree to fp32 rounding."""
    B, N, T, d = 4, 49, 8, 512
    V, Qs, P, gv, gq = case(B, N, T, d, [8, 6, 4, 2])
    P = _identity(P)
    ext = _lib.IMPL_GENERAL if impl == "general" else 0
    r = run(V, Qs, P, gv, gq, flags=flag | ext)
    ref = _reference_call(V, Qs, P, gv, gq, flag | ext)
    for k in ("v", "q"):
        if mode == "exact":
            assert torch.equal(r[k], ref[k]), k
        else:                                        # (tolerance mode: K = Q I on two FP16 pieces, not Q itself)
            assert rel(r[k], ref[k]) < 1e-6, k
    for k in ("dV_phys", "dQ"):
        assert rel(r[k], ref[k]) < 1e-6, k


def test_accumulate_adds_and_runs_are_bitwise_repeatable():
    B, N, T, d = 4, 49, 8, 256
    V, Qs, P, gv, gq = case(B, N, T, d, [8, 5, 3, 1])
    a = run(V, Qs, P, gv, gq)
    b = run(V, Qs, P, gv, gq)
    for k in ("v", "q") + GRADS:
        assert torch.equal(a[k], b[k]), k
    init = [torch.from_numpy(O.hash_normal(tuple(P[k].shape), 60 + i)).float() for i, k in enumerate(PNAMES)]
    c = run(V, Qs, P, gv, gq, accumulate=1, grads_init=init)
    for i, k in enumerate(PNAMES):
        assert rel(c["d" + k] - init[i].to(DEV), a["d" + k], 1.0 if "d" + k in ABS else 1e-30) < 1e-5, k


def test_fast16_range_report_covers_K_and_W_b():
    """Tolerance mode, fused shape: K is phase 1's FP16-piece operand, so a W_b that makes |K| exceed 65,504 makes coattn_status
    return -4 (and coattn_status_accumulate record it); a W_b beyond 255.87 does too (the |256 W| rule of W_q).  The exact mode
    gives the oracle's value there.  An ordinary W_b reports 0."""
    B, N, T, d = 8, 49, 26, 512
    V, Qs, P, gv, gq = case(B, N, T, d)
    lib = _lib.load()
    amax = (C.c_float * 2)()
    r = run(V, Qs, P, flags=_lib.FLAG_FAST16)
    assert lib.coattn_status(_ptr(r["saved"]), B, N, T, d, 3, _lib.F32, C.c_void_p(0), amax) == 0
    big = dict(P)
    big["W_b.bias"] = P["W_b.bias"] * 3e6             # the weights stay ordinary, |K| > 65,504
    r = run(V, Qs, big, flags=_lib.FLAG_FAST16)
    assert lib.coattn_status(_ptr(r["saved"]), B, N, T, d, 3, _lib.F32, C.c_void_p(0), amax) == -4
    assert amax[0] > 65504 and amax[1] <= 65504
    acc = torch.zeros(2, device=DEV)
    assert lib.coattn_status_accumulate(_ptr(r["saved"]), B, N, T, d, 3, _lib.F32, _ptr(acc), C.c_void_p(0)) == 0
    assert float(acc.max()) > 65504
    ex = run(V, Qs, big, gv, gq, flags=0)
    check(ex, oracle(V, Qs, big, gv, gq), 1e-5, ("v", "q"))
    wide = dict(P)
    wide["W_b.weight"] = P["W_b.weight"] * 1e4        # |W_b| > 255.87
    r = run(V, Qs, wide, flags=_lib.FLAG_FAST16)
    assert lib.coattn_status(_ptr(r["saved"]), B, N, T, d, 3, _lib.F32, C.c_void_p(0), amax) == -4
    assert amax[1] > 65504


@pytest.mark.parametrize("impl", ("fused", "general"))
def test_forced_paths_agree(impl):
    """IMPL_FUSED / IMPL_GENERAL are honoured under the flag, both against the oracle."""
    B, N, T, d = 4, 49, 8, 512
    V, Qs, P, gv, gq = case(B, N, T, d, [8, 6, 4, 2])
    r = run(V, Qs, P, gv, gq, flags=_lib.IMPL_FUSED if impl == "fused" else _lib.IMPL_GENERAL)
    check(r, oracle(V, Qs, P, gv, gq), 1e-5, ("v", "q") + GRADS)


def test_refusals():
    B, N, T, d = 2, 49, 6, 256
    V, Qs, P, gv, gq = case(B, N, T, d)
    lib = _lib.load()
    assert run(V, Qs, P, flags=_lib.FLAG_BF16_PROJ, expect_rc=1)["rc"] < 0
    assert "BF16_PROJ" in lib.coattn_last_error().decode()
    assert run(V, Qs, P, null_wb=True, expect_rc=1)["rc"] < 0
    assert "W_b" in lib.coattn_last_error().decode()
    assert run(V, Qs, P, gv, gq, null_dwb=True, expect_rc=1)["rc"] < 0
    assert "dW_b" in lib.coattn_last_error().decode()
    m = vqa_amd.ParallelCoAttention(d, affinity="bilinear").to(DEV)
    m.bf16_projections = True
    with pytest.raises(RuntimeError, match="reduced-precision"):
        m(V.to(DEV).permute(0, 2, 1), [q.to(DEV) for q in Qs])


def _module_case(d=256, B=4, N=49, T=8):
    V, Qs, P, gv, gq = case(B, N, T, d, [8, 6, 4, 2])
    m = vqa_amd.ParallelCoAttention(d, affinity="bilinear")
    m.load_state_dict(P)
    return V, Qs, P, gv, gq, m.to(DEV)


@pytest.mark.parametrize("fast", (False, True))
def test_module_autograd_vs_oracle(fast):
    V, Qs, P, gv, gq, m = _module_case()
    m.fast_products = fast
    x = V.to(DEV).permute(0, 2, 1).contiguous().requires_grad_(True)
    Qg = [q.to(DEV).requires_grad_(True) for q in Qs]
    vs, qs = m(x, Qg)
    (sum((vs[l] * gv[l].to(DEV)).sum() + (qs[l] * gq[l].to(DEV)).sum() for l in range(3))).backward()
    ref = oracle(V, Qs, P, gv, gq)
    tol = 5e-5 if fast else 1e-5
    assert rel(torch.stack(vs), ref["v"]) < tol and rel(torch.stack(qs), ref["q"]) < tol
    assert rel(x.grad.permute(0, 2, 1), ref["dV_phys"]) < tol
    assert rel(torch.stack([q.grad for q in Qg]), ref["dQ"]) < tol
    for k in PNAMES:
        mod, attr = k.split(".")
        assert rel(getattr(getattr(m, mod), attr).grad, ref["d" + k], 1.0 if "d" + k in ABS else 1e-30) < tol, k
    # with the default form W_b takes no part
    m2 = vqa_amd.ParallelCoAttention(256).to(DEV)
    vs, qs = m2(x.detach(), [q.detach() for q in Qg])
    (torch.stack(vs).sum() + torch.stack(qs).sum()).backward()
    assert m2.W_b.weight.grad is None and m2.W_b.bias.grad is None


def _batch(B=8, T=26, vocab=100, K=10, seed=1):
    from vqa_amd import train as T_
    b = T_.synthetic_batch(B, (64, 64), T, vocab, K + 1, seed=seed)
    return T_.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])


def test_hot_path_modes_are_bit_identical_and_train_W_b():
    from vqa_amd import train as T
    im, qu, la, ln = _batch()
    torch.manual_seed(0)
    model = T.build_model("attention", 100, 10, affinity="bilinear").to(DEV)
    with torch.no_grad():
        feats = model.image_encoder(im.to(DEV)).detach()
    res = {}
    for mode in ("modules", "static", "graph"):
        model.hot_path_static = mode == "static"
        model.hot_path_graph = mode == "graph"
        model.hot_path_direct_grads = mode != "modules"
        for p in model.parameters():
            p.grad = None
        logits, loss = model.forward_features(feats, qu.to(DEV), ln, labels=la.to(DEV))
        loss.backward()
        res[mode] = (loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    assert "co_attention.W_b.weight" in res["modules"][1] and "co_attention.W_b.bias" in res["modules"][1]
    assert all(k[-1] == "bilinear" for k in model._graphs)       # the affinity is part of the node's key
    for mode in ("static", "graph"):
        assert torch.equal(res[mode][0], res["modules"][0]), mode
        assert res[mode][1].keys() == res["modules"][1].keys()
        for n in res["modules"][1]:
            if n.startswith("question_encoder"):
                assert rel(res[mode][1][n], res["modules"][1][n]) < 1e-4, (mode, n)
            else:
                assert torch.equal(res[mode][1][n], res["modules"][1][n]), (mode, n)
    # a few Trainer steps move W_b; with the default affinity W_b keeps no gradient and does not move
    for aff in ("bilinear", "reference"):
        torch.manual_seed(0)
        m = T.build_model("attention", 100, 10, affinity=aff).to(DEV)
        w0 = m.co_attention.W_b.weight.detach().clone()
        tr = T.Trainer(m, 1e-3, DEV)
        for s in range(3):
            im, qu, la, ln = _batch(seed=10 + s)
            loss = float(tr.step(im.to(DEV), qu.to(DEV), ln, la.to(DEV)))
            assert loss == loss
        moved = not torch.equal(m.co_attention.W_b.weight.detach(), w0)
        assert moved == (aff == "bilinear"), aff
        if aff == "reference":
            assert m.co_attention.W_b.weight.grad is None


def test_train_and_predict_cli(tmp_path, capsys):
    from vqa_amd import predict as Pr
    from vqa_amd import train as T
    ck = str(tmp_path / "bil.pth")
    T.main(["--model", "attention", "--affinity", "bilinear", "--num_steps", "3", "--batch_size", "4", "--log_interval", "1",
            "--num_cls", "10", "--vocab_size", "100", "--image_size", "64", "--save_path", ck])
    preds, maps = str(tmp_path / "p.jsonl"), str(tmp_path / "m.npz")
    Pr.main(["--model", "attention", "--affinity", "bilinear", "--model_ckpt", ck, "--num_cls", "10", "--vocab_size", "100",
             "--image_size", "64", "--test_size", "6", "--batch_size", "3", "--predictions", preds, "--attention_maps", maps])
    assert len(open(preds).read().strip().splitlines()) == 6
    import numpy as np
    z = np.load(maps)
    assert np.isfinite(z["a_q"]).all() and np.isfinite(z["a_v"]).all()

"""Every route of the backward's host driver (csrc/coattn_fused_bwd.hip fused_backward, csrc/api.hip backward_general), one
row each, over the raw C-ABI: one forward + backward between coattn_profile_begin / _end, the sequence of launch-group marks
against a literal list (recorded with the library of the commit before the driver was split into decide-then-run steps: the
split must reproduce them), and
every output and gradient against the float64 oracle of tests/_bilinear.py at the suite's bounds -- 2e-5 of max|.| in the
exact mode, 1e-4 in the tolerance mode (COATTN_FLAG_FAST16), and in the reduced-precision mode (COATTN_FLAG_BF16_PROJ) the
8e-2 that test_gpu_edges.py::test_bf16_mfma_projections states for it.  The score biases' gradients dc_v / dc_q are zero in
exact arithmetic and are compared as absolute errors.

The single-product weight-gradient route (gemm_bf.hip's 256 x 256 tiles, bf16-stored dP) wants contraction lengths B N and
B T that are multiples of 32 and a dQ projection of 256 rows or more: it is not in this table, whose T is 26, but it is
reached at B = 16, T = 16, N = 32 / 96, d = 512 by tests/test_gpu_fused_backward.py (rows dpb_* and bf_tn_*), beside
test_gpu_edges.py::test_bf16_mode_stores_its_gemm_only_gradients_as_bf16 (d = 2048, B = 160).
"""
import ctypes as C

import pytest
import torch

from vqa_amd import _lib
from oracle import coattn_oracle as O

from tests import _bilinear as BL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES = BL.NAMES
T = 26

PRE = ["bwd_pre", "bwd_dc32", "bwd_nat32"]
# the forward: weight split, both projections in one launch, the fused kernel (which also attends V on small location-major grids)
FWD = ["wsplit", "projections", "coattn_fwd32"]
# the weight gradients, the dQ projection's tiles and the small reductions in ONE launch, their partial sums in the dQ kernel's
COMBINED = PRE + ["bwd_gemm", "bwd_dq"]
# the dQ projection as a launch of its own in front of the dQ kernel
OWN_PROJ = PRE + ["bwd_gemm_dq_projection", "bwd_dq"]
# bilinear: the dQ kernel writes dK = dA V ("bwd_dq"), then the [dP_q | dK] projection, dW_b / db_b, the two weight gradients
BILINEAR = PRE + ["bwd_dq", "bwd_bilinear_dq", "bwd_bilinear_dwb", "bwd_gemm_dw", "reduce_partials"]

# id: (B, N, d, L, layout, flags, options, marks)
#   layout: "lm" [B,N,d] / "cm" [B,d,N] / "lm_gap" (sB = N d + 64) / "pitch" (location-major rows d + 8 floats apart: no
#   fused layout, the general path's strides)
#   options: dv (dV requested), q_off (Q_l 4 bytes off a 16-byte boundary), acc (accumulate = 1 onto given gradients),
#   len (the *_len entry points with the lengths), maps ("both" / "av": coattn_forward_maps / _backward_maps with G_av and
#   G_aq / with G_aq NULL)
FAST, BF16, BIL, GENERAL = _lib.FLAG_FAST16, _lib.FLAG_BF16_PROJ, _lib.FLAG_BILINEAR, _lib.IMPL_GENERAL
ROWS = {
    "lm49_B8": (8, 49, 512, 3, "lm", 0, {}, FWD + COMBINED),
    "lm49_B8_dV": (8, 49, 512, 3, "lm", 0, {"dv": 1}, FWD + COMBINED),
    "lm196_B5": (5, 196, 512, 3, "lm", 0, {"dv": 1}, FWD + ["attend_v"] + COMBINED),
    "cm196_B5": (5, 196, 512, 3, "cm", 0, {"dv": 1}, FWD + ["attend_v"] + COMBINED),
    "cm49_B8": (8, 49, 512, 3, "cm", 0, {"dv": 1}, ["wsplit", "coattn_fwd32", "attend_v"] + PRE + ["bwd_dq"]),
    "lm49_B2": (2, 49, 512, 3, "lm", 0, {"dv": 1}, ["coattn_fwd32"] + OWN_PROJ + ["bwd_gemm_dw", "reduce_partials"]),
    "lm49_gap": (8, 49, 512, 3, "lm_gap", 0, {"dv": 1}, ["wsplit", "coattn_fwd32"] + OWN_PROJ),
    "lm49_q_off4": (8, 49, 512, 3, "lm", 0, {"dv": 1, "q_off": 1}, ["wsplit", "coattn_fwd32"] + OWN_PROJ),
    "lm49_L1": (8, 49, 512, 1, "lm", 0, {"dv": 1}, FWD + COMBINED),
    "lm49_L2": (8, 49, 512, 2, "lm", 0, {"dv": 1}, FWD + COMBINED),
    "lm49_accumulate": (8, 49, 512, 3, "lm", 0, {"dv": 1, "acc": 1}, FWD + COMBINED),
    "lm49_fast16": (8, 49, 512, 3, "lm", FAST, {}, FWD + COMBINED),
    "lm49_bf16_proj": (8, 49, 512, 3, "lm", BF16, {}, FWD + COMBINED),
    "lm49_len": (8, 49, 512, 3, "lm", 0, {"dv": 1, "len": 1}, FWD + COMBINED),
    "lm49_maps_both": (8, 49, 512, 3, "lm", 0, {"dv": 1, "maps": "both"}, FWD + COMBINED),
    "lm49_maps_av_only": (8, 49, 512, 3, "lm", 0, {"dv": 1, "maps": "av"}, FWD + COMBINED),
    "lm49_bilinear_B8": (8, 49, 512, 3, "lm", BIL, {"dv": 1}, FWD[:2] + ["bilinear_projection", "coattn_fwd32"] + BILINEAR),
    "lm49_bilinear_B2": (2, 49, 512, 3, "lm", BIL, {"dv": 1}, ["coattn_fwd32"] + BILINEAR),
    "general_pitch": (3, 49, 256, 3, "pitch", GENERAL, {"dv": 1}, ["wsplit"]),
    "general_pitch_bilinear": (3, 49, 256, 3, "pitch", GENERAL | BIL, {"dv": 1}, ["wsplit"]),
}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _lens(B):
    return [T] + [3 + (7 * b) % 23 for b in range(1, B)]         # ragged: zero pad rows behind every question but the first


def _features(V, layout):
    """The buffer handed to the C-ABI, its (sB, sN, sD) and the [B,d,N] view of it."""
    B, d, N = V.shape
    if layout == "cm":
        buf = V.contiguous().to(DEV)
        return buf, (d * N, 1, N), buf
    pitch = d + 8 if layout == "pitch" else d
    sB = N * pitch + (64 if layout == "lm_gap" else 0)
    buf = torch.full((B, sB), float("nan"), device=DEV)
    view = buf[:, :N * pitch].view(B, N, pitch)[:, :, :d]
    view.copy_(V.permute(0, 2, 1))
    return buf, (sB, pitch, 1), view.permute(0, 2, 1)


_cases = {}


def case(name):
    """Inputs and the float64 oracle of a row, computed once."""
    if name in _cases:
        return _cases[name]
    B, N, d, L, layout, flags, opt, _ = ROWS[name]
    bil = bool(flags & _lib.FLAG_BILINEAR)
    lens = _lens(B)
    P = O.make_params(d, 3)
    V, Qs = O.make_inputs(B, N, T, d, 13, lens=lens, scale_q=(2.0 / d) ** 0.5, L=L)
    gv = torch.from_numpy(O.hash_normal((L, B, d), 23)).float()
    gq = torch.from_numpy(O.hash_normal((L, B, d), 24)).float()
    maps = opt.get("maps")
    g_av = torch.from_numpy(O.hash_normal((L, B, N), 41)).float() if maps else None
    g_aq = torch.from_numpy(O.hash_normal((L, B, T), 42)).float() if maps == "both" else None
    ref = BL.forward_backward(V, Qs, P, gv, gq, bilinear=bil, lens=lens if opt.get("len") else None, g_av=g_av, g_aq=g_aq,
                              device=DEV)
    # accumulate = 1: gradients to add onto, of each gradient's own magnitude (the sum then rounds at that magnitude, which
    # the bound is relative to)
    init = None
    if opt.get("acc"):
        init = [torch.from_numpy(O.hash_normal(tuple(P[k].shape), 60 + i)).float() *
                (1.0 if ref["d" + k] is None else float(ref["d" + k].abs().max())) for i, k in enumerate(NAMES)]
    _cases[name] = (V, Qs, P, gv, gq, g_av, g_aq, lens, init, ref)
    return _cases[name]


def run_row(name, lib=None):
    """One profiled forward + backward of a row.  Returns (marks, outputs): v, q, (a_v, a_q,) dV_phys as [B,d,N] values (or
    None), dQ and d<parameter>."""
    lib = lib or _lib.load()
    B, N, d, L, layout, flags, opt, _ = ROWS[name]
    V, Qs, P, gv, gq, g_av, g_aq, lens, init, _ = case(name)
    bil = bool(flags & _lib.FLAG_BILINEAR)
    Vbuf, vstr, _ = _features(V, layout)
    if opt.get("q_off"):
        base = [torch.zeros(B * T * d + 1, device=DEV) for _ in Qs]
        Qd = [b[1:].view(B, T, d) for b in base]
        for t, q in zip(Qd, Qs):
            t.copy_(q)
        assert all(t.data_ptr() % 16 == 4 for t in Qd)
    else:
        Qd = [q.to(DEV).contiguous() for q in Qs]
    ps = [P[k].to(DEV).contiguous() for k in NAMES]
    p = _lib.Params(*[t.data_ptr() for t in ps[:8]], *([t.data_ptr() for t in ps[8:]] if bil else []))
    sb, fb, bb = _lib.workspace_bytes(B, N, T, d, L, flags)
    saved = torch.zeros(sb // 4, device=DEV)
    ws = torch.full((max(fb, bb) // 4,), float("nan"), device=DEV)
    v = torch.full((L, B, d), float("nan"), device=DEV)
    q = torch.full((L, B, d), float("nan"), device=DEV)
    maps = opt.get("maps")
    av = torch.full((L, B, N), float("nan"), device=DEV) if maps else None
    aq = torch.full((L, B, T), float("nan"), device=DEV) if maps else None
    qlen = torch.tensor(lens, dtype=torch.int32, device=DEV) if opt.get("len") else None
    with_len, sfx = ((_ptr(qlen),), "_len") if opt.get("len") else ((), "")
    qptr = (C.c_void_p * L)(*[t.data_ptr() for t in Qd])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dims = (B, N, T, d, L, _lib.F32, flags, st)
    dVbuf, _, dVview = _features(torch.full_like(V, float("nan")), layout) if opt.get("dv") else (None, None, None)
    dQ = [torch.full_like(t, float("nan")) for t in Qd]
    grads = [torch.full_like(t, float("nan")) for t in ps] if init is None else [g.clone().to(DEV) for g in init]
    pg = _lib.ParamGrads(*[g.data_ptr() for g in grads[:8]], *([g.data_ptr() for g in grads[8:]] if bil else []))
    dqptr = (C.c_void_p * L)(*[t.data_ptr() for t in dQ])
    gvd, gqd = gv.to(DEV), gq.to(DEV)
    gavd = g_av.to(DEV) if g_av is not None else None
    gaqd = g_aq.to(DEV) if g_aq is not None else None
    tail = (_ptr(dVbuf), *(vstr if dVbuf is not None else (0, 0, 0)), dqptr, C.byref(pg), 1 if init is not None else 0,
            _ptr(ws), *dims)
    torch.cuda.synchronize()
    _lib.check(lib.coattn_profile_begin(st), "coattn_profile_begin")
    if maps:
        rc = getattr(lib, "coattn_forward_maps" + sfx)(_ptr(Vbuf), *vstr, qptr, *with_len, C.byref(p), _ptr(v), _ptr(q),
                                                       _ptr(av), _ptr(aq), _ptr(saved), _ptr(ws), *dims)
        _lib.check(rc, "coattn_forward_maps")
        rc = getattr(lib, "coattn_backward_maps" + sfx)(_ptr(Vbuf), *vstr, qptr, *with_len, C.byref(p), _ptr(saved), _ptr(gvd),
                                                        _ptr(gqd), _ptr(gavd), _ptr(gaqd), *tail)
        _lib.check(rc, "coattn_backward_maps")
    else:
        rc = getattr(lib, "coattn_forward" + sfx)(_ptr(Vbuf), *vstr, qptr, *with_len, C.byref(p), _ptr(v), _ptr(q),
                                                  _ptr(saved), _ptr(ws), *dims)
        _lib.check(rc, "coattn_forward")
        rc = getattr(lib, "coattn_backward" + sfx)(_ptr(Vbuf), *vstr, qptr, *with_len, C.byref(p), _ptr(saved), _ptr(gvd),
                                                   _ptr(gqd), *tail)
        _lib.check(rc, "coattn_backward")
    us = (C.c_float * 48)()
    names = C.create_string_buffer(2048)
    n = lib.coattn_profile_end(us, names, 2048, 48)
    assert n >= 0, lib.coattn_last_error().decode()
    torch.cuda.synchronize()
    marks = names.value.decode().split("\n") if n else []
    assert len(marks) == n
    out = {"v": v, "q": q, "dV_phys": dVview, "dQ": torch.stack(dQ)}
    if maps:
        out["a_v"], out["a_q"] = av, aq
    for k, g in zip(NAMES if bil else NAMES[:8], grads):
        out["d" + k] = g
    return marks, out


ABS = ("dw_v.bias", "dw_q.bias")       # dc_v, dc_q


def errors(name, out):
    """{key: error of the row's output against the oracle, as a fraction of max|oracle| (dc_v, dc_q: absolute)}."""
    init, ref = case(name)[-2:]
    errs = {}
    for k, got in out.items():
        if got is None:
            continue
        want = ref[k].double().to(DEV).reshape(got.shape)
        scale = 1.0 if k in ABS else float(want.abs().max())
        if init is not None and k[1:] in NAMES:
            want = want + init[NAMES.index(k[1:])].double().to(DEV)
        errs[k] = float((got.double() - want).abs().max()) / scale
    return errs


def bound(flags):
    return 8e-2 if flags & _lib.FLAG_BF16_PROJ else (1e-4 if flags & _lib.FLAG_FAST16 else 2e-5)


@pytest.mark.parametrize("name", list(ROWS))
def test_route(name):
    marks, out = run_row(name)
    errs = errors(name, out)
    print(name, marks, {k: "%.2e" % e for k, e in errs.items()})
    assert marks == ROWS[name][7]
    tol = bound(ROWS[name][5])
    for k, e in errs.items():
        assert e < tol, (k, e, tol)           # (a NaN fails)

"""float64 oracle of the alternating co-attention (include/coattn.h v0.11.0; Lu et al. 2016 section 3.3): torch autograd of
the definition, per sample on Q[b, :len_b] when masked (the maps padded with 0), as tests/_bilinear.py does for the bilinear
form; the C-ABI runner of the family (case, run, check: feature and gradient layouts, guard words behind every buffer the
calls write); and paths(), the dispatch rules of csrc/coattn_alt.hip (alt_linear, alt_wgrad) restated in plain Python."""
import ctypes as C

import torch

NAMES = ("W_x1", "b_x1", "w_h1", "c_h1", "W_x2", "b_x2", "W_g2", "b_g2", "w_h2", "c_h2",
         "W_x3", "b_x3", "W_g3", "b_g3", "w_h3", "c_h3")
def state_key(name: str) -> str:
    """C-ABI parameter name -> AlternatingCoAttention state_dict key: W_x1 -> W_x1.weight, b_x1 -> W_x1.bias,
    w_h1 -> w_h1.weight, c_h1 -> w_h1.bias."""
    if name.startswith("b_"):
        return "W_" + name[2:] + ".bias"
    if name.startswith("c_"):
        return "w_" + name[2:] + ".bias"
    return name + ".weight"


def make_params(d: int, seed: int = 0, scale: float = 1.0):
    g = torch.Generator().manual_seed(seed)
    P = {}
    for n in NAMES:
        if n[0] == "W":
            P[n] = torch.randn(d, d, generator=g, dtype=torch.float64) * (scale / d ** 0.5)
        elif n[0] == "w":
            P[n] = torch.randn(1, d, generator=g, dtype=torch.float64) * (scale / d ** 0.5)
        elif n[0] == "c":
            P[n] = torch.randn(1, generator=g, dtype=torch.float64) * 0.1
        else:
            P[n] = torch.randn(d, generator=g, dtype=torch.float64) * 0.1
    return P


def _guided(X, g, W, b, w, c):
    H = torch.tanh(X @ W.T + b + g)
    a = torch.softmax((H @ w.T).squeeze(-1) + c, dim=0)
    return a @ X, a


def forward(V, Qs, P, lens=None):
    """V [B,N,d], Qs: L x [B,T,d] (float64) -> v [L,B,d], q [L,B,d], a_v [L,B,N], a_q [L,B,T] (differentiable)."""
    B, N, d = V.shape
    T = Qs[0].shape[1]
    vs, qs, avs, aqs = [], [], [], []
    for Q in Qs:
        vl, ql, avl, aql = [], [], [], []
        for b in range(B):
            n = T if lens is None else max(1, min(int(lens[b]), T))
            Qb = Q[b, :n]
            s, _ = _guided(Qb, 0.0, P["W_x1"], P["b_x1"], P["w_h1"], P["c_h1"])
            v, av = _guided(V[b], s @ P["W_g2"].T + P["b_g2"], P["W_x2"], P["b_x2"], P["w_h2"], P["c_h2"])
            q, aq = _guided(Qb, v @ P["W_g3"].T + P["b_g3"], P["W_x3"], P["b_x3"], P["w_h3"], P["c_h3"])
            vl.append(v); ql.append(q); avl.append(av)
            aql.append(torch.cat([aq, aq.new_zeros(T - n)]))
        vs.append(torch.stack(vl)); qs.append(torch.stack(ql)); avs.append(torch.stack(avl)); aqs.append(torch.stack(aql))
    return torch.stack(vs), torch.stack(qs), torch.stack(avs), torch.stack(aqs)


def forward_backward(V, Qs, P, gv, gq, g_av=None, g_aq=None, lens=None, dtype=torch.float64):
    """Outputs and gradients (float64): dict with v, q, a_v, a_q, dV, dQ (list), and d<name> for every parameter.
    dtype=torch.float32 evaluates the same definition in float32: its distance from the float64 result is the error a
    float32 evaluation has at that case."""
    gv, gq = gv.to(dtype), gq.to(dtype)
    g_av = g_av.to(dtype) if g_av is not None else None
    g_aq = g_aq.to(dtype) if g_aq is not None else None
    V = V.to(dtype).detach().requires_grad_(True)
    Qs = [q.to(dtype).detach().requires_grad_(True) for q in Qs]
    Pg = {k: v.to(dtype).detach().requires_grad_(True) for k, v in P.items()}
    v, q, av, aq = forward(V, Qs, Pg, lens)
    loss = (v * gv).sum() + (q * gq).sum()
    if g_av is not None:
        loss = loss + (av * g_av).sum()
    if g_aq is not None:
        if lens is not None:
            T = aq.shape[-1]
            m = (torch.arange(T)[None, :] < torch.as_tensor(lens).clamp(1, T)[:, None]).to(dtype)
            loss = loss + (aq * g_aq * m).sum()
        else:
            loss = loss + (aq * g_aq).sum()
    loss.backward()
    out = {"v": v.detach(), "q": q.detach(), "a_v": av.detach(), "a_q": aq.detach(), "dV": V.grad, "dQ": [x.grad for x in Qs]}
    for k, t in Pg.items():
        out["d" + k] = t.grad
    return out


# ---- the C-ABI runner -----------------------------------------------------------------------------------------------------

TOL = 2e-5
GUARD_FLOATS = 256
GUARD_BITS = 0x5A5AA5A5            # the bit pattern of the guard words (a finite float)
LAYOUTS = ("lm", "cm", "pad", "cmpad", "col2")


def _dev():
    return torch.device("cuda:0")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def case(B, N, T, d, seed=3, L=3, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    P = make_params(d, seed, scale)
    V = torch.randn(B, N, d, generator=g, dtype=torch.float64)
    Qs = [torch.randn(B, T, d, generator=g, dtype=torch.float64) * (2.0 / d) ** 0.5 for _ in range(L)]
    gv = torch.randn(L, B, d, generator=g, dtype=torch.float64)
    gq = torch.randn(L, B, d, generator=g, dtype=torch.float64)
    return V, Qs, P, gv, gq


def layout_geometry(B, N, d, layout):
    """(buffer shape, offset of element (0,0,0) in floats, (sB, sN, sD)) of the [B,N,d] view a layout hands to the C-ABI."""
    if layout == "lm":
        return (B, N, d), 0, (N * d, d, 1)
    if layout == "cm":
        return (B, d, N), 0, (d * N, 1, N)
    if layout == "pad":              # buf[:, 1:1+N, 2:2+d] of [B, N+2, d+5]
        return (B, N + 2, d + 5), (d + 5) + 2, ((N + 2) * (d + 5), d + 5, 1)
    if layout == "cmpad":            # buf[:, 1:, 2:2+N] of [B, d+1, N+3], viewed [B,N,d]
        return (B, d + 1, N + 3), (N + 3) + 2, ((d + 1) * (N + 3), 1, N + 3)
    if layout == "col2":             # buf[:, :, ::2] of [B, N, 2d]
        return (B, N, 2 * d), 0, (N * 2 * d, 2 * d, 2)
    raise ValueError(layout)


class Guarded:
    """A device buffer of exactly `n` floats with GUARD_FLOATS guard words behind it.  body: the n floats (filled with NaN
    unless `fill` says otherwise); check(): the guard words, and every cell of the body outside `view`, are bit-unchanged."""

    def __init__(self, n, fill=float("nan")):
        self.n = int(n)
        self.flat = torch.empty(self.n + GUARD_FLOATS, device=_dev())
        self.flat.view(torch.int32).fill_(GUARD_BITS)
        self.body = self.flat[:self.n]
        if fill is not None:
            self.body.fill_(fill)
        self.view = self.body
        self.before = None

    def shaped(self, *shape):
        self.view = self.body.view(*shape)
        return self.view

    def placed(self, B, N, d, layout, values=None):
        """The [B,N,d] view of `layout` inside the body (the body keeps the guard pattern outside the view)."""
        shape, off, strides = layout_geometry(B, N, d, layout)
        self.body.view(torch.int32).fill_(GUARD_BITS)
        self.view = torch.as_strided(self.body, (B, N, d), strides, off)
        if values is not None:
            self.view.copy_(values)
        else:
            self.view.fill_(float("nan"))
        assert tuple(self.view.stride()) == strides or 1 in (B, N, d)
        return self.view

    def snapshot(self):
        self.before = self.flat.clone()

    def check(self, what):
        tail = self.flat[self.n:].view(torch.int32)
        assert bool((tail == GUARD_BITS).all()), "%s: a guard word behind the buffer was overwritten" % what
        if self.before is not None:                  # a padded buffer: nothing outside the view may change
            now = self.flat.clone()
            ref = self.before.clone()
            for t in (now, ref):
                torch.as_strided(t, self.view.shape, self.view.stride(), self.view.storage_offset()).zero_()
            assert torch.equal(now.view(torch.int32), ref.view(torch.int32)), "%s: a cell outside the view was written" % what


def _layout_numel(B, N, d, layout):
    shape = layout_geometry(B, N, d, layout)[0]
    return shape[0] * shape[1] * shape[2]


def run(V, Qs, P, gv=None, gq=None, layout="lm", lens=None, g_av=None, g_aq=None, accumulate=0, grads_init=None,
        need_dv=True, infer=False, flags=0, expect_rc=0, dv_layout="same", maps_out=True):
    """One C-ABI forward (+ backward when gv is given).  V [B,N,d] values; `layout` says how the features are handed over
    (LAYOUTS: "lm" a [B,N,d] buffer, "cm" a [B,d,N] one, "pad" / "cmpad" / "col2" views of larger buffers), `dv_layout` the
    same for dV ("same": V's; None or need_dv=False: no dV).  maps_out=False passes NULL for av_out / aq_out.  L = len(Qs).
    Every buffer a call writes has exactly the size the shape or coattn_alt_workspace_bytes gives and guard words behind it,
    which are verified after the calls (as are the cells of a padded dV outside the view).  Returns a dict of fp32 results on
    the host."""
    from vqa_amd import _lib
    lib = _lib.load()
    DEV = _dev()
    B, N, d = V.shape
    L, T = len(Qs), Qs[0].shape[1]
    assert 1 <= L <= 4
    if dv_layout == "same":
        dv_layout = layout
    if not need_dv:
        dv_layout = None
    Vg = Guarded(_layout_numel(B, N, d, layout), fill=None)
    Vd = Vg.placed(B, N, d, layout, V.float().to(DEV))
    sB, sN, sD = layout_geometry(B, N, d, layout)[2]
    Qd = [q.float().to(DEV).contiguous() for q in Qs]
    ps = [P[n].float().to(DEV).contiguous() for n in NAMES]
    p = _lib.AltParams(*[t.data_ptr() for t in ps])
    qlen = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens is not None else None
    s = C.c_size_t(); f = C.c_size_t(); b = C.c_size_t()
    rc = lib.coattn_alt_workspace_bytes(B, N, T, d, L, 0, flags, C.byref(s), C.byref(f), C.byref(b))
    if flags:
        assert rc < 0 and b"flags" in lib.coattn_last_error()
        s, f, b = (C.c_size_t(x) for x in _lib.alt_workspace_bytes(B, N, T, d, L))
    else:
        assert rc == 0
    assert s.value % 4 == 0 and f.value % 4 == 0 and b.value % 4 == 0
    guards = {}
    saved = None
    if not infer:
        guards["saved"] = Guarded(s.value // 4)
        saved = guards["saved"].body
    guards["ws_fwd"] = Guarded(f.value // 4)
    for k, n in (("v", L * B * d), ("q", L * B * d), ("a_v", L * B * N), ("a_q", L * B * T)):
        guards[k] = Guarded(n)
    v, q = guards["v"].shaped(L, B, d), guards["q"].shaped(L, B, d)
    av, aq = guards["a_v"].shaped(L, B, N), guards["a_q"].shaped(L, B, T)
    qptr = (C.c_void_p * L)(*[x.data_ptr() for x in Qd])
    rc = lib.coattn_alt_forward(_ptr(Vd), sB, sN, sD, qptr, _ptr(qlen), C.byref(p), _ptr(v), _ptr(q),
                                _ptr(av if maps_out else None), _ptr(aq if maps_out else None),
                                _ptr(saved), _ptr(guards["ws_fwd"].body), B, N, T, d, L, 0, flags, None)
    if expect_rc:
        assert rc < 0, rc
        return None
    assert rc == 0, lib.coattn_last_error()
    out = {"v": v, "q": q, "a_v": av if maps_out else None, "a_q": aq if maps_out else None}
    if gv is not None:
        assert saved is not None
        gvd, gqd = gv.float().to(DEV).contiguous(), gq.float().to(DEV).contiguous()
        gavd = g_av.float().to(DEV).contiguous() if g_av is not None else None
        gaqd = g_aq.float().to(DEV).contiguous() if g_aq is not None else None
        guards["ws_bwd"] = Guarded(b.value // 4)
        dV, dvs = None, (0, 0, 0)
        if dv_layout is not None:
            guards["dV"] = Guarded(_layout_numel(B, N, d, dv_layout), fill=None)
            dV = guards["dV"].placed(B, N, d, dv_layout)
            guards["dV"].snapshot()
            dvs = layout_geometry(B, N, d, dv_layout)[2]
        dQ = []
        for l in range(L):
            guards["dQ%d" % l] = Guarded(B * T * d)
            dQ.append(guards["dQ%d" % l].shaped(B, T, d))
        grads = []
        for i, (n, t) in enumerate(zip(NAMES, ps)):
            guards["d" + n] = Guarded(t.numel())
            gt = guards["d" + n].shaped(*t.shape)
            if grads_init is not None:
                gt.copy_(grads_init[i].float().reshape(t.shape))
            grads.append(gt)
        pg = _lib.AltParamGrads(*[t.data_ptr() for t in grads])
        dqptr = (C.c_void_p * L)(*[x.data_ptr() for x in dQ])
        rc = lib.coattn_alt_backward(_ptr(Vd), sB, sN, sD, qptr, _ptr(qlen), C.byref(p), _ptr(saved), _ptr(gvd), _ptr(gqd),
                                     _ptr(gavd), _ptr(gaqd), _ptr(dV), *dvs, dqptr, C.byref(pg), accumulate,
                                     _ptr(guards["ws_bwd"].body), B, N, T, d, L, 0, 0, None)
        assert rc == 0, lib.coattn_last_error()
        out["dV"] = dV
        out["dQ"] = torch.stack(dQ)
        for n, t in zip(NAMES, grads):
            out["d" + n] = t
    torch.cuda.synchronize()
    for k, g in guards.items():
        g.check(k)
    return {k: (x.cpu().contiguous() if x is not None else None) for k, x in out.items()}


def rel(a, b, floor=1e-30):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(floor))


# The gradients of the score biases c_h1..3 are zero in exact arithmetic (a softmax does not see a shift): they are compared as
# absolute errors, as tests/test_gpu_bilinear.py does for c_v, c_q
ABS = ("dc_h1", "dc_h2", "dc_h3")


def check(out, ref, tol=TOL, keys=None, loose=None):
    loose = loose or {}
    keys = keys or [k for k in out if out[k] is not None]
    errs = {}
    for k in keys:
        r = torch.stack(ref[k]) if isinstance(ref[k], list) else ref[k]
        errs[k] = rel(out[k], r.reshape(out[k].shape), 1.0 if k in ABS else 1e-30)
    bad = {k: e for k, e in errs.items() if not e <= loose.get(k, tol)}
    assert not bad, (bad, errs)
    return errs


# ---- the dispatch rules of csrc/coattn_alt.hip, restated ------------------------------------------------------------------

MAX_PARTS = 32                     # kAltMaxParts


def _projection(M, K, strides=(), aligned=True):
    """The linear job alt_linear over plain rows (gemm_w_supported, exact mode): the pre-split-weight kernel or the general
    GEMM."""
    ok = M >= 128 and K >= 32 and K % 32 == 0 and all(s % 4 == 0 for s in strides) and aligned
    return "gemm_w" if ok else "general"


def _tn_parts(rows, levels, n_out, n_in):
    """gemm_tn_plan with max_parts = kAltMaxParts (128 x 128 tiles, 16-row k steps)."""
    ntiles = (n_out // 128) * (n_in // 128)
    want = -(-512 // ntiles) // levels
    if want * levels > MAX_PARTS:
        want = MAX_PARTS // levels
    want = max(want, 1)
    ks = -(-(-(-rows // want)) // 16) * 16
    return levels * -(-rows // ks)


def _splitk_parts(rows, levels):
    per = max(MAX_PARTS // levels, 1)
    ks = -(-(-(-rows // per)) // 16) * 16
    return levels * -(-rows // ks)


def _wgrad(rows, levels, n_out, d, aligned=True):
    """alt_wgrad (gemm_tn_supported): (path, parts)."""
    if d % 128 == 0 and rows >= 16 and aligned:
        return "gemm_tn", _tn_parts(rows, levels, n_out, d)
    return "splitk", _splitk_parts(rows, levels)


def paths(B, N, T, d, L, layout="lm", dv_layout="same"):
    """Which GEMM every product of one forward + backward call takes, from the rules of the linear job alt_linear (rows and
    strided views of V / dV) and the weight-gradient job alt_wgrad of csrc/coattn_alt.hip (exact mode: gemm_bf never
    applies; workspace offsets and whole allocations are 16-byte aligned).  Returns a dict: per product one of "gemm_w",
    "gemm_w_ask", "general", "general_mdiv", "gemm_tn", "splitk", "grouped" (dV: None without a dV), and "parts": the part
    count of every fixed-order reduction."""
    if dv_layout == "same":
        dv_layout = layout
    _, off, (sB, sN, sD) = layout_geometry(B, N, d, layout)
    aligned = off % 4 == 0
    v_rows = sD == 1 and sN == d and sB == N * d
    r = {}
    r["x13"] = _projection(B * T, d, (d, 2 * d))
    if v_rows:
        r["x2"] = _projection(B * N, d, (d,), aligned)
    elif (sN == 1 and N % 4 == 0 and sD % 4 == 0 and sB % 4 == 0 and (B * N) % 4 == 0 and B * N >= 128 and d % 32 == 0
          and aligned):
        r["x2"] = "gemm_w_ask"
    else:
        r["x2"] = "general_mdiv" if sB != N * sN else "general"
    for k in ("g2", "g3", "dvt", "dsh"):
        r[k] = _projection(L * B, d, (d,))
    r["dq"] = _projection(B * T, 2 * d, (2 * d, d))
    if dv_layout is None:
        r["dv"] = None
    else:
        _, _, (dB, dN, dD) = layout_geometry(B, N, d, dv_layout)
        if dD == 1 and dN == d and dB == N * d:
            r["dv"] = _projection(B * N, d, (d,))
        else:
            r["dv"] = "general_mdiv" if dB != N * dN else "general"
    parts = {}
    r["dw_x13"], parts["dw_x13"] = _wgrad(B * T, L, 2 * d, d)
    if v_rows:
        r["dw_x2"], parts["dw_x2"] = _wgrad(B * N, 1, d, d, aligned)
    else:
        G = -(-B // MAX_PARTS)
        r["dw_x2"], parts["dw_x2"] = "grouped", -(-B // G)
        parts["group"] = G
    r["dw_g"], parts["dw_g"] = _wgrad(L * B, 1, d, d)
    parts["steps13"], parts["step2"] = L * B, B          # w_h / c_h / bias partials of the guided kernels
    r["parts"] = parts
    return r


def path_id(B, N, T, d, L, layout="lm", dv_layout="same"):
    """A test id that states the path of every product of the case."""
    r = paths(B, N, T, d, L, layout, dv_layout)
    short = {"gemm_w": "w", "gemm_w_ask": "wask", "general": "gen", "general_mdiv": "mdiv", "gemm_tn": "tn", "splitk": "sk",
             "grouped": "grp", None: "none"}
    p = r["parts"]
    return ("B%d_N%d_T%d_d%d_L%d-%s-x13.%s-x2.%s-g.%s-dq.%s-dv.%s-dwx13.%s%d-dwx2.%s%d-dwg.%s%d"
            % (B, N, T, d, L, layout, short[r["x13"]], short[r["x2"]], short[r["g2"]], short[r["dq"]], short[r["dv"]],
               short[r["dw_x13"]], p["dw_x13"], short[r["dw_x2"]], p["dw_x2"], short[r["dw_g"]], p["dw_g"]))

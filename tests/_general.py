"""The general-shape path of the parallel co-attention (csrc/api.hip general_projections, general_attention, backward_general;
csrc/small_kernels.hip; csrc/gemm.hip launch_gemm_impl) for the tests: run(), one forward (+ backward) through the C-ABI
with every buffer the calls write inside a marker-filled arena, and paths(), the path's dispatch rules restated in plain
Python (tests/test_general_cpu.py pins them at every threshold; tests/test_gpu_general_paths.py holds its table against
them).

paths() assumes what run() provides: every buffer starts 16-byte aligned (the arenas put a buffer 4096 floats into a
torch allocation), the defaults of the developer switches, the exact mode (COATTN_FLAG_BF16_PROJ never set), and extents
below the 1 GiB limits of gemm_w_supported."""
import ctypes as C

import torch

from vqa_amd import _lib

NAMES = ("W_v.weight", "W_v.bias", "W_q.weight", "W_q.bias", "w_v.weight", "w_v.bias", "w_q.weight", "w_q.bias")
BIL_NAMES = ("W_b.weight", "W_b.bias")
FAMILIES = ("plain", "len", "maps", "maps_len", "infer")
LAYOUTS = ("cm", "lm", "strided", "sd2")
GUARD_FLOATS = 4096
GUARD_BITS = 0x5A5AA5A5            # the marker: a finite float (1.5e16), so a read of it cannot hide as a NaN


def _dev():
    return torch.device("cuda:0")


def layout_geometry(B, N, d, layout):
    """(floats of the buffer, (sB, sN, sD)) of the [B,N,d] view a layout hands to the C-ABI.  cm: [B,d,N]; lm: [B,N,d];
    strided: location-major rows padded to sN = d + 4, every sample padded by 8 floats (neither dense layout);
    sd2: every second float of a [B,N,2d] buffer (sD = 2: neither axis contiguous).  Not in LAYOUTS (tests/_fused.py): the
    dense layouts with a gap behind every sample -- lm_gap (sB = N d + 64), lm_gap4 (+ 4), lm_gap1 (+ 1: samples off the
    16-byte boundary), cm_gap (sB = d N + 64), cm_gap4 (+ 4), cm_gap1 (+ 1) -- and pitch, location-major rows d + 8 floats
    apart with the samples abutting (sB = N sN: tests/test_gpu_backward_routes.py's general-shape rows)."""
    gaps = {"lm_gap": 64, "lm_gap4": 4, "lm_gap1": 1, "cm_gap": 64, "cm_gap4": 4, "cm_gap1": 1}
    if layout in gaps:
        sB = N * d + gaps[layout]
        return B * sB, ((sB, d, 1) if layout.startswith("lm") else (sB, 1, N))
    if layout == "lm":
        return B * N * d, (N * d, d, 1)
    if layout == "cm":
        return B * N * d, (d * N, 1, N)
    if layout == "strided":
        sB = N * (d + 4) + 8
        return B * sB, (sB, d + 4, 1)
    if layout == "sd2":
        return B * N * 2 * d, (N * 2 * d, 2 * d, 2)
    if layout == "pitch":
        return B * N * (d + 8), (N * (d + 8), d + 8, 1)
    raise ValueError(layout)


class Arena:
    """A device buffer of exactly `n` floats with GUARD_FLOATS marker words on both sides.  body: the n floats, NaN-filled
    (fill=None: marker-filled).  check(): both margins still hold the marker, and -- after placed() -- so does every cell of
    the body outside the view."""

    def __init__(self, n, fill=float("nan")):
        self.n = int(n)
        self.flat = torch.empty(self.n + 2 * GUARD_FLOATS, device=_dev())
        self.flat.view(torch.int32).fill_(GUARD_BITS)
        self.body = self.flat[GUARD_FLOATS:GUARD_FLOATS + self.n]
        assert self.body.data_ptr() % 16 == 0
        if fill is not None:
            self.body.fill_(fill)
        self.view = None

    def placed(self, B, N, d, layout, values=None, offset=0):
        """The [B,N,d] view of `layout` in the body, `offset` floats behind its start: `values`, or NaN; the body's other
        cells keep the marker."""
        n, strides = layout_geometry(B, N, d, layout)
        assert n + offset == self.n
        self.body.view(torch.int32).fill_(GUARD_BITS)
        self.view = torch.as_strided(self.body, (B, N, d), strides, self.body.storage_offset() + offset)
        if values is not None:
            self.view.copy_(values)
        else:
            self.view.fill_(float("nan"))
        return self.view

    def check(self, what):
        bits = self.flat.view(torch.int32)
        assert bool((bits[:GUARD_FLOATS] == GUARD_BITS).all()), "%s: a word in front of the buffer was overwritten" % what
        assert bool((bits[GUARD_FLOATS + self.n:] == GUARD_BITS).all()), "%s: a word behind the buffer was overwritten" % what
        if self.view is not None:
            rest = self.flat.clone()
            torch.as_strided(rest, self.view.shape, self.view.stride(), self.view.storage_offset()).view(torch.int32).fill_(GUARD_BITS)
            assert bool((rest.view(torch.int32) == GUARD_BITS).all()), "%s: a cell outside the view was written" % what


def _al64(n):
    return (n + 63) & ~63


def state_views(saved, B, N, T, d, L):
    """C [L,B,T,N], a_v [L,B,N], a_q [L,B,T] of the forward's state (tests/_hip.py saved_views)."""
    o = _al64(B * N * d) + _al64(L * B * T * d)
    out = {}
    for name, shape in (("C", (L, B, T, N)), ("a_v", (L, B, N)), ("a_q", (L, B, T))):
        n = 1
        for s in shape:
            n *= s
        out[name] = saved[o:o + n].view(*shape)
        o += _al64(n)
    return out


def profile_marks(lib):
    """coattn_profile_end: the launch marks recorded since coattn_profile_begin on this thread."""
    us = (C.c_float * 48)()
    names = C.create_string_buffer(2048)
    n = lib.coattn_profile_end(us, names, 2048, 48)
    assert n >= 0, lib.coattn_last_error().decode()
    torch.cuda.synchronize()
    marks = names.value.decode().split("\n") if n else []
    assert len(marks) == n
    return marks


def run(V, Qs, P, family="plain", lens=None, gv=None, gq=None, g_av=None, g_aq=None, layout="cm", dv_layout="same",
        flags=_lib.IMPL_GENERAL, accumulate=0, grads_init=None, v_off=0, q_off=0, attn=False, profile=False, allow_nan=False,
        profile_bwd=False):
    """One forward (+ backward when gv is given) through the C-ABI.  V [B,d,N] values (as oracle.coattn_oracle makes them),
    handed over in the physical `layout` (LAYOUTS); family (FAMILIES): coattn_forward / _backward ("plain"), their _len
    forms ("len", with `lens`), coattn_forward_maps / _backward_maps ("maps", "maps_len": g_av / g_aq may be given) or
    coattn_infer / coattn_infer_len ("infer": forward only, _len when `lens` is given).  dv_layout: dV's own layout ("same":
    V's; None: dV = NULL).  flags: COATTN_IMPL_* | COATTN_FLAG_FAST16 | COATTN_FLAG_BILINEAR (then P holds W_b.weight /
    W_b.bias and the result dW_b.weight / dW_b.bias).
    `saved`, both workspaces, v, q, both maps, dV, every dQ[l] and every parameter gradient are allocated at exactly the size
    coattn_workspace_bytes or the shape gives, NaN-filled, inside an Arena; after the calls every margin holds the marker, a
    padded dV keeps every cell outside its view, and no output cell is NaN.  Returns fp32 results on the host: v, q, a_v,
    a_q, C (from the state, not for "infer"), and with a backward dV_phys [B,d,N] (None without dV), dQ [L,B,T,d] and
    d<name>.
    v_off / q_off: floats (0 or 1) by which the V view / every Q_l is moved off its 16-byte aligned start.  attn (families
    "plain" and "len"): coattn_attention_forward(_len) follows on the same `saved` with fresh NaN-filled v, q and workspace
    arenas; v, q are then that call's and "v_fwd", "q_fwd" the forward's.  profile: the forward call(s) run between
    coattn_profile_begin / _end and "marks" is the list of launch marks; profile_bwd: so does the backward call, a profile of
    its own, and "marks_bwd" is the list of its launch marks.  allow_nan: outputs may hold NaN (poisoned inputs)."""
    lib = _lib.load()
    DEV = _dev()
    assert family in FAMILIES
    B, d, N = V.shape
    L, T = len(Qs), Qs[0].shape[1]
    masked = lens is not None
    assert family == "infer" or masked == (family in ("len", "maps_len"))
    bil = bool(flags & _lib.FLAG_BILINEAR)
    names = NAMES + (BIL_NAMES if bil else ())
    if dv_layout == "same":
        dv_layout = layout
    n_v, vstr = layout_geometry(B, N, d, layout)
    Vd = Arena(n_v + v_off, fill=None).placed(B, N, d, layout, V.float().permute(0, 2, 1).to(DEV), offset=v_off)
    assert Vd.data_ptr() % 16 == 4 * v_off
    Qd = [q.float().to(DEV).contiguous() for q in Qs]
    if q_off:
        Qd = [torch.cat([q.new_zeros(q_off), q.reshape(-1)])[q_off:].view(q.shape) for q in Qd]
        assert all(q.data_ptr() % 16 == 4 * q_off for q in Qd)
    ps = [P[k].float().to(DEV).contiguous() for k in names]
    p = _lib.Params(*[t.data_ptr() for t in ps])
    sb, fb, bb = (C.c_size_t() for _ in range(3))
    rc = lib.coattn_workspace_bytes(B, N, T, d, L, _lib.F32, flags, C.byref(sb), C.byref(fb), C.byref(bb))
    assert rc == 0, lib.coattn_last_error()
    assert sb.value % 4 == 0 and fb.value % 4 == 0 and bb.value % 4 == 0
    st = torch.cuda.current_stream().cuda_stream
    dims = dict(B=B, N=N, T=T, d=d, L=L, dtype=_lib.F32, flags=flags, stream=st)
    qlen = torch.tensor(lens, dtype=torch.int32, device=DEV) if masked else None
    g = {"ws_fwd": Arena(fb.value // 4)}
    for k, n in (("v", L * B * d), ("q", L * B * d), ("a_v", L * B * N), ("a_q", L * B * T)):
        g[k] = Arena(n)
    v, q = g["v"].body.view(L, B, d), g["q"].body.view(L, B, d)
    a_v, a_q = g["a_v"].body.view(L, B, N), g["a_q"].body.view(L, B, T)
    fwd = dict(V=Vd, v_sB=vstr[0], v_sN=vstr[1], v_sD=vstr[2], Q=_lib.ptr_array(Qd), p=p, v_out=v, q_out=q,
               ws=g["ws_fwd"].body, **dims)
    if masked:
        fwd["q_len"] = qlen
    sfx = "_len" if masked else ""
    saved = None
    if family == "infer":
        symbol = "coattn_infer" + sfx
        fwd.update(av_out=a_v, aq_out=a_q)
    else:
        g["saved"] = Arena(sb.value // 4)
        saved = g["saved"].body
        fwd["saved"] = saved
        if family.startswith("maps"):
            symbol = "coattn_forward_maps" + sfx
            fwd.update(av_out=a_v, aq_out=a_q)
        else:
            symbol = "coattn_forward" + sfx
    call = _lib.bind(symbol, **fwd)
    if profile:
        torch.cuda.synchronize()
        _lib.check(lib.coattn_profile_begin(st), "coattn_profile_begin")
    rc = call.fn(*call)
    assert rc == 0, (symbol, lib.coattn_last_error())
    out = {"v": v, "q": q}
    written = ["v", "q"]
    if attn:
        assert family in ("plain", "len")
        for k, n in (("ws_attn", fb.value // 4), ("v_attn", L * B * d), ("q_attn", L * B * d)):
            g[k] = Arena(n)
        out.update(v_fwd=v, q_fwd=q, v=g["v_attn"].body.view(L, B, d), q=g["q_attn"].body.view(L, B, d))
        written += ["v_fwd", "q_fwd"]
        call = _lib.bind("coattn_attention_forward" + sfx, **dict(fwd, v_out=out["v"], q_out=out["q"], ws=g["ws_attn"].body))
        rc = call.fn(*call)
        assert rc == 0, (call.name, lib.coattn_last_error())
    marks = profile_marks(lib) if profile else None
    torch.cuda.synchronize()
    if family == "infer" or family.startswith("maps"):
        out.update(a_v=a_v, a_q=a_q)
        written += ["a_v", "a_q"]
    if saved is not None:
        sv = state_views(saved, B, N, T, d, L)
        out["C"] = sv["C"]
        written += ["C", "a_v", "a_q"]
        if "a_v" in out:                                     # the caller's maps are the state's, bit for bit
            assert torch.equal(a_v.view(torch.int32), sv["a_v"].view(torch.int32))
            assert torch.equal(a_q.view(torch.int32), sv["a_q"].view(torch.int32))
        else:
            out.update(a_v=sv["a_v"], a_q=sv["a_q"])
    if gv is not None:
        assert saved is not None
        to = lambda t: None if t is None else t.float().to(DEV).contiguous()    # noqa: E731
        g["ws_bwd"] = Arena(bb.value // 4)
        dV, dvs = None, (0, 0, 0)
        if dv_layout is not None:
            n_dv, dvs = layout_geometry(B, N, d, dv_layout)
            g["dV"] = Arena(n_dv, fill=None)
            dV = g["dV"].placed(B, N, d, dv_layout)
        dQ = []
        for l in range(L):
            g["dQ%d" % l] = Arena(B * T * d)
            dQ.append(g["dQ%d" % l].body.view(B, T, d))
        grads = []
        for i, (k, t) in enumerate(zip(names, ps)):
            g["d" + k] = Arena(t.numel())
            gt = g["d" + k].body.view(t.shape)
            if grads_init is not None:
                gt.copy_(grads_init[i].float().reshape(t.shape))
            grads.append(gt)
        pg = _lib.ParamGrads(*[t.data_ptr() for t in grads])
        bwd = dict(V=Vd, v_sB=vstr[0], v_sN=vstr[1], v_sD=vstr[2], Q=_lib.ptr_array(Qd), p=p, saved=saved, gv=to(gv),
                   gq=to(gq), dV=dV, dv_sB=dvs[0], dv_sN=dvs[1], dv_sD=dvs[2], dQ=_lib.ptr_array(dQ), pg=pg,
                   accumulate=accumulate, ws=g["ws_bwd"].body, **dims)
        if masked:
            bwd["q_len"] = qlen
        if family.startswith("maps"):
            symbol = "coattn_backward_maps" + sfx
            bwd.update(g_av=to(g_av), g_aq=to(g_aq))
        else:
            assert g_av is None and g_aq is None
            symbol = "coattn_backward" + sfx
        call = _lib.bind(symbol, **bwd)
        if profile_bwd:
            torch.cuda.synchronize()
            _lib.check(lib.coattn_profile_begin(st), "coattn_profile_begin")
        rc = call.fn(*call)
        assert rc == 0, (symbol, lib.coattn_last_error())
        marks_bwd = profile_marks(lib) if profile_bwd else None
        torch.cuda.synchronize()
        out["dV_phys"] = dV.permute(0, 2, 1) if dV is not None else None
        out["dQ"] = torch.stack(dQ)
        written.append("dQ")
        for k, t in zip(names, grads):
            out["d" + k] = t
            written.append("d" + k)
        if dV is not None:
            written.append("dV_phys")
    for k, a in g.items():
        a.check(k)
    for k in written:
        assert allow_nan or not bool(torch.isnan(out[k]).any()), "%s: a cell is NaN (left unwritten, or computed from one that was)" % k
    res = {k: (x.detach().cpu().contiguous() if x is not None else None) for k, x in out.items()}
    if profile:
        res["marks"] = marks
    if profile_bwd and gv is not None:
        res["marks_bwd"] = marks_bwd
    return res


# ---- the dispatch rules, restated ------------------------------------------------------------------------------------------

def fused_supported(N, T, d, L):
    """csrc/coattn_fused.hip fused_supported."""
    return d > 0 and d % 256 == 0 and d <= 4096 and T <= 28 and N <= 208 and L <= 3


def _al4(*xs):
    return all(x % 4 == 0 for x in xs)


def gemm_kernel(M, N, K, batch=1, a_sm=0, a_sk=0, a_sz=0, a_si=0, a_mdiv=0, a_sdiv=0, b_sk=0, b_sn=0, b_sz=0, b_si=0,
                ksplit=0, x3=True):
    """launch_gemm_f32 -> launch_gemm_impl (csrc/gemm.hip) for 16-byte aligned operands: (kernel, xcd_group).  The aligned
    fast path ("vec": M >= 128, each operand contiguous along one axis, every other stride, K and the split a multiple of 4)
    runs gemm_f32_vec_kernel: by default (COATTN_GEMM_X3 = 1) its fp32-accurate three-piece form on 128-row tiles
    ("vec128"); x3=False is the f32-MFMA form behind that developer switch, which takes 64-row tiles ("vec64") when
    768 < wg128 < 2304.  Everything else runs gemm_f32_kernel<32> (M <= 64: "f32_32") or <128> ("f32_128").  xcd_group: 32
    or more row tiles (the vec kernels only)."""
    a_m = a_sm == 1 and a_sk != 1
    b_n = b_sn == 1
    vec = M >= 128 and (a_sk == 1 or a_sm == 1) and (b_sk == 1 or b_sn == 1)
    if vec:
        vec = _al4(M, a_sk, a_mdiv, a_sdiv) if a_m else _al4(a_sm, a_sdiv)
        vec = vec and (_al4(N, b_sk) if b_n else _al4(b_sn))
        vec = vec and _al4(K, ksplit, a_sz, a_si, b_sz, b_si)
    if vec:
        bm = 128
        if not x3:
            wg128 = -(-N // 128) * -(-M // 128) * batch
            bm = 64 if 768 < wg128 < 3 * 768 else 128
        return "vec%d" % bm, -(-M // bm) >= 32
    return ("f32_32" if M <= 64 else "f32_128"), False


def gemv_kernel(I, x_si, x_sk):
    """launch_gemv: (kernel, workgroups along i)."""
    if x_sk == 1:
        return "kcontig", -(-I // 4)
    return ("icontig" if x_si == 1 else "generic"), -(-I // 256)


def splitk_plan(K):
    """fused.h splitk_plan: (ks, S)."""
    ks = -(-(-(-K // 32)) // 16) * 16
    return ks, -(-K // ks)


def sample_groups(B):
    """grad_dw_sample_groups: (G samples per part, S parts); the last part is short when G S > B."""
    G = -(-B // 32)
    return G, -(-B // G)


def colsum_plan(R):
    """grad_colsum: (rpc rows per chunk, nch chunks); the last chunk is short when rpc nch > R."""
    rpc = max(-(-R // 256), 32)
    return rpc, -(-R // rpc)


def reduce_kernel(n):
    """launch_reduce_partials over aligned buffers."""
    return "reduce4" if n % 4 == 0 else "reduce1"


def add_kernel(n):
    """launch_add_inplace over aligned buffers."""
    return "add4" if n % 4 == 0 else "add1"


def mask_rows_grid(R, W):
    """launch_mask_rows: (workgroups along x, whether the kernel's loop can make a second pass: R W past the capped grid)."""
    n = R * W
    gx = min(-(-n // 256), 1024)
    return gx, n > gx * 256


def _gemm_w(M, K, batch, a_sm=0, a_sz=0, a_sk=0, a_mdiv=0, a_sdiv=0, f16=False):
    """gemm_w_supported (aligned pointers, weight image below 1 GiB).  f16: the tolerance mode's two FP16 pieces, whose range
    report lives in this kernel -- any M runs on it then; otherwise M >= 128."""
    ok = M >= (1 if f16 else 128) and K >= 32 and K % 32 == 0 and a_sz % 4 == 0 and 1 <= batch <= 8
    if a_sk:
        return (ok and a_mdiv > 0 and _al4(a_mdiv, a_sk, a_sdiv, M)
                and (((M - 1) // a_mdiv + 1) * a_sdiv + K * a_sk) * 4 < 0x40000000)
    return ok and a_sm % 4 == 0 and (M * a_sm + K) * 4 < 0x40000000


def projection_jobs(B, N, T, d, L, strides, f16=False, v_aligned=True, q_aligned=True):
    """api.hip projection_jobs: (v_w, q_w), which projections run on the pre-split-weight kernel.  f16: asked for two FP16
    pieces (want_f16); v_aligned / q_aligned: V / every Q_l on a 16-byte boundary (gemm_w_supported's `pal`)."""
    sB, sN, sD = strides
    v_w = False
    if sD == 1 and sB == N * sN and sN < (1 << 24):
        v_w = _gemm_w(B * N, d, 1, a_sm=sN, f16=f16)
    elif sN == 1 and sD < (1 << 24):
        v_w = _gemm_w(B * N, d, 1, a_sk=sD, a_mdiv=N, a_sdiv=sB, f16=f16)
    return v_w and v_aligned, _gemm_w(B * T, d, L, a_sm=d, f16=f16) and q_aligned


def paths(B, N, T, d, L, layout="cm", dv_layout="same", flags=_lib.IMPL_GENERAL, keep=True):
    """What one forward + backward of run() reaches (keep=False: coattn_infer, no state kept).  {"fused": True} when the
    call leaves the general path (COATTN_IMPL_AUTO on a fused shape in a dense layout); else a dict with
      v_w, q_w, wqT, rowbits: projection_jobs, the W_q^T image and the live-row bitmap (rowbits_predicate);
      marks: the launch marks of the forward (the backward of this path records none);
      gemm[name] = (kernel, xcd_group) for every product launch_gemm_impl takes (None: on the pre-split-weight kernel);
      gemv[name] = (kernel, workgroups along i);  reduce[name] = (kernel, parts);  add: the dP_v accumulation's kernel;
      splitk = (ks, S) of dW_q;  groups = (G, S) of dW_v;  colsum[name] = (rpc, nch), colsum_blocks workgroups along d;
      mask_rows = (grid, second pass) of C / dA under a length mask;  softmax = (passes over N, passes over T)."""
    sel = flags & 3
    bil = bool(flags & _lib.FLAG_BILINEAR)
    if dv_layout == "same":
        dv_layout = layout
    _, (sB, sN, sD) = layout_geometry(B, N, d, layout)
    if sel != _lib.IMPL_GENERAL and fused_supported(N, T, d, L) and layout in ("cm", "lm"):
        return {"fused": True}
    assert sel != _lib.IMPL_FUSED
    r = {"fused": False}
    v_w, q_w = projection_jobs(B, N, T, d, L, (sB, sN, sD))
    r["v_w"], r["q_w"] = v_w, q_w
    r["wqT"] = keep and _gemm_w(B * T, d, L, a_sm=d, a_sz=B * T * d)
    # (exact mode: gemm_wx_kernel = 0; row-major A; b_q given and aligned)
    r["rowbits"] = q_w and (B * T + 31) // 32 <= 512 and d % 256 == 0 and d <= 1024
    marks = []
    if v_w or q_w or r["wqT"]:
        marks.append("wsplit")
    if v_w and q_w:
        marks.append("projections")
    if bil and q_w:
        marks.append("bilinear_projection")
    r["marks"] = marks
    gm = {}
    mdiv = dict(a_mdiv=N, a_sdiv=sB) if sB != N * sN else {}
    gm["proj_v"] = None if v_w else gemm_kernel(B * N, d, d, 1, a_sm=sN, a_sk=sD, b_sk=1, b_sn=d, **mdiv)
    rows_q = dict(a_sm=d, a_sk=1, b_sk=1, b_sn=d)
    gm["proj_q"] = None if q_w else gemm_kernel(B * T, d, d, L, **rows_q)
    if bil:
        gm["proj_k"] = None if q_w else gemm_kernel(B * T, d, d, L, **rows_q)
    gm["affinity"] = gemm_kernel(T, N, d, B, a_sm=d, a_sk=1, a_sz=T * d, b_sk=sD, b_sn=sN, b_sz=sB)
    gm["ct_times"] = gemm_kernel(N, d, T, B, a_sm=1, a_sk=N, a_sz=T * N, b_sk=d, b_sn=1, b_sz=T * d)
    gm["c_times"] = gemm_kernel(T, d, N, B, a_sm=N, a_sk=1, a_sz=T * N, b_sk=d, b_sn=1, b_sz=N * d)
    gm["dC"] = gemm_kernel(T, N, d, B, a_sm=d, a_sk=1, a_sz=T * d, b_sk=1, b_sn=d, b_sz=N * d)
    gm["dQ"] = gemm_kernel(T, d, N, B, a_sm=N, a_sk=1, a_sz=T * N, b_sk=sN, b_sn=sD, b_sz=sB)
    gm["dq_proj"] = gemm_kernel(B * T, d, d, 1, a_sm=d, a_sk=1, b_sk=d, b_sn=1)
    if dv_layout is not None:
        gm["dv_kt_da"] = gemm_kernel(d, N, T, B, a_sm=1, a_sk=d, a_sz=T * d, b_sk=N, b_sn=1, b_sz=T * N)
        gm["dv_wv"] = gemm_kernel(d, N, d, B, a_sm=1, a_sk=d, b_sk=1, b_sn=d, b_sz=N * d)
    G, S = sample_groups(B)
    gm["dw_v"] = gemm_kernel(d, d, N, S, a_sm=1, a_sk=d, a_si=N * d, a_sz=G * N * d, b_sk=sN, b_sn=sD, b_si=sB, b_sz=G * sB)
    ks, Sk = splitk_plan(B * T)
    gm["dw_q"] = gemm_kernel(d, d, B * T, Sk, a_sm=1, a_sk=d, b_sk=d, b_sn=1, ksplit=ks)
    r["gemm"] = gm
    r["gemv"] = {"v": gemv_kernel(d, sD, sN), "q": gemv_kernel(d, 1, d), "da_v": gemv_kernel(N, sN, sD),
                 "da_q": gemv_kernel(T, d, 1)}
    r["groups"], r["splitk"] = (G, S), (ks, Sk)
    cs = {"dw_v": colsum_plan(B * N), "dw_q": colsum_plan(B * T), "db_v": colsum_plan(B * N), "db_q": colsum_plan(L * B * T)}
    if bil:
        cs["db_b"] = colsum_plan(L * B * T)
    r["colsum"] = cs
    r["colsum_blocks"] = -(-d // 256)
    red = {k: (reduce_kernel(d), nch) for k, (_, nch) in cs.items()}
    red["dW_v"] = (reduce_kernel(d * d), S)
    red["dW_q"] = (reduce_kernel(d * d), Sk)
    r["reduce"] = red
    r["add"] = add_kernel(B * N * d)
    r["mask_rows"] = mask_rows_grid(T, N)
    r["softmax"] = (-(-N // 256), -(-T // 256))
    return r

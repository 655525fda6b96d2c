"""The fused forward of the parallel co-attention (csrc/coattn_fwd32.hip coattn_fwd32_kernel and attend_v_lm_kernel,
csrc/coattn_fused.hip attend_v_kernel and fused_attention_forward) for the tests: run_row(), one forward-only call through
the C-ABI with every buffer it writes inside a marker-filled arena (tests/_general.py run()); reference(), the float64
oracle with the affinity C; and fwd_path(), the dispatch restated in plain Python (tests/test_fused_forward_cpu.py pins it at
every threshold, tests/test_gpu_fused_forward.py holds its table against it and the library's launch marks against its)."""
import math

import torch
import torch.nn.functional as F

from vqa_amd import _lib
from oracle import coattn_oracle as O

from tests import _general as G

FAST, BF16, BIL, EXACT3 = _lib.FLAG_FAST16, _lib.FLAG_BF16_PROJ, _lib.FLAG_BILINEAR, _lib.FLAG_EXACT3
AUTO, GENERAL, FUSED = _lib.IMPL_AUTO, _lib.IMPL_GENERAL, _lib.IMPL_FUSED
# G.FAMILIES, and: coattn_infer_len; coattn_forward(_len) followed by coattn_attention_forward(_len) on the same state
FAMILIES = ("plain", "len", "maps", "maps_len", "infer", "infer_len", "attn", "attn_len")
MASKED = ("len", "maps_len", "infer_len", "attn_len")
LAYOUTS = ("lm", "cm", "lm_gap", "lm_gap4", "cm_gap")          # the fused layouts (G.layout_geometry)
NAMES = G.NAMES + G.BIL_NAMES


def bound(flags):
    """The suite's bounds, as a fraction of max|reference|."""
    return 8e-2 if flags & BF16 else (1e-4 if flags & FAST else 2e-5)


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------

def fwd_path(B, N, T, d, L, layout, flags, family, v_aligned=True, q_aligned=True):
    """What one forward call of `family` reaches: csrc/api.hip check_bilinear, pick_impl, call_modes (f16_path over
    projection_jobs, np_fwd), general_projections' and bilinear_projection's launch marks, fused.h map_dst,
    csrc/coattn_fused.hip fused_attention_forward and csrc/coattn_fwd32.hip fused32_forward(_bil) / dispatch_fwd32, with the
    developer switches at their defaults (a shipped build ignores the environment).  v_aligned: V on a 16-byte boundary
    (v_sB comes from the layout); q_aligned: every Q_l.

    Returns a dict: "refused" (the call returns -1 before any launch), else "fused"; "marks", the launch marks of the call(s)
    (the attn families: the forward's, then coattn_attention_forward's); "f16", whether the projections and the kernel run on
    two FP16 pieces; "proj" = (v_w, q_w), which projections run on the pre-split-weight kernel; and on the fused path "tuple"
    = (NT, NW, LM, NP_, FV, MASK, MAPS, BIL), the instantiation of coattn_fwd32_kernel, and "attend": None (FV: the kernel
    attends V itself), "lm" (attend_v_lm_kernel), "cm4" / "cm13" (attend_v_kernel<4> / <13>).

    Compiled but reached only by a -DCOATTN_DEV_SWITCHES build, and so deliberately untested:
      * every NP_ = 2 form (phase 2 on two bf16 pieces: COATTN_FWD_F16=0 or COATTN_FWD_F16_KERNEL=0 under COATTN_FLAG_FAST16);
      * the location-major NT = 2, NW = 4 forms without FV (COATTN_FUSE_V=0: attend_v_lm_kernel behind the small-grid kernel)."""
    assert family in FAMILIES
    sel = flags & 3
    bil, bf16 = bool(flags & BIL), bool(flags & BF16)
    fast = bool(flags & FAST) and not flags & EXACT3
    if bil and bf16:
        return {"refused": True}                                # check_bilinear
    _, (sB, sN, sD) = G.layout_geometry(B, N, d, layout)
    lm, cm = sD == 1 and sN == d, sN == 1 and sD == N           # v_is_lm first (fused_attention_forward)
    ok = G.fused_supported(N, T, d, L) and (lm or cm) and v_aligned and sB % 4 == 0
    if sel == FUSED and not ok:
        return {"refused": True}
    fused = ok and sel != GENERAL
    keep = not family.startswith("infer")
    jobs = lambda f16: G.projection_jobs(B, N, T, d, L, (sB, sN, sD), f16=f16, v_aligned=v_aligned, q_aligned=q_aligned)  # noqa: E731
    f16 = fused and fast and not bf16 and all(jobs(True))       # f16_path: both projections on the kernel that range-checks
    v_w, q_w = jobs(f16)
    wqT = keep and B * T >= 128                                 # dq_proj_job on gemm_w: the image of W_q^T for the backward
    marks = ["wsplit"] if (v_w or q_w or wqT) else []
    if v_w and q_w:
        marks.append("projections")
    if bil and q_w:
        marks.append("bilinear_projection")
    r = {"refused": False, "fused": bool(fused), "f16": bool(f16), "proj": (bool(v_w), bool(q_w))}
    if not fused:
        assert not family.startswith("attn")
        r["marks"] = marks                                      # (the general path records no mark behind the projections)
        return r
    NT, NW = (2 if N <= 64 else 7), (4 if d % 512 == 0 else 2)
    FV = lm and N <= 64 and d % 512 == 0
    if bf16:
        NP = 1 if d % 512 == 0 else 3                           # (np = 3; the two-wave forms have no single-product kernel)
    else:
        NP = 4 if f16 else 3                                    # np_fwd: FAST16 without the FP16 path computes exactly
    MAPS = family in ("maps", "maps_len")                       # map_dst: a copy only beside a kept state
    r["tuple"] = (NT, NW, lm, NP, FV, family in MASKED, MAPS, bil)
    r["attend"] = None if FV else ("lm" if lm else ("cm4" if N <= 64 else "cm13"))
    kernel = ["coattn_fwd32"] + ([] if FV else ["attend_v"])
    r["marks"] = marks + kernel + (kernel if family.startswith("attn") else [])
    return r


# ---- inputs and the float64 oracle ----------------------------------------------------------------------------------------------

def ragged(B, T):
    """Zero pad rows behind every question but the first (the workload's questions)."""
    return [T] + [1 + (7 * b) % T for b in range(1, B)]


_params, _inputs, _refs = {}, {}, {}


def params(d):
    if d not in _params:
        _params[d] = O.make_params(d, 3)
    return _params[d]


def inputs(B, N, T, d, L, lens=None):
    """V [B,d,N] >= 0 of unit scale and L questions [B,T,d] of scale sqrt(2/d) -- the affinity's pre-activation then has unit
    variance and tanh stays off its flat ends -- whose rows from `lens` (default ragged()) on are exact zeros."""
    key = (B, N, T, d, L, None if lens is None else tuple(lens))
    if key not in _inputs:
        pad = [min(max(int(x), 1), T) for x in (lens if lens is not None else ragged(B, T))]    # (the kernels' clamp)
        _inputs[key] = O.make_inputs(B, N, T, d, 13, lens=pad, scale_q=(2.0 / d) ** 0.5, L=L)
    return _inputs[key]


def reference(V, Qs, P, bilinear=False, lens=None, dtype=torch.float64, device="cpu"):
    """The co-attention of the reference (model.py:372-392; with `bilinear` the affinity tanh((Q W_b^T + b_b) V^T)) in `dtype`:
    v, q [L,B,d], a_v [L,B,N], a_q [L,B,T], C [L,B,T,N].  Under `lens` it is the unmasked computation on Q[b, :len_b] alone
    (lengths clamped into [1, T]), written with the masked rows of C set to zero -- they then add exact zeros to H_v -- and
    the softmax over t < len_b; a_q and C are 0 past a length.  (tests/_bilinear.py forward() is the same definition sample
    by sample; tests/test_fused_forward_cpu.py holds the two against each other.)"""
    dd = dict(device=device, dtype=dtype)
    V = V.to(**dd)
    Pd = {k: P[k].to(**dd) for k in NAMES}
    B, T = Qs[0].shape[0], Qs[0].shape[1]
    Vn = V.permute(0, 2, 1)
    Pv = F.linear(Vn, Pd["W_v.weight"], Pd["W_v.bias"])
    live = None
    if lens is not None:
        n = torch.tensor([min(max(int(x), 1), T) for x in lens], device=device)
        live = torch.arange(T, device=device)[None, :] < n[:, None]            # [B,T]
    out = {k: [] for k in ("v", "q", "a_v", "a_q", "C")}
    for Q in Qs:
        Q = Q.to(**dd)
        if live is not None:
            Q = Q * live[:, :, None]
        K = F.linear(Q, Pd["W_b.weight"], Pd["W_b.bias"]) if bilinear else Q
        C = torch.tanh(torch.bmm(K, V))
        if live is not None:
            C = C * live[:, :, None]
        Pq = F.linear(Q, Pd["W_q.weight"], Pd["W_q.bias"])
        H_v = torch.tanh(Pv + torch.bmm(C.transpose(2, 1), Pq))
        H_q = torch.tanh(Pq + torch.bmm(C, Pv))
        s_v = F.linear(H_v, Pd["w_v.weight"], Pd["w_v.bias"]).squeeze(2)
        s_q = F.linear(H_q, Pd["w_q.weight"], Pd["w_q.bias"]).squeeze(2)
        if live is not None:
            s_q = s_q.masked_fill(~live, -math.inf)
        a_v, a_q = F.softmax(s_v, dim=1), F.softmax(s_q, dim=1)
        out["v"].append(torch.bmm(a_v[:, None, :], Vn).squeeze(1))
        out["q"].append(torch.bmm(a_q[:, None, :], Q).squeeze(1))
        out["a_v"].append(a_v); out["a_q"].append(a_q); out["C"].append(C)
    return {k: torch.stack(x).cpu() for k, x in out.items()}


def row_reference(row, dtype=torch.float64, device="cpu"):
    """reference() of a table row (B, N, T, d, L, layout, flags, family, lens, options), computed once per distinct input."""
    B, N, T, d, L, _, flags, family, lens = row[:9]
    masked = family in MASKED
    key = (B, N, T, d, L, bool(flags & BIL), tuple(lens) if lens is not None else None, masked, dtype)
    if key not in _refs:
        V, Qs = inputs(B, N, T, d, L, lens)
        _refs[key] = reference(V, Qs, params(d), bool(flags & BIL), lens if masked else None, dtype, device)
    return _refs[key]


def errors(out, ref):
    """{output: max|out - ref| / max|ref|} over the outputs both hold."""
    return {k: float((out[k].double() - ref[k].double()).abs().max()) / float(ref[k].abs().max())
            for k in ("v", "q", "a_v", "a_q", "C") if k in out}


# ---- the runner -----------------------------------------------------------------------------------------------------------------

def run_row(row, V=None, Qs=None, profile=True, allow_nan=False, **over):
    """One forward-only call (the attn families: two) of a table row through G.run(): `saved`, the workspace, v, q and both
    maps between marker words at their exact sizes.  V, Qs: other inputs than inputs() of the row; over: fields of the row
    replaced by name (layout, flags, family, lens).  Returns G.run()'s outputs and "marks"."""
    B, N, T, d, L, layout, flags, family, lens = row[:9]
    opt = dict(row[9]) if len(row) > 9 else {}
    layout, flags, family = over.get("layout", layout), over.get("flags", flags), over.get("family", family)
    lens = over.get("lens", lens)
    if V is None:
        V, Qs = inputs(B, N, T, d, L, lens)
    masked = family in MASKED
    base = {"infer_len": "infer", "attn": "plain", "attn_len": "len"}.get(family, family)
    return G.run(V, Qs, params(d), family=base, lens=lens if masked else None, layout=layout, flags=flags,
                 attn=family.startswith("attn"), profile=profile, allow_nan=allow_nan, v_off=opt.get("v_off", 0),
                 q_off=opt.get("q_off", 0))


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))

"""The fused backward of the parallel co-attention (csrc/coattn_fused_bwd.hip fused_backward, bwd_pre_kernel and
bwd_dq_kernel; csrc/coattn_bwd32.hip bwd_dc32_kernel, bwd_nat32_kernel, bwd_dq32_kernel and bwd_dq32x_kernel) for the tests:
bwd_path(), the backward's dispatch restated in plain Python (tests/test_fused_backward_cpu.py pins it at every threshold
and against the twenty recorded mark lists of tests/test_gpu_backward_routes.py; tests/test_gpu_fused_backward.py holds its
table against it and the library's launch marks against its); case(), the inputs, upstream gradients and float64 oracle of
a table row; run_row(), one forward + backward through the C-ABI with every buffer the calls write inside a marker-filled
arena (tests/_general.py run()); and errors(), every compared tensor against the oracle.

A row is the forward table's (tests/_fused.py): (B, N, T, d, L, layout, flags, family, lens, options) with family one of
FAMILIES and the options  dv (default 1; 0: dV = NULL), gm ("both": G_av and G_aq given, "av": G_aq = NULL -- the maps
families), acc (accumulate = 1 onto given gradients), q_off / v_off (every Q_l / V four bytes off a 16-byte boundary)."""
import torch

from oracle import coattn_oracle as O

from tests import _bilinear as BL
from tests import _fused as FU
from tests import _general as G

FAST, BF16, BIL, EXACT3 = FU.FAST, FU.BF16, FU.BIL, FU.EXACT3
AUTO, GENERAL, FUSED = FU.AUTO, FU.GENERAL, FU.FUSED
FAMILIES = ("plain", "len", "maps", "maps_len")             # coattn_backward, _len, _maps, _maps_len behind their forwards
MASKED = ("len", "maps_len")
NAMES = BL.NAMES
ABS = ("dw_v.bias", "dw_q.bias")                            # dc_v, dc_q: zero in exact arithmetic, compared absolute
TN_PARTS, MAX_PARTS, DYN_LEVELS, ROWBITS_MAX_WORDS, DYN_MAX_ROWS = 32, 40, 4, 512, 8192   # fused.h; decide_route


# ---- the predicates the route asks, restated (aligned operands unless a flag says otherwise) ---------------------------------

def gemm_tn(M, Nc, K, levels=1, a_ld=4, b_ld=4, b_kdiv=0, b_sdiv=0, aligned=True, a_bf16=False):
    """csrc/gemm_tn.hip gemm_tn_supported (128 x 128 tiles, BK = 16; the 1 GiB extents are far off every fused shape)."""
    ok = (not a_bf16 and M > 0 and Nc > 0 and M % 128 == 0 and Nc % 128 == 0 and K >= 16 and 1 <= levels <= 8
          and a_ld % 4 == 0 and b_ld % 4 == 0 and aligned)
    if b_kdiv:                                                  # B contiguous along k inside groups of b_kdiv rows
        ok = ok and levels == 1 and b_kdiv >= 16 and b_kdiv % 4 == 0 and b_sdiv % 4 == 0 and K % b_kdiv == 0
    return bool(ok)


def gemm_tn_wide(M, Nc, bf16, tn):
    """csrc/gemm_tn_wide.hip gemm_tn_wide_supported (128 x 256 tiles) of a job gemm_tn_supported takes."""
    return tn and not bf16 and M % 128 == 0 and Nc % 256 == 0


def gemm_bf_tn(M, Nc, K, bf16, levels=1, b_kdiv=0, aligned=True, a_bf16=False, a_ld=8, a_term=0, a_sl=0):
    """csrc/gemm_bf.hip gemm_bf_tn_supported (256 x 256 tiles, 32-row steps; reduced-precision mode only)."""
    ok = (bf16 and not b_kdiv and M >= 256 and Nc >= 256 and M % 256 == 0 and Nc % 256 == 0 and K >= 32 and K % 32 == 0
          and 1 <= levels <= 8 and a_ld % 4 == 0 and a_term % 4 == 0 and a_sl % 4 == 0 and aligned)
    if a_bf16:
        ok = ok and a_ld % 8 == 0 and a_term % 8 == 0 and a_sl % 8 == 0
    return bool(ok)


def gemm_bf(M, Nc, K, batch, bf16, a_sm, a_sz, a_bf16=False):
    """csrc/gemm_bf.hip gemm_bf_supported (TM = TN = 256, TK = 64), row-major A."""
    ok = (bf16 and M >= 256 and Nc >= 256 and Nc % 256 == 0 and K >= 64 and K % 64 == 0 and a_sm % 4 == 0 and a_sz % 4 == 0
          and 1 <= batch <= 8)
    if a_bf16:
        ok = ok and a_sm % 8 == 0 and a_sz % 8 == 0
    return bool(ok)


def gemm_w(M, K, batch, a_sm, a_sz):
    """csrc/gemm_w.hip gemm_w_supported of the dQ projection's job (fused.h dq_proj_job: row-major A, never two FP16 pieces)."""
    return bool(G._gemm_w(M, K, batch, a_sm=a_sm, a_sz=a_sz))


def live_rows(fp, d, flags):
    """csrc/api.hip rowbits_in_saved: may `saved` hold the forward's bitmap of the non-zero question rows?  P_q on the
    pre-split-weight kernel (fwd_path()'s "proj"), computed exactly on gemm_w_kernel (no FP16 pieces, not the reduced-precision
    mode), d % 256 == 0 and d <= 1024; b_q and `saved` are 16-byte aligned in every call of the tests, and B T / 32 words stay
    below kRowBitsMaxWords wherever the fused path reaches."""
    return bool(fp["proj"][1] and not fp["f16"] and not flags & BF16 and d % 256 == 0 and d <= 1024)


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------

def bwd_path(B, N, T, d, L, layout, flags, family, dv=True, v_aligned=True, q_aligned=True, grads_aligned=True, gm="both"):
    """What one backward call of `family` behind its forward reaches: csrc/api.hip backward_impl (check_bilinear, pick_impl,
    call_modes' np_bwd, rowbits_in_saved), csrc/coattn_fused_bwd.hip fused_backward (decide_route, run_pre / launch_pre, run_dq,
    the three weight-gradient drivers) and csrc/coattn_bwd32.hip dispatch_dc32, dispatch_nat32 and launch_bwd_dq32, with the
    predicates they ask (gemm_tn, gemm_tn_wide, gemm_bf_tn, gemm_bf, gemm_w over fused.h dq_proj_job) and the developer
    switches at their defaults (a shipped build ignores the environment).  dv: dV requested; v_aligned / q_aligned: V / every
    Q_l on a 16-byte boundary; grads_aligned: dW_v and dW_q; gm (the maps families): "both" map gradients given, "av" (G_aq
    NULL), "aq" (G_av NULL) or None (both NULL).  Only the forward puts the state in `saved`: what the backward learns from it
    is taken from tests/_fused.py fwd_path() of the same call -- which projections ran on the pre-split-weight kernel and in
    which pieces (the row bitmap), and with them whether the image of W_q^T exists (fwd_path: B T >= 128, the same
    gemm_w_supported(dq_proj_job) the backward asks).

    Returns a dict: "refused" (the call returns -1 before any launch), else "fused" (False: backward_general, which records no
    launch mark); "marks", the launch marks of the backward call; and on the fused path
      "dc32" = (NT, NW, NP, MASK, GMAP) of bwd_dc32_kernel, "nat32" = (NT, NW, NP, DPB, GMAP) of bwd_nat32_kernel,
      "dq" = ("x" | "32" | "f32", NT, LM, NP): bwd_dq32x_kernel<2, LM, NP>, bwd_dq32_kernel<7, LM, NP> or the exact-f32
          bwd_dq_kernel<4 | 13, false, false> (NP = 3: fp32 products),
      "pre" = (GMAP, "lm" | "cm", plan): bwd_pre_maps_kernel or bwd_pre_kernel, its da_v block, the plan workgroup,
      "group" = (NT, NW, LM), and the route booleans that change results or launches: "tn_v", "tn_q", "dq32", "wdq",
      "combine", "wide", "bf_tn", "red_in_dq", "use_dyn", "sum_in_gemm", "dp_bf16".

    Compiled but reached only by a -DCOATTN_DEV_SWITCHES build, and so deliberately untested:
      * bwd_dq32_kernel<2, LM, NP> (COATTN_DQ32X=0: the per-level kernel at N <= 64);
      * bwd_dq_kernel<NT, true, LM> and <NT, ALIGNED, true> (the exact-f32 kernel runs only for channel-major features with
        N % 4 != 0: rows off the 16-byte boundary, never location-major);
      * the own-dQ route (COATTN_OWN_DQ=1: the dQ projection on gemm_h2.hip's persistent kernel behind the weight gradients),
        and with it "bwd_gemm_dq_projection" behind "bwd_gemm_dw";
      * COATTN_NO_COMBINE, COATTN_RED_IN_DQ=0, COATTN_DW_LIVE_ROWS=0, COATTN_DP_BF16=0, COATTN_TN_WIDE(3)=0, COATTN_TN_PARTS
        and the knock-outs COATTN_KO_DPV / COATTN_KO_SUM3."""
    assert family in FAMILIES and gm in ("both", "av", "aq", None)
    bil, bf16 = bool(flags & BIL), bool(flags & BF16)
    fast = bool(flags & FAST) and not flags & EXACT3
    if bil and bf16:
        return {"refused": True}                                # check_bilinear
    fp = FU.fwd_path(B, N, T, d, L, layout, flags, family, v_aligned=v_aligned, q_aligned=q_aligned)
    if fp["refused"]:
        return {"refused": True}                                # pick_impl, on the same V: the same answer as the forward's
    if not fp["fused"]:
        return {"refused": False, "fused": False, "marks": []}
    _, (sB, sN, sD) = G.layout_geometry(B, N, d, layout)
    lm = sD == 1 and sN == d
    maps, masked = family.startswith("maps"), family in MASKED
    g_av, g_aq = maps and gm in ("both", "av"), maps and gm in ("both", "aq")
    np_ = 2 if fast and not bf16 else 3                         # decide_route: r.np
    dyn = live_rows(fp, d, flags) and L <= DYN_LEVELS and (B * T + 31) // 32 <= ROWBITS_MAX_WORDS and TN_PARTS > L
    # which of the backward's GEMMs take the hand-scheduled kernels
    BNd, BTd = B * N * d, B * T * d
    if lm and sB == N * sN:
        tnv = dict(b_ld=sN)                                     # location-major rows, samples abutting
    elif not lm:
        tnv = dict(b_ld=sD, b_kdiv=N, b_sdiv=sB)                # channel-major, read in place
    else:
        tnv = None                                              # a gap behind location-major samples: the general GEMM
    tn_v = tnv is not None and gemm_tn(d, d, B * N, 1, a_ld=d, aligned=v_aligned, **tnv)
    tn_q = gemm_tn(d, d, B * T, L, a_ld=d, b_ld=d, aligned=q_aligned)
    dq32 = lm or N % 4 == 0
    wdq = gemm_w(B * T, d, L, a_sm=d, a_sz=BTd)
    assert wdq == (B * T >= 128)                                # the forward wrote the image it reads (fwd_path: wqT)
    wdq_bf = gemm_bf(B * T, d, d, L, bf16, a_sm=d, a_sz=BTd)
    all3 = dq32 and wdq and tn_v and tn_q
    combine = all3 and not wdq_bf and not bil
    late_dq = combine                                           # (own_dq: a developer switch)
    bf_v = lambda abf, term: tn_v and gemm_bf_tn(d, d, B * N, bf16, 1, b_kdiv=0 if lm else N, a_bf16=abf, a_ld=d, a_term=term)   # noqa: E731
    bf_q = lambda abf: tn_q and gemm_bf_tn(d, d, B * T, bf16, L, a_bf16=abf, a_ld=d, a_sl=BTd)   # noqa: E731
    dp_bf16 = (bf16 and not dv and L == 3 and d % 512 == 0 and all3 and bf_v(True, BNd) and bf_q(True)
               and gemm_bf(B * T, d, d, L, bf16, a_sm=d, a_sz=BTd, a_bf16=True))
    sum_in_gemm = tn_v and L == 3 and not dv
    bf_tn = tn_v and tn_q and bf_v(dp_bf16, BNd if sum_in_gemm else 0) and bf_q(dp_bf16)
    if bf_tn:                                                   # gemm_bf.hip's weight-gradient launch carries no dQ tiles
        combine = late_dq = False
    wide = red_in_dq = use_dyn = False
    if tn_v and tn_q and not bf_tn:
        wide = gemm_tn_wide(d, d, bf16, tn_v) and gemm_tn_wide(d, d, bf16, tn_q)     # (combine: d % 256 == 0, equal widths)
        red_in_dq = late_dq and dq32 and (d * d) % 4 == 0 and grads_aligned
        use_dyn = (dyn and wide and red_in_dq and B * T <= DYN_MAX_ROWS and not dp_bf16
                   and (B * T + 31) // 32 <= ROWBITS_MAX_WORDS and L < TN_PARTS <= MAX_PARTS and L <= DYN_LEVELS)
    # the launches
    marks = ["bwd_pre", "bwd_dc32", "bwd_nat32"]
    if bil:                                                     # run_bilinear_dq_dwb: dK = dA V on the dA V kernel
        marks += ["bwd_dq", "bwd_bilinear_dq", "bwd_bilinear_dwb"]
    elif not late_dq:
        marks += (["bwd_gemm_dq_projection"] if dq32 else []) + ["bwd_dq"]
    if bf_tn:                                                   # run_dw_bf_tn
        marks += ["bwd_gemm_dw", "reduce_partials"]
    elif tn_v and tn_q:                                         # run_dw_tn_pair
        marks.append("bwd_gemm" if combine else "bwd_gemm_dw")
        marks += ["bwd_dq"] if red_in_dq else ((["bwd_dq"] if late_dq else []) + ["reduce_partials"])
    # (run_dw_separate, run_dv and run_sum_dpv record no mark)
    NT, NW = (2 if N <= 64 else 7), (4 if d % 512 == 0 else 2)
    NP = (1 if bf16 else np_) if NW == 4 else np_               # (the two-wave forms have no single-product kernel)
    if dq32:
        dq = ("x" if N <= 64 and L <= 3 else "32", NT, lm, 1 if bf16 else np_)
    else:
        dq = ("f32", 4 if N <= 64 else 13, False, 3)
    return {"refused": False, "fused": True, "marks": marks, "group": (NT, NW, lm),
            "dc32": (NT, NW, NP, masked, bool(g_av)), "nat32": (NT, NW, NP, bool(dp_bf16), bool(g_av)), "dq": dq,
            "pre": (bool(g_aq), "lm" if lm else "cm", bool(dyn)),
            "tn_v": bool(tn_v), "tn_q": bool(tn_q), "dq32": bool(dq32), "wdq": bool(wdq), "combine": bool(combine),
            "wide": bool(wide), "bf_tn": bool(bf_tn), "red_in_dq": bool(red_in_dq), "use_dyn": bool(use_dyn),
            "sum_in_gemm": bool(sum_in_gemm), "dp_bf16": bool(dp_bf16)}


def mirror(row):
    """(fwd_path(), bwd_path()) of a table row."""
    B, N, T, d, L, layout, flags, family, _, opt = row
    al = dict(v_aligned=not opt.get("v_off"), q_aligned=not opt.get("q_off"))
    return (FU.fwd_path(B, N, T, d, L, layout, flags, family, **al),
            bwd_path(B, N, T, d, L, layout, flags, family, dv=bool(opt.get("dv", 1)), gm=opt.get("gm", "both"), **al))


# ---- inputs, upstream gradients and the float64 oracle ---------------------------------------------------------------------------

_cases = {}


def upstream(row):
    """gv, gq [L,B,d] and, in the maps families, G_av [L,B,N] and G_aq [L,B,T] (None where the row passes NULL).  gq and the
    map gradients are unit normals; gv is normal of scale d^-1/2: the image features are of unit scale in every channel, the
    question rows of norm sqrt(2) (FU.inputs), so the score gradients da_v[n] = gv . V_n and da_q[t] = gq . Q_t both come out of
    unit scale -- neither side of the softmax backward drowns the other or the map gradients added to it, and dc_v, dc_q, which
    are compared as absolute errors, are sums of terms of unit scale at every d."""
    B, N, T, d, L, _, _, family, _, opt = row
    hn = lambda shape, seed: torch.from_numpy(O.hash_normal(shape, seed)).float()      # noqa: E731
    gm = opt.get("gm", "both") if family.startswith("maps") else None
    return (hn((L, B, d), 23) * d ** -0.5, hn((L, B, d), 24), hn((L, B, N), 41) if gm in ("both", "av") else None,
            hn((L, B, T), 42) if gm in ("both", "aq") else None)


def case(row, dtype=torch.float64, device="cpu"):
    """(V, Qs, P, gv, gq, g_av, g_aq, ref) of a row: FU.inputs / FU.params, upstream(), and tests/_bilinear.py
    forward_backward in `dtype`, computed once per distinct input."""
    B, N, T, d, L, _, flags, family, lens, opt = row
    masked = family in MASKED
    gm = opt.get("gm", "both") if family.startswith("maps") else None
    key = (B, N, T, d, L, bool(flags & BIL), tuple(lens) if lens is not None else None, masked, gm, dtype)
    if key not in _cases:
        V, Qs = FU.inputs(B, N, T, d, L, lens)
        P = FU.params(d)
        gv, gq, g_av, g_aq = upstream(row)
        ref = BL.forward_backward(V, Qs, P, gv, gq, bilinear=bool(flags & BIL), lens=lens if masked else None, g_av=g_av,
                                  g_aq=g_aq, device=device, dtype=dtype)
        _cases[key] = (V, Qs, P, gv, gq, g_av, g_aq, ref)
    return _cases[key]


def grads_init(row, ref):
    """accumulate = 1: gradients to add onto, of each gradient's own magnitude (the sum then rounds at that magnitude, which
    the bound is relative to)."""
    names = NAMES if row[6] & BIL else NAMES[:8]
    P = FU.params(row[3])
    return [torch.from_numpy(O.hash_normal(tuple(P[k].shape), 60 + i)).float() * float(ref["d" + k].abs().max())
            for i, k in enumerate(names)]


def compared(row):
    """The tensors a row is compared in."""
    names = NAMES if row[6] & BIL else NAMES[:8]
    return ("v", "q", "a_v", "a_q", "dQ") + (("dV_phys",) if row[9].get("dv", 1) else ()) + tuple("d" + k for k in names)


def absolute(row):
    """The gradients of a row that are zero in exact arithmetic -- sums over a softmax backward, which adds up to nothing -- and so
    are compared as absolute errors: dc_v and dc_q always; dw_v over a single location (N = 1: a_v = 1, ds_v = 0) and dw_q over
    a single token (T = 1, or every length 1) too; with both, nothing reaches the projections: dW_v, db_v, dW_q, db_q."""
    N, T, family, lens = row[1], row[2], row[7], row[8]
    if family in MASKED:
        T = max(min(max(int(x), 1), T) for x in lens)
    both = ("dW_v.weight", "dW_v.bias", "dW_q.weight", "dW_q.bias") if N == 1 and T == 1 else ()
    return ABS + (("dw_v.weight",) if N == 1 else ()) + (("dw_q.weight",) if T == 1 else ()) + both


def errors(row, out, ref, init=None):
    """{tensor: max|out - ref| as a fraction of max|ref| (absolute(row): absolute)} over compared(row); init: grads_init() of an
    accumulate = 1 row."""
    names = NAMES if row[6] & BIL else NAMES[:8]
    errs = {}
    for k in compared(row):
        want = ref[k].double().reshape(out[k].shape)
        scale = 1.0 if k in absolute(row) else float(want.abs().max())
        if init is not None and k[1:] in names:
            want = want + init[names.index(k[1:])].double().reshape(want.shape)
        errs[k] = float((out[k].double() - want).abs().max()) / scale
    return errs


# ---- the runner -----------------------------------------------------------------------------------------------------------------

def run_row(row, V=None, Qs=None, profile=True, device=None, **over):
    """One forward + backward of a table row through G.run(): `saved`, both workspaces, every output and every gradient between
    marker words at their exact sizes.  V, Qs: other inputs than FU.inputs() of the row; over: fields of the row or of its
    options replaced by name (layout, flags, family, lens, dv, gm, acc, g_av, g_aq).  Returns G.run()'s outputs, with
    "marks" (the forward's) and "marks_bwd" when profiled, and "init" (the gradients an accumulate = 1 row adds onto)."""
    B, N, T, d, L, layout, flags, family, lens, opt = row
    opt = dict(opt)
    for k in ("dv", "gm", "acc"):
        if k in over:
            opt[k] = over[k]
    layout, flags, family = over.get("layout", layout), over.get("flags", flags), over.get("family", family)
    lens = over.get("lens", lens)
    row = (B, N, T, d, L, layout, flags, family, lens, opt)
    if V is None:
        V, Qs = FU.inputs(B, N, T, d, L, lens)
    gv, gq, g_av, g_aq = upstream(row)
    g_av, g_aq = over.get("g_av", g_av), over.get("g_aq", g_aq)
    init = None
    if opt.get("acc"):
        init = grads_init(row, case(row, device=device or "cpu")[-1])
    out = G.run(V, Qs, FU.params(d), family=family, lens=lens if family in MASKED else None, gv=gv, gq=gq, g_av=g_av, g_aq=g_aq,
                layout=layout, dv_layout="same" if opt.get("dv", 1) else None, flags=flags, accumulate=1 if init else 0,
                grads_init=init, v_off=opt.get("v_off", 0), q_off=opt.get("q_off", 0), profile=profile, profile_bwd=profile)
    out["init"] = init
    return out

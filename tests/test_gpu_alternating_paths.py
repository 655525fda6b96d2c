"""GPU: every dispatch, stride and limit branch of csrc/coattn_alt.hip against the float64 oracle of tests/_alternating.py,
through the C-ABI runner of that module: the guided kernels' column / row / lane passes and level counts, each GEMM family
per product (gemm_w with partial tiles and its channel-major a_sk form, the general GEMM with and without the row split,
gemm_tn with K tails, the general split-K and the grouped weight gradient), every feature and gradient layout, the length
clamp, the optional arguments, saturated and non-finite inputs, and the argument checks.

Bound (that of tests/test_gpu_alternating.py): max|err| / max|ref| <= 2e-5 on every output and gradient, the score biases'
gradients dc_h* (zero in exact arithmetic) as absolute errors.  Every case prints its worst error per output group.

Which kernel a product reaches is stated in the case's id; the id comes from tests/_alternating.py paths(), the dispatch
rules of the linear job (alt_linear) and the weight-gradient job (alt_wgrad) restated in Python
(tests/test_alternating_cpu.py pins them at every threshold), and every table row below is held against paths() when the
module is collected.  The library's launch marks (coattn_profile_begin / _end) are per phase, not per kernel, so the path
is not asserted on the GPU; the marks themselves are pinned by test_launch_marks.

Every run also checks the guard words of tests/_alternating.py run(): `saved`, both workspaces, every output and gradient
are allocated at exactly their size, and a padded dV keeps every cell outside its view."""
import ctypes as C
import functools

import pytest
import torch

import vqa_amd
from vqa_amd import _lib

from tests import _alternating as AL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES = AL.NAMES
TOL = AL.TOL
GROUPS = {
    "fwd": ("v", "q", "a_v", "a_q"), "dV": ("dV",), "dQ": ("dQ",),
    "W": tuple("d" + n for n in NAMES if n[0] == "W"),
    "b_wh": tuple("d" + n for n in NAMES if n[0] != "W"),
}


def _report(tag, ident, errs):
    worst = {g: max([errs[k] for k in ks if k in errs], default=None) for g, ks in GROUPS.items()}
    print("alt_paths %s %s" % (tag, ident), {g: "%.1e" % e for g, e in worst.items() if e is not None})


def _lens(B, T):
    return [1 + (3 * b) % T for b in range(B)]


@functools.lru_cache(maxsize=None)
def _reference(B, N, T, d, L, lens, g_av=True, g_aq=True, seed=None, scale=1.0, c_h=None):
    """The case and its float64 reference, computed once per argument set (the layouts of a case share it; nothing
    changes it afterwards)."""
    V, Qs, P, gv, gq = AL.case(B, N, T, d, seed=(B + 3 * N + 5 * T + d + L) if seed is None else seed, L=L, scale=scale)
    if c_h is not None:
        for n, x in zip(("c_h1", "c_h2", "c_h3"), c_h):
            P[n] = torch.full((1,), float(x), dtype=torch.float64)
    g = torch.Generator().manual_seed(7 + B)
    gav = torch.randn(L, B, N, generator=g, dtype=torch.float64) if g_av else None
    gaq = torch.randn(L, B, T, generator=g, dtype=torch.float64) if g_aq else None
    lens = list(lens) if lens is not None else None
    ref = AL.forward_backward(V, Qs, P, gv, gq, gav, gaq, lens)
    return (V, Qs, P, gv, gq, gav, gaq), ref


def _check_case(tag, ident, shape, L, layout, masked, dv_layout="same", lens=None):
    B, N, T, d = shape
    if lens is None and masked:
        lens = _lens(B, T)
    (V, Qs, P, gv, gq, gav, gaq), ref = _reference(B, N, T, d, L, tuple(lens) if lens is not None else None)
    out = AL.run(V, Qs, P, gv, gq, layout=layout, dv_layout=dv_layout, lens=lens, g_av=gav, g_aq=gaq)
    keys = [k for k in out if out[k] is not None]
    errs = {k: AL.rel(out[k], (torch.stack(ref[k]) if isinstance(ref[k], list) else ref[k]).reshape(out[k].shape),
                      1.0 if k in AL.ABS else 1e-30) for k in keys}
    _report(tag, ident, errs)
    loose = None
    if (shape, L, lens is not None) in F32_BOUND:
        # the bound of such a case: 4 x the error of the oracle's own float32 evaluation, per output, where that is above
        # the family's bound (the factor: the kernels' summation order and tanh_fast's 2e-7)
        e32 = AL.forward_backward(V, Qs, P, gv, gq, gav, gaq, lens, dtype=torch.float32)
        loose = {k: max(TOL, 4 * AL.rel(torch.stack(e32[k]) if isinstance(e32[k], list) else e32[k],
                                         torch.stack(ref[k]) if isinstance(ref[k], list) else ref[k],
                                         1.0 if k in AL.ABS else 1e-30)) for k in keys}
        print("alt_paths f32_bound %s" % ident, {k: "%.1e" % v for k, v in loose.items() if v > TOL})
    AL.check(out, ref, loose=loose)
    if lens is not None:
        for b, n in enumerate(lens):
            n = max(1, min(n, T))
            assert (out["a_q"][:, b, n:] == 0).all() and (out["dQ"][:, b, n:] == 0).all()
    return out, ref


def _expect(shape, L, layout, dv_layout, want):
    """Collection-time check that a table row reaches the path it names."""
    got = AL.paths(*shape, L, layout, dv_layout)
    for k, v in want.items():
        have = got["parts"][k[6:]] if k.startswith("parts.") else got[k]
        assert have == v, (shape, L, layout, k, have, v)


# Cases (shape, L, masked) whose bound comes from the float32 evaluation of the oracle: above the family's bound with no
# defect found by reading (LAB_NOTES.md section 11)
F32_BOUND = {((2, 3, 2, 1), 3, False)}

MASKS = [pytest.param(False, id="unmasked"), pytest.param(True, id="masked")]

# ---- a. guided-kernel sizes ----------------------------------------------------------------------------------------------
# (shape, L, what the guided kernels reach).  Every product on the general GEMM and the split-K unless `want` says otherwise.
ALL_GENERAL = {"x13": "general", "g2": "general", "dq": "general", "dw_x13": "splitk", "dw_g": "splitk"}
GUIDED = [
    ((2, 3, 2, 1), 3, "d1", ALL_GENERAL),
    ((3, 7, 5, 7), 3, "odd_d_unaligned_halves", ALL_GENERAL),
    ((2, 7, 5, 65), 3, "one_lane_in_second_lane_pass", ALL_GENERAL),
    ((2, 7, 5, 100), 3, "d_mod4_not_mod32", ALL_GENERAL),
    ((2, 7, 5, 576), 3, "second_column_pass", ALL_GENERAL),
    # the d limit.  B T = 10, B N = 14 and L B = 6 rows: under gemm_tn's 16-row floor, so the weights stay on the split-K
    ((2, 7, 5, 1024), 3, "d_limit", ALL_GENERAL),
    # ... and with 20 / 28 rows the weight gradients of the d limit on gemm_tn (an 16 x 8 and an 8 x 8 tile grid)
    ((4, 7, 5, 1024), 3, "d_limit_gemm_tn", {"dw_x13": "gemm_tn", "dw_x2": "gemm_tn", "dw_g": "splitk"}),
    ((2, 1, 1, 64), 3, "R1", ALL_GENERAL),
    ((2, 17, 9, 64), 3, "second_row_pass", ALL_GENERAL),
    ((2, 70, 65, 64), 3, "R_over_64", {"x13": "gemm_w", "x2": "gemm_w", "dq": "gemm_w", "g2": "general"}),
    ((2, 512, 512, 64), 3, "R_limit", {"x13": "gemm_w", "x2": "gemm_w", "g2": "general"}),
    ((3, 7, 5, 64), 1, "one_level", ALL_GENERAL),
    ((3, 7, 5, 64), 2, "two_levels", ALL_GENERAL),
    ((3, 7, 5, 64), 4, "four_levels", ALL_GENERAL),
    ((6, 7, 5, 128), 4, "four_levels_gemm_tn_8_parts_per_level",
     {"dw_x13": "gemm_tn", "parts.dw_x13": 8, "dw_x2": "gemm_tn", "dw_g": "gemm_tn"}),
]


def _guided_params():
    ps = []
    for shape, L, what, want in GUIDED:
        for layout in ("lm", "cm"):
            w = dict(want)
            if layout == "cm":
                w.pop("x2", None)
                w["dw_x2"] = "grouped"
            _expect(shape, L, layout, "same", w)
            ps.append(pytest.param(shape, L, layout, id="%s-%s" % (what, AL.path_id(*shape, L, layout))))
    return ps


# lengths of the R limit's masked run: 1 and 511 (the unmasked run is 512 everywhere)
R_LIMIT_LENS = {(2, 512, 512, 64): [1, 511]}


@pytest.mark.parametrize("masked", MASKS)
@pytest.mark.parametrize("shape,L,layout", _guided_params())
def test_guided_kernel_sizes(shape, L, layout, masked):
    """(2, 3, 2, 1) unmasked takes its bound from the oracle's float32 evaluation (F32_BOUND): dW_g3, one scalar at d = 1,
    is off by 3.0e-5 on the GPU and by 1.25e-5 in the float32 evaluation, bound 5.0e-5 (LAB_NOTES.md section 11)."""
    _check_case("guided", "%s L%d %s %s" % (shape, L, layout, "masked" if masked else "unmasked"), shape, L, layout, masked,
                lens=R_LIMIT_LENS.get(shape) if masked else None)


# ---- b. dispatch ---------------------------------------------------------------------------------------------------------
W4 = {"x13": "gemm_w", "g2": "gemm_w", "g3": "gemm_w", "dvt": "gemm_w", "dsh": "gemm_w", "dq": "gemm_w"}
DISPATCH = [
    # 129 rows everywhere: gemm_w for every projection with a 1-row partial last tile; cm: N % 4 != 0 -> general + a_mdiv
    ((43, 3, 3, 64), 3, "lm", dict(W4, x2="gemm_w", dv="gemm_w")),
    ((43, 3, 3, 64), 3, "cm", dict(W4, x2="general_mdiv", dv="general_mdiv")),
    # 130 / 208 rows on gemm_w, the 78 rows of g2, g3, dvt, dsh on the general GEMM; cm: the a_sk form at its smallest,
    # cmpad (sD = 11, an unaligned base): refused -> general + a_mdiv
    ((26, 8, 5, 64), 3, "lm", {"x13": "gemm_w", "x2": "gemm_w", "dq": "gemm_w", "dv": "gemm_w", "g2": "general",
                               "g3": "general", "dvt": "general", "dsh": "general"}),
    ((26, 8, 5, 64), 3, "cm", {"x13": "gemm_w", "x2": "gemm_w_ask", "dq": "gemm_w", "g2": "general"}),
    ((26, 8, 5, 64), 3, "cmpad", {"x13": "gemm_w", "x2": "general_mdiv", "dq": "gemm_w", "dv": "general_mdiv"}),
    # K = 32: one k-step; B T = 90 general, B N = 180 and L B = 135 gemm_w
    ((45, 4, 2, 32), 3, "lm", {"x13": "general", "dq": "general", "x2": "gemm_w", "dv": "gemm_w", "g2": "gemm_w",
                               "dsh": "gemm_w"}),
    ((45, 4, 2, 32), 3, "cm", {"x13": "general", "x2": "gemm_w_ask", "g2": "gemm_w"}),
    # only dQ (K = 2d = 96, 32) qualifies for gemm_w
    ((26, 7, 5, 48), 3, "lm", {"x13": "general", "x2": "general", "dv": "general", "g2": "general", "dq": "gemm_w"}),
    ((26, 7, 5, 48), 3, "cm", {"x13": "general", "x2": "general_mdiv", "dq": "gemm_w"}),
    ((26, 7, 5, 16), 3, "lm", {"x13": "general", "x2": "general", "dv": "general", "g2": "general", "dq": "gemm_w"}),
    ((26, 7, 5, 16), 3, "cm", {"x13": "general", "x2": "general_mdiv", "dq": "gemm_w"}),
    # d = 128 around gemm_tn's 16-row floor: 15 and 9 rows on the split-K (the 21 rows of dW_x2 already on gemm_tn);
    # K tails 20 and 28 with dW_g (12 rows) on the split-K; all four on gemm_tn (30, 42, 18 rows)
    ((3, 7, 5, 128), 3, "lm", {"dw_x13": "splitk", "dw_x2": "gemm_tn", "dw_g": "splitk"}),
    ((3, 7, 5, 128), 3, "cm", {"dw_x13": "splitk", "dw_x2": "grouped", "dw_g": "splitk"}),
    ((4, 7, 5, 128), 3, "lm", {"dw_x13": "gemm_tn", "dw_x2": "gemm_tn", "dw_g": "splitk"}),
    ((4, 7, 5, 128), 3, "cm", {"dw_x13": "gemm_tn", "dw_x2": "grouped", "dw_g": "splitk"}),
    ((6, 7, 5, 128), 3, "lm", {"dw_x13": "gemm_tn", "dw_x2": "gemm_tn", "dw_g": "gemm_tn"}),
    ((6, 7, 5, 128), 3, "cm", {"dw_x13": "gemm_tn", "dw_x2": "grouped", "dw_g": "gemm_tn"}),
    # d = 256, L = 2: a 4 x 2 tile grid with odd K = 35, 45
    ((5, 9, 7, 256), 2, "lm", {"dw_x13": "gemm_tn", "dw_x2": "gemm_tn", "dw_g": "splitk"}),
    ((5, 9, 7, 256), 2, "cm", {"dw_x13": "gemm_tn", "dw_x2": "grouped", "dw_g": "splitk"}),
]
# the grouped dW_x2 (any V that is not location-major): G = 2 with S = 17 and a 1-sample last group; G = 3 with S = 24 and
# a 1-sample last group; G = 2 exact; the reduce's part counts 29, 33 and 99 either side of its unrolled loop
for _layout in ("cm", "pad"):
    DISPATCH += [
        ((33, 7, 5, 64), 3, _layout, {"dw_x2": "grouped", "parts.group": 2, "parts.dw_x2": 17, "parts.step2": 33,
                                      "parts.steps13": 99}),
        ((70, 4, 3, 64), 3, _layout, {"dw_x2": "grouped", "parts.group": 3, "parts.dw_x2": 24}),
        ((64, 4, 3, 32), 3, _layout, {"dw_x2": "grouped", "parts.group": 2, "parts.dw_x2": 32}),
        ((29, 7, 5, 64), 1, _layout, {"dw_x2": "grouped", "parts.group": 1, "parts.dw_x2": 29, "parts.steps13": 29}),
    ]


def _dispatch_params():
    ps = []
    for shape, L, layout, want in DISPATCH:
        _expect(shape, L, layout, "same", want)
        ps.append(pytest.param(shape, L, layout, id=AL.path_id(*shape, L, layout)))
    return ps


@pytest.mark.parametrize("masked", MASKS)
@pytest.mark.parametrize("shape,L,layout", _dispatch_params())
def test_dispatch(shape, L, layout, masked):
    _check_case("dispatch", "%s %s" % (AL.path_id(*shape, L, layout), "masked" if masked else "unmasked"), shape, L, layout,
                masked)


# ---- c. strides ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dv_layout", ["lm", "cm", "pad", None])
@pytest.mark.parametrize("layout", AL.LAYOUTS)
@pytest.mark.parametrize("shape", [(4, 7, 5, 64), (26, 8, 5, 64)])
def test_strides(shape, layout, dv_layout):
    """Every feature layout against every dV layout, masked, with map gradients.  run()'s guard check is the assertion
    that no write lands in a padded buffer's padding."""
    out, _ = _check_case("strides", "%s V=%s dV=%s" % (shape, layout, dv_layout), shape, 3, layout, True, dv_layout=dv_layout)
    assert (out["dV"] is None) == (dv_layout is None)


@pytest.mark.parametrize("view", ["rows_and_columns_sliced", "every_second_column"])
def test_module_takes_strided_views(view):
    """AlternatingCoAttention hands a positive-stride view over by pointer: x = big[:, 1:, :d] and x = big[:, :, ::2]."""
    B, N, T, d = 3, 7, 5, 64
    V, Qs, P, gv, gq = AL.case(B, N, T, d, seed=41)
    mod = vqa_amd.AlternatingCoAttention(d, question_mask=True)
    mod.load_state_dict({AL.state_key(n): P[n].float().reshape(mod.state_dict()[AL.state_key(n)].shape) for n in NAMES})
    mod = mod.to(DEV)
    lens = [5, 2, 1]
    ref = AL.forward_backward(V, Qs, P, gv, gq, lens=lens)
    if view == "rows_and_columns_sliced":
        big = torch.randn(B, N + 1, d + 3, device=DEV)
        x = big[:, 1:, :d]
    else:
        big = torch.randn(B, N, 2 * d, device=DEV)
        x = big[:, :, ::2]
    x.copy_(V.float())
    x = x.detach().requires_grad_(True)
    assert not x.is_contiguous()
    Qd = [q.float().to(DEV).requires_grad_(True) for q in Qs]
    vs, qs, a_v, a_q = mod(x, Qd, lens, return_attention=True)
    (sum((vs[l] * gv[l].float().to(DEV)).sum() + (qs[l] * gq[l].float().to(DEV)).sum() for l in range(3))).backward()
    errs = {"v": AL.rel(torch.stack(vs).cpu(), ref["v"]), "q": AL.rel(torch.stack(qs).cpu(), ref["q"]),
            "a_v": AL.rel(a_v.detach().cpu(), ref["a_v"]), "a_q": AL.rel(a_q.detach().cpu(), ref["a_q"]),
            "dV": AL.rel(x.grad.cpu(), ref["dV"]),
            "dQ": AL.rel(torch.stack([q.grad for q in Qd]).cpu(), torch.stack(ref["dQ"]))}
    for n in NAMES:
        g = mod.state_dict(keep_vars=True)[AL.state_key(n)].grad
        errs["d" + n] = AL.rel(g.cpu().reshape(-1), ref["d" + n].reshape(-1), 1.0 if "d" + n in AL.ABS else 1e-30)
    _report("module", view, errs)
    assert all(e <= TOL for e in errs.values()), errs


# ---- d. lengths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["lm", "cm"])
def test_lengths_are_clamped(layout):
    """alt_rows clamps a length into [1, T]: 0, -3 -> 1; 6, 1000 -> 5 (the oracle's clamp); a_q and dQ are exactly 0 past it
    (asserted by _check_case)."""
    _check_case("lengths", layout, (6, 7, 5, 64), 3, layout, True, lens=[0, -3, 1, 5, 6, 1000])


# ---- e. optional arguments -----------------------------------------------------------------------------------------------
OPT_SHAPES = [(4, 7, 5, 96), (26, 8, 5, 64)]


@pytest.mark.parametrize("infer", [False, True], ids=["saved", "stateless"])
@pytest.mark.parametrize("shape", OPT_SHAPES)
def test_null_map_outputs(shape, infer):
    """av_out = aq_out = NULL: v, q bit-equal to the run with maps; the backward behind it still matches the oracle (its
    a_v, a_q come from `saved`)."""
    B, N, T, d = shape
    lens = _lens(B, T)
    (V, Qs, P, gv, gq, gav, gaq), ref = _reference(B, N, T, d, 3, tuple(lens))
    with_maps = AL.run(V, Qs, P, lens=lens, infer=infer)
    if infer:
        out = AL.run(V, Qs, P, lens=lens, infer=True, maps_out=False)
    else:
        out = AL.run(V, Qs, P, gv, gq, lens=lens, g_av=gav, g_aq=gaq, maps_out=False)
        AL.check(out, ref)
    assert out["a_v"] is None and out["a_q"] is None
    for k in ("v", "q"):
        assert torch.equal(out[k].view(torch.int32), with_maps[k].view(torch.int32)), k
    AL.check(with_maps, ref, keys=["v", "q", "a_v", "a_q"])


@pytest.mark.parametrize("maps", ["g_av", "g_aq", "neither"])
@pytest.mark.parametrize("shape", OPT_SHAPES)
def test_map_gradients_are_optional(shape, maps):
    B, N, T, d = shape
    lens = _lens(B, T)
    (V, Qs, P, gv, gq, gav, gaq), ref = _reference(B, N, T, d, 3, tuple(lens), g_av=maps == "g_av", g_aq=maps == "g_aq")
    out = AL.run(V, Qs, P, gv, gq, lens=lens, g_av=gav, g_aq=gaq)
    AL.check(out, ref)


@pytest.mark.parametrize("shape,layout,dv_layout,want", [
    ((33, 7, 5, 64), "cm", "same", {"dw_x2": "grouped"}),                    # the grouped reduce's own accumulate
    ((6, 7, 5, 128), "lm", "same", {"dw_x13": "gemm_tn", "dw_g": "gemm_tn"}),  # gemm_tn parts
    ((4, 7, 5, 96), "cm", None, {"dw_x2": "grouped", "dv": None}),           # no dV with channel-major V
], ids=["grouped_cm", "gemm_tn", "cm_no_dV"])
def test_accumulate_adds_into_gradients(shape, layout, dv_layout, want):
    B, N, T, d = shape
    _expect(shape, 3, layout, dv_layout, want)
    (V, Qs, P, gv, gq, gav, gaq), ref = _reference(B, N, T, d, 3, None)
    init = [torch.randn(P[n].shape, generator=torch.Generator().manual_seed(i), dtype=torch.float64) for i, n in enumerate(NAMES)]
    out = AL.run(V, Qs, P, gv, gq, layout=layout, dv_layout=dv_layout, g_av=gav, g_aq=gaq, accumulate=1, grads_init=init)
    want_ref = dict(ref)
    for i, n in enumerate(NAMES):
        want_ref["d" + n] = ref["d" + n] + init[i]
    AL.check(out, want_ref)
    assert (out["dV"] is None) == (dv_layout is None)


# ---- f. numerics ---------------------------------------------------------------------------------------------------------
NUM = (3, 9, 6, 64)


@pytest.mark.parametrize("layout", ["lm", "cm"])
def test_saturated_tanh(layout):
    """Weights six times the usual scale: tanh saturates (1 - H^2 cancels) and the maps are near one-hot."""
    B, N, T, d = NUM
    (V, Qs, P, gv, gq, gav, gaq), ref = _reference(B, N, T, d, 3, None, scale=6.0)
    assert float(ref["a_v"].max()) > 0.9
    out = AL.run(V, Qs, P, gv, gq, layout=layout, g_av=gav, g_aq=gaq)
    _report("saturated", layout, AL.check(out, ref))


@pytest.mark.parametrize("c_h", [(80.0, 80.0, 80.0), (-80.0, -80.0, -80.0), (80.0, -80.0, 80.0)], ids=["plus", "minus", "mixed"])
def test_large_score_biases(c_h):
    """c_h* = +-80: the softmax does not see the shift; the scores lose the bits below ulp(80)."""
    B, N, T, d = NUM
    (V, Qs, P, gv, gq, gav, gaq), ref = _reference(B, N, T, d, 3, None, c_h=c_h)
    out = AL.run(V, Qs, P, gv, gq, g_av=gav, g_aq=gaq)
    _report("c_h", str(c_h), AL.check(out, ref))


@pytest.mark.parametrize("layout", ["lm", "cm"])
def test_nan_stays_in_its_sample(layout):
    """One NaN in V[1, 2, 3] (forward only): sample 1's outputs are NaN exactly where the oracle's are, every other sample's
    outputs keep every bit of the clean run."""
    B, N, T, d = NUM
    V, Qs, P, _, _ = AL.case(B, N, T, d, seed=43)
    lens = _lens(B, T)
    clean = AL.run(V, Qs, P, layout=layout, lens=lens)
    Vn = V.clone()
    Vn[1, 2, 3] = float("nan")
    out = AL.run(Vn, Qs, P, layout=layout, lens=lens)
    with torch.no_grad():
        ref = dict(zip(("v", "q", "a_v", "a_q"), AL.forward(Vn, Qs, P, lens)))
    for k in ("v", "q", "a_v", "a_q"):
        assert torch.equal(torch.isnan(out[k][:, 1]), torch.isnan(ref[k][:, 1])), k
        assert bool(torch.isnan(ref[k][:, 1]).any()), k
        for b in (0, 2):
            assert torch.equal(out[k][:, b].contiguous().view(torch.int32), clean[k][:, b].contiguous().view(torch.int32)), (k, b)


# ---- g. refusals ---------------------------------------------------------------------------------------------------------
# Real buffers at (2, 7, 5, 64); one argument wrong per call.  Every check sits before the first launch of its entry point
# (alt_check, check_vlayout and the NULL / accumulate checks at the head of coattn_alt_forward / coattn_alt_backward), so
# no call below reaches a kernel: it returns < 0, names the argument and leaves every pre-filled buffer as it was.
RB, RN, RT, RD, RL = 2, 7, 5, 64, 3
FILL = 0x3FC00000 + 0x1234          # the bit pattern the buffers are pre-filled with


class _Refusal:
    def __init__(self):
        lib = _lib.load()
        B, N, T, d, L = RB, RN, RT, RD, RL
        V, Qs, P, gv, gq = AL.case(B, N, T, d, seed=47)
        self.V = V.float().to(DEV).contiguous()
        self.Q = [q.float().to(DEV).contiguous() for q in Qs]
        self.ps = [P[n].float().to(DEV).contiguous() for n in NAMES]
        sizes = _lib.alt_workspace_bytes(B, N, T, d, L)
        mk = lambda *shape: torch.zeros(*shape, device=DEV)
        self.saved, self.ws = mk(sizes[0] // 4), mk(max(sizes[1], sizes[2]) // 4)
        self.out = {"v_out": mk(L, B, d), "q_out": mk(L, B, d), "av_out": mk(L, B, N), "aq_out": mk(L, B, T)}
        self.gv, self.gq = gv.float().to(DEV).contiguous(), gq.float().to(DEV).contiguous()
        self.dV = mk(B, N, d)
        self.dQ = [mk(B, T, d) for _ in range(L)]
        self.grads = [torch.zeros_like(t) for t in self.ps]
        self.dims = dict(B=B, N=N, T=T, d=d, L=L, dtype=0, flags=0, stream=None)
        # a valid forward leaves the state the backward's refusals run against
        assert self.forward() == 0, lib.coattn_last_error()
        torch.cuda.synchronize()

    def params(self, null=None):
        return _lib.AltParams(*[None if i == null else t.data_ptr() for i, t in enumerate(self.ps)])

    def param_grads(self, null=None):
        return _lib.AltParamGrads(*[None if i == null else t.data_ptr() for i, t in enumerate(self.grads)])

    @staticmethod
    def table(tensors, null=None):
        return (C.c_void_p * len(tensors))(*[None if i == null else t.data_ptr() for i, t in enumerate(tensors)])

    def forward(self, **kw):
        a = dict(V=self.V, v_sB=RN * RD, v_sN=RD, v_sD=1, Q=self.table(self.Q), p=self.params(), saved=self.saved, ws=self.ws,
                 **self.out, **self.dims)
        a.update(kw)
        call = _lib.bind("coattn_alt_forward", **a)
        return call.fn(*call)

    def backward(self, **kw):
        a = dict(V=self.V, v_sB=RN * RD, v_sN=RD, v_sD=1, Q=self.table(self.Q), p=self.params(), saved=self.saved, gv=self.gv,
                 gq=self.gq, dV=self.dV, dv_sB=RN * RD, dv_sN=RD, dv_sD=1, dQ=self.table(self.dQ), pg=self.param_grads(),
                 accumulate=0, ws=self.ws, **self.dims)
        a.update(kw)
        call = _lib.bind("coattn_alt_backward", **a)
        return call.fn(*call)

    def written(self):
        return list(self.out.values()) + [self.saved, self.ws, self.dV] + self.dQ + self.grads


@pytest.fixture(scope="module")
def refusal():
    return _Refusal()


def _refused(r, fn, names, **kw):
    lib = _lib.load()
    torch.cuda.synchronize()
    for t in r.written():
        t.view(torch.int32).fill_(FILL)
    rc = fn(**kw)
    msg = lib.coattn_last_error()
    torch.cuda.synchronize()
    assert rc < 0, rc
    for n in names:
        assert n.encode() in msg, (n, msg)
    for t in r.written():
        assert bool((t.view(torch.int32) == FILL).all())


EXTENT = (RN - 1) * RD + (RD - 1)        # the last element of a location-major sample: sB must be larger


@pytest.mark.parametrize("kw,names", [
    (dict(V=None), ["coattn_alt_forward: V is NULL"]),
    (dict(v_out=None), ["coattn_alt_forward: v_out is NULL"]),
    (dict(q_out=None), ["coattn_alt_forward: q_out is NULL"]),
    (dict(ws=None), ["coattn_alt_forward: ws is NULL"]),
    (dict(Q=1), ["Q[1]"]),
    (dict(p=0), ["parameter 0 "]),
    (dict(p=7), ["parameter 7 "]),
    (dict(p=15), ["parameter 15 "]),
    (dict(v_sN=0), ["coattn_alt_forward: V", "sN=0"]),
    (dict(v_sD=-1), ["coattn_alt_forward: V", "sD=-1"]),
    (dict(v_sB=EXTENT), ["coattn_alt_forward: V", "sample stride %d" % EXTENT]),
    (dict(dtype=1), ["dtype 1"]),
], ids=["V", "v_out", "q_out", "ws", "Q1", "param0", "param7", "param15", "sN_0", "sD_negative", "sB_short", "dtype"])
def test_forward_refusals(refusal, kw, names):
    r = refusal
    if "Q" in kw:
        kw = dict(Q=r.table(r.Q, null=kw["Q"]))
    if "p" in kw:
        kw = dict(p=r.params(null=kw["p"]))
    _refused(r, r.forward, names, **kw)


@pytest.mark.parametrize("kw,names", [
    (dict(saved=None), ["coattn_alt_backward: saved is NULL"]),
    (dict(gv=None), ["coattn_alt_backward: gv is NULL"]),
    (dict(gq=None), ["coattn_alt_backward: gq is NULL"]),
    (dict(dQ=2), ["dQ[2]"]),
    (dict(pg=4), ["gradient 4 "]),
    (dict(accumulate=2), ["accumulate"]),
    (dict(dv_sN=0), ["coattn_alt_backward: dV", "sN=0"]),
    (dict(dv_sD=-1), ["coattn_alt_backward: dV", "sD=-1"]),
    (dict(dv_sB=EXTENT), ["coattn_alt_backward: dV", "sample stride %d" % EXTENT]),
], ids=["saved", "gv", "gq", "dQ2", "grad4", "accumulate", "dV_sN_0", "dV_sD_negative", "dV_sB_short"])
def test_backward_refusals(refusal, kw, names):
    r = refusal
    if "dQ" in kw:
        kw = dict(dQ=r.table(r.dQ, null=kw["dQ"]))
    if "pg" in kw:
        kw = dict(pg=r.param_grads(null=kw["pg"]))
    _refused(r, r.backward, names, **kw)


def test_bad_dv_strides_are_ignored_without_dv(refusal):
    """dV = NULL: its strides are not looked at, and the call computes everything else."""
    r = refusal
    assert r.forward() == 0
    assert r.backward(dV=None, dv_sB=EXTENT, dv_sN=0, dv_sD=-1) == 0, _lib.load().coattn_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(g).all()) for g in r.grads)


# ---- h. launch marks -----------------------------------------------------------------------------------------------------
# The marks of one forward and of one backward, recorded with the library of the commit before the host driver was split
# into AltCall and its named steps: the split must reproduce them.
FWD_MARKS = ["alt_projections", "alt_guided"]
BWD_MARKS = ["alt_guided_bwd", "alt_input_grads", "alt_param_grads"]


def profiled_marks(stateless):
    """The launch-group marks of run() between coattn_profile_begin / _end at (2, 3, 2, 64), L = 3, location-major: a
    forward with `saved` and its backward with dV, or (stateless) a forward without `saved`, then a forward + backward
    without dV."""
    lib = _lib.load()
    V, Qs, P, gv, gq = AL.case(2, 3, 2, 64, seed=5)
    torch.cuda.synchronize()
    _lib.check(lib.coattn_profile_begin(None), "coattn_profile_begin")
    if stateless:
        AL.run(V, Qs, P, infer=True)
    AL.run(V, Qs, P, gv, gq, need_dv=not stateless)
    us = (C.c_float * 48)()
    names = C.create_string_buffer(2048)
    n = lib.coattn_profile_end(us, names, 2048, 48)
    assert n >= 0, lib.coattn_last_error().decode()
    marks = names.value.decode().split("\n") if n else []
    assert len(marks) == n
    return marks


@pytest.mark.parametrize("stateless", [False, True], ids=["saved_dV", "stateless_no_dV"])
def test_launch_marks(stateless):
    assert profiled_marks(stateless) == (FWD_MARKS if stateless else []) + FWD_MARKS + BWD_MARKS

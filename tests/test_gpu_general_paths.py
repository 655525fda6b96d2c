"""GPU: every kernel of the parallel co-attention's general-shape path past the fused limits (csrc/api.hip
general_projections, general_attention, backward_general; csrc/small_kernels.hip; gemm_f32_vec_kernel and gemm_f32_kernel
through launch_gemm_f32; the grad_* jobs) against float64 autograd of oracle.coattn_oracle.coattn_forward, as
tests/test_gpu_attention_grad.py oracle() builds it (under the mask: the reference on the truncated questions); the bilinear
cases against tests/_bilinear.py forward_backward.

Bound: that of tests/test_gpu_fuzz.py (EXACT_TOL), max|err| / max|ref| <= 2e-5 per array -- a_v, a_q, v and q too: at
N = 4096 the largest a_v is 4.9e-4, and an absolute bound would let a row dropped from the softmax pass -- with dw_v.bias
and dw_q.bias (zero in exact arithmetic) as absolute errors on the fuzz's BIAS_SCALE.  No case needs a bound of its own.
Every case prints its worst error per output group before it asserts.

Which kernel a product, a reduction or a loop of a case reaches is stated by tests/_general.py paths(), the path's dispatch
rules restated in Python (tests/test_general_cpu.py pins them at every threshold); every row of the tables below names what
it is there to reach and is held against paths() when the module is collected.  The library's launch marks
(coattn_profile_begin / _end) are per phase, not per kernel -- on this path "wsplit", and "projections" only when both
projections ride one launch -- so the kernel a product took is asserted by paths(), not on the GPU; the marks themselves
are pinned by test_launch_marks.

Every run goes through tests/_general.py run(): `saved`, both workspaces, every output and every gradient are allocated at
exactly their size inside marker-filled arenas, NaN-filled; after the calls the margins hold the marker, a padded dV keeps
every cell outside its view, and no output cell is NaN.  Every case also runs twice (bit-identical), checks that a_v and a_q
sum to 1 and that a_q, C and dQ are exactly 0 past each clamped length, and -- in the maps families -- that coattn_infer(_len)
gives the maps of coattn_forward_maps(_len) bit for bit."""
import ctypes as C
import functools

import pytest
import torch

import vqa_amd
from oracle import coattn_oracle as O
from vqa_amd import _lib

from tests import _bilinear as BL
from tests import _general as G
from tests.test_gpu_attention_grad import oracle as grad_oracle
from tests.test_gpu_fuzz import BIAS_SCALE, EXACT_TOL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GEN, AUTO, FAST16, BIL = _lib.IMPL_GENERAL, _lib.IMPL_AUTO, _lib.FLAG_FAST16, _lib.FLAG_BILINEAR
TOL = EXACT_TOL
ABS = ("dw_v.bias", "dw_q.bias")
FWD = ("v", "q", "a_v", "a_q")

def _lens(B, T):
    return [min(max((1, T, T - 1, 3, T // 2)[b % 5], 1), T) for b in range(B)]


def _group(k):
    if k in FWD:
        return "fwd"
    if k in ("dV_phys", "dQ"):
        return k[:2]
    return "W" if k.endswith(".weight") and k[1] == "W" else "b_w"


@functools.lru_cache(maxsize=None)
def _case(shape, lens, junk, bil, maps):
    """Inputs seeded from the shape and their float64 reference, computed once per argument set (the layouts of a case share
    it; nothing changes it afterwards).  lens: None or a tuple; junk: the question rows past each length hold finite values
    instead of the pad tokens' zeros."""
    B, N, T, d, L = shape
    seed = B + 3 * N + 5 * T + 7 * d + 11 * L
    P = O.make_params(d, seed)
    V, Qs = O.make_inputs(B, N, T, d, seed + 10, lens=None if junk else lens, scale_q=(2.0 / d) ** 0.5, L=L)
    gv = torch.from_numpy(O.hash_normal((L, B, d), seed + 5)).float()
    gq = torch.from_numpy(O.hash_normal((L, B, d), seed + 6)).float()
    g_av = torch.from_numpy(O.hash_normal((L, B, N), seed + 7, 4.0)).float() if maps else None
    g_aq = torch.from_numpy(O.hash_normal((L, B, T), seed + 8, 4.0)).float() if maps else None
    ln = list(lens) if lens is not None else None
    if bil:
        ref = BL.forward_backward(V, Qs, P, gv, gq, True, ln, g_av, g_aq)
    else:
        ref = grad_oracle(V, Qs, P, ln, gv, gq, g_av if maps else torch.zeros(L, B, N), g_aq if maps else torch.zeros(L, B, T))
    return (V, Qs, P, gv, gq, g_av, g_aq), ref


def _errors(out, ref, keys):
    errs = {}
    for k in keys:
        r = ref[k].double().reshape(out[k].shape)
        errs[k] = float((out[k].double() - r).abs().max() / max(float(r.abs().max()), BIAS_SCALE if k in ABS else 1e-30))
    return errs


def _report(tag, ident, errs):
    worst = {}
    for k, e in errs.items():
        worst[_group(k)] = max(worst.get(_group(k), 0.0), e)
    print("general_paths %s %s" % (tag, ident), {g: "%.1e" % e for g, e in worst.items()})


def _same_bits(a, b, keys=None):
    for k in keys or a:
        if a[k] is None or b.get(k) is None:
            assert a[k] is None and b.get(k) is None, k
        else:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def _check(tag, shape, family, layout, flags=GEN, dv_layout="same", accumulate=0, lens=None, junk=None):
    B, N, T, d, L = shape
    masked = family in ("len", "maps_len")
    maps = family.startswith("maps")
    bil = bool(flags & BIL)
    if masked and lens is None:
        lens = _lens(B, T)
    if junk is None:                                          # pad rows: zeros on even cases, finite junk on odd ones
        junk = masked and (sum(shape) + G.LAYOUTS.index(layout)) % 2 == 1
    (V, Qs, P, gv, gq, g_av, g_aq), ref = _case(shape, tuple(lens) if masked else None, bool(junk and masked), bil, maps)
    names = G.NAMES + (G.BIL_NAMES if bil else ())
    init = None
    if accumulate:
        init = [torch.from_numpy(O.hash_normal(tuple(P[k].shape), 90 + i)).float() for i, k in enumerate(names)]
        ref = dict(ref)
        for i, k in enumerate(names):
            ref["d" + k] = ref["d" + k] + init[i].double()
    kw = dict(family=family, lens=lens if masked else None, gv=gv, gq=gq, g_av=g_av, g_aq=g_aq, layout=layout,
              dv_layout=dv_layout, flags=flags, accumulate=accumulate, grads_init=init)
    out = G.run(V, Qs, P, **kw)
    ident = "%s %s %s%s" % (shape, family, layout, "" if dv_layout == "same" else " dV=%s" % dv_layout)
    keys = [k for k in FWD + ("dV_phys", "dQ") + tuple("d" + n for n in names) if out[k] is not None]
    errs = _errors(out, ref, keys)
    _report(tag, ident, errs)
    bad = {k: e for k, e in errs.items() if not e <= TOL}
    assert not bad, (bad, errs)
    for k in ("a_v", "a_q"):
        assert float((out[k].double().sum(-1) - 1).abs().max()) <= 1e-5, k
    if masked:
        for b, n in enumerate(lens):
            n = min(max(n, 1), T)
            assert (out["a_q"][:, b, n:] == 0).all() and (out["C"][:, b, n:] == 0).all() and (out["dQ"][:, b, n:] == 0).all(), b
    _same_bits(out, G.run(V, Qs, P, **kw))                     # two runs are bit-identical
    if maps:
        inf = G.run(V, Qs, P, family="infer", lens=lens if masked else None, layout=layout, flags=flags)
        _same_bits(inf, out, FWD)
    return out


def _expect(shape, layout, want, flags=GEN, dv_layout="same"):
    """Collection-time check that a table row reaches what it names."""
    got = G.paths(*shape, layout, dv_layout, flags)
    for k, v in want.items():
        have = got
        for part in k.split("."):
            have = have[part]
        assert have == v, (shape, layout, k, have, v)


F128, F32S, VEC, VECX = ("f32_128", False), ("f32_32", False), ("vec128", False), ("vec128", True)

# (what the row reaches, shape (B, N, T, d, L), layouts, families, what paths() must say -- "@layout": for that layout only)
TABLE = [
    ("softmax_one_pass_N256_grid_of_image_size_512_v_w_alone", (2, 256, 29, 512, 3), ("cm", "lm"), ("plain", "len", "maps_len"),
     {"softmax": (1, 1), "v_w": True, "q_w": False, "wqT": False, "marks": ["wsplit"], "gemm.proj_q": F32S,
      "gemv.da_v@cm": ("icontig", 1), "gemv.v@lm": ("icontig", 2)}),
    ("softmax_two_passes_R257", (2, 257, 29, 100, 2), ("cm", "lm"), ("plain", "len", "maps_len"),
     {"softmax": (2, 1), "v_w": False, "q_w": False, "marks": [], "gemv.da_v@cm": ("icontig", 2), "gemm.proj_v@cm": F128,
      "gemm.proj_v@lm": VEC}),
    ("q_w_bitmap_and_WqT_image_with_T_over_28", (5, 256, 29, 256, 3), ("cm", "lm"), ("plain", "len"),
     {"v_w": True, "q_w": True, "wqT": True, "rowbits": True, "marks": ["wsplit", "projections"], "gemm.proj_q": None}),
    ("R4096_16_softmax_passes_gemv_I4096_ct_times_M4096_on_f32_128", (2, 4096, 5, 36, 3), ("cm", "lm", "strided"), ("plain", "maps"),
     {"softmax": (16, 1), "gemm.ct_times": F128, "gemv.da_v@cm": ("icontig", 16), "gemv.da_v@lm": ("kcontig", 1024),
      "gemv.da_v@strided": ("kcontig", 1024), "v_w@strided": False}),
    ("M4096_on_the_vec_kernel_with_xcd_group", (1, 4096, 8, 64, 1), ("cm", "lm"), ("plain",),
     {"gemm.ct_times": VECX, "softmax": (16, 1)}),
    ("T4096_on_the_question_side", (1, 7, 4096, 20, 1), ("cm",), ("plain", "len", "maps_len"),
     {"softmax": (1, 16), "gemm.affinity": F128, "gemm.c_times": F128, "gemm.dC": VECX, "gemv.da_q": ("kcontig", 1024),
      "splitk": (128, 32), "mask_rows": (112, False)}),
    ("mask_rows_past_its_grid_cap_T_over_128_on_the_vec_kernel", (2, 600, 600, 36, 1), ("cm", "lm"), ("len", "maps_len"),
     {"mask_rows": (1024, True), "gemm.affinity": VEC, "gemm.c_times": VEC, "gemm.dC": VEC, "gemm.dQ": VEC, "gemm.ct_times": VEC,
      "add": "add4"}),
    ("the_odd_twin_on_the_scalar_kernels", (2, 601, 599, 37, 1), ("cm", "lm"), ("len", "maps_len"),
     {"mask_rows": (1024, True), "gemm.affinity": F128, "gemm.c_times": F128, "gemm.dC": F128, "gemm.dQ": F128,
      "gemm.ct_times": F128, "add": "add1", "reduce.dW_v": ("reduce1", 2), "reduce.dw_v": ("reduce1", 38)}),
    ("T_between_64_and_128_on_f32_128", (2, 50, 100, 64, 2), ("cm", "lm"), ("plain", "len"),
     {"gemm.affinity": F128, "gemm.c_times": F128, "gemm.dC": F128, "gemm.dQ": F128}),
    ("three_sample_groups_the_last_short", (65, 130, 3, 20, 1), ("cm", "lm"), ("plain",),
     {"groups": (3, 22), "reduce.dW_v": ("reduce4", 22), "colsum.dw_v": (34, 249)}),
    ("d_odd_over_512_scalar_reduce_gemv_and_colsum_over_three_workgroups", (2, 70, 30, 513, 2), ("cm", "lm", "sd2"), ("plain",),
     {"reduce.dW_v": ("reduce1", 2), "reduce.dW_q": ("reduce1", 4), "reduce.dw_v": ("reduce1", 5), "colsum_blocks": 3,
      "gemv.q": ("icontig", 3), "gemv.v@lm": ("icontig", 3), "gemv.v@sd2": ("generic", 3), "gemv.da_v@sd2": ("generic", 1)}),
    ("d_mod4_not_mod32_N_over_1024", (3, 1025, 33, 260, 2), ("cm", "lm"), ("maps",),
     {"v_w": False, "q_w": False, "add": "add4", "softmax": (5, 1), "gemm.proj_v@lm": VEC, "gemm.proj_v@cm": F128,
      "gemv.da_v@cm": ("icontig", 5)}),
    ("L4_auto_dispatch_leaves_the_fused_path", (5, 49, 26, 256, 4), ("cm", "lm"), ("plain", "len"),
     {"fused": False, "q_w": True, "rowbits": True}),
    ("L8_on_gemm_w", (5, 49, 29, 256, 8), ("cm", "lm"), ("plain", "len"), {"q_w": True, "v_w@lm": True, "v_w@cm": False}),
    ("L8_on_the_general_gemm", (2, 20, 6, 36, 8), ("cm", "lm"), ("plain", "len"), {"q_w": False, "gemm.proj_q": F32S}),
]
ROW_FLAGS = {(5, 49, 26, 256, 4): AUTO}
# lengths of the T = 4096 row: 3 (the zero-fill of 4093 rows) and T - 1 (a masked softmax over all 16 passes)
ROW_LENS = {((1, 7, 4096, 20, 1), "len"): [3], ((1, 7, 4096, 20, 1), "maps_len"): [4095]}


def _for_layout(want, layout):
    out = {}
    for k, v in want.items():
        name, _, only = k.partition("@")
        if not only or only == layout:
            out[name] = v
    return out


def _table_params():
    ps = []
    for what, shape, layouts, families, want in TABLE:
        for layout in layouts:
            _expect(shape, layout, _for_layout(want, layout), ROW_FLAGS.get(shape, GEN))
            for family in families:
                ps.append(pytest.param(shape, family, layout, id="%s-B%d_N%d_T%d_d%d_L%d-%s-%s" % ((what,) + shape + (layout, family))))
    return ps


@pytest.mark.parametrize("shape,family,layout", _table_params())
def test_general_path(shape, family, layout):
    """(2, 4096, 5, 36, 3) maps, in all three layouts, is the regression case of gemm_f32_kernel<32>'s two accumulators: with
    one, dW_v.bias was off by 3.4e-5 of max|ref| and dW_v.weight by 2.3e-5 (LAB_NOTES.md section 13); now 5.7e-6 and 9.5e-6."""
    flags = ROW_FLAGS.get(shape, GEN)
    if flags == AUTO:
        assert not _lib.load().coattn_fused_supported(*shape, _lib.F32)
    _check("table", shape, family, layout, flags=flags, lens=ROW_LENS.get((shape, family)))


# ---- rpc > 32 with a short last chunk; sample groups 17 + 16 ----------------------------------------------------------------
GROUPS_SHAPE = (33, 257, 5, 100, 2)
for _layout in ("cm", "lm"):
    _expect(GROUPS_SHAPE, _layout, {"colsum.dw_v": (34, 250), "colsum.db_v": (34, 250), "groups": (2, 17),
                                    "reduce.dW_v": ("reduce4", 17), "reduce.dw_v": ("reduce4", 250), "reduce.dW_q": ("reduce4", 11)})


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("layout", ["cm", "lm"])
def test_colsum_chunks_and_sample_groups(layout, accumulate):
    """B N = 8481 rows: rpc = 34, 250 chunks, the last of 15 rows; B = 33: two sample groups of 17 and 16; the reductions'
    tails behind their groups of eight (250 = 31 x 8 + 2, 17 = 2 x 8 + 1, 11 = 8 + 3)."""
    _check("groups", GROUPS_SHAPE, "plain", layout, accumulate=accumulate)


# ---- dV in the other layout, in a padded view, and NULL ---------------------------------------------------------------------
DV_SHAPE = (2, 257, 29, 100, 2)


@pytest.mark.parametrize("layout,dv_layout", [("cm", "lm"), ("lm", "cm"), ("cm", "strided"), ("lm", "strided"), ("strided", "cm")])
def test_dv_in_its_own_layout(layout, dv_layout):
    """run()'s arena check is the assertion that no write lands in a padded dV's padding."""
    _check("dV", DV_SHAPE, "maps_len", layout, dv_layout=dv_layout)


@pytest.mark.parametrize("layout", ["cm", "lm"])
def test_null_dv_leaves_every_other_gradient_unchanged(layout):
    with_dv = _check("dV", DV_SHAPE, "len", layout)
    without = _check("dV", DV_SHAPE, "len", layout, dv_layout=None)
    assert without["dV_phys"] is None and with_dv["dV_phys"] is not None
    _same_bits(without, with_dv, [k for k in with_dv if k != "dV_phys"])


# ---- bilinear: proj_k on the general GEMM and on gemm_w, grad_bilinear_wb ---------------------------------------------------
BILINEAR = [((2, 257, 29, 100, 2), {"q_w": False, "gemm.proj_k": F32S, "marks": [], "colsum.db_b": (32, 4)}),
            ((5, 256, 29, 256, 3), {"q_w": True, "gemm.proj_k": None, "marks": ["wsplit", "projections", "bilinear_projection"]})]
for _shape, _want in BILINEAR:
    for _layout in ("cm", "lm"):
        _expect(_shape, _layout, _want, GEN | BIL)


@pytest.mark.parametrize("family", ["plain", "len"])
@pytest.mark.parametrize("layout", ["cm", "lm"])
@pytest.mark.parametrize("shape", [s for s, _ in BILINEAR], ids=["proj_k_general", "proj_k_gemm_w"])
def test_bilinear(shape, layout, family):
    _check("bilinear", shape, family, layout, flags=GEN | BIL)


# ---- flags ------------------------------------------------------------------------------------------------------------------
FLAG_SHAPES = [(2, 257, 29, 100, 2), (5, 256, 29, 256, 3), (2, 50, 100, 64, 2)]


def _run_flags(shape, layout, flags):
    B, N, T, d, L = shape
    lens = _lens(B, T)
    (V, Qs, P, gv, gq, g_av, g_aq), _ = _case(shape, tuple(lens), False, False, True)
    return G.run(V, Qs, P, family="maps_len", lens=lens, gv=gv, gq=gq, g_av=g_av, g_aq=g_aq, layout=layout, flags=flags)


@pytest.mark.parametrize("layout", ["cm", "lm"])
@pytest.mark.parametrize("shape", FLAG_SHAPES, ids=str)
def test_fast16_on_the_general_path_is_the_exact_arithmetic(shape, layout):
    """COATTN_FLAG_FAST16 | COATTN_IMPL_GENERAL: the general-shape path has one arithmetic -- the bits of flags =
    COATTN_IMPL_GENERAL."""
    _same_bits(_run_flags(shape, layout, GEN | FAST16), _run_flags(shape, layout, GEN))


@pytest.mark.parametrize("layout", ["cm", "lm", "strided"])
@pytest.mark.parametrize("shape", FLAG_SHAPES + [(5, 49, 26, 256, 4)], ids=str)
def test_auto_is_general_where_nothing_is_fused(shape, layout):
    assert not _lib.load().coattn_fused_supported(*shape, _lib.F32)
    _same_bits(_run_flags(shape, layout, AUTO), _run_flags(shape, layout, GEN))


def test_auto_leaves_the_fused_path_for_a_padded_view():
    """A fused shape in a layout the fused kernels do not take: COATTN_IMPL_AUTO runs the general path."""
    shape = (3, 49, 26, 256, 3)
    assert _lib.load().coattn_fused_supported(*shape, _lib.F32) and G.paths(*shape, "strided", flags=AUTO)["fused"] is False
    _same_bits(_run_flags(shape, "strided", AUTO), _run_flags(shape, "strided", GEN))


# ---- launch marks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,flags", [((5, 256, 29, 256, 3), GEN), ((2, 256, 29, 512, 3), GEN), ((2, 257, 29, 100, 2), GEN),
                                         ((5, 256, 29, 256, 3), GEN | BIL), ((5, 49, 26, 256, 4), AUTO)], ids=str)
def test_launch_marks(shape, flags):
    """The marks of one forward + backward on this path: "wsplit" when a weight image is written, "projections" only when
    both projections ride one launch, "bilinear_projection" when K runs on the pre-split-weight kernel; the backward of the
    general path records none."""
    lib = _lib.load()
    B, N, T, d, L = shape
    (V, Qs, P, gv, gq, _, _), _ = _case(shape, None, False, bool(flags & BIL), False)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _lib.check(lib.coattn_profile_begin(st), "coattn_profile_begin")
    G.run(V, Qs, P, family="plain", gv=gv, gq=gq, layout="lm", flags=flags)
    us = (C.c_float * 48)()
    names = C.create_string_buffer(2048)
    n = lib.coattn_profile_end(us, names, 2048, 48)
    assert n >= 0, lib.coattn_last_error()
    marks = names.value.decode().split("\n") if n else []
    want = G.paths(*shape, "lm", flags=flags)["marks"]
    assert marks == want and len(marks) == n, (marks, want)


# ---- the module at the 16 x 16 grid of a 512 x 512 image --------------------------------------------------------------------
@pytest.mark.parametrize("memory_format", ["contiguous", "channels_last"])
def test_module_on_a_16x16_grid_with_29_tokens(memory_format):
    """ParallelCoAttention(512) on encoder features [2, 512, 16, 16] (N = 256: past the fused kernels' 208), NCHW-contiguous
    (the permuted view: channel-major) and channels_last (location-major), with three question levels of 29 tokens:
    forward and autograd against the float64 oracle under the family's bound."""
    B, N, T, d, L = shape = (2, 256, 29, 512, 3)
    (V, Qs, P, gv, gq, _, _), ref = _case(shape, None, False, False, False)
    mod = vqa_amd.ParallelCoAttention(d)
    mod.load_state_dict(P)
    mod = mod.to(DEV)
    feats = V.reshape(B, d, 16, 16).to(DEV)
    if memory_format == "channels_last":
        feats = feats.contiguous(memory_format=torch.channels_last)
    feats.requires_grad_(True)
    x = feats.flatten(2).permute(0, 2, 1) if memory_format == "contiguous" else feats.permute(0, 2, 3, 1).reshape(B, N, d)
    assert tuple(x.stride()) == ((d * N, 1, N) if memory_format == "contiguous" else (N * d, d, 1))
    Qd = [q.to(DEV).requires_grad_(True) for q in Qs]
    vs, qs, a_v, a_q = mod(x, Qd, return_attention=True)
    (sum((vs[l] * gv[l].to(DEV)).sum() + (qs[l] * gq[l].to(DEV)).sum() for l in range(L))).backward()
    out = {"v": torch.stack(vs), "q": torch.stack(qs), "a_v": a_v, "a_q": a_q, "dV_phys": feats.grad.reshape(B, d, N),
           "dQ": torch.stack([q.grad for q in Qd])}
    mp = dict(mod.named_parameters())
    for k in G.NAMES:
        out["d" + k] = mp[k].grad
    out = {k: t.detach().cpu() for k, t in out.items()}
    errs = _errors(out, ref, list(out))
    _report("module", memory_format, errs)
    assert all(e <= TOL for e in errs.values()), errs
    assert mp["W_b.weight"].grad is None

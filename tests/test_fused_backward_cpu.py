"""The fused backward of the parallel co-attention without a GPU: tests/_fused_bwd.py bwd_path() -- the dispatch of
csrc/api.hip backward_impl, csrc/coattn_fused_bwd.hip decide_route / fused_backward and csrc/coattn_bwd32.hip restated in
Python -- pinned on both sides of every threshold it encodes and against the twenty mark lists that
tests/test_gpu_backward_routes.py recorded from a library that ran; the coverage of the table of
tests/test_gpu_fused_backward.py over everything that mirror can produce; the refusals the backward makes before any device
work; and two conditions on the float64 oracle that make the GPU rows' bounds meaningful: its own float32 evaluation stays
within half of every exact row's bound in every compared tensor, and tanh is unsaturated in every row."""
import ctypes as C
import itertools

import pytest
import torch

from vqa_amd import _lib

from tests import _fused as FU
from tests import _fused_bwd as FB
from tests import _general as G
from tests import test_fused_forward_cpu as FC
from tests import test_gpu_backward_routes as RT
from tests import test_gpu_fused_backward as GB

FAST, BF16, BIL = FU.FAST, FU.BF16, FU.BIL
PRE = ["bwd_pre", "bwd_dc32", "bwd_nat32"]


def path(B=8, N=49, T=26, d=512, L=3, layout="lm", flags=0, family="plain", **kw):
    return FB.bwd_path(B, N, T, d, L, layout, flags, family, **kw)


# ---- thresholds -----------------------------------------------------------------------------------------------------------------
def test_width_thresholds():
    """d % 512: four waves or two; the single-product forms of bwd_dc32 / bwd_nat32 exist on four waves only, the dA V kernel's
    on both; COATTN_FLAG_FAST16 is two bf16 pieces everywhere."""
    for d, NW in ((256, 2), (512, 4), (768, 2), (1024, 4), (3840, 2), (4096, 4)):
        p = path(d=d)
        assert p["dc32"][:3] == (2, NW, 3) and p["nat32"][:3] == (2, NW, 3) and p["group"] == (2, NW, True), d
    for d in (128, 384, 4352):
        assert not path(d=d)["fused"] and path(d=d, flags=FU.FUSED) == {"refused": True}
    assert path(flags=BF16)["dc32"][2] == 1 and path(flags=BF16)["nat32"][2] == 1 and path(flags=BF16)["dq"][3] == 1
    assert path(flags=BF16, d=256)["dc32"][2] == 3 and path(flags=BF16, d=768)["nat32"][2] == 3
    assert path(flags=BF16, d=256)["dq"] == ("x", 2, True, 1) and path(flags=BF16, d=768, N=196)["dq"] == ("32", 7, True, 1)
    for d in (256, 512):
        p = path(flags=FAST, d=d)
        assert p["dc32"][2] == p["nat32"][2] == p["dq"][3] == 2, d
        p = path(flags=FAST | FU.EXACT3, d=d)
        assert p["dc32"][2] == p["nat32"][2] == p["dq"][3] == 3, d
    assert path(flags=FAST | BF16)["dc32"][2] == 1 and path(flags=FAST | BF16, d=256)["dc32"][2] == 3
    assert path(flags=FAST, layout="lm_gap")["dc32"][2] == 2    # (the backward's width does not follow the forward's FP16 path)
    for family in FB.FAMILIES:
        assert path(flags=BF16 | BIL, family=family) == {"refused": True}


def test_tile_and_shape_thresholds():
    for N, NT in ((1, 2), (64, 2), (65, 7), (208, 7)):
        p = path(N=N)
        assert p["dc32"][0] == p["nat32"][0] == p["dq"][1] == NT and p["dq"][0] == ("x" if NT == 2 else "32"), N
    assert not path(N=209)["fused"] and path(N=209, flags=FU.FUSED) == {"refused": True}
    assert path(T=28)["fused"] and not path(T=29)["fused"] and path(T=29, flags=FU.FUSED) == {"refused": True}
    assert path(L=3)["fused"] and not path(L=4)["fused"] and path(L=4, flags=FU.FUSED) == {"refused": True}
    assert path(flags=FU.GENERAL) == {"refused": False, "fused": False, "marks": []}
    # the exact-f32 dA V kernel: channel-major rows off the 16-byte boundary only
    assert path(N=63, layout="cm")["dq"] == ("f32", 4, False, 3) and path(N=65, layout="cm")["dq"] == ("f32", 13, False, 3)
    assert path(N=64, layout="cm")["dq"] == ("x", 2, False, 3) and path(N=68, layout="cm")["dq"] == ("32", 7, False, 3)
    assert path(N=63)["dq"] == ("x", 2, True, 3) and path(N=65)["dq"] == ("32", 7, True, 3)


def test_families_select_mask_and_map_operands():
    for family in FB.FAMILIES:
        for gm in ("both", "av", "aq", None):
            p = path(family=family, gm=gm)
            maps = family.startswith("maps")
            g_av, g_aq = maps and gm in ("both", "av"), maps and gm in ("both", "aq")
            assert p["dc32"][3:] == (family.endswith("len"), g_av) and p["nat32"][4] == g_av and p["pre"][0] == g_aq, (family, gm)
            assert p["marks"] == path()["marks"]


def test_channel_major_row_alignment():
    """N % 4 for channel-major features: the bf16 dA V kernel and dW_v on the hand-scheduled kernel want rows of 16 bytes."""
    for N in (49, 50, 51):
        p = path(N=N, layout="cm")
        assert not p["dq32"] and not p["tn_v"] and not p["combine"] and p["marks"] == PRE + ["bwd_dq"], N
    p = path(N=52, layout="cm")
    assert p["dq32"] and p["tn_v"] and p["combine"] and p["use_dyn"] and p["marks"] == PRE + ["bwd_gemm", "bwd_dq"]
    assert path(N=52, layout="cm_gap")["tn_v"] and path(N=52, layout="cm_gap4")["tn_v"]
    # rows shorter than one k step of the weight-gradient kernel
    assert not path(N=12, layout="cm")["tn_v"] and path(N=12, layout="cm")["dq32"] and path(N=16, layout="cm")["tn_v"]
    assert path(N=12, layout="cm")["marks"] == PRE + ["bwd_gemm_dq_projection", "bwd_dq"]
    # location-major: any N; a gap behind the samples takes dW_v off the kernel
    assert path(N=49)["tn_v"] and not path(layout="lm_gap")["tn_v"] and not path(layout="lm_gap4")["tn_v"]
    assert path(layout="lm_gap")["marks"] == PRE + ["bwd_gemm_dq_projection", "bwd_dq"]
    # contraction lengths below one k step: B N and B T at 15 / 16
    assert not path(B=1, N=15)["tn_v"] and path(B=1, N=16)["tn_v"] and not path(B=1, T=15)["tn_q"] and path(B=1, T=16)["tn_q"]
    assert not path(q_aligned=False)["tn_q"] and path(q_aligned=False)["marks"] == PRE + ["bwd_gemm_dq_projection", "bwd_dq"]


def test_dq_projection_thresholds():
    """B T at 127 / 128: the dQ projection on the pre-split-weight kernel, inside the weight-gradient launch; B T at 255 / 256
    in the reduced-precision mode: on gemm_bf.hip, a launch of its own again."""
    own = PRE + ["bwd_gemm_dq_projection", "bwd_dq", "bwd_gemm_dw", "reduce_partials"]
    for B, T in ((127, 1), (9, 14), (4, 26)):
        p = path(B=B, T=T)
        assert not p["wdq"] and not p["combine"] and not p["use_dyn"] and not p["pre"][2] and p["marks"] == own, (B, T)
    for B, T in ((128, 1), (10, 14), (5, 26)):
        p = path(B=B, T=T)
        assert p["wdq"] and p["combine"] and p["red_in_dq"] and p["use_dyn"] and p["pre"][2], (B, T)
        assert p["marks"] == PRE + ["bwd_gemm", "bwd_dq"], (B, T)
    p = path(B=255, T=1, flags=BF16)
    assert p["combine"] and not p["wide"] and p["red_in_dq"] and p["marks"] == PRE + ["bwd_gemm", "bwd_dq"]
    p = path(B=256, T=1, flags=BF16)
    assert not p["combine"] and not p["red_in_dq"] and p["marks"] == own
    assert path(B=256, T=1)["combine"]                          # (the exact mode never leaves the shared launch)
    # bilinear: dQ from its own projection [dP_q | dK] [W_q; W_b]
    for B in (2, 8):
        p = path(B=B, flags=BIL)
        assert not p["combine"] and not p["use_dyn"]
        assert p["marks"] == PRE + ["bwd_dq", "bwd_bilinear_dq", "bwd_bilinear_dwb", "bwd_gemm_dw", "reduce_partials"]
    assert path(flags=BIL, layout="cm")["marks"] == PRE + ["bwd_dq", "bwd_bilinear_dq", "bwd_bilinear_dwb"]
    # dW_v and dW_q off 16 bytes: their partial sums leave the dQ kernel's launch
    p = path(grads_aligned=False)
    assert p["combine"] and not p["red_in_dq"] and not p["use_dyn"] and p["marks"] == PRE + ["bwd_gemm", "bwd_dq", "reduce_partials"]


def test_sum_in_gemm_and_bf16_stored_dp():
    """L = 3 and dV = NULL: the weight-gradient kernel adds the levels of dP_v itself; in the reduced-precision mode, on
    gemm_bf.hip throughout, bwd_nat32 then stores dP as bf16."""
    assert path(dv=False)["sum_in_gemm"] and not path(dv=True)["sum_in_gemm"] and not path(dv=False, L=2)["sum_in_gemm"]
    assert not path(dv=False, layout="lm_gap")["sum_in_gemm"] and path(dv=False, N=52, layout="cm")["sum_in_gemm"]
    dpb = dict(B=16, N=32, T=16, flags=BF16, dv=False)
    for N in (32, 96):
        p = path(**dict(dpb, N=N))
        assert p["dp_bf16"] and p["bf_tn"] and p["sum_in_gemm"] and p["nat32"] == (2 if N == 32 else 7, 4, 1, True, False), N
        assert p["marks"] == PRE + ["bwd_gemm_dq_projection", "bwd_dq", "bwd_gemm_dw", "reduce_partials"]
    assert path(**dict(dpb, d=1024))["dp_bf16"]
    for kw in (dict(dv=True), dict(L=2), dict(d=768), dict(d=256), dict(layout="cm"), dict(layout="lm_gap"), dict(flags=0),
               dict(flags=FAST), dict(q_aligned=False), dict(B=15), dict(N=33), dict(T=15), dict(T=17), dict(B=8)):
        p = path(**dict(dpb, **kw))
        assert not p["dp_bf16"] and not p["nat32"][3], kw
    # B T = 256 exactly (B = 8 T = 16 is 128: the projection is not on gemm_bf.hip); 255 cannot be a multiple of 32
    assert path(**dict(dpb, B=32, T=8))["dp_bf16"] and not path(**dict(dpb, B=28, T=8))["dp_bf16"]


def test_single_product_weight_gradient_route():
    """B N and B T at multiples of 32 (reduced-precision mode, location-major): both weight gradients on gemm_bf.hip."""
    bf = dict(B=16, N=32, T=16, flags=BF16)
    p = path(**bf)
    assert p["bf_tn"] and not p["wide"] and not p["red_in_dq"] and not p["combine"]
    # B T = 128 .. 224: the dQ projection is not on gemm_bf.hip, and that launch carries no dQ tiles: a launch of its own
    own = PRE + ["bwd_gemm_dq_projection", "bwd_dq", "bwd_gemm_dw", "reduce_partials"]
    for B in (8, 10, 12, 14):
        p = path(**dict(bf, B=B))
        assert p["bf_tn"] and p["wdq"] and not p["combine"] and not p["red_in_dq"] and p["marks"] == own, B
    assert path(**dict(bf, B=6))["bf_tn"] and not path(**dict(bf, B=6))["wdq"] and path(**dict(bf, B=6))["marks"] == own
    assert path(**dict(bf, B=9))["combine"] and path(**dict(bf, B=9))["marks"] == PRE + ["bwd_gemm", "bwd_dq"]
    for kw in (dict(N=33), dict(N=31), dict(T=15), dict(T=17), dict(B=15), dict(layout="cm"), dict(flags=0), dict(d=256, B=1)):
        assert not path(**dict(bf, **kw))["bf_tn"], kw
    assert path(**dict(bf, d=256))["bf_tn"] and path(**dict(bf, B=1, N=32, T=4))["bf_tn"] is False    # (K = 4 < 32)
    assert path(**dict(bf, B=2, N=16, T=16))["bf_tn"]                                    # K = 32: one step


def test_device_plan_limits():
    """use_dyn: the forward's bitmap of the live question rows (exact mode, P_q on gemm_w_kernel, d <= 1024), the wide
    weight-gradient kernel, the partial sums in the dQ kernel's launch, at most 8192 rows and 512 bitmap words."""
    assert path()["use_dyn"] and path()["pre"] == (False, "lm", True) and path(layout="cm", N=52)["pre"] == (False, "cm", True)
    assert path(d=1024)["use_dyn"] and path(d=256)["use_dyn"]
    for d in (1280, 2048):                                      # no bitmap past d = 1024
        p = path(d=d)
        assert not p["use_dyn"] and not p["pre"][2] and p["combine"] and p["wide"] and p["red_in_dq"], d
    for flags in (FAST, BF16):                                  # two FP16 pieces / one product: every row is computed
        assert not path(flags=flags)["use_dyn"] and not path(flags=flags)["pre"][2]
    assert path(flags=FAST)["wide"] and not path(flags=BF16)["wide"]
    # the tolerance mode without its FP16 path computes P_q exactly over the live rows: the plan is back
    assert path(flags=FAST, layout="cm", N=52)["pre"][2] is False and path(flags=FAST, layout="cm", N=196)["use_dyn"] is False
    p = path(flags=FAST, layout="cm", N=50)
    assert p["pre"][2] and not p["use_dyn"] and not p["tn_v"]
    assert not path(q_aligned=False)["pre"][2] and not path(B=4)["pre"][2]
    # the plan exists, the launch does not follow it: a gap behind the samples, bilinear, unaligned gradients
    for kw in (dict(layout="lm_gap"), dict(flags=BIL), dict(grads_aligned=False), dict(layout="cm")):
        p = path(**kw)
        assert p["pre"][2] and not p["use_dyn"], kw
    assert path(B=8192, T=1)["use_dyn"] and not path(B=8193, T=1)["use_dyn"] and path(B=8193, T=1)["pre"][2]
    assert path(B=16384, T=1)["pre"][2] and not path(B=16385, T=1)["pre"][2]
    assert path(B=512, T=16)["use_dyn"] and not path(B=513, T=16)["use_dyn"]


def test_v_alignment_is_part_of_the_fused_layout():
    for layout in ("lm", "cm"):
        assert path(layout=layout, v_aligned=False) == {"refused": False, "fused": False, "marks": []}
        assert path(layout=layout, v_aligned=False, flags=FU.FUSED) == {"refused": True}
        assert not path(layout=layout + "_gap1")["fused"] and path(layout=layout + "_gap1", flags=FU.FUSED)["refused"]
    assert not path(layout="strided")["fused"] and path(layout="strided", flags=FU.FUSED)["refused"]


# ---- the recorded mark lists ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RT.ROWS))
def test_mirror_reproduces_the_recorded_marks(name):
    """tests/test_gpu_backward_routes.py ROWS: literal mark lists of a forward + backward, recorded from the library."""
    B, N, d, L, layout, flags, opt, marks = RT.ROWS[name]
    family = {(False, False): "plain", (True, False): "len", (False, True): "maps", (True, True): "maps_len"}[
        (bool(opt.get("len")), bool(opt.get("maps")))]
    al = dict(q_aligned=not opt.get("q_off"))
    fwd = FU.fwd_path(B, N, RT.T, d, L, layout, flags, family, **al)
    bwd = FB.bwd_path(B, N, RT.T, d, L, layout, flags, family, dv=bool(opt.get("dv")), gm=opt.get("maps", "both"), **al)
    assert fwd["marks"] + bwd["marks"] == marks


def test_every_recorded_row_is_there():
    assert len(RT.ROWS) == 20


# ---- coverage ---------------------------------------------------------------------------------------------------------------------
def _domain():
    """Every tuple the mirror produces over the fused domain: every layout, width class, tile count and alignment, batch
    sizes on both sides of every row threshold, modes, entry points, map-gradient combinations, dV, Q alignment."""
    found = {k: set() for k in GB.KINDS}
    fams = [(f, gm) for f in FB.FAMILIES for gm in (("both", "av", "aq", None) if f.startswith("maps") else (None,))]
    for layout, d, N, (B, T), L, flags in itertools.product(
            FU.LAYOUTS + ("cm_gap4",), (256, 512, 1280, 2048, 4096), (1, 4, 32, 49, 52, 64, 65, 96, 100, 197, 208),
            ((1, 1), (8, 26), (9, 28), (16, 16), (32, 8), (10, 26)), (1, 3), GB.MODES.values()):
        for (family, gm), dv, qa in itertools.product(fams, (True, False), (True, False)):
            p = FB.bwd_path(B, N, T, d, L, layout, flags, family, dv=dv, q_aligned=qa, gm=gm)
            if not p["refused"]:
                found["dc32"].add((p["dc32"], p["group"][2]))
                for k in GB.KINDS[1:]:
                    found[k].add(p[k])
    return found


def test_table_reaches_every_reachable_tuple():
    want = _domain()
    reach = GB.reachable()
    got, _ = GB._hits(GB.ROWS)
    for k in GB.KINDS:
        assert want[k] == set(reach[k]), (k, sorted(want[k] ^ set(reach[k])))
        assert got[k] == want[k], (k, "unreached:", sorted(want[k] - got[k]))
    assert {k: len(v) for k, v in want.items()} == {"dc32": 80, "nat32": 24, "dq": 14, "pre": 8}
    assert len({t for t, _ in want["dc32"]}) == 40
    # none of the developer-switch forms
    assert all(not (kind == "32" and NT == 2) and (kind != "f32" or not LM) for kind, NT, LM, _ in want["dq"])
    assert len(GB.form_rows()) == 80


def test_table_has_every_axis_value_on_every_group():
    _, axes = GB._hits(GB.ROWS)
    assert len(axes) == 8
    for (NT, NW, LM), a in axes.items():
        assert a["N"] >= set(GB.N_AXIS[NT]) and a["T"] >= set(GB.T_AXIS) and a["L"] >= set(GB.L_AXIS), (NT, NW, LM)
        assert a["B"] >= set(GB.B_AXIS) and a["d"] >= set(GB.D_AXIS[NW]), (NT, NW, LM)
    hits = {n: p for n, (_, p) in GB.PATHS.items() if p["fused"]}
    groups = {}
    for n, p in hits.items():
        groups.setdefault(p["group"], []).append(GB.ROWS[n])
    for g, rows in groups.items():
        assert {r[7] for r in rows} == set(FB.FAMILIES), g
        assert any(r[6] & BIL for r in rows) and any(r[6] & BF16 for r in rows) and any(r[6] & FAST for r in rows), g
        lens = {x for r in rows if r[8] for x in r[8]}
        assert lens >= {0, 1, 4, 5} and any(r[8] and r[2] in r[8] and r[2] + 5 in r[8] for r in rows), (g, "lengths")
        assert {r[9].get("gm", "both") for r in rows if r[7].startswith("maps")} >= {"both", "av"}, g
        if not g[2] and g[0] == 2:
            assert {r[1] for r in rows} >= set(GB.CM_N)
    every = list(GB.ROWS.values())
    route = lambda key: {p[key] for p in hits.values()}         # noqa: E731
    for key in ("tn_v", "tn_q", "dq32", "wdq", "combine", "wide", "bf_tn", "red_in_dq", "use_dyn", "sum_in_gemm", "dp_bf16"):
        assert route(key) == {True, False}, key
    assert {r[5] for r in every} >= {"lm", "cm", "lm_gap", "lm_gap4", "cm_gap", "cm_gap4"}
    assert {r[5] for r in every if r[9].get("q_off")} == {"lm", "cm", "lm_gap", "cm_gap"}
    assert {(r[5][:2], bool(r[6] & BIL)) for r in every if r[9].get("acc")} >= {("lm", False), ("cm", False), ("lm", True)}
    assert sum(r[3] > 1024 for r in every) == 2 and {r[3] for r in every} >= {256, 512, 768, 1024, 2048, 4096}
    assert all(r[0] <= 3 for r in every if r[3] == 2048) and all(r[0] == 1 for r in every if r[3] == 4096)
    assert max(r[0] for r in every) == 16 and all(r[3] == 512 for r in every if r[0] > 9)
    # the smallest shapes with bf16-stored dP (and the single-product weight-gradient route beside them)
    dpb = {(r[0], r[1], r[2], r[3]) for n, r in GB.ROWS.items() if hits.get(n, {}).get("dp_bf16")}
    assert dpb == {(16, 32, 16, 512), (16, 96, 16, 512)}
    off = [(r, GB.PATHS[n][1]) for n, r in GB.ROWS.items() if r[9].get("v_off") or r[5].endswith("gap1")]
    assert len(off) == 2 and all(not p["fused"] and not p["refused"] and r[6] & 3 == FU.AUTO for r, p in off)


def test_piece_rows_are_the_four_exact_four_wave_forms():
    assert {GB.PATHS[n][1]["group"] for n in GB.PIECE_ROWS} == {(2, 4, True), (2, 4, False), (7, 4, True), (7, 4, False)}
    assert all(GB.ROWS[n][6] == 0 and GB.ROWS[n][2] in (16, 28) for n in GB.PIECE_ROWS)


# ---- refusals, before any device work -----------------------------------------------------------------------------------------------
BACKWARDS, OK_SHAPE = FC.BACKWARDS, FC.OK_SHAPE


def _st(shape=OK_SHAPE, layout="lm"):
    return G.layout_geometry(shape["B"], shape["N"], shape["d"], layout)[1]


@pytest.mark.parametrize("bad", [dict(d=128), dict(d=384), dict(d=4352), dict(T=29), dict(N=209), dict(N=256), dict(N=257), dict(L=4)],
                         ids=lambda b: "%s_%d" % next(iter(b.items())))
def test_a_fused_state_with_an_unsupported_shape_is_refused(bad):
    """COATTN_IMPL_FUSED says the state is the fused forward's: pick_impl refuses the shapes that forward cannot have written,
    ahead of backward_impl's and fused_backward's own shape checks (which nothing reaches: LAB_NOTES)."""
    h = FC._Host()
    shape = dict(OK_SHAPE, **bad)
    for family, symbol in zip(FB.FAMILIES, ("coattn_backward", "coattn_backward_len", "coattn_backward_maps", "coattn_backward_maps_len")):
        assert FB.bwd_path(*[shape[k] for k in "BNTdL"], "lm", FU.FUSED, family) == {"refused": True}
        for layout in ("lm", "cm"):
            rc, msg = h.call(symbol, shape, _st(shape, layout), FU.FUSED)
            assert rc == -1 and b"fused kernels do not support" in msg, (symbol, layout, rc, msg)


@pytest.mark.parametrize("layout", ("lm", "cm"))
def test_v_off_the_16_byte_boundary_is_refused_under_impl_fused(layout):
    h = FC._Host()
    sB, sN, sD = _st(layout=layout)
    assert FB.bwd_path(*[OK_SHAPE[k] for k in "BNTdL"], layout, FU.FUSED, "plain", v_aligned=False) == {"refused": True}
    for symbol in BACKWARDS:
        for off in (4, 8, 12):
            rc, msg = h.call(symbol, OK_SHAPE, (sB, sN, sD), FU.FUSED, V=h.at + off)
            assert rc == -1 and b"V and v_sB must be 16-byte aligned" in msg, (symbol, off, rc, msg)
        for gap in (1, 2, 3):
            rc, msg = h.call(symbol, OK_SHAPE, (sB + gap, sN, sD), FU.FUSED)
            assert rc == -1 and b"V and v_sB must be 16-byte aligned" in msg, (symbol, gap, rc, msg)


def test_null_arguments_bad_strides_and_bilinear_are_refused():
    h = FC._Host()
    st = _st()
    for symbol in BACKWARDS:
        for name in ("saved", "gv", "gq", "dQ", "pg", "ws", "Q", "p"):
            rc, msg = h.call(symbol, OK_SHAPE, st, 0, **{name: None})
            assert rc == -1 and b"backward: null argument" in msg, (symbol, name, rc, msg)
        rc, msg = h.call(symbol, OK_SHAPE, st, 0, dQ=(C.c_void_p * 8)(h.at, None, *[h.at] * 6))
        assert rc == -1 and b"Q[1]/dQ[1] is null" in msg, (symbol, rc, msg)
        for field in ("dW_v", "db_q", "dc_q"):
            pg = _lib.ParamGrads(*[h.at] * 10)
            setattr(pg, field, None)
            rc, msg = h.call(symbol, OK_SHAPE, st, 0, pg=pg)
            assert rc == -1 and b"null parameter-gradient pointer" in msg, (symbol, field, rc, msg)
        rc, msg = h.call(symbol, OK_SHAPE, (st[0], 0, st[2]), 0)
        assert rc == -1 and b"backward: V: strides must be positive" in msg, (symbol, rc, msg)
        rc, msg = h.call(symbol, OK_SHAPE, st, 0, dv_sB=st[0] - 1)
        assert rc == -1 and b"backward: dV: sample stride" in msg, (symbol, rc, msg)
        rc, msg = h.call(symbol, OK_SHAPE, (st[0] - 1, st[1], st[2]), 0, dV=None)      # dV = NULL: its strides are not read
        assert rc == -1 and b"backward: V: sample stride" in msg, (symbol, rc, msg)
        rc, msg = h.call(symbol, OK_SHAPE, st, BIL | BF16)
        assert rc == -1 and b"COATTN_FLAG_BILINEAR is not available" in msg, (symbol, rc, msg)
        pg = _lib.ParamGrads(*[h.at] * 8)                       # (dW_b, db_b left NULL)
        rc, msg = h.call(symbol, OK_SHAPE, st, BIL, pg=pg)
        assert rc == -1 and b"COATTN_FLAG_BILINEAR: null dW_b / db_b" in msg, (symbol, rc, msg)
        rc, msg = h.call(symbol, OK_SHAPE, st, BIL, p=_lib.Params(*[h.at] * 8))
        assert rc == -1 and b"COATTN_FLAG_BILINEAR: null W_b / b_b" in msg, (symbol, rc, msg)


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GB.ROWS))
def test_reference_conditions(name):
    """Attainable bound: the oracle's own float32 evaluation is within half the row's bound of its float64 evaluation in every
    compared tensor (rows of the exact mode).  Unsaturated tanh: at most 10 % of |C| exceeds 0.99, so an affinity error is not
    hidden (tests/test_fused_forward_cpu.py's condition)."""
    row = GB.ROWS[name]
    assert float((FU.row_reference(row)["C"].abs() > 0.99).double().mean()) <= 0.10
    if not row[6] & (FAST | BF16):
        ref = FB.case(row)[-1]
        errs = FB.errors(row, FB.case(row, dtype=torch.float32)[-1], ref)
        assert set(errs) == set(FB.compared(row))
        for k, e in errs.items():
            assert e < 0.5 * FU.bound(row[6]), (k, e)


@pytest.mark.parametrize("name", list(GB.PIECE_ROWS))
def test_piece_product_bounds_are_twice_the_float32_oracle_error(name):
    """The rows of test_gradients_keep_every_piece_product carry bounds of their own for dQ, dV, dW_v and dW_q: twice the error
    of the oracle's float32 evaluation (the literals within a quarter of it, whatever order this machine's BLAS adds in)."""
    row = GB.ROWS[name]
    errs = FB.errors(row, FB.case(row, dtype=torch.float32)[-1], FB.case(row)[-1])
    print(name, {k: "%.3e" % errs[k] for k in GB.PIECE_KEYS})
    assert set(GB.PIECE_ROWS[name]) <= set(GB.PIECE_KEYS)
    for k, b in GB.PIECE_ROWS[name].items():
        assert 0.8 <= b / (2 * errs[k]) <= 1.25, (name, k, errs[k])

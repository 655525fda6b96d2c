"""The fused forward of the parallel co-attention without a GPU: tests/_fused.py fwd_path() -- the dispatch of csrc/api.hip,
csrc/coattn_fused.hip and csrc/coattn_fwd32.hip restated in Python -- pinned on both sides of every threshold it encodes;
the coverage of the table of tests/test_gpu_fused_forward.py over everything that mirror can produce; the refusals the
library makes before any device work; and two conditions on the float64 oracle that make the GPU rows' bounds meaningful:
its own float32 evaluation stays within half of every exact row's bound, and tanh is unsaturated in every row."""
import ctypes as C

import pytest
import torch

from vqa_amd import _lib

from tests import _bilinear as BL
from tests import _fused as FU
from tests import _general as G
from tests import test_gpu_fused_forward as GF

FAST, BF16, BIL = FU.FAST, FU.BF16, FU.BIL


def path(B=8, N=49, T=26, d=512, L=3, layout="lm", flags=0, family="plain", **kw):
    return FU.fwd_path(B, N, T, d, L, layout, flags, family, **kw)


def tup(**kw):
    return path(**kw)["tuple"]


# ---- thresholds -----------------------------------------------------------------------------------------------------------------
def test_width_thresholds():
    assert tup(d=512)[1] == 4 and tup(d=1024)[1] == 4 and tup(d=256)[1] == 2 and tup(d=768)[1] == 2
    assert tup(d=4096)[1] == 4 and tup(d=3840)[1] == 2
    for d in (128, 384, 4352):                                  # d % 256, d > 4096: no fused shape
        assert not path(d=d)["fused"] and path(d=d, flags=FU.FUSED)["refused"]


def test_tile_and_shape_thresholds():
    assert tup(N=64)[0] == 2 and tup(N=65)[0] == 7 and tup(N=208)[0] == 7 and tup(N=1)[0] == 2
    assert not path(N=209)["fused"] and path(N=209, flags=FU.FUSED)["refused"]
    assert path(T=28)["fused"] and not path(T=29)["fused"] and path(T=29, flags=FU.FUSED)["refused"]
    assert path(L=3)["fused"] and not path(L=4)["fused"] and path(L=4, flags=FU.FUSED)["refused"]
    assert not path(flags=FU.GENERAL)["fused"]
    # the attended-feature pass behind the kernel
    assert path(N=64)["attend"] is None and path(N=65)["attend"] == "lm" and path(N=64, d=256)["attend"] == "lm"
    assert path(N=64, layout="cm")["attend"] == "cm4" and path(N=65, layout="cm")["attend"] == "cm13"


def test_projection_thresholds_and_marks():
    """B N and B T at 127 / 128: the exact projections run on the pre-split-weight kernel from 128 rows on (one launch when
    both do), and a kept state holds the image of W_q^T from B T = 128 on."""
    k = ["coattn_fwd32", "attend_v"]
    # N = 127 / 128 at B = 1, T = 1: P_v alone
    assert path(B=1, N=127, T=1)["marks"] == k and path(B=1, N=128, T=1)["marks"] == ["wsplit"] + k
    assert path(B=1, N=127, T=1)["proj"] == (False, False) and path(B=1, N=128, T=1)["proj"] == (True, False)
    # B T = 126 / 140 (T = 14): P_q and the W_q^T image; B N = 9 / 10 stays below
    assert path(B=9, N=1, T=14)["marks"] == ["coattn_fwd32"] and path(B=10, N=1, T=14)["marks"] == ["wsplit", "coattn_fwd32"]
    assert path(B=10, N=1, T=14)["proj"] == (False, True)
    assert path(B=10, N=1, T=14, family="infer")["marks"] == ["wsplit", "coattn_fwd32"]       # (P_q; no image without a state)
    # T = 127 / 128 cannot be fused (T <= 28): B T crosses at B = 5, T = 26 -- with B N = 245
    assert path(B=4)["marks"] == ["wsplit", "coattn_fwd32"] and path(B=4)["proj"] == (True, False)
    assert path(B=5)["marks"] == ["wsplit", "projections", "coattn_fwd32"]
    assert path(B=5, flags=BIL)["marks"] == ["wsplit", "projections", "bilinear_projection", "coattn_fwd32"]
    assert path(B=4, flags=BIL)["marks"] == ["wsplit", "coattn_fwd32"]
    assert path(B=5, family="attn")["marks"] == ["wsplit", "projections", "coattn_fwd32", "coattn_fwd32"]
    assert path(B=5, N=196, family="attn_len")["marks"] == ["wsplit", "projections"] + k + k
    # Q off the 16-byte boundary, a gap behind location-major samples, channel-major rows off it: off that kernel
    assert path(B=5, q_aligned=False)["proj"] == (True, False) and path(B=5, layout="lm_gap")["proj"] == (False, True)
    assert path(B=5, layout="cm")["proj"] == (False, True) and path(B=5, N=52, layout="cm")["proj"] == (True, True)
    assert path(B=5, N=52, layout="cm_gap")["proj"] == (True, True)
    assert path(B=5, N=50, layout="cm")["proj"] == (False, True) and path(B=5, N=51, layout="cm")["proj"] == (False, True)


def test_fp16_pieces_only_with_both_projections_on_the_range_checking_kernel():
    assert tup(flags=FAST)[3] == 4 and tup(flags=0)[3] == 3 and tup(flags=FAST | FU.EXACT3)[3] == 3
    # two FP16 pieces run on that kernel at any row count: B N = B T = 1
    assert path(B=1, N=1, T=1, flags=FAST)["f16"] and tup(B=1, N=1, T=1, flags=FAST)[3] == 4
    assert path(B=1, N=1, T=1, flags=FAST)["marks"] == ["wsplit", "projections", "coattn_fwd32"]
    # FAST16 without the FP16 path computes exactly: NP_ = 3
    for kw in (dict(q_aligned=False), dict(layout="lm_gap"), dict(layout="lm_gap4"), dict(layout="cm"), dict(layout="cm", N=50)):
        p = path(flags=FAST, **kw)
        assert p["fused"] and not p["f16"] and p["tuple"][3] == 3, kw
    assert tup(flags=FAST, layout="cm", N=52)[3] == 4 and tup(flags=FAST, layout="cm_gap", N=52)[3] == 4
    assert tup(flags=FAST, layout="cm", N=196, d=256)[3] == 4 and tup(flags=FAST | BIL, d=768)[3] == 4
    # the reduced-precision mode: one product at d % 512 == 0, the exact two-wave forms otherwise; never with BILINEAR
    assert tup(flags=BF16)[3] == 1 and tup(flags=BF16, d=1024, N=196)[3] == 1
    assert tup(flags=BF16, d=256)[3] == 3 and tup(flags=BF16, d=768, N=196)[3] == 3
    assert tup(flags=BF16 | FAST)[3] == 1 and tup(flags=BF16 | FAST, d=256)[3] == 3
    for family in FU.FAMILIES:
        assert path(flags=BF16 | BIL, family=family) == {"refused": True}
    assert tup(flags=BIL)[7] and not tup()[7]


def test_in_kernel_v_pass_and_map_copies():
    # FV only for location-major features, N <= 64, d % 512 == 0
    assert tup()[4] and tup(N=64)[4] and tup(d=1024)[4] and tup(d=4096)[4] and tup(layout="lm_gap")[4]
    assert not tup(N=65)[4] and not tup(d=256)[4] and not tup(d=768)[4] and not tup(layout="cm")[4]
    assert path()["marks"][-1] == "coattn_fwd32" and path(N=65)["marks"][-1] == "attend_v"
    # MAPS only for the maps families (coattn_infer writes the caller's buffers alone); MASK for every _len form
    for family in FU.FAMILIES:
        t = tup(family=family)
        assert t[6] == (family in ("maps", "maps_len")) and t[5] == family.endswith("len"), family


def test_v_alignment_is_part_of_the_fused_layout():
    for layout in ("lm", "cm"):
        assert not path(layout=layout, v_aligned=False)["fused"] and path(layout=layout, v_aligned=False, flags=FU.FUSED)["refused"]
        assert not path(layout=layout + "_gap1")["fused"] and path(layout=layout + "_gap1", flags=FU.FUSED)["refused"]
        assert path(layout=layout + "_gap")["fused"]
    assert path(layout="lm_gap4")["fused"] and not path(layout="strided")["fused"] and path(layout="strided", flags=FU.FUSED)["refused"]
    assert path(B=5, v_aligned=False)["marks"] == ["wsplit"]      # the general path: P_q alone on the pre-split-weight kernel


# ---- coverage ---------------------------------------------------------------------------------------------------------------------
def _domain():
    found = set()
    for layout in FU.LAYOUTS:
        for d in range(256, 4097, 256):
            for N in (1, 4, 49, 64, 65, 100, 208):
                for B, T in ((1, 1), (8, 26), (9, 28)):
                    for flags in GF.MODES.values():
                        for family in FU.FAMILIES:
                            for qa in (True, False):
                                found.add(FU.fwd_path(B, N, T, d, 3, layout, flags, family, q_aligned=qa)["tuple"])
    return found


def _hits():
    return {name: GF.mirror(row) for name, row in GF.ROWS.items()}


def test_table_reaches_every_reachable_tuple():
    want = _domain()
    assert want == set(GF.reachable())
    assert len(want) == 144
    # none of the developer-switch forms: NP_ = 2, and location-major NT = 2, NW = 4 without FV
    assert all(t[3] in (1, 3, 4) and (t[4] or not (t[2] and t[0] == 2 and t[1] == 4)) for t in want)
    got = {p["tuple"] for p in _hits().values() if p["fused"]}
    assert got == want, sorted(want - got)
    assert len(GF.form_rows()) == 144 and len(GF.ROWS) == 184


def test_table_reaches_the_attend_kernels_on_both_sides_of_their_branches():
    rows = [(GF.ROWS[n], p) for n, p in _hits().items() if p["fused"]]
    at = lambda kind, cond: any(p["attend"] == kind and cond(r[1]) for r, p in rows)      # noqa: E731
    assert at("lm", lambda N: N <= 128) and at("lm", lambda N: N > 128) and at("lm", lambda N: N == 128) and at("lm", lambda N: N == 129)
    for kind in ("cm4", "cm13"):
        assert at(kind, lambda N: N % 16 != 0) and at(kind, lambda N: N % 16 == 0), kind
    assert at(None, lambda N: N <= 32) and at(None, lambda N: N > 32)


def test_table_has_every_axis_value_on_every_group():
    groups = {}
    for name, p in _hits().items():
        if p["fused"]:
            groups.setdefault(p["tuple"][:3], []).append(GF.ROWS[name])
    assert len(groups) == 8
    for (NT, NW, LM), rows in groups.items():
        have = lambda i: {r[i] for r in rows}                   # noqa: E731
        assert have(1) >= set(GF.N_AXIS[NT]), (NT, NW, LM, "N")
        assert have(2) >= set(GF.T_AXIS) and have(4) >= set(GF.L_AXIS) and have(0) >= set(GF.B_AXIS), (NT, NW, LM)
        assert have(3) >= set(GF.D_AXIS[NW]) and have(6) >= set(GF.MODES.values()) and have(7) == set(FU.FAMILIES), (NT, NW, LM)
        if not LM and NT == 2:
            assert have(1) >= set(GF.CM_N)
        lens = {x for r in rows if r[8] for x in r[8]}
        assert lens >= {0, 1, 4, 5} and any(r[8] and r[2] in r[8] and r[2] + 5 in r[8] for r in rows), (NT, NW, LM, "lengths")
    every = list(GF.ROWS.values())
    assert {r[3] for r in every} >= {256, 512, 768, 1024, 2048, 4096}
    assert sum(r[3] == 4096 for r in every) == 2 and {r[5] for r in every if r[3] == 4096} == {"lm", "cm"}
    assert {r[5] for r in every} >= set(FU.LAYOUTS)
    assert {r[5] for r in every if r[9].get("q_off")} == {"lm", "cm", "lm_gap", "cm_gap"}
    # V off the 16-byte boundary, base and sample stride, both layouts: general-shape calls through COATTN_IMPL_AUTO
    off = [(r, GF.mirror(r)) for r in every if r[9].get("v_off") or r[5].endswith("gap1")]
    assert {(r[5], bool(r[9].get("v_off"))) for r, _ in off} == {("lm", True), ("cm", True), ("lm_gap1", False), ("cm_gap1", False)}
    assert all(not p["fused"] and not p["refused"] and r[6] & 3 == FU.AUTO for r, p in off)


def test_every_row_is_small():
    for name, (B, N, T, d, L, *_) in GF.ROWS.items():
        assert B <= 9 and B * N * d <= 9 * 208 * 1024, name


# ---- refusals, before any device work -----------------------------------------------------------------------------------------------
class _Host:
    """Host memory standing in for every pointer of a call that is refused before it reads one (pick_impl comes behind the
    NULL checks of the question table and the parameters, so those hold host addresses)."""

    def __init__(self):
        self.buf = (C.c_float * 4096)()
        self.at = (C.addressof(self.buf) + 15) & ~15              # 16-byte aligned
        self.table = (C.c_void_p * 8)(*[self.at] * 8)
        self.p = _lib.Params(*[self.at] * len(_lib.Params._fields_))
        self.pg = _lib.ParamGrads(*[self.at] * len(_lib.ParamGrads._fields_))

    def call(self, symbol, shape, strides, flags, V=None, **kw):
        names = [n for n, _ in _lib.SIGNATURES[symbol]]
        b = self.at
        a = dict(V=b if V is None else V, v_sB=strides[0], v_sN=strides[1], v_sD=strides[2], Q=self.table, p=self.p, ws=b,
                 dtype=_lib.F32, flags=flags, stream=None, **shape)
        a.update({n: b for n in ("saved", "av_out", "aq_out", "q_len", "v_out", "q_out", "gv", "gq", "dV") if n in names})
        if "dQ" in names:
            a.update(dQ=self.table, pg=self.pg, accumulate=0, dv_sB=strides[0], dv_sN=strides[1], dv_sD=strides[2])
        a.update(kw)
        call = _lib.bind(symbol, **a)
        return call.fn(*call), _lib.load().coattn_last_error()


FORWARDS = ("coattn_forward", "coattn_forward_len", "coattn_forward_maps", "coattn_forward_maps_len", "coattn_infer",
            "coattn_infer_len", "coattn_attention_forward", "coattn_attention_forward_len")
BACKWARDS = ("coattn_backward", "coattn_backward_len", "coattn_backward_maps", "coattn_backward_maps_len")
OK_SHAPE = dict(B=2, N=7, T=5, d=256, L=2)


def _strides(shape, layout):
    return G.layout_geometry(shape["B"], shape["N"], shape["d"], layout)[1]


@pytest.mark.parametrize("bad", [dict(d=128), dict(d=384), dict(d=4352), dict(T=29), dict(N=209), dict(L=4)],
                         ids=lambda b: "%s_%d" % next(iter(b.items())))
def test_impl_fused_refuses_an_unsupported_shape(bad):
    h = _Host()
    shape = dict(OK_SHAPE, **bad)
    assert FU.fwd_path(*[shape[k] for k in "BNTdL"], "lm", FU.FUSED, "plain") == {"refused": True}
    for symbol in FORWARDS + BACKWARDS:
        rc, msg = h.call(symbol, shape, _strides(shape, "lm"), FU.FUSED)
        assert rc == -1 and b"fused kernels do not support" in msg, (symbol, rc, msg)


def test_impl_fused_refuses_other_strides():
    h = _Host()
    for symbol in FORWARDS + BACKWARDS:
        for layout in ("strided", "sd2"):
            rc, msg = h.call(symbol, OK_SHAPE, _strides(OK_SHAPE, layout), FU.FUSED)
            assert rc == -1 and b"fused kernels do not support" in msg, (symbol, layout, rc, msg)


@pytest.mark.parametrize("layout", ("lm", "cm"))
def test_impl_fused_refuses_v_off_the_16_byte_boundary(layout):
    """include/coattn.h "Layouts": V and v_sB are 16-byte aligned on the fused kernels; the forward and the backward alike."""
    h = _Host()
    for symbol in FORWARDS + BACKWARDS:
        for off in (4, 8, 12):
            rc, msg = h.call(symbol, OK_SHAPE, _strides(OK_SHAPE, layout), FU.FUSED, V=h.at + off)
            assert rc == -1 and b"16-byte aligned" in msg, (symbol, off, rc, msg)
        for gap in (1, 2, 3):
            sB, sN, sD = _strides(OK_SHAPE, layout)
            rc, msg = h.call(symbol, OK_SHAPE, (sB + gap, sN, sD), FU.FUSED)
            assert rc == -1 and b"16-byte aligned" in msg, (symbol, gap, rc, msg)
        rc, msg = h.call(symbol, OK_SHAPE, _strides(OK_SHAPE, layout + "_gap1"), FU.FUSED)
        assert rc == -1 and b"16-byte aligned" in msg, (symbol, rc, msg)


def test_null_state_and_null_maps_are_refused():
    h = _Host()
    st = _strides(OK_SHAPE, "lm")
    for symbol in ("coattn_attention_forward", "coattn_attention_forward_len"):
        rc, msg = h.call(symbol, OK_SHAPE, st, 0, saved=None)
        assert rc == -1 and b"needs the saved buffer" in msg, (symbol, rc, msg)
    for symbol in ("coattn_forward_maps", "coattn_forward_maps_len"):
        for kw in (dict(av_out=None), dict(aq_out=None)):
            rc, msg = h.call(symbol, OK_SHAPE, st, 0, **kw)
            assert rc == -1 and b"null map buffer" in msg, (symbol, kw, rc, msg)
        rc, msg = h.call(symbol, OK_SHAPE, st, 0, saved=None)
        assert rc == -1 and b"null `saved`" in msg, (symbol, rc, msg)
    for symbol in FORWARDS:                                     # BILINEAR with BF16_PROJ: refused ahead of the dispatch
        rc, msg = h.call(symbol, OK_SHAPE, st, BIL | BF16)
        assert rc == -1 and b"COATTN_FLAG_BILINEAR is not available" in msg, (symbol, rc, msg)


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def test_reference_is_the_sample_by_sample_definition():
    B, N, T, d, L = 6, 9, 7, 256, 2
    lens = GF.mask_lens(B, T, 0)
    V, Qs = FU.inputs(B, N, T, d, L, lens)
    P = {k: v.double() for k, v in FU.params(d).items()}
    for bil in (False, True):
        for ln in (None, lens):
            a = FU.reference(V, Qs, P, bil, ln)
            b = BL.forward(V.double(), [q.double() for q in Qs], P, bil, ln)
            for k in ("v", "q", "a_v", "a_q"):
                assert float((a[k] - b[k]).abs().max()) < 1e-13, (bil, ln, k)
    masked = FU.reference(V, Qs, P, True, lens)
    for b, n in enumerate(lens):
        n = min(max(n, 1), T)
        assert bool((masked["C"][:, b, n:] == 0).all()) and bool((masked["a_q"][:, b, n:] == 0).all())


@pytest.mark.parametrize("name", list(GF.ROWS))
def test_reference_conditions(name):
    """Attainable bound: the oracle's own float32 evaluation is within half the row's bound of its float64 evaluation (rows
    of the exact mode).  Unsaturated tanh: at most 10 % of |C| exceeds 0.99, so an affinity error is not hidden."""
    row = GF.ROWS[name]
    ref = FU.row_reference(row)
    assert float((ref["C"].abs() > 0.99).double().mean()) <= 0.10
    if not row[6] & (FAST | BF16):
        errs = FU.errors(FU.row_reference(row, dtype=torch.float32), ref)
        for k, e in errs.items():
            assert e < 0.5 * FU.bound(row[6]), (k, e)


@pytest.mark.parametrize("name", list(GF.PIECE_ROWS))
def test_piece_product_bound_is_twice_the_float32_oracle_error(name):
    """The rows of test_affinity_keeps_every_piece_product carry a bound of their own for C: twice the error of the oracle's
    float32 evaluation (the literal within a quarter of it, whatever order this machine's BLAS adds in)."""
    row = GF.ROWS[name]
    assert row[6] == 0 and not row[7].startswith("infer")
    e = FU.errors(FU.row_reference(row, dtype=torch.float32), FU.row_reference(row))["C"]
    assert 0.8 <= GF.PIECE_ROWS[name] / (2 * e) <= 1.25, (name, e)

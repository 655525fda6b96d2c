"""The fused backward of the parallel co-attention, every code object a shipped build reaches and every edge of its tiles:
bwd_dc32_kernel<NT, NW, NP, MASK, GMAP>, bwd_nat32_kernel<NT, NW, NP, DPB, GMAP>, bwd_dq32x_kernel<2, LM, NP> and
bwd_dq32_kernel<7, LM, NP> (csrc/coattn_bwd32.hip), the exact-f32 bwd_dq_kernel<4 | 13, false, false>, bwd_pre_kernel and
bwd_pre_maps_kernel (csrc/coattn_fused_bwd.hip), through the raw C-ABI.  One table, ROWS, drives it: each row is one forward
+ backward with every buffer the calls write between marker words at its exact size, the backward's workspace included
(tests/_general.py run()), compared with the float64 oracle of tests/_bilinear.py forward_backward in v, q, a_v, a_q, dV, dQ
and every parameter gradient at the suite's bounds -- 2e-5 of max|.| under flags = 0, 1e-4 under COATTN_FLAG_FAST16, 8e-2
under COATTN_FLAG_BF16_PROJ; dc_v and dc_q, zero in exact arithmetic, as absolute errors.  The launch marks of both calls
must be those of the dispatch restated in Python (tests/_fused.py fwd_path(), tests/_fused_bwd.py bwd_path());
tests/test_fused_backward_cpu.py asserts without a GPU that the table reaches every template tuple the backward's mirror
can produce and every axis value on every (NT, NW, LM) group, that the oracle's own float32 evaluation stays within half of
each exact row's bound, and that tanh is unsaturated in every row.  Four rows also hold dQ, dV, dW_v and dW_q to twice that
float32 error: the one bound here that notices a partial product missing from the exact split.

The table is built by rule, not typed: form_rows() takes the reachable bwd_dc32 tuples in order, in both layouts, and gives
each one row, cycling N through the tile edges of its NT, T through 1 .. 28, L, B and d through their axes per (NT, NW, LM)
group; axis_rows() is written out -- the sample gaps, Q off the 16-byte boundary, the channel-major row alignments,
accumulate = 1, dV = NULL beside dV, d = 2048 and 4096, the bilinear affinity, the reduced-precision mode on the two-wave
forms and with bf16-stored dP, and V off the 16-byte boundary, which is a general-shape call under COATTN_IMPL_AUTO;
fill_rows() adds rows by rule until every bwd_nat32, dQ and pre-pass tuple and every axis value of every group is reached."""
import itertools

import pytest
import torch

from tests import _fused as FU
from tests import _fused_bwd as FB
from tests.test_gpu_fused_forward import B_AXIS, CM_N, D_AXIS, GROUPS, L_AXIS, MODES, N_AXIS, T_AXIS, mask_lens

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FAST, BF16, BIL = FU.FAST, FU.BF16, FU.BIL
MODE_NAME = {v: k for k, v in MODES.items()}
KINDS = ("dc32", "nat32", "dq", "pre")
# (family, gm): the four entry points, the maps families with both map gradients and with G_aq = NULL
CALLS = (("plain", None), ("len", None), ("maps", "both"), ("maps", "av"), ("maps_len", "both"), ("maps_len", "av"))


def reachable():
    """{kind: every template tuple bwd_path() produces over the shapes a row may take, in order}; "dc32" is paired with the
    layout, (tuple, LM): the table gives each bwd_dc32 form a row on both."""
    found = {k: set() for k in KINDS}
    for layout, d, N, (B, T), flags, (family, gm), dv, qa in itertools.product(
            ("lm", "cm"), (256, 512), (32, 49, 96, 197), ((8, 26), (16, 16)), MODES.values(), CALLS, (True, False), (True, False)):
        p = FB.bwd_path(B, N, T, d, 3, layout, flags, family, dv=dv, q_aligned=qa, gm=gm)
        if not p["refused"]:
            found["dc32"].add((p["dc32"], p["group"][2]))
            for k in KINDS[1:]:
                found[k].add(p[k])
    return {k: sorted(v) for k, v in found.items()}


def _name(row):
    B, N, T, d, L, layout, flags, family, _, opt = row
    return "%s%d_d%d_T%d_L%d_B%d_%s_%s%s%s" % (layout, N, d, T, L, B, family, MODE_NAME[flags],
                                               "_av" if opt.get("gm") == "av" else "", "" if opt.get("dv", 1) else "_nodv")


def form_rows():
    """One row per reachable (bwd_dc32 tuple, layout)."""
    rows, count = {}, {}
    for tup, LM in reachable()["dc32"]:
        NT, NW, NP, MASK, GMAP = tup
        g = (NT, NW, LM)
        i = count.get(g, 0)
        count[g] = i + 1
        flags = BF16 if NP == 1 else FAST if NP == 2 else 0
        family = (("maps_len" if GMAP else "len") if MASK else ("maps" if GMAP else "plain"))
        T, L, B, d = T_AXIS[(i + 3) % 7], L_AXIS[i % 3], B_AXIS[(i + 1) % 4], D_AXIS[NW][i % 2]     # (N = 1 not beside T = 1, B = 1)
        N = N_AXIS[NT][i % len(N_AXIS[NT])]
        opt = {"dv": 0 if i % 4 == 3 else 1}
        if GMAP:
            opt["gm"] = ("both", "av")[(i // 2) % 2]
        row = (B, N, T, d, L, "lm" if LM else "cm", flags, family, mask_lens(B, T, i) if MASK else None, opt)
        assert FB.mirror(row)[1]["dc32"] == tup and FB.mirror(row)[1]["group"] == g, (row, tup)
        assert _name(row) not in rows, _name(row)
        rows[_name(row)] = row
    return rows


def axis_rows():
    """The rows written out: (B, N, T, d, L, layout, flags, family, lens, options)."""
    ln = mask_lens
    rows = {
        # a gap behind every sample (64 floats; 4: the smallest the fused path takes), both layouts, both tile and wave counts:
        # behind a gap the location-major dW_v leaves the hand-scheduled kernels
        "gap_lm49": (8, 49, 26, 512, 3, "lm_gap", 0, "plain", None, {}),
        "gap4_lm33_d256": (9, 33, 17, 256, 2, "lm_gap4", 0, "len", ln(9, 17, 1), {}),
        "gap_lm196_d768": (7, 196, 26, 768, 3, "lm_gap", 0, "maps_len", ln(7, 26, 2), {}),
        "gap4_lm129_fast16": (8, 129, 16, 512, 3, "lm_gap4", FAST, "maps", None, {"gm": "av"}),
        "gap_cm49": (8, 49, 26, 512, 3, "cm_gap", 0, "plain", None, {}),
        "gap4_cm52": (8, 52, 26, 512, 3, "cm_gap4", 0, "maps", None, {}),
        "gap_cm196_d256": (7, 196, 28, 256, 3, "cm_gap", 0, "len", ln(7, 28, 3), {}),
        "gap4_cm96_d768_fast16": (9, 96, 16, 768, 2, "cm_gap4", FAST, "maps_len", ln(9, 16, 4), {}),
        "gap_cm97_bf16": (9, 97, 16, 1024, 2, "cm_gap", BF16, "plain", None, {}),
        # every Q_l four bytes off a 16-byte boundary: dW_q leaves the hand-scheduled kernel, P_q the pre-split-weight one
        "qoff_lm49": (8, 49, 26, 512, 3, "lm", 0, "plain", None, {"q_off": 1}),
        "qoff_cm196_fast16": (8, 196, 26, 512, 3, "cm", FAST, "maps", None, {"q_off": 1}),
        "qoff_lm_gap65_d256": (7, 65, 27, 256, 3, "lm_gap", 0, "len", ln(7, 27, 0), {"q_off": 1}),
        "qoff_cm_gap32_d768": (9, 32, 4, 768, 2, "cm_gap", 0, "maps_len", ln(9, 4, 1), {"q_off": 1, "gm": "av"}),
        # accumulate = 1: onto the partial sums in the dQ kernel's launch, onto the separate reductions, and bilinear
        "acc_lm49": (8, 49, 26, 512, 3, "lm", 0, "plain", None, {"acc": 1}),
        "acc_lm49_B2": (2, 49, 26, 512, 3, "lm", 0, "maps", None, {"acc": 1}),
        "acc_cm49": (8, 49, 26, 512, 3, "cm", 0, "len", ln(8, 26, 2), {"acc": 1}),
        "acc_cm100_d256_fast16": (7, 100, 27, 256, 2, "cm", FAST, "plain", None, {"acc": 1}),
        "acc_lm97_bil": (8, 97, 17, 512, 3, "lm", BIL, "plain", None, {"acc": 1}),
        # dV = NULL beside dV given at the same shape (L = 3: the weight-gradient kernel then adds the levels of dP_v itself)
        "lm49_B8_dv": (8, 49, 26, 512, 3, "lm", 0, "plain", None, {"dv": 1}),
        "lm49_B8_nodv": (8, 49, 26, 512, 3, "lm", 0, "plain", None, {"dv": 0}),
        "cm196_B5_d256_dv": (5, 196, 26, 256, 3, "cm", 0, "maps", None, {"dv": 1}),
        "cm196_B5_d256_nodv": (5, 196, 26, 256, 3, "cm", 0, "maps", None, {"dv": 0}),
        # d = 2048 and 4096 (the workspace is 40 d^2 floats: these two rows only)
        "lm49_d2048": (3, 49, 26, 2048, 3, "lm", 0, "maps_len", ln(3, 26, 4), {}),
        "cm196_d4096": (1, 196, 26, 4096, 2, "cm", 0, "plain", None, {}),
        # the reduced-precision mode on the two-wave forms: bwd_dc32 and bwd_nat32 at the exact width, the dA V kernel on one product
        "lm31_d256_bf16": (9, 31, 28, 256, 3, "lm", BF16, "plain", None, {}),
        "lm129_d768_bf16": (7, 129, 5, 768, 2, "lm", BF16, "maps_len", ln(7, 5, 2), {}),
        "cm64_d768_bf16": (8, 64, 17, 768, 3, "cm", BF16, "maps", None, {"gm": "av"}),
        "cm96_d256_bf16": (9, 96, 4, 256, 1, "cm", BF16, "len", ln(9, 4, 4), {"dv": 0}),
        # bf16-stored dP (reduced-precision mode, dV = NULL, L = 3, d % 512 == 0, location-major abutting samples, B N and B T
        # multiples of 32, B T >= 256): the smallest shapes that have it, on both tile counts, with and without G_av -- and the
        # single-product weight-gradient route of gemm_bf.hip with them
        "dpb_lm32": (16, 32, 16, 512, 3, "lm", BF16, "plain", None, {"dv": 0}),
        "dpb_lm96": (16, 96, 16, 512, 3, "lm", BF16, "len", ln(16, 16, 3), {"dv": 0}),
        "dpb_lm32_maps": (16, 32, 16, 512, 3, "lm", BF16, "maps_len", ln(16, 16, 1), {"dv": 0, "gm": "av"}),
        "dpb_lm96_maps": (16, 96, 16, 512, 3, "lm", BF16, "maps", None, {"dv": 0}),
        "dpb_lm32_dv_f32": (16, 32, 16, 512, 3, "lm", BF16, "plain", None, {"dv": 1}),       # beside them: dV keeps dP in fp32
        # the same route with the dQ projection off gemm_bf.hip (B T < 256)
        "bf_tn_lm32_B8": (8, 32, 16, 512, 3, "lm", BF16, "plain", None, {}),
        "bf_tn_lm96_B8": (8, 96, 16, 1024, 2, "lm", BF16, "maps_len", ln(8, 16, 2), {"dv": 0}),
        # V off the 16-byte boundary: a general-shape call under COATTN_IMPL_AUTO
        "voff_lm49_auto": (8, 49, 26, 512, 3, "lm", 0, "plain", None, {"v_off": 1}),
        "gap1_cm52_auto": (5, 52, 26, 512, 2, "cm_gap1", 0, "maps_len", ln(5, 26, 1), {}),
    }
    for N in CM_N:                                              # the row alignments mod 4, four waves and two
        rows["cm%d_rows" % N] = (8, N, 26, 512, 3, "cm", 0, "plain", None, {})
        rows["cm%d_rows_d256" % N] = (9, N, 17, 256, 3, "cm", 0, "maps_len", ln(9, 17, N), {})
    for i, (g, (layout, N, d)) in enumerate(GROUPS.items()):    # the bilinear affinity on each (NT, NW, LM) group
        family, gm = CALLS[i % 6]
        B, T = B_AXIS[(i + 1) % 4], T_AXIS[(i + 3) % 7]
        rows["bil_" + g] = (B, N, T, d, L_AXIS[(i + 2) % 3], layout, BIL | (FAST if i % 4 == 3 else 0), family,
                            ln(B, T, i) if family in FB.MASKED else None, {"gm": gm} if gm else {})
    # the piece-product rows (PIECE_ROWS): both layouts at NT = 2 and NT = 7, four waves, T = 28 and 16
    for layout in ("lm", "cm"):
        rows["piece_%s64" % layout] = (8, 64, 28, 512, 1, layout, 0, "plain", None, {})
        rows["piece_%s96" % layout] = (8, 96, 16, 512, 2, layout, 0, "len", ln(8, 16, 0), {})
    return rows


def _hits(rows):
    """(tuples reached per kind, {(NT, NW, LM): {axis: values}}) of a dict of rows."""
    got, axes = {k: set() for k in KINDS}, {}
    for row in rows.values():
        p = FB.mirror(row)[1]
        if p["refused"] or not p["fused"]:
            continue
        got["dc32"].add((p["dc32"], p["group"][2]))
        for k in KINDS[1:]:
            got[k].add(p[k])
        a = axes.setdefault(p["group"], {"N": set(), "T": set(), "L": set(), "B": set(), "d": set()})
        for k, v in zip("BNTdL", row[:5]):
            a[k].add(v)
    return got, axes


def fill_rows(rows):
    """Rows by rule until every reachable bwd_nat32, dQ and pre-pass tuple and every value of the N, T, L, B and d axes of
    every (NT, NW, LM) group is reached: for each thing missing, the first candidate of a fixed order whose mirror reaches it."""
    want = reachable()
    got, axes = _hits(rows)
    out = {}

    def add(row):
        assert _name(row) not in rows and _name(row) not in out, _name(row)
        out[_name(row)] = row
        g2, a2 = _hits({"": row})
        for k in KINDS:
            got[k] |= g2[k]
        for g, a in a2.items():
            for k, v in a.items():
                axes.setdefault(g, {x: set() for x in "NTLBd"})[k] |= v

    def candidates():
        shapes = [(B, T) for T in (26,) + T_AXIS[::-1] for B in B_AXIS[::-1]]
        for (B, T), layout, d, flags, (family, gm), dv in itertools.product(
                shapes, ("lm", "cm"), (512, 256), (0, FAST, BF16), CALLS, (1, 0)):
            for N in (49, 52, 196, 197) + N_AXIS[2] + N_AXIS[7]:
                yield (B, N, T, d, 3, layout, flags, family, mask_lens(B, T, N) if family in FB.MASKED else None,
                       dict({"dv": dv}, **({"gm": gm} if gm else {})))

    for kind in KINDS[1:]:
        for tup in want[kind]:
            if tup in got[kind]:
                continue
            for row in candidates():
                if _name(row) not in rows and _name(row) not in out and FB.mirror(row)[1][kind] == tup:
                    add(row)
                    break
            else:
                raise AssertionError((kind, tup))
    i = 0
    for NT, NW, LM in sorted(itertools.product((2, 7), (2, 4), (False, True))):
        full = {"N": N_AXIS[NT], "T": T_AXIS, "L": L_AXIS, "B": B_AXIS, "d": D_AXIS[NW]}
        for ax in "NTLBd":
            for v in full[ax]:
                if v in axes.get((NT, NW, LM), {}).get(ax, ()):
                    continue
                i += 1
                s = {"N": N_AXIS[NT][i % len(N_AXIS[NT])], "T": T_AXIS[i % 7], "L": L_AXIS[i % 3], "B": B_AXIS[i % 4],
                     "d": D_AXIS[NW][i % 2]}
                s[ax] = v
                family, gm = CALLS[i % 6]
                add((s["B"], s["N"], s["T"], s["d"], s["L"], "lm" if LM else "cm", 0, family,
                     mask_lens(s["B"], s["T"], i) if family in FB.MASKED else None, {"gm": gm} if gm else {}))
    return out


ROWS = dict(form_rows(), **axis_rows())
ROWS.update(fill_rows(ROWS))

# every row is held against the mirrors at collection: none is refused, the names say what they reach
PATHS = {name: FB.mirror(row) for name, row in ROWS.items()}
for _name_, (_f, _p) in PATHS.items():
    assert not _p["refused"] and not _f["refused"] and _p["fused"] == _f["fused"] == (not _name_.endswith("_auto")), _name_
    assert not _name_.startswith("dpb_") or _p["dp_bf16"] == (not _name_.endswith("f32")) and _p["bf_tn"], _name_
    assert ROWS[_name_][0] <= 16 and (ROWS[_name_][3] <= 1024 or _name_ in ("lm49_d2048", "cm196_d4096")), _name_


def reference(row):
    return FB.case(row, device=DEV)[-1]


def check_marks(out, paths):
    fwd, bwd = paths
    assert out["marks"] == fwd["marks"], (out["marks"], fwd["marks"])
    assert out["marks_bwd"] == bwd["marks"], (out["marks_bwd"], bwd["marks"])


@pytest.mark.parametrize("name", list(ROWS))
def test_row(name):
    row, paths = ROWS[name], PATHS[name]
    ref = reference(row)
    out = FB.run_row(row, device=DEV)
    errs = FB.errors(row, out, ref, out["init"])
    tol = FU.bound(row[6])
    print(name, {k: paths[1].get(k) for k in KINDS}, out["marks_bwd"], {k: "%.2f" % (e / tol) for k, e in errs.items()})
    check_marks(out, paths)
    assert set(errs) == set(FB.compared(row))
    assert (out["dV_phys"] is None) == (not row[9].get("dv", 1))
    for k, e in errs.items():
        assert e < tol, (k, e, tol)                             # (a NaN fails)


# ---- every piece product of the exact split ------------------------------------------------------------------------------------------
# One partial product missing from an exact contraction (mid x mid, 2^-16 of a term) moves its result by a few 1e-6 of max|.|:
# no row notices at the suite's 2e-5.  These rows hold dQ, dV, dW_v and dW_q to a bound of their own, twice the error of the
# oracle's own float32 evaluation on the same inputs (tests/test_fused_backward_cpu.py pins the literals to that figure).
PIECE_KEYS = ("dQ", "dV_phys", "dW_v.weight", "dW_q.weight")
PIECE_ROWS = {
    "piece_lm64": {"dQ": 1.0e-6, "dV_phys": 1.6e-6, "dW_v.weight": 1.6e-6, "dW_q.weight": 1.2e-6},
    "piece_cm64": {"dQ": 1.0e-6, "dV_phys": 1.6e-6, "dW_v.weight": 1.6e-6, "dW_q.weight": 1.2e-6},
    "piece_lm96": {"dQ": 7.8e-7, "dV_phys": 1.3e-6, "dW_v.weight": 1.6e-6, "dW_q.weight": 1.5e-6},
    "piece_cm96": {"dQ": 7.8e-7, "dV_phys": 1.3e-6, "dW_v.weight": 1.6e-6, "dW_q.weight": 1.5e-6},
}


@pytest.mark.parametrize("name", list(PIECE_ROWS))
def test_gradients_keep_every_piece_product(name):
    row = ROWS[name]
    errs = FB.errors(row, FB.run_row(row, profile=False), reference(row))
    print(name, {k: "%.2e of %.2e" % (errs[k], b) for k, b in PIECE_ROWS[name].items()})
    for k, b in PIECE_ROWS[name].items():
        assert errs[k] < b, (k, errs[k], b)


# ---- bit for bit ------------------------------------------------------------------------------------------------------------------
# one shape per (NT, NW, LM) group and mode: the forward file's GROUPS (N is no multiple of the tile), B = 3 (five empty pairs in
# the group of eight) and B = 9 (two groups)
BIT_MODES = ("exact", "fast16", "bf16", "bil")
GRADS = ("dV_phys", "dQ") + tuple("d" + k for k in FB.NAMES)
T_BITS = 17


def group_row(g, mode, B=3, family="plain", lens=None, **opt):
    layout, N, d = GROUPS[g]
    return (B, N, T_BITS, d, 3, layout, MODES[mode], family, lens, opt)


def same(a, b, what, keys=GRADS):
    for k in keys:
        if k in a or k in b:
            assert FU.bits_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("mode", BIT_MODES)
@pytest.mark.parametrize("g", list(GROUPS))
def test_repeats_entry_points_and_full_lengths_agree_bit_for_bit(g, mode):
    row = group_row(g, mode)
    B, N, T, d, L = row[:5]
    base = FB.run_row(row, profile=False)
    same(FB.run_row(row, profile=False), base, "a second call")
    # coattn_backward_maps without map gradients is coattn_backward (tests/test_gpu_attention_grad.py
    # test_backward_maps_without_map_gradients_is_the_plain_backward): NULL map gradients, and zero tensors
    same(FB.run_row(row, profile=False, family="maps", gm=None), base, "coattn_backward_maps, G_av = G_aq = NULL")
    same(FB.run_row(row, profile=False, family="maps", gm=None, g_av=torch.zeros(L, B, N), g_aq=torch.zeros(L, B, T)), base,
         "coattn_backward_maps, zero map gradients")
    V, Qs = FU.inputs(B, N, T, d, L)                            # the same inputs, now with lengths: all equal to T
    full = dict(V=V, Qs=Qs, profile=False, lens=[T] * B)
    same(FB.run_row(row, family="len", **full), base, "lengths all equal to T")
    maps = FB.run_row(row, profile=False, family="maps")
    same(FB.run_row(row, family="maps_len", **full), maps, "coattn_backward_maps_len, lengths T")


@pytest.mark.parametrize("mode", BIT_MODES)
@pytest.mark.parametrize("g", list(GROUPS))
def test_mask_ignores_pad_rows_and_pad_slots_and_zeroes_dq_beyond_the_length(g, mode):
    B, T = 9, T_BITS
    lens = mask_lens(B, T, 0)
    row = group_row(g, mode, B=B, family="maps_len", lens=lens)
    N, d = row[1], row[3]
    V, Qs = FU.inputs(B, N, T, d, 3, lens)
    base = FB.run_row(row, profile=False)
    g_aq = FB.upstream(row)[3].clone()
    junk = [q.clone() for q in Qs]
    for b, n in enumerate(lens):                                # the pad rows and pad slots filled with other finite values
        n = min(max(n, 1), T)
        g_aq[:, b, n:] = 3.0 + torch.arange(T - n, dtype=torch.float32)
        for l, q in enumerate(junk):
            q[b, n:] = 0.25 * (1 + l) * torch.cos(torch.arange((T - n) * d, dtype=torch.float32)).view(T - n, d)
    keys = GRADS + ("v", "q", "a_v", "a_q")
    same(FB.run_row(row, V=V, Qs=junk, profile=False), base, "pad rows of Q", keys)
    same(FB.run_row(row, profile=False, g_aq=g_aq), base, "pad slots of G_aq", keys)
    for b, n in enumerate(lens):
        n = min(max(n, 1), T)
        assert bool((base["dQ"][:, b, n:] == 0).all()), (b, n)
        assert bool((base["dQ"][:, b, :n] != 0).any())


@pytest.mark.parametrize("mode", BIT_MODES)
@pytest.mark.parametrize("g", list(GROUPS))
def test_samples_are_independent(g, mode):
    """Other finite values in V and Q of the middle sample of nine (two groups of eight) leave dV[b] and dQ[:, b] of the other
    eight bit-identical."""
    B, b0 = 9, 4
    row = group_row(g, mode, B=B, family="maps")
    V, Qs = FU.inputs(*row[:5])
    base = FB.run_row(row, profile=False)
    V2 = V.clone()
    V2[b0] = 0.75 * V[b0].flip(1)
    Q2 = [q.clone() for q in Qs]
    for q in Q2:
        q[b0] = -1.25 * q[b0]
    out = FB.run_row(row, V=V2, Qs=Q2, profile=False)
    others = [b for b in range(B) if b != b0]
    assert FU.bits_equal(out["dV_phys"][others], base["dV_phys"][others])
    assert FU.bits_equal(out["dQ"][:, others], base["dQ"][:, others])
    for k in ("v", "q", "a_v", "a_q"):
        assert FU.bits_equal(out[k][:, others], base[k][:, others]), k
    assert not FU.bits_equal(out["dV_phys"][b0], base["dV_phys"][b0]) and not FU.bits_equal(out["dQ"][:, b0], base["dQ"][:, b0])

"""The fused forward of the parallel co-attention, every code object a shipped build reaches and every edge of its tiles:
coattn_fwd32_kernel<NT, NW, LM, NP_, FV, MASK, MAPS, BIL> (csrc/coattn_fwd32.hip), attend_v_lm_kernel and attend_v_kernel<4>,
<13> (csrc/coattn_fused.hip), through the raw C-ABI.  One table, ROWS, drives it: each row is one forward-only call (the attn
families: coattn_forward then coattn_attention_forward on its state) with every buffer it writes between marker words
(tests/_general.py run()), compared with the float64 oracle of tests/_fused.py at the suite's bounds -- 2e-5 of max|.| under
flags = 0, 1e-4 under COATTN_FLAG_FAST16, 8e-2 under COATTN_FLAG_BF16_PROJ -- in v, q, a_v, a_q and, where a state is kept,
C; P_v, P_q and H_q of the state are stored in the kernels' own scaling and are not compared.  The launch marks of every
row must be those of tests/_fused.py fwd_path(), the dispatch restated in Python; tests/test_fused_forward_cpu.py asserts
without a GPU that the table reaches every template tuple that mirror can produce and every axis value on every
(NT, NW, LM) group, that the oracle's own float32 evaluation stays within half of each exact row's bound, and that tanh is
unsaturated in every row.  Four rows also hold C to twice that float32 error: the one bound here that notices a partial
product missing from the exact split.

The table is built by rule, not typed: form_rows() takes the reachable tuples in order and gives each one row, cycling N
through the tile edges of its NT, T through 1 .. 28, L, B and d through their axes per (NT, NW, LM) group; the rows behind it
are written out -- the sample gaps, Q off the 16-byte boundary, the channel-major row alignments, d = 2048 and 4096, the
tolerance mode where it falls back to exact arithmetic, and V off the 16-byte boundary, which is a general-shape call under
COATTN_IMPL_AUTO (include/coattn.h "Layouts")."""
import pytest
import torch

from tests import _fused as FU

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FAST, BF16, BIL = FU.FAST, FU.BF16, FU.BIL

N_AXIS = {2: (1, 31, 32, 33, 49, 63, 64), 7: (65, 96, 97, 128, 129, 193, 196, 207, 208)}
CM_N = (50, 51, 52)                     # channel-major rows at every alignment mod 4 (with 49)
T_AXIS = (1, 4, 5, 16, 17, 27, 28)
L_AXIS = (1, 2, 3)
B_AXIS = (1, 7, 8, 9)                   # a partly empty group of eight, a full one, two groups
D_AXIS = {2: (256, 768), 4: (512, 1024)}
MODES = {"exact": 0, "fast16": FAST, "bf16": BF16, "bil": BIL, "bil_fast16": BIL | FAST}


def mask_lens(B, T, i):
    """Lengths under the mask: 1, 4, 5, T and the values the kernels clamp, 0 and T + 5, starting at position i."""
    pat = (T, 1, 4, 5, 0, T + 5)
    return tuple(pat[(b + i) % 6] for b in range(B))


def reachable():
    """Every template tuple fwd_path() produces over the fused domain, in order."""
    found = set()
    for layout in FU.LAYOUTS:
        for d in (256, 512, 768, 1024):
            for N in (49, 52, 196):
                for flags in MODES.values():
                    for family in FU.FAMILIES:
                        for q_aligned in (True, False):
                            r = FU.fwd_path(8, N, 26, d, 3, layout, flags, family, q_aligned=q_aligned)
                            found.add(r["tuple"])
    return sorted(found)


def form_rows():
    """One row per reachable tuple."""
    rows, count = {}, {}
    for tup in reachable():
        NT, NW, LM, NP, FV, MASK, MAPS, BIL_ = tup
        g = (NT, NW, LM)
        i = count.get(g, 0)
        count[g] = i + 1
        flags = (BF16 if NP == 1 else FAST if NP == 4 else 0) | (BIL if BIL_ else 0)
        fams = (("maps_len",) if MAPS else ("len", "infer_len", "attn_len")) if MASK else \
               (("maps",) if MAPS else ("plain", "infer", "attn"))
        family = fams[i % len(fams)]
        layout = "lm" if LM else "cm"
        T, L, B, d = T_AXIS[i % 7], L_AXIS[i % 3], B_AXIS[i % 4], D_AXIS[NW][i % 2]
        ns = N_AXIS[NT]
        for k in range(len(ns)):                                # the next N of the cycle at which the mirror gives this form
            N = ns[(i + k) % len(ns)]                           # (two FP16 pieces from channel-major features: N % 4 == 0)
            if FU.fwd_path(B, N, T, d, L, layout, flags, family)["tuple"] == tup:
                break
        else:
            raise AssertionError(tup)
        lens = mask_lens(B, T, i) if MASK else None
        name = "%s%d_d%d_T%d_L%d_B%d_%s_%s" % (layout, N, d, T, L, B, family,
                                                {0: "exact", FAST: "fast16", BF16: "bf16", BIL: "bil", BIL | FAST: "bil_fast16"}[flags])
        assert name not in rows, name
        rows[name] = (B, N, T, d, L, layout, flags, family, lens, {})
    return rows


def axis_rows():
    """The rows written out: (B, N, T, d, L, layout, flags, family, lens, options)."""
    ln = mask_lens
    rows = {
        # a gap behind every sample (64 floats; 4: the smallest the fused path takes), in both tile counts and wave counts
        "gap_lm49": (8, 49, 26, 512, 3, "lm_gap", 0, "plain", None, {}),
        "gap_lm49_fast16_is_exact": (8, 49, 26, 512, 3, "lm_gap", FAST, "maps", None, {}),
        "gap4_lm33_d256": (9, 33, 17, 256, 2, "lm_gap4", 0, "len", ln(9, 17, 1), {}),
        "gap_lm196_d768": (7, 196, 26, 768, 3, "lm_gap", 0, "maps_len", ln(7, 26, 2), {}),
        "gap4_lm129": (3, 129, 5, 512, 1, "lm_gap4", BIL, "infer", None, {}),
        "gap_cm49": (8, 49, 26, 512, 3, "cm_gap", 0, "plain", None, {}),
        "gap_cm52_fast16": (8, 52, 26, 512, 3, "cm_gap", FAST, "maps", None, {}),
        "gap_cm196_d256": (7, 196, 28, 256, 3, "cm_gap", 0, "len", ln(7, 28, 3), {}),
        "gap_cm97_bf16": (9, 97, 16, 1024, 2, "cm_gap", BF16, "attn", None, {}),
        # Q_l four bytes off a 16-byte boundary (P_q leaves the pre-split-weight kernel; the tolerance mode computes exactly)
        "qoff_lm49": (8, 49, 26, 512, 3, "lm", 0, "plain", None, {"q_off": 1}),
        "qoff_cm196_fast16_is_exact": (8, 196, 26, 512, 3, "cm", FAST, "maps", None, {"q_off": 1}),
        "qoff_lm_gap65_d256": (7, 65, 27, 256, 3, "lm_gap", 0, "len", ln(7, 27, 0), {"q_off": 1}),
        "qoff_cm_gap32_bil": (9, 32, 4, 768, 2, "cm_gap", BIL, "infer", None, {"q_off": 1}),
        # d = 2048: four slices per wave, four sweeps of the in-kernel v pass and of q = a_q^T Q's tail loop; 4096: the limit
        "lm49_d2048": (8, 49, 26, 2048, 3, "lm", 0, "plain", None, {}),
        "lm49_d2048_fast16": (8, 49, 26, 2048, 3, "lm", FAST, "maps_len", ln(8, 26, 4), {}),
        "cm196_d2048": (3, 196, 26, 2048, 3, "cm", 0, "maps", None, {}),
        "lm208_d2048_bf16": (2, 208, 28, 2048, 3, "lm", BF16, "infer", None, {}),
        "lm49_d4096": (2, 49, 26, 4096, 3, "lm", 0, "plain", None, {}),
        "cm196_d4096": (1, 196, 26, 4096, 2, "cm", 0, "maps", None, {}),
        # the tolerance mode where the FP16 path is not available: channel-major rows that are no multiple of 16 bytes
        "cm49_fast16_is_exact": (8, 49, 26, 512, 3, "cm", FAST, "plain", None, {}),
        "cm193_bil_fast16_is_exact": (7, 193, 26, 768, 3, "cm", BIL | FAST, "maps", None, {}),
        # the reduced-precision mode on the two-wave forms, which have no single-product kernel: NP_ = 3 behind bf16 projections
        "lm31_d256_bf16": (9, 31, 28, 256, 3, "lm", BF16, "plain", None, {}),
        "lm129_d768_bf16": (7, 129, 5, 768, 2, "lm", BF16, "maps_len", ln(7, 5, 2), {}),
        "cm63_d768_bf16": (8, 63, 17, 768, 3, "cm", BF16, "infer", None, {}),
        "cm96_d256_bf16": (9, 96, 4, 256, 1, "cm", BF16, "attn_len", ln(9, 4, 4), {}),
        # two FP16 pieces at a batch of one (any row count runs on the range-checking projection kernel)
        "lm49_B1_fast16": (1, 49, 26, 512, 3, "lm", FAST, "plain", None, {}),
        "lm1_B1_T1_fast16": (1, 1, 1, 512, 1, "lm", FAST, "maps", None, {}),
        "cm196_B1_bil_fast16": (1, 196, 5, 256, 3, "cm", BIL | FAST, "len", ln(1, 5, 0), {}),
        # both projections in one launch and the image of W_q^T (B N, B T >= 128), and neither (B = 1)
        "lm49_B5_projections": (5, 49, 26, 512, 3, "lm", 0, "plain", None, {}),
        "lm49_B4_no_wqT": (4, 49, 26, 512, 3, "lm", 0, "plain", None, {}),
        # V off the 16-byte boundary: a general-shape call under COATTN_IMPL_AUTO
        "voff_lm49_auto": (8, 49, 26, 512, 3, "lm", 0, "plain", None, {"v_off": 1}),
        "voff_cm196_auto": (3, 196, 26, 256, 3, "cm", 0, "maps_len", ln(3, 26, 1), {"v_off": 1}),
        "gap1_lm49_auto": (8, 49, 26, 512, 3, "lm_gap1", 0, "maps", None, {}),
        "gap1_cm52_auto": (5, 52, 26, 512, 2, "cm_gap1", 0, "infer", None, {}),
    }
    for N in CM_N:                                              # the row alignments mod 4, four waves and two
        rows["cm%d_rows" % N] = (8, N, 26, 512, 3, "cm", 0, "plain", None, {})
        rows["cm%d_rows_d256" % N] = (9, N, 17, 256, 3, "cm", 0, "maps_len", ln(9, 17, N), {})
    return rows


ROWS = dict(form_rows(), **axis_rows())


def mirror(row):
    B, N, T, d, L, layout, flags, family, _, opt = row
    return FU.fwd_path(B, N, T, d, L, layout, flags, family, v_aligned=not opt.get("v_off"), q_aligned=not opt.get("q_off"))


# every row is held against the mirror at collection: none is refused, the names say what they reach
PATHS = {name: mirror(row) for name, row in ROWS.items()}
for _name, _p in PATHS.items():
    assert not _p["refused"] and _p["fused"] == (not _name.endswith("_auto")), _name
    assert not _name.endswith("is_exact") or (ROWS[_name][6] & FAST and not _p["f16"] and _p["tuple"][3] == 3), _name
    assert not _name.endswith("fast16") or (_p["f16"] and _p["tuple"][3] == 4), _name
    assert not _name.endswith("bf16") or _p["tuple"][3] == (1 if ROWS[_name][3] % 512 == 0 else 3), _name


def reference(row):
    return FU.row_reference(row, device=DEV)


@pytest.mark.parametrize("name", list(ROWS))
def test_row(name):
    row, path = ROWS[name], PATHS[name]
    out = FU.run_row(row)
    ref = reference(row)
    errs = FU.errors(out, ref)
    print(name, path.get("tuple"), out["marks"], {k: "%.2e" % e for k, e in errs.items()})
    assert out["marks"] == path["marks"], (out["marks"], path["marks"])
    assert set(errs) == ({"v", "q", "a_v", "a_q"} if row[7].startswith("infer") else {"v", "q", "a_v", "a_q", "C"})
    tol = FU.bound(row[6])
    for k, e in errs.items():
        assert e < tol, (k, e, tol)                             # (a NaN fails)
    if row[7].startswith("attn"):                               # coattn_attention_forward reproduces the forward on its state
        assert FU.bits_equal(out["v"], out["v_fwd"]) and FU.bits_equal(out["q"], out["q_fwd"])


# ---- the affinity's six piece products ---------------------------------------------------------------------------------------------
# One partial product missing from the exact split of phase 1 (mid x mid, 2^-16 of a term) moves C by about 5e-6 of max|C|: no
# row notices at the suite's 2e-5.  These rows hold C to a bound of their own, twice the error of the oracle's own float32
# evaluation on the same inputs (tests/test_fused_forward_cpu.py pins the literals to that; the kernel is at 0.5 .. 0.7 of it).
PIECE_ROWS = {"lm64_d512_T28_L1_B8_maps_exact": 2.0e-6, "cm64_d512_T28_L1_B8_maps_exact": 2.0e-6,
              "lm96_d512_T16_L2_B8_maps_len_exact": 2.2e-6, "cm96_d512_T16_L2_B8_maps_len_exact": 2.2e-6}


@pytest.mark.parametrize("name", list(PIECE_ROWS))
def test_affinity_keeps_every_piece_product(name):
    row = ROWS[name]
    err = FU.errors(FU.run_row(row, profile=False), reference(row))["C"]
    print(name, "C %.2e of %.2e" % (err, PIECE_ROWS[name]))
    assert err < PIECE_ROWS[name]


# ---- bit for bit ------------------------------------------------------------------------------------------------------------------
# one shape per (NT, NW, LM) group (FV is the (2, 4, lm) group) and mode; N is no multiple of the tile, B = 3 leaves five
# empty pairs in the group of eight
GROUPS = {"lm33_d512": ("lm", 33, 512), "lm33_d256": ("lm", 33, 256), "lm97_d512": ("lm", 97, 512), "lm97_d768": ("lm", 97, 768),
          "cm36_d512": ("cm", 36, 512), "cm36_d256": ("cm", 36, 256), "cm100_d512": ("cm", 100, 512), "cm100_d768": ("cm", 100, 768)}
BIT_MODES = ("exact", "fast16", "bf16", "bil")
KEYS = ("v", "q", "a_v", "a_q", "C")


def group_row(g, mode, B=3, family="plain", lens=None):
    layout, N, d = GROUPS[g]
    return (B, N, 17, d, 3, layout, MODES[mode], family, lens, {})


def same(a, b, keys, what):
    for k in keys:
        assert FU.bits_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("mode", BIT_MODES)
@pytest.mark.parametrize("g", list(GROUPS))
def test_families_layouts_and_repeats_agree_bit_for_bit(g, mode):
    row = group_row(g, mode)
    base = FU.run_row(row, profile=False)
    same(FU.run_row(row, profile=False), base, KEYS, "a second call")
    same(FU.run_row(row, profile=False, family="infer"), base, KEYS[:4], "coattn_infer")
    same(FU.run_row(row, profile=False, family="maps"), base, KEYS, "coattn_forward_maps")
    attn = FU.run_row(row, profile=False, family="attn")
    same(attn, base, KEYS, "coattn_attention_forward")
    same({"v": attn["v_fwd"], "q": attn["q_fwd"]}, base, KEYS[:2], "the forward before coattn_attention_forward")
    V, Qs = FU.inputs(*row[:5])                                 # the same inputs, now with lengths: all equal to T
    full = dict(V=V, Qs=Qs, profile=False, lens=[17] * 3)
    same(FU.run_row(row, family="len", **full), base, KEYS, "lengths all equal to T")
    same(FU.run_row(row, family="maps_len", **full), base, KEYS, "coattn_forward_maps_len, lengths T")
    same(FU.run_row(row, family="infer_len", **full), base, KEYS[:4], "coattn_infer_len, lengths T")
    # A gap behind the samples changes addresses only -- wherever the projections stay on the same kernels: behind a gap
    # the location-major P_v leaves the pre-split-weight kernel (api.hip projection_jobs), and with it the tolerance mode's
    # FP16 pieces; those calls are held against the oracle in test_row alone.
    gap = row[5] + "_gap"
    one = lambda lay, B: FU.fwd_path(B, row[1], row[2], row[3], row[4], lay, row[6], "plain")      # noqa: E731
    for B in (3, 1):
        a, b = one(row[5], B), one(gap, B)
        if (a["proj"], a["f16"], a["tuple"]) == (b["proj"], b["f16"], b["tuple"]):
            r1 = group_row(g, mode, B=B)
            same(FU.run_row(r1, profile=False, layout=gap), FU.run_row(r1, profile=False), KEYS, "a gap behind every sample")
            break


@pytest.mark.parametrize("mode", ("exact", "fast16"))
@pytest.mark.parametrize("g", list(GROUPS))
def test_mask_ignores_pad_rows_and_zeroes_beyond_the_length(g, mode):
    B, T = 9, 17
    lens = mask_lens(B, T, 0)
    row = group_row(g, mode, B=B, family="maps_len", lens=lens)
    V, Qs = FU.inputs(B, row[1], T, row[3], 3, lens)
    base = FU.run_row(row, profile=False)
    junk = []
    for l, q in enumerate(Qs):                                  # the pad rows filled with other finite values
        q = q.clone()
        for b, n in enumerate(lens):
            n = min(max(n, 1), T)
            q[b, n:] = 0.25 * (1 + l) * torch.cos(torch.arange((T - n) * q.shape[2], dtype=torch.float32)).view(T - n, q.shape[2])
        junk.append(q)
    same(FU.run_row(row, V=V, Qs=junk, profile=False), base, KEYS, "pad rows of Q")
    for b, n in enumerate(lens):
        n = min(max(n, 1), T)
        assert bool((base["a_q"][:, b, n:] == 0).all()) and bool((base["C"][:, b, n:] == 0).all()), (b, n)
        assert bool((base["a_q"][:, b, :n] > 0).all())


# ---- sample independence, and "inf / NaN inputs give inf / NaN outputs" ---------------------------------------------------------------
@pytest.mark.parametrize("mode", BIT_MODES)
@pytest.mark.parametrize("poison", ("nan", "inf"))
@pytest.mark.parametrize("layout", ("lm", "cm"))
def test_a_poisoned_sample_stays_alone(layout, poison, mode):
    """One NaN / +inf in V of the middle sample of nine (two groups of eight; N = 49: the padded columns of a channel-major
    tile read the next channel row).  Ordinary finite-sized arrays and range-checked reads: nothing here can fault."""
    B, N, T, d, b0, n0 = 9, 49, 26, 512, 4, 48
    row = (B, N, T, d, 3, layout, MODES[mode], "maps", None, {})
    V, Qs = FU.inputs(B, N, T, d, 3)
    clean = FU.run_row(row, profile=False)
    bad = V.clone()
    bad[b0, 300, n0] = float("nan") if poison == "nan" else float("inf")
    out = FU.run_row(row, V=bad, Qs=Qs, profile=False, allow_nan=True)
    others = [b for b in range(B) if b != b0]
    for k in KEYS:
        assert FU.bits_equal(out[k][:, others], clean[k][:, others]), k
    if mode == "exact":
        for k in ("v", "q", "a_v", "a_q"):
            assert not bool(torch.isfinite(out[k][:, b0]).any()), k
        assert not bool(torch.isfinite(out["C"][:, b0, :, n0]).any())

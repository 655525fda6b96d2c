"""GPU: every staging, tile and launch-form branch of csrc/head.hip (and the loss kernels of csrc/ce.hip behind it) through the
C-ABI runner of tests/_head.py, every buffer between guard bands that are asserted intact in every test.

Which branch a case reaches rests on these rules (head.hip; shapes are (B, d, mlp, K)):
  staging         whole 128-byte lines iff d % 32 == 0 and mlp % 32 == 0 and v[l], q[l], the four weights and `saved` (forward) /
                  `saved` and `ws` (backward) are 16-byte aligned; else a lane per element.  The logits layer's backward
                  (vec_h; BwdAll::vec0 in the one-launch form) also needs an added g_logits to have K % 4 == 0 and be aligned
  straddle        d % 32 != 0: the chunk / dW tile that holds the concatenation [q_l + v_l | h] boundary sums three loads per
                  element (the third branch of stage2 on a CompR, dw_tile MODE 2)
  chunks          a contraction of length L (d, 2 d, mlp or K) is ceil(L / 32) chunks dealt round-robin to eight waves; dx_tile takes
                  two per trip and leaves its loop from two places; dw_tile does the same over ceil(B / 32) row blocks
  one-launch form forward grid = min(256, most tiles of a layer), backward grid 256; barrier groups by blockIdx.x & 7

Bounds.  Error measure: max|err| / max|ref| per output tensor (tests/_head.py rel).
  exact mode   8 x e32 of the same case, capped at 1e-4.  e32 is the worst such error of the float32 CPU evaluation of the oracle
               modules against the float64 one (tests/test_head_cpu.py pins it below 2e-6): the reference arithmetic's own error;
               8 for the kernel's eight-way split of every contraction, the cross-wave sum order and the device tanhf / expf
               being a few ulp from the host's.
  bf16 mode    against tests/_head.py oracle_head_bf16 (the kernel's rounding points restated in float64): BF_BOUND, four times
               the worst error measured over this file's bf16 ids (LAB_NOTES section 10 has the table).  An operand within fp32
               rounding distance of a bf16 tie rounds the other way than the restatement's and moves one operand element by
               2^-9 of itself; the ids print how many did (`flips`), and the measured worst includes them.
  bit equality where two calls run the same tiles on the same values (misaligned against aligned, one-launch against per-layer,
               dq against dv, a reused `saved` against a fresh one)."""
import ctypes as C

import pytest
import torch

from oracle import coattn_oracle as O
from tests import _head as H

pytestmark = pytest.mark.gpu

CAP = 1e-4
# measured on one MI355X over the 40 bf16 ids of groups 1 and 2: worst 1.94e-4 (logits at (127, 32, 32, 5), 11 flipped operand
# elements: one flipped h_w element moves its row of z_p by ~1e-4, and a few of that row's 160 later operands then cross a bf16
# boundary too); 9.1e-5 and 1.3e-6 at the two other ids with a flip; <= 1.2e-5 at the 37 ids without one (14 flips in all)
BF_BOUND = 4 * 1.94e-4
EXACT, BF16, ONE = 0, H.BF16, H.PERSISTENT
MODE_NAME = {EXACT: "exact", BF16: "bf16", ONE: "one_launch"}

# (target, g_loss, with g_logits): the upstream-gradient variants
V_LOSS = ("hard", 1.7, False)
V_BOTH = ("hard", 0.5, True)
V_GX_AFTER_LABELS = ("hard", None, True)
V_GX_ONLY = (None, None, True)
UPSTREAM = {"g_loss": V_LOSS, "g_logits_after_labels": V_GX_AFTER_LABELS, "g_logits_no_labels": V_GX_ONLY, "both": V_BOTH}


def _sid(s):
    return "B%d_d%d_mlp%d_K%d" % s


# Input seeds.  At d = 1 the gradients are sums of B = 2 or 3 products, and at seed 0 (and 1, 3) those of dW_w cancel to a tenth of
# their terms: the float32 evaluation is then 2e-6 ... 1e-5 off -- the conditioning of that one element, not arithmetic.  Seed 2
# has no such cancellation at either d = 1 shape (e32 2e-7, as everywhere else), so the yardstick stays a yardstick there.
SEEDS = {(2, 1, 1, 2): 2, (3, 1, 32, 5): 2}


def _seed(shape):
    return SEEDS.get(shape, 0)


def _run(shape, var=V_LOSS, **kw):
    target, g_loss, gx = var
    seed = _seed(shape)
    P, v, q, _ = H.case(*shape, seed)
    return H.run_head(P, v, q, H.target_of(shape, target, seed), g_loss, H.upstream(shape[0], shape[3], seed) if gx else None, **kw)


def _al64(n):
    return (n + 63) & ~63


def _flips(res, ora, shape):
    """bf16 mode: how many MFMA operand elements the device rounds to another bf16 than the restatement (h_w, h_p, h_s from
    `saved`, dz_s, dz_p, dz_w from the backward's workspace: head.hip head_saved / head_bwd)"""
    B, d, mlp, K = shape
    n = 0
    sv, o = res["saved"].t, 0
    for h, w in zip(ora["h"], (d, d, mlp)):
        n += int((H.round_bf16(sv[o:o + B * w].cpu().double()) != H.round_bf16(h.reshape(-1))).sum())
        o += _al64(B * w)
    if res["ws"] is not None:
        ws, o = res["ws"].t, 0
        for dz, w in zip(ora["dz"][1:], (mlp, d, d)):
            n += int((H.round_bf16(ws[o:o + B * w].cpu().double()) != H.round_bf16(dz.reshape(-1))).sum())
            o += _al64(B * w)
    return n


def _intact(res):
    broken = [k for k, ok in res["intact"].items() if not ok]
    assert not broken, "stores outside: guard bands of %s overwritten" % broken


def _outputs(res, init=None):
    got = {k: res[k] for k in ("logits", "loss") + H.NAMES if res.get(k) is not None}
    if res["dv"] is not None:
        got["dv"] = torch.stack(res["dv"])
    if init is not None:
        for k in H.NAMES:
            got[k] = res[k].cpu().double() - init[k].double()
    return got


def _check(tag, res, shape, var=V_LOSS, flags=EXACT, init=None):
    """guard bands, every output finite, and every output within the mode's bound of its oracle"""
    seed = _seed(shape)
    _intact(res)
    got = _outputs(res, init)
    for k, t in got.items():
        assert torch.isfinite(t).all(), k
    if flags & BF16:
        ora = H.oracle_head_bf16(shape, *var, seed)
        bound, extra = BF_BOUND, " flips %d" % _flips(res, ora, shape)
    else:
        ora = H.oracle_head(shape, *var, seed)
        y = H.e32(shape, *var, seed)
        bound, extra = min(8 * y, CAP), " e32 %.2e" % y
    e = H.errors(got, ora)
    worst = max(e, key=e.get)
    print("head_paths %s %s %s worst %.2e (%s) bound %s%s" % (tag, _sid(shape), MODE_NAME[flags & ~ONE], e[worst], worst,
                                                             "%.2e" % bound if bound else "unset", extra),
          {k: "%.1e" % x for k, x in e.items()})
    assert bound is not None, "BF_BOUND is not set"
    assert e[worst] < bound, (worst, e[worst], bound)
    return e


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same_bits(r0, r1):
    for k in ("logits", "loss") + H.NAMES:
        assert (r0.get(k) is None) == (r1.get(k) is None), k
        if r0.get(k) is not None:
            assert _bits(r0[k], r1[k]), k
    for k in ("dv", "dq"):
        assert (r0[k] is None) == (r1[k] is None), k
        for l in range(3 if r0[k] is not None else 0):
            assert _bits(r0[k][l], r1[k][l]), (k, l)


# ---- 1. batch sweep: dw_tile's row-block loop (two blocks per trip, two exits; bf16: the other row-to-lane map) ----------
BATCHES = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 161)
G1 = [((B, 32, 32, 5), m) for B in BATCHES for m in (EXACT, BF16)] + \
     [((B, 20, 12, 5), m) for B in (32, 33, 64, 65, 97) for m in (EXACT, BF16)]

# ---- 2. contraction sweeps: chunks per wave 1, 2, 3, 4 and mixed, in layer 0's backward (K), the logits layer (mlp), the
# hidden layers (d, 2 d); ragged d: the straddling chunk first (20), later (48, 72, 100, 130), one column from either side (31, 33)
KS = (1, 31, 32, 33, 255, 256, 257, 288, 512, 513, 544, 768, 769, 800)
MLPS = (32, 224, 256, 288, 512, 544, 800, 36, 250, 260)
DS = (32, 64, 128, 160, 256, 288, 1, 20, 31, 33, 48, 72, 100, 130)
G2_SHAPES = [(3, 32, 32, 5)] + [(3, 32, 32, K) for K in KS] + [(3, 32, m, 5) for m in MLPS if m != 32] + [(3, d, 32, 5) for d in DS if d != 32] + \
            [(3, 64, 40, 5), (3, 48, 64, 5), (1, 1, 1, 1), (2, 1, 1, 2)]
# bf16: 1 chunk per wave (256), mixed 2 / 1 (288), 2 (512), mixed 3 / 2 (544), 3 (768), mixed 4 / 3 (800) and the ragged paths
G2_BF16 = [(3, 32, 32, K) for K in (33, 256, 288, 512, 544, 768, 800)] + [(3, 32, m, 5) for m in (256, 288, 544, 800, 36)] + \
          [(3, d, 32, 5) for d in (128, 160, 288, 20, 33, 72)] + [(3, 64, 40, 5), (2, 1, 1, 2)]
G2 = [(s, EXACT) for s in G2_SHAPES] + [(s, BF16) for s in G2_BF16]

G3_SHAPE, G3_SHAPE_K37 = (33, 64, 96, 36), (33, 64, 96, 37)
G4_SHAPES = [(37, 64, 128, 20), (5, 20, 12, 7)]
# every (shape, variant) whose e32 scales a bound in this file (tests/test_head_cpu.py pins them)
E32_CASES = sorted(set([(s, V_LOSS) for s, _ in G1 + G2] + [(s, v) for s in G4_SHAPES for v in UPSTREAM.values()] +
                       [(s, v) for s in (G3_SHAPE, G3_SHAPE_K37) for v in (V_GX_AFTER_LABELS, V_BOTH)]), key=str)


def _sweep_ids(cases):
    return [pytest.param(s, m, id="%s-%s" % (_sid(s), MODE_NAME[m])) for s, m in cases]


@pytest.mark.parametrize("shape,flags", _sweep_ids(G1))
def test_head_batch_sweep(shape, flags):
    """B from 1 to 161 across every exit of dw_tile's two-blocks-per-trip loop (B = 32 k, 32 k + 1, 64 k, 64 k + 1), on the
    whole-line path (32, 32, 5) and the per-element path with a straddle (20, 12, 5), in both arithmetic modes."""
    _check("batch", _run(shape, flags=flags, dq=("separate",) * 3), shape, flags=flags)


@pytest.mark.parametrize("shape,flags", _sweep_ids(G2))
def test_head_contraction_sweep(shape, flags):
    """K, mlp and d each across the chunk counts 1 ... 25 (8 / 9 / 16 / 17 / 24 / 25: one, two, three chunks per wave and the
    mixed distributions), unaligned mlp, ragged d with the concatenation boundary in the first, a later or the last chunk
    and with a single column on one side of it, mixed alignment (d % 32 == 0 with mlp % 32 != 0 and the reverse), d = 1."""
    _check("contraction", _run(shape, flags=flags), shape, flags=flags)


# ---- 3. staging selection -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operand", ["v1", "q2", "W_p", "W_h", "saved", "ws", "g_logits", "logits"])
def test_head_misaligned_operand_gives_the_aligned_bits(operand):
    """One operand one float off 16-byte alignment at a % 32 shape: the per-element path (for `g_logits`: in the logits layer's
    backward alone; `logits` is never staged: the loss kernel reads it) builds the same LDS image and issues the same MFMAs
    in the same order as the whole-line path, so every output has the aligned call's bits -- and those are within the exact
    bound of the oracle."""
    ref = _run(G3_SHAPE, V_BOTH)
    _check("staging_aligned", ref, G3_SHAPE, V_BOTH)
    res = _run(G3_SHAPE, V_BOTH, offsets={operand: 1})
    _intact(res)
    _same_bits(ref, res)


@pytest.mark.parametrize("var", [V_GX_AFTER_LABELS, V_BOTH], ids=["alone", "with_g_loss"])
@pytest.mark.parametrize("shape", [G3_SHAPE, G3_SHAPE_K37], ids=["K36_whole_lines", "K37_per_element_layer0"])
def test_head_added_logits_gradient_staging(shape, var):
    """g_logits aligned: K % 4 == 0 stages it in whole lines beside the padded d loss / d logits (row strides K and
    kpad(K)); K % 4 != 0 sends the logits layer's backward alone down the per-element path."""
    _check("g_logits", _run(shape, var), shape, var)


# ---- 4. upstream gradients x accumulate x input-gradient forms ----------------------------------------------------------------
FORMS = {"dq_none": dict(dq=None), "dq_separate": dict(dq=("separate",) * 3), "dq_alias_all": dict(dq=("alias",) * 3),
         "dq_alias_level0": dict(dq=("alias", "separate", "separate")), "dv_null": dict(want_dv=False)}


def _init_grads(ora, seed):
    """hash values scaled to half of each oracle gradient's max|g|: out - init keeps the sweep's bound"""
    return {k: torch.from_numpy(O.hash_unit(tuple(ora[k].shape), seed + i, 0.5 * ora[k].abs().max().item())).float()
            for i, k in enumerate(H.NAMES)}


def _variant(shape, up, acc, form, flags=EXACT):
    var = UPSTREAM[up]
    init = _init_grads(H.oracle_head(shape, *var, _seed(shape)), 900) if acc else None
    return _run(shape, var, flags=flags, accumulate=acc, grads_init=init, **FORMS[form]), var, init


def _check_forms(res, form):
    if form == "dv_null":
        assert res["dv"] is None and res["dq"] is None
    elif form == "dq_none":
        assert res["dq"] is None
    else:
        for l, m in enumerate(FORMS[form]["dq"]):
            if m == "alias":
                assert res["dq"][l].data_ptr() == res["dv"][l].data_ptr()   # (stored once; its values are checked as dv)
            else:
                assert _bits(res["dq"][l], res["dv"][l]), l


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("acc", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("up", list(UPSTREAM))
@pytest.mark.parametrize("shape", G4_SHAPES, ids=_sid)
def test_head_upstream_accumulate_forms(shape, up, acc, form):
    """Every combination against the oracle: g_loss / g_logits (after a forward with and without a loss) / both; accumulate
    onto gradients of the oracle gradients' own magnitude (NaN-filled buffers otherwise); dq absent, separate (the bits of
    dv), the same pointer as dv at every level or at level 0 only; dv = NULL (parameter gradients only)."""
    res, var, init = _variant(shape, up, acc, form)
    _check("forms-%s-%d-%s" % (up, acc, form), res, shape, var, init=init)
    _check_forms(res, form)


# ---- 5. the one-launch form -----------------------------------------------------------------------------------------------
def _one_launch_pair(shape, var=V_LOSS, **kw):
    a, b = _run(shape, var, **kw), _run(shape, var, flags=ONE, **kw)
    _intact(a)
    _intact(b)
    for t in _outputs(b).values():                               # (a barrier time-out shows as NaN in the first output element)
        assert torch.isfinite(t).all()
    _same_bits(a, b)
    return b


@pytest.mark.parametrize("shape", [(3, 32, 32, 5), (3, 32, 64, 5), (3, 32, 224, 5), (3, 32, 256, 5), (3, 32, 288, 5),
                                   (33, 32, 32, 4128)], ids=_sid)
def test_one_launch_grids(shape):
    """Forward grids of 1, 2, 7, 8 and 9 workgroups (the two-level barrier with 1, 2, 7, 8 groups and with a second member in
    group 0), and 258 tiles on the 256-workgroup grid: the per-layer launches' bits."""
    _one_launch_pair(shape)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("acc", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("up", list(UPSTREAM))
def test_one_launch_upstream_accumulate_forms(up, acc, form):
    """Group 4's variants at (37, 64, 128, 20) with flags = 1: bit for bit the per-layer launches (dv = NULL moves the
    time-out's poison target to dW_w and gives the last phase no dX tiles)."""
    shape = G4_SHAPES[0]
    a, var, _ = _variant(shape, up, acc, form)
    b, _, _ = _variant(shape, up, acc, form, flags=ONE)
    _intact(b)
    for t in _outputs(b).values():
        assert torch.isfinite(t).all()
    _same_bits(a, b)
    _check_forms(b, form)


@pytest.mark.parametrize("case", ["misaligned_v1", "misaligned_ws", "K37_g_logits", "soft_ce", "bce", "per_element_straddle"])
def test_one_launch_other_paths(case):
    kw = {"misaligned_v1": dict(shape=G3_SHAPE, var=V_BOTH, offsets={"v1": 1}),
          "misaligned_ws": dict(shape=G3_SHAPE, var=V_BOTH, offsets={"ws": 1}),
          "K37_g_logits": dict(shape=G3_SHAPE_K37, var=V_BOTH),                # BwdAll::vec0 = false at a % 32 shape
          "soft_ce": dict(shape=G3_SHAPE, var=("soft_ce", 1.7, False)),
          "bce": dict(shape=G3_SHAPE, var=("bce", 1.7, True)),
          "per_element_straddle": dict(shape=(65, 20, 12, 7), var=V_LOSS)}[case]
    _one_launch_pair(**kw)


# ---- 6. `saved` reuse and the status word -----------------------------------------------------------------------------------
def _bad_target(tgt, row, K):
    if tgt[0] == "hard":
        lab = tgt[1].clone()
        lab[row] = K
        return ("hard", lab)
    idx = tgt[1].clone()
    idx[row, 1] = K
    return (tgt[0], idx, tgt[2])


@pytest.mark.parametrize("flags", [EXACT, ONE], ids=["per_layer", "one_launch"])
@pytest.mark.parametrize("kind", ["hard", "soft_ce", "bce"])
def test_head_saved_reuse_and_status(kind, flags):
    """ONE `saved` buffer through five forwards, as HotPathGraph's static buffers see them.  The logits layer's workgroup 0
    (per-layer) or a memset (one-launch form) clears the loss's status word and ticket in front of every loss: a bad label
    (== K) gives a NaN loss and coattn_head_status -2 naming the row; the next good call on the same buffer reports 0 and has
    the bits of a fresh-buffer call in logits, loss and every gradient; the bad one again -2.
    A logits-only forward (labels NULL) runs no loss and clears nothing: coattn_head_status keeps reporting the last
    forward that had a loss -- 0 after a good one, -2 after a bad one (include/coattn.h states this)."""
    shape, row = G3_SHAPE, 2
    P, v, q, _ = H.case(*shape)
    good = H.target_of(shape, kind)
    bad = _bad_target(good, row, shape[3])
    sv = H.new_saved(shape)
    fresh = H.run_head(P, v, q, good, g_loss=1.3, flags=flags)
    assert H.head_status(fresh["saved"], shape) == (0, "")
    for step in range(2):
        r = H.run_head(P, v, q, bad, flags=flags, saved=sv)
        assert torch.isnan(r["loss"])
        rc, msg = H.head_status(sv, shape)
        assert rc == -2 and "row %d" % row in msg, (step, rc, msg)
        assert _bits(r["logits"], fresh["logits"])
        if step == 1:
            r = H.run_head(P, v, q, None, flags=flags, saved=sv)                 # logits only: the word stays
            assert H.head_status(sv, shape)[0] == -2
        r = H.run_head(P, v, q, good, g_loss=1.3, flags=flags, saved=sv)
        assert H.head_status(sv, shape) == (0, ""), step
        _intact(r)
        _same_bits(fresh, r)
    r = H.run_head(P, v, q, None, flags=flags, saved=sv)
    assert H.head_status(sv, shape) == (0, "") and _bits(r["logits"], fresh["logits"])
    assert sv.intact()


# ---- 7. non-finite confinement ----------------------------------------------------------------------------------------------
NONFINITE_SHAPES = [(5, 20, 12, 7), (33, 64, 96, 36)]


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("shape", NONFINITE_SHAPES, ids=_sid)
def test_head_nonfinite_input_row_is_confined(shape, value):
    """One NaN / +inf at v[1][B-1][d-1].  The other rows of logits and dv keep the clean call's bits, and the set of non-finite
    elements of every output is the float64 oracle's (NaN: the row everywhere, the loss and all parameter gradients; inf:
    tanh saturates, tanh' = 0, and 0 . inf = NaN reaches column d-1 of dW_p alone)."""
    B, d, mlp, K = shape
    P, v, q, labels = H.case(*shape)
    clean = _run(shape)
    v2 = v.clone()
    v2[1, B - 1, d - 1] = value
    res = H.run_head(P, v2, q, ("hard", labels), g_loss=1.7)
    ora = H.oracle(P, v2, q, ("hard", labels), g_loss=1.7)
    _intact(res)
    assert _bits(res["logits"][:B - 1], clean["logits"][:B - 1])
    for l in range(3):
        assert _bits(res["dv"][l][:B - 1], clean["dv"][l][:B - 1]), l
    got = _outputs(res)
    n = {}
    for k in H.OUTPUTS:
        g, o = ~torch.isfinite(got[k].cpu()), ~torch.isfinite(ora[k])
        n[k] = int(o.sum())
        assert torch.equal(g, o), (k, int(g.sum()), int(o.sum()), (g != o).nonzero()[:8].tolist())
    print("head_paths nonfinite", _sid(shape), value, n)
    assert n["W_p.weight"] > 0


@pytest.mark.parametrize("shape", NONFINITE_SHAPES, ids=_sid)
def test_head_inf_weight_row_is_confined(shape):
    """+inf at W_h[K-1][mlp-1]: only logits column K-1 is non-finite (as the oracle's), every other column keeps the clean
    call's bits -- nothing leaks from the zero-filled tails of the ragged tiles (0 . inf = NaN lands in rows >= B and columns
    >= K of the accumulator, which the epilogue must not store)."""
    B, d, mlp, K = shape
    P, v, q, _ = H.case(*shape)
    clean = H.run_head(P, v, q)
    P2 = dict(P)
    P2[H.NAMES[6]] = P[H.NAMES[6]].clone()
    P2[H.NAMES[6]][K - 1, mlp - 1] = float("inf")
    res = H.run_head(P2, v, q)
    _intact(res)
    bad = ~torch.isfinite(res["logits"].cpu())
    assert torch.equal(bad, ~torch.isfinite(H.oracle(P2, v, q)["logits"]))
    assert bad[:, K - 1].all() and not bad[:, :K - 1].any()
    assert _bits(res["logits"][:, :K - 1], clean["logits"][:, :K - 1])


# ---- 8. argument checks -----------------------------------------------------------------------------------------------------
def _raw(which, dtype=None, dims=(4, 8, 8, 3), labels=True, loss=True, g_loss=True, g_logits=False, dv=True, dq=False,
         null_dv_level=None, null_grad=False, A=2, kind=1):
    """One C-ABI call on sentinel-filled buffers sized for (4, 8, 8, 3).  Returns (rc, message, every buffer untouched)."""
    from vqa_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    SV = 1234.5
    mk = lambda n: torch.full((n,), SV, device=dev)     # noqa: E731
    vs, qs, dvs, dqs = [[mk(32) for _ in range(3)] for _ in range(4)]
    ps, gs = [mk(128) for _ in range(8)], [mk(128) for _ in range(8)]
    logits, lossb, gl, gx, saved, ws = mk(12), mk(1), mk(1), mk(12), mk(4096), mk(4096)
    lab = torch.zeros(4, dtype=torch.int64, device=dev)
    idx, sc = torch.zeros(4, 16, dtype=torch.int32, device=dev), torch.ones(4, 16, device=dev)
    arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() if t is not None else None for t in ts])   # noqa: E731
    if null_dv_level is not None:
        dvs[null_dv_level] = None
    gp = [t.data_ptr() for t in gs]
    if null_grad:
        gp[5] = None
    p, pg = _lib.HeadParams(*[t.data_ptr() for t in ps]), _lib.HeadParamGrads(*gp)
    dtype = _lib.F32 if dtype is None else dtype
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if which == "forward":
        rc = lib.coattn_head_forward(arr(vs), arr(qs), C.byref(p), lab.data_ptr() if labels else None, logits.data_ptr(),
                                     lossb.data_ptr() if loss else None, saved.data_ptr(), *dims, dtype, 0, stream)
    elif which == "forward_soft":
        rc = lib.coattn_head_forward_soft(arr(vs), arr(qs), C.byref(p), idx.data_ptr(), sc.data_ptr(), A, kind, logits.data_ptr(),
                                          lossb.data_ptr() if loss else None, saved.data_ptr(), *dims, dtype, 0, stream)
    else:
        rc = lib.coattn_head_backward(arr(vs), arr(qs), C.byref(p), saved.data_ptr(), gl.data_ptr() if g_loss else None,
                                      gx.data_ptr() if g_logits else None, arr(dvs) if dv else None, arr(dqs) if dq else None,
                                      C.byref(pg), 0, ws.data_ptr(), *dims, dtype, 0, stream)
    msg = lib.coattn_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    bufs = [t for ts in (vs, qs, dvs, dqs, ps, gs) for t in ts if t is not None] + [logits, lossb, gl, gx, saved, ws]
    return rc, msg, all(bool((t == SV).all()) for t in bufs)


ARG_CASES = {
    "forward_dtype": ("forward", dict(dtype=1), "unsupported dtype"),
    "backward_dtype": ("backward", dict(dtype=1), "unsupported dtype"),
    "forward_bad_dims": ("forward", dict(dims=(4, 0, 8, 3)), "bad B="),
    "labels_without_loss": ("forward", dict(loss=False), "labels and loss go together"),
    "loss_without_labels": ("forward", dict(labels=False), "labels and loss go together"),
    "soft_without_loss": ("forward_soft", dict(loss=False), "null loss"),
    "soft_A0": ("forward_soft", dict(A=0), "A=0 answer slots"),
    "soft_A17": ("forward_soft", dict(A=17), "A=17 answer slots"),
    "soft_unknown_kind": ("forward_soft", dict(kind=3), "unknown loss kind 3"),
    "dq_without_dv": ("backward", dict(dv=False, dq=True), "dq without dv"),
    "null_dv_level": ("backward", dict(null_dv_level=1), "dv[1] is null"),
    "no_upstream_gradient": ("backward", dict(g_loss=False), "neither g_loss nor g_logits"),
    "null_parameter_gradient": ("backward", dict(null_grad=True), "null parameter-gradient pointer"),
}


@pytest.mark.parametrize("name", list(ARG_CASES))
def test_head_argument_checks(name):
    """Every refusal of head.hip returns a negative code with its message and launches nothing: every buffer the call was
    handed still holds its sentinel."""
    which, kw, text = ARG_CASES[name]
    rc, msg, untouched = _raw(which, **kw)
    assert rc < 0 and text in msg, (rc, msg)
    assert untouched


@pytest.mark.parametrize("which", ["forward", "forward_soft", "backward"])
def test_head_argument_checks_pass_the_good_call(which):
    """(the same calls with nothing wrong go through and write: the refusals above are the arguments', not the harness's)"""
    rc, msg, untouched = _raw(which, g_logits=True)
    assert rc == 0 and not untouched, (rc, msg)


@pytest.mark.parametrize("dims", [(1 << 20, 16384, 32, 5), (1, 16384, 16384, 5), (1, 32, 16384, 1 << 20), (1 << 20, 32, 32, 1 << 20)],
                         ids=["B_x_2d", "mlp_x_2d", "K_x_mlp", "B_x_K"])
def test_head_refuses_dimensions_beyond_its_descriptors(dims):
    """Every operand is addressed through a buffer descriptor with 32-bit byte offsets below 1 GB: sizes beyond that are
    refused by coattn_head_workspace_bytes (and by every entry point, through the same check) -- nothing is allocated here."""
    from vqa_amd import _lib
    lib = _lib.load()
    a, b = C.c_size_t(), C.c_size_t()
    assert lib.coattn_head_workspace_bytes(*dims, _lib.F32, C.byref(a), C.byref(b)) < 0
    assert "beyond the 1 GB per operand" in lib.coattn_last_error().decode()
    assert lib.coattn_head_status(None, *dims, None) < 0

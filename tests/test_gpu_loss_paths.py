"""GPU: the three kernels of csrc/ce.hip -- the hard-label cross entropy, the two soft-target losses, the VQA score -- straight
through the C-ABI (tests/_loss.py: every buffer an arena of its exact size between guard bands, outputs and workspace NaN-filled,
every margin checked after every call) against the float64 oracles, at the shapes where the kernels' loops change their trip
count or a wave falls idle, at constructed extremes, with bad labels and indices, and through the Python layer.

The rule (tests/_loss.check_grad / check_scalar): the deviation from float64 is at most 8 x the deviation of stock fp32 ops on
the same inputs, with a floor of 16 fp32 ulps -- for d loss / d logits separately on the target entries and on the rest, the
floor at each group's own largest magnitude; for the loss with the floor at the mean of the magnitudes it subtracts.  Every
figure is printed before it is asserted (LAB_NOTES section 18 has the table of one run: no case above 0.2 of its bound, so the
yardstick is the single stock-fp32 evaluation, not the worst of five seeds).

CASES is the list tests/test_loss_rule_cpu.py runs its checker over."""
import re

import numpy as np
import pytest
import torch

from tests import _loss as U
from tests import _soft_loss as SL

pytestmark = pytest.mark.gpu

# (B, K): the smallest shapes at which the strided loop over K (256 threads, four waves) changes its trip count or a wave falls idle
K_SHAPES = [(1, 1), (1, 2), (2, 63), (3, 64), (2, 65), (2, 255), (2, 256), (3, 257), (2, 511), (2, 513), (5, 1001), (3, 3001)]
# ... and the last-ticket workgroup's strided loop over the B row losses; the last two: a gradient of the order of 1 / B at the bound
B_SHAPES = [(255, 5), (256, 5), (257, 5), (513, 3), (257, 1001), (1000, 7)]
SHAPES = K_SHAPES + B_SHAPES
SCALES = (0.5, 3.0, 30.0)
ANSWERS = (1, 2, 16)
SHIFTS = {"hard": ("logits", "dlogits"), "soft_ce": ("logits", "dlogits", "ans_idx", "ans_score"),
          "bce": ("logits", "dlogits", "ans_idx", "ans_score")}
INT64_MIN, INT32_MIN = -2 ** 63, -2 ** 31


def cases_of(kind, shape):
    B, K = shape
    return [(kind, B, K, A, scale) for A in ((0,) if kind == "hard" else ANSWERS) for scale in SCALES]


CASES = [c for kind in U.KINDS for shape in SHAPES for c in cases_of(kind, shape)]
_id = lambda s: "B%d_K%d" % s                                             # noqa: E731


def _same(a, b):
    return U.same_bits(a.reshape(-1), b.reshape(-1))


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("kind", U.KINDS)
def test_loss_and_gradient_at_every_loop_boundary(kind, shape):
    """Per case: loss and both gradient groups under the rule, margins intact, the two status words 0, dlogits = NULL and a
    second call on the same workspace give the same bits, and so does every operand handed over 4 bytes behind its start."""
    for _, B, K, A, scale in cases_of(kind, shape):
        z, tgt, (l64, g64), (l32, g32), mask, lscale = U.references(kind, B, K, A, scale)
        name = "%s B%d K%d A%d s%g" % (kind, B, K, A, scale)
        r = U.run_loss(kind, z, tgt)
        assert r["status"] == 0 and r["words"] == [0, 0], (name, r["status"], r["words"], r["err"])
        U.check_scalar(name, r["loss"], l64, l32, lscale)
        U.check_grad(name, r["dlogits"], g64, g32, mask)
        if kind == "hard" and K == 1:
            assert float(r["loss"]) == 0.0 and bool((r["dlogits"] == 0).all())          # lse = z: exact zeros
        r0 = U.run_loss(kind, z, tgt, dlogits=False)
        assert r0["dlogits"] is None and _same(r0["loss"], r["loss"]) and r0["words"] == [0, 0], name
        r2 = U.run_loss(kind, z, tgt, ws=r["ws"])
        assert _same(r2["loss"], r["loss"]) and _same(r2["dlogits"], r["dlogits"]) and r2["words"] == [0, 0], name
        for shift in SHIFTS[kind]:
            rs = U.run_loss(kind, z, tgt, shift=shift)
            assert _same(rs["loss"], r["loss"]) and _same(rs["dlogits"], r["dlogits"]), (name, shift)


# ---- constructed rows -----------------------------------------------------------------------------------------------------
def _constructed(kind, B=6, K=300, A=3, scale=3.0):
    """Logits, labels and (for the soft kinds) slots whose slot 0 is (label, 1.0), as fresh tensors."""
    z = U.make_logits(B, K, scale, seed=17).clone()
    lab = U.make_labels(B, K, seed=18).clone()
    if kind == "hard":
        return z, lab, lab
    idx, sc = SL.make_targets(B, K, A, seed=19, label=lab)
    return z, lab, (idx, sc)


def _free_class(kind, tgt, shape, b, start, n=1):
    """The first `n` classes from `start` on (cyclically) that row b has no target at."""
    free = ~U.target_mask(kind, tgt, *shape)[b]
    K = shape[1]
    ks = [(start + j) % K for j in range(K) if bool(free[(start + j) % K])][:n]
    return ks if n > 1 else ks[0]


def _rule(kind, name, z, tgt, r, rows=None):
    l64, g64 = U.oracle(kind, z, tgt)
    l32, g32 = U.oracle(kind, z, tgt, torch.float32)
    U.check_scalar(name, r["loss"], l64, l32, U.loss_scale(kind, z, tgt))
    U.check_grad(name, r["dlogits"], g64, g32, U.target_mask(kind, tgt, *z.shape), rows)
    return l64, g64


@pytest.mark.parametrize("kind", U.KINDS)
def test_confident_and_huge_logits_in_value(kind):
    """A confident row (z[label] += 50: the loss cancels to about 0), a logit of 8e4 and of -8e4 at the label and away from it:
    loss and gradient against the oracle under the rule, not only finite."""
    z, lab, tgt = _constructed(kind)
    other = (lab + 7) % z.shape[1]
    z[0, lab[0]] += 50.0
    z[1, lab[1]] = 8.0e4
    z[2, other[2]] = 8.0e4
    z[3, lab[3]] = -8.0e4
    z[4, other[4]] = -8.0e4
    r = U.run_loss(kind, z, tgt)
    assert r["status"] == 0 and bool(torch.isfinite(r["loss"])) and bool(torch.isfinite(r["dlogits"]).all())
    _rule(kind, "%s extremes" % kind, z, tgt, r)
    zc = U.make_logits(4, 70, 3.0, seed=23).clone()                        # every row confident: the mean itself is about 0
    labc = U.make_labels(4, 70, seed=24)
    tgtc = labc if kind == "hard" else SL.one_hot_targets(labc, 2)
    zc[torch.arange(4), labc] += 50.0
    rc = U.run_loss(kind, zc, tgtc)
    _rule(kind, "%s confident" % kind, zc, tgtc, rc)


@pytest.mark.parametrize("kind", ["hard", "soft_ce"])
def test_minus_infinity_masks_a_class(kind):
    """-inf at classes without a target (two in row 0, every one in row 1): a finite loss, a gradient of exactly +0.0 there,
    the rest under the rule.  -inf at the label: the loss is +inf, as torch's, and the gradient has the oracle's pattern."""
    z, lab, tgt = _constructed(kind)
    B, K = z.shape
    free = ~U.target_mask(kind, tgt, B, K)
    masked = torch.zeros(B, K, dtype=torch.bool)
    masked[0, _free_class(kind, tgt, (B, K), 0, int(lab[0]) + 5, 2)] = True
    masked[1] = free[1]
    assert int(masked[0].sum()) == 2 and int(masked[1].sum()) >= K - 3
    z[masked] = float("-inf")
    r = U.run_loss(kind, z, tgt)
    assert r["status"] == 0 and bool(torch.isfinite(r["loss"])), r["loss"]
    assert bool((r["dlogits"][masked].view(torch.int32) == 0).all())                     # +0.0, not -0.0
    l64, g64 = _rule(kind, "%s -inf mask" % kind, z, tgt, r)
    assert bool(torch.isfinite(l64)) and bool((g64[masked] == 0).all())
    z2 = _constructed(kind)[0]
    z2[2, lab[2]] = float("-inf")
    r2 = U.run_loss(kind, z2, tgt)
    l64, g64 = U.oracle(kind, z2, tgt)
    assert float(l64) == float("inf") and float(r2["loss"]) == float("inf")
    assert torch.equal(U.nan_pattern(r2["dlogits"]), U.nan_pattern(g64))


@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("kind", U.KINDS)
def test_a_non_finite_logit_stays_in_its_row(kind, value):
    """+inf / NaN at a class without a target in row 2 and at the label in row 4: the loss and those rows' dlogits have the
    float64 oracle's NaN / inf pattern, every other row's dlogits keeps the finite case's bits."""
    z, lab, tgt = _constructed(kind)
    base = U.run_loss(kind, z, tgt)
    z[2, _free_class(kind, tgt, tuple(z.shape), 2, int(lab[2]) + 5)] = value
    z[4, lab[4]] = value
    r = U.run_loss(kind, z, tgt)
    l64, g64 = U.oracle(kind, z, tgt)
    print("non-finite %s %s: loss %s oracle %s" % (kind, value, float(r["loss"]), float(l64)))
    assert torch.equal(U.nan_pattern(r["loss"]), U.nan_pattern(l64)) and not bool(torch.isfinite(l64))
    for b in (2, 4):
        assert torch.equal(U.nan_pattern(r["dlogits"][b]), U.nan_pattern(g64[b])), (b, r["dlogits"][b], g64[b])
    rest = [0, 1, 3, 5]
    assert _same(r["dlogits"][rest], base["dlogits"][rest])


def test_bce_around_expf_limits():
    """BCE logits at +-87, +-89, +-103, +-105, +-1e4 -- where expf(-|z|) turns denormal and then 0 around softplus_safe /
    sigmoid_safe --, with and without a target: value and gradient under the rule.  A -inf logit: the oracle's NaN pattern."""
    values = torch.tensor([87.0, 89.0, 103.0, 105.0, 1.0e4])
    B, K, A = 4, 12, 2
    z = U.make_logits(B, K, 3.0, seed=29).clone()
    z[0, :5], z[1, :5], z[2, 5:10], z[3, 5:10] = values, -values, values, -values
    idx = torch.tensor([[0, 3], [1, 4], [-1, 11], [10, -1]], dtype=torch.int32)          # targets on some of them, none on others
    sc = torch.tensor([[1.0, 0.3], [0.6, 0.9], [0.0, 0.6], [0.3, 0.0]])
    r = U.run_soft(z, idx, sc, "bce")
    assert r["status"] == 0
    _rule("bce", "bce expf limits", z, (idx, sc), r)
    z[1, 7] = z[2, 11] = float("-inf")                                   # without and with a target
    r = U.run_soft(z, idx, sc, "bce")
    l64, g64 = U.oracle("bce", z, (idx, sc))
    assert torch.equal(U.nan_pattern(r["loss"]), U.nan_pattern(l64))
    assert torch.equal(U.nan_pattern(r["dlogits"]), U.nan_pattern(g64))
    fin = torch.isfinite(g64)
    assert bool((r["dlogits"][fin].double() - g64[fin]).abs().max() <= 16 * 2.0 ** -24 / B)


# ---- labels and indices ---------------------------------------------------------------------------------------------------
def _named_row(err):
    m = re.search(r"row (\d+)", err)
    assert m, err
    return int(m.group(1))


@pytest.mark.parametrize("want_grad", [True, False], ids=["dlogits", "null"])
def test_bad_labels(want_grad):
    """-1, -100 (torch's ignore_index, which the kernel does not implement), K, 2^31, 2^32 + 1 (a truncating cast would read
    class 1) and INT64_MIN, each in row 3: the loss NaN, coattn_ce_status -2 with the row named, the other rows' gradient
    untouched, and 0 after a good call on the same workspace.  Two bad rows: one of them is named.  (ce_rows_kernel indexes
    with the label only behind `ok`: nothing here reads out of range.)"""
    B, K = 6, 300
    z, lab = U.make_logits(B, K, 3.0, seed=17), U.make_labels(B, K, seed=18)
    good = U.run_ce(z, lab, dlogits=want_grad)
    assert good["status"] == 0
    for bad in (-1, -100, K, 2 ** 31, 2 ** 32 + 1, INT64_MIN):
        l2 = lab.clone()
        l2[3] = bad
        r = U.run_ce(z, l2, dlogits=want_grad)
        assert bool(torch.isnan(r["loss"])) and r["status"] == -2 and _named_row(r["err"]) == 3, (bad, r["loss"], r["status"], r["err"])
        assert r["words"] == [4, 0], (bad, r["words"])
        if want_grad:
            rest = [0, 1, 2, 4, 5]
            assert _same(r["dlogits"][rest], good["dlogits"][rest]) and bool(torch.isfinite(r["dlogits"][3]).all()), bad
        again = U.run_ce(z, lab, dlogits=want_grad, ws=r["ws"])
        assert again["status"] == 0 and again["words"] == [0, 0] and _same(again["loss"], good["loss"]), bad
    l2 = lab.clone()
    l2[1], l2[4] = -1, K + 5
    r = U.run_ce(z, l2, dlogits=want_grad)
    assert bool(torch.isnan(r["loss"])) and r["status"] == -2 and _named_row(r["err"]) in (1, 4), r["err"]


@pytest.mark.parametrize("what", ["soft_ce", "bce", "score"])
def test_bad_slot_indices(what):
    """K, -2 and INT32_MIN in a slot of row 3: NaN, -2 naming the row, 0 after a good call on the same workspace."""
    B, K, A = 6, 300, 3
    z = U.make_logits(B, K, 3.0, seed=17)
    idx, sc = SL.make_targets(B, K, A, seed=19, label=U.make_labels(B, K, seed=18))

    def call(i, ws=None):
        r = U.run_score(z, i, sc, ws=ws) if what == "score" else U.run_soft(z, i, sc, what, ws=ws)
        return r, (r["score_sum"] if what == "score" else r["loss"])

    good, v_good = call(idx)
    assert good["status"] == 0 and bool(torch.isfinite(v_good))
    for bad in (K, -2, INT32_MIN):
        i2 = idx.clone()
        i2[3, 1] = bad
        r, v = call(i2)
        assert bool(torch.isnan(v)) and r["status"] == -2 and _named_row(r["err"]) == 3, (bad, v, r["status"], r["err"])
        if what == "score":
            assert bool(torch.isnan(r["row_score"][3])) and _same(r["row_score"][[0, 1, 2, 4, 5]], good["row_score"][[0, 1, 2, 4, 5]])
            assert torch.equal(r["pred"], good["pred"])
        again, v2 = call(idx, ws=r["ws"])
        assert again["status"] == 0 and again["words"] == [0, 0] and _same(v2, v_good), bad


# ---- the score ------------------------------------------------------------------------------------------------------------
def _score_case(B, K, A):
    """Logits with every constructed row the shape has room for, and slots that name the predicted class in every second row."""
    z = U.make_logits(B, K, 3.0, seed=41).clone()
    top = float(z.max()) + 1.0
    z[0, K - 1] = top                                                    # the maximum in the last column
    rows = {0: K - 1}
    plan = [("equal", None), ("minus_inf", None), ("tie", (0, K - 1)), ("tie", (3, 259)), ("tie", (63, 64)), ("tie", (255, 256)),
            ("tie", (K - 2, K - 1))]
    b = 1
    for what, pair in plan:
        if b >= B:
            break
        if what == "equal":
            z[b] = 0.25
            rows[b] = 0
        elif what == "minus_inf":
            z[b] = float("-inf")
            rows[b] = 0
        elif 0 <= pair[0] < pair[1] < K:
            z[b, pair[0]] = z[b, pair[1]] = top
            rows[b] = pair[0]
        else:
            continue
        b += 1
    pred = np.argmax(z.numpy(), axis=1)
    idx, sc = [t.clone() for t in U.make_slots(B, K, A, seed=43)]
    idx[::2, 0] = torch.from_numpy(pred[::2]).to(torch.int32)
    sc[::2, 0] = 0.6
    return z, idx, sc, rows


@pytest.mark.parametrize("A", ANSWERS)
@pytest.mark.parametrize("shape", [(8, K) for K in (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1001, 3001)] + B_SHAPES[:4], ids=_id)
def test_score_ties_edges_and_sum(shape, A):
    """Ties inside one thread's stride (k, k + 256), across lanes and waves (63 / 64, 255 / 256), between K - 1 and 0 and at
    the last two columns, a row of equal logits and a row of -inf (index 0), the maximum in the last column: pred is
    numpy.argmax and < K, row_score the oracle's selection bit for bit, score_sum under the loss rule with scale sum row_score;
    row_score = NULL, a second call on the workspace and every shifted operand give the same bits; the CPU fallback of
    vqa_amd.loss.vqa_score agrees."""
    from vqa_amd import loss as L
    B, K = shape
    z, idx, sc, rows = _score_case(B, K, A)
    r = U.run_score(z, idx, sc)
    assert r["status"] == 0 and r["words"] == [0, 0]
    p_ref = U.check_score("score B%d K%d A%d" % (B, K, A), r["pred"], r["row_score"], r["score_sum"], z, idx, sc)[0]
    assert all(int(p_ref[b]) == k for b, k in rows.items()), (rows, p_ref)
    r0 = U.run_score(z, idx, sc, row_score=False)
    assert r0["row_score"] is None and _same(r0["score_sum"], r["score_sum"]) and torch.equal(r0["pred"], r["pred"])
    r2 = U.run_score(z, idx, sc, ws=r["ws"])
    assert _same(r2["score_sum"], r["score_sum"]) and _same(r2["row_score"], r["row_score"]) and torch.equal(r2["pred"], r["pred"])
    for shift in ("logits", "ans_idx", "ans_score", "pred", "row_score"):
        rs = U.run_score(z, idx, sc, shift=shift)
        assert _same(rs["score_sum"], r["score_sum"]) and _same(rs["row_score"], r["row_score"]) and torch.equal(rs["pred"], r["pred"]), shift
    p_cpu, r_cpu, _ = L.vqa_score(z, idx, sc)
    assert p_cpu.tolist() == r["pred"].tolist() and _same(r_cpu, r["row_score"])


# ---- non-finite scores and NaN logits in the score (include/coattn.h states both) -------------------------------------------
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_score_in_a_live_slot(value):
    """Row 1's live slot 0 holds NaN / +inf.  BCE: the loss and the row's dlogits have the oracle's pattern (NaN: the loss and
    that one entry NaN; +inf: the target clamps to 1, everything under the rule).  SOFT_CE with NaN: the oracle's pattern (the
    whole row, through S_b).  Score: the row's score NaN, or 1 for +inf.  Every other row keeps the finite case's bits.  (A min
    that returns its non-NaN argument made the NaN a target of 1: a perfect score for the row.)"""
    from vqa_amd import loss as L
    B, K, A = 4, 70, 3
    z = U.make_logits(B, K, 3.0, seed=51).clone()
    lab = U.make_labels(B, K, seed=52)
    idx, sc = SL.make_targets(B, K, A, seed=53, label=lab)
    z[torch.arange(B), lab] += 20.0                                       # every row predicts its slot-0 class
    bad = sc.clone()
    bad[1, 0] = value
    others = [0, 2, 3]
    for kind in ("bce", "soft_ce") if value != value else ("bce",):
        base, r = U.run_soft(z, idx, sc, kind), U.run_soft(z, idx, bad, kind)
        l64, g64 = U.oracle(kind, z, (idx, bad))
        print("non-finite score %s %s: loss %s oracle %s" % (kind, value, float(r["loss"]), float(l64)))
        assert r["status"] == 0 and torch.equal(U.nan_pattern(r["loss"]), U.nan_pattern(l64))
        assert torch.equal(U.nan_pattern(r["dlogits"]), U.nan_pattern(g64))
        assert bool(torch.isnan(l64)) == (value != value)
        if value != value and kind == "bce":
            assert int(torch.isnan(r["dlogits"]).sum()) == 1 and bool(torch.isnan(r["dlogits"][1, lab[1]]))
        if value == float("inf"):
            _rule(kind, "bce inf score", z, (idx, bad), r)
        assert _same(r["dlogits"][others], base["dlogits"][others])
    base, r = U.run_score(z, idx, sc), U.run_score(z, idx, bad)
    print("non-finite score %s: row_score %s sum %s" % (value, r["row_score"].tolist(), float(r["score_sum"])))
    p_ref, r_ref, s64, _ = U.check_score("score %s" % value, r["pred"], r["row_score"], r["score_sum"], z, idx, bad)
    assert p_ref.tolist() == lab.tolist()
    if value != value:
        assert bool(torch.isnan(r["row_score"][1])) and bool(torch.isnan(r["score_sum"]))
    else:
        assert float(r["row_score"][1]) == 1.0 and float(r["score_sum"]) == float(s64)
    assert _same(r["row_score"][others], base["row_score"][others])
    r0 = U.run_score(z, idx, bad, row_score=False)
    assert _same(r0["score_sum"], r["score_sum"])
    p_cpu, r_cpu, _ = L.vqa_score(z, idx, bad)
    assert p_cpu.tolist() == r["pred"].tolist() and _same(r_cpu, r["row_score"])


@pytest.mark.parametrize("K", [5, 300, 513, 1001])
def test_nan_logits_in_the_score(K):
    """pred is the FIRST NaN index, as numpy.argmax and torch.argmax give it: one NaN; two in different threads; two in one
    thread's stride (k, k + 256); NaNs behind and in front of a larger finite maximum and of +inf; a row of NaN."""
    from vqa_amd import loss as L
    nan = float("nan")
    B, A = 8, 2
    z = U.make_logits(B, K, 3.0, seed=61).clone()
    top = float(z.max()) + 5.0
    want = {}
    z[0, K - 1] = nan
    want[0] = K - 1
    z[1, 3], z[1, 1] = nan, top
    want[1] = 3
    z[2, 2], z[2, 4] = nan, float("inf")
    want[2] = 2
    z[3, 0], z[3, 4] = float("inf"), nan
    want[3] = 4
    z[4] = nan
    want[4] = 0
    if K > 300:                                                          # (room for a second trip of the strided loop)
        z[5, 44], z[5, 300] = nan, nan                                   # one thread: 44 and 300
        want[5] = 44
        z[6, 299], z[6, 70] = nan, nan                                   # two waves
        want[6] = 70
        z[7, 257], z[7, 2] = nan, top                                    # the NaN in the second trip, the maximum in the first
        want[7] = 257
    idx, sc = [t.clone() for t in U.make_slots(B, K, A, seed=63)]
    for b, k in want.items():
        idx[b, 0], sc[b, 0] = k, 0.9
    r = U.run_score(z, idx, sc)
    print("nan logits K%d: pred %s want %s" % (K, r["pred"].tolist(), want))
    assert r["status"] == 0
    p_ref = U.check_score("score nan K%d" % K, r["pred"], r["row_score"], r["score_sum"], z, idx, sc)[0]
    assert all(int(p_ref[b]) == k for b, k in want.items()), (want, p_ref)
    p_cpu, r_cpu, _ = L.vqa_score(z, idx, sc)
    assert p_cpu.tolist() == r["pred"].tolist() and _same(r_cpu, r["row_score"])


# ---- the Python layer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", U.KINDS)
def test_python_layer(kind):
    """vqa_amd.loss: non-contiguous logits give the contiguous copy's bits, bf16 logits under autocast the bits of their
    .float(), no requires_grad the same loss, backward with an upstream gradient other than 1 twice over a retained graph; CPU
    tensors (and int32 labels) fall back to stock ops with the stock value."""
    import torch.nn.functional as F
    from vqa_amd import loss as L
    B, K, A = 5, 70, 3
    z = U.make_logits(B, K, 3.0, seed=71)
    lab = U.make_labels(B, K, seed=72)
    idx, sc = SL.make_targets(B, K, A, seed=73, label=lab)
    dev = torch.device("cuda:0")
    tg = (lab.to(dev),) if kind == "hard" else (idx.to(dev), sc.to(dev))
    fn = (lambda x: L.cross_entropy(x, *tg)) if kind == "hard" else (lambda x: L.soft_target_loss(x, *tg, kind))   # noqa: E731

    def both(x):
        x = x.detach().requires_grad_(True)
        out = fn(x)
        (g,) = torch.autograd.grad(out, x)
        return out.detach(), g

    l0, g0 = both(z.to(dev))
    ref = U.run_loss(kind, z, lab if kind == "hard" else (idx, sc))
    assert _same(l0.cpu(), ref["loss"]) and _same(g0.cpu(), ref["dlogits"])
    lt, gt = both(z.t().contiguous().to(dev).t())                        # [B,K] with strides (1, B)
    assert not z.t().contiguous().t().is_contiguous() and _same(lt, l0) and _same(gt, g0)
    wide = torch.zeros(B, 2 * K)
    wide[:, ::2] = z
    ls, gs = both(wide.to(dev)[:, ::2])
    assert _same(ls, l0) and _same(gs, g0)
    zb = z.to(dev).bfloat16()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lb = fn(zb)
    assert _same(lb.float(), fn(zb.float()))
    with torch.no_grad():
        assert _same(fn(z.to(dev)), l0)
    x = z.to(dev).requires_grad_(True)
    out = fn(x)
    for _ in range(2):
        x.grad = None
        (out * 2.5).backward(retain_graph=True)
        assert _same(x.grad, g0 * 2.5)
    if kind == "hard":
        crit, stock = L.CrossEntropyLoss(), F.cross_entropy(z, lab)
        assert _same(crit(z, lab), stock) and _same(crit(z.to(dev), lab.to(dev)), l0)
        for zz, ll in ((z, lab.int()), (z.to(dev), lab.to(dev).int())):                  # int32 labels: the stock functional's
            with pytest.raises(RuntimeError, match="Long|Int|int"):                      # own refusal, not the HIP kernel on
                crit(zz, ll)                                                              # 4-byte labels
        l64, _ = U.oracle_ce(z.double(), lab)
        assert _same(crit(z.double(), lab), l64)
    else:
        crit = L.SoftTargetLoss(kind)
        l64, _ = U.oracle_soft(z, idx, sc, kind)
        assert _same(crit(z.to(dev), *tg), l0)
        assert abs(float(crit(z.double(), idx, sc)) - float(l64)) <= 1e-12 * max(1.0, abs(float(l64)))
        l32, _ = U.oracle_soft(z, idx, sc, kind, torch.float32)
        assert abs(float(crit(z, idx, sc)) - float(l32)) <= 16 * 2.0 ** -24 * U.loss_scale(kind, z, (idx, sc))

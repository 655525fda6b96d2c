"""The checker of tests/test_gpu_loss_paths.py without a GPU (tests/_loss.check_grad / check_scalar / check_score), over that
file's own case list: (a) the stock-fp32 evaluation of every case is accepted -- and so is the float64 result rounded to fp32 --,
so the reference alone stays inside the rule; (b) planted errors of the kinds a loss kernel can make are rejected, each planted
into a copy of the float64 result rounded to fp32, which is accepted without the plant."""
import pytest
import torch

from tests import _loss as U
from tests import _soft_loss as SL
from tests.test_gpu_loss_paths import CASES, SHAPES, cases_of


def test_the_case_list_covers_every_boundary_the_kernels_have():
    Ks, Bs = {K for _, K in SHAPES}, {B for B, _ in SHAPES}
    assert {1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1001, 3001} <= Ks and {1, 255, 256, 257, 513, 1000} <= Bs
    assert len(CASES) == len(SHAPES) * (3 + 9 + 9) and len(set(CASES)) == len(CASES)
    for kind, B, K, A, scale in CASES:
        tgt = U.references(kind, B, K, A, scale)[1]
        if kind == "hard" and B >= 2:
            assert int(tgt[0]) == 0 and int(tgt[1]) == K - 1                             # class 0 and class K - 1
    idx, sc = U.make_slots(257, 1001, 16)
    assert bool((idx == -1).all(1).any()) and bool((idx[::5, 0] == idx[::5, 1]).all()) and bool((idx == -1).any())
    t = U.dense((idx, sc), 1001)
    assert abs(float(t[2].sum()) - 1.6) < 1e-6 and float(t[2].max()) > 1.5               # the sixteen-slot row: S_b = 1.6, t > 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_K%d" % s)
@pytest.mark.parametrize("kind", U.KINDS)
def test_the_yardstick_and_the_rounded_reference_are_accepted(kind, shape):
    for _, B, K, A, scale in cases_of(kind, shape):
        z, tgt, (l64, g64), (l32, g32), mask, lscale = U.references(kind, B, K, A, scale)
        name = "%s B%d K%d A%d s%g" % (kind, B, K, A, scale)
        assert bool(torch.isfinite(g64).all()) and bool(torch.isfinite(l64)) and lscale >= 0
        U.check_scalar(name + " stock", l32, l64, l32, lscale)
        U.check_grad(name + " stock", g32, g64, g32, mask)
        U.check_scalar(name + " rounded", l64.float(), l64, l32, lscale)
        U.check_grad(name + " rounded", g64.float(), g64, g32, mask)


# ---- planted errors -------------------------------------------------------------------------------------------------------
def _case(kind, B, K, A, scale):
    assert (kind, B, K, A, scale) in CASES
    z, tgt, (l64, g64), (l32, g32), mask, lscale = U.references(kind, B, K, A, scale)
    U.check_grad("unplanted", g64.float(), g64, g32, mask)
    U.check_scalar("unplanted", l64.float(), l64, l32, lscale)
    return z.double(), tgt, l64, g64, l32, g32, mask, lscale


def _rejected_grad(name, g, g64, g32, mask):
    with pytest.raises(AssertionError):
        U.check_grad(name, g.float(), g64, g32, mask)


def _rejected_loss(name, l, l64, l32, lscale):
    with pytest.raises(AssertionError):
        U.check_scalar(name, l.float(), l64, l32, lscale)


def test_a_strip_of_the_bulk_scaled_by_1_001_is_rejected():
    """Case hard (257, 1001) at scale 0.5 -- the shape at which a bound of 1e-6 absolute passes a bulk 2 % wrong: the bulk
    entries of the columns 256..511 times 1.001."""
    z, lab, l64, g64, l32, g32, mask, _ = _case("hard", 257, 1001, 0, 0.5)
    g = g64.clone()
    strip = torch.zeros_like(mask)
    strip[:, 256:512] = True
    g[strip & ~mask] *= 1.001
    assert float((g - g64).abs().max()) < 1e-6                           # the earlier bound does not see it
    _rejected_grad("strip", g, g64, g32, mask)


def test_the_last_class_left_out_of_the_normaliser_is_rejected():
    """Case hard (5, 1001) at scale 0.5: softmax normalised by s - exp(z[K - 1] - m)."""
    z, lab, l64, g64, l32, g32, mask, _ = _case("hard", 5, 1001, 0, 0.5)
    B, K = z.shape
    p = torch.softmax(z, 1)
    g = p / (1.0 - p[:, -1:]) / B
    g[torch.arange(B), lab] -= 1.0 / B
    _rejected_grad("normaliser", g, g64, g32, mask)


def test_the_one_hot_subtracted_one_class_late_is_rejected():
    """Case hard (3, 257) at scale 3: the 1 / B taken off at label + 1."""
    z, lab, l64, g64, l32, g32, mask, _ = _case("hard", 3, 257, 0, 3.0)
    B, K = z.shape
    g = torch.softmax(z, 1) / B
    g[torch.arange(B), (lab + 1) % K] -= 1.0 / B
    _rejected_grad("one-hot", g, g64, g32, mask)


def test_one_over_b_plus_one_is_rejected_at_b_1000():
    """Case hard (1000, 7) at scale 3: the gradient and the loss scaled by 1 / (B + 1) instead of 1 / B."""
    z, lab, l64, g64, l32, g32, mask, lscale = _case("hard", 1000, 7, 0, 3.0)
    _rejected_grad("1/(B+1)", g64 * (1000.0 / 1001.0), g64, g32, mask)
    _rejected_loss("1/(B+1)", l64 * (1000.0 / 1001.0), l64, l32, lscale)


@pytest.mark.parametrize("kind", ["soft_ce", "bce"])
def test_the_last_row_stored_one_row_early_is_rejected(kind):
    """Cases soft_ce and bce (3, 64), A = 2, at scale 3: row B - 2 holds row B - 1's gradient."""
    z, tgt, l64, g64, l32, g32, mask, _ = _case(kind, 3, 64, 2, 3.0)
    g = g64.clone()
    g[-2] = g64[-1]
    _rejected_grad("row early", g, g64, g32, mask)


def _custom_soft(kind, B, K, A, scale, row_idx, row_sc):
    """Case (kind, B, K, A, scale) with row 0's slots replaced: its references, recomputed."""
    assert (kind, B, K, A, scale) in CASES
    z = U.make_logits(B, K, scale)
    idx, sc = [t.clone() for t in U.make_slots(B, K, A)]
    idx[0], sc[0] = torch.tensor(row_idx, dtype=torch.int32), torch.tensor(row_sc)
    tgt = (idx, sc)
    (l64, g64), (l32, g32) = U.oracle(kind, z, tgt), U.oracle(kind, z, tgt, torch.float32)
    mask, lscale = U.target_mask(kind, tgt, B, K), U.loss_scale(kind, z, tgt)
    U.check_grad("unplanted", g64.float(), g64, g32, mask)
    U.check_scalar("unplanted", l64.float(), l64, l32, lscale)
    return z.double(), U.dense(tgt, K), l64, g64, l32, g32, mask, lscale


def test_bce_without_the_clamp_is_rejected():
    """Case bce (5, 1001), A = 2, at scale 3, row 0's two slots naming the class of its largest |logit| with 0.6 each (t = 1.2):
    the target taken as 1.2 in the gradient and in the loss."""
    k = int(U.make_logits(5, 1001, 3.0)[0].abs().argmax())
    z, t, l64, g64, l32, g32, mask, lscale = _custom_soft("bce", 5, 1001, 2, 3.0, [k, k], [0.6, 0.6])
    assert abs(float(t[0, k]) - 1.2) < 1e-6
    g = g64.clone()
    g[0, k] -= (float(t[0, k]) - 1.0) / 5
    _rejected_grad("no clamp", g, g64, g32, mask)
    _rejected_loss("no clamp", l64 - (float(t[0, k]) - 1.0) * z[0, k] / 5, l64, l32, lscale)


def test_a_duplicate_pair_counted_once_in_s_is_rejected():
    """Case soft_ce (5, 1001), A = 2, at scale 3, whose row 0 is make_targets' duplicate pair (0.3 and 0.6 at one class):
    S_0 = 0.6 instead of 0.9, in the gradient's bulk and in the loss."""
    z, tgt, l64, g64, l32, g32, mask, lscale = _case("soft_ce", 5, 1001, 2, 3.0)
    idx, sc = tgt
    assert int(idx[0, 0]) == int(idx[0, 1]) >= 0 and sc[0].tolist() == pytest.approx([0.3, 0.6])
    g = g64.clone()
    g[0] -= 0.3 * torch.softmax(z[0], 0) / 5
    _rejected_grad("S_b", g, g64, g32, mask)
    _rejected_loss("S_b", l64 - 0.3 * torch.logsumexp(z[0], 0) / 5, l64, l32, lscale)


def test_the_mean_without_row_256_is_rejected_at_b_257():
    """Case hard (257, 5) at scale 3: the strided sum over the B row losses stopping at 256."""
    z, lab, l64, g64, l32, g32, mask, lscale = _case("hard", 257, 5, 0, 3.0)
    rows = torch.logsumexp(z, 1) - z[torch.arange(257), lab]
    assert abs(float(rows.mean()) - float(l64)) < 1e-12
    _rejected_loss("row 256", rows[:256].sum() / 257, l64, l32, lscale)


def test_score_plants_are_rejected():
    """(4, 70), A = 3: the higher index of a tie as pred; t[pred] = 1.2 left unclamped in row_score and in the sum."""
    B, K, A = 4, 70, 3
    z = U.make_logits(B, K, 3.0, seed=41).clone()
    z[1, 5] = z[1, 69] = float(z.max()) + 1.0
    z[2, 9] = float(z.max()) + 2.0
    idx, sc = [t.clone() for t in U.make_slots(B, K, A, seed=43)]
    idx[1, 0], sc[1, 0] = 5, 0.9
    idx[2], sc[2] = torch.tensor([9, 9, -1], dtype=torch.int32), torch.tensor([0.6, 0.6, 0.0])
    pred, rows, s64, s32 = U.oracle_score(z, idx, sc)
    assert int(pred[1]) == 5 and int(pred[2]) == 9 and float(rows[2]) == 1.0
    pred32, rows32 = pred.to(torch.int32), rows.float()
    U.check_score("unplanted", pred32, rows32, s32, z, idx, sc)
    U.check_score("unplanted", pred32, None, s64.float(), z, idx, sc)
    p = pred32.clone()
    p[1] = 69
    with pytest.raises(AssertionError):
        U.check_score("tie", p, rows32, s32, z, idx, sc)
    r = rows32.clone()
    r[2] = 1.2
    with pytest.raises(AssertionError):
        U.check_score("unclamped", pred32, r, s32, z, idx, sc)
    with pytest.raises(AssertionError):
        U.check_score("unclamped sum", pred32, rows32, r.sum(), z, idx, sc)
    p[1] = K
    with pytest.raises(AssertionError):
        U.check_score("pred = K", p, rows32, s32, z, idx, sc)
    assert SL.score(z, idx, sc)[0].tolist() == pred.tolist()

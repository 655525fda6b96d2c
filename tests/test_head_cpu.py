"""CPU: the oracles tests/test_gpu_head_paths.py measures the answer head against (tests/_head.py).  The restatement of the
reduced-precision mode with its rounding switched off IS the float64 oracle (so what it adds is the rounding alone); with the
rounding on it stays inside the bf16 bounds tests/test_gpu_head.py holds the kernel to; and the float32 evaluation -- the
yardstick whose distance e32 from the float64 oracle scales the exact mode's bound -- is pinned below 2e-6 at every shape of
the GPU sweeps, so that a broken yardstick cannot loosen that bound."""
import pytest
import torch

from tests import _head as H

VARIANTS = [pytest.param("hard", 1.7, False, id="g_loss"), pytest.param("hard", 0.5, True, id="g_loss+g_logits"),
            pytest.param(None, None, True, id="g_logits_only"), pytest.param("soft_ce", 1.7, False, id="soft_ce"),
            pytest.param("bce", 1.7, True, id="bce+g_logits")]


@pytest.mark.parametrize("target,g_loss,gx", VARIANTS)
@pytest.mark.parametrize("shape", [(5, 20, 12, 7), (37, 64, 128, 20)], ids=lambda s: "B%d_d%d_mlp%d_K%d" % s)
def test_bf16_restatement_without_rounding_is_the_oracle(shape, target, g_loss, gx):
    ora = H.oracle_head(shape, target, g_loss, gx)
    res = H.oracle_head_bf16(shape, target, g_loss, gx, rounding=False)
    e = H.errors(res, ora)
    assert set(e) >= {"logits", "dv"} | set(H.NAMES)
    assert max(e.values()) < 1e-12, e


@pytest.mark.parametrize("shape", [(70, 96, 160, 33), (3, 20, 12, 5)], ids=lambda s: "B%d_d%d_mlp%d_K%d" % s)
def test_bf16_restatement_is_within_the_bf16_bounds(shape):
    """2e-2 of max|.| on every output and 1e-2 relative L2 (test_gpu_head.py's bounds for the kernel in this mode), and
    the rounding is really on: no output equals the oracle's."""
    ora = H.oracle_head(shape)
    res = H.oracle_head_bf16(shape)
    for k in ("logits", "dv") + H.NAMES:
        l2 = ((res[k] - ora[k]).norm() / ora[k].norm()).item()
        assert 0 < H.rel(res[k], ora[k]) < 2e-2 and l2 < 1e-2, (k, H.rel(res[k], ora[k]), l2)
    assert abs(res["loss"].item() - ora["loss"].item()) < 2e-2 * abs(ora["loss"].item())


def test_f32_yardstick_is_pinned():
    """e32 < 2e-6 at every (shape, upstream-gradient variant) whose e32 scales a bound of the GPU file, and at cfg 2's shape,
    the largest the head's direct test runs -- and > 0 wherever the case has a gradient: the yardstick measures something."""
    from tests import test_gpu_head_paths as T
    worst = {}
    for shape, var in T.E32_CASES + [((160, 512, 1024, 1001), T.V_LOSS)]:
        e = H.e32(shape, *var, T.SEEDS.get(shape, 0))
        worst[(shape, var)] = e
        assert e < 2e-6, (shape, var, e)
        if shape[3] > 1:
            assert e > 0, (shape, var)
    top = max(worst, key=worst.get)
    low = min(worst, key=worst.get)
    print("head e32: %d cases, worst %.2e at %s, least %.2e at %s" % (len(worst), worst[top], top, worst[low], low))

"""The forward -> backward contract of `saved` (include/coattn.h): the backward needs the forward's inputs with the same VALUES,
shapes, mode and lengths -- not at the same addresses.  Whatever the forward chose to keep in `saved` for the backward (the
image of W_q^T for the dQ projection, the exact mode's bitmap of the live question rows) must be read only when that forward
wrote it: here the two calls see the same question features at differently aligned addresses, share one `saved` buffer with an
earlier forward of other values, or come from the two entry-point families the header lets one pair.

Every gradient is held against the float64 oracle of tests/test_gpu_attention_grad.py (exact mode 2e-5, tolerance mode 1e-4 of
max|ref|; dc_v / dc_q on an absolute scale).  The question features end in zero pad rows (mixed lengths), so that the exact
mode's bitmap really drops rows.  Every output, `saved` and workspace buffer is NaN-filled first."""
import pytest
import torch

from tests.test_gpu_attention_grad import DEV, GRADS, call, case, err, mixed_lens, oracle, same_bits
from vqa_amd import _lib

pytestmark = pytest.mark.gpu

# (B, N, T, d, impl, layout): the fused kernels at cfg 2's grids in both layouts, and a general-path shape (T > 28) whose P_q
# projection still runs on the pre-split-weight kernel (B T >= 128, d % 32 == 0).  (B T = 104 < 128 at n196_cm: neither the
# bitmap nor the W_q^T image exists there; n196_cm_b6 has both.)
SHAPES = {"n49_lm": (8, 49, 26, 512, "fused", "lm"), "n196_cm": (4, 196, 26, 512, "fused", "cm"),
          "n196_cm_b6": (6, 196, 26, 512, "fused", "cm"), "general_t32": (4, 49, 32, 256, "auto", "lm")}
TOL = {"exact": 2e-5, "fast16": 1e-4}
KEYS = ("v", "q") + tuple(GRADS)

_ORACLE = {}


def _case(shape, masked, seed=43):
    B, N, T, d, impl, layout = SHAPES[shape]
    lens = mixed_lens(B, T)
    V, Qs, P, gv, gq, g_av, g_aq = case(B, N, T, d, lens, seed=seed)
    key = (shape, masked, seed)
    if key not in _ORACLE:
        _ORACLE[key] = oracle(V, Qs, P, lens if masked else None, gv, gq, torch.zeros_like(g_av), torch.zeros_like(g_aq))
    return (V, Qs, P, gv, gq), (lens if masked else None), impl, layout, _ORACLE[key]


def at(q, offset):
    """q on the device, `offset` floats past the start of a fresh allocation: offset 0 is 16-byte aligned, offset 1 is not."""
    buf = torch.empty(q.numel() + 64, device=DEV)
    v = buf[offset:offset + q.numel()].view(q.shape)
    v.copy_(q.to(DEV))
    assert (v.data_ptr() % 16 == 0) == (offset % 4 == 0)
    return v


def check(r, o, mode, what):
    for k in KEYS:
        assert torch.isfinite(r[k]).all(), (what, k)
        assert err(r, o, k) < TOL[mode], (what, k, err(r, o, k))


def test_full_length_inputs_have_pad_rows_to_drop():
    """(the premise of this file: the mixed lengths leave rows of exact zeros in every level)"""
    for shape in SHAPES:
        B, N, T, d, *_ = SHAPES[shape]
        _, Qs, *_ = case(B, N, T, d, mixed_lens(B, T), seed=43)
        assert all((q.abs().sum(-1) == 0).any() for q in Qs)
        assert _lib.load().coattn_fused_supported(B, N, T, d, 3, 0) == (SHAPES[shape][4] == "fused")


# ---- 1. the same values at other addresses -------------------------------------------------------------------------------------
# forward Q offsets per level -> backward Q offsets per level
ALIGNS = {"fwd_unaligned": ((1, 1, 1), (0, 0, 0)), "bwd_unaligned": ((0, 0, 0), (1, 1, 1)),
          "fwd_level1_unaligned": ((0, 1, 0), (0, 0, 0))}


@pytest.mark.parametrize("align", list(ALIGNS))
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", ["exact", "fast16"])
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_backward_does_not_need_the_forwards_addresses(align, shape, mode, masked):
    (V, Qs, P, gv, gq), lens, impl, layout, o = _case(shape, masked)
    fo, bo = ALIGNS[align]
    Qf = [at(q, k) for q, k in zip(Qs, fo)]
    Qb = [at(q, k) for q, k in zip(Qs, bo)]
    r = call(V, Qf, P, lens, gv, gq, mode=mode, impl=impl, layout=layout, api="plain", Qs_bwd=Qb)
    check(r, o, mode, align)
    if lens is not None:
        for b, n in enumerate(lens):
            assert (r["dQ"][:, b, n:] == 0).all()


# ---- 2. a `saved` buffer that an earlier forward wrote --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", ["exact", "fast16"])
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_backward_reads_nothing_stale_from_saved(shape, mode, masked):
    """forward #1 (aligned Q1: the bitmap and the W_q^T image written), forward #2 into the same `saved` (unaligned Q2 of other
    values and another pad pattern), backward #2 with aligned copies of Q2: the gradients of Q2."""
    B, N, T, d, impl, layout = SHAPES[shape]
    (V, Q1, P, gv, gq), lens1, *_ = _case(shape, masked)
    V2, Q2, _, _, _, _, _ = case(B, N, T, d, [T - (b * 5) % T for b in range(B)], seed=47)
    lens2 = [T - (b * 5) % T for b in range(B)] if masked else None
    assert not all(torch.equal(a.abs().sum(-1) == 0, b.abs().sum(-1) == 0) for a, b in zip(Q1, Q2))
    o2 = oracle(V, Q2, P, lens2, gv, gq, torch.zeros(3, B, N), torch.zeros(3, B, T))
    sb = _lib.workspace_bytes(B, N, T, d, 3, 0)[0]
    saved = torch.full((sb // 4,), float("nan"), device=DEV)
    r1 = call(V, [at(q, 0) for q in Q1], P, lens1, mode=mode, impl=impl, layout=layout, api="plain", saved=saved)
    assert torch.isfinite(r1["v"]).all()
    r = call(V, [at(q, 1) for q in Q2], P, lens2, gv, gq, mode=mode, impl=impl, layout=layout, api="plain", saved=saved,
             Qs_bwd=[at(q, 0) for q in Q2])
    check(r, o2, mode, "stale saved")


# ---- 3. the pairs the header allows across the two families ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", ["exact", "fast16"])
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_forward_and_backward_families_pair_freely(shape, mode, masked):
    """coattn_forward_maps(_len) + coattn_backward(_len), and coattn_forward(_len) + coattn_backward_maps(_len) with
    g_av = g_aq = NULL: the same bits as each family's own pair (and the oracle's gradients)."""
    (V, Qs, P, gv, gq), lens, impl, layout, o = _case(shape, masked)
    kw = dict(mode=mode, impl=impl, layout=layout)
    plain = call(V, Qs, P, lens, gv, gq, api="plain", **kw)
    maps = call(V, Qs, P, lens, gv, gq, api="maps", **kw)
    maps_plain = call(V, Qs, P, lens, gv, gq, api="maps", api_bwd="plain", **kw)
    plain_maps = call(V, Qs, P, lens, gv, gq, api="plain", api_bwd="maps", **kw)
    check(plain, o, mode, "plain")
    for k in KEYS:
        assert same_bits(maps[k], plain[k]), ("maps", k)
        assert same_bits(maps_plain[k], plain[k]), ("forward_maps + backward", k)
        assert same_bits(plain_maps[k], plain[k]), ("forward + backward_maps", k)

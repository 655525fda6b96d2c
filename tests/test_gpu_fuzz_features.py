"""GPU: the length-masked (*_len) and map-gradient (*_maps) entry points over the shapes of tests/test_gpu_fuzz.py, against the
float64 oracle of tests/test_gpu_attention_grad.py -- every fused tile count, T up to the fused limit and past it, d up to 4096,
one to three levels, single samples, and tiny or odd d on the general path, where the plain call alone was swept before.

Per shape (seeded): lengths cycling through 1, T, T - 1 and the out-of-range 0, -2, T + 3 (clamped into [1, T] on the device);
pad rows of zeros on half the shapes and of finite junk (drawn like the question rows, from another seed) on the other half;
random G_av and G_aq, the latter non-zero in its pad slots.  Three call pairs each: forward_len + backward_len, forward_maps_len + backward_maps_len, forward_maps + backward_maps.
Besides the tolerances of the plain fuzz, exact properties: a_q, C and dQ are 0 past each clamped length, coattn_infer_len is
forward_maps_len bit for bit, and lengths all at T give the unmasked call's bits.

The last tests run the exact mode's live-row machinery under the mask on both sides of its size limits (as
tests/test_gpu_edges.py does unmasked): there the row bitmap also drops the rows past each question's length."""
import random

import pytest
import torch

from oracle import coattn_oracle as O
from tests._hip import LAYOUTS
from tests.test_gpu_attention_grad import GRADS, call, oracle, same_bits
from tests.test_gpu_fuzz import BIAS_SCALE, EXACT_TOL, FWD_TOL, GRAD_TOL, _shapes
from vqa_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = _shapes()
FWD_KEYS = ("v", "q", "a_v", "a_q")


def clamp(lens, T):
    return [min(max(int(n), 1), T) for n in lens]


def inputs(B, N, T, d, L, seed, junk_pad):
    """V [B,d,N], L questions [B,T,d] (rows past each clamped length: zeros, or finite junk), parameters, upstream gradients of
    v / q and of the two maps, and the lengths as handed to the device (out-of-range values included)."""
    rng = random.Random(seed)
    special = [1, T, T - 1, 0, -2, T + 3]
    k0 = rng.randrange(len(special))
    lens = [special[(k0 + b) % len(special)] if b < len(special) else rng.randint(-2, T + 3) for b in range(B)]
    cl = clamp(lens, T)
    P = O.make_params(d, seed)
    V, Qs = O.make_inputs(B, N, T, d, seed + 10, lens=cl, scale_q=(2.0 / d) ** 0.5, L=L)
    if junk_pad:
        for l, q in enumerate(Qs):
            junk = torch.from_numpy(O.hash_normal((B, T, d), seed + 50 + l, (2.0 / d) ** 0.5)).float()
            for b, n in enumerate(cl):
                q[b, n:] = junk[b, n:]
    gv = torch.from_numpy(O.hash_normal((L, B, d), seed + 5)).float()
    gq = torch.from_numpy(O.hash_normal((L, B, d), seed + 6)).float()
    g_av = torch.from_numpy(O.hash_normal((L, B, N), seed + 7, 4.0)).float()
    g_aq = torch.from_numpy(O.hash_normal((L, B, T), seed + 8, 4.0)).float()
    return V, Qs, P, gv, gq, g_av, g_aq, lens


def c_ref(V, Qs, lens):
    """C = tanh(Q V) [L,B,T,N] in float64, rows t >= len_b zero (lens None: unmasked)"""
    C = torch.stack([torch.tanh(torch.einsum("btk,bkn->btn", q.double(), V.double())) for q in Qs])
    if lens is not None:
        for b, n in enumerate(lens):
            C[:, b, n:] = 0.
    return C


_ORACLE = {}


def references(idx):
    """the shape's inputs and its three float64 references (shared by the two mode ids)"""
    B, N, T, d, L = SHAPES[idx]
    seed = 3000 + B * 7 + N * 13 + T * 17 + d + L
    x = inputs(B, N, T, d, L, seed, junk_pad=idx % 2 == 1)
    if idx not in _ORACLE:
        V, Qs, P, gv, gq, g_av, g_aq, lens = x
        cl = clamp(lens, T)
        z_av, z_aq = torch.zeros_like(g_av), torch.zeros_like(g_aq)
        o_len = oracle(V, Qs, P, cl, gv, gq, z_av, z_aq)
        o_maps_len = oracle(V, Qs, P, cl, gv, gq, g_av, g_aq)
        o_maps = oracle(V, Qs, P, None, gv, gq, g_av, g_aq)
        o_len["C"] = o_maps_len["C"] = c_ref(V, Qs, cl)
        o_maps["C"] = c_ref(V, Qs, None)
        _ORACLE.clear()                                       # (one shape at a time: the d = 4096 references are large)
        _ORACLE[idx] = (o_len, o_maps_len, o_maps)
    return x, _ORACLE[idx]


def check(r, o, fwd_tol, grad_tol, what):
    r = dict(r, C=r["saved_views"]["C"])
    for k in FWD_KEYS + ("C",):
        if k not in r:
            continue
        e = (r[k].double().cpu() - o[k]).abs().max().item()
        assert e < fwd_tol, (what, k, e)
    for k in GRADS:
        ref = o[k]
        got = r[k].double().cpu().reshape(ref.shape)
        assert torch.isfinite(got).all(), (what, k)
        scale = max(ref.abs().max().item(), BIAS_SCALE if k in ("dw_v.bias", "dw_q.bias") else 1e-30)
        e = (got - ref).abs().max().item() / scale
        assert e < grad_tol, (what, k, e)


def zero_past_lengths(r, cl, what):
    C = r["saved_views"]["C"]
    for b, n in enumerate(cl):
        assert (C[:, b, n:] == 0).all(), (what, "C", b)
        assert (r["dQ"][:, b, n:] == 0).all(), (what, "dQ", b)
        if "a_q" in r:
            assert (r["a_q"][:, b, n:] == 0).all(), (what, "a_q", b)
    a_q = r["saved_views"]["a_q"]
    for b, n in enumerate(cl):
        assert (a_q[:, b, n:] == 0).all(), (what, "saved a_q", b)


@pytest.mark.parametrize("exact3", [False, True], ids=["fast16", "exact"])
@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=["B%d_N%d_T%d_d%d_L%d" % s for s in SHAPES])
def test_masked_and_map_calls_vs_oracle(idx, exact3):
    B, N, T, d, L = SHAPES[idx]
    impls = ["general"] if exact3 else []
    if _lib.load().coattn_fused_supported(B, N, T, d, L, 0):
        impls.append("fused")
    if not impls:
        pytest.skip("general-shape path only: one arithmetic (exact), swept under the exact id")
    (V, Qs, P, gv, gq, g_av, g_aq, lens), (o_len, o_maps_len, o_maps) = references(idx)
    cl = clamp(lens, T)
    mode = "exact" if exact3 else "fast16"
    fwd_tol, grad_tol = (EXACT_TOL, EXACT_TOL) if exact3 else (FWD_TOL, GRAD_TOL)
    full = [T] * B
    for impl in impls:
        for layout in LAYOUTS:
            kw = dict(mode=mode, impl=impl, layout=layout)
            what = "%s/%s" % (impl, layout)
            r_len = call(V, Qs, P, lens, gv, gq, api="plain", **kw)
            check(r_len, o_len, fwd_tol, grad_tol, what + " forward_len + backward_len")
            zero_past_lengths(r_len, cl, what + " _len")
            r_ml = call(V, Qs, P, lens, gv, gq, g_av, g_aq, api="maps", **kw)
            check(r_ml, o_maps_len, fwd_tol, grad_tol, what + " forward_maps_len + backward_maps_len")
            zero_past_lengths(r_ml, cl, what + " _maps_len")
            r_m = call(V, Qs, P, None, gv, gq, g_av, g_aq, api="maps", **kw)
            check(r_m, o_maps, fwd_tol, grad_tol, what + " forward_maps + backward_maps")
            # coattn_infer_len: the saving forward's maps and outputs, bit for bit
            r_i = call(V, Qs, P, lens, api="infer", **kw)
            for k in FWD_KEYS:
                assert same_bits(r_i[k], r_ml[k]), (what, "infer_len", k)
            # every length at T: the unmasked calls' bits
            r_mt = call(V, Qs, P, full, gv, gq, g_av, g_aq, api="maps", **kw)
            r_lt = call(V, Qs, P, full, gv, gq, api="plain", **kw)
            r_p = call(V, Qs, P, None, gv, gq, api="plain", **kw)
            for k in FWD_KEYS + tuple(GRADS):
                assert same_bits(r_mt[k], r_m[k]), (what, "maps_len at T", k)
                if k in r_p:
                    assert same_bits(r_lt[k], r_p[k]), (what, "len at T", k)


# ---- the live-row limits under the mask -----------------------------------------------------------------------------------------
LIVE_KEYS = ("dQ", "dW_v.weight", "dW_q.weight", "dw_v.weight", "dw_q.weight", "dW_v.bias", "dW_q.bias")


def _live_case(B, junk_pad, seed=61):
    N, T, d = 49, 26, 512
    lens = [[T, 1, T - 1, 0, -2, T + 3][b] if b < 6 else 1 + (7 * b) % T for b in range(B)]
    cl = clamp(lens, T)
    P = O.make_params(d, seed)
    V, Qs = O.make_inputs(B, N, T, d, seed + 10, lens=cl, scale_q=(2.0 / d) ** 0.5)
    if junk_pad:
        for l, q in enumerate(Qs):
            junk = torch.from_numpy(O.hash_normal((B, T, d), seed + 50 + l, (2.0 / d) ** 0.5)).float()
            for b, n in enumerate(cl):
                q[b, n:] = junk[b, n:]
    gv = torch.from_numpy(O.hash_normal((3, B, d), seed + 5)).float()
    gq = torch.from_numpy(O.hash_normal((3, B, d), seed + 6)).float()
    g_av = torch.from_numpy(O.hash_normal((3, B, N), seed + 7, 4.0)).float()
    g_aq = torch.from_numpy(O.hash_normal((3, B, T), seed + 8, 4.0)).float()
    return V, Qs, P, gv, gq, g_av, g_aq, lens


def _fused_vs_general(a, b, what):
    assert (a["v"] - b["v"]).abs().max().item() < 1e-5 and (a["q"] - b["q"]).abs().max().item() < 1e-5, what
    for k in LIVE_KEYS:
        assert (a[k] - b[k]).abs().max().item() <= 2e-5 * max(1e-3, b[k].abs().max().item()), (what, k)


@pytest.mark.parametrize("junk_pad", [False, True], ids=["zero_pad", "junk_pad"])
@pytest.mark.parametrize("B", [315, 330, 520, 631])
def test_masked_live_row_paths_on_both_sides_of_their_limits(B, junk_pad):
    """B T = 8,190 (the largest gathered map), 8,580 and 13,520 (the bitmap with the host's dense plan), 16,406 (just past the
    bitmap's 16,384 rows: no bitmap).  Masked fused against masked general (which has no bitmap), and repeatable bit for bit."""
    V, Qs, P, gv, gq, _, _, lens = _live_case(B, junk_pad)
    a = call(V, Qs, P, lens, gv, gq, mode="exact", impl="fused", api="plain")
    g = call(V, Qs, P, lens, gv, gq, mode="exact", impl="general", api="plain")
    _fused_vs_general(a, g, (B, junk_pad))
    a2 = call(V, Qs, P, lens, gv, gq, mode="exact", impl="fused", api="plain")
    for k in ("v", "q") + LIVE_KEYS:
        assert same_bits(a[k], a2[k]), (B, junk_pad, k)
    for b, n in enumerate(clamp(lens, 26)):
        assert (a["dQ"][:, b, n:] == 0).all(), b


def test_masked_maps_live_row_path_at_the_gathered_map_limit():
    V, Qs, P, gv, gq, g_av, g_aq, lens = _live_case(315, True)
    a = call(V, Qs, P, lens, gv, gq, g_av, g_aq, mode="exact", impl="fused", api="maps")
    g = call(V, Qs, P, lens, gv, gq, g_av, g_aq, mode="exact", impl="general", api="maps")
    _fused_vs_general(a, g, "maps_len")
    for k in ("a_v", "a_q"):
        assert (a[k] - g[k]).abs().max().item() < 1e-5, k
    a2 = call(V, Qs, P, lens, gv, gq, g_av, g_aq, mode="exact", impl="fused", api="maps")
    for k in ("v", "q", "a_v", "a_q") + LIVE_KEYS:
        assert same_bits(a[k], a2[k]), k

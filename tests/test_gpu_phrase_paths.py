"""GPU: every kernel-selection branch of csrc/phrase.hip against the float64 oracle (oracle/net_oracle.py), through the
C-ABI runner of tests/_phrase.py: scalar / vector im2col, the general GEMM (dense and with k bands), gemm_w, gemm_tn with
its bias-sum workgroups, the general split-K weight gradient, gemm_bf_tn and its refusals; requested-output variants,
accumulate = 1, the saved-state contract, argmax ties, non-finite inputs and the argument checks.

Bounds (those of tests/test_gpu_phrase.py): forward |err| < 1e-5 (exact) / 5e-5 (tolerance mode); gradients
max|err| / max|ref| under the same numbers; bf16 mode 3e-2 forward, 1e-1 relative L2 on the gradients.

Which kernel a case reaches is stated in its id and rests on these rules (M = B T rows, N = K = 3E):
  im2col          vector iff E % 4 == 0 and X, Xcat 16-byte aligned (phrase.hip build_operands), else scalar
  Z, dXcat        gemm_w iff E % 128 == 0 and gemm_w_supported: M >= 128, or any M for Z in the tolerance mode (its FP16
                  pieces and range report live in that kernel: "a lone partial tile"); dXcat also needs dX != NULL.
                  Else the general GEMM of gemm.hip, with k bands iff E % 128 == 0.  In the fp32 modes gemm_w runs
                  128-column tiles at every E (E / 128 tiles per band); its 256-column tile and gemm_bf.hip
                  (gemm_bf_supported: M >= 256, N % 256 == 0) belong to the bf16 mode
  dWcat           gemm_tn (tile mask, mask_blk = E / 128, bias sums by extra workgroups of the launch: TnReduce) iff
                  E % 128 == 0 and gemm_tn_supported: M >= 16; in the bf16 mode gemm_bf_tn instead iff
                  gemm_bf_tn_supported: 3E % 256 == 0, M % 32 == 0, mask_blk even.  Else three general split-K launches
                  and phrase_unpack_db_kernel
The library's launch marks (coattn_profile_begin / _end) do not cover the phrase calls, so the path is not asserted."""
import ctypes as C

import pytest
import torch

from oracle import coattn_oracle as O
from tests import _phrase as P

pytestmark = pytest.mark.gpu

EXACT, FAST = 0, P.FAST16
MODES = [pytest.param(EXACT, id="exact"), pytest.param(FAST, id="tolerance")]
TOL = {EXACT: 1e-5, FAST: 5e-5}


def _rel(a, r):
    return (a.detach().cpu().double() - r).abs().max().item() / max(r.abs().max().item(), 1e-30)


def _errors(res, ora):
    """forward absolute error and max|err| / max|ref| of every gradient the call produced"""
    e = {"fwd": (res["out"].cpu().double() - ora["out"]).abs().max().item()}
    if res["dx"] is not None:
        e["dx"] = _rel(res["dx"], ora["dx"])
    if res["grads"] is not None:
        for k in P.PKEYS:
            e[k] = _rel(res["grads"][k], ora["grads"][k])
    return e


def _report(tag, shape, flags, e):
    print("phrase_paths %s %s %s" % (tag, shape, {EXACT: "exact", FAST: "tolerance", P.BF16: "bf16"}[flags]),
          {k: "%.1e" % v for k, v in e.items()})


def _bits_equal(a, b):
    return a is b or torch.equal(a.view(torch.int32), b.view(torch.int32))


def _same_bits(r0, r1, what=("out", "dx", "grads")):
    for k in what:
        if k == "grads":
            for n in P.PKEYS:
                assert _bits_equal(r0["grads"][n], r1["grads"][n]), n
        else:
            assert _bits_equal(r0[k], r1[k]), k


# ---- a. path sweep ------------------------------------------------------------------------------------------------------
# (shape, x_offset_floats, modes, expected path).  M = B T.
BOTH = (EXACT, FAST)
SWEEP = [
    # scalar im2col by size: E % 4 != 0 (build_operands); general dense GEMM, three split-K launches, unpack_db
    ((2, 5, 6), 0, BOTH, "im2col_scalar_E6-general_dense"),
    ((3, 7, 7), 0, BOTH, "im2col_scalar_E7-general_dense"),
    ((1, 1, 1), 0, BOTH, "im2col_scalar_E1-general_dense"),
    ((2, 4, 9), 0, BOTH, "im2col_scalar_E9-general_dense"),
    # scalar im2col by alignment: E % 4 == 0 but X is not 16-byte aligned
    ((2, 5, 8), 1, BOTH, "im2col_scalar_misaligned1-general_dense"),
    ((2, 5, 8), 2, BOTH, "im2col_scalar_misaligned2-general_dense"),
    ((2, 5, 8), 3, BOTH, "im2col_scalar_misaligned3-general_dense"),
    # E = 128, one 128-column tile per band, mask_blk = 1.  gemm_w_supported: M >= 128 -> 127 rows take the general GEMM
    # with k bands in the exact mode (the tolerance mode's Z: gemm_w at any M); gemm_tn from M >= 16, K = M odd
    ((127, 1, 128), 0, BOTH, "M127_E128-Z_dX_general_kbands(exact)-tn_K127"),
    ((128, 1, 128), 0, BOTH, "M128_E128-gemm_w_one_full_tile-tn_K128"),
    ((43, 3, 128), 0, BOTH, "M129_T3_E128-gemm_w_partial_row_tile-tn_K129"),
    ((131, 1, 128), 0, BOTH, "M131_T1_E128-gemm_w_all_taps_padding-tn_K131"),
    ((3, 43, 128), 0, BOTH, "M129_T43_E128-gemm_w_partial_row_tile-tn_K129"),
    ((257, 1, 128), 0, BOTH, "M257_E128-gemm_w_three_row_tiles-tn_K257"),
    # E = 256: two 128-column tiles per band, mask_blk = 2
    ((43, 3, 256), 0, BOTH, "M129_E256-gemm_w_two_tiles_per_band-tn_mask2"),
    ((8, 25, 256), 0, BOTH, "M200_E256-gemm_w_two_tiles_per_band-tn_mask2"),
    ((24, 11, 256), 0, BOTH, "M264_E256-gemm_w_two_tiles_per_band-tn_mask2"),
    # E = 384 / 640: three / five tiles per band, mask_blk = 3 / 5 (odd)
    ((43, 3, 384), 0, BOTH, "M129_E384-gemm_w_three_tiles_per_band-tn_mask3"),
    ((27, 5, 640), 0, BOTH, "M135_E640-gemm_w_five_tiles_per_band-tn_mask5"),
    # tolerance mode below 128 rows: gemm_w_supported admits any M for the FP16-piece forward ("a lone partial tile");
    # dXcat (bf16 pieces) stays on the general GEMM with k bands; M < 16: gemm_tn_supported refuses (K >= 16) -> three general
    # split-K launches at E % 128 == 0
    ((1, 1, 128), 0, (FAST,), "M1_E128-Z_gemm_w_lone_partial_tile-dW_general_splitk"),
    ((1, 2, 256), 0, (FAST,), "M2_E256-Z_gemm_w_lone_partial_tile-dW_general_splitk"),
    ((3, 5, 128), 0, (FAST,), "M15_E128-Z_gemm_w_lone_partial_tile-dW_general_splitk"),
]
SWEEP_PARAMS = [pytest.param(shape, off, flags, id="%s-%s" % (path, "exact" if flags == EXACT else "tolerance"))
                for shape, off, modes, path in SWEEP for flags in modes]


@pytest.mark.parametrize("shape,off,flags", SWEEP_PARAMS)
def test_phrase_path_sweep(shape, off, flags):
    """Forward, dx and the six parameter gradients of one selection branch against the float64 oracle."""
    sd, x, g, ora = P.case(*shape, 100 + shape[2])
    res = P.run_phrase(x, sd, g, flags=flags, x_offset_floats=off)
    e = _errors(res, ora)
    _report("sweep", shape, flags, e)
    assert res["out"].shape == shape
    assert e["fwd"] < TOL[flags], e
    assert max(v for k, v in e.items() if k != "fwd") < TOL[flags], e
    assert res["status"][0] == 0, res["status"]          # (tolerance mode: nothing left the FP16-piece range)


# ---- b. requested-output variants ---------------------------------------------------------------------------------------
VARIANT_SHAPES = [(43, 3, 128), (12, 11, 256), (2, 5, 6)]
shapes = pytest.mark.parametrize("shape", VARIANT_SHAPES, ids=lambda s: "B%d_T%d_E%d" % s)
modes = pytest.mark.parametrize("flags", MODES)


@shapes
@modes
def test_phrase_without_dx(shape, flags):
    """dX = NULL (frozen embedding): the backward builds Wcat with phrase_pack_w_kernel and skips dXcat / col2im; the
    parameter gradients equal the oracle's and, dWcat being independent of the dXcat kernel, the bits of the full call's."""
    sd, x, g, ora = P.case(*shape, 100 + shape[2])
    res = P.run_phrase(x, sd, g, flags=flags, need_dx=False, poison=True)
    full = P.run_phrase(x, sd, g, flags=flags, need_dx=True)
    assert res["dx"] is None
    e = _errors(res, ora)
    _report("no_dx", shape, flags, e)
    assert max(e.values()) < TOL[flags], e
    _same_bits(res, full, what=("out", "grads"))


@shapes
def test_phrase_without_saved(shape):
    """saved = NULL (inference): the exact forward's bits; with COATTN_FLAG_FAST16 too -- the status words live in `saved`,
    so without it the forward runs the exact product (the documented fallback)."""
    sd, x, g, ora = P.case(*shape, 100 + shape[2])
    keep = P.run_phrase(x, sd, flags=EXACT)
    for flags in (EXACT, FAST):
        res = P.run_phrase(x, sd, flags=flags, need_saved=False, poison=True)
        assert res["amax"] is None
        assert _bits_equal(res["out"], keep["out"]), flags
    assert (keep["out"].cpu().double() - ora["out"]).abs().max().item() < TOL[EXACT]


@shapes
@pytest.mark.parametrize("frozen", ["x", "weights"])
def test_phrase_module_frozen_inputs(shape, frozen):
    """Through vqa_amd.modules.PhraseConvPool: x without a gradient and trainable weights (dX = NULL in the backward), and
    frozen weights with x.requires_grad."""
    import vqa_amd  # noqa: F401
    from vqa_amd.modules import PhraseConvPool
    B, T, E = shape
    sd, x, g, ora = P.case(*shape, 100 + E)
    mod = PhraseConvPool(E)
    mod.load_state_dict(sd)
    mod = mod.cuda()
    mod.fast_products = False
    xg = x.cuda()
    if frozen == "weights":
        for p in mod.parameters():
            p.requires_grad_(False)
        xg.requires_grad_(True)
    y = mod(xg)
    y.backward(g.cuda())
    assert (y.detach().cpu().double() - ora["out"]).abs().max().item() < TOL[EXACT]
    if frozen == "weights":
        assert all(p.grad is None for p in mod.parameters())
        assert _rel(xg.grad, ora["dx"]) < TOL[EXACT]
    else:
        assert xg.grad is None
        for k, p in mod.named_parameters():
            assert _rel(p.grad, ora["grads"][k]) < TOL[EXACT], k


# ---- c. accumulate = 1 --------------------------------------------------------------------------------------------------
def _g0(ora, seed):
    """hash-normal start values at each gradient's own magnitude (its rms)"""
    return {k: torch.from_numpy(O.hash_normal(tuple(v.shape), seed + i, v.pow(2).mean().sqrt().item())).float()
            for i, (k, v) in enumerate(ora["grads"].items())}


@pytest.mark.parametrize("shape,flags", [
    pytest.param((43, 3, 128), EXACT, id="B43_T3_E128-gemm_tn_TnReduce-exact"),
    pytest.param((43, 3, 128), FAST, id="B43_T3_E128-gemm_tn_TnReduce-tolerance"),
    pytest.param((2, 5, 20), EXACT, id="B2_T5_E20-unpack_kernels-exact"),
    pytest.param((2, 5, 20), FAST, id="B2_T5_E20-unpack_kernels-tolerance"),
    pytest.param((16, 26, 256), P.BF16, id="B16_T26_E256-gemm_bf_tn-bf16")])
def test_phrase_accumulate(shape, flags):
    """accumulate = 1 adds to what the gradient buffers hold: G0 + grad, neither grad (accumulate ignored) nor G0 + 2 grad
    (added twice).  fp32 modes: max|err| / max|ref| under the sweep's bound, both alternatives off by more than 100 x the
    bound.  bf16 mode: relative L2 < 1e-1; both alternatives cannot be 100 x 1e-1 = 10 away at once (||G0|| and ||grad||
    would each have to exceed 10 ||G0 + grad||), so with ||G0|| = ||grad|| (independent: ||G0 + grad|| ~ sqrt(2) ||grad||,
    each alternative ~0.7 away) they are required to be more than 5 x the bound away."""
    sd, x, g, ora = P.case(*shape, 100 + shape[2])
    G0 = _g0(ora, 900)
    res = P.run_phrase(x, sd, g, flags=flags, accumulate=1, grads_init=G0)
    bf = flags == P.BF16
    worst = {}
    for k in P.PKEYS:
        got, g0, gr = res["grads"][k].cpu().double(), G0[k].double(), ora["grads"][k]
        ref = g0 + gr
        if bf:
            dist = lambda a: ((got - a).norm() / ref.norm()).item()     # noqa: E731
            bound, far = 1e-1, 5
        else:
            dist = lambda a: (got - a).abs().max().item() / ref.abs().max().item()     # noqa: E731
            bound, far = TOL[flags], 100
        worst[k] = dist(ref)
        assert dist(ref) < bound, (k, dist(ref))
        assert dist(gr) > far * bound and dist(g0 + 2 * gr) > far * bound, (k, dist(gr), dist(g0 + 2 * gr))
    _report("accumulate", shape, flags, worst)


# ---- d. saved-state contract and repeatability ---------------------------------------------------------------------------
@shapes
@modes
def test_phrase_saved_state_and_repeat(shape, flags):
    """The backward depends on X, out, saved, g and the parameters only: NaN-filled outputs, `saved` and workspaces (the
    backward's a fresh one), or one workspace shared by both calls and overwritten in between, change no bit of out, dx or
    the six gradients; three runs give the same bits (fixed split-K summation order); nothing is NaN."""
    sd, x, g, _ = P.case(*shape, 100 + shape[2])
    clean = P.run_phrase(x, sd, g, flags=flags)
    for t in [clean["out"], clean["dx"]] + list(clean["grads"].values()):
        assert torch.isfinite(t).all()
    for i in range(3):
        _same_bits(clean, P.run_phrase(x, sd, g, flags=flags, poison=True))
    _same_bits(clean, P.run_phrase(x, sd, g, flags=flags, poison=True, share_ws=True))
    assert torch.equal(clean["amax"], P.run_phrase(x, sd, flags=flags, poison=True)["amax"])


# ---- e. ties ------------------------------------------------------------------------------------------------------------
TIE_SHAPES = pytest.mark.parametrize("shape", [(43, 3, 128), (2, 5, 20)], ids=lambda s: "B%d_T%d_E%d" % s)


def _check_vs(res, ora, flags, tag, shape):
    e = _errors(res, ora)
    _report(tag, shape, flags, e)
    assert max(e.values()) < TOL[flags], e


@TIE_SHAPES
@modes
def test_phrase_tie_all_zero_sample(shape, flags):
    """Zero biases and an all-zero sample: Z == 0 there, a three-way tie in every group -> argmax 0 (first of equals, as
    MaxPool), and the gradients -- bias gradients included -- go to the first channel of each group as the oracle's do."""
    B, T, E = shape
    sd, x, g, _ = P.case(*shape, 100 + E)
    sd = dict(sd)
    for k in P.PKEYS[1::2]:
        sd[k] = torch.zeros(E)
    x = x.clone()
    x[1] = 0
    ora = P.oracle_phrase(x, sd, g)
    res = P.run_phrase(x, sd, g, flags=flags, poison=True)
    assert (res["out"][1] == 0).all()
    assert (res["amax"][1] == 0).all()
    assert (res["amax"] <= 2).all()
    _check_vs(res, ora, flags, "tie_zero", shape)


@TIE_SHAPES
@modes
def test_phrase_tie_equal_bias(shape, flags):
    """Non-zero biases equal inside every pooled group (groups straddle b1 | b2 | b3) and the last two rows of every
    sample zero: the last row's Z is the bias exactly (its taps x[T-2], x[T-1], padding are zeros) -> argmax 0 there."""
    B, T, E = shape
    sd, x, g, _ = P.case(*shape, 100 + E)
    sd = dict(sd)
    bcat = torch.from_numpy(O.hash_unit((E,), 77, 0.5)).float().repeat_interleave(3)      # bcat[3e + j] = v[e]
    assert bcat.abs().min() > 0
    for i, k in enumerate(P.PKEYS[1::2]):
        sd[k] = bcat[i * E:(i + 1) * E].clone()
    x = x.clone()
    x[:, T - 2:] = 0
    ora = P.oracle_phrase(x, sd, g)
    res = P.run_phrase(x, sd, g, flags=flags, poison=True)
    assert (res["amax"][:, T - 1] == 0).all()
    assert (res["out"][:, T - 1].cpu().double() - torch.tanh(bcat[::3].double())).abs().max().item() < TOL[flags]
    _check_vs(res, ora, flags, "tie_bias", shape)


# ---- f. non-finite inputs (exact mode, forward) --------------------------------------------------------------------------
# (shape, t0, k bands?)  (3,6,128): M = 18 -> general GEMM with k bands; (43,3,128): gemm_w; (3,6,20): dense general GEMM
NONFINITE = [pytest.param((3, 6, 128), 3, True, id="B3_T6_E128-general_kbands"),
             pytest.param((43, 3, 128), 1, True, id="B43_T3_E128-gemm_w"),
             pytest.param((3, 6, 20), 3, False, id="B3_T6_E20-general_dense")]


def _plant(shape, t0, value):
    sd, x, _, _ = P.case(*shape, 100 + shape[2])
    clean = P.oracle_phrase(x, sd)["out"]
    x = x.clone()
    x[1, t0, 5] = value
    rows = torch.zeros(shape[:2], dtype=torch.bool)
    rows[1, max(0, t0 - 1):t0 + 2] = True                 # the rows whose n-grams read x[1, t0]
    return sd, x, clean, rows


@pytest.mark.parametrize("shape,t0,kbands", NONFINITE)
def test_phrase_nan_input_propagates(shape, t0, kbands):
    """One NaN at x[1, t0, 5]: every output the oracle makes NaN is NaN (max(finite, NaN) = NaN as MaxPool: the pool takes
    a later NaN channel -- groups that straddle an n-gram boundary have a finite first channel); every other sample and every
    row outside t0-1 .. t0+1 is finite and within tolerance.  With k bands the zero tap blocks are never read and the NaN
    set equals the oracle's; the dense contraction also computes 0 . NaN for the absent taps, so there the set may be a
    superset confined to those three rows (a known property of the dense path)."""
    sd, x, clean, rows = _plant(shape, t0, float("nan"))
    ora = P.oracle_phrase(x, sd)["out"]
    want = torch.isnan(ora)
    assert want.any() and not (want & ~rows[..., None]).any()
    out = P.run_phrase(x, sd, flags=EXACT, poison=True)["out"].cpu()
    got = torch.isnan(out)
    lost = want & ~got
    print("phrase_paths nan", shape, "oracle NaN", int(want.sum()), "hip NaN", int(got.sum()), "lost at", lost.nonzero()[:8].tolist())
    assert not lost.any(), lost.nonzero()[:8].tolist()
    assert not (got & ~rows[..., None]).any()
    if kbands:
        assert torch.equal(got, want)
    ok = ~got
    assert torch.isfinite(out[ok]).all()
    assert (out[ok].double() - ora[ok]).abs().max().item() < TOL[EXACT]
    away = ~rows[..., None].expand_as(out)
    assert (out[away].double() - clean[away]).abs().max().item() < TOL[EXACT]


@pytest.mark.parametrize("shape,t0,kbands", NONFINITE)
def test_phrase_inf_input_is_confined(shape, t0, kbands):
    """One +inf at x[1, t0, 5].  The float64 oracle saturates: conv -> +-inf, tanh -> +-1, so it has no non-finite output
    (printed; "every element the oracle makes non-finite" is then the empty set, and still asserted).  The kernels differ:
    the general GEMM of gemm.hip carries the inf through and the saturated tanh gives the oracle's +-1; gemm_w's three-piece
    split turns it into NaN (inf - inf in the residual; include/coattn.h: "inf / NaN inputs give inf / NaN outputs"); the
    dense contraction adds 0 . inf = NaN for the absent taps.  Held on every path: a non-finite output lies in rows
    t0-1 .. t0+1 of sample 1 and, with k bands, in a group that reads x[1, t0, 5]; every finite output -- the saturated
    ones included -- is within tolerance of the oracle."""
    sd, x, clean, rows = _plant(shape, t0, float("inf"))
    ora = P.oracle_phrase(x, sd)["out"]
    xn = x.clone()
    xn[1, t0, 5] = float("nan")
    touched = torch.isnan(P.oracle_phrase(xn, sd)["out"])          # the outputs whose groups read x[1, t0, 5]
    out = P.run_phrase(x, sd, flags=EXACT, poison=True)["out"].cpu()
    bad = ~torch.isfinite(out)
    print("phrase_paths inf", shape, "oracle non-finite", int((~torch.isfinite(ora)).sum()), "hip non-finite", int(bad.sum()),
          "touched", int(touched.sum()))
    assert not (~torch.isfinite(ora) & ~bad).any()
    assert not (bad & ~rows[..., None]).any()
    if kbands:
        assert not (bad & ~touched).any()
    ok = ~bad
    assert (out[ok].double() - ora[ok]).abs().max().item() < TOL[EXACT]
    away = ~rows[..., None].expand_as(out)
    assert (out[away].double() - clean[away]).abs().max().item() < TOL[EXACT]


# ---- g. bf16 mode at the shapes gemm_bf_tn refuses -----------------------------------------------------------------------
# (6,26,128): 3E = 384 is no multiple of 256; (16,26,384): 3E = 1152 neither (E / 256 = 1 with a remainder);
# (27,5,640): mask_blk = 5 is odd and M = 135 no multiple of 32 -> gemm_tn in single-piece mode for dWcat at all three
@pytest.mark.parametrize("shape", [(6, 26, 128), (16, 26, 384), (27, 5, 640)], ids=lambda s: "B%d_T%d_E%d" % s)
def test_phrase_bf16_mode_refused_shapes(shape):
    sd, x, g, ora = P.case(*shape, 100 + shape[2])
    res = P.run_phrase(x, sd, g, flags=P.BF16, poison=True)
    y32 = P.run_phrase(x, sd, flags=EXACT)["out"]
    assert (res["out"] - y32).abs().max().item() > 0
    fwd = (res["out"].cpu().double() - ora["out"]).abs().max().item()

    def rel(a, r):      # relative L2: a reduced-precision max-pool may route single gradients to another channel
        return ((a.cpu().double() - r).norm() / r.norm()).item()
    e = {"fwd": fwd, "dx": rel(res["dx"], ora["dx"])}
    for k in P.PKEYS:
        e[k] = rel(res["grads"][k], ora["grads"][k])
    _report("bf16", shape, P.BF16, e)
    assert fwd < 3e-2, e
    assert max(v for k, v in e.items() if k != "fwd") < 1e-1, e


# ---- h. argument checks -------------------------------------------------------------------------------------------------
def _raw_call(which, B=2, T=3, E=8, dtype=None, null_param=False, null_grad=False):
    """One C-ABI call on small sentinel-filled buffers (sizes as given, buffers for (2,3,8) at most: the checks precede any
    access).  Returns (rc, message, buffers, their contents before the call)."""
    from vqa_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    S = 1234.5
    mk = lambda n: torch.full((n,), S, device=dev)     # noqa: E731
    x, out, g, dx = mk(48), mk(48), mk(48), mk(48)
    saved, ws = mk(4096), mk(1 << 16)
    ps = [mk(8 * 8 * 3) for _ in range(6)]
    grads = [mk(8 * 8 * 3) for _ in range(6)]
    pp = [t.data_ptr() for t in ps]
    gp = [t.data_ptr() for t in grads]
    if null_param:
        pp[3] = None
    if null_grad:
        gp[4] = None
    p, pg = _lib.PhraseParams(*pp), _lib.PhraseParamGrads(*gp)
    dtype = _lib.F32 if dtype is None else dtype
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if which == "forward":
        rc = lib.coattn_phrase_forward(x.data_ptr(), C.byref(p), out.data_ptr(), saved.data_ptr(), ws.data_ptr(), B, T, E,
                                       dtype, 0, stream)
    else:
        rc = lib.coattn_phrase_backward(x.data_ptr(), C.byref(p), out.data_ptr(), saved.data_ptr(), g.data_ptr(),
                                        dx.data_ptr(), C.byref(pg), 0, ws.data_ptr(), B, T, E, dtype, 0, stream)
    msg = lib.coattn_last_error().decode()
    torch.cuda.synchronize()
    untouched = all(bool((t == S).all()) for t in [x, out, g, dx, saved, ws] + ps + grads)
    return rc, msg, untouched


@pytest.mark.parametrize("which", ["forward", "backward"])
@pytest.mark.parametrize("bad", [dict(dtype=1), dict(B=0), dict(null_param=True), dict(B=40000, T=4000, E=8)],
                         ids=["dtype_not_f32", "B0", "null_parameter", "B_T_3E_beyond_2^31"])
def test_phrase_argument_checks(which, bad):
    """A refused call returns a negative code, leaves a message in coattn_last_error() and launches nothing: every buffer
    it was handed still holds its sentinel."""
    rc, msg, untouched = _raw_call(which, **bad)
    assert rc < 0 and msg, (rc, msg)
    assert untouched


def test_phrase_backward_null_gradient_pointer():
    rc, msg, untouched = _raw_call("backward", null_grad=True)
    assert rc < 0 and "gradient" in msg, (rc, msg)
    assert untouched
    rc, msg, untouched = _raw_call("backward")            # (the same call with every pointer set goes through)
    assert rc == 0 and not untouched

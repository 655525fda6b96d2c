"""GPU: every kernel form, shape edge and descriptor field of the GEMM layer's C-ABI -- coattn_gemm_f32 / coattn_gemm_bf16
(csrc/gemm.hip), coattn_linear_forward (gemm_w.hip / gemm_w_body.h, gemm_h2.hip, gemm_bf.hip) and
coattn_linear_weight_grad (gemm_tn.hip, gemm_bf.hip) -- against a float64 reference of include/coattn.h's contract on the
operands the mode multiplies, at the smallest shapes that reach each branch.

Which kernel a row reaches is stated by the mirrors of tests/_gemm.py (tests/test_gemm_cpu.py pins them at every
threshold); every row names its form and is held against the mirror when this module is collected.  Every call goes through
the runners of tests/_gemm.py: each buffer sits in a marker-filled arena of exactly its size, the pads of the operands hold
NaN, and after the call the margins hold the marker, C's arena holds it outside the view, and no cell of the result is
non-finite unless the case plants one.

Bounds, of max|ref| (absolute where act = tanh) -- the project's own (tests/test_gpu_gemm.py), none of a row's own:
coattn_gemm_f32, the exact linear call and weight gradient 2e-6; COATTN_FLAG_SPLIT2 2e-6 against the two-piece product and
below 3e-5 against the true one; COATTN_FLAG_F16PAIR 4e-6; coattn_gemm_bf16 2e-6 against the product of the rounded
operands; COATTN_FLAG_BF16_PROJ on the linear calls 2e-5 against the same.  tests/test_gemm_cpu.py shows on the CPU, row by
row, that float32 arithmetic meets each bound with half of it to spare and that the neighbouring mode misses it five times
over.  Every row prints its error before it asserts."""
import functools

import pytest
import torch

from tests import _gemm as X

pytestmark = pytest.mark.gpu

LAYOUTS = (("k", "k"), ("k", "n"), ("m", "k"), ("m", "n"))          # (A contiguous along, B contiguous along)
TOL = 2e-6


# ---- (a) the general GEMM: shape edges per kernel form -----------------------------------------------------------------------
# rows: (id, entry point "f32" / "bf16", the form the mirror must name, gemm_case arguments)
GEMM_ROWS = []


def _row(ident, entry, form, **kw):
    GEMM_ROWS.append((ident, entry, form, kw))


def _edges(tag, entry, form, base, Ms, Ns, Ks, **kw):
    """Every value of an edge list once, the other two extents at the form's interior value."""
    for i, M in enumerate(Ms):
        _row("%s-M%d" % (tag, M), entry, form, **dict(base, M=M, seed=i, **kw))
    for i, N in enumerate(Ns):
        _row("%s-N%d" % (tag, N), entry, form, **dict(base, N=N, seed=10 + i, **kw))
    for i, K in enumerate(Ks):
        _row("%s-K%d" % (tag, K), entry, form, **dict(base, K=K, seed=20 + i, **kw))


NV_N, NV_K = (1, 127, 128, 129), (1, 3, 15, 16, 17, 33)              # the non-vector forms: BK = 16
for form, Ms, M0, lay in (("f32_32", (1, 31, 32, 33, 64), 33, LAYOUTS[3]), ("f32_128", (65, 127, 129), 100, LAYOUTS[1])):
    base = dict(M=M0, N=70, K=19, a=lay[0], b=lay[1])
    _edges(form, "f32", form, base, Ms, NV_N, NV_K)
    _edges("bf16_exact_" + form, "bf16", "exact:" + form, base, Ms[-2:], NV_N[-1:], NV_K[-1:])
    for off in (1, 2, 3):                                            # operands 4, 8, 12 bytes off a 16-byte boundary
        for j, (a, b) in enumerate(LAYOUTS):
            offs = dict(a_off=off, b_off=off % 3 + 1, c_off=off, bn_off=off, bias_n=True)
            _row("%s-off%d-%s%s" % (form, off, a, b), "f32", form, **dict(base, K=20, a=a, b=b, seed=30 + off + 4 * j, **offs))
        # (K = 20, rows along k: only the operands' addresses keep the bf16 entry off its own kernels)
        _row("bf16_exact_%s-off%d" % (form, off), "bf16", "exact:" + form,
             **dict(base, K=20, a="k", b="k", a_off=off, b_off=off % 3 + 1, c_off=off, seed=50 + off))
VEC = dict(Ms=(128, 132, 260), Ns=(4, 128, 132), Ks=(4, 28, 32, 36, 68))          # the vector forms: BK = 32
for a, b in LAYOUTS:
    base = dict(M=132, N=132, K=36, a=a, b=b)
    _edges("vec128_%s%s" % (a, b), "f32", "vec128", base, **VEC)
    _edges("vec128_bf16_%s%s" % (a, b), "bf16", "vec128_bf16", base, **VEC)
    # 33 row tiles padded to 40 workgroups per column tile: the XCD-grouped tile order
    _row("vec128_%s%s-xcd" % (a, b), "f32", "vec128", M=4100, N=132, K=32, batch=2, a=a, b=b, xcd=True)
    _row("vec128_bf16_%s%s-xcd" % (a, b), "bf16", "vec128_bf16", M=4100, N=132, K=32, batch=2, a=a, b=b, xcd=True)
BF_K = (4, 32, 36)
_edges("bf16in_ak", "bf16", "bf16in_ak", dict(M=100, N=70, K=36, a="k", b="k"), (1, 31, 32, 33, 64, 65, 127), NV_N, BF_K)
_edges("bf16in_am_vec", "bf16", "bf16in_am_vec", dict(M=104, N=70, K=36, a="m", b="k", a_mdiv=52), (4, 52, 124), NV_N, BF_K)
_row("bf16in_am_vec-plain", "bf16", "bf16in_am_vec", M=100, N=70, K=36, a="m", b="k")
_edges("bf16in_am_scalar", "bf16", "bf16in_am_scalar", dict(M=98, N=70, K=36, a="m", b="k", a_mdiv=49), (1, 49, 127, 129, 147),
       NV_N, BF_K)
_row("bf16in_am_scalar-plain", "bf16", "bf16in_am_scalar", M=65, N=70, K=36, a="m", b="k")
_row("bf16in_am_scalar-xcd", "bf16", "bf16in_am_scalar", M=4100, N=132, K=32, batch=2, a="m", b="k", a_mdiv=49, xcd=True)
# (gemm_bf16in_kernel's other two forms take 32 row tiles only where an unused stride -- a_si, inner <= 1 -- keeps the shape off
#  the aligned path: the padded grid is the kernel's own code all the same)
_row("bf16in_am_vec-xcd", "bf16", "bf16in_am_vec", M=4100, N=132, K=32, batch=2, a="m", b="k", a_mdiv=52, a_si_odd=True, xcd=True)
_row("bf16in_ak-xcd", "bf16", "bf16in_ak", M=4100, N=132, K=32, batch=2, a="k", b="k", a_si_odd=True, xcd=True)

# ---- (b) every descriptor field on every form that honours it ------------------------------------------------------------------
ALL = dict(bias_n=True, bias_m=True, cin="n", beta=0.5, act=1, out_scale=2.5)


def _kb(K):
    """Three k bands inside [0, K], the middle one empty (lo == hi): multiples of 4."""
    q = K // 4 * 4
    h = q // 8 * 4
    return ((0, h), (h, h), (4, q))


def _fields(K):
    kb = _kb(K)
    f = {
        "bias_n": dict(bias_n=True), "bias_m": dict(bias_m=True), "cin_beta": dict(cin="n", beta=0.5), "tanh": dict(act=1),
        "out_scale": dict(out_scale=2.5), "all": dict(ALL),
        "cin_padded": dict(cin="n", cin_pad=3, beta=-1.5, out_scale=2.5),
        "cin_transposed": dict(cin="t", beta=0.5, bias_n=True), "cin_div": dict(cin="div", cin_mdiv=7, cin_pad=2, beta=2.0),
        "c_div": dict(c="div", c_mdiv=7), "c_div_cin": dict(c="div", c_mdiv=7, c_pad=1, cin="n", beta=0.5, out_scale=2.5),
        "c_transposed_cin_div": dict(c="t", cin="div", cin_mdiv=5, beta=1.0, act=1),
        "ksplit_short_last": dict(K=100, ksplit=48, batch=3), "ksplit_all": dict(K=100, ksplit=48, batch=3, **ALL),
        "inner_short_last": dict(inner=3, inner_total=7, batch=3), "inner_full": dict(inner=2, batch=2, bias_m=True),
        "b_imod": dict(inner=3, inner_total=7, batch=3, b_imod=2), "b_imod_inner1": dict(inner=1, inner_total=3, batch=3, b_imod=2),
        "inner_total_short_of_batch": dict(inner=1, inner_total=2, batch=3, bias_n=True),
        "inner_total_covers_batch": dict(inner=1, inner_total=3, batch=3, bias_n=True),
        "a_tab1": dict(a_tab=True, batch=1), "a_tab3": dict(a_tab=True, batch=3, bias_n=True), "a_tab8": dict(a_tab=True, batch=8),
        "b_tab3": dict(b_tab=True, batch=3), "c_tab1": dict(c_tab=True, batch=1), "c_tab3": dict(c_tab=True, batch=3, out_scale=2.5),
        "c_tab8": dict(c_tab=True, batch=8), "cin_tab3": dict(cin="n", cin_tab=True, beta=0.5, batch=3),
        "cin_tab8_c_tab8": dict(cin="t", cin_tab=True, c_tab=True, beta=0.5, batch=8),
        "all_tabs3": dict(a_tab=True, b_tab=True, c_tab=True, cin="n", cin_tab=True, beta=0.5, batch=3),
        "tabs_by_inner8": dict(a_tab=True, b_tab=True, by_inner=True, inner=3, inner_total=8, batch=3),
        "tabs_by_inner3": dict(a_tab=True, b_tab=True, by_inner=True, inner=3, batch=1),
        "kband1": dict(N=100, kband_n=128, kband=kb[2:], nan_outside=True),
        "kband2": dict(N=200, kband_n=128, kband=(kb[0], kb[2]), nan_outside=True, bias_n=True),
        "kband3_empty": dict(N=300, kband_n=128, kband=kb, nan_outside=True, bias_n=True, out_scale=2.5, act=1),
        "kband2_wide": dict(N=300, kband_n=256, kband=(kb[2], kb[0]), nan_outside=True),
        "kband3_ksplit": dict(N=300, K=100, ksplit=48, batch=3, kband_n=128, kband=((0, 52), (52, 52), (44, 100)), nan_outside=True,
                              bias_n=True),
    }
    if K % 4:                                                # (a k range of one row: the non-vector forms only)
        f["ksplit_last_of_one"] = dict(K=97, ksplit=48, batch=3)
    return f


# what gemm_bf16in_kernel honours itself; with every other field coattn_gemm_bf16 must leave it for the exact path
BF16IN_OWN = ("bias_n", "out_scale", "a_tab1", "a_tab3", "a_tab8", "c_div", "inner_total_covers_batch")
FIELD_BASES = (
    ("f32_32", "f32", "f32_32", dict(M=33, N=70, K=19, a="m", b="n")),
    ("f32_128", "f32", "f32_128", dict(M=100, N=70, K=19, a="k", b="n")),
    ("vec128_mk", "f32", "vec128", dict(M=132, N=132, K=36, a="m", b="k")),
    ("vec128_kn", "f32", "vec128", dict(M=132, N=132, K=36, a="k", b="n")),
    ("vec128_bf16_mn", "bf16", "vec128_bf16", dict(M=132, N=132, K=36, a="m", b="n")),
    ("vec128_bf16_kk", "bf16", "vec128_bf16", dict(M=132, N=132, K=36, a="k", b="k")),
    # the shape gemm_bf16in_kernel takes when the descriptor asks for nothing else: M = 127, A row-major, B along k
    ("bf16_m127", "bf16", None, dict(M=127, N=70, K=36, a="k", b="k")),
)
for tag, entry, form, base in FIELD_BASES:
    for j, (name, kw) in enumerate(_fields(base["K"]).items()):
        f = form or ("bf16in_ak" if name in BF16IN_OWN else "exact:f32_128")
        _row("%s-%s" % (tag, name), entry, f, **dict(base, seed=100 + j, **kw))
# the row splits on gemm_bf16in_kernel's m-contiguous forms, with the fields it honours together
_row("bf16in_am_scalar-own_fields", "bf16", "bf16in_am_scalar", M=147, N=130, K=36, batch=3, a="m", b="k", a_mdiv=49, a_pad=4, a_tab=True,
     bias_n=True, out_scale=2.5, c="div", c_mdiv=49)
_row("bf16in_am_vec-own_fields", "bf16", "bf16in_am_vec", M=104, N=130, K=36, batch=2, a="m", b="k", a_mdiv=52, a_pad=4, bias_n=True,
     out_scale=2.5, c="div", c_mdiv=52)
# the weight gradient over sample groups of one (grad_dw_sample_groups at B <= 32, channel-major V, d = 64): inner = 1 and
# inner_total = batch clip nothing, and the shape keeps gemm_bf16in_kernel
_row("bf16in_am_vec-sample_groups_of_one", "bf16", "bf16in_am_vec", M=64, N=64, K=196, batch=8, a="m", b="k", inner=1, inner_total=8)
_row("bf16in_am_scalar-kband", "bf16", "exact:f32_128", M=98, N=200, K=36, a="m", b="k", a_mdiv=49, kband_n=128, kband=((0, 16), (20, 36)),
     nan_outside=True)
_row("bf16in_am_vec-cin_tab", "bf16", "exact:f32_128", M=104, N=70, K=36, batch=2, a="m", b="k", a_mdiv=52, cin="n", cin_tab=True, beta=0.5)

GEMM_IDS = [r[0] for r in GEMM_ROWS]
assert len(set(GEMM_IDS)) == len(GEMM_IDS)


def gemm_row_case(kw, data=True):
    kw = dict(kw)
    kw.pop("xcd", None)
    return X.gemm_case(data=data, **kw)


def gemm_row_mirror(entry, kw):
    """(form, xcd_group) the mirror gives a row."""
    d = gemm_row_case(kw, data=False)
    if entry == "bf16":
        return X.gemm_bf16_kernel(**d), X.gemm_bf16_xcd_group(**d)
    return X.gemm_f32_kernel(**d)


for _id, _entry, _form, _kw in GEMM_ROWS:
    assert gemm_row_mirror(_entry, _kw) == (_form, bool(_kw.get("xcd"))), (_id, gemm_row_mirror(_entry, _kw))


def gemm_row_rounds(form):
    """Whether a form multiplies operands rounded to bf16."""
    return form.startswith("vec128_bf16") or form.startswith("bf16in")


@functools.lru_cache(maxsize=None)
def _gemm_ref(ident):
    _, _, form, kw = GEMM_ROWS[GEMM_IDS.index(ident)]
    d = gemm_row_case(kw)
    return d, X.gemm_reference(d, bf16=gemm_row_rounds(form))


def _bound(d, out, ref, tol, what):
    scale = 1.0 if d.get("act") == 1 else max(float(ref.abs().max()), 1e-9)
    err = float((out.double() - ref).abs().max()) / scale
    print("gemm_paths %s: %.2e (bound %.0e)" % (what, err, tol))
    assert err < tol, (what, err)


@pytest.mark.parametrize("ident", GEMM_IDS)
def test_gemm_form_edge_and_field(ident):
    _, entry, form, _ = GEMM_ROWS[GEMM_IDS.index(ident)]
    d, ref = _gemm_ref(ident)
    out = X.run_gemm(d, bf16=entry == "bf16")
    _bound(d, out, ref, TOL, ident)


# ---- (c) non-finite operands, per kernel form ----------------------------------------------------------------------------------
NONFINITE = [(i, e, f, k) for i, e, f, k in GEMM_ROWS if i in (
    "f32_32-M33", "f32_128-M127", "bf16_exact_f32_128-M129", "bf16in_ak-M65", "bf16in_am_vec-M124", "bf16in_am_scalar-M147",
    "vec128_kk-M260", "vec128_kn-M260", "vec128_mk-M260", "vec128_mn-M260",
    "vec128_bf16_kk-M260", "vec128_bf16_kn-M260", "vec128_bf16_mk-M260", "vec128_bf16_mn-M260")]
assert len(NONFINITE) == 14
NAN, INF, NAN_7F, NAN_FF = 0x7FC00000, 0x7F800000, 0x7FFFFFFF, 0xFFFFFFFF


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("ident", [r[0] for r in NONFINITE])
def test_gemm_nonfinite_operand_stays_in_its_row_and_column(ident):
    """One NaN (then one +inf) in one element of A makes exactly that row of C non-finite and leaves every other cell
    bit-identical to the clean run; the same for an element of B and its column; and the NaNs with every payload bit set
    (0x7FFFFFFF in A, 0xFFFFFFFF in B, one run) do what the canonical NaN does -- the bf16 staging keeps them NaN."""
    _, entry, form, kw = [r for r in NONFINITE if r[0] == ident][0]
    bf = entry == "bf16"
    M, N, K = kw["M"], kw["N"], kw["K"]
    m, ka, kb_, n = M - 2, K // 2, K - 1, N // 3
    clean = X.run_gemm(gemm_row_case(kw), bf16=bf)[0]
    for what, pokes, rows, cols in (("A nan", [("A", 0, m, ka, NAN)], [m], []), ("A inf", [("A", 0, m, ka, INF)], [m], []),
                                    ("B nan", [("B", 0, kb_, n, NAN)], [], [n]), ("B inf", [("B", 0, kb_, n, INF)], [], [n]),
                                    ("payload NaNs", [("A", 0, m, ka, NAN_7F), ("B", 0, kb_, n, NAN_FF)], [m], [n])):
        out = X.run_gemm(gemm_row_case(dict(kw, poke=pokes)), bf16=bf, finite=False)[0]
        bad = torch.zeros(M, N, dtype=torch.bool)
        bad[rows, :] = True
        bad[:, cols] = True
        nonfinite = ~torch.isfinite(out)
        print("gemm_paths %s %s: %d cells non-finite, %d expected" % (ident, what, int(nonfinite.sum()), int(bad.sum())))
        assert torch.equal(nonfinite, bad), (ident, what, int(nonfinite.sum()), int(bad.sum()))
        assert torch.equal(_bits(out)[~bad], _bits(clean)[~bad]), (ident, what)


# ---- (d) coattn_linear_forward ---------------------------------------------------------------------------------------------------
# rows: (id, kernel the mirror must name, flags, M, N, K)
LINEAR_ROWS = []


def _lin(form, flags, M, N, K, tag=None):
    LINEAR_ROWS.append(("%s-%dx%dx%d" % (tag or form, M, N, K), form, flags, M, N, K))


def _lin_edges(form, flags, base, Ms, Ns, Ks):
    M0, N0, K0 = base
    seen = set()
    for shape in [(M, N0, K0) for M in Ms] + [(M0, N, K0) for N in Ns] + [(M0, N0, K) for K in Ks]:
        if shape not in seen:
            seen.add(shape)
            _lin(form, flags, *shape)


for form, flags in (("gemm_w3", 0), ("gemm_w2", X.SPLIT2)):
    _lin_edges(form, flags, (129, 200, 64), (128, 129, 255, 257), (1, 32, 33, 127, 129, 200), (32, 64, 160))
    _lin(form, flags, 4100, 33, 32)                                  # 33 row tiles: xcd_group
_lin_edges("gemm_w_f16", X.F16PAIR, (129, 200, 96), (1, 2, 127, 129), (1, 96, 200), (32, 96))
# gemm_h2: an LDS ring of three weight buffers -- one and two k steps (fewer than the ring), three, four, many
_lin_edges("gemm_h2", X.F16PAIR, (129, 256, 96), (1, 127, 128, 129, 1025), (256, 512), (32, 64, 96, 128, 1024))
# gemm_h2p (K = 512): one workgroup per CU walks its tiles as one pipeline, alternating two accumulator sets
_lin_edges("gemm_h2p", X.F16PAIR, (129, 256, 512), (1, 128, 129, 1025), (256, 512), (512,))
H2P_WALKS = {"gemm_h2p-two_tiles": 1, "gemm_h2p-three_tiles": 2}      # padded tiles = k CUs + 8: the first 8 workgroups walk k + 1


def h2p_walk_rows(cus):
    """[(id, form, flags, M, N, K)] of the two shapes whose padded tile count is the first multiple of 8 past cus and past
    2 cus (cus + 8 and 2 cus + 8 where cus % 8 == 0).  Built where they are used: the CU count is the device's."""
    return [(ident, "gemm_h2p", X.F16PAIR, 128 * (k * cus // 8 + 1) * 8, 256, 512) for ident, k in H2P_WALKS.items()]


def check_h2p_walk_row(cus, ident, form, flags, M, N, K):
    """The mirror's answer for a walk row: gemm_h2p, and more padded tiles than k cus but no more than (k + 1) cus."""
    k = H2P_WALKS[ident]
    assert X.linear_kernel(M, N, K, K, flags) == (16, True, form) and X.linear_kernel(M, N, K, K + 4, flags)[2] == form
    assert k * cus < X.h2p_tiles(M, N) <= k * cus + 8 and X.h2p_tiles(M, N) <= (k + 1) * cus, (ident, cus)


for M, N, K in ((128, 200, 32),):
    _lin("gemm_w_bf16", X.BF16_PROJ, M, N, K)
for M, N, K in ((129, 256, 32), (255, 256, 64), (300, 512, 96)):
    _lin("gemm_w_bf16_wide", X.BF16_PROJ, M, N, K)
_lin_edges("gemm_bf", X.BF16_PROJ, (257, 256, 128), (256, 257, 511, 513), (256, 512), (64, 128, 192))
LINEAR_IDS = [r[0] for r in LINEAR_ROWS]
assert len(set(LINEAR_IDS)) == len(LINEAR_IDS)
for _id, _form, _flags, _M, _N, _K in LINEAR_ROWS:
    for _ld in (_K, _K + 4, _K + 8):
        assert X.linear_kernel(_M, _N, _K, _ld, _flags)[2] == _form, (_id, _ld, X.linear_kernel(_M, _N, _K, _ld, _flags))
    assert X.linear_kernel(_M, _N, _K, _K, _flags)[1] == (_form in ("gemm_h2", "gemm_h2p", "gemm_bf") or _M >= 3969), _id
    if _form == "gemm_bf":
        assert X.linear_kernel(_M, _N, _K, _K + 8, _flags | X.BF16_IN) == (1, True, "gemm_bf"), _id


def linear_variants(flags, K):
    """(bias, ld_x, out_scale) of the two calls every row makes."""
    return ((True, K, 0.0), (False, K + (8 if flags & X.BF16_IN else 4), 2.5))


def _linear_check(ident, x, ld, W, b, M, N, K, scale, flags, wimg=None, ref_on=None):
    y, wimg = X.run_linear(x, ld, W if not flags & X.REUSE else torch.zeros_like(W), b, M, N, K, scale, flags, wimg)
    dev = ref_on or "cpu"
    to = lambda t: None if t is None else t.to(dev)          # noqa: E731
    fl = flags & ~X.REUSE
    ref = X.linear_reference(to(x), to(W), to(b), scale, fl).cpu()
    e = X.rel(y, ref)
    print("gemm_paths %s ld %d flags %d: %.2e (bound %.0e)" % (ident, ld, flags, e, X.linear_tolerance(fl)))
    assert e < X.linear_tolerance(fl), (ident, ld, flags, e)
    if fl & X.SPLIT2:                                        # it IS the two-piece product, and no worse than its budget
        et = X.rel(y, X.linear_reference(to(x), to(W), to(b), scale, fl, neighbour=True).cpu())
        print("gemm_paths %s: %.2e from the true product" % (ident, et))
        assert 1e-5 < et < 3e-5, (ident, et)
    return y, wimg


def _linear_row(ident, form, flags, M, N, K, ref_on=None):
    x, W, b, x2 = X.linear_inputs(M, N, K, flags, seed=len(ident) + M + N + K)
    for bias, ld, scale in linear_variants(flags, K):
        bb = b if bias else None
        y, wimg = _linear_check(ident, x, ld, W, bb, M, N, K, scale, flags, ref_on=ref_on)
        _linear_check(ident, x2, ld, W, bb, M, N, K, scale, flags | X.REUSE, wimg, ref_on=ref_on)     # other x, the image reused
        if form == "gemm_bf":                                # x stored as bf16: bit for bit the fp32-stored call on the rounded values
            xr = x.bfloat16().float()
            y32, _ = X.run_linear(xr, ld, W, bb, M, N, K, scale, flags)
            ld8 = K + 8 if ld != K else K
            yb, wb = _linear_check(ident, xr, ld8, W, bb, M, N, K, scale, flags | X.BF16_IN)
            assert torch.equal(_bits(yb), _bits(y32)), ident
            _linear_check(ident, x2.bfloat16().float(), ld8, W, bb, M, N, K, scale, flags | X.BF16_IN | X.REUSE, wb)


@pytest.mark.parametrize("ident", LINEAR_IDS)
def test_linear_forward_form_and_edge(ident):
    _linear_row(*LINEAR_ROWS[LINEAR_IDS.index(ident)])


@pytest.mark.parametrize("ident", list(H2P_WALKS))
def test_linear_h2p_workgroups_walk_two_and_three_tiles(ident):
    """Padded tiles = CUs + 8 (the first multiple of 8 past the CU count): the first eight workgroups walk two tiles, the
    rest one.  2 CUs + 8: the first eight walk three -- both accumulator sets are used and the first one is used again.  (Reference: float64 on the device.)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    row = [r for r in h2p_walk_rows(cus) if r[0] == ident][0]
    check_h2p_walk_row(cus, *row)
    _linear_row(*row, ref_on="cuda")


RING_ROWS = [r for r in LINEAR_ROWS if r[0] in ("gemm_h2-129x256x32", "gemm_h2-129x256x1024", "gemm_h2p-1x256x512", "gemm_h2p-1025x256x512",
                                                "gemm_bf-257x256x64", "gemm_bf-513x256x128")]
assert len(RING_ROWS) == 6


@pytest.mark.parametrize("ident", [r[0] for r in RING_ROWS])
def test_ring_kernels_repeat_bit_for_bit(ident):
    """The kernels with hand-counted operand rings: 10 launches on the same inputs, every one bit-identical to the first
    (every other one reuses the weight image)."""
    _, form, flags, M, N, K = [r for r in RING_ROWS if r[0] == ident][0]
    x, W, b, _ = X.linear_inputs(M, N, K, flags, seed=7)
    y0, wimg = X.run_linear(x, K, W, b, M, N, K, 0.0, flags)
    for rep in range(10):
        y, _ = X.run_linear(x, K, W, b, M, N, K, 0.0, flags | (rep & 1), wimg)
        assert torch.equal(_bits(y), _bits(y0)), (ident, rep, int((y != y0).sum()))


# ---- (e) coattn_linear_weight_grad ------------------------------------------------------------------------------------------------
# rows: (id, kernel, mode flags, M, n_out, n_in)
WGRAD_ROWS = []
TN_SHAPES = [(M, 128, 128) for M in (16, 17, 31, 33, 47, 512, 513)] + [(33, 128, 256), (33, 256, 128), (33, 512, 512)]
for tag, mode in (("exact", 0), ("split2", X.SPLIT2), ("bf16", X.BF16_PROJ)):
    for M, n_out, n_in in TN_SHAPES:
        WGRAD_ROWS.append(("gemm_tn_%s-%dx%dx%d" % (tag, M, n_out, n_in), "gemm_tn", mode, M, n_out, n_in))
WGRAD_ROWS.append(("gemm_tn_bf16-1024x128x256", "gemm_tn", X.BF16_PROJ, 1024, 128, 256))      # rows % 32 == 0: n_out = 128 refuses the wide form
BF_TN_SHAPES = [(M, 256, 256) for M in (32, 64, 1024, 1056)] + [(64, 256, 512), (64, 512, 256)]
for M, n_out, n_in in BF_TN_SHAPES:
    WGRAD_ROWS.append(("gemm_bf_tn-%dx%dx%d" % (M, n_out, n_in), "gemm_bf_tn", X.BF16_PROJ, M, n_out, n_in))
    WGRAD_ROWS.append(("gemm_bf_tn_stored-%dx%dx%d" % (M, n_out, n_in), "gemm_bf_tn", X.BF16_PROJ | X.BF16_IN, M, n_out, n_in))
WGRAD_IDS = [r[0] for r in WGRAD_ROWS]
assert len(set(WGRAD_IDS)) == len(WGRAD_IDS)
for _id, _form, _mode, _M, _no, _ni in WGRAD_ROWS:
    for _pad in (0, 8):
        assert X.wgrad_plan(_M, _no, _ni, _no + _pad, _ni + _pad // 2, _mode)[0] == _form, _id
# one part, a last part of one row, exactly 32 parts, the first ks = 32 with 17 parts; one step, 32 parts, 17 parts of two steps
assert [X.wgrad_plan(M, 128, 128, 128, 128, 0)[1:] for M in (16, 17, 512, 513)] == [(16, 1), (16, 2), (16, 32), (32, 17)]
assert [X.wgrad_plan(M, 256, 256, 256, 256, X.BF16_PROJ)[1:] for M in (32, 1024, 1056)] == [(1, 1), (1, 32), (2, 17)]


@pytest.mark.parametrize("ident", WGRAD_IDS)
def test_linear_weight_grad_form_and_edge(ident):
    """accumulate 0 on contiguous rows and accumulate 1 on padded ones, each run twice: bit-identical."""
    _, form, mode, M, n_out, n_in = WGRAD_ROWS[WGRAD_IDS.index(ident)]
    dy, x, dW0 = X.wgrad_inputs(M, n_out, n_in, mode, seed=M + n_out + n_in)
    tol = 2e-5 if mode & X.BF16_PROJ else 2e-6
    for acc, pad_dy, pad_x in ((0, 0, 0), (1, 8, 4)):
        fl = mode | acc
        dW = X.run_wgrad(dy, n_out + pad_dy, x, n_in + pad_x, M, n_out, n_in, fl, dW0 if acc else None)
        ref = X.wgrad_reference(dy, x, dW0, fl)
        e = X.rel(dW, ref)
        print("gemm_paths %s accumulate %d: %.2e (bound %.0e)" % (ident, acc, e, tol))
        assert e < tol, (ident, acc, e)
        if mode & X.SPLIT2:
            et = X.rel(dW, X.wgrad_reference(dy, x, dW0, fl, neighbour=True))
            print("gemm_paths %s: %.2e from the true product" % (ident, et))
            assert et < 3e-5, (ident, et)
        again = X.run_wgrad(dy, n_out + pad_dy, x, n_in + pad_x, M, n_out, n_in, fl, dW0 if acc else None)
        assert torch.equal(_bits(dW), _bits(again)), (ident, acc)
        if mode & X.BF16_IN:                                 # bit for bit the fp32-stored call on the same (rounded) values
            same = X.run_wgrad(dy, n_out + pad_dy, x, n_in + pad_x, M, n_out, n_in, fl & ~X.BF16_IN, dW0 if acc else None)
            assert torch.equal(_bits(dW), _bits(same)), (ident, acc)

"""The GEMM layer's C-ABI without a GPU: the dispatch mirrors of tests/_gemm.py (launch_gemm_bf16in; coattn_linear_forward ->
gemm_wx_kernel -> launch_gemm_w / launch_gemm_h2 / launch_gemm_bf; coattn_linear_weight_grad -> gemm_tn_plan /
gemm_bf_tn_plan) pinned on both sides of every threshold they encode; every refusal of coattn_gemm_f32 / coattn_gemm_bf16,
coattn_linear_forward and coattn_linear_weight_grad, made before any HIP call (the pointers are host memory or NULL), next
to the mirror's answer for the neighbouring accepted shape -- which is not launched here; the workspace byte counts; and,
for every row of the tables of tests/test_gpu_gemm_paths.py, that its bound can be met (the float32 torch.matmul form of
the reference lies within half of it) and tells the modes apart (the neighbouring mode's reference misses it five times
over)."""
import ctypes as C

import pytest
import torch

from vqa_amd import _lib

from tests import _gemm as X
from tests import test_gpu_gemm_paths as T

BF, IN, S2, F16 = X.BF16_PROJ, X.BF16_IN, X.SPLIT2, X.F16PAIR


# ---- the mirrors at their thresholds ---------------------------------------------------------------------------------------------
def _bf(M, N=64, K=8, a="k", b="k", **kw):
    return X.gemm_bf16_kernel(**X.gemm_case(M, N, K, a=a, b=b, data=False, **kw))


def test_bf16_entry_row_thresholds():
    # A along k: the aligned path from 128 rows on, gemm_bf16in_kernel<false, true> below -- 64 / 65 changes nothing here
    assert _bf(127) == "bf16in_ak" and _bf(128) == "vec128_bf16"
    assert _bf(64) == "bf16in_ak" and _bf(65) == "bf16in_ak"
    # A along m: M % 4 decides between the aligned path (>= 128), the float4 form and the scalar form
    assert _bf(128, a="m") == "vec128_bf16" and _bf(129, a="m") == "bf16in_am_scalar" and _bf(124, a="m") == "bf16in_am_vec"
    assert _bf(127, a="m") == "bf16in_am_scalar"
    assert _bf(104, a="m", a_mdiv=52) == "bf16in_am_vec" and _bf(98, a="m", a_mdiv=49) == "bf16in_am_scalar"
    assert _bf(196, a="m", a_mdiv=49) == "bf16in_am_scalar" and _bf(208, a="m", a_mdiv=52) == "vec128_bf16"
    # the exact fallback takes the 32-row kernel up to 64 rows
    assert _bf(64, K=7) == "exact:f32_32" and _bf(65, K=7) == "exact:f32_128"


def test_bf16_entry_stride_thresholds():
    assert _bf(100, K=8) == "bf16in_ak" and _bf(100, K=6) == "exact:f32_128"               # K % 4
    assert _bf(100, b="n") == "exact:f32_128"                                              # B must run along k
    assert _bf(100, K=8, a_pad=4) == "bf16in_ak" and _bf(100, K=8, a_pad=2) == "exact:f32_128"       # A's row stride % 4
    assert _bf(100, K=8, b_pad=4) == "bf16in_ak" and _bf(100, K=8, b_pad=2) == "exact:f32_128"       # B's column stride % 4
    assert _bf(100, a_off=1) == "exact:f32_128" and _bf(100, b_off=2) == "exact:f32_128" and _bf(100, c_off=3) == "bf16in_ak"
    assert _bf(132, a_off=1) == "exact:f32_128" and _bf(132, K=6) == "exact:f32_128"


def test_bf16_entry_fields_the_unaligned_kernel_does_not_read():
    """gemm_bf16in_kernel copies A, B, C, bias_n, out_scale, an a_ptrs table and the row splits: every other field must send
    the shape to the exact path (kband_n, cin_ptrs, b_imod and an inner_total below batch did not before this file existed)."""
    own = (dict(bias_n=True), dict(out_scale=2.5), dict(a_tab=True, batch=3), dict(c="div", c_mdiv=7), dict(batch=3),
           # inner <= 1 with an inner_total that covers every batch entry clips nothing (grad_dw_sample_groups at B <= 32)
           dict(inner=1, inner_total=1), dict(inner=1, inner_total=3, batch=3), dict(inner=1, inner_total=4, batch=3))
    other = (dict(bias_m=True), dict(cin="n", beta=0.5), dict(cin="n", cin_tab=True, beta=0.5), dict(act=1), dict(inner=2),
             dict(inner=1, inner_total=2, batch=3), dict(K=96, ksplit=48, batch=2), dict(b_tab=True), dict(c_tab=True),
             dict(a_tab=True, b_tab=True, by_inner=True, inner=2), dict(inner=1, inner_total=2, batch=2, b_imod=1),
             dict(N=200, K=8, kband_n=128, kband=((0, 4), (4, 8))))
    for kw in own:
        assert _bf(127, **kw) == "bf16in_ak", kw
        assert _bf(132, **kw) == "vec128_bf16", kw
    for kw in other:
        assert _bf(127, **kw) == "exact:f32_128", kw
        assert _bf(132, **kw) == "vec128_bf16", kw           # the aligned path honours every field
    assert _bf(127, a_tab=True, batch=8) == "bf16in_ak"


def test_gemm_xcd_group_from_32_row_tiles():
    for M, want in ((3968, False), (3972, True)):            # 31 / 32 tiles of 128 rows
        d = X.gemm_case(M, 64, 8, data=False)
        assert X.gemm_f32_kernel(**d) == ("vec128", want) and X.gemm_bf16_xcd_group(**d) == want
        d = X.gemm_case(M, 64, 8, a="m", a_mdiv=49, data=False)
        assert X.gemm_bf16_kernel(**d) == "bf16in_am_scalar" and X.gemm_bf16_xcd_group(**d) == want
        assert X.linear_kernel(M, 64, 32, 32, 0)[1] == want and X.linear_kernel(M, 64, 32, 32, F16)[1] == want


def test_linear_kernel_thresholds():
    K = X.linear_kernel
    assert K(127, 64, 32, 32, 0)[2] == "refused" and K(128, 64, 32, 32, 0) == (3, False, "gemm_w3")
    assert K(128, 64, 32, 32, S2) == (3, False, "gemm_w2") and K(127, 64, 32, 32, S2)[2] == "refused"
    assert K(127, 64, 32, 32, F16) == (16, False, "gemm_w_f16") and K(1, 64, 32, 32, F16)[2] == "gemm_w_f16"
    assert K(0, 64, 32, 32, F16)[2] == "refused"
    # N % 256: the FP16-pair form moves to gemm_h2, the single-piece form to the 256-column tile
    assert K(1, 256, 32, 32, F16) == (16, True, "gemm_h2") and K(1, 255, 32, 32, F16)[2] == "gemm_w_f16"
    assert K(1, 512, 32, 32, F16)[2] == "gemm_h2" and K(1, 384, 32, 32, F16)[2] == "gemm_w_f16"
    assert K(128, 256, 32, 32, BF) == (3, False, "gemm_w_bf16_wide") and K(128, 255, 32, 32, BF) == (3, False, "gemm_w_bf16")
    # K % 32, K % 64, K == 512
    assert K(128, 64, 33, 36, 0)[2] == "refused" and K(128, 64, 64, 64, 0)[2] == "gemm_w3" and K(128, 64, 16, 16, 0)[2] == "refused"
    assert K(1, 256, 512, 512, F16)[2] == "gemm_h2p" and K(1, 256, 480, 480, F16)[2] == "gemm_h2" and K(1, 256, 544, 544, F16)[2] == "gemm_h2"
    assert K(1, 255, 512, 512, F16)[2] == "gemm_w_f16"
    assert K(256, 256, 64, 64, BF) == (1, True, "gemm_bf") and K(256, 256, 96, 96, BF)[2] == "gemm_w_bf16_wide"
    assert K(256, 256, 32, 32, BF)[2] == "gemm_w_bf16_wide"
    # M 255 / 256 (gemm_bf asks M >= 256, no multiple: 257 stays)
    assert K(255, 256, 64, 64, BF)[2] == "gemm_w_bf16_wide" and K(257, 256, 64, 64, BF)[2] == "gemm_bf"
    assert K(256, 255, 64, 64, BF)[2] == "gemm_w_bf16"
    # F16PAIR gives way to BF16_PROJ; SPLIT2 under F16PAIR changes nothing
    assert K(128, 64, 32, 32, F16 | BF)[2] == "gemm_w_bf16" and K(1, 64, 32, 32, F16 | BF)[2] == "refused"
    assert K(1, 256, 32, 32, F16 | S2)[2] == "gemm_h2"
    # ld_x: >= K, % 4, below 2^24, % 8 for bf16-stored rows; the address
    assert K(128, 64, 32, 31, 0)[2] == "refused" and K(128, 64, 32, 36, 0)[2] == "gemm_w3" and K(128, 64, 32, 34, 0)[2] == "refused"
    assert K(1, 64, 32, (1 << 24) - 4, F16)[2] == "gemm_w_f16" and K(1, 64, 32, 1 << 24, F16)[2] == "refused"
    assert K(16, 64, 32, (1 << 24) - 4, F16)[2] == "gemm_w_f16" and K(17, 64, 32, (1 << 24) - 4, F16)[2] == "refused"     # rows span 1 GiB
    assert K(128, 64, 32, 32, 0, aligned=False)[2] == "refused"
    assert K(256, 256, 64, 72, BF | IN)[2] == "gemm_bf" and K(256, 256, 64, 68, BF | IN)[2] == "refused"
    assert K(256, 256, 64, 68, BF)[2] == "gemm_bf"
    assert K(256, 256, 64, 64, IN)[2] == "refused"                                           # BF16_IN without BF16_PROJ
    assert K(255, 256, 64, 64, BF | IN)[2] == "refused" and K(256, 128, 64, 64, BF | IN)[2] == "refused"
    assert K(256, 256, 96, 96, BF | IN)[2] == "refused"


def test_wgrad_plan_thresholds():
    P = X.wgrad_plan
    assert P(15, 128, 128, 128, 128, 0)[0] == "refused" and P(16, 128, 128, 128, 128, 0) == ("gemm_tn", 16, 1)
    assert P(16, 127, 128, 128, 128, 0)[0] == "refused" and P(16, 128, 192, 128, 192, 0)[0] == "refused"
    assert P(16, 128, 128, 130, 128, 0)[0] == "refused" and P(16, 128, 128, 132, 128, 0)[0] == "gemm_tn"
    assert P(16, 128, 128, 128, 130, 0)[0] == "refused" and P(16, 128, 128, 124, 128, 0)[0] == "refused"
    assert P(16, 128, 128, 128, 128, 0, aligned=False)[0] == "refused"
    # one 128 x 128 tile: one part, a last part of one row, exactly 32 parts, the first ks = 32
    assert [P(M, 128, 128, 128, 128, 0)[1:] for M in (16, 17, 512, 513)] == [(16, 1), (16, 2), (16, 32), (32, 17)]
    assert P(512, 128, 128, 128, 128, S2)[1:] == (16, 32)
    # more tiles: 512 slots once -- still the cap of 32 parts at 16 tiles, 8 parts at 64
    assert P(4096, 512, 512, 512, 512, 0)[1:] == (128, 32) and P(4096, 1024, 1024, 1024, 1024, 0)[1:] == (512, 8)
    # the wide reduced-precision form: n % 256, M % 32, M >= 32
    assert P(32, 256, 256, 256, 256, BF) == ("gemm_bf_tn", 1, 1) and P(16, 256, 256, 256, 256, BF)[0] == "gemm_tn"
    assert P(33, 256, 256, 256, 256, BF)[0] == "gemm_tn" and P(64, 128, 256, 128, 256, BF)[0] == "gemm_tn"
    assert P(64, 256, 384, 256, 384, BF)[0] == "gemm_tn" and P(64, 256, 512, 256, 512, BF)[0] == "gemm_bf_tn"
    # one 256 x 256 tile: one part, 32 parts, 17 parts of two steps with the last one step long
    assert [P(M, 256, 256, 256, 256, BF)[1:] for M in (32, 1024, 1056)] == [(1, 1), (1, 32), (2, 17)]
    assert 17 * 2 > 1056 // 32 > 16 * 2
    assert P(2048, 512, 512, 512, 512, BF)[1:] == (2, 32)        # four tiles: 64 parts wanted, capped at 32 of two steps
    # bf16-stored dy
    assert P(64, 256, 256, 264, 256, BF | IN)[0] == "gemm_bf_tn" and P(64, 256, 256, 260, 256, BF | IN)[0] == "refused"
    assert P(64, 256, 256, 256, 256, IN)[0] == "refused" and P(64, 128, 256, 128, 256, BF | IN)[0] == "refused"
    assert P(48, 256, 256, 256, 256, BF | IN)[0] == "refused" and P(64, 256, 256, 260, 256, BF)[0] == "gemm_bf_tn"


def test_h2p_tiles():
    assert X.h2p_tiles(1, 256) == 8 and X.h2p_tiles(1025, 512) == 32 and X.h2p_tiles(128 * 264, 256) == 264
    for cus in (256, 304, 100):                              # (a CU count that is no multiple of 8: the next multiple)
        for row in T.h2p_walk_rows(cus):
            T.check_h2p_walk_row(cus, *row)
    assert [X.h2p_tiles(r[3], r[4]) for r in T.h2p_walk_rows(256)] == [264, 520] and [X.h2p_tiles(r[3], r[4]) for r in T.h2p_walk_rows(100)] == [104, 208]


# ---- byte counts -----------------------------------------------------------------------------------------------------------------
def test_workspace_byte_counts():
    lib = _lib.load()
    for N, K in ((32, 16), (33, 16), (32, 17), (1, 1), (200, 160), (257, 33), (512, 512), (0, 32), (32, 0), (-1, 32), (32, -5)):
        assert lib.coattn_linear_workspace_bytes(N, K) == X.linear_workspace_bytes(N, K), (N, K)
    assert X.linear_workspace_bytes(33, 17) == 2 * 2 * 3072 and X.linear_workspace_bytes(0, 32) == 0 == X.linear_workspace_bytes(32, -5)
    for n_out, n_in in ((128, 128), (256, 384), (1, 1), (0, 128), (128, 0), (-128, 128)):
        assert lib.coattn_linear_wgrad_workspace_bytes(n_out, n_in) == X.wgrad_workspace_bytes(n_out, n_in), (n_out, n_in)
    assert X.wgrad_workspace_bytes(128, 256) == 32 * 128 * 256 * 4 and X.wgrad_workspace_bytes(0, 128) == 0


# ---- refusals: -1 with the documented message before any HIP call ---------------------------------------------------------------
class _Host:
    """Host memory standing in for the device pointers of a call that is refused before it reads one: 16-byte aligned."""

    def __init__(self):
        self.raw = (C.c_char * 4096)()
        self.p = (C.addressof(self.raw) + 15) & ~15


LINEAR_REFUSALS = [
    ("K_33", dict(K=33, ld=36), b"not supported"), ("K_16", dict(K=16, ld=16), b"not supported"),
    ("M_127", dict(M=127), b"not supported"), ("M_127_split2", dict(M=127, flags=S2), b"not supported"),
    ("M_0_f16pair", dict(M=0, flags=F16), b"bad argument"),
    ("ld_below_K", dict(ld=28), b"bad argument"), ("ld_34", dict(ld=34), b"not supported"), ("ld_2p24", dict(ld=1 << 24), b"bad argument"),
    ("x_misaligned", dict(x_off=4), b"not supported"), ("x_null", dict(x=None), b"bad argument"), ("W_null", dict(W=None), b"bad argument"),
    ("y_null", dict(y=None), b"bad argument"), ("wimg_null", dict(wimg=None), b"bad argument"),
    ("bf16_in_alone", dict(M=256, N=256, K=64, ld=64, flags=IN), b"COATTN_FLAG_BF16_IN needs COATTN_FLAG_BF16_PROJ"),
    ("bf16_in_M_255", dict(M=255, N=256, K=64, ld=64, flags=BF | IN), b"not supported"),
    ("bf16_in_N_128", dict(M=256, N=128, K=64, ld=64, flags=BF | IN), b"not supported"),
    ("bf16_in_K_96", dict(M=256, N=256, K=96, ld=96, flags=BF | IN), b"not supported"),
    ("bf16_in_ld_68", dict(M=256, N=256, K=64, ld=68, flags=BF | IN), b"not supported"),
]
# the accepted neighbour of each refusal, by the mirror alone (nothing is launched here)
LINEAR_NEIGHBOURS = [dict(K=32, ld=36), dict(K=64, ld=64), dict(M=128), dict(M=127, flags=F16), dict(M=1, flags=F16), dict(ld=32), dict(ld=36),
                     dict(M=1, ld=(1 << 24) - 4, flags=F16), dict(M=256, N=256, K=64, ld=64, flags=BF | IN), dict(M=256, N=256, K=64, ld=72, flags=BF | IN)]


def _linear_args(kw):
    a = dict(M=128, N=64, K=32, ld=32, flags=0)
    a.update({k: v for k, v in kw.items() if k in a})
    return a


@pytest.mark.parametrize("name,kw,msg", LINEAR_REFUSALS, ids=[r[0] for r in LINEAR_REFUSALS])
def test_linear_forward_refuses(name, kw, msg):
    h = _Host()
    a = _linear_args(kw)
    ptr = {k: kw.get(k, h.p) for k in ("x", "W", "y", "wimg")}
    if "x_off" in kw:
        ptr["x"] = h.p + kw["x_off"]
    rc, err = X.linear_call(ptr["x"], a["ld"], ptr["W"], None, ptr["y"], ptr["wimg"], a["M"], a["N"], a["K"], 0.0, a["flags"])
    assert rc == -1 and msg in err, (rc, err)
    aligned = "x_off" not in kw
    if all(ptr.values()):
        assert X.linear_kernel(a["M"], a["N"], a["K"], a["ld"], a["flags"], aligned=aligned)[2] == "refused"


def test_linear_forward_neighbours_are_accepted_by_the_mirror():
    for kw in LINEAR_NEIGHBOURS:
        a = _linear_args(kw)
        assert X.linear_kernel(a["M"], a["N"], a["K"], a["ld"], a["flags"])[2] != "refused", kw


WGRAD_REFUSALS = [
    ("n_out_96", dict(n_out=96, ld_dy=96), b"not supported"), ("n_in_192", dict(n_in=192, ld_x=192), b"not supported"),
    ("M_15", dict(M=15), b"not supported"), ("ld_dy_130", dict(ld_dy=130), b"not supported"), ("ld_x_130", dict(ld_x=130), b"not supported"),
    ("ld_dy_short", dict(ld_dy=124), b"bad argument"), ("ld_x_2p24", dict(ld_x=1 << 24), b"bad argument"),
    ("dy_misaligned", dict(dy_off=8), b"not supported"), ("x_misaligned", dict(x_off=4), b"not supported"),
    ("dy_null", dict(dy=None), b"bad argument"), ("x_null", dict(x=None), b"bad argument"), ("dW_null", dict(dW=None), b"bad argument"),
    ("ws_null", dict(ws=None), b"bad argument"),
    ("bf16_in_alone", dict(M=64, n_out=256, n_in=256, ld_dy=256, ld_x=256, acc=IN), b"COATTN_FLAG_BF16_IN needs COATTN_FLAG_BF16_PROJ"),
    ("bf16_in_ld_260", dict(M=64, n_out=256, n_in=256, ld_dy=260, ld_x=256, acc=BF | IN), b"not supported"),
    ("bf16_in_n_out_128", dict(M=64, n_out=128, n_in=256, ld_dy=128, ld_x=256, acc=BF | IN), b"not supported"),
    ("bf16_in_n_in_384", dict(M=64, n_out=256, n_in=384, ld_dy=256, ld_x=384, acc=BF | IN), b"not supported"),
    ("bf16_in_M_48", dict(M=48, n_out=256, n_in=256, ld_dy=256, ld_x=256, acc=BF | IN), b"not supported"),
]
WGRAD_NEIGHBOURS = [dict(), dict(M=16), dict(ld_dy=132), dict(ld_x=132), dict(n_in=256, ld_x=256),
                    dict(M=64, n_out=256, n_in=256, ld_dy=264, ld_x=256, acc=BF | IN), dict(M=64, n_out=128, n_in=256, ld_dy=128, ld_x=256, acc=BF),
                    dict(M=48, n_out=256, n_in=256, ld_dy=256, ld_x=256, acc=BF)]


def _wgrad_args(kw):
    a = dict(M=16, n_out=128, n_in=128, ld_dy=128, ld_x=128, acc=0)
    a.update({k: v for k, v in kw.items() if k in a})
    return a


@pytest.mark.parametrize("name,kw,msg", WGRAD_REFUSALS, ids=[r[0] for r in WGRAD_REFUSALS])
def test_linear_weight_grad_refuses(name, kw, msg):
    h = _Host()
    a = _wgrad_args(kw)
    ptr = {k: kw.get(k, h.p) for k in ("dy", "x", "dW", "ws")}
    ptr["dy"] = h.p + kw["dy_off"] if "dy_off" in kw else ptr["dy"]
    ptr["x"] = h.p + kw["x_off"] if "x_off" in kw else ptr["x"]
    rc, err = X.wgrad_call(ptr["dy"], a["ld_dy"], ptr["x"], a["ld_x"], ptr["dW"], ptr["ws"], a["M"], a["n_out"], a["n_in"], a["acc"])
    assert rc == -1 and msg in err, (rc, err)
    if all(ptr.values()):
        aligned = "dy_off" not in kw and "x_off" not in kw
        assert X.wgrad_plan(a["M"], a["n_out"], a["n_in"], a["ld_dy"], a["ld_x"], a["acc"], aligned=aligned)[0] == "refused"


def test_linear_weight_grad_neighbours_are_accepted_by_the_mirror():
    for kw in WGRAD_NEIGHBOURS:
        a = _wgrad_args(kw)
        assert X.wgrad_plan(a["M"], a["n_out"], a["n_in"], a["ld_dy"], a["ld_x"], a["acc"])[0] != "refused", kw


def _desc(h, **kw):
    g = _lib.GemmDesc()
    base = dict(A=h.p, B=h.p, C=h.p, M=8, N=8, K=8, batch=1, a_sm=8, a_sk=1, b_sk=1, b_sn=8, c_sm=8, c_sn=1)
    base.update(kw)
    for k, v in base.items():
        if k in ("kband_lo", "kband_hi"):
            for j in range(3):
                getattr(g, k)[j] = v[j]
        else:
            setattr(g, k, v)
    return g


def _tab(h, n):
    return (C.c_void_p * 8)(*([h.p] * n + [None] * (8 - n)))


GEMM_REFUSALS = [
    ("A_null", lambda h: dict(A=None), b"null operand"), ("B_null", lambda h: dict(B=None), b"null operand"),
    ("C_null", lambda h: dict(C=None), b"null operand"),
    ("c_ptrs_by_inner", lambda h: dict(c_ptrs=_tab(h, 2), ptr_by_inner=1, inner=2), b"C tables are indexed by batch only"),
    ("cin_ptrs_by_inner", lambda h: dict(cin_ptrs=_tab(h, 2), ptr_by_inner=1, inner=2), b"C tables are indexed by batch only"),
    ("table_of_9_by_batch", lambda h: dict(a_ptrs=_tab(h, 8), batch=9), b"pointer tables hold at most 8 entries"),
    ("table_of_9_by_inner", lambda h: dict(b_ptrs=_tab(h, 8), ptr_by_inner=1, inner=3, inner_total=9, batch=3), b"pointer tables hold at most 8 entries"),
    ("c_table_of_9", lambda h: dict(c_ptrs=_tab(h, 8), batch=9), b"pointer tables hold at most 8 entries"),
    ("kband_n_64", lambda h: dict(N=128, kband_n=64), b"kband_n must be a multiple of 128"),
    ("kband_n_130", lambda h: dict(N=128, kband_n=130), b"kband_n must be a multiple of 128"),
    ("four_bands", lambda h: dict(N=385, kband_n=128, kband_hi=(8, 8, 8)), b"at most 3 bands"),
    ("band_past_K", lambda h: dict(N=128, kband_n=128, kband_hi=(12, 8, 8)), b"k bands must lie in [0,K]"),
    ("band_below_0", lambda h: dict(N=128, kband_n=128, kband_lo=(0, -4, 0), kband_hi=(8, 8, 8)), b"k bands must lie in [0,K]"),
    ("band_not_of_4", lambda h: dict(N=128, kband_n=128, kband_lo=(2, 0, 0), kband_hi=(8, 8, 8)), b"multiples of 4"),
    ("batch_65536", lambda h: dict(batch=65536), b"batch 65536 exceeds grid.z"),
    ("batch_0", lambda h: dict(batch=0), b"bad shape"), ("K_0", lambda h: dict(K=0), b"bad shape"),
]


@pytest.mark.parametrize("entry", ["coattn_gemm_f32", "coattn_gemm_bf16"])
@pytest.mark.parametrize("name,kw,msg", GEMM_REFUSALS, ids=[r[0] for r in GEMM_REFUSALS])
def test_gemm_refuses(name, kw, msg, entry):
    lib = _lib.load()
    h = _Host()
    g = _desc(h, **kw(h))
    rc = getattr(lib, entry)(C.byref(g), None)
    assert rc == -1 and msg in lib.coattn_last_error(), (rc, lib.coattn_last_error())


@pytest.mark.parametrize("entry", ["coattn_gemm_f32", "coattn_gemm_bf16"])
def test_gemm_refuses_a_null_descriptor(entry):
    lib = _lib.load()
    assert getattr(lib, entry)(None, None) == -1 and b"null descriptor" in lib.coattn_last_error()


# ---- the bounds of the GPU tables: attainable in float32, and telling the modes apart -------------------------------------------
@pytest.mark.parametrize("ident", T.GEMM_IDS)
def test_gemm_row_bound_is_attainable_and_separates(ident):
    _, entry, form, kw = T.GEMM_ROWS[T.GEMM_IDS.index(ident)]
    assert T.gemm_row_mirror(entry, kw) == (form, bool(kw.get("xcd")))
    d = T.gemm_row_case(kw)
    rounds = T.gemm_row_rounds(form)
    ref = X.gemm_reference(d, bf16=rounds)
    assert bool(torch.isfinite(ref).all())
    scale = 1.0 if d.get("act") == 1 else float(ref.abs().max())
    e32 = float((X.gemm_reference(d, bf16=rounds, dtype=torch.float32).double() - ref).abs().max()) / scale
    assert e32 < T.TOL / 2, (ident, e32)
    if rounds:                                               # the exact product is what the bound must exclude
        away = float((X.gemm_reference(d, bf16=False) - ref).abs().max()) / scale
        assert away > 5 * T.TOL, (ident, away)


def _sub(M):
    """Every row up to 4,100 rows; of the taller shapes every 37th (the bound's margins are statistics of the rows)."""
    return slice(None) if M <= 4100 else slice(0, None, 37)


@pytest.mark.parametrize("ident", T.LINEAR_IDS + list(T.H2P_WALKS))
def test_linear_row_bound_is_attainable_and_separates(ident):
    _, form, flags, M, N, K = [r for r in T.LINEAR_ROWS + T.h2p_walk_rows(256) if r[0] == ident][0]
    assert X.linear_kernel(M, N, K, K, flags)[2] == form
    x, W, b, x2 = X.linear_inputs(M, N, K, flags, seed=len(ident) + M + N + K)
    tol = X.linear_tolerance(flags)
    for xx in (x[_sub(M)], x2[_sub(M)]):
        for bias, _, scale in T.linear_variants(flags, K):
            bb = b if bias else None
            ref = X.linear_reference(xx, W, bb, scale, flags)
            e32 = X.rel(X.linear_reference(xx, W, bb, scale, flags, dtype=torch.float32), ref)
            assert e32 < tol / 2, (ident, e32)
            if flags & (BF | S2 | F16):
                away = X.rel(X.linear_reference(xx, W, bb, scale, flags, neighbour=True), ref)
                assert away > 5 * tol, (ident, away)
                if flags & S2:                               # and the two-piece product keeps inside its own budget
                    assert away < 3e-5, (ident, away)


@pytest.mark.parametrize("ident", T.WGRAD_IDS)
def test_wgrad_row_bound_is_attainable_and_separates(ident):
    _, form, mode, M, n_out, n_in = T.WGRAD_ROWS[T.WGRAD_IDS.index(ident)]
    assert X.wgrad_plan(M, n_out, n_in, n_out, n_in, mode)[0] == form
    dy, x, dW0 = X.wgrad_inputs(M, n_out, n_in, mode, seed=M + n_out + n_in)
    tol = 2e-5 if mode & BF else 2e-6
    for acc in (0, 1):
        ref = X.wgrad_reference(dy, x, dW0, mode | acc)
        e32 = X.rel(X.wgrad_reference(dy, x, dW0, mode | acc, dtype=torch.float32), ref)
        assert e32 < tol / 2, (ident, acc, e32)
        if mode & (BF | S2):
            away = X.rel(X.wgrad_reference(dy, x, dW0, mode | acc, neighbour=True), ref)
            assert away > 5 * tol, (ident, acc, away)
            if mode & S2:
                assert away < 3e-5, (ident, acc, away)

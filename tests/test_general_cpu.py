"""The general-shape path of the parallel co-attention without a GPU: tests/_general.py paths() -- the dispatch rules of
csrc/api.hip, csrc/small_kernels.hip and csrc/gemm.hip launch_gemm_impl restated in Python -- pinned on both sides of every
threshold it encodes, and the refusals of coattn_workspace_bytes and of the forward and backward entry points at the limits
of check_shape and check_vlayout.  Every refusal below is made before any device work: a shape check comes first in each
entry point, and the stride checks are reached with question tables that hold NULL, which the next check would refuse."""
import ctypes as C

import pytest

from vqa_amd import _lib

from tests import _general as G

GEN = _lib.IMPL_GENERAL


# ---- launch_gemm_impl --------------------------------------------------------------------------------------------------------
def _ct(M, K=8, N=64, batch=2, **kw):
    """ct_times' strides: A contiguous along m, B along n."""
    return G.gemm_kernel(M, N, K, batch, a_sm=1, a_sk=M, a_sz=K * M, b_sk=N, b_sn=1, b_sz=K * N, **kw)


def test_gemm_row_thresholds():
    assert _ct(64) == ("f32_32", False) and _ct(65) == ("f32_128", False)
    assert _ct(127) == ("f32_128", False) and _ct(124) == ("f32_128", False)
    assert _ct(128) == ("vec128", False)
    assert _ct(129) == ("f32_128", False)                      # A runs along m: M % 4
    # through paths(): affinity / c_times / dC / dQ have M = T
    for T, want in ((64, "f32_32"), (65, "f32_128"), (127, "f32_128"), (128, "vec128")):
        p = G.paths(2, 52, T, 64, 1, "lm")
        for name in ("affinity", "c_times", "dC", "dQ"):
            assert p["gemm"][name][0] == want, (T, name, p["gemm"][name])


def test_gemm_alignment_of_k_and_strides():
    assert _ct(128, K=8)[0] == "vec128" and _ct(128, K=5)[0] == "f32_128" and _ct(128, K=6)[0] == "f32_128"
    assert _ct(4096, K=5) == ("f32_128", False)                # M = 4096 off the vec kernel: no xcd_group
    # B along n: N % 4 and its row stride
    assert _ct(128, N=37)[0] == "f32_128" and _ct(128, N=36)[0] == "vec128"
    # an operand with no contiguous axis (sD = 2) is never vec
    assert G.gemm_kernel(128, 64, 64, 1, a_sm=128, a_sk=2, b_sk=1, b_sn=64)[0] == "f32_128"
    # the split-K step and the batch strides
    kw = dict(a_sm=1, a_sk=256, b_sk=256, b_sn=1)
    assert G.gemm_kernel(256, 256, 160, 10, ksplit=16, **kw)[0] == "vec128"
    assert G.gemm_kernel(256, 256, 160, 10, ksplit=18, **kw)[0] == "f32_128"
    assert G.gemm_kernel(256, 256, 160, 2, a_sz=6, **kw)[0] == "f32_128"
    # through paths(): K = T for ct_times and dv_kt_da, K = N for c_times / dQ / dw_v, K = d elsewhere
    assert G.paths(2, 256, 8, 64, 1)["gemm"]["ct_times"][0] == "vec128"
    assert G.paths(2, 256, 7, 64, 1)["gemm"]["ct_times"][0] == "f32_128"
    assert G.paths(2, 256, 8, 256, 1)["gemm"]["dv_kt_da"][0] == "vec128"
    assert G.paths(2, 256, 6, 256, 1)["gemm"]["dv_kt_da"][0] == "f32_128"
    assert G.paths(2, 256, 8, 256, 1)["gemm"]["dw_v"][0] == "vec128" and G.paths(2, 257, 8, 256, 1)["gemm"]["dw_v"][0] == "f32_128"


def test_gemm_xcd_group_from_32_row_tiles():
    assert _ct(3968) == ("vec128", False) and _ct(3972) == ("vec128", True)       # ntm = 31 / 32
    assert G.paths(1, 3968, 8, 64, 1)["gemm"]["ct_times"] == ("vec128", False)
    assert G.paths(1, 4096, 8, 64, 1)["gemm"]["ct_times"] == ("vec128", True)
    # with 64-row tiles (x3=False) the count doubles
    assert _ct(1984, batch=60, x3=False) == ("vec64", False) and _ct(1988, batch=60, x3=False) == ("vec64", True)


def test_gemm_small_tiles_of_the_f32_mfma_form():
    """768 < wg128 < 2304 picks 64-row tiles -- only on the f32-MFMA form of the vec kernel (COATTN_GEMM_X3 = 0, a developer
    switch): by default launch_gemm_f32 takes the three-piece form first, which has 128-row tiles at every size."""
    for batch, want in ((768, "vec128"), (769, "vec64"), (2303, "vec64"), (2304, "vec128")):
        assert _ct(128, batch=batch, x3=False)[0] == want, batch           # wg128 = 1 * 1 * batch
        assert _ct(128, batch=batch)[0] == "vec128"


# ---- the small kernels ---------------------------------------------------------------------------------------------------------
def test_gemv_kernel_and_workgroups_along_i():
    assert G.gemv_kernel(256, 1, 300) == ("icontig", 1) and G.gemv_kernel(257, 1, 300) == ("icontig", 2)
    assert G.gemv_kernel(256, 2, 300) == ("generic", 1) and G.gemv_kernel(257, 2, 300) == ("generic", 2)
    assert G.gemv_kernel(257, 300, 1) == ("kcontig", 65)
    # da_v: I = N; v: I = d
    assert G.paths(2, 256, 5, 36, 1, "cm")["gemv"]["da_v"] == ("icontig", 1)
    assert G.paths(2, 257, 5, 36, 1, "cm")["gemv"]["da_v"] == ("icontig", 2)
    assert G.paths(2, 257, 5, 36, 1, "lm")["gemv"]["da_v"] == ("kcontig", 65)
    assert G.paths(2, 257, 5, 36, 1, "strided")["gemv"]["da_v"] == ("kcontig", 65)
    assert G.paths(2, 7, 5, 256, 1, "lm")["gemv"]["v"] == ("icontig", 1) and G.paths(2, 7, 5, 257, 1, "lm")["gemv"]["v"] == ("icontig", 2)
    assert G.paths(2, 7, 5, 257, 1, "cm")["gemv"]["v"] == ("kcontig", 65)
    assert G.paths(2, 7, 5, 513, 1, "sd2")["gemv"]["v"] == ("generic", 3) and G.paths(2, 257, 5, 20, 1, "sd2")["gemv"]["da_v"] == ("generic", 2)
    p = G.paths(2, 7, 5, 513, 1, "cm")["gemv"]
    assert p["q"] == ("icontig", 3) and p["da_q"] == ("kcontig", 2)


def test_mask_rows_grid_cap():
    assert G.mask_rows_grid(1023, 256) == (1023, False)        # R W = 262,144 - 256
    assert G.mask_rows_grid(1024, 256) == (1024, False)        # = 262,144: the cap, still one pass
    assert G.mask_rows_grid(1025, 256) == (1024, True)         # + 256: a grid-stride loop
    assert G.mask_rows_grid(262145, 1) == (1024, True)
    assert G.paths(2, 512, 512, 36, 1)["mask_rows"] == (1024, False) and G.paths(2, 600, 600, 36, 1)["mask_rows"] == (1024, True)
    assert G.paths(2, 257, 29, 100, 2)["mask_rows"] == (30, False)


def test_colsum_chunks():
    assert G.colsum_plan(8192) == (32, 256) and G.colsum_plan(8193) == (33, 249)
    assert G.colsum_plan(8481) == (34, 250) and 34 * 250 > 8481 > 34 * 249        # a short last chunk
    assert G.colsum_plan(1) == (32, 1) and G.colsum_plan(33) == (32, 2)
    assert G.paths(32, 256, 5, 100, 2)["colsum"]["dw_v"] == (32, 256)
    p = G.paths(33, 257, 5, 100, 2)
    assert p["colsum"]["dw_v"] == (34, 250) and p["colsum"]["db_v"] == (34, 250) and p["colsum"]["dw_q"] == (32, 6)
    assert p["colsum"]["db_q"] == (32, 11)
    assert G.paths(2, 7, 5, 512, 1)["colsum_blocks"] == 2 and G.paths(2, 7, 5, 513, 1)["colsum_blocks"] == 3
    assert 260 >= max(nch for _, nch in (G.colsum_plan(R) for R in (8193, 65535 * 4096, 4096 * 8))), "plan_bwd's 260 d part region"


def test_reduce_and_add_kernels():
    # a tail behind the groups of eight, and the scalar kernels for n % 4 != 0
    p = G.paths(33, 257, 5, 100, 2)
    assert p["reduce"]["dw_v"] == ("reduce4", 250) and p["reduce"]["dW_v"] == ("reduce4", 17) and p["reduce"]["dW_q"] == ("reduce4", 11)
    p = G.paths(2, 70, 30, 513, 2)
    assert p["reduce"]["dw_v"] == ("reduce1", 5) and p["reduce"]["dW_v"] == ("reduce1", 2)
    assert p["add"] == "add4" and G.paths(2, 601, 599, 37, 1)["add"] == "add1"        # (B N d = 71,820 / 44,474)
    assert G.paths(2, 70, 30, 514, 2)["reduce"]["dW_v"][0] == "reduce4" and G.paths(2, 70, 30, 514, 2)["reduce"]["db_v"][0] == "reduce1"
    assert G.paths(3, 1025, 33, 260, 2)["add"] == "add4" and G.paths(3, 1025, 33, 37, 2)["add"] == "add1"
    assert G.paths(4, 1025, 33, 37, 2)["add"] == "add4"


def test_sample_groups_and_splitk():
    for B, want in ((32, (1, 32)), (33, (2, 17)), (64, (2, 32)), (65, (3, 22)), (160, (5, 32))):
        assert G.sample_groups(B) == want and G.paths(B, 9, 3, 20, 1)["groups"] == want, B
    assert 2 * 17 > 33 and 3 * 22 > 65                         # short last groups
    assert G.splitk_plan(165) == (16, 11) and G.splitk_plan(512) == (16, 32) and G.splitk_plan(513) == (32, 17)
    assert G.splitk_plan(1) == (16, 1) and G.splitk_plan(65535 * 4096)[1] <= 32
    assert G.paths(33, 257, 5, 100, 2)["splitk"] == (16, 11)


def test_softmax_passes():
    assert G.paths(2, 256, 29, 100, 2)["softmax"] == (1, 1) and G.paths(2, 257, 29, 100, 2)["softmax"] == (2, 1)
    assert G.paths(2, 4096, 5, 36, 3)["softmax"] == (16, 1) and G.paths(1, 7, 4096, 20, 1)["softmax"] == (1, 16)


# ---- projection_jobs ---------------------------------------------------------------------------------------------------------
def test_projection_jobs_thresholds():
    p = G.paths
    # B T = 127 / 128 (q_w), with v_w on B N = 127 / 128 beside it
    assert p(127, 1, 1, 64, 1, "lm")["q_w"] is False and p(128, 1, 1, 64, 1, "lm")["q_w"] is True
    assert p(127, 1, 1, 64, 1, "lm")["v_w"] is False and p(128, 1, 1, 64, 1, "lm")["v_w"] is True
    assert (p(2, 256, 29, 512, 3)["v_w"], p(2, 256, 29, 512, 3)["q_w"]) == (True, False)
    assert (p(5, 256, 29, 256, 3)["v_w"], p(5, 256, 29, 256, 3)["q_w"]) == (True, True)
    assert (p(5, 20, 29, 256, 3)["v_w"], p(5, 20, 29, 256, 3)["q_w"]) == (False, True)
    assert (p(2, 20, 29, 256, 3)["v_w"], p(2, 20, 29, 256, 3)["q_w"]) == (False, False)
    # d % 32
    for d, want in ((32, True), (48, False), (100, False), (260, False), (288, True)):
        r = p(5, 256, 29, d, 3, "lm")
        assert (r["v_w"], r["q_w"], r["wqT"]) == (want,) * 3, d
        assert (r["gemm"]["proj_v"] is None) == want and (r["gemm"]["proj_q"] is None) == want
    # channel-major: N % 4 (then sD = N and sB = d N are multiples of 4 too); padded and sD = 2 views never
    assert p(5, 256, 29, 256, 3, "cm")["v_w"] is True and p(5, 257, 29, 256, 3, "cm")["v_w"] is False
    assert p(5, 257, 29, 256, 3, "lm")["v_w"] is True
    assert p(5, 256, 29, 256, 3, "strided")["v_w"] is False and p(5, 256, 29, 256, 3, "sd2")["v_w"] is False
    assert p(5, 256, 29, 256, 3, "strided")["gemm"]["proj_v"] == ("vec128", False)      # rows split by a_mdiv, all % 4
    assert p(5, 256, 29, 256, 3, "sd2")["gemm"]["proj_v"] == ("f32_128", False)
    # the W_q^T image: only when a state is kept
    assert p(5, 256, 29, 256, 3)["wqT"] is True and p(5, 256, 29, 256, 3, keep=False)["wqT"] is False
    # marks
    assert p(5, 256, 29, 256, 3)["marks"] == ["wsplit", "projections"] and p(2, 256, 29, 512, 3)["marks"] == ["wsplit"]
    assert p(5, 20, 29, 256, 3)["marks"] == ["wsplit"] and p(2, 257, 29, 100, 2)["marks"] == []
    assert p(5, 256, 29, 256, 3, flags=GEN | _lib.FLAG_BILINEAR)["marks"] == ["wsplit", "projections", "bilinear_projection"]
    assert p(2, 257, 29, 100, 2, flags=GEN | _lib.FLAG_BILINEAR)["gemm"]["proj_k"] == ("f32_32", False)


def test_row_bitmap_thresholds():
    p = G.paths
    assert p(5, 256, 29, 1024, 3)["rowbits"] is True and p(5, 256, 29, 1280, 3)["rowbits"] is False
    assert p(5, 256, 29, 256, 3)["rowbits"] is True and p(5, 256, 29, 288, 3)["rowbits"] is False     # d % 256
    assert p(4, 256, 29, 256, 3)["rowbits"] is False                                                # no q_w: no bitmap
    # (M + 31) / 32 = 512 / 513 words
    assert p(512, 4, 32, 256, 1)["rowbits"] is True and p(565, 4, 29, 256, 1)["rowbits"] is False
    assert (512 * 32 + 31) // 32 == 512 and (565 * 29 + 31) // 32 == 513


def test_auto_dispatch_leaves_the_fused_path():
    p = G.paths
    assert p(5, 49, 26, 256, 3, "cm", flags=_lib.IMPL_AUTO) == {"fused": True}
    assert p(5, 49, 26, 256, 3, "cm", flags=GEN)["fused"] is False
    for shape in ((5, 49, 26, 256, 4), (5, 49, 29, 256, 3), (5, 209, 26, 256, 3), (5, 49, 26, 260, 3)):
        assert p(*shape, "lm", flags=_lib.IMPL_AUTO)["fused"] is False, shape
    assert p(5, 49, 26, 256, 3, "strided", flags=_lib.IMPL_AUTO)["fused"] is False
    lib = _lib.load()
    for shape in ((5, 49, 26, 256, 3), (5, 49, 26, 256, 4), (5, 49, 29, 256, 3), (5, 208, 28, 512, 3), (5, 209, 26, 256, 3),
                  (5, 49, 26, 260, 3), (5, 49, 26, 4352, 3)):
        assert bool(lib.coattn_fused_supported(*shape, 0)) == G.fused_supported(*shape[1:]), shape


def test_layout_geometry_matches_torch_views():
    import torch
    B, N, d = 3, 5, 8
    views = {
        "lm": torch.empty(B, N, d),
        "cm": torch.empty(B, d, N).permute(0, 2, 1),
        "strided": torch.empty(B * (N * (d + 4) + 8)).as_strided((B, N, d), (N * (d + 4) + 8, d + 4, 1)),
        "sd2": torch.empty(B, N, 2 * d)[:, :, ::2],
    }
    assert set(views) == set(G.LAYOUTS)
    for name, v in views.items():
        n, strides = G.layout_geometry(B, N, d, name)
        assert tuple(v.stride()) == strides and n == v.untyped_storage().nbytes() // 4, name
        assert (N - 1) * strides[1] + (d - 1) * strides[2] < strides[0]


# ---- refusals ------------------------------------------------------------------------------------------------------------------
BASE = dict(B=2, N=7, T=5, d=64, L=2)
BAD_SHAPES = [("N", 4097, b"N=4097"), ("T", 4097, b"T=4097"), ("d", 8193, b"d=8193"), ("L", 9, b"L=9"), ("B", 65536, b"B=65536"),
              ("B", 0, b"B=0")]


def _sizes(**shape):
    lib = _lib.load()
    s, f, b = C.c_size_t(), C.c_size_t(), C.c_size_t()
    rc = lib.coattn_workspace_bytes(shape["B"], shape["N"], shape["T"], shape["d"], shape["L"], _lib.F32, GEN, C.byref(s),
                                    C.byref(f), C.byref(b))
    return rc, (s.value, f.value, b.value), lib.coattn_last_error()


@pytest.mark.parametrize("arg,bad,name", BAD_SHAPES, ids=["%s_%d" % (a, b) for a, b, _ in BAD_SHAPES])
def test_workspace_bytes_refuses_past_the_limits(arg, bad, name):
    rc, _, msg = _sizes(**dict(BASE, **{arg: bad}))
    assert rc < 0 and name in msg, (rc, msg)


def test_workspace_bytes_accepts_the_limits():
    for shape in (dict(BASE, N=4096), dict(BASE, T=4096), dict(BASE, d=8192), dict(BASE, L=8), dict(BASE, B=65535),
                  dict(B=1, N=1, T=1, d=1, L=1)):
        rc, sizes, msg = _sizes(**shape)
        assert rc == 0 and all(x > 0 and x % 256 == 0 for x in sizes), (shape, rc, msg)


class _Host:
    """Host memory standing in for every pointer of a call that is refused before it reads one; the question tables hold
    NULL, which forward_impl / backward_impl refuse right behind the stride checks."""

    def __init__(self):
        self.buf = (C.c_float * 64)()
        self.table = (C.c_void_p * 8)()
        self.p, self.pg = _lib.Params(), _lib.ParamGrads()

    def forward(self, symbol, **kw):
        b = C.addressof(self.buf)
        a = dict(V=b, v_sB=7 * 64, v_sN=64, v_sD=1, Q=self.table, p=self.p, v_out=b, q_out=b, ws=b, dtype=_lib.F32, flags=GEN,
                 stream=None, **BASE)
        names = [n for n, _ in _lib.SIGNATURES[symbol]]
        a.update({n: b for n in ("saved", "av_out", "aq_out", "q_len") if n in names})
        a.update(kw)
        call = _lib.bind(symbol, **a)
        return call.fn(*call), _lib.load().coattn_last_error()

    def backward(self, symbol, **kw):
        b = C.addressof(self.buf)
        a = dict(V=b, v_sB=7 * 64, v_sN=64, v_sD=1, Q=self.table, p=self.p, saved=b, gv=b, gq=b, dV=b, dv_sB=7 * 64, dv_sN=64,
                 dv_sD=1, dQ=self.table, pg=self.pg, accumulate=0, ws=b, dtype=_lib.F32, flags=GEN, stream=None, **BASE)
        if "q_len" in [n for n, _ in _lib.SIGNATURES[symbol]]:
            a["q_len"] = b
        a.update(kw)
        call = _lib.bind(symbol, **a)
        return call.fn(*call), _lib.load().coattn_last_error()


FORWARDS = ("coattn_forward", "coattn_forward_len", "coattn_forward_maps", "coattn_forward_maps_len", "coattn_infer",
            "coattn_infer_len")
BACKWARDS = ("coattn_backward", "coattn_backward_len", "coattn_backward_maps", "coattn_backward_maps_len")
EXTENT = 6 * 64 + 63               # the last element of a location-major sample at (N, d) = (7, 64): sB must be larger


@pytest.mark.parametrize("arg,bad,name", BAD_SHAPES, ids=["%s_%d" % (a, b) for a, b, _ in BAD_SHAPES])
def test_entry_points_refuse_past_the_limits(arg, bad, name):
    h = _Host()
    for symbol in FORWARDS:
        rc, msg = h.forward(symbol, **{arg: bad})
        assert rc < 0 and name in msg, (symbol, rc, msg)
    for symbol in BACKWARDS:
        rc, msg = h.backward(symbol, **{arg: bad})
        assert rc < 0 and name in msg, (symbol, rc, msg)


@pytest.mark.parametrize("kw,names", [
    (dict(v_sN=0), [b"forward: V", b"sN=0"]), (dict(v_sD=0), [b"forward: V", b"sD=0"]), (dict(v_sB=0), [b"forward: V", b"sB=0"]),
    (dict(v_sB=EXTENT), [b"forward: V", b"sample stride %d" % EXTENT]),
], ids=["sN_0", "sD_0", "sB_0", "sB_short"])
def test_forwards_refuse_bad_strides(kw, names):
    h = _Host()
    for symbol in FORWARDS:
        rc, msg = h.forward(symbol, **kw)
        assert rc < 0 and all(n in msg for n in names), (symbol, rc, msg)
    rc, msg = h.forward("coattn_forward", v_sB=EXTENT + 1)     # the smallest stride that holds a sample: the next check speaks
    assert rc < 0 and b"Q[0] is null" in msg, msg


@pytest.mark.parametrize("kw,names", [
    (dict(v_sN=0), [b"backward: V", b"sN=0"]), (dict(v_sB=EXTENT), [b"backward: V", b"sample stride %d" % EXTENT]),
    (dict(dv_sN=0), [b"backward: dV", b"sN=0"]), (dict(dv_sD=0), [b"backward: dV", b"sD=0"]), (dict(dv_sB=0), [b"backward: dV", b"sB=0"]),
    (dict(dv_sB=EXTENT), [b"backward: dV", b"sample stride %d" % EXTENT]),
], ids=["V_sN_0", "V_sB_short", "dV_sN_0", "dV_sD_0", "dV_sB_0", "dV_sB_short"])
def test_backwards_refuse_bad_strides(kw, names):
    h = _Host()
    for symbol in BACKWARDS:
        rc, msg = h.backward(symbol, **kw)
        assert rc < 0 and all(n in msg for n in names), (symbol, rc, msg)
    rc, msg = h.backward("coattn_backward", dv_sB=EXTENT + 1)
    assert rc < 0 and b"Q[0]/dQ[0] is null" in msg, msg
    rc, msg = h.backward("coattn_backward", dV=None, dv_sB=0, dv_sN=0, dv_sD=0)     # without dV its strides are not looked at
    assert rc < 0 and b"Q[0]/dQ[0] is null" in msg, msg

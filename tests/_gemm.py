"""The GEMM layer's C-ABI (coattn_gemm_f32 / coattn_gemm_bf16, coattn_linear_forward, coattn_linear_weight_grad; csrc/gemm.hip,
gemm_w.hip / gemm_w_body.h, gemm_h2.hip, gemm_bf.hip, gemm_tn.hip) for the tests: runners that put every buffer a call
touches inside a marker-filled arena of exactly its size, float64 references of the header's contracts, and the dispatch
rules restated in plain Python (tests/test_gemm_cpu.py pins them at every threshold; tests/test_gpu_gemm_paths.py holds its
tables against them).

The mirrors assume what the runners provide -- every arena starts 16-byte aligned (an operand is unaligned only where a
case offsets it by 1 to 3 floats) -- the defaults of the developer switches, and extents far below the 1 GiB limits.

A general-GEMM case is a dict: the fields of coattn_gemm_desc by name, where A, B, Cin, bias_n and bias_m are 1-D float32
host tensors holding the operand's memory as the strides address it, a_ptrs / b_ptrs / cin_ptrs lists of such tensors,
c_ptrs the number of entries of C's table, and a_off / b_off / cin_off / bn_off / bm_off / c_off offsets in floats of the
operand's first element from its arena's (aligned) start."""
import ctypes as C
import math

import torch

from vqa_amd import _lib

from tests.test_gpu_gemm import _r, _two_piece          # the operands a mode multiplies: bf16-rounded; hi + mid pieces
from tests._general import GUARD_BITS, GUARD_FLOATS, Arena, gemm_kernel  # noqa: F401  (GUARD_FLOATS: the arenas' margin)

BF16_PROJ, BF16_IN, SPLIT2, F16PAIR = _lib.FLAG_BF16_PROJ, _lib.FLAG_BF16_IN, _lib.FLAG_SPLIT2, _lib.FLAG_F16PAIR
REUSE = 1                                  # flags bit 0 of coattn_linear_forward: wimg already holds the image
STRIDES = ("a_sm", "a_sk", "a_sz", "a_si", "a_mdiv", "a_sdiv", "b_sk", "b_sn", "b_sz", "b_si", "c_sm", "c_sn", "c_sz", "c_mdiv",
           "c_sdiv", "cin_sm", "cin_sn", "cin_sz", "cin_mdiv", "cin_sdiv")
SCALARS = ("M", "N", "K", "batch", "inner", "inner_total", "ksplit", "act", "beta", "ptr_by_inner", "b_imod", "kband_n",
           "out_scale") + STRIDES


def _dev():
    return torch.device("cuda:0")


def float_bits(bits):
    """The float32 with the bit pattern `bits` (0x7FFFFFFF, 0xFFFFFFFF: NaNs with every payload bit set)."""
    return torch.tensor([bits - (1 << 32) if bits >= (1 << 31) else bits], dtype=torch.int32).view(torch.float32)[0]


def rel(x, ref):
    return float((x.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-9))


# ---- the header's contract of coattn_gemm_desc, in float64 (or any dtype) ---------------------------------------------------
def _rows(M, sm, mdiv, sdiv):
    m = torch.arange(M)
    return (m // mdiv) * sdiv + (m % mdiv) * sm if mdiv > 0 else m * sm


def c_cells(d, which="c"):
    """Offsets [batch, M, N] (floats, relative to the operand's first element) of the C (or "cin") view; with a pointer
    table the batch stride is 0: entry z of the table is its own buffer."""
    g = lambda k: int(d.get(which + "_" + k, 0))            # noqa: E731
    rows = _rows(d["M"], g("sm"), g("mdiv"), g("sdiv"))
    one = rows[:, None] + torch.arange(d["N"])[None, :] * g("sn")
    sz = 0 if d.get(which + "_ptrs") else g("sz")
    return torch.arange(d.get("batch", 1))[:, None, None] * sz + one[None]


def bands(d):
    """[(n0, n1, k_lo, k_hi)] of the k bands (one band over all of K without them)."""
    N, K, kb = d["N"], d["K"], int(d.get("kband_n", 0))
    if kb <= 0:
        return [(0, N, 0, K)]
    return [(j * kb, min(N, (j + 1) * kb), d["kband_lo"][j], d["kband_hi"][j]) for j in range(-(-N // kb))]


def gemm_reference(d, bf16=False, dtype=torch.float64):
    """C [batch, M, N] as include/coattn.h states it: act(out_scale * (sum_i sum_k A B + bias_n + bias_m) + beta * Cin), the
    operands rounded to bf16 first in the bf16 mode; elements outside the k range of a part or a band are never read.
    dtype = float32: the same contract in float32 torch.matmul arithmetic (what a correct fp32 kernel may give)."""
    M, N, K, batch = d["M"], d["N"], d["K"], d.get("batch", 1)
    g = lambda k: int(d.get(k, 0))                          # noqa: E731
    inner, total, ksplit = max(g("inner"), 1), g("inner_total"), g("ksplit")
    rnd = lambda x: _r(x, bf16).to(dtype)                   # noqa: E731
    ar, n_all = _rows(M, g("a_sm"), g("a_mdiv"), g("a_sdiv")), torch.arange(N)
    osc = float(d.get("out_scale", 0.0)) or 1.0
    out = torch.zeros(batch, M, N, dtype=dtype)
    cin = c_cells(d, "cin") if (d.get("Cin") is not None or d.get("cin_ptrs")) else None
    for z in range(batch):
        k0, k1 = (z * ksplit, min(K, (z + 1) * ksplit)) if ksplit > 0 else (0, K)
        nin = inner if total <= 0 else max(0, min(inner, total - z * inner))
        acc = torch.zeros(M, N, dtype=dtype)
        for i in range(nin):
            ig = z * inner + i if total > 0 else i
            pt = ig if g("ptr_by_inner") else z
            Ab, a0 = (d["a_ptrs"][pt], 0) if d.get("a_ptrs") else (d["A"], z * g("a_sz") + i * g("a_si"))
            if d.get("b_ptrs"):
                Bb, b0 = d["b_ptrs"][pt], 0
            else:
                Bb, b0 = d["B"], ((ig % g("b_imod")) * g("b_si") if g("b_imod") > 0 else z * g("b_sz") + i * g("b_si"))
            for n0, n1, lo, hi in bands(d):
                if min(k1, hi) <= max(k0, lo):
                    continue
                ks = torch.arange(max(k0, lo), min(k1, hi))
                Am = Ab[a0 + ar[:, None] + ks[None, :] * g("a_sk")]
                Bm = Bb[b0 + ks[:, None] * g("b_sk") + n_all[None, n0:n1] * g("b_sn")]
                acc[:, n0:n1] += rnd(Am) @ rnd(Bm)
        if d.get("bias_n") is not None:
            acc = acc + d["bias_n"].to(dtype)[None, :]
        if d.get("bias_m") is not None:
            acc = acc + d["bias_m"].to(dtype)[:, None]
        acc = acc * osc
        if cin is not None:
            buf = d["cin_ptrs"][z] if d.get("cin_ptrs") else d["Cin"]
            acc = acc + float(d.get("beta", 0.0)) * buf[cin[z]].to(dtype)
        out[z] = torch.tanh(acc) if g("act") == 1 else acc
    return out


# ---- runners -------------------------------------------------------------------------------------------------------------------
def _place(buf, off=0):
    """A host buffer in an arena of exactly its size (+ `off` floats in front of it): (arena, device pointer)."""
    a = Arena(buf.numel() + off, fill=None)
    a.body[off:].copy_(buf)
    return a, a.body.data_ptr() + 4 * off


def _table(ptrs):
    return (C.c_void_p * 8)(*(list(ptrs) + [None] * (8 - len(ptrs))))


def run_gemm(d, bf16=False, finite=True):
    """One coattn_gemm_f32 / coattn_gemm_bf16 call on case `d` (see the module's docstring).  C lives in an arena of exactly
    the span of its view (one arena per entry of a c_ptrs table), marker-filled with NaN in the view's cells; A, B, Cin and
    the biases sit in arenas of their own.  After the call every arena's margins hold the marker, every cell of C's arena
    outside the view still does, and -- unless finite=False -- every cell of the view is finite.  Returns C [batch, M, N] on
    the host."""
    lib = _lib.load()
    g = _lib.GemmDesc()
    for k in SCALARS:
        if k in d:
            setattr(g, k, d[k])
    for j in range(3):
        if "kband_lo" in d:
            g.kband_lo[j], g.kband_hi[j] = d["kband_lo"][j], d["kband_hi"][j]
    arenas = {}
    for name, off in (("A", "a_off"), ("B", "b_off"), ("Cin", "cin_off"), ("bias_n", "bn_off"), ("bias_m", "bm_off")):
        if d.get(name) is not None:
            arenas[name], p = _place(d[name], int(d.get(off, 0)))
            setattr(g, name, p)
    for name in ("a_ptrs", "b_ptrs", "cin_ptrs"):
        if d.get(name):
            ptrs = []
            for t, buf in enumerate(d[name]):
                arenas["%s[%d]" % (name, t)], p = _place(buf)
                ptrs.append(p)
            setattr(g, name, _table(ptrs))
    cells = c_cells(d, "c")
    c_off = int(d.get("c_off", 0))
    nc = int(d.get("c_ptrs", 0))
    outs = []
    for t in range(nc if nc else 1):
        idx = (cells[t] if nc else cells).reshape(-1).to(_dev()) + c_off
        assert int(idx.min()) == c_off and idx.unique().numel() == idx.numel(), "the C view must start at 0 and not overlap"
        a = Arena(int(idx.max()) + 1, fill=None)
        a.body[idx] = float("nan")
        arenas["C[%d]" % t] = a
        outs.append((a, idx))
    if nc:
        g.c_ptrs = _table([a.body.data_ptr() + 4 * c_off for a, _ in outs])
    else:
        g.C = outs[0][0].body.data_ptr() + 4 * c_off
    fn = lib.coattn_gemm_bf16 if bf16 else lib.coattn_gemm_f32
    rc = fn(C.byref(g), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.coattn_last_error()
    torch.cuda.synchronize()
    for k, a in arenas.items():
        a.check(k)
    res = []
    for a, idx in outs:
        rest = a.body.view(torch.int32).clone()
        rest[idx] = GUARD_BITS
        assert bool((rest == GUARD_BITS).all()), "a cell of C's arena outside the view was written"
        res.append(a.body[idx].cpu())
    out = (torch.stack(res) if nc else res[0]).reshape(cells.shape)
    if finite:
        assert bool(torch.isfinite(out).all()), "a cell of C is not finite (left unwritten, or computed from a cell never to be read)"
    return out


def linear_call(x_ptr, ld, W_ptr, bias_ptr, y_ptr, wimg_ptr, M, N, K, scale, flags, stream=None):
    lib = _lib.load()
    rc = lib.coattn_linear_forward(x_ptr, ld, W_ptr, bias_ptr, y_ptr, wimg_ptr, M, N, K, scale, flags, C.c_void_p(stream))
    return rc, lib.coattn_last_error()


def wgrad_call(dy_ptr, ld_dy, x_ptr, ld_x, dW_ptr, ws_ptr, M, n_out, n_in, accumulate, stream=None):
    lib = _lib.load()
    rc = lib.coattn_linear_weight_grad(dy_ptr, ld_dy, x_ptr, ld_x, dW_ptr, ws_ptr, M, n_out, n_in, accumulate,
                                       C.c_void_p(stream))
    return rc, lib.coattn_last_error()


def _place_rows(t, rows, ld, width, bf16_stored):
    """`t` [rows, width] in an arena of exactly (rows - 1) * ld + width elements, the padding holding the marker."""
    n = (rows - 1) * ld + width
    if bf16_stored:                                          # bf16 elements: two to a float of the arena
        a = Arena((n + 1) // 2, fill=None)
        flat = a.body.view(torch.bfloat16)[:n]
    else:
        a = Arena(n, fill=None)
        flat = a.body
    torch.as_strided(flat, (rows, width), (ld, 1)).copy_(t[:, :width])
    return a


def run_linear(x, ld, W, bias, M, N, K, scale, flags, wimg=None):
    """One coattn_linear_forward: x [M, K] (host; bf16-stored under COATTN_FLAG_BF16_IN) rows ld apart, W [N, K], bias [N]
    or None.  y, wimg and x get arenas of exactly M N floats, coattn_linear_workspace_bytes and the span of x; a wimg handed
    back in (flags bit 0) must come back bit-identical.  Returns (y on the host, the wimg arena)."""
    lib = _lib.load()
    stored = bool(flags & BF16_IN)
    ax = _place_rows(x.bfloat16() if stored else x.float(), M, ld, K, stored)
    aw, _ = _place(W.float().reshape(-1))
    arenas = {"x": ax, "W": aw}
    bp = None
    if bias is not None:
        arenas["bias"], bp = _place(bias.float())
    ay = Arena(M * N)
    arenas["y"] = ay
    nbytes = lib.coattn_linear_workspace_bytes(N, K)
    assert nbytes == linear_workspace_bytes(N, K) and nbytes % 4 == 0
    before = None
    if wimg is None:
        assert not flags & REUSE
        wimg = Arena(nbytes // 4)
    else:
        assert wimg.n == nbytes // 4
        before = wimg.body.view(torch.int32).clone() if flags & REUSE else None
    arenas["wimg"] = wimg
    rc, msg = linear_call(ax.body.data_ptr(), ld, aw.body.data_ptr(), bp, ay.body.data_ptr(), wimg.body.data_ptr(), M, N, K,
                          scale, flags, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, msg
    torch.cuda.synchronize()
    for k, a in arenas.items():
        a.check(k)
    if before is not None:
        assert torch.equal(before, wimg.body.view(torch.int32)), "a reused weight image was written"
    y = ay.body.view(M, N).cpu()
    assert bool(torch.isfinite(y).all()), "a cell of y is not finite"
    return y, wimg


def run_wgrad(dy, ld_dy, x, ld_x, M, n_out, n_in, accumulate, dW0=None):
    """One coattn_linear_weight_grad: dy [M, n_out] (bf16-stored under COATTN_FLAG_BF16_IN), x [M, n_in] on the host.  dW
    and ws get arenas of exactly n_out n_in floats (holding dW0 when given, else NaN) and
    coattn_linear_wgrad_workspace_bytes.  Returns dW on the host."""
    lib = _lib.load()
    stored = bool(accumulate & BF16_IN)
    ady = _place_rows(dy.bfloat16() if stored else dy.float(), M, ld_dy, n_out, stored)
    axx = _place_rows(x.float(), M, ld_x, n_in, False)
    adw = Arena(n_out * n_in)
    if dW0 is not None:
        adw.body.copy_(dW0.float().reshape(-1))
    nbytes = lib.coattn_linear_wgrad_workspace_bytes(n_out, n_in)
    assert nbytes == wgrad_workspace_bytes(n_out, n_in) and nbytes % 4 == 0
    aws = Arena(nbytes // 4)
    rc, msg = wgrad_call(ady.body.data_ptr(), ld_dy, axx.body.data_ptr(), ld_x, adw.body.data_ptr(), aws.body.data_ptr(), M,
                         n_out, n_in, accumulate, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, msg
    torch.cuda.synchronize()
    for k, a in (("dy", ady), ("x", axx), ("dW", adw), ("ws", aws)):
        a.check(k)
    dW = adw.body.view(n_out, n_in).cpu()
    assert bool(torch.isfinite(dW).all()), "a cell of dW is not finite"
    return dW


# ---- the dispatch rules, restated ----------------------------------------------------------------------------------------------
def _al4(*xs):
    return all(int(x) % 4 == 0 for x in xs)


def _strides(d):
    return {k: int(d.get(k, 0)) for k in ("a_sm", "a_sk", "a_sz", "a_si", "a_mdiv", "a_sdiv", "b_sk", "b_sn", "b_sz", "b_si",
                                          "ksplit")}


def _aligned(d):
    """A and B (and every table entry) 16-byte aligned: the arenas are, unless the case offsets the operand."""
    return int(d.get("a_off", 0)) % 4 == 0 and int(d.get("b_off", 0)) % 4 == 0


def gemm_f32_kernel(**d):
    """launch_gemm_f32 (csrc/gemm.hip) on a case: (kernel, xcd_group) of tests/_general.py gemm_kernel, where an operand
    that is not 16-byte aligned leaves the vector form as an unaligned stride does."""
    if _aligned(d):
        return gemm_kernel(d["M"], d["N"], d["K"], d.get("batch", 1), **_strides(d))
    return ("f32_32" if d["M"] <= 64 else "f32_128"), False


def gemm_bf16_kernel(**d):
    """launch_gemm_bf16in (csrc/gemm.hip): "vec128_bf16" (every shape the aligned path takes, all descriptor fields),
    "bf16in_am_vec" / "bf16in_am_scalar" / "bf16in_ak" (gemm_bf16in_kernel<AM, AVEC>: B contiguous along k, and of the
    descriptor only bias_n, out_scale, an a_ptrs table by batch and the row splits of A and C; an inner_total that covers
    every batch entry at inner <= 1 clips nothing and is let through), or "exact:" + the kernel of launch_gemm_f32 for
    everything else."""
    if gemm_f32_kernel(**d)[0].startswith("vec"):
        return "vec128_bf16"
    s = _strides(d)
    a_m = s["a_sm"] == 1 and s["a_sk"] != 1
    has = lambda k: d.get(k) is not None and d.get(k) != [] and d.get(k) != 0       # noqa: E731
    ok = (_aligned(d) and (not has("a_ptrs") or d.get("batch", 1) <= 8) and not has("b_ptrs") and not has("c_ptrs")
          and not has("Cin") and not has("bias_m") and int(d.get("act", 0)) == 0 and int(d.get("inner", 0)) <= 1
          and s["ksplit"] == 0 and not int(d.get("ptr_by_inner", 0))
          and int(d.get("kband_n", 0)) == 0 and not has("cin_ptrs") and int(d.get("b_imod", 0)) == 0
          and (int(d.get("inner_total", 0)) == 0 or int(d.get("inner_total", 0)) >= d.get("batch", 1))
          and s["b_sk"] == 1 and _al4(s["b_sn"], d["K"]) and (a_m or (s["a_sk"] == 1 and _al4(s["a_sm"])))
          and _al4(s["a_sz"], s["b_sz"]))
    if not ok:
        return "exact:" + gemm_f32_kernel(**d)[0]
    if not a_m:
        return "bf16in_ak"
    return "bf16in_am_vec" if _al4(d["M"], s["a_sk"], s["a_mdiv"], s["a_sdiv"]) else "bf16in_am_scalar"


def gemm_bf16_xcd_group(**d):
    """xcd_group of the bf16 entry's kernels: 32 or more 128-row tiles on the vector form and on gemm_bf16in_kernel."""
    return not gemm_bf16_kernel(**d).startswith("exact:") and -(-d["M"] // 128) >= 32


def linear_workspace_bytes(N, K):
    """wsplit_bytes (csrc/gemm_w.hip): three 1 KB fragments per (32 columns, 16 k) chunk."""
    return -(-N // 32) * -(-K // 16) * 3072 if N > 0 and K > 0 else 0


def wgrad_workspace_bytes(n_out, n_in):
    """32 split-K parts of n_out x n_in floats."""
    return 32 * n_out * n_in * 4 if n_out > 0 and n_in > 0 else 0


def _modes(flags):
    bf16 = bool(flags & BF16_PROJ)
    f16 = bool(flags & F16PAIR) and not bf16
    np_ = 2 if (flags & SPLIT2 or f16) else 3
    return bf16, f16, np_, bool(flags & BF16_IN)


def linear_kernel(M, N, K, ld, flags, aligned=True):
    """coattn_linear_forward -> gemm_wx_kernel -> the template launch_gemm_w / launch_gemm_h2 / launch_gemm_bf pick:
    (pieces of the weight image: 1, 3 or 16; xcd_group; kernel).  xcd_group: gemm_w groups its row tiles by XCD from 32 row
    tiles on; gemm_h2, gemm_h2p and gemm_bf always pad the row tiles to a multiple of 8 (reported as True).
    ("refused": (0, False, "refused").)"""
    refused = (0, False, "refused")
    bf16, f16, np_, stored = _modes(flags)
    if not (M > 0 and N > 0 and K > 0 and K <= ld < (1 << 24)) or (stored and not bf16):
        return refused
    small = (M * ld + K) * 4 < 0x40000000 and linear_workspace_bytes(N, K) < 0x40000000
    bf_ok = (bf16 and M >= 256 and N >= 256 and N % 256 == 0 and K >= 64 and K % 64 == 0 and ld % 4 == 0 and aligned and small
             and (not stored or ld % 8 == 0))
    w_ok = not stored and M >= (1 if f16 else 128) and K >= 32 and K % 32 == 0 and ld % 4 == 0 and aligned and small
    if not (bf_ok if stored else w_ok):
        return refused
    if bf_ok:
        return 1, True, "gemm_bf"
    pieces = 16 if f16 else 3
    if f16 and N >= 256 and N % 256 == 0:
        return pieces, True, ("gemm_h2p" if K == 512 else "gemm_h2")
    xcd = -(-M // 128) >= 32
    if f16:
        return pieces, xcd, "gemm_w_f16"
    if bf16:
        return pieces, xcd, ("gemm_w_bf16_wide" if N % 256 == 0 else "gemm_w_bf16")
    return pieces, xcd, ("gemm_w2" if np_ == 2 else "gemm_w3")


def gemm_tn_plan(M, n_out, n_in, max_parts=32):
    """gemm_tn_plan (csrc/gemm_tn.hip), one level: (ks, parts) -- the parts fill 512 workgroup slots once, at most 32."""
    ntiles = (n_out // 128) * (n_in // 128)
    want = max(1, min(-(-512 // ntiles), max_parts))
    ks = -(-(-(-M // want)) // 16) * 16
    return ks, -(-M // ks)


def gemm_bf_tn_plan(M, n_out, n_in):
    """coattn_linear_weight_grad's request (one round of 256 workgroups, at most 32 parts) through gemm_bf_tn_plan
    (csrc/gemm_bf.hip): (32-row steps per part, parts)."""
    ntiles = (n_out // 256) * (n_in // 256)
    total = M // 32
    want = max(1, min(min(-(-256 // ntiles), 32), total))
    spp = -(-total // want)
    return spp, -(-total // spp)


def wgrad_plan(M, n_out, n_in, ld_dy, ld_x, accumulate, aligned=True):
    """coattn_linear_weight_grad: ("refused" | "gemm_tn" | "gemm_bf_tn", ks or steps per part, parts)."""
    refused = ("refused", 0, 0)
    bf16, _, _, stored = _modes(accumulate)
    if not (M > 0 and n_out > 0 and n_in > 0 and n_out <= ld_dy < (1 << 24) and n_in <= ld_x < (1 << 24)):
        return refused
    if stored and not bf16:
        return refused
    al = ld_dy % 4 == 0 and ld_x % 4 == 0 and aligned
    bf_ok = (bf16 and n_out >= 256 and n_in >= 256 and n_out % 256 == 0 and n_in % 256 == 0 and M >= 32 and M % 32 == 0 and al
             and M * max(ld_dy, ld_x) * 4 < 0x40000000 and (not stored or ld_dy % 8 == 0))
    tn_ok = (not stored and n_out % 128 == 0 and n_in % 128 == 0 and M >= 16 and al
             and (M + 32) * max(ld_dy, ld_x) * 4 < 0x40000000)
    if not (bf_ok if stored else tn_ok):
        return refused
    if bf_ok:
        return ("gemm_bf_tn",) + gemm_bf_tn_plan(M, n_out, n_in)
    return ("gemm_tn",) + gemm_tn_plan(M, n_out, n_in)


def h2p_tiles(M, N):
    """Padded tiles the persistent gemm_h2p_kernel walks: the row tiles rounded up to a multiple of 8, per 256 columns."""
    return (N // 256) * (-(-(-(-M // 128)) // 8) * 8)


# ---- cases of the general GEMM ---------------------------------------------------------------------------------------------------
def _c_layout(prefix, kind, M, N, mdiv, pad):
    """Strides of a C / Cin view: "n" row-major (rows N + pad apart), "t" transposed, "div" rows split by mdiv with the
    columns mdiv apart (a [groups][N][mdiv] buffer, as the channel-major dV is written)."""
    if kind == "n":
        s = dict(sm=N + pad, sn=1, sz=M * (N + pad))
    elif kind == "t":
        s = dict(sm=1, sn=M + pad, sz=N * (M + pad))
    else:
        s = dict(sm=1, sn=mdiv, mdiv=mdiv, sdiv=N * mdiv + pad, sz=-(-M // mdiv) * (N * mdiv + pad))
    return {prefix + "_" + k: v for k, v in s.items()}


def gemm_case(M, N, K, batch=1, a="k", b="k", seed=0, data=True, a_mdiv=0, a_pad=0, b_pad=0, a_si_odd=False, c="n", c_mdiv=0,
              c_pad=0, bias_n=False, bias_m=False, cin=None, cin_mdiv=0, cin_pad=0, beta=0.0, act=0, out_scale=0.0, ksplit=0,
              inner=0, inner_total=0, b_imod=0, a_tab=False, b_tab=False, c_tab=False, cin_tab=False, by_inner=False,
              kband_n=0, kband=(), nan_outside=False, poke=(), **offs):
    """A case of run_gemm / gemm_reference / the mirrors.
    a: "k" A[M][K + a_pad] rows, "m" A[K][M + a_pad] (contiguous along m), with a_mdiv the channel-major [groups][K][a_mdiv];
    b: "k" B[N][K + b_pad] (nn.Linear's weight), "n" B[K][N + b_pad];  c / cin: see _c_layout.
    batch entries (or, with inner, the inner_total / inner indices) have operands of their own; ksplit: ONE product whose k
    range the batch index cuts.  b_imod: B has b_imod blocks that the inner index wraps over.  *_tab: the operand through
    its pointer table (by batch, or with by_inner by inner index).  kband: ((lo, hi), ...) per band of kband_n columns;
    nan_outside: B holds NaN wherever a band does not read.  a_si_odd: an inner stride of A of 2 floats that no kernel
    uses (inner <= 1) -- it only keeps the shape off the aligned path.  poke: ((operand, block, i, j, bits), ...) writes a
    bit pattern into A(block)(i, j) / B(block)(i, j).  data=False: the scalar fields only (presence of an operand: True).
    Every pad of an operand holds NaN: nothing may read it."""
    G = torch.Generator().manual_seed(1000 + seed)
    d = dict(M=M, N=N, K=K, batch=batch, act=act, beta=beta, out_scale=out_scale, ksplit=ksplit, inner=inner,
             inner_total=inner_total, b_imod=b_imod, ptr_by_inner=int(by_inner), kband_n=kband_n)
    d.update(offs)
    if ksplit:
        assert batch == -(-K // ksplit) and not inner
    nblk = 1 if ksplit else ((inner_total or inner * batch) if inner else batch)
    nblk_b = b_imod if b_imod else nblk
    # A
    if a_mdiv:
        assert a == "m"
        grp = -(-M // a_mdiv)
        d.update(a_sm=1, a_sk=a_mdiv, a_mdiv=a_mdiv, a_sdiv=K * a_mdiv + a_pad)
        blk_a = grp * (K * a_mdiv + a_pad)
    elif a == "m":
        d.update(a_sm=1, a_sk=M + a_pad)
        blk_a = K * (M + a_pad)
    else:
        d.update(a_sm=K + a_pad, a_sk=1)
        blk_a = M * (K + a_pad)
    if b == "n":
        d.update(b_sk=N + b_pad, b_sn=1)
        blk_b = K * (N + b_pad)
    else:
        d.update(b_sk=1, b_sn=K + b_pad)
        blk_b = N * (K + b_pad)
    if not ksplit:
        if inner:
            d.update(a_si=blk_a, a_sz=inner * blk_a)
            d.update(b_si=blk_b) if b_imod else d.update(b_si=blk_b, b_sz=inner * blk_b)
        else:
            d.update(a_sz=blk_a, b_sz=blk_b)
            if b_imod:
                d.update(b_si=blk_b)
    if a_si_odd:
        assert inner <= 1
        d["a_si"] = 2
    d.update(_c_layout("c", c, M, N, c_mdiv, c_pad))
    if cin:
        d.update(_c_layout("cin", cin, M, N, cin_mdiv, cin_pad))
    if kband_n:
        lo = [kb[0] for kb in kband] + [0] * (3 - len(kband))
        hi = [kb[1] for kb in kband] + [0] * (3 - len(kband))
        d.update(kband_lo=lo, kband_hi=hi)
    if not data:
        d.update(A=None if a_tab else True, B=None if b_tab else True, a_ptrs=[True] * nblk if a_tab else None,
                 b_ptrs=[True] * nblk_b if b_tab else None, c_ptrs=batch if c_tab else 0,
                 Cin=True if (cin and not cin_tab) else None, cin_ptrs=[True] * batch if (cin and cin_tab) else None,
                 bias_n=True if bias_n else None, bias_m=True if bias_m else None)
        return d
    nan = float("nan")
    amp = 0.25 if act else 1.0                             # (tanh: arguments of order 1, where an absolute bound is as tight as a relative one)
    # (the significand pattern of _low_bits: on the three-piece form a dropped partial product then shows at 2e-6; the
    #  scales are powers of two, which keep it)
    A_log = _low_bits(torch.randn(nblk, M, K, generator=G)) * amp
    B_log = _low_bits(torch.randn(nblk_b, K, N, generator=G)) * 2.0 ** -round(math.log2(max(K * max(inner, 1), 1)) / 2 + 0.5)
    if nan_outside:
        for n0, n1, lo_, hi_ in bands(d):
            B_log[:, :lo_, n0:n1] = nan
            B_log[:, hi_:, n0:n1] = nan
    for op, blk, i, j, bits in poke:
        (A_log if op == "A" else B_log)[blk, i, j] = float_bits(bits)

    def lay_a(x):                                            # [M, K] -> the block's memory
        if a_mdiv:
            full = torch.full((grp * a_mdiv, K), nan)
            full[:M] = x
            body = full.view(grp, a_mdiv, K).permute(0, 2, 1).reshape(grp, K * a_mdiv)
            return torch.cat([body, torch.full((grp, a_pad), nan)], 1).reshape(-1)
        x = x.t() if a == "m" else x
        return torch.cat([x, torch.full((x.shape[0], a_pad), nan)], 1).reshape(-1)

    def lay_b(x):                                            # [K, N]
        x = x if b == "n" else x.t()
        return torch.cat([x, torch.full((x.shape[0], b_pad), nan)], 1).reshape(-1)

    a_blocks, b_blocks = [lay_a(x) for x in A_log], [lay_b(x) for x in B_log]
    d["A"], d["a_ptrs"] = (None, a_blocks) if a_tab else (torch.cat(a_blocks), None)
    d["B"], d["b_ptrs"] = (None, b_blocks) if b_tab else (torch.cat(b_blocks), None)
    d["c_ptrs"] = batch if c_tab else 0
    d["bias_n"] = torch.randn(N, generator=G) * amp if bias_n else None
    d["bias_m"] = torch.randn(M, generator=G) * amp if bias_m else None
    d["Cin"], d["cin_ptrs"] = None, None
    if cin:
        cells = c_cells(dict(d, cin_ptrs=None), "cin")
        per = int(d["cin_sz"])
        bufs = []
        for z in range(batch):
            buf = torch.full((per,), nan)
            buf[(cells[z] - z * per).reshape(-1)] = torch.randn(M * N, generator=G) * amp
            bufs.append(buf)
        if cin_tab:
            d["cin_ptrs"] = bufs
        else:
            d["Cin"] = torch.cat(bufs)
    return d


# ---- inputs and references of the linear entry points ---------------------------------------------------------------------------
def _low_bits(t):
    """Values (|t| + 0.5, the sign kept) whose sixteen lowest significand bits are 0x7F3F: hi rounds towards zero, mid is
    0x7F00 units and lo 0x3F units of the same sign as the value.  Every term the two-piece width drops (mid * mid,
    lo * hi, hi * lo) then has the sign of its product x w, so what is dropped is ~2e-5 of the result wherever the result
    is large -- inside the width's 3e-5 budget and far enough from the true product for a 2e-6 bound to tell the two
    apart at every K (with unrelated signs the distance shrinks to the bound itself).  On the exact three-piece width the
    same pattern makes each single partial product that a kernel could drop worth 5e-6 or more of the result."""
    t = torch.where(t < 0, t - 0.5, t + 0.5)
    return ((t.view(torch.int32) & ~0xFFFF) | 0x7F3F).view(torch.float32)


def linear_inputs(M, N, K, flags, seed=0):
    """x [M, K], W [N, K], bias [N], and x2 (the values of the second, image-reusing call)."""
    G = torch.Generator().manual_seed(2000 + seed)
    x, x2 = torch.randn(M, K, generator=G), torch.randn(M, K, generator=G)
    W, b = torch.randn(N, K, generator=G) / K ** 0.5, torch.randn(N, generator=G)
    if not flags & (BF16_PROJ | F16PAIR):                    # the bf16-piece widths: exact (three pieces) and SPLIT2 (two)
        x, x2, W = _low_bits(x), _low_bits(x2), _low_bits(W)
    if flags & BF16_IN:
        x, x2 = x.bfloat16().float(), x2.bfloat16().float()
    return x, W, b, x2


def product_reference(a, bt, flags, dtype=torch.float64, neighbour=False):
    """a [M, K] times bt [N, K]^T on the operands the mode of `flags` multiplies: rounded to bf16 (COATTN_FLAG_BF16_PROJ),
    the three partial products of the hi + mid pieces (COATTN_FLAG_SPLIT2), the values themselves otherwise (exact, and
    COATTN_FLAG_F16PAIR, whose 22 bits are held to the true product).  neighbour=True: the mode next to it, which the
    row's bound must exclude -- the true product for the first two, the product of the FP16 hi pieces alone for F16PAIR."""
    bf16, f16, np_, _ = _modes(flags)
    if neighbour:
        assert bf16 or f16 or np_ == 2
        if f16:
            return a.half().to(dtype) @ bt.half().to(dtype).t()
        return a.to(dtype) @ bt.to(dtype).t()
    if bf16:
        return _r(a, True).to(dtype) @ _r(bt, True).to(dtype).t()
    if np_ == 2 and not f16:
        (ah, am), (bh, bm) = _two_piece(a), _two_piece(bt)
        return ((ah + am).to(dtype) @ bh.to(dtype).t()) + (ah.to(dtype) @ bm.to(dtype).t())
    return a.to(dtype) @ bt.to(dtype).t()


def linear_reference(x, W, b, scale, flags, dtype=torch.float64, neighbour=False):
    y = product_reference(x, W, flags, dtype, neighbour)
    if b is not None:
        y = y + b.to(dtype)
    return y * (scale or 1.0)


def linear_tolerance(flags):
    """The project's bounds (tests/test_gpu_gemm.py), of max|ref|."""
    bf16, f16, _, _ = _modes(flags)
    return 2e-5 if bf16 else (4e-6 if f16 else 2e-6)


def wgrad_inputs(M, n_out, n_in, accumulate, seed=0):
    G = torch.Generator().manual_seed(3000 + seed)
    dy, x = torch.randn(M, n_out, generator=G) * 0.1, torch.randn(M, n_in, generator=G)
    dW0 = torch.randn(n_out, n_in, generator=G) * 0.1 * M ** 0.5
    if not accumulate & BF16_PROJ:
        dy, x = _low_bits(dy), _low_bits(x)
    if accumulate & BF16_IN:
        dy = dy.bfloat16().float()
    return dy, x, dW0


def wgrad_reference(dy, x, dW0, accumulate, dtype=torch.float64, neighbour=False):
    r = product_reference(dy.t().contiguous(), x.t().contiguous(), accumulate & ~F16PAIR, dtype, neighbour)
    return r + dW0.to(dtype) if accumulate & 1 else r

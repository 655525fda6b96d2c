"""Test helper for the answer head (csrc/head.hip, csrc/ce.hip): run coattn_head_forward / coattn_head_forward_soft /
coattn_head_backward straight through the C-ABI (ctypes) with caller-chosen flags, targets, upstream gradients, accumulate,
input-gradient forms, per-operand misalignment and a reusable `saved`, every buffer between guard bands; and three oracles of
the same operation: float64 (oracle.coattn_oracle.OracleMLPClassifier + cross entropy / tests/_soft_loss.py), the same modules
in float32 on the CPU (the yardstick of the exact mode) and a float64 restatement of the reduced-precision mode.  Shared by
tests/test_gpu_head_paths.py and tests/test_head_cpu.py (which uses the CPU half only: nothing here needs a GPU to import)."""
import ctypes as C
import functools
import math

import torch

from oracle import coattn_oracle as O
from tests import _soft_loss as S

NAMES = ("W_w.weight", "W_w.bias", "W_p.weight", "W_p.bias", "W_s.weight", "W_s.bias", "W_h.weight", "W_h.bias")
PERSISTENT = 1          # include/coattn.h COATTN_HEAD_PERSISTENT: the one-launch form
BF16 = 4                # COATTN_FLAG_BF16_PROJ: the reduced-precision mode
SOFT_A = 4              # answer slots per sample of the soft-target cases
OUTPUTS = ("logits", "loss", "dv") + NAMES


# ---- cases (CPU, closed form) ---------------------------------------------------------------------------------------------
def make_params(d, mlp, K, seed):
    """The eight parameters at nn.Linear's default scale U(+-1/sqrt(fan_in)), in closed form (fp32, CPU)."""
    shapes = ((d, d), (d, 2 * d), (mlp, 2 * d), (K, mlp))
    P = {}
    for i, (n, k) in enumerate(shapes):
        bd = 1.0 / math.sqrt(k)
        P[NAMES[2 * i]] = torch.from_numpy(O.hash_unit((n, k), seed + 10 * i, bd)).float()
        P[NAMES[2 * i + 1]] = torch.from_numpy(O.hash_unit((n,), seed + 10 * i + 1, bd)).float()
    return P


@functools.lru_cache(maxsize=None)
def case(B, d, mlp, K, seed=0):
    """(P, v [3,B,d], q [3,B,d], labels int64 [B]) of one shape, fp32, computed once and shared (treat as read-only)."""
    P = make_params(d, mlp, K, 500 + seed)
    v = torch.from_numpy(O.hash_normal((3, B, d), 11 + seed, 1.0)).float()
    q = torch.from_numpy(O.hash_normal((3, B, d), 12 + seed, 0.5)).float()
    labels = torch.from_numpy((O.hash_uniform(B, 13 + seed) * K).astype("int64")).clamp_(0, K - 1)
    return P, v, q, labels


@functools.lru_cache(maxsize=None)
def soft_targets(B, K, seed=0):
    return S.make_targets(B, K, SOFT_A, 40 + seed)


@functools.lru_cache(maxsize=None)
def upstream(B, K, seed=0):
    """g_logits [B,K] fp32: hash-normal at the scale of d loss / d logits of a batch of B."""
    return torch.from_numpy(O.hash_normal((B, K), 77 + seed, 0.5 / B)).float()


def target_of(shape, target, seed=0):
    """What the loss is computed against: None, ("hard", labels) or (kind, ans_idx, ans_score) with kind "soft_ce" / "bce"."""
    B, d, mlp, K = shape
    if target is None:
        return None
    if target == "hard":
        return ("hard", case(B, d, mlp, K, seed)[3])
    return (target,) + soft_targets(B, K, seed)


# ---- oracles ----------------------------------------------------------------------------------------------------------------
def _loss(z, tgt):
    if tgt[0] == "hard":
        return torch.nn.functional.cross_entropy(z, tgt[1])
    return S.loss(z, tgt[1], tgt[2], tgt[0])


def oracle(P, v, q, tgt=None, g_loss=None, g_logits=None, dtype=torch.float64):
    """OracleMLPClassifier + loss + autograd in `dtype` on the CPU.  Returns {"logits", "loss", "dv" [3,B,d] (= d q too),
    NAMES...} as float64; the gradients are those of  g_loss * loss + sum(g_logits * logits)."""
    d, mlp, K = P[NAMES[0]].shape[0], P[NAMES[4]].shape[0], P[NAMES[6]].shape[0]
    ref = O.OracleMLPClassifier(d, mlp, K).to(dtype)
    ref.load_state_dict({k: t.to(dtype) for k, t in P.items()})
    vr, qr = v.detach().to(dtype).clone().requires_grad_(True), q.detach().to(dtype).clone().requires_grad_(True)
    z = ref([vr[l] for l in range(3)], [qr[l] for l in range(3)])
    res = {"logits": z.detach().double(), "loss": None}
    loss = None
    if tgt is not None:
        # (the soft oracles are float64 functions of the logits: in float32 mode the logits carry the rounding)
        loss = _loss(z, tgt) if (tgt[0] == "hard" or dtype == torch.float64) else _loss(z.double(), tgt).to(dtype)
        res["loss"] = loss.detach().double()
    if g_loss is None and g_logits is None:
        return res
    tot = 0
    if g_loss is not None:
        tot = g_loss * loss
    if g_logits is not None:
        tot = tot + (z * g_logits.to(dtype)).sum()
    tot.backward()
    assert torch.allclose(vr.grad, qr.grad, rtol=0, atol=0, equal_nan=True)
    res["dv"] = vr.grad.double()
    for k, p in ref.named_parameters():
        res[k] = p.grad.double()
    return res


@functools.lru_cache(maxsize=None)
def oracle_head(shape, target="hard", g_loss=1.7, with_g_logits=False, seed=0, dtype=torch.float64):
    """float64 oracle of one case, cached (treat as read-only)."""
    B, d, mlp, K = shape
    P, v, q, _ = case(B, d, mlp, K, seed)
    gx = upstream(B, K, seed) if with_g_logits else None
    return oracle(P, v, q, target_of(shape, target, seed), g_loss, gx, dtype)


def oracle_head_f32(shape, target="hard", g_loss=1.7, with_g_logits=False, seed=0):
    """The same modules evaluated in float32 on the CPU (cached)."""
    return oracle_head(shape, target, g_loss, with_g_logits, seed, torch.float32)


def rel(a, r):
    """The head tests' error measure: max|a - r| / max|r| of one tensor (r: float64 reference)."""
    a, r = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(r).double()
    return (a - r).abs().max().item() / max(r.abs().max().item(), 1e-30)


def errors(res, ora):
    """rel() of every output both sides hold"""
    return {k: rel(res[k], ora[k]) for k in OUTPUTS if res.get(k) is not None and ora.get(k) is not None}


@functools.lru_cache(maxsize=None)
def e32(shape, target="hard", g_loss=1.7, with_g_logits=False, seed=0):
    """The exact mode's yardstick: the worst rel() over the outputs of the float32 CPU evaluation against the float64 one --
    what the reference's own arithmetic is off by at this case."""
    args = (shape, target, g_loss, with_g_logits, seed)
    return max(errors(oracle_head_f32(*args), oracle_head(*args)).values())


def round_bf16(x):
    """float64 -> fp32 -> bf16 (both round to nearest even) -> float64: what v_cvt_pk_bf16_f32 does to a stored fp32 value"""
    return x.float().bfloat16().double()


def round_f32(x):
    return x.float().double()


def head_bf16_math(P, v, q, tgt=None, g_loss=None, g_logits=None, rounding=True):
    """What head.hip computes with COATTN_FLAG_BF16_PROJ, restated in float64 from the kernel: every MFMA operand is rounded
    to bf16 where the kernel rounds it -- the q_l + v_l sum formed in fp32, the hidden activations as stored in fp32, the
    weights, dY after p * scale + add (in the dW tiles without an added gradient the scale follows the product) -- the sums
    are exact, biases / tanh / tanh' / the loss / the bias gradients (column sums of the UNROUNDED dY) are not rounded beyond
    the fp32 stores between the layers.  rounding = False: no rounding anywhere (= the float64 oracle).
    Returns oracle()'s dict plus "h" (h_w, h_p, h_s) and "dz" (dY of the four backward layers, logits layer first)."""
    R = round_bf16 if rounding else (lambda x: x)
    st = round_f32 if rounding else (lambda x: x)         # a value stored as fp32 between two launches
    W = [P[NAMES[2 * i]].double() for i in range(4)]
    b = [P[NAMES[2 * i + 1]].double() for i in range(4)]
    x = [st(q[l].double() + v[l].double()) for l in range(3)]
    h_w = st(torch.tanh(R(x[0]) @ R(W[0]).T + b[0]))
    in_p = torch.cat([x[1], h_w], 1)
    h_p = st(torch.tanh(R(in_p) @ R(W[1]).T + b[1]))
    in_s = torch.cat([x[2], h_p], 1)
    h_s = st(torch.tanh(R(in_s) @ R(W[2]).T + b[2]))
    z = st(R(h_s) @ R(W[3]).T + b[3])
    res = {"logits": z, "loss": None, "h": (h_w, h_p, h_s)}
    dl = None
    if tgt is not None:
        zr = z.clone().requires_grad_(True)
        loss = _loss(zr, tgt)
        loss.backward()
        res["loss"], dl = loss.detach(), st(zr.grad)      # (ce.hip: fp32, stored in `saved`)
    if g_loss is None and g_logits is None:
        return res
    d = x[0].shape[1]
    if g_loss is not None:
        sc = float(torch.tensor(g_loss, dtype=torch.float32)) if rounding else g_loss
        dy = st(dl * sc + g_logits.double()) if g_logits is not None else None
        dy_x = dy if dy is not None else st(dl * sc)      # dX tiles: rounded after the scale
        dW_h = R(dy).T @ R(h_s) if dy is not None else sc * (R(dl).T @ R(h_s))
        db_h = dy.sum(0) if dy is not None else sc * dl.sum(0)
    else:
        dy_x = g_logits.double()
        dW_h, db_h = R(dy_x).T @ R(h_s), dy_x.sum(0)
    dz_s = st((R(dy_x) @ R(W[3])) * (1 - h_s * h_s))
    dx_s = R(dz_s) @ R(W[2])
    dz_p = st(dx_s[:, d:] * (1 - h_p * h_p))
    dx_p = R(dz_p) @ R(W[1])
    dz_w = st(dx_p[:, d:] * (1 - h_w * h_w))
    dx_w = R(dz_w) @ R(W[0])
    res["dz"] = (dy_x, dz_s, dz_p, dz_w)
    res["dv"] = torch.stack([dx_w, dx_p[:, :d], dx_s[:, :d]])
    grads = (R(dz_w).T @ R(x[0]), dz_w.sum(0), R(dz_p).T @ R(in_p), dz_p.sum(0), R(dz_s).T @ R(in_s), dz_s.sum(0), dW_h, db_h)
    res.update(dict(zip(NAMES, grads)))
    return res


@functools.lru_cache(maxsize=None)
def oracle_head_bf16(shape, target="hard", g_loss=1.7, with_g_logits=False, seed=0, rounding=True):
    """head_bf16_math of one case, cached (treat as read-only)."""
    B, d, mlp, K = shape
    P, v, q, _ = case(B, d, mlp, K, seed)
    gx = upstream(B, K, seed) if with_g_logits else None
    return head_bf16_math(P, v, q, target_of(shape, target, seed), g_loss, gx, rounding)


# ---- the C-ABI runner (GPU) -------------------------------------------------------------------------------------------------
GUARD = 64                         # words of guard band on either side (256 bytes: keeps the interior's alignment)
SENTINEL = 0x5A17C0DE              # as fp32: 1.07e+13, finite


class Guarded:
    """n fp32 words `off` floats into a larger allocation, sentinel words on both sides.  The interior starts as `init`
    or, without one, as 0xFF bytes (NaN)."""

    def __init__(self, n, dev, off=0, init=None):
        self.raw = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.t = self.raw[self.lo:self.hi].view(torch.float32)
        if init is None:
            self.raw[self.lo:self.hi] = -1
        else:
            self.t.copy_(init.reshape(-1))
        assert self.t.data_ptr() == self.raw.data_ptr() + 4 * self.lo

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.raw[:self.lo] == SENTINEL).all()) and bool((self.raw[self.hi:] == SENTINEL).all())


def workspace_bytes(B, d, mlp, K):
    from vqa_amd import _lib
    sb, wb = C.c_size_t(), C.c_size_t()
    _lib.check(_lib.load().coattn_head_workspace_bytes(B, d, mlp, K, _lib.F32, C.byref(sb), C.byref(wb)), "coattn_head_workspace_bytes")
    return sb.value, wb.value


def new_saved(shape, off=0):
    """A `saved` buffer (0xFF bytes between guard bands) to hand to several run_head calls"""
    return Guarded(workspace_bytes(*shape)[0] // 4, torch.device("cuda:0"), off)


def head_status(saved, shape):
    """(rc, message) of coattn_head_status on a Guarded `saved`"""
    from vqa_amd import _lib
    lib = _lib.load()
    rc = lib.coattn_head_status(saved.ptr(), *shape, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, (lib.coattn_last_error().decode() if rc else "")


def run_head(P, v, q, tgt=None, g_loss=None, g_logits=None, flags=0, accumulate=0, grads_init=None, want_dv=True, dq=None,
             offsets=None, saved=None):
    """One forward and, with g_loss / g_logits, one backward.
    tgt: None (logits only), ("hard", labels) or (kind, ans_idx, ans_score);  dq: None (dq = NULL) or three of "separate" /
    "alias" (dq[l] is dv[l]);  offsets: {operand: floats} for "v0".."v2", "q0".."q2", "W_w", "W_p", "W_s", "W_h", "saved", "ws",
    "g_logits", "logits" -- the operand starts that many floats into its allocation;  saved: a Guarded from new_saved() to
    reuse (else a fresh one);  grads_init: {name: tensor}, what the eight gradient buffers hold before the call.
    Returns {"logits", "loss", "dv" [3 tensors] / None, "dq" [3] / None, NAMES..., "saved", "ws" (Guarded), "intact":
    {buffer: bool}} -- intact[k] says the guard bands of buffer k still hold the sentinel."""
    from vqa_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    off = dict(offsets or {})
    _, B, d = v.shape
    mlp, K = P[NAMES[4]].shape[0], P[NAMES[6]].shape[0]
    shape = (B, d, mlp, K)
    vs = [Guarded(B * d, dev, off.pop("v%d" % l, 0), v[l].float()) for l in range(3)]
    qs = [Guarded(B * d, dev, off.pop("q%d" % l, 0), q[l].float()) for l in range(3)]
    ps = [Guarded(P[k].numel(), dev, off.pop(k[:3], 0) if k.endswith("weight") else 0, P[k].float()) for k in NAMES]
    sb, wb = workspace_bytes(*shape)
    if saved is None:
        saved = Guarded(sb // 4, dev, off.pop("saved", 0))
    logits = Guarded(B * K, dev, off.pop("logits", 0))
    loss = Guarded(1, dev) if tgt is not None else None
    guarded = {"logits": logits, "saved": saved}
    if loss is not None:
        guarded["loss"] = loss
    arr = lambda gs: (C.c_void_p * 3)(*[g.ptr() if g is not None else None for g in gs])   # noqa: E731
    p = _lib.HeadParams(*[g.ptr() for g in ps])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if tgt is None or tgt[0] == "hard":
        lab = tgt[1].to(dev) if tgt is not None else None
        _lib.check(lib.coattn_head_forward(arr(vs), arr(qs), C.byref(p), lab.data_ptr() if lab is not None else None, logits.ptr(),
                                           loss.ptr() if loss is not None else None, saved.ptr(), B, d, mlp, K, _lib.F32, flags, stream),
                   "coattn_head_forward")
    else:
        idx, sc = tgt[1].to(dev).contiguous(), tgt[2].to(dev).contiguous()
        _lib.check(lib.coattn_head_forward_soft(arr(vs), arr(qs), C.byref(p), idx.data_ptr(), sc.data_ptr(), idx.shape[1],
                                                S.KINDS[tgt[0]], logits.ptr(), loss.ptr(), saved.ptr(), B, d, mlp, K, _lib.F32, flags,
                                                stream), "coattn_head_forward_soft")
    torch.cuda.synchronize()
    res = {"logits": logits.t.view(B, K), "loss": loss.t[0] if loss is not None else None, "dv": None, "dq": None, "saved": saved,
           "ws": None}
    if g_loss is not None or g_logits is not None:
        ws = Guarded(wb // 4, dev, off.pop("ws", 0))
        dvs = [Guarded(B * d, dev) for _ in range(3)] if want_dv else None
        dqs = None
        if dq is not None:
            assert want_dv
            dqs = [dvs[l] if m == "alias" else Guarded(B * d, dev) for l, m in enumerate(dq)]
        grads = [Guarded(P[k].numel(), dev, 0, grads_init[k].float() if grads_init else None) for k in NAMES]
        pg = _lib.HeadParamGrads(*[g.ptr() for g in grads])
        gl = torch.tensor([g_loss], device=dev, dtype=torch.float32) if g_loss is not None else None
        gx = Guarded(B * K, dev, off.pop("g_logits", 0), g_logits.float()) if g_logits is not None else None
        _lib.check(lib.coattn_head_backward(arr(vs), arr(qs), C.byref(p), saved.ptr(), gl.data_ptr() if gl is not None else None,
                                            gx.ptr() if gx is not None else None, arr(dvs) if want_dv else None,
                                            arr(dqs) if dqs is not None else None, C.byref(pg), accumulate, ws.ptr(), B, d, mlp, K,
                                            _lib.F32, flags, stream), "coattn_head_backward")
        torch.cuda.synchronize()
        res["ws"] = ws
        guarded["ws"] = ws
        if want_dv:
            res["dv"] = [g.t.view(B, d) for g in dvs]
            guarded.update({"dv%d" % l: g for l, g in enumerate(dvs)})
        if dqs is not None:
            res["dq"] = [g.t.view(B, d) for g in dqs]
            guarded.update({"dq%d" % l: g for l, g in enumerate(dqs)})
        for k, g in zip(NAMES, grads):
            res[k] = g.t.view(P[k].shape)
            guarded["d" + k] = g
        if gx is not None:
            guarded["g_logits"] = gx
    for i, g in enumerate(vs + qs + ps):              # (inputs: nothing may be stored near them either)
        guarded["in%d" % i] = g
    assert not off, "unknown operand offsets: %s" % sorted(off)
    res["intact"] = {k: g.intact() for k, g in guarded.items()}
    return res

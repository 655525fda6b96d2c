"""The fusion head's C-ABI (coattn_fusion_forward / coattn_fusion_backward; csrc/fusion.hip, include/coattn_fusion.h) for the
tests: a runner over ``_lib.bind`` that puts every device buffer of a call at its exact size inside a marker-filled arena with
the outputs pre-filled with NaN and checks the margins after every call, and the oracle -- the header's formulas in torch on
the CPU, in float64 (the reference) or float32 (the yardstick of the error bound), the dropout mask taken from
``tests/_dropout.keep`` -- never the code under test."""
import functools

import numpy as np
import torch

from vqa_amd import _lib

from tests import _dropout as D
from tests._general import Arena
from tests._lstm import bound_check, same_bits  # noqa: F401  (re-exported for the test files)

PARAMS = _lib.FUSION_PARAM_NAMES                       # W_i b_i W_q b_q W_m b_m W_f b_f
GRADS = tuple("d" + n for n in PARAMS)
OUTPUTS = ("logits", "dh") + GRADS
SEED = 0x1234_5678_9ABC_DEF1
STEP0 = 6                                              # the state's step in front of a forward: the forward draws mask STEP0 + 1
BASELINE = (160, 4096, 1024, 1024, 1000, 1001)
SMALL = [(1, 4, 4, 4, 4, 2), (3, 36, 32, 40, 28, 5), (33, 260, 96, 64, 100, 8), (40, 512, 288, 1024, 1000, 11)]


def _shapes(Di, H, J, Mh, K):
    return dict(W_i=(J, Di), b_i=(J,), W_q=(J, H), b_q=(J,), W_m=(Mh, J), b_m=(Mh,), W_f=(K, Mh), b_f=(K,))


@functools.lru_cache(None)
def make_case(B, Di, H, J, Mh, K, seed=0):
    """Inputs on the host (float32, shared and never written): features of fc7's kind (non-negative), a hidden state in
    (-1, 1), nn.Linear's default U(-1/sqrt(fan_in), 1/sqrt(fan_in)) parameters, the incoming gradient."""
    g = torch.Generator().manual_seed(2600 + seed + B + K)
    u = lambda s, k: (torch.rand(*s, generator=g) * 2 - 1) * k          # noqa: E731
    c = dict(B=B, Di=Di, H=H, J=J, Mh=Mh, K=K, f=torch.randn(B, Di, generator=g).clamp_min(0) * 2, h=u((B, H), 1.0),
             g=torch.randn(B, K, generator=g))
    for n, s in _shapes(Di, H, J, Mh, K).items():
        c[n] = u(s, (s[-1] if n.startswith("W") else c["W" + n[1:]].shape[1]) ** -0.5)
    return c


def dims(c):
    return {k: c[k] for k in ("B", "Di", "H", "J", "Mh", "K")}


def mask(c, p, step, seed=SEED):
    """[B, Mh] float64 multiplier of the header: scale where `tests/_dropout.keep` keeps element b Mh + n, 0 where not; None at
    p = 0."""
    if p == 0:
        return None
    n = c["B"] * c["Mh"]
    return torch.from_numpy(np.where(D.keep(n, seed, step, p), np.float64(D.scale(p)), 0.0)).view(c["B"], c["Mh"])


def formulas(f, h, P, mult):
    """The header's forward, operation by operation, in the dtype of its inputs: (logits, m).  `mult`: the mask's multiplier
    or None."""
    ss = (f * f).sum(1, keepdim=True)
    inv = 1.0 / ss.sqrt().clamp_min(1e-12)
    e_i = torch.tanh(inv * (f @ P["W_i"].T) + P["b_i"])
    e_q = torch.tanh(h @ P["W_q"].T + P["b_q"])
    pre = (e_i * e_q) @ P["W_m"].T + P["b_m"]
    m = torch.tanh(pre if mult is None else pre * mult.to(pre.dtype))
    return m @ P["W_f"].T + P["b_f"], m


def oracle(c, dtype=torch.float64, p=0.0, step=STEP0 + 1, f=None, h=None, g=None, seed=SEED):
    """logits, m, dh and the eight parameter gradients of sum(logits * g) by the header's formulas with autograd, on the CPU."""
    P = {n: c[n].to(dtype, copy=True).requires_grad_(True) for n in PARAMS}
    hh = (c["h"] if h is None else h).to(dtype, copy=True).requires_grad_(True)
    ff = (c["f"] if f is None else f).to(dtype, copy=True)
    logits, m = formulas(ff, hh, P, mask(c, p, step, seed))
    (logits * (c["g"] if g is None else g).to(dtype)).sum().backward()
    out = dict(logits=logits.detach(), m=m.detach(), dh=hh.grad)
    out.update({"d" + n: P[n].grad for n in PARAMS})
    return out


@functools.lru_cache(None)
def references(shape, p):
    """(float64 oracle, float32 oracle) of make_case(*shape) at dropout p, computed once and shared."""
    c = make_case(*shape)
    return oracle(c, torch.float64, p), oracle(c, torch.float32, p)


def _put(t, ld=None):
    """An arena holding `t` at its exact size; ld: rows `ld` floats apart, the padding NaN, the arena ending with the last row."""
    if ld is None:
        a = Arena(t.numel(), fill=None)
        a.body.copy_(t.reshape(-1))
        return a
    rows, cols = t.shape
    a = Arena((rows - 1) * ld + cols)
    torch.as_strided(a.body, (rows, cols), (ld, 1)).copy_(t)
    return a


class State:
    """The 32-byte dropout state in an arena of its own."""

    def __init__(self, seed=SEED, step=STEP0):
        self.arena = Arena(8, fill=None)
        self.arena.body.view(torch.int32).copy_(D.state_words(seed, step))

    def words(self):
        return self.arena.body.view(torch.int32).cpu()

    def step(self):
        w = self.words().to(torch.int64) & 0xFFFFFFFF
        return int(w[2]) | (int(w[3]) << 32)


def run(c, p=0.0, state=None, saved=True, backward=True, dh=True, accumulate=0, prefill=None, ld_f=None, ld_h=None, f=None,
        h=None, g=None, flags=0, shift=None, backwards=1, expect_rc=0, expect_rc_bwd=None):
    """One coattn_fusion_forward (+ `backwards` coattn_fusion_backward calls, each into fresh NaN-filled buffers) on case `c`
    through _lib.bind.  Every buffer is an arena of its exact size; the outputs start as NaN (the parameter gradients as
    `prefill` [name] with accumulate = 1); the margins of every arena are checked after the calls.  `shift`: the name of ONE
    operand handed over 4 bytes behind its start (the call that takes it is expected to be refused: `expect_rc`, and
    `expect_rc_bwd` for the backward where it differs).  Returns the outputs on the host
    ("bwd": the list of the backwards' outputs when there are several), "m" out of `saved`, "rc", and "state"."""
    d = dims(c)
    B, H, J, Mh, K = d["B"], d["H"], d["J"], d["Mh"], d["K"]
    sb, bb = _lib.fusion_workspace_bytes(*d.values())
    dev = torch.device("cuda:0")
    ar = {"f": _put(c["f"] if f is None else f, ld_f), "h": _put(c["h"] if h is None else h, ld_h),
          "g": _put(c["g"] if g is None else g)}
    for n in PARAMS:
        ar[n] = _put(c[n])
    ar["logits"], ar["saved"] = Arena(B * K), Arena(sb // 4)
    if p > 0 and state is None:
        state = State()
    if state is not None:
        ar["state"] = state.arena
    stream = torch.cuda.current_stream(dev).cuda_stream

    def P(k, on=True):
        if not on:
            return None
        return ar[k].body.data_ptr() + (4 if shift == k else 0)

    def params(names, pre=""):
        return [P(pre + n) for n in names]

    common = dict(f=P("f"), ld_f=ld_f or d["Di"], h=P("h"), ld_h=ld_h or H, p_drop=p, drop_state=P("state", state is not None),
                  dtype=_lib.F32, flags=flags, stream=stream, **d)
    rc_f = _lib.bind("coattn_fusion_forward", p=_lib.FusionParams(*params(PARAMS)), logits=P("logits"), saved=P("saved", saved),
                     **common).code()
    outs, rc_b = [], None
    for i in range(backwards if backward and saved and rc_f == 0 else 0):
        tag = "#%d" % i
        ar["dh" + tag], ar["ws" + tag] = Arena(B * H), Arena(bb // 4)
        for n in PARAMS:
            ar["d" + n + tag] = Arena(c[n].numel())
            if prefill is not None:
                ar["d" + n + tag].body.copy_(prefill["d" + n].reshape(-1))
        shifted = lambda k: (4 if shift == k else 0)                     # noqa: E731
        pg = _lib.FusionParamGrads(*[ar["d" + n + tag].body.data_ptr() + shifted("d" + n) for n in PARAMS])
        rc_b = _lib.bind("coattn_fusion_backward", p=_lib.FusionParams(*params(PARAMS)), saved=P("saved"), g_logits=P("g"),
                         dh=(ar["dh" + tag].body.data_ptr() + shifted("dh")) if dh else None, pg=pg, accumulate=accumulate,
                         ws=ar["ws" + tag].body.data_ptr() + shifted("ws"), **common).code()
        torch.cuda.synchronize()
        o = dict(dh=ar["dh" + tag].body.cpu().view(B, H))
        o.update({"d" + n: ar["d" + n + tag].body.cpu().view(c[n].shape) for n in PARAMS})
        outs.append(o)
    torch.cuda.synchronize()
    err = _lib.load().coattn_last_error().decode()
    assert rc_f == expect_rc, (rc_f, err)
    assert rc_b in (None, expect_rc if expect_rc_bwd is None else expect_rc_bwd), (rc_b, err)
    for k, a in ar.items():
        a.check("fusion %s" % k)
    res = dict(rc=(rc_f, rc_b), logits=ar["logits"].body.cpu().view(B, K), state=state, err=err)
    if saved:
        sv = ar["saved"].body.cpu()
        al = lambda n: (n + 63) & ~63                                    # noqa: E731  (the header's layout: inv, e_i, e_q, m)
        off = al(B) + 2 * al(B * J)
        res["m"] = sv[off:off + B * Mh].view(B, Mh)
        res["saved_raw"] = sv
    if outs:
        res.update(outs[0])
        res["bwd"] = outs
    return res

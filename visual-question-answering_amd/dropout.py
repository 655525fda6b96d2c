"""Feature dropout on MI355X: the paper's dropout on every ``q_l + v_l`` in front of the answer head (Lu et al. 2016), as one
HIP launch per direction (``csrc/dropout.hip``, include/coattn.h v0.19.0).  The mask is a pure function of (element, step,
seed) through Philox4x32-10: nothing is stored, the backward regenerates it, and the step counter lives on the device, so the
calls are capture-safe and consume nothing from torch's generators.  DESIGN.md section 3.15.

    state = DropoutState(seed=1234, device="cuda")
    y = dropout(x, 0.5, state)                                  # fp32 contiguous CUDA, out of place, autograd-aware
    v, q = feature_dropout(v, q, 0.5, state)                    # one shared mask over [3, B, d], same structure back

One state serves ONE dropout site per step: the backward multiplies by the mask most recently drawn from its state, so it must
run before the next forward on the same state (a later forward in between raises in the backward).  There is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib

_U64 = (1 << 64) - 1


def rank_seed(seed: int, rank: int) -> int:
    """The seed data-parallel rank `rank` draws its masks from: seed + rank (ranks see different samples and must not share
    a mask)."""
    return int(seed) + int(rank)


def check_p(p) -> float:
    p = float(p)
    if not 0.0 <= p < 1.0:                                       # (NaN fails both comparisons)
        raise ValueError("dropout probability must be in [0, 1), got %r" % (p,))
    return p


def _signed(u: int) -> int:
    u &= _U64
    return u - (1 << 64) if u >> 63 else u


class DropoutState:
    """The 32-byte state of include/coattn.h's dropout calls: u64 seed, u64 step (the index of the mask most recently drawn),
    16 bytes the library keeps at zero between calls.  Lives on `device`; written in stream order, never read by a step."""

    def __init__(self, seed: int = 0, device=None):
        self.device = torch.device("cuda" if device is None else device)
        self.buf = torch.zeros(4, dtype=torch.int64, device=self.device)
        self.draws = 0                                           # advancing forwards issued from Python (a host-side tag for the
        self.reseed(seed)                                        # backward's "still my mask?" check; the kernels never see it)

    def reseed(self, seed: int, step: int = 0) -> None:
        """Start over from (seed, step): the next advancing forward draws mask step + 1.  Asynchronous, in stream order."""
        self.seed = int(seed) & _U64
        self.buf.copy_(torch.tensor([_signed(self.seed), _signed(step), 0, 0], dtype=torch.int64))
        self.draws += 1                                          # (a backward of an earlier forward no longer has its mask)

    def step(self) -> int:
        """The index of the mask most recently drawn.  A HOST READ (synchronises): for tests and logging, not for the step."""
        return int(self.buf[1].item()) & _U64

    def data_ptr(self) -> int:
        return self.buf.data_ptr()


def _check(x, p, state, what):
    if not isinstance(state, DropoutState):
        raise TypeError("%s: state must be a DropoutState, got %s" % (what, type(state).__name__))
    if not x.is_cuda:
        raise RuntimeError("%s (HIP) needs tensors on the GPU: there is no CPU fallback" % what)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise RuntimeError("%s (HIP) takes contiguous fp32 tensors; got %s, contiguous=%s" % (what, x.dtype, x.is_contiguous()))
    if state.device != x.device:
        raise RuntimeError("%s: the DropoutState lives on %s, the tensor on %s" % (what, state.device, x.device))
    if not _lib.load().coattn_dropout_supported(x.numel()):
        raise RuntimeError("%s: %d elements not supported (1 .. 2^31 - 4)" % (what, x.numel()))


def _backward(g, p, state, draw, what):
    if draw != state.draws:
        raise RuntimeError("%s: the state has drawn another mask (or was re-seeded) since this forward; its backward must run "
                           "before the next forward on the same DropoutState" % what)
    g = g.contiguous().float()
    dx = torch.empty_like(g)
    with _lib.on_device(g.device):
        _lib.bind("coattn_dropout_backward", g=g, dx=dx, n=g.numel(), p=p, state=state.buf, stream=_lib.stream_ptr(g.device))()
    return dx


class _DropoutFn(torch.autograd.Function):
    """forward -> coattn_dropout_forward (advance = 1), backward -> coattn_dropout_backward on the same state."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, x1, p, state):
        xs = (x,) if x1 is None else (x, x1)
        for t in xs:
            _check(t, p, state, "dropout")
        if x1 is not None and x1.shape != x.shape:
            raise RuntimeError("dropout: the two tensors of a shared mask must have one shape")
        ys = tuple(torch.empty_like(t) for t in xs)
        pair1 = dict(x1=x1, y1=ys[1]) if x1 is not None else {}
        with _lib.on_device(x.device):
            _lib.bind("coattn_dropout_forward", x0=x, y0=ys[0], n=x.numel(), p=p, state=state.buf, advance=1,
                      stream=_lib.stream_ptr(x.device), **pair1)()
        state.draws += 1
        ctx.p, ctx.state, ctx.draw = p, state, state.draws
        ctx.set_materialize_grads(False)
        return ys if x1 is not None else ys[0]

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gs):
        out = [None if g is None else _backward(g, ctx.p, ctx.state, ctx.draw, "dropout") for g in gs]
        return (out[0], out[1] if len(out) > 1 else None, None, None)


def dropout(x, p, state, training: bool = True):
    """x (fp32, contiguous, CUDA) -> x * mask / (1 - p) out of place, the mask drawn from `state` (which advances by one);
    ``training=False`` or p = 0: x itself, the state untouched.  A CPU tensor with p > 0 in training raises."""
    p = check_p(p)
    if not training or p == 0.0:
        return x
    return _DropoutFn.apply(x, None, p, state)


def feature_dropout(v, q, p, state, training: bool = True):
    """The six attended features as the co-attention returns them -- two lists of three [B, d] tensors, or two [3, B, d] tensors
    -- under ONE mask shared by v and q, over the layout i = (l B + b) d + c (graph.HotPathGraph's static buffers: both routes
    draw the same bits).  Returns the same structure."""
    p = check_p(p)
    if not training or p == 0.0:
        return v, q
    as_list = not torch.is_tensor(v)
    if as_list != (not torch.is_tensor(q)):
        raise TypeError("feature_dropout: v and q must both be lists or both be tensors")
    vs, qs = (torch.stack(list(v)), torch.stack(list(q))) if as_list else (v, q)
    yv, yq = _DropoutFn.apply(vs.contiguous(), qs.contiguous(), p, state)
    return (list(yv.unbind(0)), list(yq.unbind(0))) if as_list else (yv, yq)

"""``fusion_head``: what the baseline model computes behind its two encoders (reference model.py VQABaselineNet: F.normalize ->
Linear -> Tanh on the image features, Linear -> Tanh on the GRU's last state, the elementwise product, Linear -> Dropout ->
Tanh, Linear) on MI355X -- four HIP launches forward, three backward (``csrc/fusion.hip``), the row norm as a scale in the
epilogue of the 4096-wide product, the dropout mask a Philox function of (element, step, seed) drawn in the epilogue in front
of the tanh and regenerated in the backward -- through the C-ABI of ``include/coattn_fusion.h`` on the caller's current stream.
Nothing is consumed from torch's generators.  DESIGN.md section 3.21.
"""
from __future__ import annotations

import torch

from . import _lib
from .dropout import DropoutState, check_p


def supported(B, Di, H, J, Mh, K) -> bool:
    """Does the HIP path take this shape (include/coattn_fusion.h coattn_fusion_supported)?  No GPU call."""
    return bool(_lib.bind("coattn_fusion_supported", B=B, Di=Di, H=H, J=J, Mh=Mh, K=K, dtype=_lib.F32).code())


def _dims(f, h, ps):
    (B, Di), H = f.shape, h.shape[1]
    J, Mh, K = ps[0].shape[0], ps[4].shape[0], ps[6].shape[0]
    want = ((J, Di), (J,), (J, H), (J,), (Mh, J), (Mh,), (K, Mh), (K,))
    if h.shape[0] != B or any(tuple(t.shape) != w for t, w in zip(ps, want)):
        raise RuntimeError("fusion_head: parameters must be [J,Di], [J], [J,H], [J], [Mh,J], [Mh], [K,Mh], [K] for f [B,Di] and "
                           "h [B,H]; got f %s, h %s, %s" % (tuple(f.shape), tuple(h.shape), [tuple(t.shape) for t in ps]))
    return dict(B=B, Di=Di, H=H, J=J, Mh=Mh, K=K)


def _rows(t):
    """A 2-D operand the kernels take as it is: unit stride along the row, rows a multiple of 4 floats apart; a copy otherwise."""
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 else t.contiguous()


class _FusionHeadFn(torch.autograd.Function):
    """forward -> coattn_fusion_forward, backward -> coattn_fusion_backward (once differentiable: the backward is a kernel call,
    not autograd operations).  The saved activations are written only when an input needs a gradient (the inference form of the
    call otherwise); the backward computes the eight parameter gradients together and returns those that are asked for, and
    skips the dh product when h needs none.  `f` is not differentiable: the image encoder in front of the head is frozen."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)     # fp32 island under autocast
    def forward(ctx, f, h, p, state, *ps):
        if not (f.is_cuda and h.is_cuda):
            raise RuntimeError("fusion_head (HIP) needs tensors on the GPU: there is no CPU fallback")
        if f.dtype != torch.float32 or h.dtype != torch.float32:
            raise RuntimeError("fusion_head (HIP) computes in fp32; got f %s, h %s" % (f.dtype, h.dtype))
        ps = [t.contiguous() for t in ps]
        d = _dims(f, h, ps)
        if not supported(**d):
            raise RuntimeError("fusion_head (HIP): shape %s not supported (include/coattn_fusion.h)" % (d,))
        f, h = _rows(f.detach()), _rows(h)
        need_grad = any(ctx.needs_input_grad)
        sb, _ = _lib.fusion_workspace_bytes(*d.values())
        logits = torch.empty((d["B"], d["K"]), dtype=torch.float32, device=f.device)
        saved = torch.empty(sb, dtype=torch.uint8, device=f.device) if need_grad or p > 0 else None   # (a mask is drawn by the saving form only)
        with _lib.on_device(f.device):
            _lib.bind("coattn_fusion_forward", f=f, ld_f=f.stride(0), h=h, ld_h=h.stride(0),
                      p=_lib.FusionParams(*[t.data_ptr() for t in ps]), logits=logits, saved=saved, p_drop=p,
                      drop_state=state.buf if p > 0 else None, dtype=_lib.F32, flags=0, stream=_lib.stream_ptr(f.device), **d)()
        if p > 0:
            state.draws += 1
        if need_grad:
            ctx.save_for_backward(f, h, saved, *ps)
            ctx.p, ctx.state, ctx.d, ctx.draw = p, state, d, state.draws if p > 0 else None
        return logits

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        f, h, saved, *ps = ctx.saved_tensors
        p, state, d = ctx.p, ctx.state, ctx.d
        if p > 0 and ctx.draw != state.draws:
            raise RuntimeError("fusion_head: the state has drawn another mask (or was re-seeded) since this forward; its backward "
                               "must run before the next forward on the same DropoutState")
        g = g.contiguous().float()
        _, bb = _lib.fusion_workspace_bytes(*d.values())
        ws = torch.empty(bb, dtype=torch.uint8, device=f.device)
        dh = torch.empty((d["B"], d["H"]), dtype=torch.float32, device=f.device) if ctx.needs_input_grad[1] else None
        grads = [torch.empty_like(t) for t in ps]
        with _lib.on_device(f.device):
            _lib.bind("coattn_fusion_backward", f=f, ld_f=f.stride(0), h=h, ld_h=h.stride(0),
                      p=_lib.FusionParams(*[t.data_ptr() for t in ps]), saved=saved, g_logits=g, dh=dh,
                      pg=_lib.FusionParamGrads(*[t.data_ptr() for t in grads]), accumulate=0, p_drop=p,
                      drop_state=state.buf if p > 0 else None, ws=ws, dtype=_lib.F32, flags=0,
                      stream=_lib.stream_ptr(f.device), **d)()
        return (None, dh, None, None, *[gr if need else None for gr, need in zip(grads, ctx.needs_input_grad[4:])])


def fusion_head(f, h, W_i, b_i, W_q, b_q, W_m, b_m, W_f, b_f, p=0.0, state=None, training=True):
    """f [B,Di] (the image encoder's features, fp32 CUDA; rows may be padded), h [B,H] (the question GRU's last hidden state) ->
    logits [B,K] = Linear_f(tanh(dropout_p(Linear_m(tanh(Linear_i(f / max(||f||, 1e-12))) * tanh(Linear_q(h)))))), with the
    nn.Linear parameters W_i [J,Di], W_q [J,H], W_m [Mh,J], W_f [K,Mh] and their biases.  `p`, `state`: the dropout in front
    of the last tanh, its masks drawn from a ``DropoutState`` (which advances by one per training forward); ``training=False``
    or p = 0: no dropout, the state untouched.  `f` gets no gradient (the encoder in front is frozen): an `f` that requires
    one raises."""
    p = check_p(p)
    if f.requires_grad:
        raise RuntimeError("fusion_head: f requires a gradient, and the HIP fusion head has none for the image features (a "
                           "trainable image encoder is out of scope: use the stock route)")
    if not training:
        p = 0.0
    if p > 0 and not isinstance(state, DropoutState):
        raise TypeError("fusion_head: p > 0 needs a DropoutState, got %s" % type(state).__name__)
    if p > 0 and state.device != f.device:
        raise RuntimeError("fusion_head: the DropoutState lives on %s, the tensors on %s" % (state.device, f.device))
    return _FusionHeadFn.apply(f, h, p, state, W_i, b_i, W_q, b_q, W_m, b_m, W_f, b_f)

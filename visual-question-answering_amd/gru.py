"""``question_gru``: the recurrent part of the baseline model's question encoder (reference model.py QuestionBaselineEncoder:
pack_padded_sequence -> nn.GRU -> the hidden state after each question's last token) on MI355X without packing -- one
exact-fp32 projection of all B T rows, then one HIP launch per time step in each direction with the gate arithmetic in the
epilogue (``csrc/gru.hip``), the per-question lengths read on the device, in any order -- through the C-ABI of
``include/coattn_rnn.h`` on the caller's current stream.  DESIGN.md section 3.20.
"""
from __future__ import annotations

import torch

from . import _lib
from .lstm import device_lengths


def supported(B, T, E, H) -> bool:
    """Does the HIP path take this shape (include/coattn_rnn.h coattn_gru_supported)?  No GPU call."""
    return bool(_lib.bind("coattn_gru_supported", B=B, T=T, E=E, H=H, dtype=_lib.F32).code())


def _forward_call(X, lens, p, seq, h_last, saved, ws, stream):
    (B, T, E), H = X.shape, seq.shape[2]
    return _lib.bind("coattn_gru_forward", X=X, len=lens, p=p, seq_out=seq, h_last=h_last, saved=saved, ws=ws, B=B, T=T, E=E,
                     H=H, dtype=_lib.F32, flags=0, stream=stream)


def _backward_call(X, lens, p, saved, g_seq, g_last, dX, pg, ws, H, stream):
    B, T, E = X.shape
    return _lib.bind("coattn_gru_backward", X=X, len=lens, p=p, saved=saved, g_seq=g_seq, g_last=g_last, dX=dX, pg=pg,
                     accumulate=0, ws=ws, B=B, T=T, E=E, H=H, dtype=_lib.F32, flags=0, stream=stream)


class _QuestionGruFn(torch.autograd.Function):
    """forward -> coattn_gru_forward, backward -> coattn_gru_backward (once differentiable: the backward is a kernel call,
    not autograd operations).  The state for the backward is written only when an input needs a gradient; the backward
    skips the dX product when x needs none, and computes the four parameter gradients together (one call of the C-ABI),
    returning those that are asked for.  A gradient that did not arrive (only `seq` or only `h_last` was used) goes in as
    NULL, not as a tensor of zeros."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)     # fp32 island under autocast
    def forward(ctx, x, lens, w_ih, w_hh, b_ih, b_hh):
        if not x.is_cuda:
            raise RuntimeError("question_gru (HIP) needs tensors on the GPU")
        if x.dtype != torch.float32:
            raise RuntimeError("question_gru (HIP) computes in fp32; got %s" % x.dtype)
        B, T, E = x.shape
        H = w_hh.shape[1]
        if tuple(w_ih.shape) != (3 * H, E) or tuple(w_hh.shape) != (3 * H, H) or tuple(b_ih.shape) != (3 * H,) \
                or tuple(b_hh.shape) != (3 * H,):
            raise RuntimeError("GRU parameters must be [3H,E], [3H,H], [3H], [3H] with E = %d, H = %d" % (E, H))
        X = x.contiguous()
        ps = [t.contiguous() for t in (w_ih, w_hh, b_ih, b_hh)]
        need_grad = any(ctx.needs_input_grad)
        sb, fb, _ = _lib.gru_workspace_bytes(B, T, E, H)
        seq = torch.empty((B, T, H), dtype=torch.float32, device=x.device)
        h_last = torch.empty((B, H), dtype=torch.float32, device=x.device)
        saved = torch.empty(sb, dtype=torch.uint8, device=x.device) if need_grad else None
        ws = torch.empty(fb, dtype=torch.uint8, device=x.device)
        p = _lib.GruParams(*[t.data_ptr() for t in ps])
        with _lib.on_device(x.device):
            _forward_call(X, lens, p, seq, h_last, saved, ws, _lib.stream_ptr(x.device))()
        if need_grad:
            ctx.save_for_backward(X, lens, saved, *ps)
        ctx.set_materialize_grads(False)                             # an unused output's gradient stays None: NULL in the call
        return seq, h_last

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_seq, g_last):
        X, lens, saved, *ps = ctx.saved_tensors
        B, T, E = X.shape
        H = ps[1].shape[1]
        if g_seq is None and g_last is None:
            return (None,) * 6
        g_seq = None if g_seq is None else g_seq.contiguous().float()
        g_last = None if g_last is None else g_last.contiguous().float()
        _, _, bb = _lib.gru_workspace_bytes(B, T, E, H)
        ws = torch.empty(bb, dtype=torch.uint8, device=X.device)
        dX = torch.empty_like(X) if ctx.needs_input_grad[0] else None
        grads = [torch.empty_like(t) for t in ps]
        p = _lib.GruParams(*[t.data_ptr() for t in ps])
        pg = _lib.GruParamGrads(*[t.data_ptr() for t in grads])
        with _lib.on_device(X.device):
            _backward_call(X, lens, p, saved, g_seq, g_last, dX, pg, ws, H, _lib.stream_ptr(X.device))()
        return (dX, None, *[g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:])])


def question_gru(x, lens, w_ih, w_hh, b_ih, b_hh):
    """x [B,T,E] (fp32, CUDA), lens [B] -> (seq [B,T,H], h_last [B,H]): the one-layer GRU with nn.GRU's parameters
    (weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0) over each question's first len_b steps from a zero state -- `seq`
    with exact zeros beyond, as pack_padded_sequence -> nn.GRU -> pad_packed_sequence return it, and `h_last` the state
    after step len_b - 1, the hidden state nn.GRU returns for a packed batch.  `lens`: any integer tensor or list, in any
    order; values outside [1, T] are clamped on the device.  No host read, no sorting."""
    return _QuestionGruFn.apply(x, device_lengths(lens, x.device), w_ih, w_hh, b_ih, b_hh)

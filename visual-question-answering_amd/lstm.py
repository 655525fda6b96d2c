"""``sentence_lstm``: the sentence level of the question hierarchy (reference model.py:286-296:
pack_padded_sequence -> nn.LSTM -> pad_packed_sequence) on MI355X without packing -- one exact-fp32
projection of all B T rows, then one HIP launch per time step in each direction with the gate
arithmetic in the epilogue (``csrc/lstm.hip``), the per-question lengths read on the device -- through
the C-ABI of ``include/coattn.h`` on the caller's current stream.  DESIGN.md section 3.13.
"""
from __future__ import annotations

import torch

from . import _lib


def supported(B, T, E, H) -> bool:
    """Does the HIP path take this shape (include/coattn.h coattn_lstm_supported)?  No GPU call."""
    return bool(_lib.load().coattn_lstm_supported(B, T, E, H, _lib.F32))


def device_lengths(lens, device):
    """`lens` (any integer tensor, or a list) as an int32 tensor on `device`, without a host read of a device tensor."""
    if torch.is_tensor(lens):
        return lens.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()
    return torch.as_tensor(list(lens), dtype=torch.int32).to(device, non_blocking=True)


def _forward_call(X, lens, p, out, x_masked, saved, ws, stream):
    (B, T, E), H = X.shape, out.shape[2]
    return _lib.bind("coattn_lstm_forward", X=X, len=lens, p=p, out=out, x_masked=x_masked, saved=saved, ws=ws, B=B, T=T, E=E,
                     H=H, dtype=_lib.F32, flags=0, stream=stream)


def _backward_call(X, lens, p, saved, g_out, g_xmasked, dX, pg, ws, H, stream):
    B, T, E = X.shape                                    # (out: reserved by the header, NULL)
    return _lib.bind("coattn_lstm_backward", X=X, len=lens, p=p, out=None, saved=saved, g_out=g_out, g_xmasked=g_xmasked, dX=dX,
                     pg=pg, accumulate=0, ws=ws, B=B, T=T, E=E, H=H, dtype=_lib.F32, flags=0, stream=stream)


class _SentenceLstmFn(torch.autograd.Function):
    """forward -> coattn_lstm_forward, backward -> coattn_lstm_backward (once differentiable: the backward is a kernel
    call, not autograd operations).  The state for the backward is written only when an input needs a gradient; the
    backward skips the dX product when x needs none, and computes the four parameter gradients together (one call of the
    C-ABI: the step kernels' gate gradients serve all four), returning those that are asked for."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)     # fp32 island under autocast
    def forward(ctx, x, lens, w_ih, w_hh, b_ih, b_hh):
        if not x.is_cuda:
            raise RuntimeError("sentence_lstm (HIP) needs tensors on the GPU")
        if x.dtype != torch.float32:
            raise RuntimeError("sentence_lstm (HIP) computes in fp32; got %s" % x.dtype)
        B, T, E = x.shape
        H = w_hh.shape[1]
        if tuple(w_ih.shape) != (4 * H, E) or tuple(w_hh.shape) != (4 * H, H) or tuple(b_ih.shape) != (4 * H,) \
                or tuple(b_hh.shape) != (4 * H,):
            raise RuntimeError("LSTM parameters must be [4H,E], [4H,H], [4H], [4H] with E = %d, H = %d" % (E, H))
        X = x.contiguous()
        ps = [t.contiguous() for t in (w_ih, w_hh, b_ih, b_hh)]
        need_grad = any(ctx.needs_input_grad)
        sb, fb, _ = _lib.lstm_workspace_bytes(B, T, E, H)
        out = torch.empty((B, T, H), dtype=torch.float32, device=x.device)
        x_masked = torch.empty_like(X)
        saved = torch.empty(sb, dtype=torch.uint8, device=x.device) if need_grad else None
        ws = torch.empty(fb, dtype=torch.uint8, device=x.device)
        p = _lib.LstmParams(*[t.data_ptr() for t in ps])
        with _lib.on_device(x.device):
            _forward_call(X, lens, p, out, x_masked, saved, ws, _lib.stream_ptr(x.device))()
        if need_grad:
            ctx.save_for_backward(X, lens, saved, *ps)           # (not out: the backward takes h_{t-1} from saved)
        return out, x_masked

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, g_xm):
        X, lens, saved, *ps = ctx.saved_tensors
        B, T, E = X.shape
        H = ps[1].shape[1]
        g_out = X.new_zeros((B, T, H)) if g_out is None else g_out.contiguous().float()
        g_xm = None if g_xm is None else g_xm.contiguous().float()
        _, _, bb = _lib.lstm_workspace_bytes(B, T, E, H)
        ws = torch.empty(bb, dtype=torch.uint8, device=X.device)
        dX = torch.empty_like(X) if ctx.needs_input_grad[0] else None
        grads = [torch.empty_like(t) for t in ps]
        p = _lib.LstmParams(*[t.data_ptr() for t in ps])
        pg = _lib.LstmParamGrads(*[t.data_ptr() for t in grads])
        with _lib.on_device(X.device):
            _backward_call(X, lens, p, saved, g_out, g_xm, dX, pg, ws, H, _lib.stream_ptr(X.device))()
        return (dX, None, *[g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:])])


def sentence_lstm(x, lens, w_ih, w_hh, b_ih, b_hh):
    """x [B,T,E] (fp32, CUDA), lens [B] -> (sentence [B,T,H], x_masked [B,T,E]): the one-layer LSTM with nn.LSTM's
    parameters (weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0) over each question's first len_b steps from a zero
    state, exact zeros beyond, and x with its rows past the lengths zeroed -- what pack_padded_sequence -> nn.LSTM ->
    pad_packed_sequence return for the LSTM's output and for its input.  `lens`: any integer tensor or list, in any order;
    values outside [1, T] are clamped on the device.  No host read, no sorting."""
    return _SentenceLstmFn.apply(x, device_lengths(lens, x.device), w_ih, w_hh, b_ih, b_hh)

"""``AlternatingCoAttention``: the paper's second co-attention form (Lu et al. 2016, section 3.3) on MI355X.

Three chained guided-attention steps instead of the parallel form's T x N affinity: a question summary s^ (step 1), the
image attended under s^ (step 2, v), the question attended under v (step 3, q).  Same call surface as
``ParallelCoAttention``; the computation runs in the HIP library through ``coattn_alt_forward`` / ``coattn_alt_backward``
(include/coattn.h v0.11.0) on the caller's current stream, in the exact mode only.
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn as nn

from . import _lib
from .coattention import _run_backward, _run_forward, _strides, question_lengths


def _features(x_img: torch.Tensor) -> torch.Tensor:
    """x_img[B,N,d] by pointer and strides when both inner strides are positive (location- or channel-major views), else a
    contiguous copy (inside autograd: the copy stays differentiable)."""
    sB, sN, sD = _strides(x_img)
    B, N, d = x_img.shape
    if sN > 0 and sD > 0 and sB > (N - 1) * sN + (d - 1) * sD:
        return x_img
    return x_img.contiguous()


class _AltFn(torch.autograd.Function):
    """forward -> coattn_alt_forward (v, q [L,B,d], a_v [L,B,N], a_q [L,B,T]); backward -> coattn_alt_backward.  With no
    input that needs a gradient the forward keeps no state (saved = NULL)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)     # fp32 island under autocast
    def forward(ctx, x_img, q_len, *tensors):
        npar = len(_lib.ALT_PARAM_NAMES)
        params, x_ques = tensors[:npar], tensors[npar:]
        B, N, d = x_img.shape
        T = x_ques[0].shape[1]
        for q in x_ques:
            if tuple(q.shape) != (B, T, d):
                raise RuntimeError("question features must all be [B,T,d] = %s, got %s" % ((B, T, d), tuple(q.shape)))
        V = _features(x_img)
        Qs = [q.contiguous() for q in x_ques]
        ps = [t.contiguous() for t in params]
        keep = any(ctx.needs_input_grad)
        outs, saved, _ = _run_forward("coattn_alt_forward", V, Qs, q_len, _lib.AltParams(*[t.data_ptr() for t in ps]),
                                      _lib.alt_workspace_bytes(B, N, T, d, len(Qs)), 0, keep, maps=True)
        ctx.set_materialize_grads(False)              # (an unused map's gradient stays None: NULL for the C-ABI)
        if keep:
            ctx.save_for_backward(V, saved, q_len, *ps, *Qs)
            ctx.x_img_stride_d = x_img.stride(2)
        return outs

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_v, g_q, g_av, g_aq):
        sv = ctx.saved_tensors
        npar = len(_lib.ALT_PARAM_NAMES)
        V, saved, q_len, params, Qs = sv[0], sv[1], sv[2], sv[3:3 + npar], sv[3 + npar:]
        (B, N, d), T = V.shape, Qs[0].shape[1]
        dV, grads, dQs = _run_backward("coattn_alt_backward", (_lib.AltParams, _lib.AltParamGrads), V, Qs, q_len, params, saved,
                                       _lib.alt_workspace_bytes(B, N, T, d, len(Qs)), 0, g_v, g_q, g_av, g_aq,
                                       ctx.x_img_stride_d if ctx.needs_input_grad[0] else None)
        return (dV, None, *grads, *dQs)


class AlternatingCoAttention(nn.Module):
    """Alternating co-attention over image and word/phrase/sentence question features (Lu et al. 2016, section 3.3, eq. 6).

    Per sample and level, with guided(X, g): H = tanh(W_x(X) + g), a = softmax(w_h(H)), x^ = a^T X,
        s^ = guided(Q, 0);  v = guided(V, W_g2(s^));  q = guided(Q, W_g3(v)).
    One parameter set serves all levels, as in ``ParallelCoAttention``; every step has its own.  The ``state_dict`` keys
    (``W_x1, w_h1, W_x2, W_g2, w_h2, W_x3, W_g3, w_h3``) differ from the parallel form's, so neither checkpoint loads into the
    other.  ``question_mask=True``: steps 1 and 3 run over the first ``x_ques_lens[b]`` tokens alone (a_s, a_q are 0 past
    the length, dQ is 0 there).  Exact fp32 products only: ``fast_products`` and ``bf16_projections`` must stay False.
    """

    def __init__(self, hidden_dim: int, question_mask: bool = False):
        super().__init__()
        self.hidden_dim = hidden_dim
        self.question_mask = bool(question_mask)
        self.W_x1 = nn.Linear(hidden_dim, hidden_dim)
        self.w_h1 = nn.Linear(hidden_dim, 1)
        self.W_x2 = nn.Linear(hidden_dim, hidden_dim)
        self.W_g2 = nn.Linear(hidden_dim, hidden_dim)
        self.w_h2 = nn.Linear(hidden_dim, 1)
        self.W_x3 = nn.Linear(hidden_dim, hidden_dim)
        self.W_g3 = nn.Linear(hidden_dim, hidden_dim)
        self.w_h3 = nn.Linear(hidden_dim, 1)
        # (the parallel form's precision switches, kept so that code that sets them finds them; only False runs here)
        self.fast_products = False
        self.bf16_projections = False

    def _params(self):
        return (self.W_x1.weight, self.W_x1.bias, self.w_h1.weight, self.w_h1.bias,
                self.W_x2.weight, self.W_x2.bias, self.W_g2.weight, self.W_g2.bias, self.w_h2.weight, self.w_h2.bias,
                self.W_x3.weight, self.W_x3.bias, self.W_g3.weight, self.W_g3.bias, self.w_h3.weight, self.w_h3.bias)

    def _check(self, x_img: torch.Tensor, ques):
        if self.fast_products or self.bf16_projections:
            raise RuntimeError("AlternatingCoAttention runs in the exact mode only: fast_products and bf16_projections must be "
                               "False")
        if not x_img.is_cuda or any(not q.is_cuda for q in ques):
            raise RuntimeError("AlternatingCoAttention (HIP) needs tensors on the GPU; there is no CPU fallback")
        if x_img.dtype != torch.float32 or any(q.dtype != torch.float32 for q in ques):
            raise RuntimeError("AlternatingCoAttention (HIP) computes in fp32; got %s" % x_img.dtype)
        if x_img.dim() != 3 or not ques:
            raise RuntimeError("x_img must be [B,N,d] and the question hierarchy non-empty")

    def _lengths(self, x_img: torch.Tensor, x_ques_lens):
        if not self.question_mask:
            return None
        if x_ques_lens is None:
            raise ValueError("AlternatingCoAttention(question_mask=True) needs x_ques_lens, the length of every question")
        return question_lengths(x_ques_lens, x_img.shape[0], x_img.device)

    def forward(self, x_img: torch.Tensor, x_ques_hierarchy: Sequence[torch.Tensor], x_ques_lens=None,
                return_attention: bool = False):
        """x_img [B,N,d]; x_ques_hierarchy: list of [B,T,d] -> (list of v_l [B,d], list of q_l [B,d]); with
        return_attention=True also a_v [L,B,N] (step 2) and a_q [L,B,T] (step 3), differentiable."""
        ques = list(x_ques_hierarchy)
        self._check(x_img, ques)
        q_len = self._lengths(x_img, x_ques_lens)
        v, q, a_v, a_q = _AltFn.apply(x_img, q_len, *self._params(), *ques)
        n = v.shape[0]
        if return_attention:
            return [v[l] for l in range(n)], [q[l] for l in range(n)], a_v, a_q
        return [v[l] for l in range(n)], [q[l] for l in range(n)]

    def forward_with_attention(self, x_img: torch.Tensor, x_ques_hierarchy: Sequence[torch.Tensor], x_ques_lens=None):
        """Inference with the maps: (list of v_l, list of q_l, a_v [L,B,N], a_q [L,B,T]); forward only (no backward state),
        v / q bit-identical to `forward`'s."""
        with torch.no_grad():
            return self.forward(x_img, x_ques_hierarchy, x_ques_lens, return_attention=True)

"""``ParallelCoAttention``: drop-in for /root/reference/model.py:337-397 on MI355X.

Same constructor, attribute names (=> identical ``state_dict`` keys ``W_b, W_v, W_q, w_v, w_q``)
and ``forward(x_img, x_ques_hierarchy)`` signature as the reference class; the computation runs
in the HIP library through the C-ABI of ``include/coattn.h`` on the caller's current stream.
Opt-in beyond the reference: ``question_mask=True`` restricts the question-side attention to the
first ``x_ques_lens[b]`` tokens of every question (the C-ABI's ``*_len`` entry points), and
``forward(..., return_attention=True)`` also returns the attention maps a_v, a_q as differentiable
tensors (the C-ABI's ``coattn_forward_maps`` / ``coattn_backward_maps``), for losses on the maps, and
``affinity="bilinear"`` uses the constructed-but-dead ``W_b`` as the published model does, C = tanh(W_b(Q) V^T)
(the C-ABI's ``COATTN_FLAG_BILINEAR``), so that it trains.
"""
from __future__ import annotations

import os
from typing import Sequence

import torch
import torch.nn as nn

from . import _lib


def _impl_flag() -> int:
    f = {"auto": _lib.IMPL_AUTO, "general": _lib.IMPL_GENERAL, "fused": _lib.IMPL_FUSED}[
        os.environ.get("COATTN_IMPL", "auto")]
    if os.environ.get("COATTN_BF16_PROJ", "0") not in ("0", ""):
        f |= _lib.FLAG_BF16_PROJ
    return f


def _is_native(x_img: torch.Tensor, lm_only: bool = False) -> bool:
    B, N, d = x_img.shape
    sB, sN, sD = _strides(x_img)
    ext = (N - 1) * sN + (d - 1) * sD
    lm = sD == 1 and sN == d
    cm = sN == 1 and sD == N and N % 4 == 0 and not lm_only
    return bool((lm or cm) and sB > ext and x_img.data_ptr() % 16 == 0)


# Frozen channel-major features (the reference's NCHW view at N = 196): the kernels read them in place through the C-ABI's
# strides, but the location-major kernels are faster by more than the library's one-pass conversion costs (cfg 2, N = 196: the
# isolated hot path 0.71 ms in place, 0.64 location-major, the conversion 28 us) -- so the host converts.  "inplace" keeps
# them where they lie (VQA_CM_FEATURES=inplace, or set this attribute).
CM_FEATURES = os.environ.get("VQA_CM_FEATURES", "convert")


def _native_layout(x_img: torch.Tensor) -> torch.Tensor:
    """The fp32 module input x_img[B,N,d] as the kernels take it: by pointer + element strides, no copy, when it is
    location-major (a channels_last encoder: contiguous [B,N,d]) or channel-major (the permuted view of an NCHW
    encoder, model.py:215-217: strides (d N, 1, N)) with rows that are 16-byte multiples (N % 4 == 0: N = 196);
    anything else is made contiguous -- location-major -- once.  That includes channel-major features at N = 49: their
    196-byte rows push the projection GEMMs onto dword loads (2 x 80 us per step), a 16 MB re-layout costs 8 us.
    (Inside autograd, where the copy must stay differentiable; features that need no gradient come through
    `native_features`, whose copy is the library's one-pass kernel.)"""
    if _is_native(x_img):
        return x_img
    return x_img.contiguous()


def native_features(x_img: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """Image features that need NO gradient (the frozen encoder of every BASELINE config, model.py:239-241), as the
    encoder left them -- fp32 or bf16 (an autocast encoder, main.py:73, :185), any strides -- in a layout the kernels
    run on: the tensor itself when it is fp32 and native already (see `_native_layout`), else ONE pass of
    coattn_features_native into fp32 [B,N,d] (`out`, if given: a contiguous fp32 buffer of that shape).  What torch
    makes of the same input is an up-cast and a strided copy: two passes, the second at a quarter of the memory rate."""
    if x_img.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("native_features is for features without a gradient (use the module: its copy is differentiable)")
    if not x_img.is_cuda or x_img.dtype not in (torch.float32, torch.bfloat16):
        x = x_img.detach().to(torch.float32)
        x = _native_layout(x)
        if out is None:
            return x
        out.copy_(x)
        return out
    if out is None and x_img.dtype == torch.float32 and _is_native(x_img, lm_only=CM_FEATURES != "inplace"):
        return x_img
    B, N, d = x_img.shape
    if _strides(x_img)[2] == 1:                      # rows along the channels already: a plain (vectorised) up-cast / copy
        if out is None:
            return _native_layout(x_img.to(torch.float32))
        out.copy_(x_img)
        return out
    if out is None:
        out = torch.empty((B, N, d), device=x_img.device, dtype=torch.float32)
    elif (tuple(out.shape) != (B, N, d) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x_img.device):
        raise RuntimeError("native_features: `out` must be a contiguous fp32 [B,N,d] tensor on the features' device")
    if min(_strides(x_img)) < 0:
        raise RuntimeError("native_features: negative strides")
    with _lib.on_device(x_img.device):
        _features_native_call(x_img, out, _lib.stream_ptr(x_img.device))()
    return out


def _features_native_call(x_img, out, stream):
    (B, N, d), (sB, sN, sD) = x_img.shape, _strides(x_img)
    return _lib.bind("coattn_features_native", x=x_img, x_dtype=_lib.BF16 if x_img.dtype == torch.bfloat16 else _lib.F32,
                     sB=sB, sN=sN, sD=sD, out=out, B=B, N=N, d=d, stream=stream)


def question_lengths(x_ques_lens, B: int, device) -> torch.Tensor:
    """The question lengths as the *_len entry points read them: a contiguous int32 [B] tensor on `device`.  A device
    tensor is converted there (no host synchronisation); host lengths (a list, a CPU tensor -- what the question encoder's
    pack_padded_sequence takes) are copied up asynchronously.  Values are not checked here (that would synchronise): the
    kernels clamp them into [1, T]."""
    if x_ques_lens is None:
        raise ValueError("question_mask=True needs the question lengths (x_ques_lens)")
    t = x_ques_lens if torch.is_tensor(x_ques_lens) else torch.as_tensor(x_ques_lens)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError("question lengths must be integers, got %s" % t.dtype)
    if tuple(t.shape) != (B,):
        raise ValueError("question lengths must have shape [B] = [%d], got %s" % (B, tuple(t.shape)))
    return t.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()


def _strides(x: torch.Tensor):
    """Element strides of x[B,N,d] for the C-ABI.  The stride torch reports for a size-1 dimension is arbitrary (and
    ``.contiguous()`` keeps it): such dimensions get the stride a contiguous [B,N,d] tensor would have."""
    B, N, d = x.shape
    sB, sN, sD = x.stride()
    if d == 1:
        sD = 1
    if N == 1:
        sN = d * sD if sD == 1 else 1
    if B == 1:
        sB = max(sB, (N - 1) * sN + (d - 1) * sD + 1, N * d)
    return sB, sN, sD


def _shared_args(V, Qs, q_len, p, ws, flags):
    """The arguments every co-attention call takes, parallel or alternating, forward or backward, by the header's names
    (all but `stream`)."""
    (B, N, d), T = V.shape, Qs[0].shape[1]
    sB, sN, sD = _strides(V)
    return dict(V=V, v_sB=sB, v_sN=sN, v_sD=sD, Q=_lib.ptr_array(Qs), q_len=q_len, p=p, ws=ws, B=B, N=N, T=T, d=d,
                L=len(Qs), dtype=_lib.F32, flags=flags)


def _run_forward(symbol, V, Qs, q_len, p, sizes, flags, keep, maps):
    """The forward `symbol` on the current stream, for V in a layout the kernels take and contiguous Qs: allocates v, q
    [L,B,d], with `maps` also a_v [L,B,N] and a_q [L,B,T], with `keep` the backward's state (NULL otherwise: nothing is kept).
    sizes: the family's (saved, ws_fwd, ws_bwd) bytes.  Returns (the outputs, saved or None, the workspace)."""
    (B, N, d), T, L, dev = V.shape, Qs[0].shape[1], len(Qs), V.device
    outs = tuple(torch.empty((L, B, n), device=dev, dtype=torch.float32) for n in ((d, d, N, T) if maps else (d, d)))
    kw = dict(zip(("v_out", "q_out", "av_out", "aq_out"), outs))
    saved = None
    if keep:
        saved = kw["saved"] = torch.empty(sizes[0] // 4, device=dev, dtype=torch.float32)
    stream = _lib.stream_ptr(dev)
    ws = _lib.scratch(sizes[1], dev, stream)             # per-stream scratch, reused from call to call
    with _lib.on_device(dev):
        _lib.bind(symbol, stream=stream, **_shared_args(V, Qs, q_len, p, ws, flags), **kw)()
    return outs, saved, ws


def _run_backward(symbol, structs, V, Qs, q_len, params, saved, sizes, flags, g_v, g_q, g_av, g_aq, dv_stride_d):
    """The backward `symbol` on the current stream.  A missing g_v / g_q goes in as zeros, a missing map gradient as NULL.
    structs: the family's (parameters, parameter gradients) structures; dv_stride_d: None when x_img needs no gradient, else
    x_img's innermost stride -- dV takes the layout of x_img itself.  Returns (dV, parameter gradients, dQs)."""
    (B, N, d), L, dev = V.shape, len(Qs), V.device
    g_v = g_v.contiguous() if g_v is not None else torch.zeros((L, B, d), device=dev)
    g_q = g_q.contiguous() if g_q is not None else torch.zeros((L, B, d), device=dev)
    g_av = g_av.contiguous() if g_av is not None else None
    g_aq = g_aq.contiguous() if g_aq is not None else None
    stream = _lib.stream_ptr(dev)
    ws = _lib.scratch(sizes[2], dev, stream)
    dV, kw = None, {}
    if dv_stride_d is not None:
        dV = (torch.empty((B, N, d), device=dev) if dv_stride_d == 1
              else torch.empty((B, d, N), device=dev).permute(0, 2, 1))
        kw = dict(zip(("dV", "dv_sB", "dv_sN", "dv_sD"), (dV, *_strides(dV))))
    dQs = [torch.empty_like(q) for q in Qs]
    grads = [torch.empty_like(t) for t in params]
    p, pg = structs[0](*[t.data_ptr() for t in params]), structs[1](*[t.data_ptr() for t in grads])
    with _lib.on_device(dev):
        _lib.bind(symbol, stream=stream, saved=saved, gv=g_v, gq=g_q, g_av=g_av, g_aq=g_aq, dQ=_lib.ptr_array(dQs), pg=pg,
                  accumulate=0, **_shared_args(V, Qs, q_len, p, ws, flags), **kw)()
    return dV, grads, dQs


def _forward(ctx, x_img, x_ques, params, impl, q_len, maps):
    """The parallel form's forward (params: the ten of `_param_list`): validate, lay out, call, note the tolerance mode's status words, and -- ctx: the autograd
    context, None from forward_with_attention -- keep the backward's state when an input needs a gradient.  With state the
    call is coattn_forward_len (coattn_forward_maps_len with `maps`), without it coattn_infer_len; q_len None = unmasked."""
    if not x_img.is_cuda:
        raise RuntimeError("ParallelCoAttention (HIP) needs tensors on the GPU; there is no CPU fallback")
    if x_img.dtype != torch.float32 or any(q.dtype != torch.float32 for q in x_ques):
        raise RuntimeError("ParallelCoAttention (HIP) computes in fp32; got %s" % x_img.dtype)
    L = len(x_ques)
    B, N, d = x_img.shape
    T = x_ques[0].shape[1]
    for q in x_ques:
        if tuple(q.shape) != (B, T, d):
            raise RuntimeError("question features must all be [B,T,d] = %s, got %s" % ((B, T, d), tuple(q.shape)))
    V = _native_layout(x_img)
    Qs = [q.contiguous() for q in x_ques]
    params = _param_list(*params, impl)
    keep = ctx is not None and any(ctx.needs_input_grad)
    symbol = "coattn_infer_len" if not keep else "coattn_forward_maps_len" if maps else "coattn_forward_len"
    outs, saved, ws = _run_forward(symbol, V, Qs, q_len, _lib.Params(*[t.data_ptr() for t in params]),
                                   _lib.workspace_bytes(B, N, T, d, L, impl), impl, keep, maps)
    if impl & _lib.FLAG_FAST16:                       # tolerance mode: where _lib.check_range() finds this call's status words
        _lib.note_status("coattn", saved if keep else ws, (B, N, T, d, L), x_img.device)
    if keep:
        ctx.save_for_backward(V, saved, *params, *Qs)
        ctx.nparams = len(params)
        ctx.impl = impl
        ctx.q_len = q_len                             # (the backward must see the forward's lengths)
    return outs


def _backward(ctx, g_v, g_q, g_av=None, g_aq=None):
    """The parallel form's backward, coattn_backward_maps_len: NULL lengths = unmasked, NULL map gradients = coattn_backward's
    bits."""
    sv = ctx.saved_tensors
    npar = ctx.nparams
    V, saved, params, Qs = sv[0], sv[1], sv[2:2 + npar], sv[2 + npar:]
    (B, N, d), T, L = V.shape, Qs[0].shape[1], len(Qs)
    dV, grads, dQs = _run_backward("coattn_backward_maps_len", (_lib.Params, _lib.ParamGrads), V, Qs, ctx.q_len, params, saved,
                                   _lib.workspace_bytes(B, N, T, d, L, ctx.impl), ctx.impl, g_v, g_q, g_av, g_aq,
                                   V.stride(2) if ctx.needs_input_grad[0] else None)
    if npar == 8:                           # (the reference's affinity: W_b, b_b take no part)
        grads += [None, None]
    return (dV, *grads, None, None, *dQs)


class _CoAttentionFn(torch.autograd.Function):
    """(v, q), each [L,B,d]: autograd of model.py:372-392.  q_len: the question lengths (int32 [B] on the device), given to
    the forward and the backward alike, or None."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)     # fp32 island under autocast
    def forward(ctx, x_img, W_v, b_v, W_q, b_q, w_v, c_v, w_q, c_q, W_b, b_b, impl, q_len, *x_ques):
        return _forward(ctx, x_img, x_ques, (W_v, b_v, W_q, b_q, w_v, c_v, w_q, c_q, W_b, b_b), impl, q_len, maps=False)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_v, g_q):
        return _backward(ctx, g_v, g_q)


class _CoAttentionMapsFn(torch.autograd.Function):
    """The co-attention with differentiable attention maps: (v, q, a_v, a_q) with v, q [L,B,d], a_v [L,B,N], a_q [L,B,T]; the
    backward adds the maps' own upstream gradients in the two softmax backward steps (include/coattn.h).  A map whose
    gradient autograd gives as None goes in as NULL (the backward is then _CoAttentionFn's bit for bit), a missing g_v / g_q
    as zeros.  With no input that needs a gradient the forward keeps no backward state: the same maps."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)     # fp32 island under autocast
    def forward(ctx, x_img, W_v, b_v, W_q, b_q, w_v, c_v, w_q, c_q, W_b, b_b, impl, q_len, *x_ques):
        ctx.set_materialize_grads(False)              # (an unused map's gradient stays None: NULL for the C-ABI)
        return _forward(ctx, x_img, x_ques, (W_v, b_v, W_q, b_q, w_v, c_v, w_q, c_q, W_b, b_b), impl, q_len, maps=True)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g_v, g_q, g_av, g_aq):
        return _backward(ctx, g_v, g_q, g_av, g_aq)


def _param_list(W_v, b_v, W_q, b_q, w_v, c_v, w_q, c_q, W_b, b_b, impl):
    """The parameters in the order of coattn_params: eight, or ten with W_b, b_b under FLAG_BILINEAR."""
    ps = [W_v, b_v, W_q, b_q, w_v, c_v, w_q, c_q]
    if impl & _lib.FLAG_BILINEAR:
        if W_b is None or b_b is None:
            raise ValueError("the bilinear affinity needs W_b and b_b")
        ps += [W_b, b_b]
    return [t.contiguous() for t in ps]


def coattention(x_img: torch.Tensor, x_ques: Sequence[torch.Tensor], W_v, b_v, W_q, b_q, w_v, c_v, w_q, c_q,
                impl: int | None = None, q_len: torch.Tensor | None = None, return_attention: bool = False,
                W_b=None, b_b=None):
    """Functional form: returns (v, q), each [L,B,d].  q_len: None (the reference's unmasked softmax over the T tokens), or
    the question lengths (see `question_lengths`): attention over the first q_len[b] tokens of question b.
    return_attention=True: returns (v, q, a_v [L,B,N], a_q [L,B,T]), the maps differentiable (a loss on them reaches every
    input through coattn_backward_maps).
    W_b, b_b given: the bilinear affinity C = tanh((Q W_b^T + b_b) V^T) (FLAG_BILINEAR is added to `impl`), and W_b, b_b
    receive gradients; None (the default): the reference's C = tanh(Q V^T)."""
    if impl is None:
        impl = _impl_flag()
    if (W_b is None) != (b_b is None):
        raise ValueError("the bilinear affinity needs both W_b and b_b")
    if W_b is not None:
        impl |= _lib.FLAG_BILINEAR
    if q_len is not None:
        q_len = question_lengths(q_len, x_img.shape[0], x_img.device)
    if return_attention:
        return _CoAttentionMapsFn.apply(x_img, W_v, b_v, W_q, b_q, w_v, c_v, w_q, c_q, W_b, b_b, impl, q_len, *x_ques)
    return _CoAttentionFn.apply(x_img, W_v, b_v, W_q, b_q, w_v, c_v, w_q, c_q, W_b, b_b, impl, q_len, *x_ques)


class ParallelCoAttention(nn.Module):
    """Parallel co-attention over image and word/phrase/sentence question features.

    Mirrors the reference class (model.py:337-397): ``W_b`` is constructed but never used
    (model.py:347 vs :377) so it stays in the state_dict and never receives a gradient;
    W_v/W_q/w_v/w_q are ``nn.Linear`` with biases; one weight set serves all levels; the
    softmax over question positions is unmasked (model.py:388).

    ``question_mask=True`` (opt-in; not in the reference): ``forward`` / ``forward_with_attention`` then REQUIRE
    ``x_ques_lens`` and compute, per sample b, the reference's co-attention on the first ``x_ques_lens[b]`` question tokens
    alone: a_q is 0 past the length and sums to 1 before it, the affinity rows there count as zero, their gradients are zero
    (include/coattn.h, "length-masked question attention").  With the default (False) the lengths are ignored, as the
    reference ignores them.  The flag is not part of the ``state_dict``: a checkpoint does not say which form trained it.

    ``affinity="bilinear"`` (opt-in; the published model, Lu et al. 2016 eq. 3): the affinity is
    C = tanh(W_b(Q) V^T) = tanh((Q W_b^T + b_b) V^T) instead of the reference's tanh(Q V^T), and ``W_b`` receives gradients
    (include/coattn.h, COATTN_FLAG_BILINEAR).  The ``state_dict`` keys are the same for both forms -- a reference checkpoint
    loads unchanged -- and, as for ``question_mask``, a checkpoint does not record the form.  Not available together with
    ``bf16_projections``.
    """

    AFFINITIES = ("reference", "bilinear")

    def __init__(self, hidden_dim: int, question_mask: bool = False, affinity: str = "reference"):
        super().__init__()
        if affinity not in self.AFFINITIES:
            raise ValueError("affinity must be one of %s, got %r" % (self.AFFINITIES, affinity))
        self.hidden_dim = hidden_dim
        self.question_mask = bool(question_mask)
        self.affinity = affinity
        self.W_b = nn.Linear(hidden_dim, hidden_dim)     # dead in the reference's forward
        self.W_v = nn.Linear(hidden_dim, hidden_dim)
        self.W_q = nn.Linear(hidden_dim, hidden_dim)
        self.w_v = nn.Linear(hidden_dim, 1)
        self.w_q = nn.Linear(hidden_dim, 1)
        # reduced-precision mode (apex O1 analogue, main.py:185): projections on the bf16 MFMA
        self.bf16_projections = False
        # Precision of the fp32 mode (include/coattn.h "Widths of the fp32 mode").  False -- the default, as the reference:
        # every product fp32-accurate over fp32's range.  True -- the tolerance mode (forward products on two FP16 pieces =
        # 22 significand bits, backward on two bf16 pieces = 16; inside the 1e-4 contract for operands below 65,504 in
        # magnitude; `vqa_amd.check_range()` reports an operand that was not): what train.Trainer(precision="fast") sets.
        self.fast_products = _lib.default_fast()

    def _impl(self) -> int:
        impl = _impl_flag() | (_lib.FLAG_BF16_PROJ if self.bf16_projections else 0) | _lib.precision_flag(self.fast_products)
        if self.affinity == "bilinear":
            if impl & _lib.FLAG_BF16_PROJ:
                raise RuntimeError("ParallelCoAttention(affinity='bilinear') is not available in the reduced-precision mode "
                                   "(bf16_projections / COATTN_BF16_PROJ)")
            impl |= _lib.FLAG_BILINEAR
        return impl

    def _wb(self):
        """(W_b, b_b) when the bilinear affinity is on, else (None, None)."""
        return (self.W_b.weight, self.W_b.bias) if self.affinity == "bilinear" else (None, None)

    def _params(self):
        """The eight parameters in coattn_params' order, then `_wb()`."""
        return (self.W_v.weight, self.W_v.bias, self.W_q.weight, self.W_q.bias, self.w_v.weight, self.w_v.bias,
                self.w_q.weight, self.w_q.bias, *self._wb())

    def _needs_grad(self, x_img, ques) -> bool:
        return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x_img, *ques, *self._params()))

    def _lengths(self, x_img: torch.Tensor, x_ques_lens):
        """int32 [B] lengths on the features' device when the mask is on (required then), else None (ignored)."""
        if not self.question_mask:
            return None
        if x_ques_lens is None:
            raise ValueError("ParallelCoAttention(question_mask=True) needs x_ques_lens, the length of every question")
        return question_lengths(x_ques_lens, x_img.shape[0], x_img.device)

    def forward(self, x_img: torch.Tensor, x_ques_hierarchy: Sequence[torch.Tensor], x_ques_lens=None,
                return_attention: bool = False):
        """x_img [B,N,d]; x_ques_hierarchy: list of [B,T,d] -> (list of v_l [B,d], list of q_l [B,d]).
        x_ques_lens ([B] integers, host or device): read only under ``question_mask``.
        return_attention=True -> (list of v_l, list of q_l, a_v [L,B,N], a_q [L,B,T]) with the maps DIFFERENTIABLE: a loss on
        them (attention supervision, an entropy penalty) reaches the parameters, the question features and x_img
        (coattn_forward_maps / coattn_backward_maps).  v / q and every gradient through them are those of the plain call.
        Where no gradient can be needed (no_grad, or no input that requires one) this is `forward_with_attention`, bit for
        bit."""
        ques = list(x_ques_hierarchy)
        if return_attention and not self._needs_grad(x_img, ques):
            return self.forward_with_attention(x_img, ques, x_ques_lens)
        impl = self._impl()
        q_len = self._lengths(x_img, x_ques_lens)
        if x_img.is_cuda and not (x_img.requires_grad and torch.is_grad_enabled()):
            x_img = native_features(x_img)           # frozen encoder: bf16 / non-native strides in one library pass
        *params, W_b, b_b = self._params()
        out = coattention(x_img, ques, *params, impl=impl, q_len=q_len, return_attention=return_attention, W_b=W_b, b_b=b_b)
        v, q = out[0], out[1]
        n = v.shape[0]
        if return_attention:
            return [v[l] for l in range(n)], [q[l] for l in range(n)], out[2], out[3]
        return [v[l] for l in range(n)], [q[l] for l in range(n)]

    def forward_with_attention(self, x_img: torch.Tensor, x_ques_hierarchy: Sequence[torch.Tensor], x_ques_lens=None):
        """Inference with the attention maps: (list of v_l [B,d], list of q_l [B,d], a_v [L,B,N], a_q [L,B,T]) through
        coattn_infer -- the forward that keeps no backward state (include/coattn.h).  v / q equal `forward`'s bit for bit.
        a_v[l, b] is the softmax over the N image locations (model.py:387), a_q[l, b] the one over the T tokens
        (model.py:388), unmasked as the reference's: pad tokens carry weight -- under ``question_mask`` (coattn_infer_len)
        a_q[l, b, t] is 0 for t >= x_ques_lens[b].  Raises if a gradient would be needed."""
        ques = list(x_ques_hierarchy)
        if self._needs_grad(x_img, ques):
            raise RuntimeError("forward_with_attention is forward only: run it under torch.no_grad() (the maps come from "
                               "the inference path, which keeps no state for a backward)")
        if not x_img.is_cuda:
            raise RuntimeError("ParallelCoAttention (HIP) needs tensors on the GPU; there is no CPU fallback")
        impl = self._impl()
        q_len = self._lengths(x_img, x_ques_lens)
        out_v, out_q, a_v, a_q = _forward(None, native_features(x_img), ques, self._params(), impl, q_len, maps=True)
        return [out_v[l] for l in range(len(ques))], [out_q[l] for l in range(len(ques))], a_v, a_q

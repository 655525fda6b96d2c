"""``word_embedding``: the word level of the question hierarchy (reference model.py: nn.Embedding over the token ids) on
MI355X -- the gather as one HIP launch of 16-byte copies, its dense gradient as one launch in which every vocabulary row is
owned by one workgroup that finds its own occurrences (``csrc/embedding.hip``: no sort, no fill, no float atomics, the ids
never read on the host) -- through the C-ABI of ``include/coattn.h`` on the caller's current stream.  DESIGN.md section 3.14.
"""
from __future__ import annotations

import torch

from . import _lib

_IDS_DTYPES = {torch.int32: _lib.IDS_I32, torch.int64: _lib.IDS_I64}


def supported(n, V, E) -> bool:
    """Does the HIP path take this shape (include/coattn.h coattn_embedding_supported)?  No GPU call."""
    return bool(_lib.load().coattn_embedding_supported(n, V, E, _lib.F32))


def device_ids(ids):
    """`ids` as the kernels read them: contiguous int32 or int64 as they are, any other integer dtype cast on the device."""
    if ids.dtype not in _IDS_DTYPES:
        if ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool:
            raise RuntimeError("word_embedding takes integer ids; got %s" % ids.dtype)
        ids = ids.to(torch.int64 if ids.element_size() == 8 else torch.int32)
    return ids.contiguous()


_bad = {}                     # device index -> int32[1] counter the forwards add to


def _counter(dev):
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    c = _bad.get(key)
    if c is None:
        c = _bad[key] = torch.zeros(1, device=torch.device("cuda", key), dtype=torch.int32)
    return c


def bad_ids() -> int:
    """How many token ids outside [0, V) the word_embedding forwards of this process have met (each gave a row of zeros
    and no gradient) since the last call, over all devices; clears the count.  Synchronises every device it reads -- the
    forwards may have run on any stream of it -- so call it where the host reads the loss, not in the step."""
    total = 0
    for key, c in _bad.items():
        torch.cuda.synchronize(key)                              # (the whole device, not the current stream alone)
        total += int(c.item())
        c.zero_()
        torch.cuda.synchronize(key)                              # the clear lands before a forward on another stream adds
    return total


class _WordEmbeddingFn(torch.autograd.Function):
    """forward -> coattn_embedding_forward, backward -> coattn_embedding_backward (once differentiable: the backward is a
    kernel call).  Saves the ids alone; the backward is not reached when the weight needs no gradient."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)     # fp32 island under autocast
    def forward(ctx, ids, weight, padding_idx):
        if not (ids.is_cuda and weight.is_cuda):
            raise RuntimeError("word_embedding (HIP) needs tensors on the GPU")
        if weight.dtype != torch.float32 or weight.dim() != 2:
            raise RuntimeError("word_embedding (HIP) takes an fp32 [V, E] weight; got %s %s" % (weight.dtype, tuple(weight.shape)))
        V, E = weight.shape
        flat = device_ids(ids).reshape(-1)
        n = flat.numel()
        pad = -1 if padding_idx is None else int(padding_idx)
        W = weight.contiguous()
        out = torch.empty((n, E), dtype=torch.float32, device=weight.device)
        with _lib.on_device(weight.device):
            _lib.bind("coattn_embedding_forward", ids=flat, ids_dtype=_IDS_DTYPES[flat.dtype], W=W, out=out,
                      bad_ids=_counter(weight.device), n=n, V=V, E=E, padding_idx=pad, dtype=_lib.F32, flags=0,
                      stream=_lib.stream_ptr(weight.device))()
        if ctx.needs_input_grad[1]:
            ctx.save_for_backward(flat)
            ctx.dims = (n, V, E, pad)
        return out.view(*ids.shape, E)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        if not ctx.needs_input_grad[1]:
            return None, None, None
        (flat,) = ctx.saved_tensors
        n, V, E, pad = ctx.dims
        g = g_out.reshape(n, E).contiguous().float()
        dW = torch.empty((V, E), dtype=torch.float32, device=g.device)            # dense; every element written by the call
        nbytes = _lib.embedding_workspace_bytes(n, V, E)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=g.device) if nbytes else None
        with _lib.on_device(g.device):
            _lib.bind("coattn_embedding_backward", ids=flat, ids_dtype=_IDS_DTYPES[flat.dtype], g_out=g, dW=dW, ws=ws, n=n, V=V,
                      E=E, padding_idx=pad, accumulate=0, dtype=_lib.F32, flags=0, stream=_lib.stream_ptr(g.device))()
        return None, dW, None


def word_embedding(ids, weight, padding_idx=0):
    """ids [...] (any integer dtype, CUDA), weight [V, E] (fp32, CUDA) -> [..., E]: weight[ids], what
    F.embedding(ids, weight, padding_idx) returns, with the dense [V, E] gradient of nn.Embedding in a fixed summation order
    (include/coattn.h).  ``padding_idx=None``: no padding row.  An id outside [0, V) gives a row of zeros and no gradient
    where stock PyTorch device-asserts; ``embedding.bad_ids()`` reports how many there were.  No host read of the ids."""
    return _WordEmbeddingFn.apply(ids, weight, padding_idx)

"""The memory-bound glue of the frozen image encoder on the HIP library (csrc/encoder.hip, include/coattn.h v0.22.0), for
channels_last fp32 tensors; the convolutions stay on MIOpen, but for the first.  ``modules.run_conv_bn_stack`` decides which
layer takes what:

* ``relu_pool``: ``MaxPool2d(2, 2)`` + ``ReLU`` in one pass.  Both are exact operations: the values are the stock kernels' bit
  for bit.  The default (``mode() == "pool"``).
* ``bn_exact``: train-mode ``BatchNorm2d`` + ``ReLU`` + an optional ``MaxPool2d(2, 2)`` in two passes, summed in MIOpen's order
  with MIOpen's formula: the stock chain's bits.  Also the default, but only for a shape that ``bn_exact_or_stock`` has compared
  with the stock chain once in this process and found equal in every bit (``exact_report()``); ``VQA_ENCODER_EXACT_BN=0``
  turns it off.
* ``bn_exact(..., conv=conv)``: the same with the first convolution (3 -> 64 channels, 3x3, padding 1) in front, computed in
  the stock kernel's arithmetic by the kernel that also sums its statistics.  The default for the first group, again only for a
  shape that ``conv1_bn_exact_or_stock`` has compared with the stock convolution and chain once and found equal in every bit;
  ``VQA_ENCODER_EXACT_CONV1=0`` turns it off (and so does whatever turns ``bn_exact`` off).  The convolution output is never
  stored: one kernel computes it for the statistics, another computes it again and normalises, pools and writes the result
  (``coattn_conv1_bn_recompute_forward``), compared with the stock kernels in the same first call.
  ``VQA_ENCODER_CONV1_RECOMPUTE=0`` keeps the form that stores the convolution output and reads it back
  (``coattn_conv1_bn_exact_forward``), for A/B runs and as an escape.
* ``bn_relu_pool``: train-mode ``BatchNorm2d`` + ``ReLU`` + an optional ``MaxPool2d(2, 2)`` in two passes over the convolution
  output, statistics in double.  More accurate than the stock chain, but not its bits: a training trajectory leaves the stock
  one at rounding level and drifts from there.  Opt-in: ``VQA_ENCODER_FUSED=1``.

* ``bn_eval`` / ``conv1_bn_eval`` (include/coattn_ext.h v0.24.0): EVAL-mode ``BatchNorm2d`` on its running statistics, the
  convolution's bias, the ReLU and an optional ``MaxPool2d(2, 2)`` in ONE launch over the convolution output, in the stock
  inference kernel's arithmetic; the first group in one launch from the image.  Opt-in (``eval_impl="hip"``,
  ``--encoder_eval hip``), and again only for a shape that ``bn_eval_or_stock`` / ``conv1_bn_eval_or_stock`` has compared with the
  stock chain once in this process and found equal in every bit (``eval_report()``).

``VQA_ENCODER_FUSED=0`` keeps every stock kernel of the train-mode routes."""
from __future__ import annotations

import os
import warnings

import torch
import torch.nn as nn

from . import _lib


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def pool_is_2x2(pool: nn.MaxPool2d) -> bool:
    """kernel 2, stride 2, no padding, no dilation, floor mode, no indices: the one pool the kernel implements."""
    stride = pool.kernel_size if pool.stride is None else pool.stride
    return (_pair(pool.kernel_size) == (2, 2) and _pair(stride) == (2, 2) and _pair(pool.padding) == (0, 0)
            and _pair(pool.dilation) == (1, 1) and not pool.ceil_mode and not pool.return_indices)


def mode() -> str:
    """VQA_ENCODER_FUSED: "0" -> "stock", "1" -> "bn" (BatchNorm too), anything else or unset -> "pool" (the exact pool + ReLU)."""
    return {"0": "stock", "1": "bn"}.get(os.environ.get("VQA_ENCODER_FUSED", ""), "pool")


def relu_pool_fusable(pool: nn.MaxPool2d, x: torch.Tensor) -> bool:
    """A 2x2 pool of a CUDA fp32 channels_last tensor that autograd need not record, of a shape the kernel takes."""
    if mode() == "stock" or not pool_is_2x2(pool) or (torch.is_grad_enabled() and x.requires_grad):
        return False
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)):
        return False
    B, Ch, H, W = x.shape
    return bool(_lib.load().coattn_bn_supported(B, H, W, Ch, 1, _lib.F32))


def relu_pool(x: torch.Tensor) -> torch.Tensor:
    """relu(max_pool2d(x, 2, 2)) of a channels_last fp32 [B,C,H,W] tensor as a channels_last tensor, bit for bit.  Forward
    only; runs on torch's current stream."""
    B, Ch, H, W = x.shape
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)):
        raise ValueError("relu_pool: needs a CUDA fp32 channels_last [B,C,H,W] tensor, got %s %s strides %s"
                         % (tuple(x.shape), x.dtype, x.stride()))
    y = _empty_y(x, Ch, True)
    with _lib.on_device(x.device):
        _relu_pool_call(x, y, _lib.stream_ptr(x.device))()
    return y


def _relu_pool_call(x, y, stream):
    B, Ch, H, W = x.shape
    return _lib.bind("coattn_relu_pool_forward", x=x, y=y, B=B, H=H, W=W, C=Ch, dtype=_lib.F32, stream=stream)


def _empty_y(x, Ch: int, pool: bool):
    """The channels_last fp32 [B,Ch,H,W] result of a group over x [B,.,H,W], H and W halved by the pool."""
    B, _, H, W = x.shape
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    return torch.empty((B, Ch, Ho, Wo), device=x.device, dtype=torch.float32, memory_format=torch.channels_last)


def _workspace(dev, symbol, *dims):
    """The fp32 workspace `symbol` sizes for dims, from torch's allocator under the current stream, per call: the encoder may
    run one step ahead on its own stream while an inline pass runs on the main one."""
    return torch.empty((_lib.size_bytes(symbol, *dims) + 3) // 4, device=dev, dtype=torch.float32)


def modules_fusable(conv: nn.Conv2d, bn: nn.BatchNorm2d, pool, x: torch.Tensor) -> bool:
    """What can be told before the convolution runs: batch statistics with tracked running statistics and a momentum, an
    affine map, nothing for autograd to record, a convolution bias that is absent or frozen (it moves into the running
    mean), a 2x2 pool or none, and VQA_ENCODER_FUSED=1."""
    return mode() == "bn" and _group_fusable(conv, bn, pool, x)


def exact_enabled() -> bool:
    """The default mode, unless VQA_ENCODER_EXACT_BN=0."""
    return mode() == "pool" and os.environ.get("VQA_ENCODER_EXACT_BN", "1") != "0"


def exact_modules_fusable(conv: nn.Conv2d, bn: nn.BatchNorm2d, pool, x: torch.Tensor) -> bool:
    """modules_fusable's conditions for the route with the stock kernels' bits: the default mode instead of VQA_ENCODER_FUSED=1,
    and no autocast (the stock BatchNorm then sees another dtype)."""
    return exact_enabled() and not torch.is_autocast_enabled() and _group_fusable(conv, bn, pool, x)


def _group_fusable(conv: nn.Conv2d, bn: nn.BatchNorm2d, pool, x: torch.Tensor) -> bool:
    if not x.is_cuda:
        return False
    if not (bn.training and bn.affine and bn.track_running_stats and bn.momentum is not None and bn.running_mean is not None):
        return False
    params = (conv.weight, conv.bias, bn.weight, bn.bias)
    if torch.is_grad_enabled() and (x.requires_grad or any(p is not None and p.requires_grad for p in params)):
        return False
    if conv.padding_mode != "zeros":
        return False
    b = conv.bias
    if b is not None and (b.requires_grad or b.dtype != torch.float32 or b.device != x.device or not b.is_contiguous()):
        return False
    return pool is None or pool_is_2x2(pool)


def output_fusable(z: torch.Tensor, bn: nn.BatchNorm2d, pool: bool) -> bool:
    """The convolution output the kernels take: CUDA, fp32, physically [B,H,W,C], a shape coattn_bn_supported accepts; and
    BatchNorm2d's parameters and buffers in fp32 beside it."""
    if not (z.is_cuda and z.dtype == torch.float32 and z.dim() == 4 and z.is_contiguous(memory_format=torch.channels_last)):
        return False
    for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
        if t.dtype != torch.float32 or t.device != z.device or not t.is_contiguous():
            return False
    B, Ch, H, W = z.shape
    return bool(_lib.load().coattn_bn_supported(B, H, W, Ch, int(pool), _lib.F32))


def _bn_relu_pool_call(x, bn, conv_bias, y, stats_out, ws, pool, stream):
    B, Ch, H, W = x.shape
    return _lib.bind("coattn_bn_relu_pool_forward", x=x, gamma=bn.weight, beta=bn.bias, conv_bias=conv_bias,
                     running_mean=bn.running_mean, running_var=bn.running_var, momentum=float(bn.momentum), eps=float(bn.eps), y=y,
                     stats_out=stats_out, ws=ws, B=B, H=H, W=W, C=Ch, pool=int(pool), relu=1, dtype=_lib.F32, stream=stream)


def bn_relu_pool(x: torch.Tensor, bn: nn.BatchNorm2d, conv_bias=None, pool: bool = False, stats_out=None) -> torch.Tensor:
    """relu(max_pool2d(bn(x), 2, 2)) (pool) or relu(bn(x)) of a channels_last fp32 [B,C,H,W] tensor with `bn` in train
    mode, as a channels_last tensor; `bn`'s running statistics and num_batches_tracked move as nn.BatchNorm2d moves them.
    `conv_bias`: the frozen bias of the convolution that produced x WITHOUT it -- added to the running mean, the only place
    it survives batch normalisation.  `stats_out`: an fp32 [2, C] tensor that receives the batch mean of x and its biased
    variance.  Forward only; runs on torch's current stream."""
    B, Ch, H, W = x.shape
    for t, shape in ((conv_bias, (Ch,)), (stats_out, (2, Ch))):
        if t is not None and not (t.dtype == torch.float32 and t.device == x.device and t.is_contiguous()
                                  and tuple(t.shape) == shape):
            raise ValueError("bn_relu_pool: conv_bias / stats_out must be contiguous fp32 [C] / [2, C] tensors on x's device")
    if not output_fusable(x, bn, pool):
        raise ValueError("bn_relu_pool: needs a CUDA fp32 channels_last [B,C,H,W] tensor of a shape coattn_bn_supported "
                         "takes, got %s %s strides %s" % (tuple(x.shape), x.dtype, x.stride()))
    y, ws = _empty_y(x, Ch, pool), _workspace(x.device, "coattn_bn_workspace_bytes", B, H, W, Ch)
    with torch.no_grad(), _lib.on_device(x.device):
        _bn_relu_pool_call(x, bn, conv_bias, y, stats_out, ws, pool, _lib.stream_ptr(x.device))()
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
    return y


# ---- the stock kernels' bits: verified per shape, or not used -------------------------------------------------------------
GEOMETRY_FIELDS = ("vec", "g0", "g1", "g2", "samples_per_thread", "pixel_groups", "sample_groups", "f0", "f1", "f2")
# (device index, B, C, H, W, pool) -> {"verified": bool, "first_difference": name or None, "geometry": {...}}, and where the
# tensor was the first convolution's output and that route was compared too, "conv1": {"verified", "first_difference"}
_exact = {}


def exact_geometry(B: int, H: int, W: int, Ch: int):
    """The geometry MIOpen's multi-kernel BatchNorm runs a channels_last fp32 [B,Ch,H,W] tensor with, as coattn_bn_exact_geometry
    reproduces it (a dict over GEOMETRY_FIELDS), or None for a shape the rule does not cover."""
    out = (_lib.C.c_int * len(GEOMETRY_FIELDS))()
    n = _lib.load().coattn_bn_exact_geometry(B, H, W, Ch, _lib.F32, out)
    return dict(zip(GEOMETRY_FIELDS, out)) if n == len(GEOMETRY_FIELDS) else None


def exact_output_fusable(z: torch.Tensor, bn: nn.BatchNorm2d, pool: bool) -> bool:
    """output_fusable, a shape whose MIOpen geometry is known, and 16-byte aligned tensors throughout (the kernels read the
    parameters and the running statistics four channels at a time; a view at an odd offset stays on the stock chain)."""
    if not output_fusable(z, bn, pool) or exact_geometry(z.shape[0], z.shape[2], z.shape[3], z.shape[1]) is None:
        return False
    return all(t.data_ptr() % 16 == 0 for t in (z, bn.weight, bn.bias, bn.running_mean, bn.running_var))


def exact_report() -> dict:
    """{(device index, B, C, H, W, pool): {"verified", "first_difference", "geometry"}} of every shape compared so far; the
    entry of a first-convolution output also holds "conv1": {"verified", "first_difference"} once conv1_bn_exact_or_stock has
    compared that route (a key of the entry: it cannot collide with a BatchNorm shape), and "conv1_recompute", the same of the
    form that never stores the convolution output, once that was compared too."""
    return {k: {n: dict(t) if n in ("conv1", "conv1_recompute") else t for n, t in v.items()} for k, v in _exact.items()}


def _exact_buffers(x, Ch: int, pool: bool, symbol, *dims):
    """What the three exact entry points write: y, the saved statistics [2,Ch] (mean, invstd) and the workspace."""
    return _empty_y(x, Ch, pool), torch.empty((2, Ch), device=x.device, dtype=torch.float32), _workspace(x.device, symbol, *dims)


def _bn_exact_call(x, gamma, beta, running_mean, running_var, momentum, eps, y, save, ws, pool, stream):
    B, Ch, H, W = x.shape
    return _lib.bind("coattn_bn_exact_forward", x=x, gamma=gamma, beta=beta, running_mean=running_mean, running_var=running_var,
                     momentum=float(momentum), eps=float(eps), y=y, save_mean=save[0], save_invstd=save[1], ws=ws, B=B, H=H, W=W,
                     C=Ch, pool=int(pool), relu=1, dtype=_lib.F32, stream=stream)


def _bn_exact_raw(x, weight, bias, running_mean, running_var, momentum, eps, pool: bool):
    B, Ch, H, W = x.shape
    y, save, ws = _exact_buffers(x, Ch, pool, "coattn_bn_exact_workspace_bytes", B, H, W, Ch)
    with torch.no_grad(), _lib.on_device(x.device):
        _bn_exact_call(x, weight, bias, running_mean, running_var, momentum, eps, y, save, ws, pool, _lib.stream_ptr(x.device))()
    return y, save[0], save[1]


def bn_exact(x: torch.Tensor, bn: nn.BatchNorm2d, pool: bool = False, conv=None, recompute=None) -> torch.Tensor:
    """relu(max_pool2d(bn(x), 2, 2)) (pool) or relu(bn(x)) of a channels_last fp32 [B,C,H,W] tensor with `bn` in train mode, summed
    in MIOpen's order: the stock chain's bits, `bn`'s running statistics and num_batches_tracked included (a convolution bias left
    out of x is the caller's to add to the running mean).  With `conv`, the encoder's first convolution, x is ITS input, a
    channels_last [B,3,H,W] image: conv2d(x, conv.weight, padding=1) without the bias is computed in the stock kernel's arithmetic
    by the kernel that sums the statistics (coattn_conv1_bn_recompute_forward, or coattn_conv1_bn_exact_forward with
    `recompute` False; None: conv1_recompute_enabled()).  Forward only; runs on torch's current stream."""
    if conv is not None:
        if not conv1_inputs_fusable(x, conv, bn, pool):
            raise ValueError("bn_exact: with conv it needs a CUDA fp32 channels_last [B,3,H,W] image, a 3 -> 64 channel 3x3 / stride 1 "
                             "/ padding 1 convolution with channels_last weights and a shape coattn_conv1_bn_exact_supported "
                             "covers, got %s %s strides %s" % (tuple(x.shape), x.dtype, x.stride()))
        _, y, _, _ = _conv1_raw(x, conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, pool, False,
                                recompute)
    else:
        if not exact_output_fusable(x, bn, pool):
            raise ValueError("bn_exact: needs a CUDA fp32 channels_last [B,C,H,W] tensor of a shape coattn_bn_exact_geometry "
                             "covers, got %s %s strides %s" % (tuple(x.shape), x.dtype, x.stride()))
        y, _, _ = _bn_exact_raw(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, pool)
    if bn.num_batches_tracked is not None:
        with torch.no_grad():
            bn.num_batches_tracked.add_(1)
    return y


def _stock_chain(x: torch.Tensor, bn: nn.BatchNorm2d, pool) -> torch.Tensor:
    """What the default route ran before there was bn_exact: the stock BatchNorm, then relu_pool or the stock ReLU."""
    z = bn(x)
    if pool is None:
        return torch.relu_(z)
    return relu_pool(z) if relu_pool_fusable(pool, z) else torch.relu_(pool(z))


def _differs(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """A 0-d bool tensor: some element of a is not b's (torch.equal with NaNs in the same places), without a host read."""
    return ~((a == b) | (a.isnan() & b.isnan())).all()


def _verify(x: torch.Tensor, bn: nn.BatchNorm2d, pool, key) -> torch.Tensor:
    """The first call of a shape: the stock chain's result, and beside it bn_exact on clones of the running statistics,
    compared bit for bit.  One host synchronisation."""
    with torch.no_grad():
        rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
        y = _stock_chain(x, bn, pool)
        _, save_mean, save_invstd = torch.miopen_batch_norm(x, bn.weight, bn.bias, rm0.clone(), rv0.clone(), True,
                                                            bn.momentum, bn.eps)
        mine_y, mine_mean, mine_invstd = _bn_exact_raw(x, bn.weight, bn.bias, rm0, rv0, bn.momentum, bn.eps, pool is not None)
        names = ("y", "running_mean", "running_var", "save_mean", "save_invstd")
        pairs = ((mine_y, y), (rm0, bn.running_mean), (rv0, bn.running_var), (mine_mean, save_mean), (mine_invstd, save_invstd))
        flags = torch.stack([_differs(a, b) for a, b in pairs]).tolist()
    first = next((n for n, f in zip(names, flags) if f), None)
    B, Ch, H, W = x.shape
    _exact[key] = {"verified": first is None, "first_difference": first, "geometry": exact_geometry(B, H, W, Ch)}
    if first is not None:
        warnings.warn("encoder: bn_exact does not reproduce the stock BatchNorm for B=%d C=%d H=%d W=%d pool=%d (%s differs); "
                      "this shape stays on the stock kernels" % (B, Ch, H, W, int(pool is not None), first))
    return y


def bn_exact_or_stock(x: torch.Tensor, bn: nn.BatchNorm2d, pool, conv=None) -> torch.Tensor:
    """relu([max_pool2d](bn(x))) with the stock chain's bits, `pool` a 2x2 MaxPool2d or None: through bn_exact for a shape that
    was compared with the stock chain once in this process and found equal, through the stock chain otherwise -- the first
    time a (device, B, C, H, W, pool) is seen (the comparison itself; not while the stream is capturing, where nothing is
    compared or remembered) and for good after a difference, which is reported once.  With `conv`, x is the input of the
    encoder's first convolution and the convolution is part of the contract: conv1_bn_exact_or_stock."""
    if conv is not None:
        return _conv1_or_stock(x, conv, bn, pool)
    return _bn_or_stock(x, bn, pool)


def _bn_or_stock(x: torch.Tensor, bn: nn.BatchNorm2d, pool) -> torch.Tensor:
    B, Ch, H, W = x.shape
    key = (x.device.index if x.device.index is not None else torch.cuda.current_device(), B, Ch, H, W, pool is not None)
    state = _exact.get(key)
    if state is None:
        if torch.cuda.is_current_stream_capturing():
            return _stock_chain(x, bn, pool)
        return _verify(x, bn, pool, key)
    return bn_exact(x, bn, pool is not None) if state["verified"] else _stock_chain(x, bn, pool)


# ---- the first convolution with its statistics riding along: verified per shape, or not used ------------------------------
def conv1_enabled() -> bool:
    """Where bn_exact is the default, unless VQA_ENCODER_EXACT_CONV1=0."""
    return exact_enabled() and os.environ.get("VQA_ENCODER_EXACT_CONV1", "1") != "0"


def conv1_inputs_fusable(x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, pool: bool) -> bool:
    """A CUDA fp32 channels_last [B,3,H,W] image, a 3 -> 64 channel 3x3 convolution of stride 1, zero padding 1, no dilation and
    no groups whose fp32 weights are channels_last too (the stock call then answers channels_last, and gemm-k runs (ky, kx, c)
    through memory), BatchNorm2d's parameters and buffers in fp32 and 16-byte aligned, a shape the library covers."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)):
        return False
    if not (conv.in_channels == 3 and conv.out_channels == 64 and _pair(conv.kernel_size) == (3, 3) and _pair(conv.stride) == (1, 1)
            and not isinstance(conv.padding, str) and _pair(conv.padding) == (1, 1) and _pair(conv.dilation) == (1, 1)
            and conv.groups == 1 and conv.padding_mode == "zeros" and x.shape[1] == 3):
        return False
    w = conv.weight
    if not (w.dtype == torch.float32 and w.device == x.device and w.is_contiguous(memory_format=torch.channels_last)):
        return False
    for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
        if t is None or t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous() or t.data_ptr() % 16 != 0:
            return False
    if bn.num_features != 64 or x.data_ptr() % 4 != 0 or w.data_ptr() % 4 != 0:
        return False
    B, _, H, W = x.shape
    return bool(_lib.load().coattn_conv1_bn_exact_supported(B, H, W, 3, 64, int(pool), _lib.F32))


def conv1_modules_fusable(conv: nn.Conv2d, bn: nn.BatchNorm2d, pool, x: torch.Tensor) -> bool:
    """exact_modules_fusable's conditions, VQA_ENCODER_EXACT_CONV1, and conv1_inputs_fusable."""
    return (conv1_enabled() and not torch.is_autocast_enabled() and _group_fusable(conv, bn, pool, x)
            and conv1_inputs_fusable(x, conv, bn, pool is not None))


def conv1_recompute_enabled() -> bool:
    """The first group computes its convolution twice and never stores it, unless VQA_ENCODER_CONV1_RECOMPUTE=0."""
    return os.environ.get("VQA_ENCODER_CONV1_RECOMPUTE", "1") != "0"


def _conv1_call(image, weight, gamma, beta, running_mean, running_var, momentum, eps, y, save, ws, pool, stream, **x_out):
    """The first group's call: given x_out (a tensor, or None: x is kept in ws) the form that stores the convolution output,
    coattn_conv1_bn_exact_forward; without it coattn_conv1_bn_recompute_forward."""
    B, _, H, W = image.shape
    return _lib.bind("coattn_conv1_bn_exact_forward" if x_out else "coattn_conv1_bn_recompute_forward", image=image, weight=weight,
                     gamma=gamma, beta=beta, running_mean=running_mean, running_var=running_var, momentum=float(momentum),
                     eps=float(eps), y=y, save_mean=save[0], save_invstd=save[1], ws=ws, B=B, H=H, W=W, Cin=3, Cout=64,
                     pool=int(pool), dtype=_lib.F32, stream=stream, **x_out)


def _conv1_recompute_raw(image, weight, gamma, beta, running_mean, running_var, momentum, eps, pool: bool):
    """(y, save_mean, save_invstd) of coattn_conv1_bn_recompute_forward: the convolution output is never stored."""
    B, _, H, W = image.shape
    y, save, ws = _exact_buffers(image, 64, pool, "coattn_conv1_bn_recompute_workspace_bytes", B, H, W)
    with torch.no_grad(), _lib.on_device(image.device):
        _conv1_call(image, weight, gamma, beta, running_mean, running_var, momentum, eps, y, save, ws, pool,
                    _lib.stream_ptr(image.device))()
    return y, save[0], save[1]


def _conv1_raw(image, weight, gamma, beta, running_mean, running_var, momentum, eps, pool: bool, want_x: bool, recompute=None):
    """(x, y, save_mean, save_invstd) of the first group.  `want_x`: the form that stores the convolution output, which is
    returned; otherwise x is None and the recompute form runs (`recompute` False, or None and VQA_ENCODER_CONV1_RECOMPUTE=0:
    the stored form with x in its workspace)."""
    if not want_x and (conv1_recompute_enabled() if recompute is None else recompute):
        return (None,) + _conv1_recompute_raw(image, weight, gamma, beta, running_mean, running_var, momentum, eps, pool)
    B, _, H, W = image.shape
    y, save, ws = _exact_buffers(image, 64, pool, "coattn_conv1_bn_exact_workspace_bytes", B, H, W, int(not want_x))
    x = _empty_y(image, 64, False) if want_x else None
    with torch.no_grad(), _lib.on_device(image.device):
        _conv1_call(image, weight, gamma, beta, running_mean, running_var, momentum, eps, y, save, ws, pool,
                    _lib.stream_ptr(image.device), x_out=x)()
    return x, y, save[0], save[1]


def _conv1_stock(x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, pool) -> torch.Tensor:
    """What the group ran before there was this route: the stock convolution without its bias, then bn_exact_or_stock's contract
    (or the stock chain, should the convolution answer in another layout)."""
    z = torch.nn.functional.conv2d(x, conv.weight, None, conv.stride, conv.padding, conv.dilation, conv.groups)
    return _bn_or_stock(z, bn, pool) if exact_output_fusable(z, bn, pool is not None) else _stock_chain(z, bn, pool)


def _verify_conv1(x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, pool, key) -> torch.Tensor:
    """The first call of a shape: the stock group's result, and beside it the one-pass route on clones of the running
    statistics, compared bit for bit.  One host synchronisation (and the BatchNorm comparison's, if this is its first call too).
    Where the stored form matched and the recompute form is enabled, that form runs once too, on further clones, and its y and
    statistics are compared (a second synchronisation): what the route runs afterwards is what was compared."""
    with torch.no_grad():
        rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
        rm1, rv1 = rm0.clone(), rv0.clone()                             # (for the recompute form, below)
        z = torch.nn.functional.conv2d(x, conv.weight, None, conv.stride, conv.padding, conv.dilation, conv.groups)
        if not exact_output_fusable(z, bn, pool is not None):
            return _stock_chain(z, bn, pool)                        # (another layout: nothing compared, nothing remembered)
        y = _bn_or_stock(z, bn, pool)
        _, save_mean, save_invstd = torch.miopen_batch_norm(z, bn.weight, bn.bias, rm0.clone(), rv0.clone(), True,
                                                            bn.momentum, bn.eps)
        mine_x, mine_y, mine_mean, mine_invstd = _conv1_raw(x, conv.weight, bn.weight, bn.bias, rm0, rv0, bn.momentum, bn.eps,
                                                            pool is not None, True)
        names = ("x", "y", "running_mean", "running_var", "save_mean", "save_invstd")
        pairs = ((mine_x, z), (mine_y, y), (rm0, bn.running_mean), (rv0, bn.running_var), (mine_mean, save_mean),
                 (mine_invstd, save_invstd))
        flags = torch.stack([_differs(a, b) for a, b in pairs]).tolist()
        first = next((n for n, f in zip(names, flags) if f), None)
        del mine_x
        again = None
        if first is None and conv1_recompute_enabled():
            re_y, re_mean, re_invstd = _conv1_recompute_raw(x, conv.weight, bn.weight, bn.bias, rm1, rv1, bn.momentum, bn.eps,
                                                            pool is not None)
            pairs = ((re_y, y), (rm1, bn.running_mean), (rv1, bn.running_var), (re_mean, save_mean), (re_invstd, save_invstd))
            flags = torch.stack([_differs(a, b) for a, b in pairs]).tolist()
            again = next((n for n, f in zip(names[1:], flags) if f), None)
    B, _, H, W = x.shape
    entry = _exact.setdefault(key, {"verified": False, "first_difference": None, "geometry": exact_geometry(B, H, W, 64)})
    entry["conv1"] = {"verified": first is None, "first_difference": first}
    if first is None and conv1_recompute_enabled():
        entry["conv1_recompute"] = {"verified": again is None, "first_difference": again}
    else:
        entry.pop("conv1_recompute", None)
    if first is not None:
        warnings.warn("encoder: the one-pass first convolution does not reproduce the stock kernels for B=%d H=%d W=%d pool=%d "
                      "(%s differs); this shape stays on the stock kernels" % (B, H, W, int(pool is not None), first))
    elif again is not None:
        warnings.warn("encoder: the recomputed first convolution does not reproduce the stock kernels for B=%d H=%d W=%d pool=%d "
                      "(%s differs); this shape keeps the form that stores the convolution output"
                      % (B, H, W, int(pool is not None), again))
    return y


def _conv1_or_stock(x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, pool) -> torch.Tensor:
    B, _, H, W = x.shape
    key = (x.device.index if x.device.index is not None else torch.cuda.current_device(), B, 64, H, W, pool is not None)
    state = (_exact.get(key) or {}).get("conv1")
    if state is None:
        if torch.cuda.is_current_stream_capturing():
            return _conv1_stock(x, conv, bn, pool)
        return _verify_conv1(x, conv, bn, pool, key)
    if not state["verified"]:
        return _conv1_stock(x, conv, bn, pool)
    recompute = conv1_recompute_enabled()
    if recompute:
        again = _exact[key].get("conv1_recompute")
        if again is None:                                               # (verified while VQA_ENCODER_CONV1_RECOMPUTE was 0)
            if not torch.cuda.is_current_stream_capturing():
                return _verify_conv1(x, conv, bn, pool, key)
            recompute = False
        else:
            recompute = again["verified"]
    return bn_exact(x, bn, pool is not None, conv=conv, recompute=recompute)


def conv1_bn_exact_or_stock(x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, pool) -> torch.Tensor:
    """relu([max_pool2d](bn(conv2d(x)))) of the encoder's first group, the convolution without its bias, with the stock kernels'
    bits; bn_exact_or_stock's contract with the convolution inside it: through the one-pass route (bn_exact with conv) for a
    (device, B, H, W, pool) that was compared with the stock convolution and chain once in this process and found equal -- the
    convolution output, y, both running statistics and both saved statistics, element for element, NaNs in place --, through
    the stock kernels the first time (the comparison itself; not while the stream is capturing) and for good after a
    difference, which is reported once.  The caller has checked conv1_modules_fusable."""
    return bn_exact_or_stock(x, bn, pool, conv=conv)


# ---- eval mode: BatchNorm on running statistics, the bias, the ReLU and the pool in one launch; verified per shape, or not used ----
EVAL_IMPLS = ("stock", "hip")
# (device index, B, C, H, W, pool, Cin) of a group's convolution output and input channels -> {"verified", "first_difference",
# "bias": "kernel" / "convolution" / None}, and for the first group also "conv1": {"verified", "first_difference"}
_eval = {}


def eval_report() -> dict:
    """{(device index, B, C, H, W, pool, Cin): {"verified", "first_difference", "bias"}} of every eval-mode group compared so far
    under eval_impl "hip".  "bias" says where the convolution's bias is added on the verified route: "kernel" (the convolution is
    issued without it), "convolution" (the stock convolution keeps it) or None (there is none).  The entry of a first group holds
    "conv1": {"verified", "first_difference"} too, once conv1_bn_eval_or_stock has compared the one-launch form."""
    return {k: {n: dict(t) if n == "conv1" else t for n, t in v.items()} for k, v in _eval.items()}


def eval_group_fusable(conv: nn.Conv2d, bn: nn.BatchNorm2d, pool, x: torch.Tensor) -> bool:
    """_group_fusable's conditions with eval mode in place of train mode (running statistics to normalise with; no momentum is
    needed, nothing moves), and no autocast."""
    if not x.is_cuda or torch.is_autocast_enabled():
        return False
    if bn.training or not bn.affine or bn.running_mean is None or bn.running_var is None:
        return False
    params = (conv.weight, conv.bias, bn.weight, bn.bias)
    if torch.is_grad_enabled() and (x.requires_grad or any(p is not None and p.requires_grad for p in params)):
        return False
    if conv.padding_mode != "zeros":
        return False
    b = conv.bias
    if b is not None and (b.requires_grad or b.dtype != torch.float32 or b.device != x.device or not b.is_contiguous()
                          or b.data_ptr() % 16 != 0):
        return False
    return pool is None or pool_is_2x2(pool)


def eval_output_fusable(z: torch.Tensor, bn: nn.BatchNorm2d, pool: bool) -> bool:
    """output_fusable (whose shape rule is coattn_bn_eval_supported's) and 16-byte aligned tensors throughout.  No MIOpen
    geometry: nothing is summed."""
    return output_fusable(z, bn, pool) and all(t.data_ptr() % 16 == 0 for t in (z, bn.weight, bn.bias, bn.running_mean, bn.running_var))


def _bn_eval_raw(x, conv_bias, gamma, beta, running_mean, running_var, eps, pool: bool, relu: bool = True):
    B, Ch, H, W = x.shape
    y = _empty_y(x, Ch, pool)
    with torch.no_grad(), _lib.on_device(x.device):
        _lib.bind("coattn_bn_eval_forward", x=x, conv_bias=conv_bias, gamma=gamma, beta=beta, running_mean=running_mean,
                  running_var=running_var, eps=float(eps), y=y, B=B, H=H, W=W, C=Ch, pool=int(pool), relu=int(relu), dtype=_lib.F32,
                  stream=_lib.stream_ptr(x.device))()
    return y


def bn_eval(x: torch.Tensor, bn: nn.BatchNorm2d, conv_bias=None, pool: bool = False) -> torch.Tensor:
    """relu(max_pool2d(bn(x + conv_bias), 2, 2)) (pool) or relu(bn(x + conv_bias)) of a channels_last fp32 [B,C,H,W] tensor with `bn`
    in EVAL mode, in one launch and in the stock inference kernel's arithmetic (include/coattn_ext.h v0.24.0), as a channels_last
    tensor.  `conv_bias`: the fp32 [C] bias of the convolution that produced x WITHOUT it, or None.  `bn`'s buffers are read only.
    Forward only; runs on torch's current stream."""
    Ch = x.shape[1] if x.dim() == 4 else -1
    if conv_bias is not None and not (conv_bias.dtype == torch.float32 and conv_bias.device == x.device and conv_bias.is_contiguous()
                                      and tuple(conv_bias.shape) == (Ch,) and conv_bias.data_ptr() % 16 == 0):
        raise ValueError("bn_eval: conv_bias must be a contiguous 16-byte aligned fp32 [C] tensor on x's device")
    if bn.training or bn.running_mean is None or bn.running_var is None or not bn.affine:
        raise ValueError("bn_eval: needs an affine BatchNorm2d in eval mode with running statistics")
    if not eval_output_fusable(x, bn, pool):
        raise ValueError("bn_eval: needs a CUDA fp32 channels_last [B,C,H,W] tensor of a shape coattn_bn_eval_supported takes and "
                         "16-byte aligned tensors, got %s %s strides %s" % (tuple(x.shape), x.dtype, x.stride()))
    return _bn_eval_raw(x, conv_bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, pool)


def conv1_eval_inputs_fusable(x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, pool: bool) -> bool:
    """conv1_inputs_fusable with coattn_conv1_bn_eval_supported's shape rule in place of the exact route's."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)):
        return False
    if not (conv.in_channels == 3 and conv.out_channels == 64 and _pair(conv.kernel_size) == (3, 3) and _pair(conv.stride) == (1, 1)
            and not isinstance(conv.padding, str) and _pair(conv.padding) == (1, 1) and _pair(conv.dilation) == (1, 1)
            and conv.groups == 1 and conv.padding_mode == "zeros" and x.shape[1] == 3):
        return False
    w = conv.weight
    if not (w.dtype == torch.float32 and w.device == x.device and w.is_contiguous(memory_format=torch.channels_last)):
        return False
    for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
        if t is None or t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous() or t.data_ptr() % 16 != 0:
            return False
    if bn.num_features != 64 or x.data_ptr() % 4 != 0 or w.data_ptr() % 4 != 0:
        return False
    B, _, H, W = x.shape
    return bool(_lib.load().coattn_conv1_bn_eval_supported(B, H, W, 3, 64, int(pool), _lib.F32))


def _conv1_eval_raw(image, weight, conv_bias, gamma, beta, running_mean, running_var, eps, pool: bool):
    B, _, H, W = image.shape
    y = _empty_y(image, 64, pool)
    with torch.no_grad(), _lib.on_device(image.device):
        _lib.bind("coattn_conv1_bn_eval_forward", image=image, weight=weight, conv_bias=conv_bias, gamma=gamma, beta=beta,
                  running_mean=running_mean, running_var=running_var, eps=float(eps), y=y, B=B, H=H, W=W, Cin=3, Cout=64,
                  pool=int(pool), dtype=_lib.F32, stream=_lib.stream_ptr(image.device))()
    return y


def conv1_bn_eval(image: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, pool: bool) -> torch.Tensor:
    """relu([max_pool2d](bn(conv(image)))) of the encoder's first group with `bn` in EVAL mode, from the channels_last [B,3,H,W]
    image to the result in ONE launch: the convolution in the stock kernel's arithmetic, its bias, then bn_eval's map.  The
    convolution output is never stored and there is no workspace.  Forward only; runs on torch's current stream."""
    if bn.training or not bn.affine or not conv1_eval_inputs_fusable(image, conv, bn, pool):
        raise ValueError("conv1_bn_eval: needs a CUDA fp32 channels_last [B,3,H,W] image, a 3 -> 64 channel 3x3 / stride 1 / padding 1 "
                         "convolution with channels_last weights, an affine BatchNorm2d in eval mode and a shape "
                         "coattn_conv1_bn_eval_supported covers, got %s %s strides %s" % (tuple(image.shape), image.dtype, image.stride()))
    b = conv.bias
    if b is not None and not (b.dtype == torch.float32 and b.device == image.device and b.is_contiguous() and b.data_ptr() % 16 == 0):
        raise ValueError("conv1_bn_eval: the convolution's bias must be a contiguous 16-byte aligned fp32 tensor on the image's device")
    return _conv1_eval_raw(image, conv.weight, b, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, pool)


def _conv(x, conv: nn.Conv2d, bias):
    return torch.nn.functional.conv2d(x, conv.weight, bias, conv.stride, conv.padding, conv.dilation, conv.groups)


def _eval_stock(x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, pool) -> torch.Tensor:
    """What an eval-mode group runs under eval_impl "stock": the convolution with its bias, then the stock chain."""
    return _stock_chain(conv(x), bn, pool)


def _eval_key(x, conv, z_shape, pool):
    dev = x.device.index if x.device.index is not None else torch.cuda.current_device()
    return (dev, z_shape[0], z_shape[1], z_shape[2], z_shape[3], pool is not None, conv.in_channels)


def _conv_out_shape(x, conv: nn.Conv2d):
    """The [B,C,H,W] of conv(x), without running it."""
    if isinstance(conv.padding, str):
        return None
    hw = []
    for n, k, s, p, d in zip(x.shape[2:], _pair(conv.kernel_size), _pair(conv.stride), _pair(conv.padding), _pair(conv.dilation)):
        hw.append((n + 2 * p - d * (k - 1) - 1) // s + 1)
    return (x.shape[0], conv.out_channels, hw[0], hw[1])


def _verify_eval(x, conv, bn, pool, key) -> torch.Tensor:
    """The first call of a shape: the stock group's result, and beside it bn_eval, compared bit for bit; the bias goes into the
    kernel only where, under deterministic solvers, the convolution without it plus an exact add gave the stock convolution's
    bits.  One host synchronisation."""
    with torch.no_grad():
        z = conv(x)
        if not eval_output_fusable(z, bn, pool is not None):
            return _stock_chain(z, bn, pool)                        # (another layout: nothing compared, nothing remembered)
        b, flags, z0 = conv.bias, [], None
        if b is not None and torch.backends.cudnn.deterministic:
            z0 = _conv(x, conv, None)
            if eval_output_fusable(z0, bn, pool is not None):
                flags.append(_differs(z0 + b.view(1, -1, 1, 1), z))
            else:
                z0 = None
        y = _stock_chain(z, bn, pool)                               # (eval-mode bn(z) writes a new tensor: z stays)
        mine_z = _bn_eval_raw(z, None, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, pool is not None)
        flags.append(_differs(mine_z, y))
        if z0 is not None:
            mine_b = _bn_eval_raw(z0, b, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, pool is not None)
            flags.append(_differs(mine_b, y))
        flags = torch.stack(flags).tolist()
    in_kernel = z0 is not None and not flags[0] and not flags[2]
    first = "y" if flags[1 if z0 is not None else 0] else None
    _eval[key] = {"verified": first is None, "first_difference": first,
                  "bias": None if b is None else "kernel" if in_kernel else "convolution"}
    if first is not None:
        warnings.warn("encoder: bn_eval does not reproduce the stock eval-mode BatchNorm for B=%d C=%d H=%d W=%d pool=%d (%s differs); "
                      "this shape stays on the stock kernels" % (key[1:5] + (int(key[5]), first)))
    return y


def bn_eval_or_stock(x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, pool) -> torch.Tensor:
    """relu([max_pool2d](bn(conv(x)))) of an eval-mode group, `pool` a 2x2 MaxPool2d or None, with the stock kernels' bits: the stock
    convolution, then bn_eval, for a (device, B, C, H, W, pool, Cin) whose first call in this process -- which runs the stock chain
    and returns its result -- found the two equal in every bit; the stock chain for good after a difference, which is reported once.
    Nothing is compared or remembered while the stream is capturing.  The convolution is issued without its bias, which the
    kernel adds, only where that first call ran under torch.backends.cudnn.deterministic and also found
    conv2d(x, w, None) + b equal to conv2d(x, w, b) in every bit (eval_report()'s "bias").  The caller has checked
    eval_group_fusable."""
    shape = _conv_out_shape(x, conv)
    if shape is None:
        return _eval_stock(x, conv, bn, pool)
    key = _eval_key(x, conv, shape, pool)
    state = _eval.get(key)
    if state is None:
        if torch.cuda.is_current_stream_capturing():
            return _eval_stock(x, conv, bn, pool)
        return _verify_eval(x, conv, bn, pool, key)
    if not state["verified"]:
        return _eval_stock(x, conv, bn, pool)
    in_kernel = state["bias"] == "kernel"
    z = _conv(x, conv, None if in_kernel else conv.bias)
    if not eval_output_fusable(z, bn, pool is not None):            # (never seen: the first call had the same layout)
        if in_kernel:
            z = z + conv.bias.view(1, -1, 1, 1)
        return _stock_chain(z, bn, pool)
    return bn_eval(z, bn, conv_bias=conv.bias if in_kernel else None, pool=pool is not None)


def conv1_bn_eval_or_stock(x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, pool) -> torch.Tensor:
    """bn_eval_or_stock for the encoder's first group with the convolution inside the contract: conv1_bn_eval, one launch from the
    image, for a shape whose first call found it equal in every bit to the stock convolution and chain; otherwise
    bn_eval_or_stock, which has a verdict of its own.  The caller has checked eval_group_fusable and conv1_eval_inputs_fusable."""
    B, _, H, W = x.shape
    key = _eval_key(x, conv, (B, 64, H, W), pool)
    state = (_eval.get(key) or {}).get("conv1")
    if state is not None and state["verified"]:
        return conv1_bn_eval(x, conv, bn, pool is not None)
    y = bn_eval_or_stock(x, conv, bn, pool)
    if state is not None or torch.cuda.is_current_stream_capturing() or key not in _eval:
        return y
    with torch.no_grad():
        mine = _conv1_eval_raw(x, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, pool is not None)
        differs = bool(_differs(mine, y))
    _eval[key]["conv1"] = {"verified": not differs, "first_difference": "y" if differs else None}
    if differs:
        warnings.warn("encoder: the one-launch eval-mode first group does not reproduce the stock kernels for B=%d H=%d W=%d pool=%d "
                      "(y differs); this shape keeps the stock convolution" % (B, H, W, int(pool is not None)))
    return y

"""``HipAdam``: the optimiser step of the train loop (reference main.py:180, :222: ``torch.optim.Adam``) through the C-ABI of
``include/coattn.h`` (``csrc/adam.hip``): one launch updates every parameter of a group, with decoupled weight decay (AdamW)
and gradient clipping by global norm (``torch.nn.utils.clip_grad_norm_``) in the same call.  There is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib


class HipAdam(torch.optim.Optimizer):
    """``torch.optim.Adam``'s arithmetic on fp32 CUDA parameters, one ``coattn_adam_step`` call per param group on the current
    stream.

    weight_decay  decoupled (``torch.optim.AdamW``: p *= 1 - lr * weight_decay ahead of the update).
    max_grad_norm ``None`` / <= 0: no clipping.  Otherwise the gradients of the GROUP are scaled by
                  min(1, max_grad_norm / (norm + 1e-6)) inside the update -- ``.grad`` itself is not written -- and the norm
                  stays on the device as ``self.grad_norm`` (a 0-dim fp32 tensor that the next step overwrites; the host
                  never reads it here).  The norm is that of one call: a model whose parameters are spread over several groups
                  is clipped group by group.

    The per-parameter state is ``step`` (a CPU fp32 scalar, as the stock optimiser keeps it), ``exp_avg`` and ``exp_avg_sq``,
    and the groups carry every key of ``torch.optim.Adam``'s (with ``decoupled_weight_decay=True``): a ``state_dict()`` of either
    optimiser loads into the other, and ``param_groups[i]["lr"]`` is read at every step, so the ``torch.optim.lr_scheduler``
    classes drive it.  Parameters whose ``.grad`` is ``None`` are left alone (no state, no step).
    Raises on CPU, non-fp32 or non-contiguous parameters, sparse gradients, ``amsgrad``, ``maximize`` and under stream capture
    (the step number is a host value of the call); a non-contiguous gradient is made contiguous."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 amsgrad=False, maximize=False):
        if isinstance(lr, torch.Tensor) or not 0.0 <= lr:
            raise ValueError("HipAdam: lr must be a non-negative float, got %r" % (lr,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("HipAdam: betas must lie in [0, 1), got %r" % (betas,))
        if not 0.0 <= eps:
            raise ValueError("HipAdam: eps must be non-negative, got %r" % (eps,))
        if not 0.0 <= weight_decay:
            raise ValueError("HipAdam: weight_decay must be non-negative, got %r" % (weight_decay,))
        if amsgrad or maximize:
            raise ValueError("HipAdam: amsgrad / maximize are not supported")
        defaults = dict(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).defaults)     # the stock keys, for state_dict exchange
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, decoupled_weight_decay=True,
                        max_grad_norm=max_grad_norm)
        self._max_grad_norm = max_grad_norm
        super().__init__(params, defaults)
        self.grad_norm = None                 # device scalar: the global gradient norm of the last clipped step
        self._norm_out = {}                   # device index -> the tensor behind grad_norm

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:       # groups saved by torch.optim.Adam know nothing of clipping: keep this optimiser's
            group.setdefault("max_grad_norm", self._max_grad_norm)

    @torch.no_grad()
    def step(self, closure=None):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("HipAdam.step cannot be captured into a graph: the step number is a host value of the call")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            self._step_group(group)
        return loss

    def _step_group(self, group):
        if group.get("amsgrad") or group.get("maximize"):
            raise RuntimeError("HipAdam: amsgrad / maximize are not supported")
        wd = float(group["weight_decay"])
        if wd != 0.0 and not group.get("decoupled_weight_decay", True):
            raise RuntimeError("HipAdam: weight decay is decoupled (AdamW); this group asks for torch.optim.Adam's L2 form")
        beta1, beta2 = group["betas"]
        clip = group.get("max_grad_norm")
        clip = float(clip) if clip is not None and clip > 0 else 0.0
        by_step = {}                          # step number -> [(p, grad, exp_avg, exp_avg_sq)]
        dev = None
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            if not p.is_cuda:
                raise RuntimeError("HipAdam needs parameters on the GPU (there is no CPU fallback)")
            if p.dtype != torch.float32 or g.dtype != torch.float32:
                raise RuntimeError("HipAdam: fp32 parameters and gradients only, got %s / %s" % (p.dtype, g.dtype))
            if g.is_sparse:
                raise RuntimeError("HipAdam does not support sparse gradients")
            if not p.is_contiguous():
                raise RuntimeError("HipAdam: parameters must be contiguous")
            if dev is None:
                dev = p.device
            elif p.device != dev:
                raise RuntimeError("HipAdam: the parameters of one group must live on one device")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            elif st["step"].is_cuda:          # the state of a capturable / fused stock optimiser: one read, then a host value
                st["step"] = st["step"].detach().cpu()
            m, v = st["exp_avg"], st["exp_avg_sq"]
            if not (m.is_contiguous() and v.is_contiguous() and m.dtype == v.dtype == torch.float32 and m.device == v.device == dev):
                raise RuntimeError("HipAdam: exp_avg / exp_avg_sq must be contiguous fp32 tensors on the parameter's device")
            st["step"] += 1
            by_step.setdefault(int(st["step"]), []).append((p, g if g.is_contiguous() else g.contiguous(), m, v))
        if not by_step:
            return
        if clip > 0.0 and len(by_step) > 1:
            raise RuntimeError("HipAdam: the parameters of a clipped group must share one step count (the norm is taken over "
                               "one call); put parameters that joined later into a group of their own")
        stream_ptr = torch.cuda.current_stream(dev).cuda_stream
        for step, entries in by_step.items():
            arr = (_lib.AdamTensor * len(entries))()
            for e, (p, g, m, v) in zip(arr, entries):
                e.p, e.g, e.m, e.v, e.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
            ws = norm = None
            nbytes = 0
            if clip > 0.0:
                nbytes = _lib.size_bytes("coattn_adam_workspace_bytes", arr, len(entries))
                if nbytes == 0:
                    _lib.check(-1, "coattn_adam_workspace_bytes")
                ws = _lib.scratch(nbytes, dev, stream_ptr)
                norm = self._norm_out.get(dev.index)
                if norm is None:
                    norm = self._norm_out[dev.index] = torch.zeros((), device=dev, dtype=torch.float32)
                self.grad_norm = norm
            with _lib.on_device(dev):
                _step_call(arr, step, float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), wd, clip, norm, ws,
                           nbytes, stream_ptr)()


def _step_call(arr, step, lr, beta1, beta2, eps, weight_decay, max_grad_norm, norm_out, ws, ws_bytes, stream):
    return _lib.bind("coattn_adam_step", t=arr, n_tensors=len(arr), step=step, lr=lr, beta1=beta1, beta2=beta2, eps=eps,
                     weight_decay=weight_decay, max_grad_norm=max_grad_norm, norm_out=norm_out, ws=ws, ws_bytes=ws_bytes,
                     stream=stream)

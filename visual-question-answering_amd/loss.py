"""``cross_entropy`` / ``CrossEntropyLoss``: the ``nn.CrossEntropyLoss()`` of the train step (reference main.py:94,
:214; mean over the batch) through the C-ABI of ``include/coattn.h`` (``csrc/ce.hip``) on the caller's current
stream: loss and d loss / d logits in one pass.  SURVEY.md section 8f-1.  The ``MLPClassifier`` that produces the
logits (model.py:400-434) is the stock module of ``modules.py``.
"""
from __future__ import annotations

import torch

from . import _lib


_last = None          # (ws, B, device) of the last call: check_labels() reads its status word


def _ce_call(logits, labels, loss, dlogits, ws, stream):
    B, K = logits.shape
    return _lib.bind("coattn_ce_forward", logits=logits, labels=labels, loss=loss, dlogits=dlogits, ws=ws, B=B, K=K,
                     dtype=_lib.F32, stream=stream)


def _soft_loss_call(logits, ans_idx, ans_score, kind, loss, dlogits, ws, stream):
    B, K = logits.shape
    return _lib.bind("coattn_soft_loss_forward", logits=logits, ans_idx=ans_idx, ans_score=ans_score, A=ans_idx.shape[1],
                     kind=kind, loss=loss, dlogits=dlogits, ws=ws, B=B, K=K, dtype=_lib.F32, stream=stream)


def _score_call(logits, ans_idx, ans_score, pred, row_score, score_sum, ws, stream):
    B, K = logits.shape
    return _lib.bind("coattn_vqa_score", logits=logits, ans_idx=ans_idx, ans_score=ans_score, A=ans_idx.shape[1], pred=pred,
                     row_score=row_score, score_sum=score_sum, ws=ws, B=B, K=K, dtype=_lib.F32, stream=stream)


class _CrossEntropyFn(torch.autograd.Function):
    """Mean cross entropy; the forward pass also produces d loss / d logits."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, logits, labels):
        if not logits.is_cuda:
            raise RuntimeError("cross_entropy (HIP) needs tensors on the GPU")
        if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0] or labels.dtype != torch.int64:
            raise RuntimeError("cross_entropy: logits [B,K] fp32 and labels [B] int64 expected")
        B, K = logits.shape
        z = logits.contiguous()
        lab = labels.contiguous()
        dev = z.device
        ws = torch.empty(_lib.ce_workspace_bytes(B, K) // 4, device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        need = ctx.needs_input_grad[0]
        dz = torch.empty_like(z) if need else None
        with _lib.on_device(dev):
            _ce_call(z, lab, loss, dz, ws, _lib.stream_ptr(dev))()
        global _last
        _last = (ws, B, dev)
        if need:
            ctx.save_for_backward(dz)
        return loss

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        (dz,) = ctx.saved_tensors
        return dz * g, None


def check_labels() -> None:
    """``nn.CrossEntropyLoss`` raises on a label outside [0, K); the HIP kernel stays asynchronous, returns NaN and sets
    a status word instead.  This SYNCHRONISES the current stream and raises IndexError if the last ``cross_entropy``
    call met such a label -- call it where the host synchronises anyway (when the loss is read).  The soft-target calls
    (``soft_target_loss``, ``vqa_score``) report an answer index outside [-1, K) through the same word."""
    if _last is None:
        return
    ws, B, dev = _last
    with _lib.on_device(dev):
        _lib.check_label_status(_lib.bind("coattn_ce_status", ws=ws, B=B, stream=_lib.stream_ptr(dev)))


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """``nn.CrossEntropyLoss()(logits, labels)`` (mean reduction, main.py:94/:214) on the HIP path."""
    return _CrossEntropyFn.apply(logits, labels)


class CrossEntropyLoss(torch.nn.Module):
    """Drop-in for the ``nn.CrossEntropyLoss()`` criterion of the train loop (main.py:94): CUDA fp32 logits take
    the fused HIP kernel, everything else (CPU tensors, the baseline model's CPU runs) the stock functional."""

    def forward(self, logits, labels):
        if logits.is_cuda and logits.dim() == 2 and labels.dtype == torch.int64:
            return cross_entropy(logits, labels)
        return torch.nn.functional.cross_entropy(logits, labels)


# ---- soft answer targets (include/coattn.h v0.12.0) ---------------------------------------------------------------------
LOSS_KINDS = ("soft_ce", "bce")


def _check_targets(what, logits, ans_idx, ans_score):
    if (logits.dim() != 2 or ans_idx.dim() != 2 or ans_idx.shape[0] != logits.shape[0] or ans_idx.shape != ans_score.shape
            or ans_idx.dtype != torch.int32 or ans_score.dtype != torch.float32):
        raise RuntimeError("%s: logits [B,K] fp32, ans_idx [B,A] int32 and ans_score [B,A] fp32 expected" % what)
    if not 1 <= ans_idx.shape[1] <= _lib.MAX_ANSWERS:
        raise RuntimeError("%s: %d answer slots per sample (1..%d supported)" % (what, ans_idx.shape[1], _lib.MAX_ANSWERS))


def _kind(kind: str) -> int:
    if kind not in _lib.LOSS_KINDS:
        raise ValueError("loss kind must be one of %s, got %r" % (LOSS_KINDS, kind))
    return _lib.LOSS_KINDS[kind]


def dense_targets(ans_idx: torch.Tensor, ans_score: torch.Tensor, K: int, dtype=None) -> torch.Tensor:
    """The dense target the slots stand for, t[b, k] = sum of ans_score[b, a] over the slots with ans_idx[b, a] == k (stock
    ops: the CPU fallback and host-side checks; the HIP kernels never form it)."""
    if bool(((ans_idx < -1) | (ans_idx >= K)).any()):
        raise IndexError("soft targets: an answer index is outside [-1, K)")
    live = ans_idx >= 0
    sc = torch.where(live, ans_score, torch.zeros_like(ans_score)).to(dtype or ans_score.dtype)
    t = torch.zeros((ans_idx.shape[0], K), dtype=sc.dtype, device=ans_idx.device)
    return t.scatter_add_(1, torch.where(live, ans_idx, torch.zeros_like(ans_idx)).long(), sc)


def soft_target_loss_stock(logits, ans_idx, ans_score, kind: str = "soft_ce") -> torch.Tensor:
    """The two losses of include/coattn.h on stock ops, in the logits' own dtype (CPU tensors; differentiable)."""
    _kind(kind)
    t = dense_targets(ans_idx, ans_score, logits.shape[1], logits.dtype)
    if kind == "soft_ce":
        tz = torch.where(t != 0, t * logits, torch.zeros_like(logits))      # (a class masked with -inf and no target: no term)
        rows = t.sum(1) * torch.logsumexp(logits, 1) - tz.sum(1)
    else:
        softplus = logits.clamp(min=0) + torch.log1p(torch.exp(-logits.abs()))      # (F.softplus switches to x beyond 20)
        rows = (softplus - t.clamp(max=1.0) * logits).sum(1)
    return rows.mean()


class _SoftTargetLossFn(torch.autograd.Function):
    """Mean soft-target loss; the forward pass also produces d loss / d logits (one launch)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, logits, ans_idx, ans_score, kind):
        if not logits.is_cuda:
            raise RuntimeError("soft_target_loss (HIP) needs tensors on the GPU")
        _check_targets("soft_target_loss", logits, ans_idx, ans_score)
        B, K = logits.shape
        z, ai, sc = logits.contiguous(), ans_idx.contiguous(), ans_score.contiguous()
        dev = z.device
        ws = torch.empty(_lib.ce_workspace_bytes(B, K) // 4, device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        need = ctx.needs_input_grad[0]
        dz = torch.empty_like(z) if need else None
        with _lib.on_device(dev):
            _soft_loss_call(z, ai, sc, kind, loss, dz, ws, _lib.stream_ptr(dev))()
        global _last
        _last = (ws, B, dev)
        if need:
            ctx.save_for_backward(dz)
        return loss

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, g):
        (dz,) = ctx.saved_tensors
        return dz * g, None, None, None


def soft_target_loss(logits: torch.Tensor, ans_idx: torch.Tensor, ans_score: torch.Tensor, kind: str = "soft_ce") -> torch.Tensor:
    """Mean over the batch of the soft cross entropy (``kind="soft_ce"``: S lse(z) - sum t z) or of the binary cross entropy
    with logits summed over the classes (``"bce"``, target clamped to 1) against sparse answer targets -- ans_idx int32
    [B,A] (-1 = empty slot), ans_score fp32 [B,A], A <= 16 -- on the HIP path.  An index outside [-1, K) gives NaN and an
    IndexError at ``check_labels()``."""
    return _SoftTargetLossFn.apply(logits, ans_idx, ans_score, _kind(kind))


class SoftTargetLoss(torch.nn.Module):
    """Criterion on VQA soft answer targets: CUDA fp32 logits take the HIP kernel, everything else (CPU tensors, float64) the
    stock-op formula -- the way ``CrossEntropyLoss`` falls back."""

    def __init__(self, kind: str = "soft_ce"):
        super().__init__()
        _kind(kind)
        self.kind = kind

    def forward(self, logits, ans_idx, ans_score):
        if logits.is_cuda and logits.dim() == 2 and logits.dtype == torch.float32:
            return soft_target_loss(logits, ans_idx, ans_score, self.kind)
        return soft_target_loss_stock(logits, ans_idx, ans_score.to(logits.dtype), self.kind)


def vqa_score_sum(logits, ans_idx, ans_score, row_score: bool = True):
    """(pred int32 [B], row_score fp32 [B] or None, sum of the row scores as a device scalar) through ``coattn_vqa_score``:
    asynchronous, nothing is read back."""
    if not logits.is_cuda:
        raise RuntimeError("vqa_score (HIP) needs tensors on the GPU")
    if logits.dtype != torch.float32:
        raise RuntimeError("vqa_score (HIP) computes in fp32; got %s" % logits.dtype)
    _check_targets("vqa_score", logits, ans_idx, ans_score)
    B, K = logits.shape
    z, ai, sc = logits.detach().contiguous(), ans_idx.contiguous(), ans_score.contiguous()
    dev = z.device
    ws = torch.empty(_lib.ce_workspace_bytes(B, K) // 4, device=dev, dtype=torch.float32)
    pred = torch.empty(B, device=dev, dtype=torch.int32)
    rows = torch.empty(B, device=dev, dtype=torch.float32) if row_score else None
    total = torch.empty((), device=dev, dtype=torch.float32)
    with _lib.on_device(dev):
        _score_call(z, ai, sc, pred, rows, total, ws, _lib.stream_ptr(dev))()
    global _last
    _last = (ws, B, dev)
    return pred, rows, total


def vqa_score(logits, ans_idx, ans_score):
    """The VQA accuracy of the arg-max answers: (pred int32 [B] -- the lowest index among equal maxima --, row_score fp32 [B] =
    min(1, t[b, pred[b]]), their mean as a device scalar).  CUDA fp32 logits take ``coattn_vqa_score``; CPU tensors stock ops."""
    if logits.is_cuda:
        pred, rows, total = vqa_score_sum(logits, ans_idx, ans_score)
        return pred, rows, total / logits.shape[0]
    t = dense_targets(ans_idx, ans_score, logits.shape[1])
    pred = logits.argmax(1)
    rows = t.gather(1, pred[:, None])[:, 0].clamp(max=1.0)
    return pred.to(torch.int32), rows, rows.mean()

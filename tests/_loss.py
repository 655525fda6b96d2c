"""The loss and score kernels' C-ABI (coattn_ce_forward, coattn_soft_loss_forward, coattn_vqa_score; csrc/ce.hip,
include/coattn.h) for the tests: runners over ``_lib.bind`` that put every device buffer of a call at its exact size inside a
marker-filled arena, the outputs and the workspace pre-filled with NaN, and check every margin after every call; the oracles --
``F.cross_entropy`` and the functions of ``tests/_soft_loss.py`` in float64 (the reference) or float32 (the yardstick of the
error bound), on the CPU, never the code under test --; and the checker: the project's rule (8 x stock fp32, floor 16 ulps;
``tests/_lstm.bound_check``) applied to the two groups of a gradient separately and, with the floor taken at the magnitudes
that are subtracted, to the scalar loss."""
import functools

import torch
import torch.nn.functional as F

from oracle import coattn_oracle as O
from vqa_amd import _lib

from tests import _soft_loss as SL
from tests._general import Arena
from tests._lstm import bound_check, same_bits  # noqa: F401  (re-exported for the test files)

KINDS = ("hard", "soft_ce", "bce")
FACTOR, FLOOR_ULPS = 8.0, 16.0


def al64(n):
    return (n + 63) & ~63


# ---- inputs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def make_logits(B, K, scale, seed=3):
    """float32 [B,K] on the host, shared and never written."""
    return torch.from_numpy(O.hash_normal((B, K), seed + 131 * B + K, scale)).float()


@functools.lru_cache(None)
def make_labels(B, K, seed=6):
    """int64 [B]; class 0 in row 0 and class K - 1 in row 1 wherever B >= 2."""
    lab = torch.from_numpy((O.hash_uniform(B, seed + B + K) * K).astype("int64")).clamp_(0, K - 1)
    if B >= 2:
        lab[0], lab[1] = 0, K - 1
    return lab


@functools.lru_cache(None)
def make_slots(B, K, A, seed=21):
    """tests/_soft_loss.make_targets (duplicate pairs, empty slots, every seventh row empty; a row that came out empty by
    chance gets one live slot, so the small shapes have targets too) with, where A = 16 and B >= 3, row 2's sixteen slots all
    naming one class with score 0.1: a 16-term sum in slot order, t > 1 for the BCE clamp, S_b = 1.6."""
    idx, sc = SL.make_targets(B, K, A, seed=seed + B + K)
    lab = make_labels(B, K)
    for b in range(B):                                   # only every seventh row stays wholly empty: the others get (label, 0.9)
        if b % 7 != 6 and bool((idx[b] == -1).all()):
            idx[b, 0], sc[b, 0] = int(lab[b]), 0.9
    if A == 16 and B >= 3:
        idx[2, :] = K // 2
        sc[2, :] = 0.1
    return idx, sc


# ---- oracles --------------------------------------------------------------------------------------------------------------
def oracle_ce(z, labels, dtype=torch.float64):
    """(loss, dlogits) of F.cross_entropy in `dtype` with autograd, on the CPU."""
    zz = z.detach().cpu().to(dtype).requires_grad_(True)
    loss = F.cross_entropy(zz, labels.cpu())
    loss.backward()
    return loss.detach(), zz.grad


def dense(tgt, K):
    """tests/_soft_loss.dense of the slots `tgt` = (ans_idx, ans_score), once per content (it is a Python loop over B A)."""
    key = (tuple(tgt[0].shape), tgt[0].cpu().numpy().tobytes(), tgt[1].cpu().numpy().tobytes(), K)
    if key not in _DENSE:
        _DENSE[key] = SL.dense(tgt[0], tgt[1], K)
    return _DENSE[key]


_DENSE = {}


def oracle_soft(z, idx, sc, kind, dtype=torch.float64):
    """(loss, dlogits) of tests/_soft_loss.row_losses over tests/_soft_loss.dense in `dtype` with autograd, on the CPU (float32:
    the dense target is the float64 sum rounded once)."""
    zz = z.detach().cpu().to(dtype).requires_grad_(True)
    t = dense((idx, sc), z.shape[1]).to(dtype)
    loss = SL.row_losses(zz, t, kind).mean()
    loss.backward()
    return loss.detach(), zz.grad


def oracle(kind, z, tgt, dtype=torch.float64):
    return oracle_ce(z, tgt, dtype) if kind == "hard" else oracle_soft(z, tgt[0], tgt[1], kind, dtype)


def oracle_score(z, idx, sc):
    """(pred int64 [B], rows float64 [B], their float64 sum, their sum by stock fp32 ops)."""
    pred, rows, _ = SL.score(z, idx, sc)
    return torch.from_numpy(pred), rows, rows.sum(), rows.float().sum()


def target_mask(kind, tgt, B, K):
    """bool [B,K]: the gradient's target entries -- (b, label_b), or the entries with t[b, k] != 0."""
    if kind == "hard":
        m = torch.zeros(B, K, dtype=torch.bool)
        m[torch.arange(B), tgt.cpu()] = True
        return m
    return dense(tgt, K) != 0


def loss_scale(kind, z, tgt):
    """The mean over the rows of the magnitudes the loss subtracts (float64): S_b |lse_b| + |sum_k t z| for the cross entropies,
    sum_k softplus(z) + |t z| for the binary one.  With confident rows the loss cancels to about 0 while its absolute error
    stays at an ulp of these."""
    z = z.detach().cpu().double()
    B, K = z.shape
    if kind == "hard":
        t = torch.zeros(B, K, dtype=torch.float64)
        t[torch.arange(B), tgt.cpu()] = 1.0
    else:
        t = dense(tgt, K)
    if kind == "bce":
        softplus = z.clamp(min=0) + torch.log1p(torch.exp(-z.abs()))
        return float((softplus + (t.clamp(max=1.0) * z).abs()).sum(1).mean())
    return float((t.sum(1) * torch.logsumexp(z, 1).abs() + (t * z).sum(1).abs()).mean())


@functools.lru_cache(None)
def references(kind, B, K, A, scale):
    """(z, targets, float64 (loss, dlogits), float32 (loss, dlogits), target mask, loss scale) of a case, computed once and shared
    between the tests, never written."""
    z = make_logits(B, K, scale)
    tgt = make_labels(B, K) if kind == "hard" else make_slots(B, K, A)
    return z, tgt, oracle(kind, z, tgt), oracle(kind, z, tgt, torch.float32), target_mask(kind, tgt, B, K), loss_scale(kind, z, tgt)


# ---- the checker ----------------------------------------------------------------------------------------------------------
def check_grad(name, got, ref64, stock32, mask, rows=None):
    """The rule on each of the two groups of a gradient: the target entries (`mask`) and the rest, each against its own stock
    deviation and with the floor at its own largest magnitude.  An empty group passes.  `rows`: the rows to look at (all).
    Returns the (err, bound) pairs; asserts."""
    if rows is not None:
        got, ref64, stock32, mask = got[rows], ref64[rows], stock32[rows], mask[rows]
    out = []
    for group, sel in (("target", mask), ("rest", ~mask)):
        if not bool(sel.any()):
            print("loss rule %s %s: empty group" % (name, group))
            continue
        err, bound = bound_check("%s %s" % (name, group), got[sel], ref64[sel], stock32[sel], FACTOR, FLOOR_ULPS)
        out.append((group, err, bound))
    for group, err, bound in out:
        assert err <= bound, (name, group, err, bound)
    return out


def check_scalar(name, got, ref64, stock32, scale):
    """The rule on a scalar whose floor is taken at `scale` instead of at |ref|.  Returns (err, bound); asserts."""
    err, stock = abs(float(got) - float(ref64)), abs(float(stock32) - float(ref64))
    floor = FLOOR_ULPS * 2.0 ** -24 * scale
    bound = max(FACTOR * stock, floor)
    print("loss rule %-9s err %.3e stock %.3e ratio %.2f floor %.3e scale %.3e ref %.7g" % (name, err, stock, err / max(stock, 1e-300),
                                                                                         floor, scale, float(ref64)))
    assert err <= bound, (name, err, bound)                  # (a NaN err fails here)
    return err, bound


def check_score(name, pred, row_score, score_sum, z, idx, sc):
    """A score call's outputs against the oracle: pred is numpy.argmax (the first of equal maxima, the first NaN) and inside
    [0, K); row_score is the oracle's selection -- the same NaNs, every other entry bit for bit --; score_sum is under the
    scalar rule with the floor at sum row_score (where that is NaN: NaN).  `row_score` may be None.  Returns the oracle's."""
    p_ref, r_ref, s64, s32 = oracle_score(z, idx, sc)
    K = z.shape[1]
    assert pred.tolist() == p_ref.tolist(), (name, pred.tolist(), p_ref.tolist())
    assert bool(((pred >= 0) & (pred < K)).all()), name
    if row_score is not None:
        nan = torch.isnan(r_ref)
        assert torch.equal(torch.isnan(row_score), nan), (name, row_score, r_ref)
        assert same_bits(row_score[~nan], r_ref.float()[~nan]), (name, row_score, r_ref)
    if bool(torch.isnan(s64)):
        assert bool(torch.isnan(score_sum)), (name, score_sum)
    else:
        check_scalar(name, score_sum, s64, s32, float(r_ref.sum()))
    return p_ref, r_ref, s64, s32


# ---- the runners ----------------------------------------------------------------------------------------------------------
class _Buf:
    """`n` floats inside an arena of exactly their size -- or, `shifted`, 4 bytes behind the start of an arena one float
    longer, whose first float must keep its fill."""

    def __init__(self, n, shifted=False, values=None, dtype=torch.float32):
        self.off = 1 if shifted else 0
        self.arena = Arena(n + self.off)
        self.data = self.arena.body[self.off:]
        self.ptr = self.arena.body.data_ptr() + 4 * self.off
        if values is not None:
            self.data.view(dtype).copy_(values.reshape(-1))

    def check(self, what):
        self.arena.check(what)
        if self.off:
            assert bool(torch.isnan(self.arena.body[0])), "%s: the float in front of the shifted operand was written" % what

    def host(self, dtype=torch.float32):
        return self.data.view(dtype).cpu()


def new_ws(B, K):
    """A NaN-filled arena of exactly coattn_ce_workspace_bytes: its contents need no initialisation by contract."""
    return Arena(_lib.ce_workspace_bytes(B, K) // 4)


def _finish(bufs, ws, B, expect_rc, rc):
    """Synchronise, check every margin, read the status through coattn_ce_status and the two words behind ws[al64(B)]."""
    stream = torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream
    torch.cuda.synchronize()
    lib = _lib.load()
    assert rc == expect_rc, (rc, lib.coattn_last_error().decode())
    for k, b in bufs.items():
        b.check("loss %s" % k)
    ws.check("loss ws")
    status = _lib.bind("coattn_ce_status", ws=ws.body.data_ptr(), B=B, stream=stream).code() if rc == 0 else None
    err = lib.coattn_last_error().decode()
    words = ws.body.view(torch.int32)[al64(B):al64(B) + 2].tolist()
    return dict(rc=rc, status=status, err=err, words=words, ws=ws)


def run_ce(z, labels, dlogits=True, ws=None, shift=None, expect_rc=0):
    """One coattn_ce_forward.  `shift`: "logits" or "dlogits" handed over 4 bytes behind its start (labels stay 8-byte aligned).
    Returns loss (0-dim), dlogits [B,K] or None, rc, status (coattn_ce_status), err, words, ws."""
    B, K = z.shape
    assert shift in (None, "logits", "dlogits")
    bufs = {"logits": _Buf(B * K, shift == "logits", z), "labels": _Buf(2 * B, False, labels, torch.int64), "loss": _Buf(1)}
    if dlogits:
        bufs["dlogits"] = _Buf(B * K, shift == "dlogits")
    ws = new_ws(B, K) if ws is None else ws
    stream = torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream
    rc = _lib.bind("coattn_ce_forward", logits=bufs["logits"].ptr, labels=bufs["labels"].ptr, loss=bufs["loss"].ptr,
                   dlogits=bufs["dlogits"].ptr if dlogits else None, ws=ws.body.data_ptr(), B=B, K=K, dtype=_lib.F32,
                   stream=stream).code()
    res = _finish(bufs, ws, B, expect_rc, rc)
    res.update(loss=bufs["loss"].host()[0], dlogits=bufs["dlogits"].host().view(B, K) if dlogits else None)
    return res


def run_soft(z, idx, sc, kind, dlogits=True, ws=None, shift=None, expect_rc=0):
    """One coattn_soft_loss_forward of `kind` ("soft_ce" / "bce").  `shift`: "logits", "dlogits", "ans_idx" or "ans_score"."""
    B, K = z.shape
    A = idx.shape[1]
    assert shift in (None, "logits", "dlogits", "ans_idx", "ans_score")
    bufs = {"logits": _Buf(B * K, shift == "logits", z), "ans_idx": _Buf(B * A, shift == "ans_idx", idx, torch.int32),
            "ans_score": _Buf(B * A, shift == "ans_score", sc), "loss": _Buf(1)}
    if dlogits:
        bufs["dlogits"] = _Buf(B * K, shift == "dlogits")
    ws = new_ws(B, K) if ws is None else ws
    stream = torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream
    rc = _lib.bind("coattn_soft_loss_forward", logits=bufs["logits"].ptr, ans_idx=bufs["ans_idx"].ptr,
                   ans_score=bufs["ans_score"].ptr, A=A, kind=SL.KINDS[kind], loss=bufs["loss"].ptr,
                   dlogits=bufs["dlogits"].ptr if dlogits else None, ws=ws.body.data_ptr(), B=B, K=K, dtype=_lib.F32,
                   stream=stream).code()
    res = _finish(bufs, ws, B, expect_rc, rc)
    res.update(loss=bufs["loss"].host()[0], dlogits=bufs["dlogits"].host().view(B, K) if dlogits else None)
    return res


def run_loss(kind, z, tgt, **kw):
    return run_ce(z, tgt, **kw) if kind == "hard" else run_soft(z, tgt[0], tgt[1], kind, **kw)


def run_score(z, idx, sc, row_score=True, ws=None, shift=None, expect_rc=0):
    """One coattn_vqa_score.  `shift`: "logits", "ans_idx", "ans_score", "pred" or "row_score".  Returns pred int32 [B],
    row_score [B] or None, score_sum (0-dim), rc, status, err, words, ws."""
    B, K = z.shape
    A = idx.shape[1]
    assert shift in (None, "logits", "ans_idx", "ans_score", "pred", "row_score")
    bufs = {"logits": _Buf(B * K, shift == "logits", z), "ans_idx": _Buf(B * A, shift == "ans_idx", idx, torch.int32),
            "ans_score": _Buf(B * A, shift == "ans_score", sc), "pred": _Buf(B, shift == "pred"), "score_sum": _Buf(1)}
    if row_score:
        bufs["row_score"] = _Buf(B, shift == "row_score")
    ws = new_ws(B, K) if ws is None else ws
    stream = torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream
    rc = _lib.bind("coattn_vqa_score", logits=bufs["logits"].ptr, ans_idx=bufs["ans_idx"].ptr, ans_score=bufs["ans_score"].ptr,
                   A=A, pred=bufs["pred"].ptr, row_score=bufs["row_score"].ptr if row_score else None,
                   score_sum=bufs["score_sum"].ptr, ws=ws.body.data_ptr(), B=B, K=K, dtype=_lib.F32, stream=stream).code()
    res = _finish(bufs, ws, B, expect_rc, rc)
    res.update(pred=bufs["pred"].host(torch.int32), row_score=bufs["row_score"].host() if row_score else None,
               score_sum=bufs["score_sum"].host()[0])
    return res


def nan_pattern(t):
    """int8 tensor: 0 finite, 1 NaN, 2 +inf, 3 -inf."""
    t = t.double()
    return (torch.isnan(t) * 1 + (t == float("inf")) * 2 + (t == float("-inf")) * 3).to(torch.int8)

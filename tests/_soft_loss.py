"""float64 oracle of the soft-answer-target losses and of the VQA score (include/coattn.h v0.12.0), shared by
test_soft_loss_cpu.py and test_gpu_soft_loss.py.  The dense target is built from the slots,

    t[b, k] = sum over the slots a with ans_idx[b, a] == k of ans_score[b, a]          (index -1: an empty slot, score not read)

and the two losses are their definitions in torch float64 with autograd, mean over the batch:

    soft cross entropy   row = S_b * logsumexp(z_b) - sum_k t z,     S_b = sum_k t[b, k]      (the sum over the k with t != 0)
    binary cross entropy row = sum_k (softplus(z) - min(t, 1) z),    softplus(z) = max(z, 0) + log1p(exp(-|z|))
"""
import numpy as np
import torch

from oracle import coattn_oracle as O

SOFT_CE, BCE = 1, 2
KINDS = {"soft_ce": SOFT_CE, "bce": BCE}
SCORES = (0.3, 0.6, 0.9, 1.0)


def dense(ans_idx, ans_score, K):
    """t [B,K] float64 from ans_idx [B,A] (int) / ans_score [B,A]; an empty slot's score is not looked at."""
    idx = ans_idx.cpu().long()
    sc = ans_score.cpu().double()
    B, A = idx.shape
    t = torch.zeros(B, K, dtype=torch.float64)
    for b in range(B):
        for a in range(A):
            k = int(idx[b, a])
            if k >= 0:
                t[b, k] += sc[b, a]
    return t


def row_losses(z, t, kind):
    if kind in ("soft_ce", SOFT_CE):
        tz = torch.where(t != 0, t * z, torch.zeros_like(z))        # a class without a target may be masked with -inf: no term
        return t.sum(1) * torch.logsumexp(z, 1) - tz.sum(1)
    softplus = z.clamp(min=0) + torch.log1p(torch.exp(-z.abs()))
    return (softplus - t.clamp(max=1.0) * z).sum(1)


def loss(z, ans_idx, ans_score, kind):
    """Mean loss of float64 logits `z` (may require grad)."""
    return row_losses(z, dense(ans_idx, ans_score, z.shape[1]), kind).mean()


def loss_and_grad(logits, ans_idx, ans_score, kind, upstream=1.0):
    z = logits.detach().cpu().double().requires_grad_(True)
    l = loss(z, ans_idx, ans_score, kind)
    (upstream * l).backward()
    return l.detach(), z.grad


def score(logits, ans_idx, ans_score):
    """(pred [B] -- numpy.argmax of the logits as they are: the first index among equal maxima --, row_score [B] float64 =
    min(1, t[b, pred[b]]), mean row score)."""
    z = logits.detach().cpu().numpy()
    pred = np.argmax(z, axis=1)
    t = dense(ans_idx, ans_score, z.shape[1])
    rows = t[torch.arange(z.shape[0]), torch.from_numpy(pred)].clamp(max=1.0)
    return pred, rows, rows.mean()


def make_targets(B, K, A, seed, label=None):
    """Deterministic slots from the oracle's hash generators: about a third of the slots empty, scores from SCORES, every
    fifth row with slot 1 repeating slot 0's class (a duplicate PAIR: its fp32 sum is the correctly rounded float64 one),
    every seventh row wholly empty.  `label` (int [B]): slot 0 becomes (label, 1.0).  Returns int32 [B,A], float32 [B,A]."""
    u = O.hash_uniform(B * A, seed).reshape(B, A)
    idx = np.minimum((O.hash_uniform(B * A, seed + 1).reshape(B, A) * K).astype("int64"), K - 1)
    sc = np.asarray(SCORES, dtype="float32")[np.minimum((O.hash_uniform(B * A, seed + 2).reshape(B, A) * 4).astype("int64"), 3)]
    empty = u < 1.0 / 3.0
    if A >= 2:                                   # (a class may otherwise repeat by chance only where K is tiny)
        for b in range(B):
            seen = set()
            for a in range(A):
                if empty[b, a]:
                    continue
                while int(idx[b, a]) in seen and len(seen) < K:
                    idx[b, a] = (idx[b, a] + 1) % K
                if int(idx[b, a]) in seen:
                    empty[b, a] = True
                else:
                    seen.add(int(idx[b, a]))
        for b in range(0, B, 5):
            empty[b, 0] = empty[b, 1] = False
            idx[b, 1] = idx[b, 0]
            sc[b, 0], sc[b, 1] = 0.3, 0.6
    for b in range(6, B, 7):
        empty[b, :] = True
    idx = np.where(empty, -1, idx)
    sc = np.where(empty, 0.0, sc).astype("float32")
    if label is not None:
        idx[:, 0] = label.cpu().numpy()
        sc[:, 0] = 1.0
    return torch.from_numpy(idx.astype("int32")), torch.from_numpy(sc)


def one_hot_targets(labels, A):
    """Slot 0 = (label, 1.0), the other slots empty: the anchor to the hard-label path."""
    B = labels.shape[0]
    idx = torch.full((B, A), -1, dtype=torch.int32)
    idx[:, 0] = labels.cpu().to(torch.int32)
    sc = torch.zeros(B, A, dtype=torch.float32)
    sc[:, 0] = 1.0
    return idx, sc

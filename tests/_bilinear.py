"""Float64 oracle of the co-attention with the bilinear affinity (include/coattn.h, COATTN_FLAG_BILINEAR), shared by
tests/test_bilinear_cpu.py and tests/test_gpu_bilinear.py.

It is torch autograd of the reference's ParallelCoAttention.forward (model.py:372-392) with one line changed,
    C = tanh(bmm(self.W_b(Q), V))           (reference: C = tanh(bmm(Q, V)))
and, with lengths, the length-masked form evaluated as the definition says: the unmasked computation on Q[b, :len_b] alone.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import torch
import torch.nn.functional as F

NAMES = ("W_v.weight", "W_v.bias", "W_q.weight", "W_q.bias", "w_v.weight", "w_v.bias", "w_q.weight", "w_q.bias",
         "W_b.weight", "W_b.bias")


def _level(V_phys, Q, P, bilinear):
    """One level of one batch: V_phys [B,d,N], Q [B,T,d] -> v, q [B,d], a_v [B,N], a_q [B,T]."""
    Vn = V_phys.permute(0, 2, 1)
    K = F.linear(Q, P["W_b.weight"], P["W_b.bias"]) if bilinear else Q
    C = torch.tanh(torch.bmm(K, V_phys))
    Pv = F.linear(Vn, P["W_v.weight"], P["W_v.bias"])
    Pq = F.linear(Q, P["W_q.weight"], P["W_q.bias"])
    H_v = torch.tanh(Pv + torch.bmm(C.transpose(2, 1), Pq))
    H_q = torch.tanh(Pq + torch.bmm(C, Pv))
    a_v = F.softmax(F.linear(H_v, P["w_v.weight"], P["w_v.bias"]), dim=1)
    a_q = F.softmax(F.linear(H_q, P["w_q.weight"], P["w_q.bias"]), dim=1)
    return torch.sum(a_v * Vn, dim=1), torch.sum(a_q * Q, dim=1), a_v.squeeze(2), a_q.squeeze(2)


def forward(V_phys: torch.Tensor, Qs: Sequence[torch.Tensor], P: Dict[str, torch.Tensor], bilinear: bool = True,
            lens: Sequence[int] | None = None):
    """v, q [L,B,d], a_v [L,B,N], a_q [L,B,T] (a_q = 0 past a length under `lens`)."""
    outs = {k: [] for k in ("v", "q", "a_v", "a_q")}
    B, T = Qs[0].shape[0], Qs[0].shape[1]
    for Q in Qs:
        if lens is None:
            v, q, a_v, a_q = _level(V_phys, Q, P, bilinear)
        else:
            vs, qs, avs, aqs = [], [], [], []
            for b in range(B):
                n = min(max(int(lens[b]), 1), T)
                v1, q1, av1, aq1 = _level(V_phys[b:b + 1], Q[b:b + 1, :n], P, bilinear)
                vs.append(v1); qs.append(q1); avs.append(av1)
                aqs.append(torch.cat([aq1, aq1.new_zeros(1, T - n)], dim=1))
            v, q, a_v, a_q = torch.cat(vs), torch.cat(qs), torch.cat(avs), torch.cat(aqs)
        outs["v"].append(v); outs["q"].append(q); outs["a_v"].append(a_v); outs["a_q"].append(a_q)
    return {k: torch.stack(x) for k, x in outs.items()}


def forward_backward(V_phys, Qs: List[torch.Tensor], P, gv, gq, bilinear=True, lens=None, g_av=None, g_aq=None,
                     device="cpu", dtype=torch.float64):
    """Float64 (or `dtype`: float32 is the reference's own arithmetic) forward and autograd backward of sum(v gv) + sum(q gq) (+ sum(a_v G_av) + sum(a_q G_aq)).
    Returns the forward outputs and dV_phys [B,d,N], dQ [L,B,T,d] and d<name> for every parameter, all float64 on CPU."""
    dd = dict(device=device, dtype=dtype)
    V = V_phys.to(**dd).requires_grad_(True)
    Q = [q.to(**dd).requires_grad_(True) for q in Qs]
    Pd = {k: P[k].to(**dd).requires_grad_(True) for k in NAMES}
    out = forward(V, Q, Pd, bilinear, lens)
    loss = (out["v"] * gv.to(**dd)).sum() + (out["q"] * gq.to(**dd)).sum()
    if g_av is not None:
        loss = loss + (out["a_v"] * g_av.to(**dd)).sum()
    if g_aq is not None:
        loss = loss + (out["a_q"] * g_aq.to(**dd)).sum()
    ins = [V, *Q, *[Pd[k] for k in NAMES]]
    grads = torch.autograd.grad(loss, ins, allow_unused=True)
    res = {k: v.detach().cpu() for k, v in out.items()}
    res["dV_phys"] = grads[0].cpu()
    res["dQ"] = torch.stack([g.cpu() for g in grads[1:1 + len(Q)]])
    for k, g in zip(NAMES, grads[1 + len(Q):]):
        res["d" + k] = None if g is None else g.cpu()
    return res

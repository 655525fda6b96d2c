"""float64 oracle of the alternating co-attention (include/coattn.h v0.11.0; Lu et al. 2016 section 3.3): torch autograd of
the definition, per sample on Q[b, :len_b] when masked (the maps padded with 0), as tests/_bilinear.py does for the bilinear
form."""
import torch

NAMES = ("W_x1", "b_x1", "w_h1", "c_h1", "W_x2", "b_x2", "W_g2", "b_g2", "w_h2", "c_h2",
         "W_x3", "b_x3", "W_g3", "b_g3", "w_h3", "c_h3")
def state_key(name: str) -> str:
    """C-ABI parameter name -> AlternatingCoAttention state_dict key: W_x1 -> W_x1.weight, b_x1 -> W_x1.bias,
    w_h1 -> w_h1.weight, c_h1 -> w_h1.bias."""
    if name.startswith("b_"):
        return "W_" + name[2:] + ".bias"
    if name.startswith("c_"):
        return "w_" + name[2:] + ".bias"
    return name + ".weight"


def make_params(d: int, seed: int = 0, scale: float = 1.0):
    g = torch.Generator().manual_seed(seed)
    P = {}
    for n in NAMES:
        if n[0] == "W":
            P[n] = torch.randn(d, d, generator=g, dtype=torch.float64) * (scale / d ** 0.5)
        elif n[0] == "w":
            P[n] = torch.randn(1, d, generator=g, dtype=torch.float64) * (scale / d ** 0.5)
        elif n[0] == "c":
            P[n] = torch.randn(1, generator=g, dtype=torch.float64) * 0.1
        else:
            P[n] = torch.randn(d, generator=g, dtype=torch.float64) * 0.1
    return P


def _guided(X, g, W, b, w, c):
    H = torch.tanh(X @ W.T + b + g)
    a = torch.softmax((H @ w.T).squeeze(-1) + c, dim=0)
    return a @ X, a


def forward(V, Qs, P, lens=None):
    """V [B,N,d], Qs: L x [B,T,d] (float64) -> v [L,B,d], q [L,B,d], a_v [L,B,N], a_q [L,B,T] (differentiable)."""
    B, N, d = V.shape
    T = Qs[0].shape[1]
    vs, qs, avs, aqs = [], [], [], []
    for Q in Qs:
        vl, ql, avl, aql = [], [], [], []
        for b in range(B):
            n = T if lens is None else max(1, min(int(lens[b]), T))
            Qb = Q[b, :n]
            s, _ = _guided(Qb, 0.0, P["W_x1"], P["b_x1"], P["w_h1"], P["c_h1"])
            v, av = _guided(V[b], s @ P["W_g2"].T + P["b_g2"], P["W_x2"], P["b_x2"], P["w_h2"], P["c_h2"])
            q, aq = _guided(Qb, v @ P["W_g3"].T + P["b_g3"], P["W_x3"], P["b_x3"], P["w_h3"], P["c_h3"])
            vl.append(v); ql.append(q); avl.append(av)
            aql.append(torch.cat([aq, aq.new_zeros(T - n)]))
        vs.append(torch.stack(vl)); qs.append(torch.stack(ql)); avs.append(torch.stack(avl)); aqs.append(torch.stack(aql))
    return torch.stack(vs), torch.stack(qs), torch.stack(avs), torch.stack(aqs)


def forward_backward(V, Qs, P, gv, gq, g_av=None, g_aq=None, lens=None):
    """Outputs and gradients (float64): dict with v, q, a_v, a_q, dV, dQ (list), and d<name> for every parameter."""
    V = V.double().detach().requires_grad_(True)
    Qs = [q.double().detach().requires_grad_(True) for q in Qs]
    Pg = {k: v.double().detach().requires_grad_(True) for k, v in P.items()}
    v, q, av, aq = forward(V, Qs, Pg, lens)
    loss = (v * gv.double()).sum() + (q * gq.double()).sum()
    if g_av is not None:
        loss = loss + (av * g_av.double()).sum()
    if g_aq is not None:
        if lens is not None:
            T = aq.shape[-1]
            m = (torch.arange(T)[None, :] < torch.as_tensor(lens).clamp(1, T)[:, None]).double()
            loss = loss + (aq * g_aq.double() * m).sum()
        else:
            loss = loss + (aq * g_aq.double()).sum()
    loss.backward()
    out = {"v": v.detach(), "q": q.detach(), "a_v": av.detach(), "a_q": aq.detach(), "dV": V.grad, "dQ": [x.grad for x in Qs]}
    for k, t in Pg.items():
        out["d" + k] = t.grad
    return out

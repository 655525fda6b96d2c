"""The question GRU's C-ABI (coattn_gru_forward / coattn_gru_backward; csrc/gru.hip, include/coattn_rnn.h) for the tests: a ctypes
runner that puts every device buffer of a call at its exact size inside a marker-filled arena with the outputs pre-filled with
NaN, and the oracle -- stock torch.nn.GRU on the CPU behind pack_padded_sequence(enforce_sorted=False), in float64 (the
reference) or float32 (the yardstick of the error bound) -- never the code under test."""
import ctypes as C

import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from vqa_amd import _lib

from tests._general import Arena
from tests._lstm import bound_check, clamp, lengths, live_mask, same_bits  # noqa: F401  (re-exported for the test files)

PARAMS = ("w_ih", "w_hh", "b_ih", "b_hh")
OUTPUTS = ("seq", "h_last", "dX", "dw_ih", "dw_hh", "db_ih", "db_hh")
PAD = 7.0                                   # what the cases put into the rows of X past a question's length
_TORCH_NAME = {"w_ih": "weight_ih_l0", "w_hh": "weight_hh_l0", "b_ih": "bias_ih_l0", "b_hh": "bias_hh_l0"}


def make_case(B, T, E, H, seed, kind="unsorted"):
    """Inputs on the host (float32): X with PAD in its pad rows, nn.GRU's parameters (its default U(-1/sqrt(H), 1/sqrt(H))
    initialisation), the two incoming gradients, the lengths."""
    g = torch.Generator().manual_seed(2000 + seed)
    k = H ** -0.5
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k          # noqa: E731
    lens = lengths(B, T, seed, kind)
    c = dict(B=B, T=T, E=E, H=H, lens=lens, X=torch.randn(B, T, E, generator=g),
             w_ih=u(3 * H, E), w_hh=u(3 * H, H), b_ih=u(3 * H), b_hh=u(3 * H),
             g_seq=torch.randn(B, T, H, generator=g), g_last=torch.randn(B, H, generator=g))
    c["X"][~live_mask(lens, T)] = PAD
    return c


def _loss(seq, h_last, c, dtype, g_seq, g_last):
    gs = c["g_seq"] if g_seq is None else g_seq
    gl = c["g_last"] if g_last is None else g_last
    return (seq * gs.to(dtype)).sum() + (h_last * gl.to(dtype)).sum()


def oracle(c, dtype=torch.float64, lens=None, g_seq=None, g_last=None):
    """seq, h_last and the five gradients of sum(seq * g_seq) + sum(h_last * g_last) from stock PyTorch on the CPU: h_last is
    the hidden state nn.GRU returns for the packed batch, seq comes from pad_packed_sequence."""
    T, E, H = c["T"], c["E"], c["H"]
    rnn = torch.nn.GRU(E, H).to(dtype)
    with torch.no_grad():
        for n in PARAMS:
            getattr(rnn, _TORCH_NAME[n]).copy_(c[n])
    x = c["X"].to(dtype, copy=True).requires_grad_(True)            # (a copy: the case's own tensors stay plain inputs)
    ln = clamp(c["lens"] if lens is None else lens, T)
    y, hidden = rnn(pack_padded_sequence(x, ln, batch_first=True, enforce_sorted=False))
    seq = pad_packed_sequence(y, batch_first=True, total_length=T)[0]
    h_last = hidden.squeeze(0)
    _loss(seq, h_last, c, dtype, g_seq, g_last).backward()
    return dict(seq=seq.detach(), h_last=h_last.detach(), dX=x.grad, dw_ih=rnn.weight_ih_l0.grad, dw_hh=rnn.weight_hh_l0.grad,
                db_ih=rnn.bias_ih_l0.grad, db_hh=rnn.bias_hh_l0.grad)


def unpacked_reference(c, dtype=torch.float64):
    """The same function written out as include/coattn_rnn.h states it, operation by operation -- no packing: the recurrence
    over all T steps with the outputs SELECTED by t < len_b and h_last taken at step len_b - 1 -- with autograd for the
    gradients."""
    B, T, H = c["B"], c["T"], c["H"]
    p = {n: c[n].to(dtype, copy=True).requires_grad_(True) for n in PARAMS}
    x = c["X"].to(dtype, copy=True).requires_grad_(True)            # (a copy: the case's own tensors stay plain inputs)
    ln = clamp(c["lens"], T)
    live = live_mask(c["lens"], T)
    zero = torch.zeros((), dtype=dtype)
    h, h_last, outs = torch.zeros(B, H, dtype=dtype), torch.zeros(B, H, dtype=dtype), []
    w_hr, w_hz, w_hn = p["w_hh"].split(H, dim=0)
    b_hr, b_hz, b_hn = p["b_hh"].split(H, dim=0)
    for t in range(T):
        xt = torch.where(live[:, t, None], x[:, t], zero)                        # (a dead row's X is not read)
        gx_r, gx_z, gx_n = (xt @ p["w_ih"].T + p["b_ih"]).split(H, dim=1)
        hr, hz, hn = (h @ w_hr.T) + b_hr, (h @ w_hz.T) + b_hz, (h @ w_hn.T) + b_hn
        r, z = torch.sigmoid(gx_r + hr), torch.sigmoid(gx_z + hz)
        n = torch.tanh(gx_n + r * hn)
        h = torch.where(live[:, t, None], n + z * (h - n), zero)                 # seq_out: h_t on live steps, zero past the length
        outs.append(h)
        h_last = torch.where((ln == t + 1)[:, None], h, h_last)
    seq = torch.stack(outs, 1)
    _loss(seq, h_last, c, dtype, None, None).backward()
    return dict(seq=seq.detach(), h_last=h_last.detach(), dX=x.grad, dw_ih=p["w_ih"].grad, dw_hh=p["w_hh"].grad,
                db_ih=p["b_ih"].grad, db_hh=p["b_hh"].grad)


def workspace_bytes(B, T, E, H):
    return _lib.gru_workspace_bytes(B, T, E, H)


def _put(t):
    a = Arena(t.numel(), fill=None)
    a.body.copy_(t.reshape(-1))
    return a


def run(c, lens=None, X=None, g_seq=None, g_last=None, saved=True, h_last=True, dX=True, with_g_seq=True, with_g_last=True,
        accumulate=0, prefill=None, flags=0, backward=True, expect_rc=0, expect_rc_bwd=None):
    """One coattn_gru_forward (+ coattn_gru_backward) on case `c` straight through the C-ABI; `lens`, `X`, `g_seq`, `g_last`
    replace the case's.  Every buffer is an arena of its exact size; the outputs start as NaN (the parameter gradients as
    `prefill` [name] with accumulate = 1).  Checks every arena's margins afterwards.  Returns the outputs on the host (a buffer
    the call was not given keeps its NaN), and "rc": the return codes (expected: `expect_rc` for both calls, `expect_rc_bwd` for
    the backward if given)."""
    lib = _lib.load()
    B, T, E, H = c["B"], c["T"], c["E"], c["H"]
    sb, fb, bb = workspace_bytes(B, T, E, H) if lib.coattn_gru_supported(B, T, E, H, _lib.F32) else (64, 64, 64)
    dev = torch.device("cuda:0")
    ar = {"X": _put(c["X"] if X is None else X), "g_seq": _put(c["g_seq"] if g_seq is None else g_seq),
          "g_last": _put(c["g_last"] if g_last is None else g_last)}
    for n in PARAMS:
        ar[n] = _put(c[n])
    ln = torch.as_tensor(c["lens"] if lens is None else lens).to(torch.int32)
    ar["len"] = Arena(B, fill=None)
    ar["len"].body.view(torch.int32).copy_(ln)
    ar["seq"] = Arena(B * T * H)
    ar["h_last"] = Arena(B * H)
    ar["dX"] = Arena(B * T * E)
    ar["saved"], ar["ws_fwd"], ar["ws_bwd"] = Arena(sb // 4), Arena(fb // 4), Arena(bb // 4)
    for n in PARAMS:
        ar["d" + n] = Arena(c[n].numel())
        if prefill is not None:
            ar["d" + n].body.copy_(prefill[n].reshape(-1))
    P = lambda k, on=True: C.c_void_p(ar[k].body.data_ptr() if on else 0)      # noqa: E731
    p = _lib.GruParams(*[ar[n].body.data_ptr() for n in PARAMS])
    pg = _lib.GruParamGrads(*[ar["d" + n].body.data_ptr() for n in PARAMS])
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc_f = lib.coattn_gru_forward(P("X"), P("len"), C.byref(p), P("seq"), P("h_last", h_last), P("saved", saved), P("ws_fwd"),
                                  B, T, E, H, _lib.F32, flags, stream)
    rc_b = None
    if backward and saved:
        rc_b = lib.coattn_gru_backward(P("X"), P("len"), C.byref(p), P("saved"), P("g_seq", with_g_seq), P("g_last", with_g_last),
                                       P("dX", dX), C.byref(pg), accumulate, P("ws_bwd"), B, T, E, H, _lib.F32, flags, stream)
    torch.cuda.synchronize()
    assert rc_f == expect_rc, (rc_f, lib.coattn_last_error().decode())
    assert rc_b in (None, expect_rc if expect_rc_bwd is None else expect_rc_bwd), (rc_b, lib.coattn_last_error().decode())
    for k, a in ar.items():
        a.check("gru %s" % k)
    res = dict(rc=(rc_f, rc_b), seq=ar["seq"].body.cpu().view(B, T, H), h_last=ar["h_last"].body.cpu().view(B, H),
               dX=ar["dX"].body.cpu().view(B, T, E))
    for n in PARAMS:
        res["d" + n] = ar["d" + n].body.cpu().view(c[n].shape)
    return res

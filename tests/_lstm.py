"""The sentence LSTM's C-ABI (coattn_lstm_forward / coattn_lstm_backward; csrc/lstm.hip) for the tests: a ctypes runner that
puts every device buffer of a call at its exact size inside a marker-filled arena with the outputs pre-filled with NaN, and
the oracle -- stock torch.nn.LSTM on the CPU behind pack_padded_sequence(enforce_sorted=False) / pad_packed_sequence, in
float64 (the reference) or float32 (the yardstick of the error bound) -- never the code under test."""
import ctypes as C

import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from vqa_amd import _lib

from tests._general import Arena

PARAMS = ("w_ih", "w_hh", "b_ih", "b_hh")
OUTPUTS = ("out", "x_masked", "dX", "dw_ih", "dw_hh", "db_ih", "db_hh")
PAD = 7.0                                   # what the cases put into the rows of X past a question's length


def lengths(B, T, seed, kind="unsorted"):
    """unsorted: [T, 1, random ...]; sorted_dead_tail (B >= 33): descending, the samples of the last 32-row tile (32 ..) all
    of length <= T // 3 -- that tile is entirely dead from step T // 3 on."""
    g = torch.Generator().manual_seed(seed)
    if kind == "unsorted":
        ln = torch.randint(1, T + 1, (B,), generator=g)
        ln[0] = T
        if B > 1:
            ln[1] = 1
        return ln.to(torch.int32)
    assert kind == "sorted_dead_tail" and B >= 33
    head = torch.randint(max(1, T // 3), T + 1, (32,), generator=g)
    head[0] = T
    tail = torch.randint(1, max(1, T // 3) + 1, (B - 32,), generator=g)
    return torch.cat([head.sort(descending=True)[0], tail.sort(descending=True)[0]]).to(torch.int32)


def clamp(lens, T):
    return torch.as_tensor(lens).to(torch.int64).clamp(1, T)


def live_mask(lens, T):
    """[B, T] bool: t < clamp(len_b, 1, T)."""
    return torch.arange(T)[None, :] < clamp(lens, T)[:, None]


def make_case(B, T, E, H, seed, kind="unsorted"):
    """Inputs on the host (float32): X with PAD in its pad rows, nn.LSTM's parameters (its default U(-1/sqrt(H), 1/sqrt(H))
    initialisation), the two incoming gradients, the lengths."""
    g = torch.Generator().manual_seed(1000 + seed)
    k = H ** -0.5
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k          # noqa: E731
    lens = lengths(B, T, seed, kind)
    c = dict(B=B, T=T, E=E, H=H, lens=lens, X=torch.randn(B, T, E, generator=g),
             w_ih=u(4 * H, E), w_hh=u(4 * H, H), b_ih=u(4 * H), b_hh=u(4 * H),
             g_out=torch.randn(B, T, H, generator=g), g_xm=torch.randn(B, T, E, generator=g))
    c["X"][~live_mask(lens, T)] = PAD
    return c


def oracle(c, dtype=torch.float64, lens=None):
    """out, x_masked and the six gradients of sum(out * g_out) + sum(x_masked * g_xm) from stock PyTorch on the CPU."""
    B, T, E, H = c["B"], c["T"], c["E"], c["H"]
    rnn = torch.nn.LSTM(E, H).to(dtype)
    with torch.no_grad():
        for n in PARAMS:
            getattr(rnn, {"w_ih": "weight_ih_l0", "w_hh": "weight_hh_l0", "b_ih": "bias_ih_l0", "b_hh": "bias_hh_l0"}[n]).copy_(c[n])
    x = c["X"].to(dtype).requires_grad_(True)
    ln = clamp(c["lens"] if lens is None else lens, T)
    packed = pack_padded_sequence(x, ln, batch_first=True, enforce_sorted=False)
    y, _ = rnn(packed)
    out = pad_packed_sequence(y, batch_first=True, total_length=T)[0]
    xm = pad_packed_sequence(packed, batch_first=True, total_length=T)[0]
    ((out * c["g_out"].to(dtype)).sum() + (xm * c["g_xm"].to(dtype)).sum()).backward()
    return dict(out=out.detach(), x_masked=xm.detach(), dX=x.grad, dw_ih=rnn.weight_ih_l0.grad, dw_hh=rnn.weight_hh_l0.grad,
                db_ih=rnn.bias_ih_l0.grad, db_hh=rnn.bias_hh_l0.grad)


def unpacked_reference(c, dtype=torch.float64):
    """The same function written out as include/coattn.h states it -- no packing: the recurrence over all T steps with the
    outputs SELECTED by t < len_b -- with autograd for the gradients."""
    B, T, E, H = c["B"], c["T"], c["E"], c["H"]
    p = {n: c[n].to(dtype).requires_grad_(True) for n in PARAMS}
    x = c["X"].to(dtype).requires_grad_(True)
    live = live_mask(c["lens"], T)
    h, cc, outs = torch.zeros(B, H, dtype=dtype), torch.zeros(B, H, dtype=dtype), []
    for t in range(T):
        xt = torch.where(live[:, t, None], x[:, t], torch.zeros((), dtype=dtype))      # (a dead row's X is not read)
        gates = xt @ p["w_ih"].T + p["b_ih"] + h @ p["w_hh"].T + p["b_hh"]
        i, f, g, o = gates.split(H, dim=1)
        cc = torch.sigmoid(f) * cc + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(cc)
        outs.append(torch.where(live[:, t, None], h, torch.zeros((), dtype=dtype)))
    out = torch.stack(outs, 1)
    xm = torch.where(live[:, :, None], x, torch.zeros((), dtype=dtype))
    ((out * c["g_out"].to(dtype)).sum() + (xm * c["g_xm"].to(dtype)).sum()).backward()
    return dict(out=out.detach(), x_masked=xm.detach(), dX=x.grad, dw_ih=p["w_ih"].grad, dw_hh=p["w_hh"].grad,
                db_ih=p["b_ih"].grad, db_hh=p["b_hh"].grad)


def workspace_bytes(B, T, E, H):
    return _lib.lstm_workspace_bytes(B, T, E, H)


def _put(t):
    a = Arena(t.numel(), fill=None)
    a.body.copy_(t.reshape(-1))
    return a


def run(c, lens=None, X=None, g_out=None, g_xm=None, saved=True, x_masked=True, dX=True, with_g_xm=True, accumulate=0,
        prefill=None, flags=0, backward=True, expect_rc=0):
    """One coattn_lstm_forward (+ coattn_lstm_backward) on case `c` straight through the C-ABI; `lens`, `X`, `g_out`, `g_xm`
    replace the case's.  Every buffer is an arena of its exact size; the outputs start as NaN (the parameter gradients as
    `prefill` [name] with accumulate = 1).  Checks every arena's margins afterwards.  Returns the outputs on the host (a
    buffer the call was not given: None), and "rc": the return codes."""
    lib = _lib.load()
    B, T, E, H = c["B"], c["T"], c["E"], c["H"]
    sb, fb, bb = workspace_bytes(B, T, E, H) if lib.coattn_lstm_supported(B, T, E, H, _lib.F32) else (64, 64, 64)
    dev = torch.device("cuda:0")
    ar = {"X": _put(c["X"] if X is None else X), "g_out": _put(c["g_out"] if g_out is None else g_out),
          "g_xm": _put(c["g_xm"] if g_xm is None else g_xm)}
    for n in PARAMS:
        ar[n] = _put(c[n])
    ln = torch.as_tensor(c["lens"] if lens is None else lens).to(torch.int32)
    ar["len"] = Arena(B, fill=None)
    ar["len"].body.view(torch.int32).copy_(ln)
    ar["out"] = Arena(B * T * H)
    ar["x_masked"] = Arena(B * T * E)
    ar["dX"] = Arena(B * T * E)
    ar["saved"], ar["ws_fwd"], ar["ws_bwd"] = Arena(sb // 4), Arena(fb // 4), Arena(bb // 4)
    for n in PARAMS:
        ar["d" + n] = Arena(c[n].numel())
        if prefill is not None:
            ar["d" + n].body.copy_(prefill[n].reshape(-1))
    P = lambda k, on=True: C.c_void_p(ar[k].body.data_ptr() if on else 0)      # noqa: E731
    p = _lib.LstmParams(*[ar[n].body.data_ptr() for n in PARAMS])
    pg = _lib.LstmParamGrads(*[ar["d" + n].body.data_ptr() for n in PARAMS])
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc_f = lib.coattn_lstm_forward(P("X"), P("len"), C.byref(p), P("out"), P("x_masked", x_masked), P("saved", saved),
                                   P("ws_fwd"), B, T, E, H, _lib.F32, flags, stream)
    rc_b = None
    if backward and saved:
        rc_b = lib.coattn_lstm_backward(P("X"), P("len"), C.byref(p), P("out"), P("saved"), P("g_out"), P("g_xm", with_g_xm),
                                        P("dX", dX), C.byref(pg), accumulate, P("ws_bwd"), B, T, E, H, _lib.F32, flags, stream)
    torch.cuda.synchronize()
    assert rc_f == expect_rc, (rc_f, lib.coattn_last_error().decode())
    assert rc_b in (None, expect_rc), (rc_b, lib.coattn_last_error().decode())
    for k, a in ar.items():
        a.check("lstm %s" % k)
    res = dict(rc=(rc_f, rc_b), out=ar["out"].body.cpu().view(B, T, H),
               x_masked=ar["x_masked"].body.cpu().view(B, T, E), dX=ar["dX"].body.cpu().view(B, T, E))
    for n in PARAMS:
        res["d" + n] = ar["d" + n].body.cpu().view(c[n].shape)
    return res


def same_bits(a, b):
    return bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def bound_check(name, got, ref64, stock32, factor=8.0, floor_ulps=16.0):
    """(deviation of `got` from the float64 reference, the bound): at most `factor` times the deviation of stock fp32
    PyTorch on the same inputs, with a floor of `floor_ulps` fp32 ulps of the reference's largest magnitude."""
    err = float((got.double() - ref64).abs().max())
    stock = float((stock32.double() - ref64).abs().max())
    scale = float(ref64.abs().max())
    bound = max(factor * stock, floor_ulps * 2.0 ** -24 * scale)
    print("lstm bound %-9s err %.3e stock %.3e ratio %.2f floor %.3e scale %.3e" % (name, err, stock, err / max(stock, 1e-300),
                                                                               floor_ulps * 2.0 ** -24 * scale, scale))
    return err, bound

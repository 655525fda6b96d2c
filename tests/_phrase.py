"""GPU-side test helper for the phrase level: run coattn_phrase_forward / coattn_phrase_backward directly through the
C-ABI (ctypes) with caller-chosen flags, outputs, accumulate and buffer contents, and the float64 oracle of the same
operation (oracle.net_oracle.OraclePhraseConvPool).  Shared by tests/test_gpu_phrase_paths.py and
tests/test_phrase_cpu.py (which uses the CPU half only)."""
import ctypes as C
import functools
import math

import torch

from oracle import coattn_oracle as O
from oracle import net_oracle as NO

# state_dict keys in the order of coattn_phrase_params (W1, b1, W2, b2, W3, b3)
PKEYS = ("conv_unigram.1.weight", "conv_unigram.1.bias", "conv_bigram.1.weight", "conv_bigram.1.bias",
         "conv_trigram.1.weight", "conv_trigram.1.bias")
FAST16 = 128            # include/coattn.h COATTN_FLAG_FAST16: the tolerance mode
BF16 = 4                # COATTN_FLAG_BF16_PROJ: the reduced-precision mode


def make_params(E, seed):
    """The six parameters at nn.Conv1d's default scale U(+-1/sqrt(E k)), in closed form (fp32, CPU)."""
    sd = {}
    for i, k in enumerate((1, 2, 3)):
        bd = 1.0 / math.sqrt(E * k)
        sd[PKEYS[2 * i]] = torch.from_numpy(O.hash_unit((E, E, k), seed + 10 * i, bd)).float()
        sd[PKEYS[2 * i + 1]] = torch.from_numpy(O.hash_unit((E,), seed + 10 * i + 1, bd)).float()
    return sd


def make_inputs(B, T, E, seed):
    """x, g as tests/test_gpu_phrase.py: hash-normal, ragged zero tails; every x[b, 0] and last live row non-zero."""
    x = torch.from_numpy(O.hash_normal((B, T, E), seed + 1, 1.0)).float()
    for b in range(B):
        x[b, max(1, T - 3 * b):] = 0
    g = torch.from_numpy(O.hash_normal((B, T, E), seed + 2, 1.0)).float()
    return x, g


def oracle_phrase(x, state_dict, g=None):
    """float64 forward and, with g, all seven gradients: {"out", "dx", "grads": {state_dict key: tensor}}."""
    E = x.shape[2]
    ref = NO.OraclePhraseConvPool(E).double()
    ref.load_state_dict({k: v.double() for k, v in state_dict.items()})
    xr = x.double().requires_grad_(g is not None)
    y = ref(xr)
    res = {"out": y.detach()}
    if g is not None:
        y.backward(g.double())
        res["dx"] = xr.grad
        res["grads"] = {k: p.grad for k, p in ref.named_parameters()}
    return res


@functools.lru_cache(maxsize=None)
def case(B, T, E, seed):
    """(state_dict, x, g, oracle results) of one shape, computed once and shared (treat as read-only)."""
    sd = make_params(E, seed)
    x, g = make_inputs(B, T, E, seed)
    return sd, x, g, oracle_phrase(x, sd, g)


def workspace_bytes(B, T, E):
    from vqa_amd import _lib
    s, f, b = C.c_size_t(), C.c_size_t(), C.c_size_t()
    _lib.check(_lib.load().coattn_phrase_workspace_bytes(B, T, E, _lib.F32, C.byref(s), C.byref(f), C.byref(b)),
               "coattn_phrase_workspace_bytes")
    return s.value, f.value, b.value


def run_phrase(x, params, g=None, flags=0, need_dx=True, need_saved=True, accumulate=0, grads_init=None, poison=False,
               x_offset_floats=0, share_ws=False):
    """x [B,T,E], params: state_dict (PKEYS), g: upstream gradient or None (forward only).
    poison: every output, `saved` and workspace starts as 0xFF bytes (NaN) instead of zeros, and the backward gets a fresh
    NaN-filled workspace, not the forward's.  share_ws: ONE buffer serves as the workspace of both calls and is overwritten
    with 0xFF bytes between them (nothing the backward needs may live in the forward's workspace).
    x_offset_floats = k: X starts k floats into a larger allocation (contiguous, misaligned for k % 4 != 0).
    Returns {"out", "amax" (uint8 [B,T,E]), "status" (rc, act, wgt of coattn_phrase_status), "dx", "grads"}."""
    from vqa_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, T, E = x.shape
    n = B * T * E
    fill = 0xFF if poison else 0
    xbuf = torch.zeros(n + x_offset_floats + 4, device=dev)
    X = xbuf[x_offset_floats:x_offset_floats + n].view(B, T, E)
    X.copy_(x)
    assert X.data_ptr() == xbuf.data_ptr() + 4 * x_offset_floats and X.is_contiguous()
    ps = [params[k].to(dev).contiguous() for k in PKEYS]
    sb, fb, bb = workspace_bytes(B, T, E)

    def raw(nbytes):
        return torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)

    out = raw(4 * n).view(torch.float32).view(B, T, E)
    saved = raw(sb) if need_saved else None
    ws = raw(max(fb, bb) if share_ws else fb)
    p = _lib.PhraseParams(*[t.data_ptr() for t in ps])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.coattn_phrase_forward(X.data_ptr(), C.byref(p), out.data_ptr(), saved.data_ptr() if need_saved else None,
                                         ws.data_ptr(), B, T, E, _lib.F32, flags, stream), "coattn_phrase_forward")
    torch.cuda.synchronize()
    res = {"out": out, "amax": None, "status": None, "dx": None, "grads": None}
    if need_saved:
        res["amax"] = saved[:n].view(B, T, E)
        am = (C.c_float * 2)()
        res["status"] = (lib.coattn_phrase_status(saved.data_ptr(), B, T, E, stream, am), am[0], am[1])
    if g is None:
        return res
    assert need_saved, "the backward needs the forward's saved state"
    g = g.to(dev).contiguous()
    if share_ws:
        ws.fill_(0xFF)
        ws2 = ws
    else:
        ws2 = raw(bb)
    dx = raw(4 * n).view(torch.float32).view(B, T, E) if need_dx else None
    if grads_init is None:
        grads = [raw(4 * t.numel()).view(torch.float32).view(t.shape) for t in ps]
    else:
        grads = [grads_init[k].to(dev).clone().contiguous() for k in PKEYS]
    pg = _lib.PhraseParamGrads(*[t.data_ptr() for t in grads])
    _lib.check(lib.coattn_phrase_backward(X.data_ptr(), C.byref(p), out.data_ptr(), saved.data_ptr(), g.data_ptr(),
                                          dx.data_ptr() if need_dx else None, C.byref(pg), accumulate, ws2.data_ptr(),
                                          B, T, E, _lib.F32, flags, stream), "coattn_phrase_backward")
    torch.cuda.synchronize()
    res["dx"] = dx
    res["grads"] = dict(zip(PKEYS, grads))
    return res

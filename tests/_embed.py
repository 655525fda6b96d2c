"""The word embedding's C-ABI (coattn_embedding_forward / coattn_embedding_backward; csrc/embedding.hip) for the tests: the
cases, a ctypes runner that puts every device buffer of a call at its exact size inside a marker-filled arena with the outputs
pre-filled with NaN, the header's summation order restated in numpy float32 (`ordered_sum`), and the oracle -- stock
F.embedding with its autograd on the CPU, in float64 (the reference) or float32 (the yardstick of the error bound) -- never
the code under test."""
import ctypes as C
import functools
import re

import numpy as np
import torch
import torch.nn.functional as F

from vqa_amd import _lib

from tests._general import Arena
from tests._header import header

IDS = {"int32": (torch.int32, _lib.IDS_I32), "int64": (torch.int64, _lib.IDS_I64)}


@functools.lru_cache(None)
def chunk():
    """c: COATTN_EMBEDDING_CHUNK as include/coattn.h defines it."""
    return int(re.search(r"^#define COATTN_EMBEDDING_CHUNK (\d+)", header(), re.M).group(1))


def _padded(B, T, V, g, lens=None):
    """[B, T] ids in [1, V) with zeros (the pad id) past each row's length."""
    ids = torch.randint(1, V, (B, T), generator=g)
    lens = torch.randint(1, T + 1, (B,), generator=g) if lens is None else torch.as_tensor(lens)
    ids[torch.arange(T)[None, :] >= lens[:, None]] = 0
    return ids.reshape(-1)


def _ids(name, g):
    c = chunk()
    hot = {"hot_c_minus_1": c - 1, "hot_c": c, "hot_c_plus_1": c + 1, "hot_2c_plus_1": 2 * c + 1}
    if name == "smallest":
        return torch.tensor([1]), 2, 4, 0
    if name in ("repeats", "no_padding_idx"):
        return _padded(3, 5, 7, g, lens=[5, 3, 1]), 7, 36, (0 if name == "repeats" else -1)
    if name in hot:
        return torch.full((hot[name],), 2), 3, 8, 0
    if name == "mostly_absent":
        ids = torch.randint(1, 4099, (130,), generator=g)
        ids[5], ids[77], ids[129], ids[9], ids[10] = 4098, 4098, 1, 0, 0
        return ids, 4099, 32, 0
    if name == "widest_row":
        return _padded(4, 16, 5, g), 5, 2048, 0
    if name == "cfg2_hot_token":
        ids = _padded(160, 26, 10000, g).view(160, 26)
        ids[:150, 0] = 7                                        # "what" opens 150 of the 160 questions
        return ids.reshape(-1), 10000, 512, 0
    assert name == "all_padding", name
    return torch.zeros(40, dtype=torch.int64), 7, 8, 0


CASES = ("smallest", "repeats", "hot_c_minus_1", "hot_c", "hot_c_plus_1", "hot_2c_plus_1", "mostly_absent", "widest_row",
         "cfg2_hot_token", "all_padding", "no_padding_idx")


@functools.lru_cache(None)
def make_case(name):
    """Inputs on the host, made once and shared (treat as read-only): ids int64 [n], W [V, E], g_out [n, E], padding_idx."""
    g = torch.Generator().manual_seed(4000 + CASES.index(name))
    ids, V, E, pad = _ids(name, g)
    n = ids.numel()
    return dict(name=name, n=n, V=V, E=E, pad=pad, ids=ids.to(torch.int64), W=torch.randn(V, E, generator=g),
                g_out=torch.randn(n, E, generator=g))


def live(c, ids=None):
    """[n] bool: the positions that contribute (id in [0, V) and not padding_idx)."""
    ids = c["ids"] if ids is None else ids
    return (ids >= 0) & (ids < c["V"]) & (ids != c["pad"])


def ordered_sum(ids, g_out, V, pad, base=None):
    """dW [V, E] in float32 by the order include/coattn.h states: the occurrences of a token ascend by flat position, chunks
    of c consecutive ones are summed serially from their first element, the chunk sums are combined left to right from the
    first; rows without an occurrence are +0.  `base`: accumulate onto it with one more rounding (rows without an occurrence
    keep their bits)."""
    c = chunk()
    as_np = lambda t, dt: (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(dt)      # noqa: E731 (a copy)
    ids, g = as_np(ids, np.int64), as_np(g_out, np.float32)
    dW = np.zeros((V, g.shape[1]), dtype=np.float32) if base is None else as_np(base, np.float32)
    with np.errstate(all="ignore"):
        for v in np.unique(ids):
            if v < 0 or v >= V or v == pad:
                continue
            pos = np.nonzero(ids == v)[0]                           # ascending
            total = None
            for k in range(0, len(pos), c):
                s = g[pos[k]].copy()
                for p in pos[k + 1:k + c]:
                    s = s + g[p]
                total = s if total is None else total + s
            dW[v] = total if base is None else dW[v] + total
    return torch.from_numpy(dW)


def oracle(c, dtype=torch.float64, g_out=None):
    """(out, dW) of stock F.embedding and its autograd on the CPU for sum(out * g_out)."""
    W = c["W"].detach().clone().to(dtype).requires_grad_(True)       # (a copy: .to() of the same dtype is the case's own tensor)
    out = F.embedding(c["ids"], W, padding_idx=c["pad"] if c["pad"] >= 0 else None)
    (out * (c["g_out"] if g_out is None else g_out).to(dtype)).sum().backward()
    return out.detach(), W.grad


@functools.lru_cache(None)
def references(name):
    """(out64, dW64, dW32 of stock fp32, ordered_sum) of a case, computed once."""
    c = make_case(name)
    out64, dW64 = oracle(c)
    return out64, dW64, oracle(c, torch.float32)[1], ordered_sum(c["ids"], c["g_out"], c["V"], c["pad"])


def _put(t):
    a = Arena(t.numel(), fill=None)
    a.body.copy_(t.reshape(-1))
    return a


def _put_ids(ids, kind):
    tdt, _ = IDS[kind]
    n = ids.numel()
    a = Arena(n * (2 if tdt == torch.int64 else 1), fill=None)
    a.body.view(tdt).copy_(ids.to(tdt))
    return a


def run(c, kind="int64", ids=None, g_out=None, accumulate=0, prefill=None, flags=0, dtype=_lib.F32, ids_dtype=None, pad=None,
        dims=None, forward=True, backward=True, expect_rc=0):
    """One coattn_embedding_forward (+ coattn_embedding_backward) on case `c` straight through the C-ABI; `ids`, `g_out`,
    `pad` replace the case's, `dims` = (n, V, E) the sizes the call is told (the buffers keep the case's).  Every buffer is
    an arena of its exact size; out and dW start as NaN (dW as `prefill` with accumulate = 1).  Checks every arena's margins
    afterwards.  Returns out, dW, the bad-id count and "rc" on the host."""
    lib = _lib.load()
    n, V, E = c["n"], c["V"], c["E"]
    ids = c["ids"] if ids is None else ids
    ar = {"ids": _put_ids(ids, kind), "W": _put(c["W"]), "g_out": _put(c["g_out"] if g_out is None else g_out),
          "out": Arena(n * E), "dW": Arena(V * E), "bad": Arena(1, fill=None)}
    ar["bad"].body.view(torch.int32).zero_()
    if prefill is not None:
        ar["dW"].body.copy_(prefill.reshape(-1))
    nbytes = _lib.embedding_workspace_bytes(n, V, E)
    if nbytes:
        ar["ws"] = Arena((nbytes + 3) // 4)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    tn, tV, tE = (n, V, E) if dims is None else dims
    common = dict(ids=ar["ids"].body, ids_dtype=IDS[kind][1] if ids_dtype is None else ids_dtype, n=tn, V=tV, E=tE,
                  padding_idx=c["pad"] if pad is None else pad, dtype=dtype, flags=flags, stream=stream)
    rc_f = rc_b = None
    if forward:
        call = _lib.bind("coattn_embedding_forward", W=ar["W"].body, out=ar["out"].body, bad_ids=ar["bad"].body, **common)
        rc_f = call.fn(*call)
    if backward:
        call = _lib.bind("coattn_embedding_backward", g_out=ar["g_out"].body, dW=ar["dW"].body,
                         ws=ar["ws"].body if "ws" in ar else None, accumulate=accumulate, **common)
        rc_b = call.fn(*call)
    torch.cuda.synchronize()
    err = lib.coattn_last_error().decode()
    assert rc_f in (None, expect_rc) and rc_b in (None, expect_rc), (rc_f, rc_b, err)
    bad = int(ar["bad"].body.view(torch.int32).cpu()[0])
    for k, a in ar.items():
        a.check("embedding %s" % k)
    return dict(rc=(rc_f, rc_b), err=err, out=ar["out"].body.cpu().view(n, E), dW=ar["dW"].body.cpu().view(V, E), bad=bad)


def same_bits(a, b):
    return bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def bound_check(name, got, ref64, stock32, factor=8.0, floor_ulps=16.0):
    """(deviation of `got` from the float64 reference, the bound): at most `factor` times the deviation of stock fp32
    PyTorch on the same inputs, with a floor of `floor_ulps` fp32 ulps of the reference's largest magnitude."""
    err = float((got.double() - ref64).abs().max())
    stock = float((stock32.double() - ref64).abs().max())
    scale = float(ref64.abs().max())
    bound = max(factor * stock, floor_ulps * 2.0 ** -24 * scale)
    print("embedding bound %-16s err %.3e stock %.3e ratio %.2f floor %.3e scale %.3e"
          % (name, err, stock, err / max(stock, 1e-300), floor_ulps * 2.0 ** -24 * scale, scale))
    return err, bound

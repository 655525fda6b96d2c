"""The cached-feature gather's C-ABI (coattn_features_gather; csrc/features.hip) for the tests: the cases, a ctypes runner that
puts every device buffer of a call at its exact size inside a marker-filled arena with the output pre-filled with NaN, and the
oracle -- `table[idx]` viewed as bits and shifted in numpy, zero rows for the indices outside the table -- never the code under
test.  Everything is compared as 32-bit patterns: a NaN equals itself only when its payload does."""
import functools
import re

import numpy as np
import torch

from vqa_amd import _lib

from tests._general import Arena
from tests._header import header

IDX = {"int32": (torch.int32, _lib.IDS_I32), "int64": (torch.int64, _lib.IDS_I64)}
TABLE = {"fp32": (_lib.F32, np.uint32, 4), "bf16": (_lib.BF16, np.uint16, 8)}      # (dtype code, bit type, elements per 16 bytes)
SHAPES = ((5, 1, 1, 8), (5, 3, 3, 8), (7, 33, 49, 64), (4, 3, 49, 512), (3, 2, 196, 512))      # (S, B, N, d)


@functools.lru_cache(None)
def constants():
    """(threads, loads): COATTN_FEATURES_THREADS and COATTN_FEATURES_LOADS as include/coattn.h defines them."""
    return tuple(int(re.search(r"^#define COATTN_FEATURES_%s (\d+)" % n, header(), re.M).group(1)) for n in ("THREADS", "LOADS"))


def pass_elements(dtype):
    """Elements of a table row that one workgroup copies: threads x loads 16-byte vectors."""
    threads, loads = constants()
    return threads * loads * TABLE[dtype][2]


@functools.lru_cache(None)
def table_bits(dtype, S, N, d, seed=0):
    """[S, N, d] bit patterns of a table of N(0,1) values (read-only: shared between tests)."""
    g = torch.Generator().manual_seed(7000 + seed)
    t = torch.randn(S, N, d, generator=g)
    if dtype == "bf16":
        bits = t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    else:
        bits = t.view(torch.int32).numpy().view(np.uint32)
    bits.setflags(write=False)
    return bits


def indices(S, B, seed=0):
    """B indices in [0, S), every one of them when B >= S (so that some repeat), made once per (S, B)."""
    g = torch.Generator().manual_seed(7100 + seed)
    return torch.randint(0, S, (B,), generator=g).numpy().astype(np.int64)


def oracle(bits, idx, dtype):
    """uint32 [B, N, d]: the fp32 bit patterns of table[idx] -- a bf16 table's 16 bits shifted into the high half -- and rows of
    zero bits where the index lies outside [0, S); plus the number of such indices."""
    S = bits.shape[0]
    idx = np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < S)
    rows = bits[np.where(ok, idx, 0)]
    out = (rows.astype(np.uint32) << np.uint32(16)) if dtype == "bf16" else rows.astype(np.uint32)
    out[~ok] = 0
    return out, int((~ok).sum())


def _put_bits(bits):
    """A host array of 16- or 32-bit patterns in an arena of its exact byte size."""
    raw = torch.from_numpy(np.ascontiguousarray(bits).reshape(-1).view(np.int16 if bits.dtype == np.uint16 else np.int32).copy())
    assert raw.numel() * raw.element_size() % 4 == 0
    a = Arena(raw.numel() * raw.element_size() // 4, fill=None)
    a.body.view(raw.dtype).copy_(raw)
    return a


def _put_idx(idx, kind):
    tdt, _ = IDX[kind]
    t = torch.from_numpy(np.asarray(idx, dtype=np.int64))
    if tdt == torch.int32:
        t = t.to(torch.int32)                                   # (callers keep int32 cases inside int32's range)
    a = Arena(t.numel() * (2 if tdt == torch.int64 else 1), fill=None)
    a.body.view(tdt).copy_(t)
    return a


def run(bits, idx, dtype, kind="int64", dims=None, flags=0, table_dtype=None, idx_dtype=None, bad=True, expect_rc=0):
    """One coattn_features_gather on the table `bits` ([S, N, d] patterns of `dtype`) and the indices `idx` straight through
    the C-ABI; `dims` = (S, B, N, d) the sizes the call is told (the buffers keep their own).  Every buffer is an arena of its
    exact size, out starts as NaN; the margins of every arena are checked afterwards.  Returns out as uint32 [B, N, d], the
    bad-index count and the return code on the host."""
    lib = _lib.load()
    S, N, d = bits.shape
    B = len(idx)
    ar = {"table": _put_bits(bits), "idx": _put_idx(idx, kind), "out": Arena(B * N * d), "bad": Arena(1, fill=None)}
    ar["bad"].body.view(torch.int32).zero_()
    tS, tB, tN, td = (S, B, N, d) if dims is None else dims
    call = _lib.bind("coattn_features_gather", table=ar["table"].body, table_dtype=TABLE[dtype][0] if table_dtype is None else table_dtype,
                     idx=ar["idx"].body, idx_dtype=IDX[kind][1] if idx_dtype is None else idx_dtype, out=ar["out"].body,
                     bad_idx=ar["bad"].body if bad else None, S=tS, B=tB, N=tN, d=td, flags=flags,
                     stream=torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)
    rc = call.fn(*call)
    torch.cuda.synchronize()
    err = lib.coattn_last_error().decode()
    assert rc == expect_rc, (rc, err)
    for k, a in ar.items():
        a.check("features_gather %s" % k)
    out = ar["out"].body.view(torch.int32).cpu().numpy().view(np.uint32).reshape(B, N, d)
    return dict(rc=rc, err=err, out=out, bad=int(ar["bad"].body.view(torch.int32).cpu()[0]))


def same(a, b):
    """torch.equal on the bit patterns of two uint32 / float arrays or tensors."""
    as_t = lambda x: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x).view(np.int32))).cpu()      # noqa: E731
    a, b = as_t(a), as_t(b)
    a = a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a
    b = b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b
    return a.shape == b.shape and torch.equal(a, b)

"""Feature dropout (coattn_dropout_forward / coattn_dropout_backward; csrc/dropout.hip) for the tests: the mask definition of
include/coattn.h restated in numpy -- Philox4x32-10 on (block, step, seed), the threshold, the scale, the float multiply --,
never the code under test, and a ctypes runner that puts every device buffer of a call at its exact size inside a marker-filled
arena with the outputs pre-filled with NaN and checks every margin afterwards."""
import functools
import struct

import numpy as np
import torch

from vqa_amd import _lib

from tests._general import GUARD_BITS, Arena

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
U32 = 0xFFFFFFFF
SEED = 1234                                    # the GPU tests' seed (tests/test_dropout_cpu.py holds its keep fractions)
SEED_HI = (0x9E3779B9 << 32) | 1234            # ... and one with a non-zero high word
P_MAX = float(np.nextafter(np.float32(1.0), np.float32(0.0)))     # the largest float below 1
PS = (0.0, 0.1, 0.5, 0.9, P_MAX)
WG = 1024                                      # elements one workgroup covers (256 threads, one 4-word block each)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> four uint32 arrays.  Ten rounds, the key bumped
    between them."""
    c = [np.asarray(x, dtype=np.uint64) & U32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & U32, int(key[1]) & U32
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)             # 32 x 32 -> 64 bits: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & U32, p1 >> np.uint64(32), p1 & U32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & U32, (k1 + W1) & U32
    return [x.astype(np.uint32) for x in c]


def random_words(n, seed, step):
    """r[i] for i < n: word i & 3 of the block i >> 2 under (step, seed), both taken as 64-bit numbers."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    j = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((j & U32, j >> np.uint64(32), step & U32, step >> 32), (seed & U32, seed >> 32))
    return np.stack(words, axis=1).reshape(-1)[:n]


def f32(p):
    """p as the C-ABI's float argument receives it."""
    return float(np.float32(p))


def thr(p):
    return int(np.floor(np.float64(f32(p)) * 4294967296.0))


def scale(p):
    return np.float32(1.0 / (1.0 - np.float64(f32(p))))


@functools.lru_cache(None)
def keep(n, seed, step, p):
    """[n] bool: element kept (shared and read-only)."""
    k = random_words(n, seed, step) >= np.uint32(thr(p))
    k.setflags(write=False)
    return k


def multiplier(n, seed, step, p):
    """[n] float32: scale where kept, +0 where dropped."""
    return np.where(keep(n, seed, step, p), scale(p), np.float32(0.0)).astype(np.float32)


def apply(x, seed, step, p):
    """y = x * multiplier as a float32 multiply (x: tensor or array of any shape, flattened in C order)."""
    a = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(np.float32)
    with np.errstate(all="ignore"):
        y = a.reshape(-1) * multiplier(a.size, seed, step, p)
    return torch.from_numpy(y.reshape(a.shape))


def _bits(t):
    """int32 view with every NaN as one pattern: the contract says where a NaN stands, not which one (inf * 0 is 0x7FC00000
    on the GPU and 0xFFC00000 on an x86 host)."""
    t = (t if torch.is_tensor(t) else torch.from_numpy(np.asarray(t))).detach().contiguous()
    return torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t).view(torch.int32)


def same_bits(a, b):
    """Equal bit for bit -- the sign of a zero and every denormal included -- with a NaN equal to any NaN."""
    return bool((_bits(a) == _bits(b)).all())


def state_words(seed, step):
    """The 32-byte state as eight int32 words: seed lo, hi, step lo, hi, four zero words."""
    b = struct.pack("<QQ16x", int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1))
    return torch.frombuffer(bytearray(b), dtype=torch.int32).clone()


def special_values(n, gen_seed=0):
    """[n] float32 normal values with NaN, +-inf, -0, +0, denormals and a negative value cycled in at fixed places."""
    g = torch.Generator().manual_seed(9000 + gen_seed)
    x = torch.randn(n, generator=g)
    sp = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, 0.0, 1e-40, -1e-40, 2.0 ** -149, -3.5, 3.0e38])
    idx = torch.arange(0, n, 3)
    x[idx] = sp[(idx // 3) % len(sp)]
    return x


class State:
    """A state in an arena of its own (eight words exactly)."""

    def __init__(self, seed, step=0):
        self.arena = Arena(8, fill=None)
        self.set(seed, step)

    def set(self, seed, step):
        self.arena.body.view(torch.int32).copy_(state_words(seed, step))

    def words(self):
        return self.arena.body.view(torch.int32).cpu()

    def step(self):
        w = self.words().numpy().astype(np.int64) & U32
        return int(w[2]) | (int(w[3]) << 32)

    def check(self, seed):
        w = self.words().numpy().astype(np.int64) & U32
        assert (int(w[0]) | (int(w[1]) << 32)) == int(seed) & (2 ** 64 - 1), "the seed words changed"
        assert not w[4:].any(), "the library's words are not back at zero: %s" % (w[4:],)
        self.arena.check("dropout state")


def _place(values, n, shift_bytes, inplace_of=None):
    """An arena holding n floats `shift_bytes` behind a 16-byte boundary (the arena is n + shift floats; the cells in front keep
    the marker).  values None: NaN-filled (an output)."""
    if inplace_of is not None:
        return inplace_of
    s = shift_bytes // 4
    a = Arena(n + s, fill=None)
    a.buf = a.body[s:]
    a.shift = s
    if values is None:
        a.buf.fill_(float("nan"))
    else:
        a.buf.copy_(values.reshape(-1))
    return a


def _check_arena(a, what):
    a.check(what)
    if a.shift:
        assert bool((a.body[:a.shift].view(torch.int32) == GUARD_BITS).all()), "%s: a word in front of the shifted buffer changed" % what


def forward(x0, p, state, x1=None, advance=1, inplace=False, shifts=(0, 0, 0, 0), n=None, expect_rc=0):
    """One coattn_dropout_forward straight through the C-ABI.  x0 (and x1): host tensors; shifts: byte offsets (multiples of 4)
    of x0, y0, x1, y1 from a 16-byte boundary; inplace: y is x.  Returns (y0, y1 or None) on the host."""
    lib = _lib.load()
    m = x0.numel()
    ax0 = _place(x0, m, shifts[0])
    ay0 = _place(None, m, shifts[1], ax0 if inplace else None)
    ax1 = ay1 = None
    if x1 is not None:
        ax1 = _place(x1, m, shifts[2])
        ay1 = _place(None, m, shifts[3], ax1 if inplace else None)
    pair1 = dict(x1=ax1.buf, y1=ay1.buf) if x1 is not None else {}
    call = _lib.bind("coattn_dropout_forward", x0=ax0.buf, y0=ay0.buf, n=m if n is None else n, p=p, state=state.arena.body,
                     advance=advance, stream=torch.cuda.current_stream().cuda_stream, **pair1)
    rc = call.fn(*call)
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, lib.coattn_last_error().decode())
    for name, a in (("x0", ax0), ("y0", ay0), ("x1", ax1), ("y1", ay1)):
        if a is not None:
            _check_arena(a, "dropout forward %s" % name)
    return ay0.buf.cpu().clone(), (ay1.buf.cpu().clone() if ay1 is not None else None)


def backward(g, p, state, inplace=False, shifts=(0, 0), expect_rc=0):
    """One coattn_dropout_backward: dx on the host."""
    lib = _lib.load()
    m = g.numel()
    ag = _place(g, m, shifts[0])
    ad = _place(None, m, shifts[1], ag if inplace else None)
    call = _lib.bind("coattn_dropout_backward", g=ag.buf, dx=ad.buf, n=m, p=p, state=state.arena.body,
                     stream=torch.cuda.current_stream().cuda_stream)
    rc = call.fn(*call)
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, lib.coattn_last_error().decode())
    _check_arena(ag, "dropout backward g")
    _check_arena(ad, "dropout backward dx")
    return ad.buf.cpu().clone()


# ---- what the GPU tests draw (tests/test_dropout_cpu.py holds the oracle's keep fraction of every one) ----------------------
SIZES = (1, 2, 3, 4, 5, 7, 8, WG - 1, WG, WG + 1, 3 * WG + 5)      # ... the last: four workgroups, a tail of one element
STATE_N = 2 * WG + 3                                               # three workgroups: the ticket is drawn more than once
STATE_STEP = 5
FN_SHAPE = (3, 256)                                                # the autograd function's tensor: n = 768
NET_DIMS = dict(B=12, N=49, T=26, d=256, mlp=128, K=19)            # the smallest shape of tests/test_gpu_graph.py
NET_N = 3 * NET_DIMS["B"] * NET_DIMS["d"]
P_NET = 0.5


def used_masks():
    """Every (seed, step, n, p) a GPU test compares against the oracle."""
    out = [(SEED, 1, n, p) for n in SIZES for p in PS]
    out += [(SEED_HI, s, STATE_N, 0.5) for s in (STATE_STEP + 1, STATE_STEP + 2, STATE_STEP + 3, 2 ** 32)]
    out += [(SEED, s, FN_SHAPE[0] * FN_SHAPE[1], p) for s in (1, 2) for p in (0.1, 0.5)]
    out += [(SEED, s, NET_N, P_NET) for s in (1, 2)]
    return out

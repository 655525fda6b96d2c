"""The attention overlays' C-ABI (coattn_overlay_render; csrc/overlay.hip) for the tests: the oracle -- the arithmetic that
include/coattn.h states, restated in numpy with every intermediate a float32, never the code under test --, the cases, and a
ctypes runner that puts every device buffer of a call at its exact size inside a marker-filled arena (tests/_general.py) with
the output pre-filled with a marker byte."""
import ctypes as C
import functools
import re

import numpy as np
import torch

from tests._header import header

F = np.float32
MARK = 0xCD                                       # what the output holds before the call
MEAN, STD = (-0.485, -0.356, -0.606), (2.29, 1.74, 2.25)      # x_hat ~ N(0.6, 0.5): both sides of the clamp are taken
ALPHA, FLOOR = 0.6, 0.3
MODES = {"heat": 0, "mask": 1}


@functools.lru_cache(None)
def constants():
    """(rows, threads): COATTN_OVERLAY_ROWS and COATTN_OVERLAY_THREADS as include/coattn.h defines them."""
    return tuple(int(re.search(r"^#define COATTN_OVERLAY_%s (\d+)" % n, header(), re.M).group(1)) for n in ("ROWS", "THREADS"))


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def clamp01(x):
    with np.errstate(invalid="ignore"):
        return np.where(x >= 0, np.where(x <= 1, x, F(1)), F(0)).astype(F)


def to_byte(o):
    return (clamp01(o) * F(255) + F(0.5)).astype(np.int32)


def normalise(a):
    """float32 [n] -> (a * (1 / max a) as float32 [n], bad); a bad row gives zeros."""
    a = np.asarray(a, dtype=F)
    with np.errstate(all="ignore"):
        bad = bool((~np.isfinite(a)).any() or (a < 0).any())
        mx = a.max()
        r = F(1) / mx
        bad = bad or bool(mx == 0) or not bool(np.isfinite(r))
        if bad:
            return np.zeros_like(a), True
        return (a * r).astype(F), False


def axis(G, extent):
    """(i0, i1, w0, w1) of every output coordinate along an axis of G cells stretched to `extent` pixels."""
    s = F(G) / F(extent)
    src = (np.arange(extent, dtype=F) + F(0.5)) * s - F(0.5)
    src = np.maximum(src, F(0)).astype(F)
    i0 = np.minimum(src.astype(np.int32), G - 1)
    i1 = np.minimum(i0 + 1, G - 1)
    w1 = (src - i0.astype(F)).astype(F)
    w0 = (F(1) - w1).astype(F)
    return i0, i1, w0, w1


def upsample(m, H, W):
    """float32 [Gh, Gw] -> float32 [H, W], bilinear with half-pixel centres and clamped edges."""
    m = np.asarray(m, dtype=F)
    i0, i1, wy0, wy1 = axis(m.shape[0], H)
    j0, j1, wx0, wx1 = axis(m.shape[1], W)
    top = (m[i0][:, j0] * wx0[None, :]).astype(F) + (m[i0][:, j1] * wx1[None, :]).astype(F)
    bot = (m[i1][:, j0] * wx0[None, :]).astype(F) + (m[i1][:, j1] * wx1[None, :]).astype(F)
    return ((top.astype(F) * wy0[:, None]).astype(F) + (bot.astype(F) * wy1[:, None]).astype(F)).astype(F)


def x_hat(image, mean=MEAN, std=STD):
    """float32 [B, 3, H, W] -> the de-normalised, clamped image [B, H, W, 3]."""
    with np.errstate(all="ignore"):
        x = np.asarray(image, dtype=F) * np.asarray(std, dtype=F)[None, :, None, None] + np.asarray(mean, dtype=F)[None, :, None, None]
    return clamp01(x.astype(F)).transpose(0, 2, 3, 1)


def blend(xh, u, mode, alpha, floor, lut):
    """xh float32 [H, W, 3], u float32 [H, W] -> the bytes [H, W, 3] of one level's panel."""
    if mode == "mask":
        g = (F(floor) + ((F(1) - F(floor)) * u).astype(F)).astype(F)
        return to_byte((xh * g[:, :, None]).astype(F))
    k = (u * F(255) + F(0.5)).astype(np.int32)
    return to_byte(((F(1) - F(alpha)) * xh).astype(F) + (F(alpha) * np.asarray(lut, dtype=F)[k]).astype(F))


def oracle(image, a_v, a_q, q_len, Gh, Gw, mode, strip, alpha=ALPHA, floor=FLOOR, mean=MEAN, std=STD, lut=None):
    """uint8 [B, L+1, H+strip, W, 3] and the number of bad maps, as include/coattn.h states them."""
    B, _, H, W = image.shape
    L = a_v.shape[0]
    out = np.zeros((B, L + 1, H + strip, W, 3), dtype=np.uint8)
    xh = x_hat(image, mean, std)
    n_bad = 0
    for b in range(B):
        out[b, 0, :H] = to_byte(xh[b])
        for l in range(L):
            m, bad = normalise(a_v[l, b])
            n_bad += bad
            out[b, 1 + l, :H] = blend(xh[b], upsample(m.reshape(Gh, Gw), H, W), mode, alpha, floor, lut)
            if not strip:
                continue
            T = a_q.shape[2]
            n = T if q_len is None else min(max(int(q_len[b]), 1), T)
            mq, bad = normalise(a_q[l, b, :n])
            n_bad += bad
            t = (np.arange(W, dtype=np.int64) * T) // W
            live = t < n
            mq = np.concatenate([mq, np.zeros(T - n, dtype=F)])[t]
            if mode == "mask":
                row = np.repeat(to_byte(mq)[:, None], 3, 1)
            else:
                row = to_byte(np.asarray(lut, dtype=F)[(mq * F(255) + F(0.5)).astype(np.int32)])
            out[b, 1 + l, H:] = np.where(live[:, None], row, 0)[None]
    return out, n_bad


# ---- the cases ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def case(B, L, H, W, Gh, Gw, T, seed=0):
    """(image [B,3,H,W], a_v [L,B,Gh*Gw], a_q [L,B,T], q_len [B]) as read-only float32 / int64 arrays: the image N(0.5, 0.25),
    the maps softmaxes of 3 N(0,1) logits, the lengths in [1, T]."""
    g = torch.Generator().manual_seed(8000 + seed)
    image = torch.randn(B, 3, H, W, generator=g) * 0.25 + 0.5
    a_v = torch.softmax(torch.randn(L, B, Gh * Gw, generator=g) * 3, dim=2)
    a_q = torch.softmax(torch.randn(L, B, T, generator=g) * 3, dim=2)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    arrs = tuple(t.numpy() for t in (image, a_v, a_q, lens))
    for a in arrs:
        a.setflags(write=False)
    return arrs


@functools.lru_cache(None)
def user_lut(seed=0):
    lut = torch.rand(256, 3, generator=torch.Generator().manual_seed(8100 + seed)).numpy()
    lut.setflags(write=False)
    return lut


def default_lut():
    from vqa_amd import overlay
    return overlay.lut_values()


# ---- the runner ---------------------------------------------------------------------------------------------------------------
LAYOUTS = ("nchw", "nhwc", "pad4", "pad1")


def image_geometry(B, H, W, layout):
    """(floats of the buffer, (sB, sC, sH, sW)) of the [B,3,H,W] view a layout hands to the C-ABI.  nchw: contiguous; nhwc:
    channels-last; pad4: rows W + 4 floats apart (still 16-byte loads); pad1: rows W + 1 apart (element loads at sW = 1)."""
    if layout == "nchw":
        return B * 3 * H * W, (3 * H * W, H * W, W, 1)
    if layout == "nhwc":
        return B * 3 * H * W, (3 * H * W, 1, 3 * W, 3)
    pad = {"pad4": 4, "pad1": 1}[layout]
    return B * 3 * H * (W + pad), (3 * H * (W + pad), H * (W + pad), W + pad, 1)


def params(lut_ptr, alpha=ALPHA, floor=FLOOR, mean=MEAN, std=STD):
    from vqa_amd import _lib
    return _lib.OverlayParams((C.c_float * 3)(*mean), (C.c_float * 3)(*std), alpha, floor, lut_ptr)


def run(image, a_v, a_q, q_len, Gh, Gw, mode, strip, layout="nchw", alpha=ALPHA, floor=FLOOR, mean=MEAN, std=STD, lut=None,
        bad=True, bad_start=0, expect_rc=0):
    """One coattn_overlay_render straight through the C-ABI on host arrays (a_q, q_len may be None).  Every buffer is an arena
    of its exact size, out starts as MARK bytes; the margins of every arena, and the padding of a padded image, are checked
    afterwards.  Returns the bytes [B, L+1, H+strip, W, 3], the counter and the return code on the host."""
    from vqa_amd import _lib
    from tests._general import Arena
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, _, H, W = image.shape
    L = a_v.shape[0]
    T = a_q.shape[2] if a_q is not None else 1
    n_img, strides = image_geometry(B, H, W, layout)
    ar = {"image": Arena(n_img, fill=None), "a_v": Arena(a_v.size, fill=None), "out": Arena(B * (L + 1) * (H + strip) * W * 3 // 4, fill=None),
          "bad": Arena(1, fill=None)}
    view = torch.as_strided(ar["image"].body, (B, 3, H, W), strides, ar["image"].body.storage_offset())
    view.copy_(torch.from_numpy(np.array(image, dtype=F)))
    ar["image"].view = view
    ar["a_v"].body.copy_(torch.from_numpy(np.array(a_v, dtype=F)).reshape(-1))
    ar["out"].body.view(torch.uint8).fill_(MARK)
    ar["bad"].body.view(torch.int32).fill_(bad_start)
    if a_q is not None:
        ar["a_q"] = Arena(a_q.size, fill=None)
        ar["a_q"].body.copy_(torch.from_numpy(np.array(a_q, dtype=F)).reshape(-1))
    if q_len is not None:
        ar["q_len"] = Arena(B, fill=None)
        ar["q_len"].body.view(torch.int32).copy_(torch.from_numpy(np.asarray(q_len, dtype=np.int32)))
    if mode == "heat":
        ar["lut"] = Arena(768, fill=None)
        ar["lut"].body.copy_(torch.from_numpy(np.array(lut, dtype=F)).reshape(-1))
    p = params(ar["lut"].body.data_ptr() if mode == "heat" else None, alpha, floor, mean, std)
    call = _lib.bind("coattn_overlay_render", image=view, sB=strides[0], sC=strides[1], sH=strides[2], sW=strides[3],
                     a_v=ar["a_v"].body, a_q=ar["a_q"].body if a_q is not None else None,
                     q_len=ar["q_len"].body if q_len is not None else None, p=p, out=ar["out"].body,
                     bad_maps=ar["bad"].body if bad else None, B=B, L=L, H=H, W=W, Gh=Gh, Gw=Gw, T=T, strip_h=strip,
                     mode=MODES[mode], stream=torch.cuda.current_stream(dev).cuda_stream)
    rc = call.fn(*call)
    torch.cuda.synchronize()
    err = lib.coattn_last_error().decode()
    assert rc == expect_rc, (rc, err)
    for k, a in ar.items():
        a.check("overlay_render %s" % k)
    out = ar["out"].body.view(torch.uint8).cpu().numpy().reshape(B, L + 1, H + strip, W, 3)
    return dict(rc=rc, err=err, out=out, bad=int(ar["bad"].body.view(torch.int32).cpu()[0]))


def run_case(shape, mode, layout="nchw", lens=True, seed=0, **kw):
    """run() and oracle() on case(*shape): (result, expected bytes, expected bad count)."""
    B, L, H, W, Gh, Gw, T, strip = shape
    image, a_v, a_q, q_len = case(B, L, H, W, Gh, Gw, T, seed)
    lut = kw.pop("lut", default_lut()) if mode == "heat" else None
    if not strip:
        a_q = q_len = None
    if not lens:
        q_len = None
    res = run(image, a_v, a_q, q_len, Gh, Gw, mode, strip, layout=layout, lut=lut, **kw)
    want, n_bad = oracle(image, a_v, a_q, q_len, Gh, Gw, mode, strip, lut=lut,
                         **{k: v for k, v in kw.items() if k in ("alpha", "floor", "mean", "std")})
    return res, want, n_bad


def read_png(path):
    """uint8 [H, W, 3] of an 8-bit RGB PNG without interlacing, decoded here: the chunks walked and their CRCs checked, the
    IDAT stream inflated, the five scanline filters undone."""
    import struct
    import zlib
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        n, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + data) & 0xFFFFFFFF, kind
        chunks.append((kind, data))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(b"".join(d for k, d in chunks if k == b"IDAT")), dtype=np.uint8).reshape(H, 1 + 3 * W)
    out = np.zeros((H, 3 * W), dtype=np.uint8)
    for y in range(H):
        f, line = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        up = out[y - 1].astype(np.int32) if y else np.zeros(3 * W, np.int32)
        if f == 0:
            out[y] = line
        elif f == 2:
            out[y] = (line + up) & 255
        else:                                                # sub, average, Paeth: byte by byte along the line
            cur = np.zeros(3 * W, np.int32)
            for i in range(3 * W):
                a = cur[i - 3] if i >= 3 else 0
                b, c = up[i], (up[i - 3] if i >= 3 else 0)
                if f == 1:
                    pred = a
                elif f == 3:
                    pred = (a + b) // 2
                else:
                    assert f == 4, f
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[i] = (line[i] + pred) & 255
            out[y] = cur
    return out.reshape(H, W, 3)


def diff(got, want):
    """A short account of where two byte arrays differ (for an assertion message)."""
    ne = np.argwhere(got != want)
    return "%d of %d bytes differ; first at %s: got %s, want %s" % (
        len(ne), got.size, ne[:3].tolist(), [int(got[tuple(i)]) for i in ne[:3]], [int(want[tuple(i)]) for i in ne[:3]])

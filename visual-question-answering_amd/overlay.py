"""Attention overlays: the maps ``forward_with_attention`` returns, drawn over the images they were computed from --
``render_attention``: every level's image attention upsampled bilinearly to the image's size and blended into the
de-normalised image, with a strip of the question attention under it, as uint8 pictures in one HIP launch per batch
(``csrc/overlay.hip``, ``coattn_overlay_render`` of ``include/coattn.h``, whose comment states the arithmetic operation by
operation); ``write_png`` and ``sheet`` to put them into files with the standard library alone.  DESIGN.md section 3.17.

There is no CPU route: CPU tensors raise.  Text rendering of the question's words, other upsampling filters and overlays from
cached features (which have no pixels) are not offered.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np
import torch

from . import _lib

IMAGENET_MEAN = (0.485, 0.456, 0.406)          # the reference's transforms.Normalize (main.py:126)
IMAGENET_STD = (0.229, 0.224, 0.225)
MODES = {"heat": _lib.OVERLAY_HEAT, "mask": _lib.OVERLAY_MASK}


def supported(B, L, H, W, Gh, Gw, T=1, strip=0, mode="heat") -> bool:
    """Does the HIP kernel take this shape (include/coattn.h coattn_overlay_supported)?  No GPU call."""
    return mode in MODES and bool(_lib.load().coattn_overlay_supported(B, L, H, W, Gh, Gw, T, strip, MODES[mode]))


def lut_values() -> np.ndarray:
    """float32 [256, 3]: the heat mode's default colours, a blue -> red -> yellow ramp over t = k / 255:
    r = clip(2 t, 0, 1), g = clip(2 t - 1, 0, 1), b = clip(1 - 2 t, 0, 1)."""
    t = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.stack([np.clip(2 * t, 0, 1), np.clip(2 * t - 1, 0, 1), np.clip(1 - 2 * t, 0, 1)], 1).astype(np.float32)


_luts = {}                    # device index -> the default table on that device
_bad = {}                     # device index -> int32[1] counter the renders add to


def _key(dev):
    return dev.index if dev.index is not None else torch.cuda.current_device()


def default_lut(device="cuda") -> torch.Tensor:
    """`lut_values()` on `device`, made once per device."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("default_lut: the overlay kernel runs on the GPU; got device %s" % device)
    key = _key(device)
    lut = _luts.get(key)
    if lut is None:
        lut = _luts[key] = torch.from_numpy(lut_values()).to(torch.device("cuda", key))
    return lut


def _counter(dev):
    key = _key(dev)
    c = _bad.get(key)
    if c is None:
        c = _bad[key] = torch.zeros(1, device=torch.device("cuda", key), dtype=torch.int32)
    return c


def bad_maps() -> int:
    """How many maps the renders of this process could not normalise (a NaN, an infinity, a negative entry, a zero or a
    denormal maximum: each was drawn as an all-zero map) since the last call, over all devices; clears the count.
    Synchronises every device it reads."""
    total = 0
    for key, c in _bad.items():
        torch.cuda.synchronize(key)
        total += int(c.item())
        c.zero_()
        torch.cuda.synchronize(key)
    return total


def render_attention(image, a_v, a_q=None, ques_len=None, *, grid=None, mode="heat", alpha=0.6, floor=0.3,
                     mean=IMAGENET_MEAN, std=IMAGENET_STD, lut=None, strip=0):
    """image fp32 [B, 3, H, W] (any strides: NCHW, channels-last, a view), a_v fp32 [L, B, N] and a_q fp32 [L, B, T] as
    ``forward_with_attention`` returns them -> uint8 [B, L+1, H+strip, W, 3]: panel 0 the de-normalised image, panel 1+l
    level l's attention over it -- ``mode="heat"``: the colour ``lut[round(255 u)]`` at weight `alpha`; ``"mask"``: the image
    at brightness ``floor + (1 - floor) u`` -- with u the map divided by its maximum and upsampled bilinearly from the
    `grid` = (Gh, Gw) (default: the square root of N).  `strip` > 0 adds that many rows under every level's panel: the T
    cells of a_q divided by its maximum over the first `ques_len` positions, black past them.  `ques_len`: [B] of any integer
    dtype, on any device; it goes to the GPU as int32 and is never read on the host.  `lut`: fp32 [256, 3] in [0, 1] on the
    image's device (default: ``default_lut``).  One launch of coattn_overlay_render on the current stream; a map that cannot be
    normalised is drawn as zeros and counted (``bad_maps()``); a shape the kernel does not take is an error."""
    if mode not in MODES:
        raise ValueError("render_attention: mode must be one of %s, got %r" % (tuple(MODES), mode))
    if not (torch.is_tensor(image) and image.dim() == 4 and image.shape[1] == 3 and image.dtype == torch.float32):
        raise RuntimeError("render_attention takes an fp32 [B, 3, H, W] image; got %s %s"
                           % (getattr(image, "dtype", type(image)), tuple(getattr(image, "shape", ()))))
    if not (torch.is_tensor(a_v) and a_v.dim() == 3 and a_v.dtype == torch.float32 and a_v.shape[1] == image.shape[0]):
        raise RuntimeError("render_attention takes fp32 [L, B, N] image attention maps (B = %d); got %s %s"
                           % (image.shape[0], getattr(a_v, "dtype", type(a_v)), tuple(getattr(a_v, "shape", ()))))
    B, _, H, W = image.shape
    L, _, N = a_v.shape
    if grid is None:
        side = int(round(N ** 0.5))
        if side * side != N:
            raise ValueError("render_attention: %d locations are no square grid; pass grid=(Gh, Gw)" % N)
        grid = (side, side)
    Gh, Gw = (int(g) for g in grid)
    if Gh * Gw != N:
        raise ValueError("render_attention: grid %dx%d does not hold the maps' %d locations" % (Gh, Gw, N))
    strip = int(strip)
    if strip < 0:
        raise ValueError("render_attention: strip must be >= 0, got %d" % strip)
    if strip and a_q is None:
        raise ValueError("render_attention: strip=%d needs a_q" % strip)
    T = 1
    if a_q is not None:
        if not (torch.is_tensor(a_q) and a_q.dim() == 3 and a_q.dtype == torch.float32 and tuple(a_q.shape[:2]) == (L, B)):
            raise RuntimeError("render_attention takes fp32 [L, B, T] question attention maps (L = %d, B = %d); got %s %s"
                               % (L, B, getattr(a_q, "dtype", type(a_q)), tuple(getattr(a_q, "shape", ()))))
        T = a_q.shape[2]
    if ques_len is not None and (not torch.is_tensor(ques_len) or ques_len.dim() != 1 or ques_len.numel() != B
                                 or ques_len.is_floating_point() or ques_len.is_complex() or ques_len.dtype == torch.bool):
        raise RuntimeError("render_attention takes ques_len as a 1-D integer tensor of B = %d lengths" % B)
    if not image.is_cuda:
        raise RuntimeError("render_attention runs on the GPU (there is no CPU fallback); got an image on %s" % image.device)
    dev = image.device
    for name, t in (("a_v", a_v), ("a_q", a_q), ("lut", lut)):
        if t is not None and t.device != dev:
            raise RuntimeError("render_attention: image on %s, %s on %s" % (dev, name, t.device))
    if lut is not None and (lut.dtype != torch.float32 or tuple(lut.shape) != (256, 3)):
        raise RuntimeError("render_attention: lut must be an fp32 [256, 3] tensor; got %s %s" % (lut.dtype, tuple(lut.shape)))
    if not supported(B, L, H, W, Gh, Gw, T, strip, mode):
        raise RuntimeError("render_attention (HIP): shape B=%d L=%d H=%d W=%d grid=%dx%d T=%d strip=%d not supported (L <= 8, "
                           "H, W, strip <= 4096, W a multiple of 4, grid sides <= 64, T <= W under a strip: "
                           "coattn_overlay_supported)" % (B, L, H, W, Gh, Gw, T, strip))
    with _lib.on_device(dev):
        if mode == "heat":
            lut = default_lut(dev) if lut is None else lut.detach().contiguous()
        else:
            lut = None
        p = _lib.OverlayParams((_lib.C.c_float * 3)(*mean), (_lib.C.c_float * 3)(*std), float(alpha), float(floor),
                               lut.data_ptr() if lut is not None else None)
        qlen = None if ques_len is None else ques_len.to(device=dev, dtype=torch.int32).contiguous()
        out = torch.empty((B, L + 1, H + strip, W, 3), dtype=torch.uint8, device=dev)
        image = image.detach()
        sB, sC, sH, sW = image.stride()
        _lib.bind("coattn_overlay_render", image=image, sB=sB, sC=sC, sH=sH, sW=sW, a_v=a_v.detach().contiguous(),
                  a_q=a_q.detach().contiguous() if strip else None, q_len=qlen, p=p, out=out, bad_maps=_counter(dev),
                  B=B, L=L, H=H, W=W, Gh=Gh, Gw=Gw, T=T, strip_h=strip, mode=MODES[mode], stream=_lib.stream_ptr(dev))()
    return out


def sheet(panels):
    """uint8 [P, H, W, 3] (one sample of `render_attention`, tensor or array) -> [H, P W, 3]: the panels side by side."""
    if panels.ndim != 4 or panels.shape[3] != 3:
        raise ValueError("sheet takes [P, H, W, 3] panels; got %s" % (tuple(panels.shape),))
    P, H, W, _ = panels.shape
    if torch.is_tensor(panels):
        return panels.permute(1, 0, 2, 3).reshape(H, P * W, 3)
    return np.ascontiguousarray(np.transpose(panels, (1, 0, 2, 3))).reshape(H, P * W, 3)


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, pixels, level=6) -> None:
    """Write uint8 [H, W, 3] (tensor or array) as an 8-bit RGB PNG: zlib and struct of the standard library, every scanline
    with filter type 0."""
    if torch.is_tensor(pixels):
        pixels = pixels.detach().cpu().numpy()
    pixels = np.ascontiguousarray(pixels)
    if pixels.dtype != np.uint8 or pixels.ndim != 3 or pixels.shape[2] != 3 or pixels.shape[0] < 1 or pixels.shape[1] < 1:
        raise ValueError("write_png takes uint8 [H, W, 3] pixels; got %s %s" % (pixels.dtype, pixels.shape))
    H, W, _ = pixels.shape
    rows = np.zeros((H, 1 + 3 * W), dtype=np.uint8)
    rows[:, 1:] = pixels.reshape(H, 3 * W)
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
                 + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b""))

"""Image preprocessing: the reference's per-sample transform ``Resize((S, S)) -> ToTensor -> Normalize`` (main.py:126) for a
batch of decoded uint8 images of different sizes -- ``ImagePreprocessor``: one HIP launch per batch (``csrc/preprocess.hip``,
``coattn_preprocess_images`` of ``include/coattn_ext.h``, whose comment states the arithmetic operation by operation: Pillow's
8-bit bilinear resize bit for bit, then a table lookup); ``preprocess_host``: the same result through PIL and the same lookup
table, for CPU runs.  DESIGN.md section 3.18.

The GPU receives the decoded pixels: a batch travels as ONE uint8 buffer (``PackedBatch``) holding its descriptor rows, the
coefficient tables of the sizes that occur in it and the pixels, so that one copy and one launch serve it on any stream.

There is no CPU route through the kernel: a buffer or an output on the CPU raises.  JPEG decoding, augmentation and other
filters are not offered.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

IMAGENET_MEAN = (0.485, 0.456, 0.406)          # the reference's transforms.Normalize (main.py:126)
IMAGENET_STD = (0.229, 0.224, 0.225)
PRECISION_BITS = 22
DESC_DTYPE = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("tab_x", "<i4"), ("tab_y", "<i4"),
                       ("taps_x", "<i4"), ("taps_y", "<i4")])             # coattn_preprocess_desc
assert DESC_DTYPE.itemsize == C.sizeof(_lib.PreprocessDesc) == 32


def supported(B, S, max_h, max_w) -> bool:
    """Does the HIP kernel take this batch (include/coattn_ext.h coattn_preprocess_supported)?  No GPU call."""
    return bool(_lib.load().coattn_preprocess_supported(int(B), int(S), int(max_h), int(max_w)))


def axis_rows(n_in: int, S: int):
    """[(lo, [K_0 .. K_{n-1}])] for the S outputs of an axis of `n_in` samples: the header's coefficient contract, in IEEE
    double (Python floats), operation by operation."""
    n_in, S = int(n_in), int(S)
    if n_in < 1 or S < 1:
        raise ValueError("axis_rows: sizes must be positive, got %d -> %d" % (n_in, S))
    scale = n_in / S
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    rows = []
    for o in range(S):
        center = (o + 0.5) * scale
        lo = max(0, int(center - support + 0.5))
        hi = min(n_in, int(center + support + 0.5))
        w = [max(0.0, 1.0 - abs((j + lo - center + 0.5) * ss)) for j in range(hi - lo)]
        ww = 0.0
        for v in w:                                      # left to right
            ww += v
        ks = []
        for v in w:
            k = v / ww
            ks.append(int(-0.5 + k * (1 << PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << PRECISION_BITS)))
        rows.append((lo, ks))
    return rows


def axis_table(n_in: int, S: int) -> np.ndarray:
    """int32 [S, 2 + taps]: per output lo, the tap count and the taps, zero-padded to the widest row of this table."""
    rows = axis_rows(n_in, S)
    taps = max(1, max(len(ks) for _, ks in rows))
    tab = np.zeros((S, 2 + taps), dtype=np.int32)
    for o, (lo, ks) in enumerate(rows):
        tab[o, 0], tab[o, 1] = lo, len(ks)
        tab[o, 2:2 + len(ks)] = ks
    return tab


def lut_values(mean=IMAGENET_MEAN, std=IMAGENET_STD) -> torch.Tensor:
    """fp32 [3, 256] on the CPU: lut[c][u] = ((float(u) / 255) - mean_c) / std_c by torch's own operations -- the bits of
    ToTensor + Normalize."""
    mean = torch.as_tensor(mean, dtype=torch.float32).reshape(3, 1)
    std = torch.as_tensor(std, dtype=torch.float32).reshape(3, 1)
    if not bool(torch.isfinite(mean).all()) or not bool(torch.isfinite(std).all()) or bool((std == 0).any()):
        raise ValueError("preprocess: mean must be finite, std finite and non-zero")
    return torch.arange(256).float().div(255).unsqueeze(0).sub(mean).div(std).contiguous()


def _as_pixels(img, i):
    if torch.is_tensor(img):
        if img.device.type != "cpu":
            raise RuntimeError("preprocess: image %d is on %s; decoded images are packed on the host" % (i, img.device))
        img = img.numpy()
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("preprocess: image %d must be uint8 [h, w, 3]; got %s %s" % (i, img.dtype, img.shape))
    return img


def _up16(n):
    return (n + 15) & ~15


class PackedBatch:
    """A batch of images as one uint8 buffer: B descriptor rows at `desc_off`, `coef_count` int32 of coefficient tables at
    `coef_off`, `pix_bytes` of pixels at `pix_off` (every image on a 16-byte boundary; descriptor offsets count from `pix_off`).
    `buf` lives on the host (pinned on request) until ``to(device)``; `sizes` is the (h, w) of every image in packing order."""

    def __init__(self, buf, B, S, sizes, desc_off, coef_off, coef_count, pix_off, pix_bytes):
        self.buf, self.B, self.S, self.sizes = buf, B, S, sizes
        self.desc_off, self.coef_off, self.coef_count, self.pix_off, self.pix_bytes = desc_off, coef_off, coef_count, pix_off, pix_bytes
        self.max_h, self.max_w = max(h for h, _ in sizes), max(w for _, w in sizes)

    def desc(self) -> np.ndarray:
        """The descriptor rows of a host buffer, as a writable structured array (DESC_DTYPE)."""
        if self.buf.device.type != "cpu":
            raise RuntimeError("PackedBatch.desc: the buffer is on %s" % self.buf.device)
        return self.buf.numpy()[self.desc_off:self.desc_off + 32 * self.B].view(DESC_DTYPE)

    def permute(self, order) -> "PackedBatch":
        """Reorder the batch in place: image i of the result is image order[i] of before.  Descriptor rows move, pixels stay."""
        order = [int(i) for i in (order.tolist() if hasattr(order, "tolist") else order)]
        if sorted(order) != list(range(self.B)):
            raise ValueError("PackedBatch.permute: not a permutation of %d images" % self.B)
        d = self.desc()
        d[:] = d[order]
        self.sizes = [self.sizes[i] for i in order]
        return self

    def __getitem__(self, order) -> "PackedBatch":
        """``batch[order]`` with a permutation, as a tensor of images takes it (train.sort_batch): THIS batch, permuted."""
        return self.permute(order)

    def __len__(self):
        return self.B

    def with_buf(self, buf) -> "PackedBatch":
        """The same batch over another copy of its buffer (a pinned one, the device's)."""
        return PackedBatch(buf, self.B, self.S, list(self.sizes), self.desc_off, self.coef_off, self.coef_count, self.pix_off,
                           self.pix_bytes)

    def to(self, device, non_blocking=False) -> "PackedBatch":
        return self.with_buf(self.buf.to(device, non_blocking=non_blocking))


_bad = {}                     # device index -> int32[1] counter the launches add to


def _key(dev):
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _counter(dev):
    key = _key(dev)
    c = _bad.get(key)
    if c is None:
        c = _bad[key] = torch.zeros(1, device=torch.device("cuda", key), dtype=torch.int32)
    return c


def bad_images() -> int:
    """How many images the launches of this process refused (a descriptor outside the pixel buffer, a size outside the
    launch's limits, a coefficient table outside its buffer: each was written as zeros) since the last call, over all devices;
    clears the count.  Synchronises every device it reads."""
    total = 0
    for key, c in _bad.items():
        torch.cuda.synchronize(key)
        total += int(c.item())
        c.zero_()
        torch.cuda.synchronize(key)
    return total


class ImagePreprocessor:
    """Resize to S x S, scale to [0, 1] and normalise batches of decoded images on the GPU.  Owns the lookup table (on the
    device) and the coefficient tables of every source size it has met (on the host: a batch carries the tables it needs)."""

    def __init__(self, S, mean=IMAGENET_MEAN, std=IMAGENET_STD, device="cuda"):
        self.S = int(S)
        if self.S < 1:
            raise ValueError("ImagePreprocessor: S must be positive, got %d" % self.S)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ImagePreprocessor runs on the GPU (there is no CPU fallback; preprocess_host is the host "
                               "route); got device %s" % self.device)
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        self.lut = lut_values(self.mean, self.std).to(self.device)
        _counter(self.device)                            # (made here, not by the first launch on whatever stream that runs on)
        self._tables = {}                                # source size -> int32 [S, 2 + taps]

    def table(self, n_in: int) -> np.ndarray:
        tab = self._tables.get(n_in)
        if tab is None:
            tab = self._tables[n_in] = axis_table(n_in, self.S)
        return tab

    def pack(self, images, pin=False) -> PackedBatch:
        """A list of uint8 [h, w, 3] arrays (or CPU tensors) -> a host PackedBatch (in pinned memory on request)."""
        imgs = [_as_pixels(im, i) for i, im in enumerate(images)]
        if not imgs:
            raise ValueError("ImagePreprocessor.pack: an empty batch")
        B, S = len(imgs), self.S
        sizes = [(im.shape[0], im.shape[1]) for im in imgs]
        tabs, coef_count = {}, 0                         # source size -> (start in int32, table)
        for n_in in sorted({n for hw in sizes for n in hw}):
            tab = self.table(n_in)
            tabs[n_in] = (coef_count, tab)
            coef_count += tab.size
        desc_off = 0
        coef_off = _up16(32 * B)
        pix_off = _up16(coef_off + 4 * coef_count)
        offsets, pix_bytes = [], 0
        for h, w in sizes:
            offsets.append(pix_bytes)
            pix_bytes = _up16(pix_bytes + 3 * h * w)
        buf = torch.empty(pix_off + pix_bytes, dtype=torch.uint8, pin_memory=bool(pin))
        raw = buf.numpy()
        raw[:pix_off] = 0
        desc = raw[desc_off:desc_off + 32 * B].view(DESC_DTYPE)
        coef = raw[coef_off:coef_off + 4 * coef_count].view(np.int32)
        for start, tab in tabs.values():
            coef[start:start + tab.size] = tab.reshape(-1)
        for i, (im, (h, w), off) in enumerate(zip(imgs, sizes, offsets)):
            n = 3 * h * w
            raw[pix_off + off:pix_off + off + n] = im.reshape(-1)
            raw[pix_off + off + n:pix_off + _up16(off + n)] = 0
            (tx, tabx), (ty, taby) = tabs[w], tabs[h]
            desc[i] = (off, h, w, tx, ty, tabx.shape[1] - 2, taby.shape[1] - 2)
        return PackedBatch(buf, B, S, sizes, desc_off, coef_off, coef_count, pix_off, pix_bytes)

    def check(self, packed: PackedBatch) -> None:
        """Raise unless the kernel takes `packed` (no GPU call)."""
        if packed.S != self.S:
            raise ValueError("ImagePreprocessor: the batch was packed for S = %d, this preprocessor has S = %d" % (packed.S, self.S))
        if not supported(packed.B, self.S, packed.max_h, packed.max_w):
            raise RuntimeError("ImagePreprocessor (HIP): batch B=%d S=%d with sources up to %dx%d not supported (S <= 2048, "
                               "sources <= 8192, the largest downscale within the 160 KiB of LDS: coattn_preprocess_supported)"
                               % (packed.B, self.S, packed.max_h, packed.max_w))

    def empty(self, B, channels_last=False) -> torch.Tensor:
        return torch.empty((B, 3, self.S, self.S), dtype=torch.float32, device=self.device,
                           memory_format=torch.channels_last if channels_last else torch.contiguous_format)

    def launch(self, packed: PackedBatch, out=None, channels_last=False) -> torch.Tensor:
        """One launch of coattn_preprocess_images on the current stream over a PackedBatch whose buffer is on this
        preprocessor's device -> fp32 [B, 3, S, S] (`out`, of any strides, or a new tensor)."""
        buf = packed.buf
        if not buf.is_cuda:
            raise RuntimeError("ImagePreprocessor.launch runs on the GPU (there is no CPU fallback); got a buffer on %s -- "
                               "PackedBatch.to(device) first, or call the preprocessor itself" % buf.device)
        if _key(buf.device) != _key(self.device):
            raise RuntimeError("ImagePreprocessor: buffer on %s, lookup table on %s" % (buf.device, self.device))
        self.check(packed)
        B, S = packed.B, self.S
        if out is None:
            out = self.empty(B, channels_last)
        elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, 3, S, S)
                  and _key(out.device) == _key(self.device)):
            raise RuntimeError("ImagePreprocessor: out must be an fp32 [%d, 3, %d, %d] tensor on %s; got %s %s on %s"
                               % (B, S, S, self.device, getattr(out, "dtype", type(out)), tuple(getattr(out, "shape", ())),
                                  getattr(out, "device", None)))
        base = buf.data_ptr()
        sB, sC, sH, sW = out.stride()
        with _lib.on_device(self.device):
            _lib.bind("coattn_preprocess_images", pixels=base + packed.pix_off, pixel_bytes=packed.pix_bytes,
                      desc=base + packed.desc_off, coef=base + packed.coef_off, coef_count=packed.coef_count, lut=self.lut,
                      out=out, sB=sB, sC=sC, sH=sH, sW=sW, bad_images=_counter(self.device), B=B, S=S, max_h=packed.max_h,
                      max_w=packed.max_w, stream=_lib.stream_ptr(self.device))()
        return out

    def __call__(self, images, channels_last=False, out=None) -> torch.Tensor:
        """A list of uint8 [h, w, 3] images, or a PackedBatch (on the host or on the device) -> fp32 [B, 3, S, S]: packs and
        uploads what is still on the host, then one launch on the current stream."""
        packed = images if isinstance(images, PackedBatch) else self.pack(images)
        if not packed.buf.is_cuda:
            self.check(packed)
            packed = packed.to(self.device, non_blocking=packed.buf.is_pinned())
        return self.launch(packed, out=out, channels_last=channels_last)


def preprocess_host(images, S, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> torch.Tensor:
    """The same fp32 [B, 3, S, S] on the CPU: PIL's ``resize((S, S), BILINEAR)`` and the lookup table."""
    try:
        from PIL import Image
    except ImportError as e:                              # pragma: no cover
        raise RuntimeError("preprocess_host needs Pillow (PIL) for the resize; it is not installed -- on a GPU, "
                           "--preprocess hip needs no Pillow for .npy images") from e
    S = int(S)
    lut = lut_values(mean, std).numpy()
    chan = np.arange(3).reshape(1, 1, 3)
    out = np.empty((len(images), 3, S, S), dtype=np.float32)
    for i, im in enumerate(images):
        small = np.asarray(Image.fromarray(np.ascontiguousarray(_as_pixels(im, i))).resize((S, S), Image.BILINEAR))
        out[i] = lut[chan, small].transpose(2, 0, 1)
    return torch.from_numpy(out)

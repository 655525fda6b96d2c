#!/usr/bin/env python3
"""Developer probe: which arithmetic reproduces the stock convolution of the frozen VGG's first layer (3 -> 64 channels, 3x3,
padding 1, channels_last fp32) bit for bit.  At the benchmark's shape (batch 160, 224 px; BATCH / SIDE override), with MIOpen's
find records seeded as bench.py seeds them, every candidate of coattn_conv1_probe (include/coattn.h) is compared with F.conv2d
on inputs that separate them: mixed magnitudes and signs inside a patch, 1e-41 subnormals, 1e19, NaN / inf, negative zeros.
Prints one JSON object: per input kind and candidate the number of elements whose bits differ (NaNs in the same places count as
equal, +0 against -0 as different).  (Which kernel MIOpen runs is read off a rocprofv3 kernel trace of bench.py; the order
tried first came from that kernel's source: LAB_NOTES Part A8.)
usage: python tools/probe_conv1_exact.py"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

bench.seed_miopen_db()
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vqa_amd import _lib  # noqa: E402

BATCH, SIDE = int(os.environ.get("BATCH", 160)), int(os.environ.get("SIDE", 224))
# (name, order, step, halves, skip)
CANDIDATES = (("mfma 32x32x2, (ky,kx,c) to 32, pairs (t, t+8)", -1, 0, 1, 0),
              ("mfma 32x32x2, (ky,kx,c) to 32, pairs (t, t+4)", -2, 0, 1, 0),
              ("fmaf (ky,kx,c) to 32, pairs (t, t+8), lower first", 6, 0, 1, 0),
              ("fmaf (ky,kx,c) to 32, pairs (t, t+8), upper first", 7, 0, 1, 0),
              ("fmaf (ky,kx,c) to 32, pairs (t, t+4), lower first", 8, 0, 1, 0),
              ("fmaf (ky,kx,c) to 32, pairs (t, t+4), upper first", 9, 0, 1, 0),
              ("fmaf (ky,kx,c) to 32, pairs (t, t+2), lower first", 10, 0, 1, 0),
              ("fmaf (ky,kx,c) to 32, pairs (t, t+16), lower first", 12, 0, 1, 0),
              ("fmaf (ky,kx,c) padded to 28", 0, 0, 1, 0),
              ("fmaf (ky,kx,c), zero terms skipped", 0, 0, 1, 1),
              ("mul+add (ky,kx,c)", 0, 1, 1, 0),
              ("fmaf (ky,c,kx)", 1, 0, 1, 0),
              ("fmaf (c,ky,kx)", 2, 0, 1, 0),
              ("fmaf (kx,ky,c)", 3, 0, 1, 0),
              ("fmaf (c,kx,ky)", 4, 0, 1, 0),
              ("fmaf (kx,c,ky)", 5, 0, 1, 0),
              ("fmaf (ky,kx,c), two halves of k added", 0, 0, 2, 0))
KINDS = ("normal", "mixed magnitude", "subnormal", "near 1e19", "NaN and inf", "negative zero", "infinite weight")


def inputs(kind, dev):
    g = torch.Generator().manual_seed(len(kind))
    img = torch.randn(BATCH, 3, SIDE, SIDE, generator=g)
    w = torch.randn(64, 3, 3, 3, generator=g) * 0.2
    if kind == "mixed magnitude":
        img *= 10.0 ** torch.randint(-4, 5, img.shape, generator=g).float()
        w *= 10.0 ** torch.randint(-2, 3, w.shape, generator=g).float()
    elif kind == "subnormal":
        img *= 1e-41
        w.mul_(5.0)
    elif kind == "near 1e19":
        img *= 1e19
        w *= 1e19
    elif kind == "NaN and inf":
        img[0, 1, 0, 0] = float("nan")
        img[BATCH - 1, 2, SIDE - 1, SIDE - 1] = float("inf")
        img[BATCH // 2, 0, SIDE // 2, 1] = float("-inf")
    elif kind == "negative zero":
        img[:, :, ::2] = -0.0
        img[:, 1] = -0.0
        w[::2] = -w[::2].abs()
        w[5] = -0.0
    elif kind == "infinite weight":
        w[3, 1, 0, 2] = float("inf")
    return (img.to(dev).contiguous(memory_format=torch.channels_last), w.to(dev).contiguous(memory_format=torch.channels_last))


def differing(a, b):
    same = (a.view(torch.int32) == b.view(torch.int32)) | (a.isnan() & b.isnan())
    return int((~same).sum())


def main():
    dev = torch.device("cuda")
    lib = _lib.load()
    st = C.c_void_p(_lib.stream_ptr(dev))
    ws = torch.empty((lib.coattn_conv1_bn_exact_workspace_bytes(BATCH, SIDE, SIDE, 0) + 3) // 4, device=dev)
    x = torch.empty((BATCH, 64, SIDE, SIDE), device=dev, memory_format=torch.channels_last)
    table = {}
    for kind in KINDS:
        img, w = inputs(kind, dev)
        with torch.no_grad():
            ref = F.conv2d(img, w, None, 1, 1)
        assert ref.is_contiguous(memory_format=torch.channels_last)
        row = table[kind] = {"elements": ref.numel(), "nan": int(ref.isnan().sum()), "negative_zero": int((ref.view(torch.int32) == -2 ** 31).sum())}
        for name, order, step, halves, skip in CANDIDATES:
            x.fill_(float("nan"))
            _lib.check(lib.coattn_conv1_probe(_lib.ptr(img), _lib.ptr(w), _lib.ptr(x), _lib.ptr(ws), BATCH, SIDE, SIDE, order, step,
                                              halves, skip, st), "coattn_conv1_probe")
            row[name] = differing(x, ref)
        print(kind, json.dumps(row), file=sys.stderr, flush=True)
        del img, w, ref
    print(json.dumps({"batch": BATCH, "side": SIDE, "differing_elements": table}, indent=1))


if __name__ == "__main__":
    main()

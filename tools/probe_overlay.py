"""Developer probe: the attention-overlay kernel (vqa_amd.overlay.render_attention, one launch) against the torch composition it
replaces -- per level F.interpolate(bilinear), the division by the map's maximum, the de-normalised image, the blend, the clamp,
the cast to uint8 and the permute to HWC --, for L = 3 levels and a question strip of 32 rows.

One process, B = 160 at 224 px (7 x 7 grid) and at 448 px (14 x 14), both modes, the image contiguous (NCHW) and channels-last
(as predict.py holds it).  Per shape and mode three variants alternate window by window: `kernel` (the C-ABI call bound once),
`wrapper` (render_attention, which adds its Python host time and allocates the output) and `torch`.  After a warm-up window
each, WINDOWS windows of ITERS calls timed by HIP events; per variant the median window and the spread of its windows
((max - min) / median).  Also: the kernel's share of the 8 TB/s HBM figure over its own byte count -- the image once in,
(L+1) (H+strip) W 3 bytes per sample out -- and the peak device memory of one call of either route above what is resident
before it.  The torch composition's bytes are compared with the kernel's once (they may differ by a code value: torch rounds
the blend differently) and the largest difference is reported.

Under `rocprofv3 --kernel-trace --stats -- python3 tools/probe_overlay.py` (ITERS=3 WINDOWS=2 for a short trace) the kernel
table shows overlay_kernel once per kernel / wrapper call and the dozens of launches of the torch route.

Environment: ITERS (20), WINDOWS (7), SIZES ("224,448"), B (160), OUT (also append the JSON lines to this file)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import vqa_amd  # noqa: E402
from vqa_amd import _lib, overlay as OV  # noqa: E402

B = int(os.environ.get("B", "160"))
L, T_, STRIP = 3, 26, 32
ITERS = int(os.environ.get("ITERS", "20"))
WINDOWS = int(os.environ.get("WINDOWS", "7"))
GRID = {224: 7, 448: 14}
HBM_TBPS = 8.0


def emit(line):
    print(json.dumps(line), flush=True)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "a") as fh:
            fh.write(json.dumps(line) + "\n")


def timed(fn, iters, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(variants, iters, stream):
    names = list(variants)
    for n in names:
        timed(variants[n], iters, stream)
    t = {n: [] for n in names}
    for w in range(WINDOWS):
        k = w % len(names)
        for n in names[k:] + names[:k]:                          # the order rotates
            t[n].append(timed(variants[n], iters, stream))
    return t


def torch_route(image, a_v, a_q, G, mode, lut, mean, std, alpha, floor):
    """The composition the kernel replaces: uint8 [B, L+1, H+STRIP, W, 3]."""
    Bn, _, H, W = image.shape
    x = (image * std.view(1, 3, 1, 1) + mean.view(1, 3, 1, 1)).clamp(0, 1)
    out = torch.zeros((Bn, L + 1, H + STRIP, W, 3), dtype=torch.uint8, device=image.device)
    out[:, 0, :H] = (x * 255 + 0.5).to(torch.uint8).permute(0, 2, 3, 1)
    cell = (torch.arange(W, device=image.device) * T_) // W
    for l in range(L):
        m = a_v[l] / a_v[l].amax(dim=1, keepdim=True)
        u = F.interpolate(m.view(Bn, 1, G, G), size=(H, W), mode="bilinear", align_corners=False)
        mq = (a_q[l] / a_q[l].amax(dim=1, keepdim=True))[:, cell]                       # [B, W]
        if mode == "mask":
            o = x * (floor + (1 - floor) * u)
            s = mq[:, None, :, None].expand(Bn, STRIP, W, 3)
        else:
            colour = lut[(u[:, 0] * 255 + 0.5).long()].permute(0, 3, 1, 2)                  # [B, 3, H, W]
            o = (1 - alpha) * x + alpha * colour
            s = lut[(mq * 255 + 0.5).long()][:, None].expand(Bn, STRIP, W, 3)
        out[:, 1 + l, :H] = (o.clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(0, 2, 3, 1)
        out[:, 1 + l, H:] = (s.clamp(0, 1) * 255 + 0.5).to(torch.uint8)
    return out


def peak_of(fn, dev):
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = fn()
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return peak


def main():
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    common = {"B": B, "L": L, "T": T_, "strip": STRIP, "windows": WINDOWS, "iters": ITERS,
              "version": vqa_amd._lib.load().coattn_version(), "device": torch.cuda.get_device_name(dev)}
    mean, std = torch.tensor(OV.IMAGENET_MEAN, device=dev), torch.tensor(OV.IMAGENET_STD, device=dev)
    lut = OV.default_lut(dev)
    for size in [int(x) for x in os.environ.get("SIZES", "224,448").split(",")]:
        G = GRID[size]
        g = torch.Generator(device=dev).manual_seed(size)
        nchw = torch.randn((B, 3, size, size), device=dev, generator=g)
        a_v = torch.softmax(torch.randn((L, B, G * G), device=dev, generator=g) * 3, 2)
        a_q = torch.softmax(torch.randn((L, B, T_), device=dev, generator=g) * 3, 2)
        out = torch.empty((B, L + 1, size + STRIP, size, 3), dtype=torch.uint8, device=dev)
        moved = nchw.numel() * 4 + out.numel()
        for layout in ("nchw", "channels_last"):
            image = nchw if layout == "nchw" else nchw.contiguous(memory_format=torch.channels_last)
            for mode in ("heat", "mask"):
                p = _lib.OverlayParams((_lib.C.c_float * 3)(*OV.IMAGENET_MEAN), (_lib.C.c_float * 3)(*OV.IMAGENET_STD), 0.6, 0.3,
                                       lut.data_ptr())
                sB, sC, sH, sW = image.stride()
                call = _lib.bind("coattn_overlay_render", image=image, sB=sB, sC=sC, sH=sH, sW=sW, a_v=a_v, a_q=a_q, q_len=None, p=p,
                                 out=out, bad_maps=None, B=B, L=L, H=size, W=size, Gh=G, Gw=G, T=T_, strip_h=STRIP,
                                 mode=OV.MODES[mode], stream=st.cuda_stream)
                kw = dict(mode=mode, strip=STRIP)
                variants = {"kernel": lambda: call(), "wrapper": lambda: OV.render_attention(image, a_v, a_q, **kw)}
                if layout == "nchw":
                    variants["torch"] = lambda: torch_route(image, a_v, a_q, G, mode, lut, mean, std, 0.6, 0.3)
                t = alternate(variants, ITERS, st)
                line = dict(common, what="overlay", image_size=size, grid=G, layout=layout, mode=mode, bytes_moved=moved)
                for n, v in t.items():
                    med = statistics.median(v)
                    line[n + "_ms"] = round(med, 4)
                    line[n + "_spread"] = round((max(v) - min(v)) / med, 4)
                    line[n + "_windows_ms"] = [round(x, 4) for x in v]
                line["kernel_TBps"] = round(moved / line["kernel_ms"] / 1e9, 3)
                line["kernel_share_of_hbm"] = round(line["kernel_TBps"] / HBM_TBPS, 4)
                line["wrapper_peak_bytes"] = peak_of(variants["wrapper"], dev)
                if layout == "nchw":
                    line["kernel_over_torch"] = round(line["kernel_ms"] / line["torch_ms"], 4)
                    line["torch_peak_bytes"] = peak_of(variants["torch"], dev)
                    call()
                    ref = variants["torch"]()
                    delta = (out.to(torch.int16) - ref.to(torch.int16)).abs()
                    line["bytes_differing_from_torch"] = int((delta != 0).sum())
                    line["largest_difference_from_torch"] = int(delta.max())
                    del ref, delta
                emit(line)
        assert OV.bad_maps() == 0
        del nchw, image, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

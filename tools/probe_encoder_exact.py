#!/usr/bin/env python3
"""Developer probe: the frozen VGG11-bn's glue at the benchmark's shapes (batch 160, 224 px; BATCH / SIDE override) on its
three routes.  Prints one JSON object: `exact_report` -- encoder.exact_report() after two passes of a channels_last
ImageCoAttentionEncoder under the default settings (the first pass compares every layer with the stock chain) -- and `layers`,
per (C, side, pool) the HIP-event median in microseconds of everything between two convolutions on the stock chain
(nn.BatchNorm2d, then relu_pool or ReLU), on bn_exact and on bn_relu_pool (VQA_ENCODER_FUSED=1's call).
usage: python tools/probe_encoder_exact.py"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqa_amd import encoder  # noqa: E402
from vqa_amd.modules import ImageCoAttentionEncoder  # noqa: E402

BATCH, SIDE, REPS = int(os.environ.get("BATCH", 160)), int(os.environ.get("SIDE", 224)), int(os.environ.get("REPS", 9))
LAYERS = ((64, 1, True), (128, 2, True), (256, 4, False), (256, 4, True), (512, 8, False), (512, 8, True), (512, 16, False),
          (512, 16, True))                              # (C, SIDE / side, a pool follows)


def median_us(fn):
    fn()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return round(sorted(times)[len(times) // 2], 1)


def main():
    for name in ("VQA_ENCODER_FUSED", "VQA_ENCODER_EXACT_BN"):
        os.environ.pop(name, None)
    dev = torch.device("cuda")
    torch.manual_seed(0)
    enc = ImageCoAttentionEncoder(is_trainable=False, weights_path=None).to(dev).to(memory_format=torch.channels_last)
    img = torch.randn(BATCH, 3, SIDE, SIDE, device=dev).contiguous(memory_format=torch.channels_last)
    for _ in range(2):
        enc(img)
    torch.cuda.synchronize()
    report = [{"device": k[0], "B": k[1], "C": k[2], "H": k[3], "W": k[4], "pool": k[5], **v}
              for k, v in encoder.exact_report().items()]
    del enc, img
    layers = []
    pool2 = torch.nn.MaxPool2d(2, 2)
    for ch, div, pool in LAYERS:
        side = SIDE // div
        x = torch.randn(BATCH, ch, side, side, device=dev).contiguous(memory_format=torch.channels_last)
        bn = torch.nn.BatchNorm2d(ch).to(dev)
        row = {"C": ch, "side": side, "pool": pool, "x_bytes": x.numel() * 4}
        with torch.no_grad():
            row["stock_us"] = median_us(lambda: encoder._stock_chain(x, bn, pool2 if pool else None))
            if encoder.exact_output_fusable(x, bn, pool):
                row["exact_us"] = median_us(lambda: encoder.bn_exact(x, bn, pool))
            row["fused_us"] = median_us(lambda: encoder.bn_relu_pool(x, bn, pool=pool))
        layers.append(row)
        del x
    print(json.dumps({"batch": BATCH, "side": SIDE, "exact_report": report, "layers": layers}, indent=1))


if __name__ == "__main__":
    main()

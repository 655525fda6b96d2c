#!/usr/bin/env python3
"""Developer probe: layer 1 of the frozen encoder at the benchmark's shape (batch 160, 224 px; BATCH / SIDE override), the form
that stores the convolution output (coattn_conv1_bn_exact_forward, x in its workspace) against the form that computes it twice
(coattn_conv1_bn_recompute_forward), alternating window by window in one process.  Every call of a window takes the next of
SETS sets of (image, y, workspace), so that nothing it reads or writes is still in the caches from its last use.  A window is
timed by HIP events around its ITERS calls and, call by call, by the launch-group marks (coattn_profile_begin / _end).  One
JSON line per window, appended to profiles/conv1_recompute_probe.jsonl (OUT overrides), and a summary line on stdout.
usage: timeout -k 10 300 python tools/probe_conv1_recompute.py      (one GPU step: run it under a time limit of its own)"""
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vqa_amd import _lib  # noqa: E402

BATCH, SIDE = int(os.environ.get("BATCH", 160)), int(os.environ.get("SIDE", 224))
SETS, ITERS, WINDOWS = int(os.environ.get("SETS", 4)), int(os.environ.get("ITERS", 8)), int(os.environ.get("WINDOWS", 6))
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "conv1_recompute_probe.jsonl"))


def main():
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, H, W = BATCH, SIDE, SIDE
    assert lib.coattn_conv1_bn_exact_supported(B, H, W, 3, 64, 1, _lib.F32) == 1
    g = torch.Generator(device=dev).manual_seed(0)
    weight = (0.2 * torch.randn(64, 3, 3, 3, device=dev, generator=g)).contiguous(memory_format=torch.channels_last)
    gamma, beta = 0.5 + torch.rand(64, device=dev, generator=g), 0.1 * torch.randn(64, device=dev, generator=g)
    sizes = {"stored": lib.coattn_conv1_bn_exact_workspace_bytes(B, H, W, 1), "recompute": lib.coattn_conv1_bn_recompute_workspace_bytes(B, H, W)}
    sets = [{"image": torch.randn(B, 3, H, W, device=dev, generator=g).contiguous(memory_format=torch.channels_last),
             "y": torch.empty(B, 64, H // 2, W // 2, device=dev).contiguous(memory_format=torch.channels_last),
             "ws": torch.empty(max(sizes.values()) // 4, device=dev), "save": torch.empty(2, 64, device=dev),
             "rm": torch.zeros(64, device=dev), "rv": torch.ones(64, device=dev)} for _ in range(SETS)]
    st = C.c_void_p(_lib.stream_ptr(dev))
    us, names = (C.c_float * 48)(), C.create_string_buffer(2048)

    def call(form, s):
        common = (_lib.ptr(s["image"]), _lib.ptr(weight), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(s["rm"]), _lib.ptr(s["rv"]), 0.1, 1e-5)
        tail = (_lib.ptr(s["y"]), _lib.ptr(s["save"][0]), _lib.ptr(s["save"][1]), _lib.ptr(s["ws"]), B, H, W, 3, 64, 1, _lib.F32, st)
        if form == "stored":
            _lib.check(lib.coattn_conv1_bn_exact_forward(*common, C.c_void_p(0), *tail), "coattn_conv1_bn_exact_forward")
        else:
            _lib.check(lib.coattn_conv1_bn_recompute_forward(*common, *tail), "coattn_conv1_bn_recompute_forward")

    turn = [0]

    def window(form, marked):
        marks = {}
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ITERS):
            s = sets[turn[0] % SETS]
            turn[0] += 1
            if marked:
                _lib.check(lib.coattn_profile_begin(st), "coattn_profile_begin")
            call(form, s)
            if marked:
                n = lib.coattn_profile_end(us, names, 2048, 48)
                if n < 0:
                    _lib.check(n, "coattn_profile_end")
                for k, nm in enumerate(names.value.decode().split("\n")[:n]):
                    marks.setdefault(nm, []).append(us[k])
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / ITERS, {k: round(statistics.median(v), 1) for k, v in marks.items()}

    for form in ("stored", "recompute"):                    # warm-up: code objects, first touch of every buffer, clocks
        window(form, False)
    ys = {}
    for form in ("stored", "recompute"):                    # the same bits, here too
        for s in sets[:1]:
            s["rm"].zero_(), s["rv"].fill_(1.0)
            call(form, s)
            ys[form] = (s["y"].clone(), s["save"].clone(), s["rm"].clone(), s["rv"].clone())
    equal = all(torch.equal(a, b) for a, b in zip(ys["stored"], ys["recompute"]))
    rows = []
    for w in range(WINDOWS):
        for form in (("stored", "recompute") if w % 2 == 0 else ("recompute", "stored")):
            plain_us, _ = window(form, False)                # events around the whole window: no synchronisation inside
            _, marks = window(form, True)                    # call by call, one synchronisation per call
            rows.append({"window": w, "form": form, "B": B, "H": H, "W": W, "iters": ITERS, "sets": SETS,
                         "us_per_call": round(plain_us, 1), "marks_us": marks, "workspace_bytes": sizes[form],
                         "equal_bits": equal, "device": torch.cuda.get_device_name(dev)})
    with open(OUT, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    med = {form: statistics.median(r["us_per_call"] for r in rows if r["form"] == form) for form in ("stored", "recompute")}
    print(json.dumps({"stored_us": med["stored"], "recompute_us": med["recompute"], "equal_bits": equal,
                      "last_marks": {r["form"]: r["marks_us"] for r in rows[-2:]}}))


if __name__ == "__main__":
    main()

"""Developer probe: what the optimiser step costs, stock against HIP.  The trainable parameter set of the BASELINE cfg 2
attention model (vocab 10000, K = 1001: 27 tensors with a gradient, ~12.2 M floats; the dead W_b has none) with fixed random
gradients, stepped by
    foreach   torch.optim.Adam (the default multi-tensor path: what Trainer(optimizer="torch") runs)
    fused     torch.optim.Adam(fused=True), if this torch build accepts it
    hip       vqa_amd.HipAdam
    hip_clip  vqa_amd.HipAdam(max_grad_norm=1.0): the norm pass ahead of the update
in one process, the variants alternating window by window (the order rotates).  Two modes: "warm" steps ONE parameter / state
set over and over (~195 MB: p, g, m, v -- it fits the 256 MB Infinity Cache), "cold" rotates over SETS sets per variant so that
every step meets data that has long left the cache.  Per window: ITERS steps between two HIP events (ms per step: the larger
of device time and host enqueue time) and the host's enqueue time for the same steps.  The median window per variant is
reported, the spread of the foreach windows, and for the HIP variants the bytes the step moves (28 B per element, + 4 B for the
norm pass) over the event time; one JSON line per mode.

Device time per kernel comes from a run of its own:  rocprofv3 --kernel-trace --stats -- python3 tools/probe_adam.py
(ITERS=10 WINDOWS=2 for a short trace): adam_step_kernel / grad_norm_kernel against the multi_tensor_apply_kernel rows.

Environment: ITERS (50), WINDOWS (8), SETS (6), MODES ("warm,cold"), OUT (also append the JSON lines to this file)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vqa_amd  # noqa: E402
from vqa_amd import train as T  # noqa: E402

ITERS = int(os.environ.get("ITERS", "50"))
WINDOWS = int(os.environ.get("WINDOWS", "8"))
SETS = int(os.environ.get("SETS", "6"))


def makers():
    out = {"foreach": lambda ps: torch.optim.Adam(ps, 1e-4)}
    try:
        torch.optim.Adam([torch.nn.Parameter(torch.zeros(1, device="cuda:0"))], 1e-4, fused=True)
        out["fused"] = lambda ps: torch.optim.Adam(ps, 1e-4, fused=True)
    except (RuntimeError, ValueError, TypeError) as e:
        print("fused=True refused by this torch build: %s" % e, file=sys.stderr)
    out["hip"] = lambda ps: vqa_amd.HipAdam(ps, 1e-4)
    out["hip_clip"] = lambda ps: vqa_amd.HipAdam(ps, 1e-4, max_grad_norm=1.0)
    return out


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = T.build_model("attention", 10000, 1001)
    shapes = [tuple(p.shape) for n, p in model.named_parameters() if p.requires_grad and not n.startswith("co_attention.W_b.")]
    elems = sum(torch.Size(s).numel() for s in shapes)
    g = torch.Generator(device=dev).manual_seed(1)
    make = makers()
    opts = {}                                                    # variant -> [optimizer per set]
    for k, mk in make.items():
        opts[k] = []
        for _ in range(SETS):
            ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g) * 0.05) for s in shapes]
            for p in ps:
                p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
            opts[k].append(mk(ps))
    st = torch.cuda.current_stream(dev)

    def window(kind, cold, at):
        sets = opts[kind]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(st)
        for i in range(ITERS):
            sets[(at + i) % SETS if cold else 0].step()
        e1.record(st)
        host = time.perf_counter() - t0
        e1.synchronize()
        return e0.elapsed_time(e1) / ITERS, 1e3 * host / ITERS

    kinds = list(make)
    for k in kinds:                                              # warm-up: code objects, optimiser state, every buffer touched
        for o in opts[k]:
            o.step()
    for mode in os.environ.get("MODES", "warm,cold").split(","):
        cold = mode == "cold"
        t = {k: [] for k in kinds}
        h = {k: [] for k in kinds}
        for w in range(WINDOWS):
            r = w % len(kinds)
            for k in kinds[r:] + kinds[:r]:
                ms, host = window(k, cold, w * ITERS)
                t[k].append(ms)
                h[k].append(host)
        med = {k: statistics.median(v) for k, v in t.items()}
        line = {"mode": mode, "tensors": len(shapes), "elements": elems, "sets": SETS if cold else 1, "iters": ITERS,
                "windows": WINDOWS, "ms_per_step": {k: round(v, 4) for k, v in med.items()},
                "host_ms_per_step": {k: round(statistics.median(v), 4) for k, v in h.items()},
                "foreach_over_hip": round(med["foreach"] / med["hip"], 3),
                "foreach_spread": round((max(t["foreach"]) - min(t["foreach"])) / med["foreach"], 4),
                "hip_TBps": round(28.0 * elems / (med["hip"] * 1e-3) / 1e12, 3),
                "hip_clip_TBps": round(32.0 * elems / (med["hip_clip"] * 1e-3) / 1e12, 3),
                "windows_ms": {k: [round(x, 4) for x in v] for k, v in t.items()},
                "grad_norm": float(opts["hip_clip"][0].grad_norm), "device": torch.cuda.get_device_name(dev)}
        if "fused" in med:
            line["fused_over_hip"] = round(med["fused"] / med["hip"], 3)
        print(json.dumps(line), flush=True)
        if os.environ.get("OUT"):
            with open(os.environ["OUT"], "a") as fh:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

"""Developer probe: what the baseline model costs behind its two encoders, stock against HIP.  The modules of VQABaselineNet
behind the VGG and the GRU at the baseline's shape (B = 160, Di = 4096, H = J = 1024, Mh = 1000, K = 1001) in training mode with
the reference's Dropout(0.5), forward + backward (a gradient at the logits; the GRU's state h needs one, the features f do not),
with
    stock   F.normalize -> Linear -> Tanh, Linear -> Tanh, the product, Linear -> nn.Dropout -> Tanh, Linear (the stock lines)
    hip     fusion.fusion_head on the same parameters, its dropout drawn in the head from a DropoutState
on the same modules in one process, the routes alternating window by window (the order rotates).  Per window: ITERS forward +
backward passes between two HIP events (ms per pass: the larger of device time and host enqueue time) and the host's enqueue
time; every window is one JSON line of OUT, the last line the summary: median and window range per route, stock / hip, and the
spread of the stock windows (the yardstick's own noise).

Launches per pass come from kernel-trace runs of their own, one per route:
    ROUTES=hip ITERS=20 WINDOWS=2 rocprofv3 --kernel-trace --stats --output-format csv -d DIR_hip -- python3 tools/probe_fusion.py
and SUMMARY=DIR_stock,DIR_hip python3 tools/probe_fusion.py folds the two kernel_stats.csv into one JSON line (appended to OUT):
launches per pass per route and the kernels that take the most time.  The SUMMARY run must be given the ITERS and WINDOWS of
the traced runs.

Environment: ITERS (200), WINDOWS (9), ROUTES ("stock,hip"), OUT (append the JSON lines to this file), BATCH (160)."""
import csv
import glob
import json
import os
import statistics
import sys
import time

ITERS = int(os.environ.get("ITERS", "200"))
WINDOWS = int(os.environ.get("WINDOWS", "9"))
ROUTES = os.environ.get("ROUTES", "stock,hip").split(",")
WARMUP = 3


def emit(line):
    print(json.dumps(line), flush=True)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "a") as fh:
            fh.write(json.dumps(line) + "\n")


def summary(dirs):
    passes = WARMUP + ITERS * WINDOWS
    line = {"kernel_trace": True, "passes_per_route": passes, "launches_per_pass": {}, "top_kernels": {}}
    for d in dirs:
        route = "hip" if "hip" in os.path.basename(d.rstrip("/")) else "stock"
        f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))[0]
        rows = list(csv.DictReader(open(f)))
        line["launches_per_pass"][route] = round(sum(int(r["Calls"]) for r in rows) / passes, 2)
        line["top_kernels"][route] = [
            {"name": r["Name"][:80], "calls_per_pass": round(int(r["Calls"]) / passes, 2), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
             "us_per_pass": round(float(r["TotalDurationNs"]) / 1e3 / passes, 1)}
            for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:8]]
    emit(line)


def main():
    import torch
    import torch.nn.functional as F
    from torch import nn

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import vqa_amd
    from vqa_amd.fusion import fusion_head

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, Di, H, J, Mh, K = int(os.environ.get("BATCH", "160")), 4096, 1024, 1024, 1000, 1001
    img = nn.Sequential(nn.Linear(Di, J), nn.Tanh()).to(dev)
    qst = nn.Sequential(nn.Linear(H, J), nn.Tanh()).to(dev)
    mlp = nn.Sequential(nn.Linear(J, Mh), nn.Dropout(0.5), nn.Tanh()).to(dev)
    fc = nn.Linear(Mh, K).to(dev)
    params = [p for m in (img, qst, mlp, fc) for p in m.parameters()]
    f = torch.randn(B, Di, device=dev).clamp_min(0)
    h = torch.tanh(torch.randn(B, H, device=dev)).requires_grad_(True)
    g = torch.randn(B, K, device=dev)
    state = vqa_amd.DropoutState(1, dev)
    st = torch.cuda.current_stream(dev)

    def one(route):
        for p in params + [h]:
            p.grad = None
        if route == "stock":
            out = fc(mlp(img(F.normalize(f, dim=1, p=2)) * qst(h)))
        else:
            out = fusion_head(f, h, img[0].weight, img[0].bias, qst[0].weight, qst[0].bias, mlp[0].weight, mlp[0].bias, fc.weight,
                              fc.bias, p=0.5, state=state)
        out.backward(g)

    def window(route):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(st)
        for _ in range(ITERS):
            one(route)
        e1.record(st)
        host = time.perf_counter() - t0
        e1.synchronize()
        return e0.elapsed_time(e1) / ITERS, 1e3 * host / ITERS

    for r in ROUTES:
        for _ in range(WARMUP):
            one(r)
    torch.cuda.synchronize()
    t = {r: [] for r in ROUTES}
    hs = {r: [] for r in ROUTES}
    for w in range(WINDOWS):
        k = w % len(ROUTES)
        for r in ROUTES[k:] + ROUTES[:k]:
            ms, host = window(r)
            t[r].append(ms)
            hs[r].append(host)
            emit({"window": w, "route": r, "iters": ITERS, "ms_per_pass": round(ms, 4), "host_ms_per_pass": round(host, 4)})
    med = {r: statistics.median(v) for r, v in t.items()}
    line = {"summary": True, "B": B, "Di": Di, "H": H, "J": J, "Mh": Mh, "K": K, "p": 0.5, "iters": ITERS, "windows": WINDOWS,
            "ms_per_pass": {r: round(v, 4) for r, v in med.items()},
            "ms_per_pass_range": {r: [round(min(v), 4), round(max(v), 4)] for r, v in t.items()},
            "host_ms_per_pass": {r: round(statistics.median(v), 4) for r, v in hs.items()},
            "device": torch.cuda.get_device_name(dev), "device_uuid": str(getattr(torch.cuda.get_device_properties(dev), "uuid", "unknown"))}
    if "stock" in med:
        line["stock_spread"] = round((max(t["stock"]) - min(t["stock"])) / med["stock"], 4)
    if "stock" in med and "hip" in med:
        line["stock_over_hip"] = round(med["stock"] / med["hip"], 3)
    emit(line)


if __name__ == "__main__":
    if os.environ.get("SUMMARY"):
        summary(os.environ["SUMMARY"].split(","))
    else:
        main()

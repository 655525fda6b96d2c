"""Developer probe: what the baseline question encoder costs, stock against HIP.  QuestionBaselineEncoder at the baseline's shape
(B = 160, T = 26, E = 300, H = 1024, vocabulary 10000) on the synthetic data's length-sorted questions (the stock route needs them
sorted), forward + backward (a gradient at the encoder's [B, 1024] output), with
    stock   gru_impl = "stock": pack_padded_sequence -> nn.GRU, lengths on the host (the trainer's call)
    hip     gru_impl = "hip": gru.question_gru, lengths on the device
on the same module in one process, the routes alternating window by window (the order rotates).  Per window: ITERS forward +
backward passes between two HIP events (ms per pass: the larger of device time and host enqueue time) and the host's enqueue
time; every window is one JSON line of OUT, the last line the summary: median and window range per route, stock / hip, and the
spread of the stock windows (the yardstick's own noise).

Launches per pass and the step kernels' time per step come from kernel-trace runs of their own, one per route:
    ROUTES=hip ITERS=20 WINDOWS=2 rocprofv3 --kernel-trace --stats --output-format csv -d DIR_hip -- python3 tools/probe_gru.py
and SUMMARY=DIR_stock,DIR_hip python3 tools/probe_gru.py folds the two kernel_stats.csv into one JSON line (appended to OUT):
launches per pass per route, and for gru_fwd_step_kernel / gru_bwd_step_kernel the calls per pass and the average microseconds.
The SUMMARY run must be given the ITERS and WINDOWS of the traced runs.

Environment: ITERS (100), WINDOWS (9), ROUTES ("stock,hip"), OUT (append the JSON lines to this file), BATCH (160)."""
import csv
import glob
import json
import os
import statistics
import sys
import time

ITERS = int(os.environ.get("ITERS", "100"))
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
    line = {"kernel_trace": True, "passes_per_route": passes, "launches_per_pass": {}, "step_kernels": {}, "top_kernels": {}}
    for d in dirs:
        route = "hip" if "hip" in os.path.basename(d.rstrip("/")) else "stock"
        f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))[0]
        rows = list(csv.DictReader(open(f)))
        line["launches_per_pass"][route] = round(sum(int(r["Calls"]) for r in rows) / passes, 2)
        line["top_kernels"][route] = [
            {"name": r["Name"][:80], "calls_per_pass": round(int(r["Calls"]) / passes, 2), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
             "us_per_pass": round(float(r["TotalDurationNs"]) / 1e3 / passes, 1)}
            for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:6]]
        for r in rows:
            for k in ("gru_fwd_step_kernel", "gru_bwd_step_kernel"):
                if k in r["Name"]:
                    line["step_kernels"][k] = {"calls_per_pass": round(int(r["Calls"]) / passes, 2),
                                               "avg_us": round(float(r["AverageNs"]) / 1e3, 2)}
    emit(line)


def main():
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import vqa_amd  # noqa: F401
    from vqa_amd import modules as M, train as T

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, Tn, E, H = int(os.environ.get("BATCH", "160")), 26, 300, 1024
    enc = M.QuestionBaselineEncoder(10000, E, H).to(dev)
    b = T.synthetic_batch(B, (8, 8), Tn, 10000, 11, seed=1)
    _, q, _, ln = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
    q = q.to(dev)
    lens = {"stock": ln, "hip": ln.to(dev)}
    g = torch.randn(B, 1024, device=dev)
    st = torch.cuda.current_stream(dev)

    def one(route):
        enc.gru_impl = route
        for p in enc.parameters():
            p.grad = None
        enc(q, lens[route]).backward(g)

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
    h = {r: [] for r in ROUTES}
    for w in range(WINDOWS):
        k = w % len(ROUTES)
        for r in ROUTES[k:] + ROUTES[:k]:
            ms, host = window(r)
            t[r].append(ms)
            h[r].append(host)
            emit({"window": w, "route": r, "iters": ITERS, "ms_per_pass": round(ms, 4), "host_ms_per_pass": round(host, 4)})
    med = {r: statistics.median(v) for r, v in t.items()}
    line = {"summary": True, "B": B, "T": Tn, "E": E, "H": H, "lengths": "sorted, synthetic U{3..26}", "iters": ITERS,
            "windows": WINDOWS, "ms_per_pass": {r: round(v, 4) for r, v in med.items()},
            "ms_per_pass_range": {r: [round(min(v), 4), round(max(v), 4)] for r, v in t.items()},
            "host_ms_per_pass": {r: round(statistics.median(v), 4) for r, v in h.items()},
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

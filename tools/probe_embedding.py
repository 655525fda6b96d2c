"""Developer probe: what the question encoder's word level costs, stock against HIP, alone and beside the HIP sentence level.
QuestionCoAttentionEncoder at BASELINE cfg 2's shape (B = 160, T = 26, E = H = 512, vocabulary 10000) on the synthetic data's
length-sorted questions with one token opening HOT (150) of the questions, forward + backward (gradients at all three levels),
with
    stock      word_impl = "stock", sentence_impl = "stock": nn.Embedding and PyTorch's embedding backward (its sort path:
               B T = 4160 > 3072), the packed nn.LSTM
    word       word_impl = "hip": embedding.word_embedding, one launch forward, one backward
    sentence   sentence_impl = "hip": lstm.sentence_lstm
    both       the two together: every level on the library, ids and lengths on the device
on the same module in one process, the routes alternating window by window (the order rotates).  Per window: ITERS forward +
backward passes between two HIP events (ms per pass: the larger of device time and host enqueue time) and the host's enqueue
time; every window is one JSON line of OUT, the last line the summary: median per route, each route against stock, and the
spread of the stock windows (the yardstick's own noise).

Device time per kernel comes from runs of their own, one per route, without counters:
    ROUTES=word ITERS=20 WINDOWS=2 rocprofv3 --kernel-trace --stats --output-format csv -d DIR_word -- python3 tools/probe_embedding.py
and SUMMARY=DIR_stock,DIR_word,DIR_sentence,DIR_both python3 tools/probe_embedding.py folds the kernel_stats.csv files into one
table (route, kernel, calls, calls per pass, average and total microseconds; a last line per route with the launches per
pass) on stdout -- profiles/embedding_kernel_stats.csv.  A directory's route is the word after its last underscore.

Environment: ITERS (100), WINDOWS (9), ROUTES ("stock,word,sentence,both"), OUT (append the JSON lines to this file), BATCH
(160), HOT (150)."""
import csv
import glob
import json
import os
import statistics
import sys
import time

ITERS = int(os.environ.get("ITERS", "100"))
WINDOWS = int(os.environ.get("WINDOWS", "9"))
ROUTES = os.environ.get("ROUTES", "stock,word,sentence,both").split(",")
IMPLS = {"stock": ("stock", "stock"), "word": ("hip", "stock"), "sentence": ("stock", "hip"), "both": ("hip", "hip")}
WARMUP = 3


def summary(dirs):
    passes = (WARMUP + ITERS * WINDOWS)
    print("Route,Name,Calls,CallsPerPass,AverageUs,TotalUs")
    for d in dirs:
        route = os.path.basename(d.rstrip("/")).rsplit("_", 1)[-1]
        f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))[0]
        launches = total = 0.0
        for r in csv.DictReader(open(f)):
            name = r["Name"]
            name = name if len(name) <= 160 else name[:157] + "..."
            launches += int(r["Calls"]) / passes
            total += float(r["TotalDurationNs"]) / 1e3 / passes
            print('%s,"%s",%s,%.2f,%.2f,%.2f' % (route, name.replace('"', "'"), r["Calls"], int(r["Calls"]) / passes,
                                                 float(r["AverageNs"]) / 1e3, float(r["TotalDurationNs"]) / 1e3))
        print('%s,"ALL KERNELS PER PASS",,%.2f,,%.2f' % (route, launches, total))


def main():
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import vqa_amd  # noqa: F401
    from vqa_amd import embedding, modules as M, train as T

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, Tn, E = int(os.environ.get("BATCH", "160")), 26, 512
    enc = M.QuestionCoAttentionEncoder(10000, E, E).to(dev)
    b = T.synthetic_batch(B, (8, 8), Tn, 10000, 11, seed=1)
    _, q, _, ln = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
    q[:min(B, int(os.environ.get("HOT", "150"))), 0] = 7
    q = q.to(dev)
    lens = {"stock": ln, "hip": ln.to(dev)}
    g = [torch.randn(B, Tn, E, device=dev) for _ in range(3)]
    st = torch.cuda.current_stream(dev)

    def one(route):
        enc.word_impl, enc.sentence_impl = IMPLS[route]
        for p in enc.parameters():
            p.grad = None
        levels = enc(q, lens[enc.sentence_impl])
        torch.autograd.backward(levels, g)

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

    def emit(line):
        print(json.dumps(line), flush=True)
        if os.environ.get("OUT"):
            with open(os.environ["OUT"], "a") as fh:
                fh.write(json.dumps(line) + "\n")

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
    line = {"summary": True, "B": B, "T": Tn, "E": E, "H": E, "V": 10000, "hot_token_on": int(os.environ.get("HOT", "150")),
            "lengths": "sorted, synthetic U{3..26}", "iters": ITERS, "windows": WINDOWS,
            "ms_per_pass": {r: round(v, 4) for r, v in med.items()},
            "host_ms_per_pass": {r: round(statistics.median(v), 4) for r, v in h.items()},
            "bad_ids": embedding.bad_ids(), "device": torch.cuda.get_device_name(dev)}
    if "stock" in med:
        line["stock_spread"] = round((max(t["stock"]) - min(t["stock"])) / med["stock"], 4)
        line["stock_over"] = {r: round(med["stock"] / v, 3) for r, v in med.items() if r != "stock"}
    emit(line)


if __name__ == "__main__":
    if os.environ.get("SUMMARY"):
        summary(os.environ["SUMMARY"].split(","))
    else:
        main()

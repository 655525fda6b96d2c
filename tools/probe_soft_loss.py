"""Developer probe: what training on soft answer targets costs on the hot path.  The isolated hot path -- co-attention forward,
answer head forward + loss, head backward, co-attention backward: graph.HotPathGraph(capture=False).run_eager(), the four
C-ABI calls the Trainer's step issues -- with loss = ce (coattn_head_forward), soft_ce and bce (coattn_head_forward_soft) on the
same modules and inputs in one process, the three variants alternating window by window.

BASELINE cfg 2 (B = 160, T = 26, d = 512, mlp = 1024, K = 1001) at N = 49 and 196, exact mode, location-major features;
questions with descending lengths and zero pad rows; targets of A = 10 slots (slot 0 = the label with score 1, a third of the
others empty).  After a warm-up window per variant, WINDOWS windows of ITERS steps each, timed by HIP events; the median
window per variant and the spread of the ce windows ((max - min) / median) are reported, one JSON line per N.

Under `rocprofv3 --kernel-trace --stats -- python3 tools/probe_soft_loss.py` (ITERS=10 WINDOWS=3 for a short trace) the
kernel table shows the launch counts: soft_rows_kernel<1> and <2> each as often as ce_rows_kernel, head_fwd_kernel /
head_bwd_kernel 4 + 4 per step whatever the loss.

Environment: ITERS (100), WINDOWS (9), SHAPES ("49,196"), OUT (also append the JSON lines to this file)."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vqa_amd  # noqa: E402
from vqa_amd.graph import HotPathGraph  # noqa: E402
from vqa_amd.modules import MLPClassifier  # noqa: E402

B, T, d, MLP, K, A = 160, 26, 512, 1024, 1001, 10
ITERS = int(os.environ.get("ITERS", "100"))
WINDOWS = int(os.environ.get("WINDOWS", "9"))
LOSSES = ("ce", "soft_ce", "bce")


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    co, head = vqa_amd.ParallelCoAttention(d).to(dev), MLPClassifier(d, MLP, K).to(dev)
    st = torch.cuda.current_stream(dev)
    for N in [int(x) for x in os.environ.get("SHAPES", "49,196").split(",")]:
        g = torch.Generator(device=dev).manual_seed(N)
        nodes = {k: HotPathGraph(co, head, B, N, T, capture=False, loss=k, num_answers=A) for k in LOSSES}
        V = torch.relu(torch.randn((B, N, d), device=dev, generator=g))
        lens = torch.tensor(sorted([T] + [3 + (7 * i) % (T - 2) for i in range(B - 1)], reverse=True), device=dev)
        Qs = [torch.randn((B, T, d), device=dev, generator=g) * (2.0 / d) ** 0.5
              * (torch.arange(T, device=dev)[None, :, None] < lens[:, None, None]) for _ in range(3)]
        labels = torch.randint(0, K, (B,), device=dev, generator=g)
        idx = torch.randint(0, K, (B, A), device=dev, generator=g).to(torch.int32)
        score = torch.tensor([0.3, 0.6, 0.9, 1.0], device=dev)[torch.randint(0, 4, (B, A), device=dev, generator=g)]
        empty = torch.rand((B, A), device=dev, generator=g) < 1.0 / 3.0
        idx[empty], score[empty] = -1, 0.0
        idx[:, 0], score[:, 0] = labels.to(torch.int32), 1.0
        for hp in nodes.values():
            hp.V.copy_(V)
            for a, b in zip(hp.Q, Qs):
                a.copy_(b)
            if hp.loss_name == "ce":
                hp.labels.copy_(labels)
            else:
                hp.ans_idx.copy_(idx)
                hp.ans_score.copy_(score)

        def window(kind):
            hp = nodes[kind]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(ITERS):
                hp.run_eager()
            e1.record(st)
            e1.synchronize()
            return e0.elapsed_time(e1) / ITERS

        for k in LOSSES:
            window(k)                                            # warm-up: code objects, first touch of every buffer
        losses = {k: float(nodes[k].loss) for k in LOSSES}
        t = {k: [] for k in LOSSES}
        for w in range(WINDOWS):
            for k in LOSSES[w % 3:] + LOSSES[:w % 3]:            # the order rotates: no variant always runs behind the same one
                t[k].append(window(k))
        med = {k: statistics.median(v) for k, v in t.items()}
        line = {"N": N, "B": B, "T": T, "d": d, "mlp": MLP, "K": K, "A": A, "mode": "exact", "iters": ITERS, "windows": WINDOWS,
                "ce_ms": round(med["ce"], 4), "soft_ce_ms": round(med["soft_ce"], 4), "bce_ms": round(med["bce"], 4),
                "soft_ce_over_ce": round(med["soft_ce"] / med["ce"], 4), "bce_over_ce": round(med["bce"] / med["ce"], 4),
                "ce_spread": round((max(t["ce"]) - min(t["ce"])) / med["ce"], 4),
                "ce_windows_ms": [round(x, 4) for x in t["ce"]], "soft_ce_windows_ms": [round(x, 4) for x in t["soft_ce"]],
                "bce_windows_ms": [round(x, 4) for x in t["bce"]], "loss_values": {k: round(v, 5) for k, v in losses.items()},
                "device": torch.cuda.get_device_name(dev)}
        print(json.dumps(line), flush=True)
        if os.environ.get("OUT"):
            with open(os.environ["OUT"], "a") as fh:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

"""Developer probe: what feature dropout costs on the hot path.  The isolated hot path -- co-attention forward, answer head
forward + loss, head backward, co-attention backward: graph.HotPathGraph -- with dropout p = 0 (the four C-ABI calls of the
parent) and p = 0.5 (coattn_dropout_forward between the forward calls, coattn_dropout_backward between the backward calls) on the
same modules and inputs in one process, the variants alternating window by window; issued eagerly (run_eager) and replayed from
captured HIP graphs (replay).

BASELINE cfg 2 (B = 160, T = 26, d = 512, mlp = 1024, K = 1001) at N = 49 and 196, exact mode, location-major features.  After a
warm-up window per variant, WINDOWS windows of ITERS steps each, timed by HIP events; per variant the median window and the
spread of its windows ((max - min) / median) are reported, one JSON line per (N, mode).

Under `rocprofv3 --kernel-trace --stats -- python3 tools/probe_dropout.py` (ITERS=10 WINDOWS=3 MODES=eager for a short trace)
the kernel table shows dropout_kernel<true> twice per p = 0.5 step and every other kernel as often as without it.

Environment: ITERS (100), WINDOWS (9), SHAPES ("49,196"), MODES ("eager,captured"), PS ("0,0.5": "0" alone also runs on a tree
from before the dropout), TREE (import vqa_amd from this checkout instead of the one the tool lies in: the parent commit, for
the p = 0 comparison on one box), OUT (also append the JSON lines to this file)."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.environ.get("TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vqa_amd  # noqa: E402
from vqa_amd.graph import HotPathGraph  # noqa: E402
from vqa_amd.modules import MLPClassifier  # noqa: E402

B, T, d, MLP, K = 160, 26, 512, 1024, 1001
ITERS = int(os.environ.get("ITERS", "100"))
WINDOWS = int(os.environ.get("WINDOWS", "9"))
PS = tuple(float(x) for x in os.environ.get("PS", "0,0.5").split(","))
MODES = tuple(os.environ.get("MODES", "eager,captured").split(","))


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    co, head = vqa_amd.ParallelCoAttention(d).to(dev), MLPClassifier(d, MLP, K).to(dev)
    st = torch.cuda.current_stream(dev)
    state = vqa_amd.DropoutState(1234, dev) if any(PS) else None
    for N in [int(x) for x in os.environ.get("SHAPES", "49,196").split(",")]:
        g = torch.Generator(device=dev).manual_seed(N)
        V = torch.relu(torch.randn((B, N, d), device=dev, generator=g))
        lens = torch.tensor(sorted([T] + [3 + (7 * i) % (T - 2) for i in range(B - 1)], reverse=True), device=dev)
        Qs = [torch.randn((B, T, d), device=dev, generator=g) * (2.0 / d) ** 0.5
              * (torch.arange(T, device=dev)[None, :, None] < lens[:, None, None]) for _ in range(3)]
        labels = torch.randint(0, K, (B,), device=dev, generator=g)
        for mode in MODES:
            nodes = {p: HotPathGraph(co, head, B, N, T, capture=mode == "captured",
                                     **(dict(dropout=p, dropout_state=state) if p else {})) for p in PS}
            for hp in nodes.values():
                hp.V.copy_(V)
                for a, b in zip(hp.Q, Qs):
                    a.copy_(b)
                hp.labels.copy_(labels)

            def window(p):
                hp = nodes[p]
                step = hp.replay if mode == "captured" else hp.run_eager
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(ITERS):
                    step()
                e1.record(st)
                e1.synchronize()
                return e0.elapsed_time(e1) / ITERS

            for p in PS:
                window(p)                                        # warm-up: code objects, first touch of every buffer
            losses = {p: float(nodes[p].loss) for p in PS}
            t = {p: [] for p in PS}
            for w in range(WINDOWS):
                k = w % len(PS)
                for p in PS[k:] + PS[:k]:                        # the order rotates: no variant always runs behind the same one
                    t[p].append(window(p))
            med = {p: statistics.median(v) for p, v in t.items()}
            line = {"N": N, "B": B, "T": T, "d": d, "mlp": MLP, "K": K, "mode": "exact", "issue": mode, "iters": ITERS,
                    "windows": WINDOWS, "tree": os.environ.get("TREE_NAME", "this"),
                    "version": vqa_amd._lib.load().coattn_version(), "device": torch.cuda.get_device_name(dev)}
            for p in PS:
                key = "p%g" % p
                line[key + "_ms"] = round(med[p], 4)
                line[key + "_spread"] = round((max(t[p]) - min(t[p])) / med[p], 4)
                line[key + "_windows_ms"] = [round(x, 4) for x in t[p]]
                line[key + "_loss"] = round(losses[p], 5)
            if len(PS) > 1:
                line["added_us"] = round((med[PS[1]] - med[PS[0]]) * 1e3, 2)
                line["ratio"] = round(med[PS[1]] / med[PS[0]], 4)
            if state is not None:
                line["masks_drawn"] = state.step()
            print(json.dumps(line), flush=True)
            if os.environ.get("OUT"):
                with open(os.environ["OUT"], "a") as fh:
                    fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

"""Developer probe: what training from cached image features costs against running the frozen encoder in the step.

One process, BASELINE cfg 2 (B = 160, T = 26, d = 512, vocabulary 10,000, K = 1001) at N = 49 (224 px) and N = 196 (448 px),
exact mode, every batch resident on the device.  Per question-side setting -- `stock` and `hip` (--sentence_lstm hip
--word_embedding hip --optimizer hip) -- three step variants on one Trainer each, alternating window by window:
  images  Trainer.step on image batches (two resident batches taking turns, the next one handed over for the encoder run-ahead,
          as train.py does),
  fp32    Trainer.step_features on rows gathered from an fp32 table of S rows (features.gather_features),
  bf16    the same from a bf16 table.
Then the gather kernel alone (`kernel`: the C-ABI call bound once per buffer pair; `wrapper`: features.gather_features, which
adds its Python host time) against the torch line it replaces -- table[idx] for fp32, table[idx].float() for bf16 -- on rotating
index and output buffers over the same tables.

After a warm-up window per variant, WINDOWS windows of ITERS steps (GATHER_ITERS gathers), timed by HIP events; per variant the
median window and the spread of its windows ((max - min) / median), one JSON line per (N, question side) and per (N, dtype).

Under `rocprofv3 --kernel-trace --stats -- python3 tools/probe_cached_features.py` (ITERS=3 WINDOWS=2 GATHER_ITERS=20 for a short
trace) the kernel table shows features_gather_kernel once per cached step.

Environment: ITERS (20), WINDOWS (7), GATHER_ITERS (200), SHAPES ("49,196"), SIDES ("stock,hip"; "none": the gather lines alone),
S (4096), OUT (also append the JSON lines to this file); COATTN_LIB_PATH loads another build of the library (the `lib` key)."""
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

bench.seed_miopen_db()                                          # MIOpen's find records, as bench.py seeds them
import torch  # noqa: E402

import vqa_amd  # noqa: E402
from vqa_amd import _lib, features as FT, train as T  # noqa: E402

B, T_, d, VOCAB, K = 160, 26, 512, 10000, 1001
ITERS = int(os.environ.get("ITERS", "20"))
WINDOWS = int(os.environ.get("WINDOWS", "7"))
GATHER_ITERS = int(os.environ.get("GATHER_ITERS", "200"))
S = int(os.environ.get("S", "4096"))
SIDES = tuple(os.environ.get("SIDES", "stock,hip").split(","))
IMAGE_SIZE = {49: 224, 196: 448}


def emit(line):
    print(json.dumps(line), flush=True)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "a") as fh:
            fh.write(json.dumps(line) + "\n")


def timed(fn, iters, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for i in range(iters):
        fn(i)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(variants, iters, stream):
    """{name: [ms per call of every window]}: a warm-up window each, then WINDOWS rounds in rotating order."""
    names = list(variants)
    for n in names:
        timed(variants[n], iters, stream)
    t = {n: [] for n in names}
    for w in range(WINDOWS):
        k = w % len(names)
        for n in names[k:] + names[:k]:                          # the order rotates: no variant always runs behind the same one
            t[n].append(timed(variants[n], iters, stream))
    return t


def summarise(line, t):
    for n, v in t.items():
        med = statistics.median(v)
        line[n + "_ms"] = round(med, 4)
        line[n + "_spread"] = round((max(v) - min(v)) / med, 4)
        line[n + "_windows_ms"] = [round(x, 4) for x in v]
    return line


def main():
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    common = {"B": B, "T": T_, "d": d, "K": K, "S": S, "windows": WINDOWS, "version": vqa_amd._lib.load().coattn_version(),
              "device": torch.cuda.get_device_name(dev), "lib": os.path.basename(_lib.LIB_PATH)}
    for N in [int(x) for x in os.environ.get("SHAPES", "49,196").split(",")]:
        size = IMAGE_SIZE[N]
        g = torch.Generator(device=dev).manual_seed(N)
        tables = {"fp32": torch.relu(torch.randn((S, N, d), device=dev, generator=g))}
        tables["bf16"] = tables["fp32"].to(torch.bfloat16)
        idx = [torch.randint(0, S, (B,), device=dev, generator=g) for _ in range(8)]
        images = [torch.randn((B, 3, size, size), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
                  for _ in range(2)]
        lens = torch.tensor(sorted([T_] + [3 + (7 * i) % (T_ - 2) for i in range(B - 1)], reverse=True))
        ques = torch.randint(2, VOCAB, (B, T_), device=dev, generator=g) * (torch.arange(T_, device=dev)[None, :] < lens.to(dev)[:, None])
        labels = torch.randint(0, K, (B,), device=dev, generator=g)
        torch.manual_seed(0)
        net0 = T.build_model("attention", VOCAB, K - 1)
        for side in SIDES:
            if side not in ("stock", "hip"):                     # (SIDES=none: the gather lines alone)
                continue
            net = copy.deepcopy(net0).to(dev)
            net.image_encoder.to(memory_format=torch.channels_last)
            kw = dict(sentence_lstm="hip", word_embedding="hip", optimizer="hip") if side == "hip" else {}
            tr = T.Trainer(net, 1e-4, dev, **kw)
            variants = {"images": lambda i: tr.step(images[i & 1], ques, lens, labels, next_image=images[(i + 1) & 1])}
            for name in ("fp32", "bf16"):
                variants[name] = lambda i, tab=tables[name]: tr.step_features(FT.gather_features(tab, idx[i & 7]), ques, lens, labels)
            t = alternate(variants, ITERS, st)
            line = summarise(dict(common, what="step", N=N, image_size=size, question_side=side, iters=ITERS), t)
            line["fp32_over_images"] = round(line["fp32_ms"] / line["images_ms"], 4)
            line["bf16_over_images"] = round(line["bf16_ms"] / line["images_ms"], 4)
            emit(line)
            del tr, net, variants
        del images
        outs = [torch.empty((B, N, d), device=dev) for _ in range(4)]
        for name, tab in tables.items():
            stock = (lambda i, tab=tab: tab[idx[i & 7]]) if name == "fp32" else (lambda i, tab=tab: tab[idx[i & 7]].float())
            # the C-ABI call bound once per (indices, output) pair: the kernel, not the Python wrapper's 12 us of host time
            calls = [_lib.bind("coattn_features_gather", table=tab, table_dtype=_lib.BF16 if name == "bf16" else _lib.F32,
                               idx=idx[k], idx_dtype=_lib.IDS_I64, out=outs[k & 3], bad_idx=None, S=S, B=B, N=N, d=d, flags=0,
                               stream=st.cuda_stream) for k in range(8)]
            t = alternate({"kernel": lambda i: calls[i & 7](), "torch": stock,
                           "wrapper": lambda i, tab=tab: FT.gather_features(tab, idx[i & 7], outs[i & 3])}, GATHER_ITERS, st)
            line = summarise(dict(common, what="gather", N=N, table_dtype=name, iters=GATHER_ITERS,
                                  torch_line="table[idx]" if name == "fp32" else "table[idx].float()"), t)
            moved = B * N * d * (4 + (4 if name == "fp32" else 2))                 # bytes read + written
            line["kernel_TBps"] = round(moved / line["kernel_ms"] / 1e9, 3)
            line["torch_TBps"] = round(moved / line["torch_ms"] / 1e9, 3)
            line["kernel_over_torch"] = round(line["kernel_ms"] / line["torch_ms"], 4)
            emit(line)
        assert FT.bad_indices() == 0
        del tables, outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

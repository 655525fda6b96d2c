#!/usr/bin/env python3
"""Benchmark of the MI355X co-attention path: QA-pairs/sec of the `--model attention` train step.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
(N > 1: either under torch.distributed.run, one rank per GPU, or from a plain shell -- bench.py then
starts the N ranks itself)

Workload (BASELINE.json configs[1], per GPU): HierarchicalCoAttentionNet, K=1000 answers (1001
logits), batch 160, synthetic 224x224 images (-> 7x7x512 grid, N=49), 26-token questions, fp32;
one step = forward + CrossEntropy + backward + Adam (+ RCCL gradient all-reduce when N > 1), all
inputs resident in HBM before the timed region.  Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times
exactly K steps and prints the headline: `value` (QA-pairs/s), `ms_per_step` (one timed step), the run's configuration
and, for N > 1, the ranks and the GPU each ran on.  --dump-outputs DIR then writes what the last timed step computed
(loss, gradients, updated parameters; dump_outputs).  Everything below is measured with --full only; with it the line
also carries
  value_fast16 / exchange  the same step in the tolerance mode (N = 1) / under the other gradient exchanges (N > 1)
ARITHMETIC: everything on the line -- `value`, `roofline`, every per-kernel leg, `hot_path` -- runs the reference's arithmetic:
fp32 storage and accumulation, fp32-ACCURATE products (C-ABI flags = 0, train.Trainer's default: three bf16 pieces per operand, six
partial products per fp32 product).  The opt-in tolerance mode (22-bit forward / 16-bit backward products) appears only under
keys that say so: value_fast16, roofline_fast16, roofline_reference_grid_fast16, roofline_backward_fast16,
hot_path[*].fast16_*, roofline_projection.fast16_f16_pair, roofline_weight_grad.fast16_two_pieces.
  roofline      the fused affinity+softmax+reduce forward kernel, timed live with HIP events on the launch stream AT THE TIMED
                STEP'S OWN SHAPE (B=160, N=49, T=26, d=512, location-major as the train step hands features over):
                algorithmic bytes per (pair, level) (SURVEY.md 8d's formula at that N) / avg launch time, against 8 TB/s HBM.
                COLD: consecutive launches rotate over >= 4 independent buffer sets totalling > 640 MiB, so a launch never finds
                its operands in the 256 MiB Infinity Cache; frac_warm = ONE set replayed (what rounds 1-5 reported);
                in_step_us / frac_in_step = the kernel between the library's own events inside forward + backward sequences;
                roofline_reference_grid: the same kernel at the reference's default grid (N=196: 913,408 B
                per (pair, level)), roofline_channel_major: on the reference's own layout
  roofline_backward  every kernel of coattn_backward, at both grids: average time between HIP events the
                library records around its launches (coattn_profile_begin / _end) inside forward + backward pairs that rotate
                over three buffer sets, algorithmic bytes against HBM -- the GEMM launch: algorithmic
                flops against the dense bf16 MFMA peak / partial products per fp32 product of its width (6: exact)
  cpu_baseline  the CPU oracle port (oracle/net_oracle.py) of the same train step, timed on the
                host cores on a bounded sample (rank 0, N=1 only); cpu_baseline_hot_path: the oracle
                port of the isolated hot path (co-attention + MLP + CE fwd+bwd) at N=196 and N=49
  roofline_projection  the MFMA-bound P_v projection GEMM (gemm_w_kernel, three-piece form), timed the same way over four rotating
                operand buffers: fp32-equivalent TFLOP/s against the dense 16-bit MFMA peak / 6 (three bf16 pieces per operand:
                six partial products per fp32 product, the form coattn_forward runs it in at flags = 0);
                roofline_weight_grad: the same for its weight gradient dW_v (gemm_tn_kernel + reduce)
  hot_path      isolated co-attention (+MLP+CE) fwd+bwd rates on device-resident features, N=196
                and N=49, both feature layouts, as train.Trainer.step runs it (one autograd node over static buffers,
                C-ABI calls issued eagerly); host_enqueue_ms = host time to queue one step; modules_*: the same step
                module by module (ParallelCoAttention -> MLPClassifier.forward_loss); graph_*: replayed from captured
                HIP graphs (vqa_amd/graph.py); the HIP op's fwd+bwd device time (pipelined calls) and the wall time
                of single synchronised calls.  The synthetic questions have pad rows (question_pad_row_fraction: exact zeros,
                as the reference's hierarchy leaves them), which the exact mode leaves out of two contractions;
                dense_questions_coattn_fwd_bwd_ms is the same measurement on questions without any.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ALG_BYTES_PER_PAIR_LEVEL = lambda N, T, d: 4 * (T * d + d * N + N * d + T * d + 2 * d)   # Q + V + P_v + P_q + v,q
HBM_PEAK_GBS = 8000.0

MIOPEN_DB_SEED = os.path.join(ROOT, "miopen_db")     # committed: MIOpen find records of the default workload on an MI355X


def seed_miopen_db():
    """The first forward of every convolution shape runs MIOpen's find step, which times each applicable solver: about 40 s
    for the eight VGG layers of the default workload, before the first step, wherever MIOpen has no records yet.  MIOpen
    keeps those records in its user database (MIOPEN_USER_DB_PATH, by default ~/.config/miopen); every committed record file
    of MIOPEN_DB_SEED that the database lacks is copied into it here, so that MIOpen runs the solvers those records rank
    first, without timing runs.  A file already there is left alone (shapes it does not hold are found and added as usual).
    Where that directory cannot be written, a temporary one, removed at exit, is seeded and used instead (for MIOpen's kernel
    cache as well, unless MIOPEN_CUSTOM_CACHE_DIR is set); if that fails too, the run goes on without the seed.  Nothing is written into the repository.  Called before anything calls MIOpen;
    ranks started by self_launch inherit the environment."""
    import atexit
    import shutil
    import tempfile
    if not os.path.isdir(MIOPEN_DB_SEED):
        return
    seed = [f for f in os.listdir(MIOPEN_DB_SEED) if f.endswith(".txt")]

    def fill(d):
        os.makedirs(d, exist_ok=True)
        for f in seed:
            dst = os.path.join(d, f)
            if not os.path.exists(dst):
                tmp = "%s.%d.tmp" % (dst, os.getpid())          # (renamed into place: a concurrent run never reads half a file)
                shutil.copyfile(os.path.join(MIOPEN_DB_SEED, f), tmp)
                os.replace(tmp, dst)

    try:
        fill(os.environ.get("MIOPEN_USER_DB_PATH") or os.path.join(os.path.expanduser("~"), ".config", "miopen"))
        return
    except OSError:
        pass
    try:
        d = tempfile.mkdtemp(prefix="miopen_db_")
        atexit.register(shutil.rmtree, d, True)
        fill(d)
    except OSError:
        return
    os.environ["MIOPEN_USER_DB_PATH"] = d
    # (an unwritable home also denies MIOpen its kernel cache, ~/.cache/miopen, and MIOpen then fails the first convolution)
    os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", os.path.join(d, "cache"))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch", type=int, default=160, help="per-GPU batch (BASELINE config 2: 160)")
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--num-cls", type=int, default=1000)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--seq-len", type=int, default=26)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline legs")
    ap.add_argument("--no-extras", action="store_true", help="--full: skip the tolerance-mode step and the roofline / hot_path legs")
    ap.add_argument("--no-configs", action="store_true",
                    help="--full: skip the compact config4 / config5 objects (BASELINE configs[3], [4])")
    ap.add_argument("--only", type=str, default="", help="developer switch: run only 'roofline' or 'hot' legs")
    ap.add_argument("--cpu-batch", type=int, default=0, help="batch of the CPU baseline leg (0: the GPU step's own batch)")
    ap.add_argument("--exchange-p2p", action="store_true",
                    help="N > 1: also time the step under exchange='p2p' (peer-mapped buckets + csrc/p2p.hip)")
    ap.add_argument("--no-runahead", dest="runahead", action="store_false",
                    help="run the frozen image encoder in series with the rest of the step (default: one step "
                         "ahead on its own HIP stream)")
    ap.add_argument("--model", default="attention", choices=["attention", "attention_resnet", "attention_bert"],
                    help="attention (BASELINE config 2 / 3, the headline); attention_resnet + --opt-lvl 1 --num-cls 3000 is "
                         "BASELINE config 4; attention_bert is BASELINE config 5 (frozen BERT-base token embeddings, 768-d, as "
                         "the word level; run it with --gpus 4)")
    ap.add_argument("--opt-lvl", type=int, default=0, help="developer switch: >0 = bf16 autocast (not the headline)")
    ap.add_argument("--precision", default="exact", choices=["fast", "exact"],
                    help="fp32 products of the HIP path in the timed step: fp32-accurate (default: the reference's arithmetic, "
                         "flags = 0, train.Trainer's default) or the opt-in tolerance mode (include/coattn.h COATTN_FLAG_FAST16)")
    ap.add_argument("--stock-graph", action="store_true",
                    help="run the frozen encoder's Sequential as is (default: ReLU/MaxPool swap and conv bias folded "
                         "into BatchNorm's running mean, modules.run_conv_bn_stack; same stock kernels, same values)")
    ap.add_argument("--nchw", dest="channels_last", action="store_false",
                    help="keep the stock VGG encoder in NCHW (default: channels_last, MIOpen NHWC kernels, ~25 %% "
                         "faster forward; its first call tunes for up to a minute)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the tolerance-mode step, the exchange legs (N > 1), the roofline / per-kernel / "
                         "hot_path legs, configs 4 and 5 and the CPU baselines (default: the headline step only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write what the last one computed (loss, gradients, updated parameters) "
                         "as float32 DIR/<name>.npy, a fixed sample of each large tensor where the whole exceeds 60 MiB")
    return ap.parse_args()


def synth_features(B, N, T, d, device, seed=1234, L=3, dense=False):
    """Device-resident synthetic features of the isolated path: V = relu(N(0,1)) stored
    channel-major [B,d,N], Q_l ~ N(0,1) [B,T,d] with rows past each (descending) length zeroed (dense: every question T
    tokens long, no pad rows -- the case in which the exact mode's zero-row paths have nothing to skip)."""
    g = torch.Generator().manual_seed(seed)
    V = torch.randn(B, d, N, generator=g).clamp_min_(0)
    lens = torch.tensor([T] * B if dense else sorted([T] + [3 + (7 * i) % (T - 2) for i in range(B - 1)], reverse=True))
    mask = (torch.arange(T)[None, :] < lens[:, None]).unsqueeze(-1).float()
    Qs = [(torch.randn(B, T, d, generator=g) * mask).to(device) for _ in range(L)]
    return V.to(device), Qs


def synth_pad_fraction(B, T):
    """Share of the question rows of synth_features that are pad rows (exact zeros): lengths [T] + [3 + (7 i) % (T - 2)]."""
    lens = [T] + [3 + (7 * i) % (T - 2) for i in range(B - 1)]
    return round(1.0 - sum(lens) / float(B * T), 4)


PAD_NOTE = ("pad rows of the questions are exact zeros (as the reference's hierarchy leaves them: model.py:263, :292-296); the exact mode "
            "finds them from the data and leaves them out of the P_q projection and of dW_q (bit-identical P_q; include/coattn.h)")


def device_batch(T, args, rank, device, batch=None, image_size=None):
    b = T.synthetic_batch(batch or args.batch, (image_size or args.image_size,) * 2, args.seq_len, args.vocab,
                          args.num_cls + 1, seed=1234 + rank)
    image, question, label, lens = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
    return image.to(device), question.to(device), lens, label.to(device)


PRIME_STEPS = 2      # untimed, before the W warm-up steps: MIOpen kernel selection, lazy library loads, reducer layout


def timed_steps(trainer, batch, steps, warmup, sync):
    """W untimed warm-up steps, then exactly K timed steps between two device+rank synchronisations; returns the
    seconds between them and the last step's loss.
    Every step is handed the next step's image batch (here: the same resident synthetic batch), so the
    frozen image encoder of step i+1 is queued on its own stream while step i's remaining work runs;
    each timed step still launches exactly one encoder forward, and the closing synchronisation waits
    for all streams."""
    nxt = batch[0]
    for _ in range(PRIME_STEPS + warmup):
        trainer.step(*batch, next_image=nxt)
    sync()
    t0 = time.perf_counter()
    loss = None
    for _ in range(steps):
        loss = trainer.step(*batch, next_image=nxt)
    sync()
    return time.perf_counter() - t0, loss


DUMP_BYTES = 60 * 2 ** 20      # --dump-outputs writes at most this much (one step of the default model holds ~100 MB)
DUMP_WHOLE = 1 << 16           # tensors of at most this many elements are always written whole


def dump_outputs(path, model, loss):
    """--dump-outputs: what the timed step hands its caller, from its last step -- the loss, the gradient of every trainable
    parameter and the parameter after the optimiser update -- as float32 <path>/<name>.npy (loss, grad.<param>,
    param.<param>).  When the whole set exceeds DUMP_BYTES, every tensor above DUMP_WHOLE elements is written as a fixed
    sample of its flattened entries (the same fraction for all of them): sorted positions drawn from a generator seeded by
    the file name, so runs with the same arguments write the same positions."""
    import zlib

    import numpy as np
    arrays = [("loss", loss.detach().reshape(1))]
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if p.grad is not None:
            arrays.append(("grad." + name, p.grad))
        arrays.append(("param." + name, p))
    n_whole = sum(t.numel() for _, t in arrays if t.numel() <= DUMP_WHOLE)
    n_big = sum(t.numel() for _, t in arrays if t.numel() > DUMP_WHOLE)
    frac = min(1.0, max(0, DUMP_BYTES // 4 - n_whole) / max(n_big, 1))
    os.makedirs(path, exist_ok=True)
    n_bytes = 0
    for name, t in arrays:
        x = t.detach().float().cpu()
        if x.numel() > DUMP_WHOLE and frac < 1.0:
            g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
            x = x.reshape(-1)[torch.randperm(x.numel(), generator=g)[:int(x.numel() * frac)].sort().values]
        np.save(os.path.join(path, name + ".npy"), x.numpy())
        n_bytes += x.numel() * 4
    print("bench.py: wrote %d arrays (%.1f MB%s) to %s" % (len(arrays), n_bytes / 1e6,
                                                          ", sampled %.3f of each large tensor" % frac if frac < 1.0 else "",
                                                          path), file=sys.stderr)


def _lib_flag(bf16, fast=False):
    """C-ABI flags of a leg: the reduced-precision mode (config 4), else flags = 0 -- fp32-accurate products, the reference's
    arithmetic and the C-ABI's / the nn.Modules' / train.Trainer's default (include/coattn.h "Widths of the fp32 mode") -- or,
    fast, the opt-in tolerance mode (COATTN_FLAG_FAST16), reported on the side keys only."""
    from vqa_amd import _lib
    return _lib.FLAG_BF16_PROJ if bf16 else (_lib.FLAG_FAST16 if fast else 0)


PRODUCTS = {"exact": "fp32-accurate: 3 x bf16 pieces per operand (hi + mid + lo = the fp32 value exactly), 6 partial products on "
                     "v_mfma_f32_32x32x16_bf16, fp32 accumulation (flags = 0)",
            "fast16": "tolerance mode (opt-in, COATTN_FLAG_FAST16): forward products on 2 x fp16 pieces = 22 significand bits, "
                      "backward products on 2 x bf16 pieces = 16 bits, 3 partial products each",
            "bf16": "reduced-precision mode: operands rounded to bf16, ONE MFMA per product (COATTN_FLAG_BF16_PROJ)"}

ARITHMETIC = ("fp32 storage and accumulation; fp32-accurate products (flags = 0, train.Trainer's default: every product of the HIP "
              "path on 3 x bf16 pieces per operand = 24 significand bits, 6 partial products: one fp32 rounding per product, as the "
              "reference's fp32 bmm / Linear); answer head: exact fp32 MFMA; stock encoders: fp32.  The opt-in tolerance mode "
              "(--precision fast: 22-bit forward / 16-bit backward products) is timed beside it on the *_fast16 keys only")


def _mode(bf16, fast):
    return "bf16" if bf16 else ("fast16" if fast else "exact")


def hot_path_leg(device, N, layout="lm", B=160, T=26, d=512, K=1000, iters=20, bf16=False):
    """Isolated hot path (co-attention + MLPClassifier + CE, fwd+bwd) on resident features.
    layout: "lm" = x_img contiguous [B,N,d] (what the channels_last encoder of the train step hands over),
    "cm" = the permuted view of a channel-major [B,d,N] buffer (the reference's NCHW encoder, model.py:215-217)."""
    import gc
    import vqa_amd
    from vqa_amd.modules import MLPClassifier
    # (the previous leg's captured graphs and their memory pools die in a garbage-collection pass -- reference cycles through
    #  the autograd nodes -- and destroying them takes milliseconds: not inside this leg's timed loops)
    gc.collect()
    torch.cuda.synchronize()
    torch.manual_seed(0)
    co = vqa_amd.ParallelCoAttention(d).to(device)
    co.bf16_projections = bf16                       # the reduced-precision mode of --opt_lvl >= 1 (config 4)
    co.fast_products = False                         # fp32-accurate products: train.Trainer's default (precision="exact")
    mlp = MLPClassifier(d, 1024, K + 1).to(device)
    mlp.bf16_products = bf16
    V, Qs = synth_features(B, N, T, d, device)
    x_img = V.permute(0, 2, 1)
    if layout == "lm":
        x_img = x_img.contiguous()
    Qs = [q.requires_grad_(True) for q in Qs]
    label = (torch.arange(B, device=device) * 7) % (K + 1)
    params = [p for p in list(co.parameters()) + list(mlp.parameters())]

    def mstep():                                     # module by module: ParallelCoAttention -> MLPClassifier.forward_loss
        for p in params:
            p.grad = None
        _, loss = mlp.forward_loss(*co(x_img, Qs), label)
        loss.backward()

    def timed(fn):
        """(wall per step, host time to ENQUEUE a step) over `iters` pipelined steps: the median of three windows (one host
        hiccup -- an allocator trim, a page fault in a fresh buffer -- used to own a whole leg's number)."""
        for _ in range(5):
            fn()
        wins = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            wins.append(((time.perf_counter() - t0) / iters, (t1 - t0) / iters))
        return sorted(wins)[1]

    mdt, mhost = timed(mstep)
    # as train.Trainer.step runs it by default: the hot path as ONE autograd node over static buffers, its four C-ABI calls
    # issued eagerly, the static gradient buffers assigned to param.grad (graph.py, capture=False, direct_grads=True) ...
    from vqa_amd.graph import HotPathGraph
    hs = HotPathGraph(co, mlp, B, N, T, flags=_lib_flag(bf16), capture=False, direct_grads=True)      # (flags = 0 unless bf16)
    # ... and replayed from captured HIP graphs (Trainer(graph=True))
    hp = HotPathGraph(co, mlp, B, N, T, flags=_lib_flag(bf16), direct_grads=True)

    def make_step(h):
        def f():
            for p in params:
                p.grad = None
            for q in Qs:
                q.grad = None
            _, loss = h(x_img, Qs, label)
            loss.backward()
        return f

    dt, host = timed(make_step(hs))
    gdt, ghost = timed(make_step(hp))
    xdt = None
    if not bf16:                                     # the same eager node in the opt-in tolerance mode (--precision fast)
        del hp
        hx = HotPathGraph(co, mlp, B, N, T, flags=_lib_flag(False, fast=True), capture=False, direct_grads=True)
        xdt, _ = timed(make_step(hx))
    # forward + backward of the HIP op alone (C-ABI calls through the autograd function):
    #  (a) device time of a pipelined run (HIP events around `iters` back-to-back fwd+bwd calls: what the train
    #      loop sees, the host runs ahead of the GPU);
    #  (b) wall time of a single forward / backward call between two device synchronisations (adds the launch
    #      latency and the host side of one call).
    args = (co.W_v.weight, co.W_v.bias, co.W_q.weight, co.W_q.bias, co.w_v.weight, co.w_v.bias, co.w_q.weight,
            co.w_q.bias)
    gv = torch.ones(3, B, d, device=device)
    gq = torch.ones(3, B, d, device=device)
    impl = _lib_flag(bf16)

    leaves = list(args) + list(Qs)

    def fb():
        for p in leaves:                           # optimizer.zero_grad() of the train loop (set_to_none): without it
            p.grad = None                          # autograd adds each new gradient onto the old one (11 add kernels)
        v, q = vqa_amd.coattention(x_img, Qs, *args, impl=impl)
        torch.autograd.backward([v, q], [gv, gq])

    for _ in range(2 * iters):                     # clock warm-up (see roofline_leg): ~40 ms of back-to-back calls
        fb()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3 * iters):
        fb()
    e1.record()
    torch.cuda.synchronize()
    t_autograd = e0.elapsed_time(e1) * 1e-3 / (3 * iters)      # (through the autograd function: host-paced on a slow host)
    # the two C-ABI calls themselves, back to back from pre-built argument blocks: device-paced whatever the host
    # (channel-major rows that are not 16-byte multiples -- N = 49 -- are re-laid once by the module before the call: the
    #  calls themselves then see location-major features)
    lay_c = layout if (layout == "lm" or N % 4 == 0) else "lm"
    t_dev = coattn_device_time(device, B=B, N=N, T=T, d=d, layout=lay_c, bf16=bf16)
    t_dev_x = None if bf16 else coattn_device_time(device, B=B, N=N, T=T, d=d, layout=lay_c, fast=True)
    # ... and with questions that have NO pad rows: what the exact mode costs when there is nothing for its zero-row paths to skip
    t_dev_dense = None if bf16 else coattn_device_time(device, B=B, N=N, T=T, d=d, layout=lay_c, dense=True)
    fwd = bwd = 0.0
    for it in range(iters + 3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        v, q = vqa_amd.coattention(x_img, Qs, *args, impl=impl)
        for p in leaves:
            p.grad = None
        torch.cuda.synchronize(); t1 = time.perf_counter()
        torch.autograd.backward([v, q], [gv, gq])
        torch.cuda.synchronize(); t3 = time.perf_counter()
        if it >= 3:
            fwd += t1 - t0; bwd += t3 - t1
    flop = 3.0 * B * (2 * N * d * d + 3 * 2 * T * d * d + 3 * (3 * 2 * T * N * d + 4 * (N + T) * d))
    return {"N": N, "d": d, "K": K, "layout": layout, "question_pad_row_fraction": synth_pad_fraction(B, T),
            "mode": ("reduced precision (every product ONE bf16 MFMA, fp32 accumulation; dP_v / dP_q stored as bf16)" if bf16 else
                     "fp32-accurate products (flags = 0: 3 x bf16 pieces per operand, 6 partial products); fast16_*: the opt-in tolerance mode "
                     "(forward products 2 x fp16 pieces = 22 bits, backward 2 x bf16 = 16 bits)"),
            "precision": "bf16" if bf16 else "exact",
            "pairs_per_s": round(B / dt, 1), "ms_per_step": round(dt * 1e3, 3), "host_enqueue_ms": round(host * 1e3, 3),
            "fast16_ms_per_step": round(xdt * 1e3, 3) if xdt is not None else None,
            "fast16_coattn_fwd_bwd_ms": round(t_dev_x * 1e3, 4) if t_dev_x is not None else None,
            "dense_questions_coattn_fwd_bwd_ms": round(t_dev_dense * 1e3, 4) if t_dev_dense is not None else None,
            "step_path": "train.Trainer's default: one autograd node over static buffers, C-ABI calls issued eagerly",
            "modules_ms_per_step": round(mdt * 1e3, 3), "modules_host_enqueue_ms": round(mhost * 1e3, 3),
            "graph_ms_per_step": round(gdt * 1e3, 3), "graph_host_enqueue_ms": round(ghost * 1e3, 3),
            "graph_pairs_per_s": round(B / gdt, 1),
            "coattn_fwd_bwd_ms": round(t_dev * 1e3, 4), "coattn_fwd_bwd_tflops": round(flop / t_dev / 1e12, 2),
            "coattn_fwd_bwd_note": "device time of coattn_forward + coattn_backward (C-ABI calls back to back, HIP events); "
                                   "coattn_fwd_bwd_autograd_ms: the same through the autograd function (host-paced on a slow host)",
            "coattn_fwd_bwd_autograd_ms": round(t_autograd * 1e3, 4),
            "coattn_fwd_wall_ms": round(fwd / iters * 1e3, 4), "coattn_bwd_wall_ms": round(bwd / iters * 1e3, 4),
            "coattn_fwd_bwd_wall_tflops": round(flop / ((fwd + bwd) / iters) / 1e12, 2)}


ROOFLINE_SKIP_WARM = False       # tools/probe_fwd_one.py: profile the cold rotation alone
COLD_BYTES = 640 << 20          # a rotation of buffer sets is "cold" when it touches more than this between two uses of a set
                                # (MI355X_MICROARCH.md: 256 MiB Infinity Cache; VERDICT r5 asks for > 512 MiB over >= 4 sets)


def _fwd_set(lib, device, co_params, B, N, T, d, L, layout, flags, seed):
    """One independent set of buffers of the fused forward (features, `saved`, workspace, outputs) with P_v / P_q already in
    `saved`; returns (argument tuple of coattn_attention_forward, bytes the kernel touches in this set, keep-alive)."""
    import ctypes as C
    from vqa_amd import _lib
    V, Qs = synth_features(B, N, T, d, device, seed=seed, L=L)
    vstr = (d * N, 1, N)
    if layout == "lm":
        V, vstr = V.permute(0, 2, 1).contiguous(), (N * d, d, 1)
    sb, fb, _ = _lib.workspace_bytes(B, N, T, d, L, flags)
    saved = torch.empty(sb // 4, device=device); ws = torch.empty(fb // 4, device=device)
    v = torch.empty(L, B, d, device=device); q = torch.empty(L, B, d, device=device)
    qptr = (C.c_void_p * L)(*[t.data_ptr() for t in Qs])
    p = _lib.Params(*[t.data_ptr() for t in co_params])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (V.data_ptr(), *vstr, qptr, C.byref(p), v.data_ptr(), q.data_ptr(), saved.data_ptr(), ws.data_ptr(),
            B, N, T, d, L, _lib.F32, flags, stream)
    _lib.check(lib.coattn_forward(*args), "coattn_forward")          # fills P_v / P_q in `saved`
    # what one launch reads and writes in THIS set: V, the Q_l, P_v, P_q (read); C, a_v, a_q, H_q, v, q (written)
    touched = 4 * (B * N * d * 2 + L * B * T * d * 3 + L * B * (T * N + N + T) + 2 * L * B * d)
    return args, touched, (V, Qs, saved, ws, v, q, qptr, p)


def roofline_leg(device, B=160, N=196, T=26, d=512, L=3, iters=100, layout="lm", fast=False, bf16=False, cold=True):
    """Average launch duration of the affinity+softmax+reduce forward kernel(s), HIP events on the
    launch stream (= torch's current stream, which the C-ABI call is given).  layout: physical layout of the
    image features, "lm" [B,N,d] (channels_last encoder: the train step's default) or "cm" [B,d,N] (NCHW).
    COLD (the headline `frac`): consecutive launches rotate over >= 4 independent buffer sets that together exceed
    COLD_BYTES, so no launch finds its operands in the 256 MiB Infinity Cache (in the train step >= 1 GB of other traffic
    separates two launches); `frac_warm` = the same kernel replayed on ONE set (what earlier rounds reported: its 113 MB /
    217 MB working set stays cache-resident); `in_step_us` = its average between the library's own events inside a
    coattn_forward + coattn_backward sequence on rotating sets."""
    import vqa_amd
    from vqa_amd import _lib
    lib = _lib.load()
    fused = bool(lib.coattn_fused_supported(B, N, T, d, L, _lib.F32))
    torch.manual_seed(0)
    co = vqa_amd.ParallelCoAttention(d).to(device)
    ps = [t.detach().contiguous() for t in (co.W_v.weight, co.W_v.bias, co.W_q.weight, co.W_q.bias, co.w_v.weight,
                                           co.w_v.bias, co.w_q.weight, co.w_q.bias)]
    flags = _lib_flag(bf16, fast)
    sets = [_fwd_set(lib, device, ps, B, N, T, d, L, layout, flags, seed=77)]
    touched = sets[0][1]
    nsets = max(4, -(-COLD_BYTES // touched) + 1) if cold else 1
    for k in range(1, nsets):
        sets.append(_fwd_set(lib, device, ps, B, N, T, d, L, layout, flags, seed=77 + k))
    calls = [a for a, _, _ in sets]
    iters = -(-iters // nsets) * nsets                # whole rotations
    for a in calls:
        _lib.check(lib.coattn_attention_forward(*a), "coattn_attention_forward")
    # Warm-up: the set-up above (weight init, synthetic features, the projection GEMMs) leaves the GPU idle for
    # milliseconds and its clocks ramp back over the first ~30 ms of load -- 100-call windows started cold read
    # 97-101, 91, 87 us per call; so 3 x `iters` untimed calls first, then three timed windows of `iters` calls each,
    # the median window's average (all three are in the line: `windows_us`).

    def windows(cs):
        n = len(cs)
        for k in range(3 * iters):
            lib.coattn_attention_forward(*cs[k % n])
        ts = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(iters):
                lib.coattn_attention_forward(*cs[k % n])
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3 / iters)
        return ts

    ts = windows(calls)
    t = sorted(ts)[1]
    ts_warm = windows(calls[:1]) if (cold and not ROOFLINE_SKIP_WARM) else ts
    t_warm = sorted(ts_warm)[1]
    del sets, calls
    alg = B * L * ALG_BYTES_PER_PAIR_LEVEL(N, T, d)
    ach = alg / t / 1e9
    mode = _mode(bf16, fast)
    in_step = None
    if cold and fused:
        seq = sequence_marks(device, B, N, T, d, L, layout, bf16, fast)
        in_step = sum(us for nm, us in seq["avg_us"].items() if nm in ("coattn_fwd32", "attend_v"))
    traffic = traffic_src = None                   # HBM bytes per launch from the committed rocprofv3 PMC passes
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as fh:
            tr = json.load(fh)
        for e in (tr["entries"] if "entries" in tr else [tr]):
            if (e.get("shape") == {"B": B, "N": N, "T": T, "d": d, "L": L} and e.get("layout", "cm") == layout
                    and e.get("products", "bf16" if d == 2048 else "fast16") == mode):
                traffic = e["hbm_bytes_per_launch"]
                traffic_src = ("profiles/pmc_traffic.json (rocprofv3 FETCH_SIZE / WRITE_SIZE passes of this kernel at this shape "
                               "and in this arithmetic, %s; committed, not measured by this run)"
                               % ("launches rotating over buffer sets: cold" if e.get("cold") else "ONE buffer set replayed: warm"))
    except (OSError, ValueError, KeyError):
        pass
    return {"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_src,
            "cold": bool(cold), "buffer_sets": nsets, "bytes_touched_per_rotation": nsets * touched,
            "frac_warm": round(alg / t_warm / 1e9 / HBM_PEAK_GBS, 4), "avg_launch_us_warm": round(t_warm * 1e6, 2),
            "in_step_us": round(in_step, 2) if in_step is not None else None,
            "frac_in_step": round(alg / (in_step * 1e-6) / 1e9 / HBM_PEAK_GBS, 4) if in_step else None,
            "kernel": "coattn_attention_fwd (affinity+tanh, H_v/H_q, scores, row-softmax, attended reductions)"
                      + (" [fused]" if fused else " [general-shape kernel sequence]"),
            "products": PRODUCTS[mode],
            "shape": {"B": B, "N": N, "T": T, "d": d, "L": L}, "v_layout": layout, "avg_launch_us": round(t * 1e6, 2),
            "windows_us": [round(x * 1e6, 2) for x in ts], "calls_per_window": iters,
            "algorithmic_bytes": alg}


def coattn_c_calls(device, B, N, T, d, L, layout, bf16, fast=False, seed=78, dense=False):
    """coattn_forward / coattn_backward (frozen image encoder: no dV) as closures over pre-built argument blocks on synthetic
    features: (lib, stream, fwd, bwd).  A call costs the host one ctypes crossing, so loops over them are device-paced."""
    import ctypes as C
    import vqa_amd
    from vqa_amd import _lib
    lib = _lib.load()
    torch.manual_seed(0)
    co = vqa_amd.ParallelCoAttention(d).to(device)
    V, Qs = synth_features(B, N, T, d, device, seed=seed, L=L, dense=dense)
    vstr = (d * N, 1, N)
    if layout == "lm":
        V, vstr = V.permute(0, 2, 1).contiguous(), (N * d, d, 1)
    ps = [t.detach().contiguous() for t in (co.W_v.weight, co.W_v.bias, co.W_q.weight, co.W_q.bias, co.w_v.weight,
                                           co.w_v.bias, co.w_q.weight, co.w_q.bias)]
    flags = _lib_flag(bf16, fast)
    sb, fb, bb = _lib.workspace_bytes(B, N, T, d, L, flags)
    saved = torch.empty(sb // 4, device=device); ws = torch.empty(max(fb, bb) // 4, device=device)
    v = torch.empty(L, B, d, device=device); q = torch.empty(L, B, d, device=device)
    gv = torch.randn(L, B, d, device=device) * 0.1; gq = torch.randn(L, B, d, device=device) * 0.1
    dQs = [torch.empty_like(t) for t in Qs]
    grads = [torch.empty_like(t) for t in ps]
    qptr = (C.c_void_p * L)(*[t.data_ptr() for t in Qs])
    dqptr = (C.c_void_p * L)(*[t.data_ptr() for t in dQs])
    p = _lib.Params(*[t.data_ptr() for t in ps])
    pg = _lib.ParamGrads(*[t.data_ptr() for t in grads])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.coattn_forward(V.data_ptr(), *vstr, qptr, C.byref(p), v.data_ptr(), q.data_ptr(), saved.data_ptr(),
                                  ws.data_ptr(), B, N, T, d, L, _lib.F32, flags, stream), "coattn_forward")

    def fwd():
        return lib.coattn_forward(V.data_ptr(), *vstr, qptr, C.byref(p), v.data_ptr(), q.data_ptr(), saved.data_ptr(),
                                  ws.data_ptr(), B, N, T, d, L, _lib.F32, flags, stream)

    def bwd():
        return lib.coattn_backward(V.data_ptr(), *vstr, qptr, C.byref(p), saved.data_ptr(), gv.data_ptr(), gq.data_ptr(),
                                   None, 0, 0, 0, dqptr, C.byref(pg), 0, ws.data_ptr(), B, N, T, d, L, _lib.F32, flags, stream)

    _lib.check(bwd(), "coattn_backward")
    fwd.keep = bwd.keep = (V, Qs, ps, saved, ws, v, q, gv, gq, dQs, grads, qptr, dqptr, p, pg)   # (the closures' buffers)
    return lib, stream, fwd, bwd


def coattn_device_time(device, B=160, N=196, T=26, d=512, L=3, layout="lm", bf16=False, iters=50, fast=False, dense=False):
    """Device time of one coattn_forward + coattn_backward (HIP events around `iters` back-to-back pairs of C-ABI calls, the
    median of three windows after a clock warm-up)."""
    lib, stream, fwd, bwd = coattn_c_calls(device, B, N, T, d, L, layout, bf16, fast, dense=dense)
    for _ in range(2 * iters):
        fwd(); bwd()
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fwd(); bwd()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3 / iters)
    return sorted(ts)[1]


_SEQ_CACHE = {}


def sequence_marks(device, B, N, T, d, L, layout, bf16, fast, iters=60, nsets=3):
    """Every launch group of coattn_forward + coattn_backward IN SEQUENCE (frozen image encoder: no dV, the train step's case),
    timed by the HIP events the library records between its launches (coattn_profile_begin / coattn_profile_end) and averaged
    over `iters` forward + backward pairs after a clock warm-up.  Consecutive pairs rotate over `nsets` independent buffer
    sets (a pair moves ~0.4 GB at N = 49, ~0.9 GB at N = 196: three sets put > 1 GB between two uses of a buffer), so every
    kernel finds in the Infinity Cache only what the kernels right before it left there -- as in the train step.
    Cached per (shape, layout, arithmetic): the forward roofline leg and the backward legs share one measurement."""
    import ctypes as C
    from vqa_amd import _lib
    key = (B, N, T, d, L, layout, bf16, fast)
    if key in _SEQ_CACHE:
        return _SEQ_CACHE[key]
    pairs = [coattn_c_calls(device, B, N, T, d, L, layout, bf16, fast, seed=78 + k) for k in range(nsets)]
    lib, stream = pairs[0][0], pairs[0][1]
    for k in range(2 * iters):                         # clock warm-up (see roofline_leg)
        pairs[k % nsets][2](); pairs[k % nsets][3]()
    us = (C.c_float * 48)()
    names = C.create_string_buffer(2048)
    tot, order = {}, []
    for k in range(iters):
        _, _, fwd, bwd = pairs[k % nsets]
        _lib.check(lib.coattn_profile_begin(stream), "coattn_profile_begin")
        fwd(); bwd()
        n = lib.coattn_profile_end(us, names, 2048, 48)
        if n < 0:
            _lib.check(n, "coattn_profile_end")
        for i, nm in enumerate(names.value.decode().split("\n")[:n]):
            if nm not in tot:
                tot[nm] = 0.0
                order.append(nm)
            tot[nm] += us[i]
    del pairs
    torch.cuda.empty_cache()
    out = {"order": order, "avg_us": {nm: tot[nm] / iters for nm in order}, "calls": iters, "buffer_sets": nsets}
    _SEQ_CACHE[key] = out
    return out


def backward_legs(device, B=160, N=196, T=26, d=512, L=3, iters=60, layout="lm", bf16=False, fast=False):
    """Every launch group of coattn_backward (frozen image encoder: no dV, the train step's case) inside the forward +
    backward sequence (sequence_marks: the library's own HIP events, rotating buffer sets).  Algorithmic bytes per launch
    (fp32, per (pair, level) unless stated): what each kernel must read and write once --
      bwd_pre    V once per pair (da_v for the three levels) + per level Q read
      bwd_dc32   P_v, P_q, H_q, C read, dA written            (dZ_q is formed from H_q where it is used, never stored)
      bwd_nat32  P_v, P_q, H_q, C read, dP_v, dP_q written
      bwd_dq     V, dA read, dQ read and written; + the weight gradients' split-K partials read and their sums written (the
                 reduction rides in this launch)
      bwd_gemm   MFMA-bound: 2 (B N d^2 + 2 L B T d^2) flops (dW_v, dW_q, dQ = dP_q W_q) against the dense bf16 peak /
                 partial products per fp32 product (6 at the exact split, 3 at the tolerance mode's two-piece width); its HBM
                 bytes beside
    against 8 TB/s."""
    seq = sequence_marks(device, B, N, T, d, L, layout, bf16, fast, iters=iters)
    fwd_marks = ("wsplit", "projections", "coattn_fwd32", "attend_v")
    order = [nm for nm in seq["order"] if nm not in fwd_marks]
    tot = {nm: seq["avg_us"][nm] for nm in order}
    mode = _mode(bf16, fast)
    f4 = 4
    per_level = {
        "bwd_dc32": f4 * (N * d + 2 * T * d + T * N + T * N),
        "bwd_nat32": f4 * (N * d + 2 * T * d + T * N + N * d + T * d),
        "bwd_dq": f4 * (N * d + T * N + 2 * T * d),
    }
    alg = {k: B * L * b for k, b in per_level.items()}
    alg["bwd_pre"] = B * f4 * (N * d + L * T * d)
    if not bf16:                                       # the 32 split-K partials of dW_v, dW_q read, the two sums written
        alg["bwd_dq"] += (32 + 2) * d * d * f4
    # kernels behind a mark (the names rocprofv3 shows): for matching against profiles/*_kernel_stats.csv
    kernels = {"bwd_pre": "bwd_pre_kernel", "bwd_dc32": "bwd_dc32_kernel", "bwd_nat32": "bwd_nat32_kernel",
               "bwd_dq": "bwd_dq32x_kernel" if N <= 64 else "bwd_dq32_kernel",
               "bwd_gemm": "gemm_tn_wide_kernel / gemm_tn_kernel (dW_v + dW_q split-K parts, dQ = dP_q W_q tiles, small reductions)",
               "bwd_gemm_dw": "gemm_tn_wide_kernel / gemm_tn_kernel / gemm_bf_tn_kernel (dW_v + dW_q split-K parts, small reductions)",
               "bwd_gemm_dq_projection": "gemm_h2p_kernel<bf16 pieces> / gemm_w_kernel / gemm_bf_kernel (dQ = dP_q W_q)",
               "reduce_partials": "reduce_partials4_kernel"}
    np_prod = 1 if bf16 else (3 if fast else 6)        # partial products per fp32 product at this arithmetic
    traffic = {}                                       # HBM-side bytes per launch from the committed rocprofv3 PMC passes
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic_backward.json")) as fh:
            for e in json.load(fh)["entries"]:
                if (e.get("shape") == {"B": B, "N": N, "T": T, "d": d, "L": L} and e.get("layout") == layout
                        and e.get("products", "fast16") == mode):
                    traffic = {k: v["hbm_bytes_per_launch"] for k, v in e["kernels"].items()}
    except (OSError, ValueError, KeyError):
        pass
    out = []
    total = sum(tot.values())
    for nm in order:
        t = tot[nm] * 1e-6
        e = {"mark": nm, "kernel": kernels.get(nm, nm), "avg_launch_us": round(t * 1e6, 2), "share": round(t * 1e6 / total, 3)}
        if nm in alg:
            ach = alg[nm] / t / 1e9
            e.update({"bound": "hbm", "algorithmic_bytes": alg[nm], "achieved": round(ach, 1), "peak": HBM_PEAK_GBS,
                      "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": traffic.get(nm)})
        elif nm.startswith("bwd_gemm"):
            fl = {"bwd_gemm": 2.0 * d * d * (B * N + 2 * L * B * T), "bwd_gemm_dw": 2.0 * d * d * (B * N + L * B * T),
                  "bwd_gemm_dq_projection": 2.0 * d * d * L * B * T}[nm]
            peak = 2500.0 / np_prod
            ach = fl / t / 1e12
            hbm = f4 * (L * B * N * d + B * N * d + (3 * L * B * T * d if nm == "bwd_gemm" else 2 * L * B * T * d))
            e.update({"bound": "mfma", "algorithmic_flops": fl, "achieved": round(ach, 1), "peak": round(peak, 1),
                      "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                      "peak_note": "dense bf16 MFMA peak 2500 TFLOP/s / %d partial product(s) per product" % np_prod,
                      "frac_of_fp32_matrix_peak": round(ach / 157.3, 4),
                      "hbm_bytes": hbm, "hbm_frac_at_this_time": round(hbm / t / 1e9 / HBM_PEAK_GBS, 4), "traffic": traffic.get(nm)})
        out.append(e)
    # (round 5: the dQ projection left the weight-gradient launch for a kernel of its own -- the two marks together are what
    #  earlier rounds' lines call bwd_gemm)
    both = [e for e in out if e["mark"] in ("bwd_gemm_dw", "bwd_gemm_dq_projection")]
    if len(both) == 2 and not any(e["mark"] == "bwd_gemm" for e in out):
        t = sum(e["avg_launch_us"] for e in both) * 1e-6
        fl = 2.0 * d * d * (B * N + 2 * L * B * T)
        peak = 2500.0 / np_prod
        out.append({"mark": "bwd_gemm", "kernel": "the two launches above together (dW_v + dW_q, then dQ = dP_q W_q)",
                    "avg_launch_us": round(t * 1e6, 2), "share": round(t * 1e6 / total, 3), "bound": "mfma",
                    "algorithmic_flops": fl, "achieved": round(fl / t / 1e12, 1), "peak": round(peak, 1), "unit": "TFLOP/s",
                    "frac": round(fl / t / 1e12 / peak, 4), "traffic": traffic.get("bwd_gemm"), "sum_of": [e["mark"] for e in both]})
    fwd_us = {nm: round(seq["avg_us"][nm], 2) for nm in seq["order"] if nm in fwd_marks}
    return {"shape": {"B": B, "N": N, "T": T, "d": d, "L": L}, "v_layout": layout, "calls": seq["calls"],
            "products": PRODUCTS[mode], "buffer_sets": seq["buffer_sets"],
            "question_pad_row_fraction": synth_pad_fraction(B, T), "question_pad_rows": PAD_NOTE,
            "total_us": round(total, 1), "kernels": out, "forward_marks_us": fwd_us,
            "fwd_plus_bwd_us": round(total + sum(fwd_us.values()), 1),
            "traffic_source": "profiles/pmc_traffic_backward.json (rocprofv3 PMC passes of tools/probe_hot.py at this shape and in this "
                              "arithmetic, committed; not measured by this run)" if traffic else None,
            "note": "time between HIP events the library records after each launch group, inside coattn_forward + coattn_backward "
                    "pairs rotating over %d buffer sets (coattn_profile_begin / _end); dV not requested (frozen image encoder)"
                    % seq["buffer_sets"]}


def _event_windows(call, iters, n=3):
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3 / iters)
    return ts


def projection_leg(device, B=160, N=196, d=512, iters=50, bf16=False):
    """The dominant MFMA-bound kernel of the path: P_v = V W_v^T + b_v (model.py:380/384, once per sample) from
    location-major features, through coattn_linear_forward -- the weight split once into MFMA-fragment order, then the GEMM
    kernel (the pair coattn_forward launches; the timed region re-uses the weight image, so it is the GEMM kernel alone; the
    split is timed beside it).  Algorithmic flops 2 B N d^2 / average launch time (HIP events on the launch
    stream).  Headline: the fp32-ACCURATE form coattn_forward runs at flags = 0 -- three bf16 pieces per operand, six partial
    products per fp32 product -- against the dense 16-bit MFMA peak / 6 (416.7 TFLOP/s fp32-equivalent); `fast16_f16_pair`: the
    tolerance mode's form (two FP16 pieces, three partial products, COATTN_FLAG_F16PAIR) against peak / 3; the fraction of the
    fp32 matrix peak (157.3 TFLOP/s, a pipe the kernel does not use) is reported too.  Two V buffers are alternated so that
    the A operand of a launch is not the one the previous launch left in the caches."""
    import ctypes as C
    from vqa_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    Vs = [torch.randn(B * N, d, generator=g).to(device) for _ in range(4)]      # 4 x 64 MB at N = 196 (+ 4 outputs): > 256 MiB
    W = (torch.randn(d, d, generator=g) / d ** 0.5).to(device)
    bias = torch.zeros(d, device=device)
    Pvs = [torch.empty(B * N, d, device=device) for _ in range(4)]
    wimg = torch.empty(lib.coattn_linear_workspace_bytes(d, d) // 4, device=device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    state = {"k": 0, "mode": _lib.FLAG_BF16_PROJ if bf16 else 0}

    def call(flags):
        k = state["k"] = (state["k"] + 1) % 4
        return lib.coattn_linear_forward(Vs[k].data_ptr(), d, W.data_ptr(), bias.data_ptr(), Pvs[k].data_ptr(), wimg.data_ptr(),
                                         B * N, d, d, 0.0, flags | state["mode"], stream)

    def check():
        state["k"] = 3
        _lib.check(call(0), "coattn_linear_forward")
        V = Vs[0]
        ref = (V[:256].bfloat16().double() @ W.bfloat16().double().t()) if bf16 else V[:256].double() @ W.double().t()
        if not torch.allclose(Pvs[0][:256].double(), ref, rtol=1e-5, atol=1e-4 if bf16 else 1e-5):
            raise SystemExit("bench.py: projection leg: coattn_linear_forward disagrees with the fp64 product (max error %.3e)"
                             % float((Pvs[0][:256].double() - ref).abs().max()))

    check()
    for _ in range(3 * iters):                     # clock warm-up, as in roofline_leg
        call(1)
    ts = _event_windows(lambda: call(1), iters)
    t = sorted(ts)[1]
    t_with_split = _event_windows(lambda: call(0), iters, 1)[0]
    flop = 2.0 * B * N * d * d
    ach = flop / t / 1e12
    side = None
    if not bf16:                                   # the tolerance mode's form of the same product (two FP16 pieces, three products), beside it
        state["mode"] = _lib.FLAG_F16PAIR
        check()
        for _ in range(iters):
            call(1)
        t3 = sorted(_event_windows(lambda: call(1), iters))[1]
        side = {"avg_launch_us": round(t3 * 1e6, 2), "achieved": round(flop / t3 / 1e12, 1), "peak": round(2500.0 / 3.0, 1),
                "frac": round(flop / t3 / 1e12 / (2500.0 / 3.0), 4),
                "note": "two FP16 pieces per operand, three partial products (COATTN_FLAG_F16PAIR: the tolerance mode's form, gemm_h2p_kernel)"}
    # the bound that applies: dense 16-bit MFMA peak -- divided by the six products per fp32 product of the exact split
    nprod = 1 if bf16 else 6
    peak = 2500.0 / nprod
    return {"bound": "mfma", "achieved": round(ach, 1), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(ach / peak, 4),
            "peak_note": ("dense bf16 MFMA peak (operands rounded to bf16, one MFMA per product, fp32 accumulation)" if bf16 else
                          "fp32-equivalent: dense 16-bit MFMA peak 2500 TFLOP/s / 6 partial products per fp32 product (three bf16 pieces per operand)"),
            "products": PRODUCTS["bf16" if bf16 else "exact"],
            "frac_of_fp32_matrix_peak": round(ach / 157.3, 4), "fast16_f16_pair": side,
            "traffic": None,
            "kernel": ("P_v projection GEMM (gemm_bf_kernel at N % 256 == 0, K % 64 == 0, else gemm_w_kernel's single-piece mode: "
                       "weight pre-rounded into a hi-only fragment image, one MFMA per product)" if bf16 else
                       "P_v projection GEMM (gemm_w_kernel<..., 3 pieces>: weight pre-split into three bf16 pieces, A split while staged)"),
            "shape": {"M": B * N, "N": d, "K": d}, "avg_launch_us": round(t * 1e6, 2),
            "windows_us": [round(x * 1e6, 2) for x in ts], "calls_per_window": iters, "algorithmic_flops": flop,
            "operand_buffers_rotated": 4,
            "bf16_mfma_frac": round(nprod * ach / 2500.0, 4),
            "weight_split_us": round(max(t_with_split - t, 0.0) * 1e6, 2)}


def weight_grad_leg(device, B=160, N=196, d=512, iters=50, bf16=False):
    """The other MFMA-bound kernel of the path: dW_v = dP_v^T V (the weight gradient of the P_v projection, autograd of
    model.py:380/384) through coattn_linear_weight_grad -- split-K parts on gemm_tn_kernel + the deterministic
    reduce, the pair coattn_backward uses (there the launch also carries dW_q, the dQ projection and the small
    reductions).  The timed region is both launches; same warm-up and windows as projection_leg.  Headline: the exact
    three-piece split (six partial products, what coattn_backward runs at flags = 0); `fast16_two_pieces`: the tolerance
    mode's two-bf16-piece width (three products).  Four operand pairs are alternated (cache-cold operands)."""
    import ctypes as C
    from vqa_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(6)
    dPs = [(torch.randn(B * N, d, generator=g) * 0.05).to(device) for _ in range(4)]
    Vs = [torch.randn(B * N, d, generator=g).to(device) for _ in range(4)]
    dW = torch.empty(d, d, device=device)
    ws = torch.empty(lib.coattn_linear_wgrad_workspace_bytes(d, d) // 4, device=device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    state = {"k": 0, "two": False}

    def call():
        k = state["k"] = (state["k"] + 1) % 4
        return lib.coattn_linear_weight_grad(dPs[k].data_ptr(), d, Vs[k].data_ptr(), d, dW.data_ptr(), ws.data_ptr(), B * N, d, d,
                                             _lib.FLAG_BF16_PROJ if bf16 else (_lib.FLAG_SPLIT2 if state["two"] else 0), stream)

    def check(atol):
        state["k"] = 3
        _lib.check(call(), "coattn_linear_weight_grad")
        dP, V = dPs[0], Vs[0]
        ref = (dP[:, :64].bfloat16().double().t() @ V.bfloat16().double()) if bf16 else dP[:, :64].double().t() @ V.double()
        if not torch.allclose(dW[:64].double(), ref, rtol=1e-5, atol=atol):
            raise SystemExit("bench.py: weight-gradient leg: coattn_linear_weight_grad disagrees with the fp64 product")

    def timed():
        for _ in range(3 * iters):
            call()
        ts = _event_windows(call, iters)
        return sorted(ts)[1], ts

    check(1e-3 if bf16 else 1e-4)
    t, ts = timed()
    flop = 2.0 * B * N * d * d
    ach = flop / t / 1e12
    nprod = 1 if bf16 else 6
    peak = 2500.0 / nprod
    side = None
    if not bf16:
        state["two"] = True
        check(3e-4)
        t3, _ = timed()
        side = {"avg_launch_us": round(t3 * 1e6, 2), "achieved": round(flop / t3 / 1e12, 1), "peak": round(2500.0 / 3.0, 1),
                "frac": round(flop / t3 / 1e12 / (2500.0 / 3.0), 4),
                "note": "two bf16 pieces per operand, three partial products (the tolerance mode's width of coattn_backward)"}
    return {"bound": "mfma", "achieved": round(ach, 1), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(ach / peak, 4),
            "peak_note": ("dense bf16 MFMA peak (operands rounded to bf16, one MFMA per product)" if bf16 else
                          "fp32-equivalent: dense bf16 MFMA peak 2500 TFLOP/s / 6 partial products per fp32 product (exact three-piece "
                          "split, as coattn_backward runs it at flags = 0)"),
            "products": PRODUCTS["bf16" if bf16 else "exact"],
            "frac_of_fp32_matrix_peak": round(ach / 157.3, 4), "bf16_mfma_frac": round(nprod * ach / 2500.0, 4),
            "fast16_two_pieces": side, "traffic": None,
            "kernel": ("dW_v weight-gradient GEMM (gemm_bf_tn_kernel at 256-multiples, else gemm_tn_kernel's single-piece mode; one round "
                       "of split-K parts) + reduce_partials4_kernel" if bf16 else
                       "dW_v weight-gradient GEMM (gemm_tn_kernel, 32 split-K parts) + reduce_partials4_kernel"),
            "shape": {"M": d, "N": d, "K": B * N}, "avg_launch_us": round(t * 1e6, 2),
            "windows_us": [round(x * 1e6, 2) for x in ts], "calls_per_window": iters, "algorithmic_flops": flop,
            "operand_buffers_rotated": 4}


def host_cores() -> int:
    """CPUs this process may actually use: affinity mask capped by the cgroup CPU quota."""
    from vqa_amd.train import usable_cpus
    return usable_cpus()


def cpu_model_string() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


CPU_WARM, CPU_TIMED = 3, 5          # >= 3 warm-up + >= 5 timed steps on the CPU


def cpu_baseline_leg(args):
    """The oracle port of the same train step on the host cores; bounded sample (BASELINE.md section 3 protocol:
    3 warm-up + 5 timed steps, median)."""
    from oracle import net_oracle as NO
    from vqa_amd import train as T
    cores = host_cores()
    torch.set_num_threads(cores)
    torch.manual_seed(0)
    qp = dict(vocab_size=args.vocab, word_emb_dim=512, hidden_dim=512)
    net = NO.OracleHierarchicalCoAttentionNet(qp, dict(is_trainable=False, weights_path=None), K=args.num_cls + 1)
    cpu_batch = args.cpu_batch or args.batch             # the same inputs as the GPU step
    b = T.synthetic_batch(cpu_batch, (args.image_size,) * 2, args.seq_len, args.vocab, args.num_cls + 1, seed=1234)
    image, question, label, lens = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
    batch = (image, question, lens, label)
    NO.train_steps(net, [batch] * CPU_WARM, lr=1e-4)
    ts = []
    for _ in range(CPU_TIMED):
        t0 = time.perf_counter()
        NO.train_steps(net, [batch], lr=1e-4)
        ts.append(time.perf_counter() - t0)
    dt = sorted(ts)[len(ts) // 2]
    return {"value": round(cpu_batch / dt, 2), "unit": "QA-pairs/s", "cores": cores, "kind": "port", "batch": cpu_batch,
            "cpu": cpu_model_string(),
            "sample": "oracle port of the same train step (reference op sequence incl. its 6x W_v(V) "
                      "re-evaluation), batch %d, %dx%d images, %d warm-up + %d timed steps (median), torch CPU fp32, "
                      "%d threads" % (cpu_batch, args.image_size, args.image_size, CPU_WARM, CPU_TIMED, cores)}


def cpu_hot_path_leg(N, B=160, T=26, d=512, K=1000):
    """The isolated hot path (co-attention + MLPClassifier + CE, forward + backward) of the
    oracle port on the host cores, on the same synthetic features as `hot_path_leg`."""
    from oracle import coattn_oracle as O
    cores = host_cores()
    torch.set_num_threads(cores)
    torch.manual_seed(0)
    co = O.OracleParallelCoAttention(d, as_executed=True)
    mlp = O.OracleMLPClassifier(d, 1024, K + 1)
    V, Qs = synth_features(B, N, T, d, torch.device("cpu"))
    x_img = V.permute(0, 2, 1)                       # the encoder's permuted view (model.py:215-217)
    Qs = [q.requires_grad_(True) for q in Qs]
    label = (torch.arange(B) * 7) % (K + 1)
    crit = torch.nn.CrossEntropyLoss()
    params = list(co.parameters()) + list(mlp.parameters())

    def step():
        for p in params:
            p.grad = None
        crit(mlp(*co(x_img, Qs)), label).backward()

    for _ in range(CPU_WARM):
        step()
    ts = []
    for _ in range(CPU_TIMED):
        t0 = time.perf_counter()
        step()
        ts.append(time.perf_counter() - t0)
    dt = sorted(ts)[len(ts) // 2]
    return {"N": N, "value": round(B / dt, 1), "unit": "QA-pairs/s", "ms_per_step": round(dt * 1e3, 1), "cores": cores,
            "kind": "port", "cpu": cpu_model_string(),
            "sample": "oracle port of co-attention + MLPClassifier + CE, fwd+bwd, B=%d N=%d T=%d d=%d, %d warm-up + %d "
                      "timed (median), torch CPU fp32, %d threads" % (B, N, T, d, CPU_WARM, CPU_TIMED, cores)}


def config_leg(T, args, device, model_name, opt_lvl, num_cls, steps=10, warmup=3):
    """BASELINE configs 4 and 5 on the driver's own command: the same train step protocol as the headline --
    resident synthetic batch, encoder one step ahead, PRIME_STEPS + `warmup` untimed steps, then exactly `steps` timed ones
    between two synchronisations -- for another model of the registry, reported as a compact object."""
    import gc
    a = argparse.Namespace(**vars(args))
    a.model, a.opt_lvl, a.num_cls = model_name, opt_lvl, num_cls
    if model_name == "attention_bert":
        a.vocab = T.BERT_VOCAB
    torch.manual_seed(0)
    model = T.build_model(model_name, a.vocab, num_cls).to(device)
    if args.channels_last:
        model.image_encoder.to(memory_format=torch.channels_last)
    trainer = T.Trainer(model, 1e-4, device, opt_lvl=opt_lvl, encoder_runahead=args.runahead, precision=args.precision)
    batch = device_batch(T, a, 0, device)
    if args.channels_last:
        batch = (batch[0].contiguous(memory_format=torch.channels_last),) + batch[1:]
    dt, _ = timed_steps(trainer, batch, steps, warmup, torch.cuda.synchronize)
    d = model.co_attention.hidden_dim
    n_grid = (args.image_size // 32) ** 2
    out = {"model": model_name, "value": round(args.batch * steps / dt, 2), "unit": "QA-pairs/s", "ms_per_step": round(dt / steps * 1e3, 3),
           "steps": steps, "warmup": warmup, "dtype": "f32" if opt_lvl == 0 else "bf16",
           "precision": "bf16" if opt_lvl > 0 else trainer.precision, "batch": args.batch, "K": num_cls,
           "grid": "%d locations x %d channels" % (n_grid, d)}
    del trainer, model, batch
    gc.collect()
    torch.cuda.empty_cache()
    return out


def preflight(rank, world, device):
    """N > 1, before anything is timed (nothing about the first multi-GPU run may end in a hang): enough visible
    GPUs, every rank on its own physical GPU (distinct UUIDs), and ONE 1-element all-reduce that must complete within 60 s.
    Any failure is a message on stderr and a hard non-zero exit of this rank (the launcher then stops the others)."""
    import datetime
    import torch.distributed as dist

    def fail(code, msg):
        print("bench.py preflight (rank %d): %s" % (rank, msg), file=sys.stderr, flush=True)
        os._exit(code)                               # (not sys.exit: a wedged communicator thread must not keep the process)

    over = os.environ.get("VQA_BENCH_OVERSUBSCRIBE") == "1"      # rehearsal: ranks share devices (use with VQA_DIST_BACKEND=gloo)
    n_dev = torch.cuda.device_count()
    if n_dev < world and not over:
        fail(12, "--gpus %d needs %d visible GPUs, found %d" % (world, world, n_dev))
    props = torch.cuda.get_device_properties(device)
    every = [None] * world
    try:
        dist.all_gather_object(every, str(getattr(props, "uuid", "unknown-%d" % device.index)))
    except Exception as e:                           # noqa: BLE001
        fail(13, "all_gather_object failed: %s" % e)
    if len(set(every)) != world and not over:
        fail(14, "ranks share a physical GPU: UUIDs %s" % every)
    t = torch.ones(1, device=device)
    try:
        work = dist.all_reduce(t, async_op=True)
        t0 = time.time()
        while not work.is_completed():
            if time.time() - t0 > 60.0:
                fail(15, "a 1-element all-reduce over %d ranks (%s) did not complete within 60 s" % (world, dist.get_backend()))
            time.sleep(0.01)
        work.wait(timeout=datetime.timedelta(seconds=60))
        torch.cuda.synchronize(device)
    except Exception as e:                           # noqa: BLE001
        fail(16, "1-element all-reduce failed: %s" % e)
    if float(t) != float(world):
        fail(17, "1-element all-reduce returned %s, expected %d" % (float(t), world))
    return {"ranks": world, "distinct_gpus": len(set(every)), "allreduce_probe_s": round(time.time() - t0, 3)}


def expected_exchange_ms(payload_bytes, n_buckets, world):
    """What the gradient exchange should cost on one xGMI node, from DESIGN.md section 6's arithmetic, so that the first
    real multi-GPU run is judged against a prediction.  xGMI: 7 links per GPU, ~77 GB/s per link and direction
    achievable (153 GB/s bidirectional spec).  A ring all-reduce moves 2 (w-1)/w S past every GPU over ONE link direction in
    2 (w-1) dependent steps per bucket; the one-shot pattern sends S/w to each of w-1 peers over separate links, twice."""
    S, w = float(payload_bytes), world
    link = 77e9
    ring = 2.0 * (w - 1) / w * S / link + n_buckets * 2 * (w - 1) * 8e-6          # + ~8 us per dependent ring step
    one_shot = 2.0 * (S / w) / link + n_buckets * 3 * 15e-6                       # every peer link at once; 3 phase boundaries
    return {"ring_one_link_ms": round(ring * 1e3, 3), "one_shot_all_links_ms": round(one_shot * 1e3, 3),
            "exposed_ms_predicted": "0 to %.2f: the exchange is queued behind the hot path's backward (~0.25 ms) on the main "
                                    "stream while the NEXT step's frozen-encoder pass (~24 ms) runs on its own stream; it is exposed "
                                    "only as far as RCCL's kernels take CUs from the convolutions" % (ring * 1e3),
            "scaling_predicted": "weak scaling >= %.2f of linear at %d GPUs (ring fully exposed: %.2f ms of a ~25.4 ms step)"
                                 % (25.4 / (25.4 + ring * 1e3), w, ring * 1e3),
            "assumptions": "xGMI 77 GB/s per link and direction; payload %.1f MB in %d buckets" % (S / 1e6, n_buckets)}


def self_launch(args) -> int:
    """`python bench.py --gpus N` from a plain shell: start the N ranks here (one process per GPU, RANK / WORLD_SIZE /
    LOCAL_RANK / MASTER_* set before anything touches a GPU -- this parent never does), relay rank 0's JSON line and
    return non-zero if any rank failed."""
    import socket
    import subprocess
    n_dev = torch.cuda.device_count()                # does not initialise the GPU
    if n_dev < args.gpus and os.environ.get("VQA_BENCH_OVERSUBSCRIBE") != "1":   # (=1: rehearsal, ranks share devices; use with VQA_DIST_BACKEND=gloo)
        print("bench.py: --gpus %d needs %d visible GPUs, found %d" % (args.gpus, args.gpus, n_dev), file=sys.stderr)
        return 2
    def start(port):
        procs = []
        for r in range(args.gpus):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_RANK=str(r), LOCAL_WORLD_SIZE=str(args.gpus),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
        return procs

    for attempt in range(3):                         # (the free port is found by bind-and-close: another process may take it first)
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        procs = start(port)
        # poll ALL ranks: if one dies at start-up the others would sit in the rendezvous until its timeout
        import threading
        out0 = []
        reader = threading.Thread(target=lambda: out0.append(procs[0].stdout.read()), daemon=True)
        reader.start()
        t0 = time.time()
        failed = None
        while any(p.poll() is None for p in procs):
            bad = [(r, p.returncode) for r, p in enumerate(procs) if p.poll() not in (None, 0)]
            if bad:
                failed = bad
                for p in procs:
                    if p.poll() is None:
                        p.terminate()
                break
            time.sleep(0.2)
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill()
        reader.join(timeout=10)
        rcs = [p.returncode for p in procs]
        if failed and time.time() - t0 < 60 and attempt < 2:
            print("bench.py: ranks failed at start-up %s; retrying on another port" % failed, file=sys.stderr)
            continue
        break
    sys.stdout.write(out0[0] if out0 else "")
    sys.stdout.flush()
    bad = [(r, rc) for r, rc in enumerate(rcs) if rc != 0]
    if bad:
        print("bench.py: ranks failed (rank, exit code): %s" % bad, file=sys.stderr)
        return 1
    return 0


def main():
    args = parse()
    seed_miopen_db()
    if args.gpus > 1 and "RANK" not in os.environ:       # not under torch.distributed.run: launch the ranks ourselves
        sys.exit(self_launch(args))
    if args.stock_graph:
        os.environ["VQA_ENCODER_REWRITE"] = "0"
    import vqa_amd
    from vqa_amd import dist as vdist
    from vqa_amd import train as T
    if args.only:
        dev = torch.device("cuda", 0)
        n_step = (args.image_size // 32) ** 2
        if args.model == "attention_resnet":             # config 4's shapes
            bf = args.opt_lvl > 0
            res = ({"roofline": roofline_leg(dev, B=args.batch, N=n_step, T=args.seq_len, d=2048, bf16=bf),
                    "roofline_projection": projection_leg(dev, B=args.batch, N=n_step, d=2048, bf16=bf),
                    "roofline_weight_grad": weight_grad_leg(dev, B=args.batch, N=n_step, d=2048, bf16=bf),
                    "roofline_backward": [backward_legs(dev, B=args.batch, N=n_step, T=args.seq_len, d=2048, bf16=bf)]}
                   if args.only == "roofline"
                   else [hot_path_leg(dev, n_step, lay, B=args.batch, T=args.seq_len, d=2048, K=args.num_cls, bf16=bf)
                         for lay in ("lm", "cm")])
        else:
            fast = args.precision == "fast"
            res = ({"roofline": roofline_leg(dev, N=49, fast=fast), "roofline_reference_grid": roofline_leg(dev, fast=fast),
                    "roofline_channel_major": roofline_leg(dev, layout="cm", fast=fast),
                    "roofline_projection": projection_leg(dev), "roofline_weight_grad": weight_grad_leg(dev),
                    "roofline_backward": [backward_legs(dev, N=49, fast=fast), backward_legs(dev, fast=fast)]}
                   if args.only == "roofline"
                   else [hot_path_leg(dev, n, lay) for n in (196, 49) for lay in ("lm", "cm")])
        print(json.dumps(res))
        return
    torch.set_num_threads(max(1, min(4, host_cores())))   # the step is GPU work; do not oversubscribe host cores per rank
    rank, world, local = vdist.init_from_env()
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    device = torch.device("cuda", local % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(device)
    pre = preflight(rank, world, device) if world > 1 else None
    torch.manual_seed(0)
    if args.model == "attention_bert":               # token ids are BERT's own WordPiece ids
        args.vocab = T.BERT_VOCAB
    model = T.build_model(args.model, args.vocab, args.num_cls).to(device)
    if args.channels_last:
        model.image_encoder.to(memory_format=torch.channels_last)
    trainer = T.Trainer(model, 1e-4, device, opt_lvl=args.opt_lvl, encoder_runahead=args.runahead, precision=args.precision)
    batch = device_batch(T, args, rank, device)
    if args.channels_last:
        batch = (batch[0].contiguous(memory_format=torch.channels_last),) + batch[1:]

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
            torch.cuda.synchronize()

    dt, loss = timed_steps(trainer, batch, args.steps, args.warmup, sync)
    if world > 1:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, loss)
    out = None
    if rank == 0:
        value = world * args.batch * args.steps / dt
        n_grid = (args.image_size // 32) ** 2
        out = {
            "metric": "QA-pairs/sec (train step, attention model, K=%d)" % args.num_cls, "value": round(value, 2),
            "unit": "QA-pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if args.opt_lvl > 0 else ("f32" if args.precision == "exact" else "f32 storage, 22/16-bit products (tolerance mode)"),
            "data": "synthetic",
            "config": {"workload": "attention model train step (fwd + CE + bwd + Adam%s), K=%d (+1 UNKNOWN), "
                                   "batch %d/GPU, %dx%d synthetic images -> %d-location x %d grid, %d-token questions, "
                                   "vocab %d, %s, frozen random-init %s (%s%s)"
                                   % (" + RCCL grad all-reduce" if world > 1 else "", args.num_cls, args.batch,
                                      args.image_size, args.image_size, n_grid, model.co_attention.hidden_dim,
                                      args.seq_len, args.vocab,
                                      "fp32" if args.opt_lvl == 0 else "bf16 autocast",
                                      {"attention": "VGG11-bn", "attention_resnet": "ResNet-152 (hidden 2048)",
                                       "attention_bert": "VGG11-bn; word level = Linear(768 -> 512) over frozen random-init "
                                                         "BERT-base token embeddings (BertEmbeddings, vocab 30,522) in place of the "
                                                         "learned embedding (BASELINE config 5)"}[args.model],
                                      "channels_last" if args.channels_last else "NCHW",
                                      (", encoder one step ahead on its own stream" if trainer.runahead else "")
                                      + ("" if args.stock_graph else ", ReLU after MaxPool, conv bias folded into BN running mean")),
                       "precision": "bf16" if args.opt_lvl > 0 else args.precision,
                       "question_pad_row_fraction": round(1.0 - float(batch[2].sum()) / (args.batch * args.seq_len), 4),
                       "question_pad_rows": PAD_NOTE,
                       "arithmetic": (ARITHMETIC if (args.opt_lvl == 0 and args.precision == "exact") else
                                      "fp32 storage and accumulation; --precision fast, the opt-in tolerance mode (COATTN_FLAG_FAST16): "
                                      "forward-side products on 2 x fp16 pieces per operand = 22 significand bits, backward products on "
                                      "2 x bf16 pieces = 16 bits (3 partial products each) -- NARROWER than the reference's fp32; answer "
                                      "head: exact fp32 MFMA; stock encoders: fp32" if args.opt_lvl == 0 else
                                      "reduced-precision mode (COATTN_FLAG_BF16_PROJ): every operand of every product of the HIP path "
                                      "rounded to bf16 (8 significant bits), ONE MFMA per product, fp32 accumulation and storage; stock "
                                      "encoders under bf16 autocast"),
                       "untimed_prime_steps": PRIME_STEPS,
                       "global_batch": world * args.batch, "parallelism": "dp%d" % world,
                       "gpu": "%s uuid %s" % (torch.cuda.get_device_properties(device).name,
                                              getattr(torch.cuda.get_device_properties(device), "uuid", "unknown")),
                       "coattn_impl": "fused" if vqa_amd._lib.load().coattn_fused_supported(
                           args.batch, n_grid, args.seq_len, model.co_attention.hidden_dim, 3, 0) else "general"},
        }
    if args.full and world == 1 and args.opt_lvl == 0 and args.precision == "exact" and not args.no_extras:
        # side key: the same step in the opt-in tolerance mode (a shorter window; the headline above is the exact mode)
        trainer.set_precision("fast")
        f_steps = max(5, args.steps // 2)
        dt_f, _ = timed_steps(trainer, batch, f_steps, 2, sync)
        ok = trainer.check_range()                           # (sticky range report over every one of those steps)
        trainer.set_precision("exact")
        out["value_fast16"] = {"value": round(args.batch * f_steps / dt_f, 2), "ms_per_step": round(dt_f / f_steps * 1e3, 3),
                               "steps": f_steps, "precision": "fast", "range_ok": bool(ok),
                               "note": "opt-in tolerance mode (22-bit forward / 16-bit backward products); NOT the headline"}
    if args.full and world > 1 and trainer.reducer is not None:
        # the exchange step, measurable: the same step under RCCL's all-reduce (the timed run above), under the
        # one-shot all-to-all / sum / all-gather pattern, and with no collective at all (compute-only: local
        # gradients, timing only) -- fewer steps each; exposed time = step time minus the compute-only step time
        ex_steps = max(4, args.steps // 2)
        ex = {"allreduce": dt / args.steps * 1e3}
        errors = {}
        # (the peer-mapped one-shot exchange, exchange="p2p", is timed only on request: it has run with ranks sharing ONE
        #  GPU only, and a first run between GPUs belongs in a session of its own, not in the scaling measurement)
        p2p = args.exchange_p2p or os.environ.get("VQA_BENCH_P2P", "0") == "1"
        for mode in ("direct",) + (("p2p",) if p2p else ()) + ("none",):
            try:
                trainer.reducer.reset(mode)
                t_m, _ = timed_steps(trainer, batch, ex_steps, 2, sync)
                tt = torch.tensor([t_m], device=device, dtype=torch.float64)
                torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
                ex[mode] = float(tt) / ex_steps * 1e3
            except RuntimeError as e:                    # (a backend without this collective: the leg is reported as failed)
                errors[mode] = str(e).splitlines()[0][:200]
                ex[mode] = None
        if rank == 0:
            diff = lambda a, b: round(a - b, 3) if a is not None and b is not None else None   # noqa: E731
            out["exchange"] = {"ms_per_step": {k: (round(v, 3) if v is not None else None) for k, v in ex.items()},
                               "errors": errors or None,
                               "allreduce_ms_exposed": diff(ex["allreduce"], ex["none"]),
                               "direct_ms_exposed": diff(ex["direct"], ex["none"]),
                               "p2p_ms_exposed": diff(ex["p2p"], ex["none"]) if p2p else "not run (opt-in: --exchange-p2p)",
                               "steps_per_leg": dict({"allreduce": args.steps, "direct": ex_steps, "none": ex_steps}, **({"p2p": ex_steps} if p2p else {})),
                               "expected_ms": expected_exchange_ms(trainer.reducer.payload_bytes() or 48.7e6,
                                                                   len(trainer.reducer.buckets or []) or 3, world),
                               "preflight": pre,
                               "world_size": torch.distributed.get_world_size(),
                               "backend": torch.distributed.get_backend(),
                               "note": "headline value = the allreduce run; 'none' keeps gradients local (timing only)"}
    if world > 1:
        # self-verifying scaling line: what the communicator itself reports, and which physical GPU every rank ran on
        # (N distinct UUIDs = N GPUs; ranks sharing a device would show here)
        props = torch.cuda.get_device_properties(device)
        mine = {"rank": rank, "local_device": device.index, "gpu": props.name, "uuid": str(getattr(props, "uuid", "unknown")),
                "host": os.uname().nodename}
        every = [None] * world
        torch.distributed.all_gather_object(every, mine)
        if rank == 0:
            out["rccl_world_size"] = torch.distributed.get_world_size()
            out["dist_backend"] = torch.distributed.get_backend()
            out["ranks"] = every
            out["distinct_gpus"] = len({e["uuid"] for e in every})
            if trainer.reducer is not None:
                out["allreduce_payload_mb"] = round(trainer.reducer.payload_bytes() / 1e6, 2)
                out["allreduce_buckets"] = len(trainer.reducer.buckets or [])
                out["grad_exchange_fallback"] = trainer.reducer.fallback_reason
        vdist.shutdown()
    if args.full and rank == 0 and not args.no_extras:
        del trainer, model, batch
        torch.cuda.empty_cache()
        n_step = (args.image_size // 32) ** 2
        if args.model == "attention_resnet":
            # BASELINE config 4: 7x7x2048 grid, reduced precision (operands of the projections rounded to bf16, one MFMA
            # per product); every leg at that shape
            d4, bf = 2048, args.opt_lvl > 0
            out["roofline"] = roofline_leg(device, B=args.batch, N=n_step, T=args.seq_len, d=d4, bf16=bf)
            out["roofline_projection"] = projection_leg(device, B=args.batch, N=n_step, d=d4, bf16=bf)
            out["roofline_weight_grad"] = weight_grad_leg(device, B=args.batch, N=n_step, d=d4, bf16=bf)
            out["roofline_backward"] = [backward_legs(device, B=args.batch, N=n_step, T=args.seq_len, d=d4, bf16=bf)]
            if world == 1:
                out["hot_path"] = [hot_path_leg(device, n_step, lay, B=args.batch, T=args.seq_len, d=d4, K=args.num_cls, bf16=bf)
                                   for lay in ("lm", "cm")]
        else:
            # per-GPU kernel, the same on every rank; image features location-major [B,N,d], as the channels_last
            # encoder of the timed step hands them over (no copy in between)
            # THE roofline object: the dominant kernel at the shape the timed step runs it at (224x224 -> 7x7 = 49 locations), in
            # the timed step's arithmetic (fp32-accurate products unless --precision fast), launches rotating over buffer sets
            fast = args.precision == "fast"
            out["roofline"] = roofline_leg(device, B=args.batch, N=n_step, T=args.seq_len, fast=fast)
            # the same kernel at the reference's default grid (448x448 -> 14x14 = 196 locations: SURVEY 8d's per-unit figure)
            out["roofline_reference_grid"] = roofline_leg(device, fast=fast)
            # ... and on the reference's own layout (NCHW encoder -> channel-major [B,d,N] behind a permuted view)
            out["roofline_channel_major"] = roofline_leg(device, layout="cm", fast=fast)
            out["roofline_projection"] = projection_leg(device)
            out["roofline_weight_grad"] = weight_grad_leg(device)
            out["roofline_backward"] = [backward_legs(device, B=args.batch, N=n_step, T=args.seq_len, fast=fast),
                                        backward_legs(device, fast=fast)]
            if not fast:
                # side keys: the opt-in tolerance mode (what rounds 2-5 put on the headline)
                out["roofline_fast16"] = roofline_leg(device, B=args.batch, N=n_step, T=args.seq_len, fast=True)
                out["roofline_reference_grid_fast16"] = roofline_leg(device, fast=True)
                out["roofline_backward_fast16"] = [backward_legs(device, B=args.batch, N=n_step, T=args.seq_len, fast=True),
                                                   backward_legs(device, fast=True)]
            if world == 1:
                out["hot_path"] = [hot_path_leg(device, n, lay) for n in (196, 49) for lay in ("lm", "cm")]
    if (args.full and rank == 0 and world == 1 and not args.no_extras and args.model == "attention" and args.opt_lvl == 0
            and not args.no_configs):
        # BASELINE configs 4 and 5 as compact objects on the same line (each ~10 timed steps of its own model; their full
        # lines: `bench.py --full --model attention_resnet --opt-lvl 1 --num-cls 3000`, `bench.py --full --model attention_bert`)
        t_cfg = time.time()
        try:
            c4 = config_leg(T, args, device, "attention_resnet", 1, 3000)
            n4 = (args.image_size // 32) ** 2
            r = roofline_leg(device, B=args.batch, N=n4, T=args.seq_len, d=2048, iters=40, bf16=True)
            pj = projection_leg(device, B=args.batch, N=n4, d=2048, bf16=True, iters=30)
            wg = weight_grad_leg(device, B=args.batch, N=n4, d=2048, bf16=True, iters=30)
            hp4 = hot_path_leg(device, n4, "lm", B=args.batch, T=args.seq_len, d=2048, K=3000, bf16=True, iters=10)
            c4.update({"config": "BASELINE configs[3]: ResNet-152 7x7x2048 features, bf16 (reduced-precision mode), K=3000",
                       "roofline": {k: r[k] for k in ("bound", "achieved", "peak", "unit", "frac", "avg_launch_us")},
                       "roofline_projection": {k: pj[k] for k in ("bound", "achieved", "peak", "unit", "frac", "avg_launch_us")},
                       "roofline_weight_grad": {k: wg[k] for k in ("bound", "achieved", "peak", "unit", "frac", "avg_launch_us")},
                       "hot_path": {k: hp4[k] for k in ("ms_per_step", "pairs_per_s", "coattn_fwd_bwd_ms", "host_enqueue_ms")}})
            out["config4"] = c4
        except Exception as e:                                 # noqa: BLE001 -- the headline line must still come out
            out["config4"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
        try:
            c5 = config_leg(T, args, device, "attention_bert", 0, args.num_cls)
            c5["config"] = ("BASELINE configs[4] on ONE GPU (its 4-GPU run is `bench.py --model attention_bert --gpus 4`): word level = "
                            "Linear(768 -> 512) over frozen random-init BERT-base token embeddings; the co-attention kernels and their "
                            "roofline legs are config 2's (same shapes)")
            out["config5"] = c5
        except Exception as e:                                 # noqa: BLE001
            out["config5"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
        out["configs_4_5_seconds"] = round(time.time() - t_cfg, 1)
    if rank == 0:
        if args.full and world == 1 and not args.no_cpu_baseline and args.model == "attention":   # (the oracle port has no ResNet encoder)
            out["cpu_baseline"] = cpu_baseline_leg(args)
            out["cpu_baseline_hot_path"] = [cpu_hot_path_leg(196), cpu_hot_path_leg(49)]
        print(json.dumps(out))


if __name__ == "__main__":
    main()

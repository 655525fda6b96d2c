"""Developer probe of the eval-mode encoder passes (include/coattn_ext.h v0.24.0; --encoder_eval hip).

  formula  which arithmetic the stock eval-mode BatchNorm runs: coattn_bn_eval_probe's candidates (rsqrt 0 .. 3 x fma or multiply +
           add x eps rounded before or after the add) against F.batch_norm on channels_last operands that tell them apart --
           ordinary, zero, negative and huge variances, var + eps subnormal (eps 1e-40) -- and, per VGG convolution shape,
           whether conv2d(x, w, b) is conv2d(x, w, None) + b in every bit.
  forward  one process, the frozen VGG11-bn in eval mode at B = 160, 224 and 448 px (SIZES), eval_impl "stock" and "hip" alternating
           window by window after a warm-up window each (which also runs the per-shape comparison): the median of WINDOWS windows of
           ITERS forwards, timed by HIP events, and the spread of the windows -- tools/probe_cached_features.py's protocol.  On
           the default solvers, the benchmark's (the convolution keeps its bias; the one-launch first group verifies);
           DETERMINISTIC=1 runs the deterministic ones (extract.py's: the bias moves into the kernel, the first convolution stays
           stock), where one forward at 224 px takes 4.7 s: set SIZES=224 and a long time limit.
  layers   the eight groups of that forward one by one, the stock chain against the route, each on its own input.
  e2e      extract.py and predict.py end to end on synthetic data at 64 px, once each way: wall seconds and equal files.

One JSON line per measurement; OUT appends them to a file (profiles/encoder_eval_probe.jsonl).  WHAT selects the parts
("formula,forward,layers,e2e").  Kernel statistics come from a run of their own:
`rocprofv3 --kernel-trace --stats -- python3 tools/probe_encoder_eval.py` with WHAT=forward ITERS=2 WINDOWS=2 SIZES=224."""
import itertools
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

bench.seed_miopen_db()                                          # MIOpen's find records, as bench.py seeds them
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import vqa_amd  # noqa: E402
from vqa_amd import _lib, encoder  # noqa: E402
from vqa_amd.modules import run_conv_bn_stack, vgg11_bn_features  # noqa: E402

B = int(os.environ.get("B", "160"))
ITERS = int(os.environ.get("ITERS", "5"))
WINDOWS = int(os.environ.get("WINDOWS", "7"))
SIZES = [int(s) for s in os.environ.get("SIZES", "224,448").split(",")]
WHAT = os.environ.get("WHAT", "formula,forward,layers,e2e").split(",")
DEV = torch.device("cuda:0")


def emit(line):
    line = dict(line, version=vqa_amd._lib.load().coattn_version(), device=torch.cuda.get_device_name(DEV))
    print(json.dumps(line), flush=True)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "a") as fh:
            fh.write(json.dumps(line) + "\n")


def timed(fn, iters):
    st = torch.cuda.current_stream(DEV)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(iters):
        fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(variants, iters):
    names = list(variants)
    for n in names:
        timed(variants[n], max(2, iters))                        # warm-up; the first "hip" call is the comparison
    t = {n: [] for n in names}
    for w in range(WINDOWS):
        k = w % len(names)
        for n in names[k:] + names[:k]:
            t[n].append(timed(variants[n], iters))
    out = {}
    for n, v in t.items():
        med = statistics.median(v)
        out[n + "_ms"], out[n + "_spread"] = round(med, 4), round((max(v) - min(v)) / med, 4)
        out[n + "_windows_ms"] = [round(x, 4) for x in v]
    return out


def equal(a, b):
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def formula():
    g = torch.Generator().manual_seed(1)
    Bs, H, W, C = 2, 5, 7, 64
    x = (torch.randn(Bs, C, H, W, generator=g) * torch.logspace(-3, 3, C).view(1, C, 1, 1)).to(DEV).contiguous(memory_format=torch.channels_last)
    gamma, beta, rm = (torch.randn(C, generator=g).to(DEV) for _ in range(3))
    rv = torch.rand(C, generator=g) * 4 + 0.01
    rv[:8] = torch.tensor([0.0, -0.5, 1e30, 1e-41, -1e-5, 3e-39, 1e-30, 1e-35])
    rv = rv.to(DEV)
    for eps in (1e-5, 1e-3, 1e-40):
        ref = F.batch_norm(x, rm, rv, gamma, beta, False, 0.0, eps)
        match = []
        for r, s, e in itertools.product(range(4), range(2), range(2)):
            y = torch.empty_like(x)
            _lib.bind("coattn_bn_eval_probe", x=x, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, eps=eps, y=y, B=Bs, H=H,
                      W=W, C=C, rsqrt=r, step=s, eps_mode=e, stream=_lib.stream_ptr(DEV))()
            if equal(y, ref):
                match.append({"rsqrt": r, "step": s, "eps_mode": e})
        mine = encoder._bn_eval_raw(x, None, gamma, beta, rm, rv, eps, False, relu=False)
        emit({"what": "formula", "eps": eps, "candidates_equal_to_stock": match, "coattn_bn_eval_forward_equal": equal(mine, ref)})
    for det in (True, False):
        torch.backends.cudnn.deterministic = det
        for cin, cout, hw in ((3, 64, 224), (64, 128, 112), (128, 256, 56), (256, 256, 56), (256, 512, 28), (512, 512, 28), (512, 512, 14)):
            conv = torch.nn.Conv2d(cin, cout, 3, padding=1).to(DEV).to(memory_format=torch.channels_last)
            xi = torch.randn(8, cin, hw, hw, device=DEV).contiguous(memory_format=torch.channels_last)
            with torch.no_grad():
                a, b = conv(xi), F.conv2d(xi, conv.weight, None, 1, 1) + conv.bias.view(1, -1, 1, 1)
            emit({"what": "bias", "deterministic": det, "Cin": cin, "Cout": cout, "HW": hw, "B": 8, "conv_with_bias_is_conv_plus_bias": equal(a, b)})


def frozen_vgg():
    torch.manual_seed(0)
    seq = vgg11_bn_features()
    for m in seq:
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.3), m.running_var.uniform_(0.5, 1.5)
    return seq.to(DEV).to(memory_format=torch.channels_last).requires_grad_(False).eval()


def forward_and_layers():
    torch.backends.cudnn.deterministic = os.environ.get("DETERMINISTIC", "0") == "1"
    seq = frozen_vgg()
    for size in SIZES:
        g = torch.Generator(device=DEV).manual_seed(size)
        img = torch.randn((B, 3, size, size), device=DEV, generator=g).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            if "forward" in WHAT:
                line = alternate({"stock": lambda: run_conv_bn_stack(seq, img), "hip": lambda: run_conv_bn_stack(seq, img, "hip")}, ITERS)
                same = equal(run_conv_bn_stack(seq, img), run_conv_bn_stack(seq, img, "hip"))
                report = {str(k): v for k, v in encoder.eval_report().items() if k[1] == B}
                emit(dict(line, what="forward", B=B, image_size=size, iters=ITERS, windows=WINDOWS, equal_bits=same,
                          deterministic=torch.backends.cudnn.deterministic, hip_over_stock=round(line["hip_ms"] / line["stock_ms"], 4),
                          verified=all(v["verified"] for v in report.values()), report=report))
            if "layers" in WHAT:
                mods, x, i = list(seq), img, 0
                while i < len(mods):
                    n = 4 if i + 3 < len(mods) and isinstance(mods[i + 3], torch.nn.MaxPool2d) else 3
                    group = torch.nn.Sequential(*mods[i:i + n])
                    xin = x
                    line = alternate({"stock": lambda: run_conv_bn_stack(group, xin), "hip": lambda: run_conv_bn_stack(group, xin, "hip"),
                                      "conv_alone": lambda: group[0](xin)}, ITERS)
                    x = run_conv_bn_stack(group, xin)
                    emit(dict(line, what="layer", B=B, image_size=size, first_module=i, Cin=xin.shape[1], Cout=x.shape[1], H=xin.shape[2],
                              pool=n == 4, conv_output_MB=round(B * x.shape[1] * xin.shape[2] * xin.shape[3] * 4 / 1e6, 1),
                              hip_minus_stock_ms=round(line["hip_ms"] - line["stock_ms"], 4)))
                    i += n
                del x
        del img
        torch.cuda.empty_cache()


def e2e():
    from vqa_amd import extract as X, predict as P, train as T
    torch.backends.cudnn.deterministic = True
    with tempfile.TemporaryDirectory() as tmp:
        torch.manual_seed(5)
        ckpt = os.path.join(tmp, "net.pth")
        torch.save(T.build_model("attention", 50, 10).state_dict(), ckpt)
        argv = ["--model", "attention", "--batch_size", "64", "--model_ckpt", ckpt, "--num_cls", "10", "--image_size", "64", "--vocab_size", "50"]
        files, secs = {}, {}
        for impl in ("stock", "hip", "stock", "hip"):               # (the first round pays the solver searches and the comparisons)
            p = {k: os.path.join(tmp, impl + k) for k in (".jsonl", ".npz", ".npy")}
            t0 = time.perf_counter()
            P.main(argv + ["--test_size", "512", "--predictions", p[".jsonl"], "--attention_maps", p[".npz"], "--encoder_eval", impl])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            X.main(argv + ["--split", "val", "--samples", "512", "--out", p[".npy"], "--encoder_eval", impl])
            torch.cuda.synchronize()
            secs[impl] = {"predict_s": round(t1 - t0, 3), "extract_s": round(time.perf_counter() - t1, 3)}
            files[impl] = [open(p[k], "rb").read() for k in (".jsonl", ".npy")] + [open(p[".npy"][:-4] + ".json", "rb").read()]
        emit({"what": "e2e", "samples": 512, "image_size": 64, "second_round_seconds": secs,
              "equal_files": files["stock"] == files["hip"]})


if __name__ == "__main__":
    if "formula" in WHAT:
        formula()
    if "forward" in WHAT or "layers" in WHAT:
        forward_and_layers()
    if "e2e" in WHAT:
        e2e()

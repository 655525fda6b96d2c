"""Developer probe: image preprocessing (vqa_amd.preprocess, one HIP launch per batch) against the host transform it replaces
(PIL resize + lookup table per image) and inside a training step fed from a directory of JPEGs.

One process, B = 160, sources mixed 640x480 / 480x640 / 500x375, S = 224 and 448.  Per size:
* `kernel` (the C-ABI call bound once over a batch already on the device), `wrapper` (ImagePreprocessor.launch: adds the Python
  host time and allocates the output) and `upload` (the packed bytes from pinned memory plus the launch) alternate window by
  window (after a warm-up window each, WINDOWS windows of ITERS calls timed by HIP events; the median window and the spread
  (max - min) / median).  The kernel's share of the 8 TB/s HBM figure is over bytes read (pixels, tables)
  plus bytes written (the fp32 output).
* `host`: the same batch through preprocess_host's per-image work on WORKERS (16) worker processes, wall time per batch.
* `step`: Trainer.step of --model attention fed by DataLoader(WORKERS) over STEP_IMAGES generated JPEGs through the
  DevicePrefetcher, with --preprocess hip and with host, ms per step over STEPS steps after a warm-up epoch; and the decode
  alone (the same loader, nothing consumed).  Needs Pillow.

Environment: ITERS (10), WINDOWS (7), SIZES ("224,448"), B (160), WORKERS (16), STEPS (12), PARTS ("kernel,host,step"), OUT
(also append the JSON lines to this file)."""
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

B = int(os.environ.get("B", "160"))
ITERS = int(os.environ.get("ITERS", "10"))
WINDOWS = int(os.environ.get("WINDOWS", "7"))
WORKERS = int(os.environ.get("WORKERS", "16"))
STEPS = int(os.environ.get("STEPS", "12"))
PARTS = os.environ.get("PARTS", "kernel,host,step").split(",")
SOURCES = ((480, 640), (640, 480), (375, 500))
HBM_TBPS = 8.0


def emit(line):
    print(json.dumps(line), flush=True)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "a") as fh:
            fh.write(json.dumps(line) + "\n")


def source(i):
    """A decoded image: smooth structure plus noise (JPEG-like statistics matter to the decoder only)."""
    h, w = SOURCES[i % len(SOURCES)]
    g = np.random.default_rng(i)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(yy + 2 * xx) % 256, (3 * yy + xx) % 256, (yy * xx // 64) % 256], 2)
    return np.clip(base + g.integers(-20, 21, size=(h, w, 3)), 0, 255).astype(np.uint8)


def host_one(args):
    """One image's share of preprocess_host (a worker process: no GPU, no torch call)."""
    from PIL import Image
    img, S, lut = args
    small = np.asarray(Image.fromarray(img).resize((S, S), Image.BILINEAR))
    return lut[np.arange(3).reshape(1, 1, 3), small].transpose(2, 0, 1)


def timed(fn, iters, stream):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(variants, iters, stream):
    names = list(variants)
    for n in names:
        timed(variants[n], iters, stream)
    t = {n: [] for n in names}
    for w in range(WINDOWS):
        k = w % len(names)
        for n in names[k:] + names[:k]:                          # the order rotates
            t[n].append(timed(variants[n], iters, stream))
    return t


def probe_kernel(size, images, common):
    import torch
    from vqa_amd import _lib, preprocess as PP
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    pre = PP.ImagePreprocessor(size, device=dev)
    host = pre.pack(images, pin=True)
    packed = host.to(dev)
    for layout in ("nchw", "channels_last"):
        out = pre.empty(B, channels_last=layout == "channels_last")
        sB, sC, sH, sW = out.stride()
        base = packed.buf.data_ptr()
        call = _lib.bind("coattn_preprocess_images", pixels=base + packed.pix_off, pixel_bytes=packed.pix_bytes,
                         desc=base + packed.desc_off, coef=base + packed.coef_off, coef_count=packed.coef_count, lut=pre.lut, out=out,
                         sB=sB, sC=sC, sH=sH, sW=sW, bad_images=None, B=B, S=size, max_h=packed.max_h, max_w=packed.max_w,
                         stream=st.cuda_stream)
        variants = {"kernel": lambda: call(), "wrapper": lambda: pre.launch(packed, channels_last=layout == "channels_last"),
                    "upload": lambda: pre(host, channels_last=layout == "channels_last")}
        t = alternate(variants, ITERS, st)
        moved = packed.pix_bytes + 4 * packed.coef_count + out.numel() * 4
        line = dict(common, what="preprocess_kernel", image_size=size, layout=layout, bytes_in=packed.pix_bytes,
                    bytes_out=out.numel() * 4, bytes_moved=moved)
        for n, v in t.items():
            med = statistics.median(v)
            line[n + "_ms"] = round(med, 4)
            line[n + "_spread"] = round((max(v) - min(v)) / med, 4)
            line[n + "_windows_ms"] = [round(x, 4) for x in v]
        line["kernel_TBps"] = round(moved / line["kernel_ms"] / 1e9, 3)
        line["kernel_share_of_hbm"] = round(line["kernel_TBps"] / HBM_TBPS, 4)
        emit(line)
    assert PP.bad_images() == 0


def probe_host(size, images, common, pool):
    from vqa_amd import preprocess as PP
    lut = PP.lut_values().numpy()
    jobs = [(im, size, lut) for im in images]
    pool.map(host_one, jobs[:WORKERS])                           # warm the workers
    t = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        pool.map(host_one, jobs, chunksize=max(1, B // (4 * WORKERS)))
        t.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(t)
    emit(dict(common, what="host_transform", image_size=size, workers=WORKERS, batch_ms=round(med, 3),
              spread=round((max(t) - min(t)) / med, 4), windows_ms=[round(x, 3) for x in t],
              note="includes returning the fp32 arrays to the parent, as a DataLoader worker does"))


def probe_step(size, root, common):
    import torch
    from vqa_amd import data as D, preprocess as PP, train as T
    dev = torch.device("cuda:0")
    argv = ["--synthetic", "false", "--model", "attention", "--num_cls", "3", "--image_size", str(size), "--batch_size", str(B),
            "--train_file", os.path.join(root, "data.txt"), "--train_img", os.path.join(root, "images"),
            "--vocab_file", os.path.join(root, "vocab.pkl"), "--num_workers", str(WORKERS)]
    for mode in ("decode_only", "hip", "host"):
        args = T.build_parser().parse_args(argv + ["--preprocess", "hip" if mode == "decode_only" else mode])
        vocab = T.file_vocab(args)
        ds = T.file_dataset(args, "train", vocab)
        loader = T.file_loader(ds, args, shuffle=True, seed=1, drop_last=True)
        if mode == "decode_only":
            t0, n = time.perf_counter(), 0
            for _ in loader:
                n += 1
            emit(dict(common, what="decode_only", image_size=size, workers=WORKERS, batches=n,
                      batch_ms=round((time.perf_counter() - t0) * 1e3 / n, 3), note="includes the workers' start-up"))
            continue
        torch.manual_seed(0)
        model, _ = T.model_from_args(args)
        model.to(dev)
        model.image_encoder.to(memory_format=torch.channels_last)
        tr = T.Trainer(model, 1e-4, dev)
        fi = T.FileImages(args, size, dev)

        def sorted_host(b):
            im, qu, la, ln = T.sort_batch(fi.host(b["image"]), b["question"], b["label"], b["ques_len"])
            return im, qu, ln, la

        times = []
        for epoch in range(2):                                   # the first epoch warms the step and the workers
            batches = T.DevicePrefetcher((sorted_host(b) for b in loader), dev, True, preprocess=fi.hip)
            torch.cuda.synchronize()
            t0, n = time.perf_counter(), 0
            for image, question, ques_len, label in batches:
                nxt, ready = batches.peek_image()
                tr.step(image, question, ques_len, label, next_image=nxt, next_ready=ready)
                n += 1
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3 / n)
        emit(dict(common, what="train_step_from_jpegs", image_size=size, preprocess=mode, workers=WORKERS, steps=n,
                  step_ms=round(times[1], 3), warm_epoch_step_ms=round(times[0], 3), bad_images=PP.bad_images()))
        del tr, model


def write_dataset(root, n_images):
    from PIL import Image
    from vqa_amd import data as D
    os.makedirs(os.path.join(root, "images"))
    lines = []
    for i in range(n_images):
        Image.fromarray(source(i)).save(os.path.join(root, "images", "im_%05d.jpg" % i), quality=90)
        lines.append("im_%05d.jpg\twhat is in picture %d of the set\t%s" % (i, i % 7, ("yes", "no", "two")[i % 3]))
    with open(os.path.join(root, "data.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    D.save_vocab(D.build_vocab(os.path.join(root, "data.txt"), 1, 3), os.path.join(root, "vocab.pkl"))


def main():
    import multiprocessing as mp
    import torch
    import vqa_amd
    images = [source(i) for i in range(B)]
    common = {"B": B, "sources": [list(s) for s in SOURCES], "windows": WINDOWS, "iters": ITERS,
              "version": vqa_amd._lib.load().coattn_version(), "device": torch.cuda.get_device_name(0)}
    sizes = [int(x) for x in os.environ.get("SIZES", "224,448").split(",")]
    if "host" in PARTS:
        with mp.get_context("spawn").Pool(WORKERS) as pool:      # (spawned: the workers never open the GPU)
            for size in sizes:
                probe_host(size, images, common, pool)
    if "kernel" in PARTS:
        for size in sizes:
            probe_kernel(size, images, common)
    if "step" in PARTS:
        with tempfile.TemporaryDirectory() as root:
            write_dataset(root, STEPS * B)
            for size in sizes:
                probe_step(size, root, common)


if __name__ == "__main__":
    main()

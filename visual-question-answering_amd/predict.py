"""Inference of a trained checkpoint over a question set, with the co-attention maps: what the reference leaves as
``--mode test`` (main.py:285-287, ``raise NotImplementedError``) and the "Inference & Attention Visualization" line of its
README roadmap.  Same command line as ``train.py`` (the reference's flags) plus the outputs:

    python -m vqa_amd.predict --model attention --model_ckpt model.pth --test_size 1000 \\
        --predictions preds.jsonl --attention_maps maps.npz

* ``--predictions`` (JSONL): one record per sample in dataset order, ``{index, label, top, prob}`` -- the ``--topk``
  answer indices and their softmax probabilities, best first (index 0 is UNKNOWN, main.py:155).
* ``--attention_maps`` (``.npz``, ``attention*`` models only): ``a_v [S,3,H,W]`` -- the image attention of the word,
  phrase and sentence levels over the encoder's H x W grid (7 x 7 at 224 px, 14 x 14 at 448 px; model.py:215-217
  flattens it row-major) --, ``a_q [S,3,T]`` -- the question attention over the T token positions: by default UNMASKED as
  the reference's softmax (model.py:388), so positions past ``ques_len`` carry weight too; with ``--question_mask true``
  (the flag the checkpoint was trained with: it is not stored in the checkpoint) it is 0 past ``ques_len`` and sums to 1
  over the question's words --, ``ques_len [S]`` and ``index [S]``.
* stdout: one JSON line ``{samples, accuracy, top{K}_accuracy, loss, pairs_per_s}`` (accuracies in percent, as
  ``Trainer.validate``; loss = mean cross entropy per sample).

* ``--loss soft_ce | bce`` (the value the checkpoint was trained with; the checkpoint does not record it): the test split
  carries soft answer targets (``--num_answers`` slots), every record gains ``score`` -- min(1, target of its top answer), the
  VQA accuracy of the prediction -- and the summary ``vqa_score``, their mean; ``loss`` is then that loss kind's mean.  With
  ``bce`` the reported probabilities are per-class sigmoids (they do not sum to 1), else softmax probabilities.

* ``--attention_overlays DIR`` (``attention*`` models on images): the maps as pictures.  For each of the first
  ``--overlay_samples`` samples in dataset order (default 16; 0 = all) ``DIR/sample_{index:06d}.png``: the image and, beside
  it, the word, phrase and sentence levels' image attention upsampled over it (with ``--co_attention alternating`` its step-2
  and step-3 image maps) -- ``--overlay_mode heat`` (default): a colour ramp blended in at ``--overlay_alpha``; ``mask``: the
  image darkened to ``--overlay_floor`` where the attention is 0, as in the paper's figures --, and under each level
  ``--overlay_strip`` rows (default 32) of its question attention, one cell per token position, black past ``ques_len`` under
  ``--question_mask true``.  ``DIR/index.json`` lists per sample ``{file, index, label, top, prob, ques_len, question}``
  (the token ids: the data is synthetic, so no words are drawn).  ``--image_mean`` / ``--image_std``: the normalisation the
  images carry (default ImageNet's, main.py:126).  Rendered per batch on the device in one HIP launch
  (``vqa_amd.overlay.render_attention``); only the chosen samples' bytes come to the host.

The maps come from the forward-only co-attention (``coattn_infer``): no state for a backward is written.  One process:
multi-GPU prediction is not offered.  Data: the synthetic test split (its own seed), every sample (no drop_last) -- or, with
``--synthetic false --test_file F --test_img DIR --vocab_file V``, the reference's dataset files (``vqa_amd.data``; images
resized and normalised by ``vqa_amd.preprocess``, ``--preprocess hip | host``): every record then gains ``image`` (the file
name), ``question`` (the cleaned words) and ``answers`` (the top-k answers as strings, through the vocabulary's ``idx2label``);
``--image_features`` takes a table of ``extract.py --synthetic false --split test``, and ``--image_mean`` / ``--image_std``
also set the normalisation the images are given.
"""
from __future__ import annotations

import json
import math
import os
import time

import numpy as np
import torch
import torch.nn.functional as F
import torch.utils.data

from . import loss as L
from . import train as T

TEST_SEED = 555555


def build_parser():
    ap = T.build_parser()
    ap.description = "Visual Question Answering: predictions and attention maps of a trained checkpoint"
    ap.add_argument("--predictions", type=str, default=None, help="write one JSON record per sample here (JSONL)")
    ap.add_argument("--topk", type=int, default=5, help="answers per record, best first")
    ap.add_argument("--attention_maps", type=str, default=None,
                    help="write the co-attention maps here (.npz; attention* models only)")
    ap.add_argument("--test_size", type=int, default=1000, help="test samples (synthetic)")
    ap.add_argument("--attention_overlays", type=str, default=None, metavar="DIR",
                    help="write the attention maps drawn over the images here (PNG sheets and index.json; attention* models on "
                         "images only)")
    ap.add_argument("--overlay_mode", default="heat", choices=["heat", "mask"],
                    help="'heat' = a colour ramp blended into the image; 'mask' = brightness follows attention")
    ap.add_argument("--overlay_samples", type=int, default=16, help="overlays of the first M samples in dataset order (0 = all)")
    ap.add_argument("--overlay_alpha", type=float, default=0.6, help="heat mode: the weight of the colour, in [0, 1]")
    ap.add_argument("--overlay_floor", type=float, default=0.3, help="mask mode: the brightness at zero attention, in [0, 1]")
    ap.add_argument("--image_mean", type=float, nargs=3, default=None, metavar=("R", "G", "B"),
                    help="the mean the images were normalised with (default: ImageNet's)")
    ap.add_argument("--image_std", type=float, nargs=3, default=None, metavar=("R", "G", "B"),
                    help="the std the images were normalised with (default: ImageNet's)")
    ap.add_argument("--overlay_strip", type=int, default=32, metavar="PX",
                    help="rows of the question-attention strip under every level (0 = none)")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.model_ckpt:
        ap.error("--model_ckpt is required: prediction runs a trained checkpoint (train.py --save_path / model_{step}.pth)")
    if args.attention_maps and not args.model.startswith("attention"):
        ap.error("--attention_maps needs a co-attention model (--model attention*); %r has no attention maps" % args.model)
    if args.attention_overlays:
        if not args.model.startswith("attention"):
            ap.error("--attention_overlays needs a co-attention model (--model attention*); %r has no attention maps" % args.model)
        if args.image_features:
            ap.error("--attention_overlays draws over the images; a run from --image_features (cached features) has no pixels")
        if args.overlay_samples < 0:
            ap.error("--overlay_samples must be >= 0 (0 = every sample), got %d" % args.overlay_samples)
        if args.overlay_strip < 0:
            ap.error("--overlay_strip must be >= 0, got %d" % args.overlay_strip)
        if not (0.0 <= args.overlay_alpha <= 1.0 and 0.0 <= args.overlay_floor <= 1.0):
            ap.error("--overlay_alpha and --overlay_floor must lie in [0, 1]")
    if args.topk < 1 or args.test_size < 1:
        ap.error("--topk and --test_size must be >= 1")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        ap.error("prediction runs in one process (WORLD_SIZE=%s): multi-GPU prediction is not offered"
                 % os.environ["WORLD_SIZE"])
    files = not args.synthetic             # the reference's dataset files: --test_file / --test_img / --vocab_file
    vocab = None
    try:
        if files:
            T.check_files(args, "test")
            vocab = T.file_vocab(args)
        T.check_loss(args.loss, args.num_answers)
        if args.val_image_features:
            raise ValueError("--val_image_features is train.py's; prediction takes the test split's table as --image_features")
        T.check_image_features(args)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    cached = bool(args.image_features)     # the test split's feature table (extract --split test) in place of the encoder

    if torch.cuda.is_available():
        device = torch.device("cuda", args.gpu_id)
        torch.cuda.set_device(device)
        torch.set_num_threads(max(1, min(4, T.usable_cpus())))
    else:
        device = torch.device("cpu")
    try:
        T.check_encoder_eval(args.model, args.encoder_eval, args.channels_last, device.type, args.opt_lvl)
    except ValueError as e:
        ap.error(str(e))
    torch.manual_seed(0)
    model, cfg = T.model_from_args(args)
    model.load_state_dict(torch.load(T.checkpoint_path(args), map_location="cpu"))
    model.to(device)
    T.set_encoder_eval(model, args.encoder_eval)
    cl = args.channels_last and device.type == "cuda" and args.model.startswith("attention")
    if cl:
        model.image_encoder.to(memory_format=torch.channels_last)
    T.set_products(model, args.precision)                       # the settings Trainer applies for --precision / --opt_lvl
    T.set_reduced_precision(model, args.opt_lvl)
    soft = args.loss != "ce"                                    # the split then carries soft answer targets
    criterion = T.SoftTargetLoss(args.loss) if soft else T.CrossEntropyLoss()
    size = (args.image_size, args.image_size) if args.image_size else cfg["image_size"]
    n_cls = args.num_cls + 1
    k = min(args.topk, n_cls)
    file_images = None
    if files:
        ds = T.file_dataset(args, "test", vocab)
        file_images = T.FileImages(args, size[0], device, args.image_mean, args.image_std)
    else:
        ds = T.SyntheticVQADataset(args.test_size, size, args.max_seq_length, args.vocab_size, n_cls, TEST_SEED,
                                   num_answers=args.num_answers if soft else 0, images=not cached)
    feats = None
    if cached:
        from .features import FeatureTable, bad_indices
        feats = FeatureTable.load(args.image_features, device)
        try:
            if files:
                feats.check_files(args.model, size[0], "test", ds.image_names)
            else:
                feats.check(args.model, size[0], "test", TEST_SEED, args.test_size)
        except ValueError as e:
            ap.error(str(e))
    if files:
        loader = T.file_loader(ds, args, shuffle=False)
    else:
        loader = torch.utils.data.DataLoader(ds, args.batch_size, shuffle=False, drop_last=False, num_workers=args.num_workers)
    maps = bool(args.attention_maps)
    overlays = bool(args.attention_overlays)
    if overlays:
        if device.type != "cuda":
            ap.error("--attention_overlays renders on the GPU (there is no CPU fallback)")
        from . import overlay as OV
        os.makedirs(args.attention_overlays, exist_ok=True)
        n_over = len(ds) if args.overlay_samples == 0 else min(args.overlay_samples, len(ds))
        over_kw = dict(mode=args.overlay_mode, alpha=args.overlay_alpha, floor=args.overlay_floor, strip=args.overlay_strip,
                       mean=tuple(args.image_mean or OV.IMAGENET_MEAN), std=tuple(args.image_std or OV.IMAGENET_STD))
        sheets = {}                                            # sample index -> (file name, token ids)

    S = len(ds)
    top = torch.zeros((S, k), dtype=torch.int64)
    prob = torch.zeros((S, k), dtype=torch.float32)
    labels = torch.zeros(S, dtype=torch.int64)
    lens = torch.zeros(S, dtype=torch.int64)
    scores = torch.zeros(S, dtype=torch.float32) if soft else None
    a_v = a_q = None
    loss_sum = 0.0
    model.eval()
    t0 = time.time()
    start = 0
    with torch.no_grad():
        for b in loader:
            n = b["label"].numel()
            index = torch.arange(start, start + n)
            start += n
            # sorted by question length for packing (main.py:196-202); the index rides along as a second label column
            extras = (b["answers"], b["answer_scores"]) if soft else ()
            if files:
                b["image"] = file_images.host(b["image"])       # the decoded pixels, packed (hip) or preprocessed (host)
            image, question, il, ques_len, *extras = T.sort_batch(b["image"], b["question"], torch.stack([index, b["label"]], 1),
                                                                  b["ques_len"], *extras)
            targets = [e.to(device) for e in extras]
            idx, label = il[:, 0], il[:, 1]
            image = file_images.device_images(image, cl and not cached) if files else image.to(device)
            if cached:
                image = feats.gather(image)                     # `image` held the batch's row indices
            elif cl and not files:
                image = image.contiguous(memory_format=torch.channels_last)
            question, label_d = question.to(device), label.to(device)
            draw = overlays and int(idx.min()) < n_over         # a chosen sample is in this batch
            with T.autocast_for(args.opt_lvl, device):
                if cached:
                    if maps:
                        logits, av, aq = model.forward_features_with_attention(image, question, ques_len)
                    else:
                        logits = model.forward_features(image, question, ques_len)
                elif maps or draw:
                    logits, av, aq = model.forward_with_attention(image, question, ques_len)
                else:
                    logits = model(image, question, ques_len)
            if soft:
                loss_sum += float(criterion(logits.float(), *targets)) * n
                scores[idx] = L.vqa_score(logits.float(), *targets)[1].cpu()
            else:
                loss_sum += float(criterion(logits.float(), label_d)) * n
            probs = torch.sigmoid(logits.float()) if args.loss == "bce" else F.softmax(logits.float(), dim=1)
            pv, pi = probs.topk(k, dim=1)
            top[idx], prob[idx], labels[idx], lens[idx] = pi.cpu(), pv.cpu(), label, ques_len
            if draw:
                # drawn on the device from the maps as they are; only the chosen samples' panels come to the host
                chosen = (idx < n_over).nonzero().flatten()
                panels = OV.render_attention(image, av.float(), aq.float(), ques_len if args.question_mask else None, **over_kw)
                panels = panels[chosen.to(device)].cpu()
                for j, i in enumerate(idx[chosen].tolist()):
                    name = "sample_%06d.png" % i
                    OV.write_png(os.path.join(args.attention_overlays, name), OV.sheet(panels[j]))
                    sheets[i] = (name, question[int(chosen[j])].tolist())
            if maps:
                if a_v is None:
                    a_v = torch.zeros((S,) + tuple(av.shape[:1]) + tuple(av.shape[2:]), dtype=torch.float32)
                    a_q = torch.zeros((S,) + tuple(aq.shape[:1]) + tuple(aq.shape[2:]), dtype=torch.float32)
                a_v[idx] = av.permute(1, 0, 2).float().cpu()
                a_q[idx] = aq.permute(1, 0, 2).float().cpu()
    if device.type == "cuda":
        torch.cuda.synchronize()
        if cached and bad_indices():
            raise IndexError("image indices lay outside the feature table (their rows were zeros)")
        if files and file_images.hip is not None:
            from .preprocess import bad_images
            if bad_images():
                raise ValueError("images were refused by the preprocessing launch (their pixels were zeros)")
        if overlays and OV.bad_maps():
            raise FloatingPointError("attention maps could not be normalised for their overlays (NaN, infinite, negative or all "
                                     "zero); those panels were drawn without attention")
        if args.precision == "fast" and args.opt_lvl == 0:
            from . import _lib
            _lib.check_range()                   # raises if an operand of the tolerance mode left the FP16-piece range
    elapsed = time.time() - t0

    hit1 = top[:, 0] == labels
    hitk = (top == labels[:, None]).any(dim=1)
    if args.predictions:
        with open(args.predictions, "w") as fh:
            for i in range(S):
                rec = {"index": i, "label": int(labels[i]), "top": top[i].tolist(), "prob": [float(x) for x in prob[i]]}
                if files:                                       # the sample in words: its image, its question, the answers
                    rec.update(image=ds.samples[i][0], question=ds.words(i),
                               answers=[vocab["idx2label"][int(t)] for t in top[i]])
                if soft:
                    rec["score"] = float(scores[i])
                fh.write(json.dumps(rec) + "\n")
    if overlays:
        with open(os.path.join(args.attention_overlays, "index.json"), "w") as fh:
            json.dump([{"file": sheets[i][0], "index": i, "label": int(labels[i]), "top": top[i].tolist(),
                        "prob": [float(x) for x in prob[i]], "ques_len": int(lens[i]), "question": sheets[i][1]}
                       for i in sorted(sheets)], fh, indent=1)
    if maps:
        N = a_v.shape[-1]
        H = int(round(math.sqrt(N)))
        if H * H != N:
            raise RuntimeError("the image grid of %d locations is not square" % N)
        np.savez(args.attention_maps, a_v=a_v.view(S, a_v.shape[1], H, H).numpy(), a_q=a_q.numpy(),
                 ques_len=lens.numpy(), index=np.arange(S))
    summary = {"samples": S, "accuracy": round(100.0 * float(hit1.float().mean()), 4),
               "top%d_accuracy" % k: round(100.0 * float(hitk.float().mean()), 4),
               "loss": round(loss_sum / S, 6), "pairs_per_s": round(S / max(elapsed, 1e-9), 2)}
    if soft:
        summary["vqa_score"] = round(float(scores.mean()), 6)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()

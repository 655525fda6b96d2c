"""Encode the images of a split once into a feature table (``features.FeatureTable``) for ``train.py --image_features`` and
``predict.py --image_features``:

    python -m vqa_amd.extract --model attention --split train --samples 1280 --out train_feats.npy
    python -m vqa_amd.train   --model attention --num_steps 8 --batch_size 160 --image_features train_feats.npy

Same model and data flags as ``train.py``.  The model is built as ``train.py`` builds it (``--model_ckpt`` optional), put in
eval mode under ``no_grad`` -- BatchNorm on its running statistics, the function ``Trainer.validate`` and ``predict.py``
evaluate with -- and the split's ``SyntheticVQADataset`` is walked in index order with the seed its consumer uses (train
``1234 + rank``, val ``987654 + rank``, test ``predict.TEST_SEED``); row i of the table is
``native_features(model.image_encoder(image_i))``, the convolutions on MIOpen's deterministic solvers
(``torch.backends.cudnn.deterministic`` for the pass: the default ones do not repeat their own bits, and a table should be a
function of the weights and the images alone).  ``--features_dtype bf16`` rounds to nearest even (torch's cast).  The
co-attention models only: the baseline has no grid.  With ``{rank}`` in ``--out`` every rank of a launcher writes its own table.

``--synthetic false --split train|val|test`` with that split's data file, image directory and ``--vocab_file`` encodes the
DISTINCT images of the data file, one row each in first-seen order (``data.VQAFileDataset.image_names``; ``--samples`` is
ignored); the sidecar additionally records ``"source": "files"``, the image count and the SHA-256 of the newline-joined names,
which ``FeatureTable.check_files`` holds a run's file list against.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import features as FT
from . import train as T
from .coattention import native_features

MODELS = ("attention", "attention_resnet", "attention_bert")


def split_seed(split: str, rank: int = 0) -> int:
    """The dataset seed the consumer of `split` uses (train.main: 1234 + rank, 987654 + rank; predict.TEST_SEED)."""
    if split == "train":
        return 1234 + rank
    if split == "val":
        return 987654 + rank
    if split == "test":
        from .predict import TEST_SEED
        return TEST_SEED
    raise ValueError("split must be one of %s, got %r" % (FT.SPLITS, split))


def build_parser():
    ap = T.build_parser()
    ap.description = "Visual Question Answering: encode a split's images once into a feature table"
    ap.add_argument("--split", default="train", choices=list(FT.SPLITS))
    ap.add_argument("--samples", type=int, default=0, help="S: images to encode, dataset indices 0 .. S - 1")
    ap.add_argument("--features_dtype", default="fp32", choices=list(FT.DTYPES),
                    help="storage of the table: fp32, or bf16 (round to nearest even; half the bytes, other values)")
    ap.add_argument("--out", type=str, default=None, help="the table (.npy); its sidecar is written beside it ({rank}: this rank's)")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.model not in MODELS:
        ap.error("feature tables hold the co-attention models' grid (--model %s); %r has none" % (" | ".join(MODELS), args.model))
    files = not args.synthetic
    if not args.out or (args.samples < 1 and not files):
        ap.error("--samples S >= 1 and --out PATH are required")
    vocab = None
    if files:
        if args.image_features:
            ap.error("--image_features is what this command writes (--out); it reads the images")
        try:
            T.check_files(args, args.split, int(os.environ.get("WORLD_SIZE", "1")))
            vocab = T.file_vocab(args)
        except (ValueError, OSError) as e:
            raise SystemExit(str(e))
    rank = int(os.environ.get("RANK", "0"))
    out_path = args.out.replace("{rank}", str(rank))
    if torch.cuda.is_available():
        device = torch.device("cuda", int(os.environ["LOCAL_RANK"]) if "LOCAL_RANK" in os.environ else args.gpu_id)
        torch.cuda.set_device(device)
        torch.set_num_threads(max(1, min(4, T.usable_cpus())))
    else:
        device = torch.device("cpu")
    try:
        T.check_encoder_eval(args.model, args.encoder_eval, args.channels_last, device.type, args.opt_lvl)
    except ValueError as e:
        ap.error(str(e))
    torch.manual_seed(0)                                        # the weights train.py starts from
    model, cfg = T.model_from_args(args)
    T.set_encoder_eval(model, args.encoder_eval)
    if args.model_ckpt:
        model.load_state_dict(torch.load(T.checkpoint_path(args), map_location="cpu"))
    model.to(device)
    cl = args.channels_last and device.type == "cuda"
    if cl:
        model.image_encoder.to(memory_format=torch.channels_last)
    model.eval()
    size = (args.image_size, args.image_size) if args.image_size else cfg["image_size"]
    file_images = names = None
    if files:
        # one row per DISTINCT image of the data file, in first-seen order (data.VQAFileDataset.image_names): VQA asks about
        # three questions per image, and `train.py --image_features` maps every line to its image's row
        from . import data as D
        ds = D.DistinctImages(T.file_dataset(args, args.split, vocab))
        names = ds.ds.image_names
        seed, args.samples = 0, len(names)
        file_images = T.FileImages(args, size[0], device)
        loader = T.file_loader(ds, args, shuffle=False)
    else:
        seed = split_seed(args.split, rank)
        ds = T.SyntheticVQADataset(args.samples, size, args.max_seq_length, args.vocab_size, args.num_cls + 1, seed)
        loader = torch.utils.data.DataLoader(ds, args.batch_size, shuffle=False, drop_last=False, num_workers=args.num_workers)
    bf16 = args.features_dtype == "bf16"
    # A table is a function of the weights and the images alone: the convolutions run on MIOpen's deterministic solvers here.
    # (The default solvers do not repeat their own bits -- measured: the eval-mode features of two passes over one batch differ
    # in 47 % of the elements, by up to 1.1e-8 at a scale of 2.5e-2, from the third convolution on; with the switch six passes
    # are identical, whatever the order of the samples inside the batch.)
    deterministic, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    try:
        _, N, d = _encode(model, loader, device, cl, args, out_path, bf16, file_images)
    finally:
        torch.backends.cudnn.deterministic = deterministic
    if files and file_images.hip is not None:
        from .preprocess import bad_images
        n_bad = bad_images()
        if n_bad:
            raise ValueError("%d images were refused by the preprocessing launch (their rows are those of zeros)" % n_bad)
    meta = FT.make_meta(args.model, size[0], N, d, args.features_dtype, args.split, seed, args.samples)
    if files:
        meta = FT.files_meta(meta, names)
    with open(FT.sidecar_path(out_path), "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
    print(json.dumps({"out": out_path, **meta}))
    return meta


def _encode(model, loader, device, cl, args, out_path, bf16, file_images=None):
    """Walk `loader` in order and write row i of the table at `out_path`; returns (rows written, N, d).  `file_images`
    (train.FileImages): the batches carry decoded pixels, resized and normalised here."""
    table = None
    start = 0
    with torch.no_grad():
        for b in loader:
            if file_images is not None:
                image = file_images.device_images(file_images.host(b["image"]), cl)
            else:
                image = b["image"].to(device)
                if cl:
                    image = image.contiguous(memory_format=torch.channels_last)
            with T.autocast_for(args.opt_lvl, device):
                feats = native_features(model.image_encoder(image))
            if bf16:
                feats = feats.to(torch.bfloat16)
            n, N, d = feats.shape
            if table is None:
                table = np.lib.format.open_memmap(out_path, mode="w+", dtype=np.uint16 if bf16 else np.float32,
                                                  shape=(args.samples, N, d))
            host = feats.contiguous().cpu()
            table[start:start + n] = host.view(torch.int16).numpy().view(np.uint16) if bf16 else host.numpy()
            start += n
    table.flush()
    return start, N, d


if __name__ == "__main__":
    main()

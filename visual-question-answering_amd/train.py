"""Training loop of the reference (``main.py``) restated for MI355X: same ``--model attention``
registry, same step order (sort batch by length -> H2D -> forward -> CrossEntropyLoss ->
zero_grad -> backward -> Adam step; main.py:193-222), plus what the reference lacks: synthetic
data (no dataset / network here) and data-parallel training, one process per GPU, with RCCL
gradient all-reduce (``vqa_amd.dist``).  apex AMP (main.py:185) is CUDA-only; ``--opt_lvl 0``
(fp32) is the parity mode, levels >= 1 map to ``torch.autocast(bfloat16)`` around the stock
encoders while the co-attention path keeps computing in fp32.

Run:  python -m torch.distributed.run --nproc-per-node N -m vqa_amd.train --synthetic ...

``--synthetic false --train_file F --train_img DIR --vocab_file V [--val_file F --val_img DIR] [--preprocess hip|host]`` trains
on the reference's dataset files (``vqa_amd.data``): the vocabulary sets the vocabulary size and the question length, an epoch
is one pass over the file, and the images are resized and normalised per batch by ``vqa_amd.preprocess`` -- on a GPU in one HIP
launch that the prefetcher queues on its copy stream behind the batch's decoded pixels.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import time
from typing import Dict

import torch
import torch.nn as nn
import torch.utils.data

from . import dist as vdist
from .loss import CrossEntropyLoss, SoftTargetLoss
from .dropout import DropoutState, rank_seed
from .modules import HierarchicalCoAttentionNet, VQABaselineNet, set_feature_dropout  # noqa: F401  (set_feature_dropout: re-exported)

PATH_VGG_WEIGHTS = None      # the reference hard-codes a local .pth (utils.py:15); none ships here


def usable_cpus() -> int:
    """CPUs this process may actually use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def str2bool(v):
    return str(v).lower() in ("yes", "true", "t", "1")


def int_min_two(k):
    k = int(k)
    if k < 2:
        raise argparse.ArgumentTypeError("must be >= 2")
    return k


def setup_model_configs(args, vocab_size: int, vgg_train: bool = False, vgg_wts_path=None) -> dict:
    """--model -> class, image size and encoder parameters (main.py:388-418).  Called as the reference calls it,
    ``setup_model_configs(args, vocab_size)`` with the parsed command line (main.py:388: ``args.model``,
    ``args.vgg_train``, ``args.vgg_wts_path`` are read), or with the model name and the two VGG settings spelled out.
    The 'attention' entry's ``mlp_dim`` key is carried but never forwarded by the reference (main.py:164), so the
    model's own default (1024, model.py:160) applies; both are 1024."""
    if isinstance(args, str):
        model_name = args
    else:                                            # the reference's argparse namespace
        model_name = args.model
        vgg_train = getattr(args, "vgg_train", vgg_train)
        vgg_wts_path = getattr(args, "vgg_wts_path", vgg_wts_path)
    img = dict(is_trainable=vgg_train, weights_path=vgg_wts_path or PATH_VGG_WEIGHTS)
    if model_name == "attention_bert":
        # BASELINE config 5 (extension; the reference lists BERT as a TODO, README.md:137-141): the attention model with
        # frozen BERT-base token embeddings (768-d, WordPiece vocabulary of 30,522; built from the config -- random init,
        # there is no network for checkpoints) projected to the hidden size as the word level.  `vocab_size` is BERT's own.
        return dict(model=HierarchicalCoAttentionNet, image_size=(448, 448), image_params=img,
                    question_params=bert_question_params(hidden_dim=512), mlp_dim=1024, vocab_size=BERT_VOCAB)
    registry = {
        "baseline": dict(model=VQABaselineNet, image_size=(224, 224), image_params=img,
                         question_params=dict(vocab_size=vocab_size, word_emb_dim=300, hidden_dim=1024)),
        "attention": dict(model=HierarchicalCoAttentionNet, image_size=(448, 448), image_params=img,
                          question_params=dict(vocab_size=vocab_size, word_emb_dim=512, hidden_dim=512),
                          mlp_dim=1024),
        # BASELINE config 4 (extension): ResNet-152 7x7x2048 grid, hidden size 2048; run with --opt_lvl 1
        # for bf16 autocast around the stock encoders and the bf16-MFMA projections of the co-attention
        "attention_resnet": dict(model=HierarchicalCoAttentionNet, image_size=(224, 224),
                                 image_params=dict(img, arch="resnet152"),
                                 question_params=dict(vocab_size=vocab_size, word_emb_dim=2048, hidden_dim=2048),
                                 mlp_dim=1024),
    }
    return registry[model_name]      # 'bert' is accepted by the reference's argparse but has no entry: KeyError


BERT_VOCAB = 30522                   # bert-base-uncased's WordPiece vocabulary


def bert_question_params(hidden_dim: int = 512, vocab_size: int = BERT_VOCAB, bert_dim: int = 768) -> dict:
    """Question-encoder parameters for BASELINE config 5: frozen BERT-base token embeddings (random
    init -- no network for checkpoints) in place of the learned word embedding."""
    from transformers import BertConfig
    from transformers.models.bert.modeling_bert import BertEmbeddings
    cfg = BertConfig(vocab_size=vocab_size, hidden_size=bert_dim)
    return dict(bert=BertEmbeddings(cfg), bert_dim=bert_dim, hidden_dim=hidden_dim)


def set_question_mask(model: nn.Module, question_mask: bool) -> None:
    """--question_mask: the co-attention's softmax over question tokens restricted to each question's length
    (ParallelCoAttention.question_mask; off = the reference's unmasked softmax, model.py:388).  The models without a
    co-attention have nothing to mask: asking for it there is an error."""
    co = getattr(model, "co_attention", None)
    if co is None or not hasattr(co, "question_mask"):
        if question_mask:
            raise ValueError("--question_mask applies to the co-attention models (--model attention*), not to %s"
                             % type(model).__name__)
        return
    co.question_mask = bool(question_mask)


def check_affinity(model_name: str, affinity: str, opt_lvl: int = 0) -> None:
    """--affinity: "reference" (the default: C = tanh(Q V^T), model.py:377, W_b untrained) or "bilinear" (the published model's
    C = tanh(W_b(Q) V^T), W_b trained; ParallelCoAttention(affinity=...)).  The bilinear form exists for the co-attention
    models only and not in the reduced-precision mode (--opt_lvl >= 1): both are errors."""
    if affinity not in ("reference", "bilinear"):
        raise ValueError("--affinity must be 'reference' or 'bilinear', got %r" % (affinity,))
    if affinity == "reference":
        return
    if not model_name.startswith("attention"):
        raise ValueError("--affinity bilinear applies to the co-attention models (--model attention*), not to %s" % model_name)
    if opt_lvl > 0:
        raise ValueError("--affinity bilinear is not available with --opt_lvl >= 1 (the reduced-precision mode)")


def check_co_attention(model_name: str, co_attention: str, affinity: str = "reference", opt_lvl: int = 0,
                       precision: str = "exact") -> None:
    """--co_attention: "parallel" (the default: the reference's ParallelCoAttention) or "alternating" (AlternatingCoAttention,
    Lu et al. 2016 section 3.3).  The alternating form exists for the co-attention models only and in the exact mode only:
    with --affinity bilinear (a parallel-form option), --opt_lvl >= 1 or --precision fast it is an error."""
    if co_attention not in ("parallel", "alternating"):
        raise ValueError("--co_attention must be 'parallel' or 'alternating', got %r" % (co_attention,))
    if co_attention == "parallel":
        return
    if not model_name.startswith("attention"):
        raise ValueError("--co_attention alternating applies to the co-attention models (--model attention*), not to %s"
                         % model_name)
    if affinity != "reference":
        raise ValueError("--co_attention alternating has no affinity matrix: --affinity %s applies to the parallel form only"
                         % affinity)
    if opt_lvl >= 1:
        raise ValueError("--co_attention alternating is not available with --opt_lvl >= 1 (the reduced-precision mode)")
    if precision == "fast":
        raise ValueError("--co_attention alternating runs in the exact mode only, not with --precision fast")


def _net_kwargs(co_attention: str) -> dict:
    return {} if co_attention == "parallel" else {"co_attention": co_attention}


def set_affinity(model: nn.Module, affinity: str) -> None:
    """The co-attention's affinity form (see `check_affinity`): a module attribute, not part of the state_dict."""
    co = getattr(model, "co_attention", None)
    if co is None or not hasattr(co, "affinity"):
        if affinity != "reference":
            raise ValueError("--affinity bilinear applies to the co-attention models (--model attention*), not to %s"
                             % type(model).__name__)
        return
    if affinity not in co.AFFINITIES:
        raise ValueError("affinity must be one of %s, got %r" % (co.AFFINITIES, affinity))
    co.affinity = affinity


SENTENCE_LSTMS = ("stock", "hip")


def set_sentence_lstm(model: nn.Module, sentence_lstm: str) -> None:
    """--sentence_lstm: "stock" (the default: pack_padded_sequence -> nn.LSTM -> pad_packed_sequence) or "hip" (the question
    encoder's sentence level on lstm.sentence_lstm: same parameters, lengths read on the device).  A module attribute
    (QuestionCoAttentionEncoder.sentence_impl), not part of the state_dict: a checkpoint does not depend on it.  The models
    without such an encoder have nothing to switch: asking for "hip" there is an error."""
    if sentence_lstm not in SENTENCE_LSTMS:
        raise ValueError("--sentence_lstm must be one of %s, got %r" % (SENTENCE_LSTMS, sentence_lstm))
    enc = getattr(model, "question_encoder", None)
    if enc is None or not hasattr(enc, "sentence_impl"):
        if sentence_lstm != "stock":
            raise ValueError("--sentence_lstm hip applies to the co-attention models (--model attention*), not to %s"
                             % type(model).__name__)
        return
    enc.sentence_impl = sentence_lstm


QUESTION_GRUS = ("stock", "hip")


def set_question_gru(model: nn.Module, question_gru: str) -> None:
    """--question_gru: "stock" (the default: pack_padded_sequence -> nn.GRU, sorted lengths, a host read of them) or "hip" (the
    baseline question encoder's GRU on gru.question_gru: same parameters, lengths read on the device in any order).  A module
    attribute (QuestionBaselineEncoder.gru_impl), not part of the state_dict: a checkpoint does not depend on it.  The models
    whose question encoder has no GRU have nothing to switch: asking for "hip" there is an error."""
    if question_gru not in QUESTION_GRUS:
        raise ValueError("--question_gru must be one of %s, got %r" % (QUESTION_GRUS, question_gru))
    enc = getattr(model, "question_encoder", None)
    if enc is None or not hasattr(enc, "gru_impl"):
        if question_gru != "stock":
            raise ValueError("--question_gru hip applies to the baseline model (--model baseline), not to %s"
                             % type(model).__name__)
        return
    enc.gru_impl = question_gru


ENCODER_EVALS = ("stock", "hip")
ENCODER_EVAL_MODELS = ("attention", "attention_bert")


def check_encoder_eval(model_name: str, encoder_eval: str, channels_last: bool = True, device_type: str = "cuda",
                       opt_lvl: int = 0) -> None:
    """--encoder_eval hip: the frozen VGG's eval-mode groups (validation, prediction, feature extraction) on the one-launch HIP
    passes of encoder.bn_eval / conv1_bn_eval; "stock", the default, leaves every route as it is.  "hip" is refused for a model
    without a VGG grid, with --channels_last false (the kernels read [B][H][W][C]), on a CPU device and with --opt_lvl >= 1
    (under autocast the stock BatchNorm sees another dtype)."""
    if encoder_eval not in ENCODER_EVALS:
        raise ValueError("--encoder_eval must be one of %s, got %r" % (ENCODER_EVALS, encoder_eval))
    if encoder_eval == "stock":
        return
    if model_name not in ENCODER_EVAL_MODELS:
        raise ValueError("--encoder_eval hip applies to the models with a VGG grid (--model %s), not to %s"
                         % (" | ".join(ENCODER_EVAL_MODELS), model_name))
    if not channels_last:
        raise ValueError("--encoder_eval hip is not available with --channels_last false: the kernels read channels_last tensors")
    if device_type != "cuda":
        raise ValueError("--encoder_eval hip needs a GPU: the kernels have no CPU form (device %s)" % device_type)
    if opt_lvl > 0:
        raise ValueError("--encoder_eval hip is not available with --opt_lvl >= 1 (the reduced-precision mode)")


def set_encoder_eval(model: nn.Module, encoder_eval: str) -> None:
    """--encoder_eval on a built model: a module attribute (ImageCoAttentionEncoder.eval_impl), not part of the state_dict.  A
    model whose image encoder has no such switch has nothing to set: asking for "hip" there is an error."""
    if encoder_eval not in ENCODER_EVALS:
        raise ValueError("--encoder_eval must be one of %s, got %r" % (ENCODER_EVALS, encoder_eval))
    enc = getattr(model, "image_encoder", None)
    if enc is None or not hasattr(enc, "eval_impl"):
        if encoder_eval != "stock":
            raise ValueError("--encoder_eval hip applies to the models with a VGG grid (--model %s), not to %s%s"
                             % (" | ".join(ENCODER_EVAL_MODELS), type(model).__name__,
                                "" if enc is None else " with " + type(enc).__name__))
        return
    enc.eval_impl = encoder_eval


WORD_EMBEDDINGS = ("stock", "hip")


def set_word_embedding(model: nn.Module, word_embedding: str) -> None:
    """--word_embedding: "stock" (the default: nn.Embedding's forward and PyTorch's embedding backward) or "hip" (the question
    encoder's word level on embedding.word_embedding: same parameter, same dense gradient, ids read on the device).  A module
    attribute (QuestionCoAttentionEncoder.word_impl), not part of the state_dict.  Only the LSTM question encoder of
    --model attention has that word level (attention_bert's is the frozen BERT, the baseline has no such encoder): asking
    for "hip" elsewhere is an error."""
    if word_embedding not in WORD_EMBEDDINGS:
        raise ValueError("--word_embedding must be one of %s, got %r" % (WORD_EMBEDDINGS, word_embedding))
    enc = getattr(model, "question_encoder", None)
    if enc is None or not hasattr(enc, "word_impl"):
        if word_embedding != "stock":
            raise ValueError("--word_embedding hip applies to the co-attention model with the embedding word level "
                             "(--model attention), not to %s%s" % (type(model).__name__, "" if enc is None else
                                                                  " with " + type(enc).__name__))
        return
    enc.word_impl = word_embedding


FUSION_HEADS = ("stock", "hip")


def check_fusion_head(model_name: str, fusion_head: str, vgg_train: bool = False, opt_lvl: int = 0) -> None:
    """--fusion_head: "stock" (the default: the nn modules behind the two encoders) or "hip" (fusion.fusion_head).  "hip" exists
    for --model baseline with a frozen image encoder in exact fp32: another model, --vgg_train true (the head has no gradient
    for the image features) and --opt_lvl >= 1 are errors, by name, before any step."""
    if fusion_head not in FUSION_HEADS:
        raise ValueError("--fusion_head must be one of %s, got %r" % (FUSION_HEADS, fusion_head))
    if fusion_head == "stock":
        return
    if str(model_name) != "baseline":
        raise ValueError("--fusion_head hip applies to the baseline model (--model baseline), not to %s" % model_name)
    if vgg_train:
        raise ValueError("--fusion_head hip is not available with --vgg_train true: the HIP fusion head has no gradient for the "
                         "image features (a trainable image encoder is out of scope)")
    if opt_lvl > 0:
        raise ValueError("--fusion_head hip is not available with --opt_lvl >= 1 (the reduced-precision mode): the head is "
                         "built in exact fp32 only")


def set_fusion_head(model: nn.Module, fusion_head: str, seed: int = 0) -> None:
    """--fusion_head on a model: ``VQABaselineNet.fusion_impl`` and, for "hip" on a model whose parameters are on the GPU,
    ``fusion_dropout_state`` = a fresh DropoutState(seed) there -- call it after moving the model.  On the CPU the attribute
    is set and the forward takes the stock lines (as --question_gru hip does).  Module attributes, not part of the state_dict.
    A model without a fusion head has nothing to switch: asking for "hip" there is an error, and so is a baseline model whose
    image encoder is trainable."""
    if fusion_head not in FUSION_HEADS:
        raise ValueError("--fusion_head must be one of %s, got %r" % (FUSION_HEADS, fusion_head))
    if not hasattr(model, "fusion_impl"):
        if fusion_head != "stock":
            raise ValueError("--fusion_head hip applies to the baseline model (--model baseline), not to %s"
                             % type(model).__name__)
        return
    if fusion_head == "hip" and any(p.requires_grad for p in model.image_encoder.vgg11_encoder.parameters()):
        raise ValueError("--fusion_head hip is not available with a trainable image encoder (--vgg_train true): the HIP fusion "
                         "head has no gradient for the image features")
    model.fusion_impl = fusion_head
    dev = next(model.parameters()).device
    model.fusion_dropout_state = DropoutState(seed, dev) if fusion_head == "hip" and dev.type == "cuda" else None


def check_dropout(model_name: str, dropout: float, opt_lvl: int = 0) -> None:
    """--dropout P: feature dropout on the six attended features in front of the answer head (dropout.py), 0 = off (the
    default).  P must lie in [0, 1); P > 0 exists for the co-attention models only and not in the reduced-precision mode
    (--opt_lvl >= 1): both are errors."""
    if not 0.0 <= float(dropout) < 1.0:
        raise ValueError("--dropout must be in [0, 1), got %r" % (dropout,))
    if dropout == 0:
        return
    if not str(model_name).startswith("attention"):
        raise ValueError("--dropout applies to the co-attention models (--model attention*), not to %s" % model_name)
    if opt_lvl > 0:
        raise ValueError("--dropout is not available with --opt_lvl >= 1 (the reduced-precision mode)")


FEATURE_MODELS = ("attention", "attention_resnet", "attention_bert")


def check_image_features(args, world: int = 1, validates: bool = False) -> None:
    """--image_features PATH [--val_image_features PATH]: train (validate) from feature tables of the frozen encoder in eval
    mode (features.FeatureTable, written by ``python -m vqa_amd.extract``) instead of running the encoder in the step.
    Refused: a trainable encoder (--vgg_train true: its features change every step), models without a feature grid, a
    validation run (`validates`) without its own table, a validation table without a training table, and a data-parallel run
    (`world` > 1) whose path does not hold ``{rank}`` -- every rank's split has its own seed, so every rank needs its own table."""
    path, val_path = getattr(args, "image_features", None), getattr(args, "val_image_features", None)
    if not path:
        if val_path:
            raise ValueError("--val_image_features needs --image_features (the training table)")
        return
    if getattr(args, "vgg_train", False):
        raise ValueError("--image_features is not available with --vgg_train true: cached features are those of a frozen encoder")
    if args.model not in FEATURE_MODELS:
        raise ValueError("--image_features applies to the co-attention models (--model %s), not to %s: it has no feature grid"
                         % (" | ".join(FEATURE_MODELS), args.model))
    if validates and not val_path:
        raise ValueError("--image_features with a validation run (--val_size / --val_batches) needs --val_image_features: the "
                         "validation split has its own images")
    if world > 1:
        for flag, p in (("--image_features", path), ("--val_image_features", val_path)):
            if p and "{rank}" not in p:
                raise ValueError("%s with WORLD_SIZE = %d needs {rank} in the path: every rank's split has its own seed, so "
                                 "every rank reads its own table" % (flag, world))


PREPROCESS = ("hip", "host")
FILE_FLAGS = {"train": ("train_file", "train_img"), "val": ("val_file", "val_img"), "test": ("test_file", "test_img")}


def check_files(args, split: str = "train", world: int = 1, validates: bool = False) -> None:
    """--synthetic false: the reference's dataset files (vqa_amd.data).  `split`'s data file, its image directory (not needed
    on cached features: no image is opened then) and --vocab_file are required; a validating training run needs --val_file
    (and --val_img) too.  Refused: --loss soft_ce | bce (a line of the text format carries one answer), the BERT models (their
    tokeniser is not offered), data-parallel runs, --preprocess hip without a GPU."""
    cached = bool(getattr(args, "image_features", None))
    needed = [split] + (["val"] if validates and split == "train" else [])
    for s in needed:
        file_flag, img_flag = FILE_FLAGS[s]
        if not getattr(args, file_flag, None):
            raise ValueError("--synthetic false needs --%s (lines of `img_name \\t question \\t answer`)" % file_flag)
        if not cached and not getattr(args, img_flag, None):
            raise ValueError("--synthetic false needs --%s (the image directory of --%s)" % (img_flag, file_flag))
    if not args.vocab_file:
        raise ValueError("--synthetic false needs --vocab_file (python -m vqa_amd.data vocab, or the reference's prepare_data.py)")
    if args.loss != "ce":
        raise ValueError("--loss %s needs soft answer targets; the data files carry one answer per line: use --loss ce" % args.loss)
    if args.model in ("bert", "attention_bert"):
        raise ValueError("--model %s reads BERT token ids; the BERT tokeniser is not offered with file data" % args.model)
    if world > 1:
        raise ValueError("file data with WORLD_SIZE = %d: data-parallel runs are offered on synthetic data only" % world)
    pre = getattr(args, "preprocess", None)
    if pre not in (None,) + PREPROCESS:
        raise ValueError("--preprocess must be one of %s, got %r" % (PREPROCESS, pre))
    if pre == "hip" and not torch.cuda.is_available():
        raise ValueError("--preprocess hip runs on the GPU (there is no CPU fallback); use --preprocess host")


def file_vocab(args) -> dict:
    """The vocabulary of --vocab_file; args.vocab_size and args.max_seq_length become its values, and its label table must
    have --num_cls + 1 entries (UNKNOWN and the K answers): the model is built from these."""
    from . import data as D
    vocab = D.load_vocab(args.vocab_file)
    if len(vocab["label2idx"]) != args.num_cls + 1:
        raise ValueError("%s holds %d labels (UNKNOWN included); --num_cls %d needs %d" % (args.vocab_file, len(vocab["label2idx"]),
                                                                                          args.num_cls, args.num_cls + 1))
    args.vocab_size, args.max_seq_length = len(vocab["word2idx"]), int(vocab["max_seq_length"])
    return vocab


def file_dataset(args, split: str, vocab: dict):
    """`split`'s VQAFileDataset: pixels, or table rows on cached features."""
    from . import data as D
    file_flag, img_flag = FILE_FLAGS[split]
    return D.VQAFileDataset(getattr(args, file_flag), getattr(args, img_flag, None), vocab,
                            images="row" if getattr(args, "image_features", None) else "pixels")


def file_loader(ds, args, shuffle: bool, seed: int = 0, drop_last: bool = False):
    from . import data as D
    return torch.utils.data.DataLoader(ds, args.batch_size, shuffle=shuffle, drop_last=drop_last, num_workers=args.num_workers,
                                       collate_fn=D.collate, generator=torch.Generator().manual_seed(seed) if shuffle else None)


class FileImages:
    """What turns a batch's decoded images into the network's input: --preprocess hip (the default on a GPU) packs them for
    ``ImagePreprocessor`` -- the launch itself is queued by whoever copies the batch (DevicePrefetcher, or ``device()`` here)
    --, --preprocess host resizes and normalises on the CPU (``preprocess_host``)."""

    def __init__(self, args, size: int, device, mean=None, std=None):
        from . import preprocess as PP
        self.mode = getattr(args, "preprocess", None) or ("hip" if device.type == "cuda" else "host")
        self.size, self.device = int(size), device
        self.mean, self.std = tuple(mean or PP.IMAGENET_MEAN), tuple(std or PP.IMAGENET_STD)
        self.hip = PP.ImagePreprocessor(self.size, self.mean, self.std, device) if self.mode == "hip" else None

    def host(self, images):
        """A list of uint8 arrays -> a PackedBatch (hip) or the fp32 tensor (host); tensors (table rows) pass through."""
        if torch.is_tensor(images):
            return images
        if self.hip is not None:
            return self.hip.pack(images)
        from .preprocess import preprocess_host
        return preprocess_host(images, self.size, self.mean, self.std)

    def device_images(self, image, channels_last: bool = False):
        """What ``host`` returned -> the fp32 [B, 3, S, S] tensor on the device, on the current stream."""
        if torch.is_tensor(image):
            image = image.to(self.device)
            return image.contiguous(memory_format=torch.channels_last) if channels_last and image.dim() == 4 else image
        return self.hip(image, channels_last=channels_last)


def build_model(model_name: str, vocab_size: int, num_cls: int, question_mask: bool = False, affinity: str = "reference",
                co_attention: str = "parallel", **kw) -> nn.Module:
    """K + 1 output classes: index 0 is UNKNOWN (main.py:155).  question_mask: see `set_question_mask`; affinity: see
    `check_affinity`; co_attention: see `check_co_attention`."""
    check_affinity(model_name, affinity)
    check_co_attention(model_name, co_attention, affinity)
    cfg = setup_model_configs(model_name, vocab_size, **kw)
    model = cfg["model"](cfg["question_params"], cfg["image_params"], K=num_cls + 1, **_net_kwargs(co_attention))
    set_question_mask(model, question_mask)
    set_affinity(model, affinity)
    return model


def model_from_args(args):
    """The model of a parsed command line, as main.py:388 builds it: (model, registry entry).  attention_bert: the token ids
    are BERT's, so args.vocab_size becomes BERT's vocabulary.  --question_mask is applied to the co-attention (the Trainer's
    steps and `validate` then pass the lengths through), --affinity likewise.  (train.main, predict.main)"""
    affinity = getattr(args, "affinity", "reference")
    check_affinity(args.model, affinity, getattr(args, "opt_lvl", 0))
    check_dropout(args.model, getattr(args, "dropout", 0.0), getattr(args, "opt_lvl", 0))
    check_fusion_head(args.model, getattr(args, "fusion_head", "stock"), getattr(args, "vgg_train", False), getattr(args, "opt_lvl", 0))
    co_attention = getattr(args, "co_attention", "parallel")
    check_co_attention(args.model, co_attention, affinity, getattr(args, "opt_lvl", 0), getattr(args, "precision", "exact"))
    cfg = setup_model_configs(args, args.vocab_size)             # (as main.py:388)
    args.vocab_size = cfg.get("vocab_size", args.vocab_size)
    model = cfg["model"](cfg["question_params"], cfg["image_params"], K=args.num_cls + 1, **_net_kwargs(co_attention))
    set_question_mask(model, getattr(args, "question_mask", False))
    set_affinity(model, affinity)
    set_sentence_lstm(model, getattr(args, "sentence_lstm", "stock"))
    set_question_gru(model, getattr(args, "question_gru", "stock"))
    if getattr(args, "fusion_head", "stock") != "stock":        # (the dropout state: Trainer, once the model is on its device)
        model.fusion_impl = args.fusion_head
    set_word_embedding(model, getattr(args, "word_embedding", "stock"))
    return model, cfg


def log_dir_of(args):
    """expt_dir/expt_name/run_name (main.py:110-114), or None without --expt_dir."""
    return os.path.join(args.expt_dir, args.expt_name, args.run_name) if args.expt_dir else None


def checkpoint_path(args):
    """--model_ckpt as a path: a relative name that exists inside the log directory is taken from there (main.py:169)."""
    ckpt = args.model_ckpt
    log_dir = log_dir_of(args)
    if ckpt and log_dir and not os.path.isabs(ckpt) and os.path.exists(os.path.join(log_dir, ckpt)):
        ckpt = os.path.join(log_dir, ckpt)
    return ckpt


def set_products(model: nn.Module, precision: str) -> None:
    """Width of the HIP path's fp32 products on every module that has the switch: "fast" = the tolerance mode."""
    fast = precision == "fast"
    co = getattr(model, "co_attention", None)
    if co is not None and hasattr(co, "fast_products"):
        co.fast_products = fast
    for m in model.modules():
        if m is not co and hasattr(m, "fast_products"):
            m.fast_products = fast


def set_reduced_precision(model: nn.Module, opt_lvl: int) -> None:
    """--opt_lvl >= 1 (AMP): the co-attention projections and the answer head on the bf16 MFMA as well."""
    if opt_lvl > 0 and hasattr(model, "co_attention"):
        model.co_attention.bf16_projections = True
        if hasattr(getattr(model, "mlp_classify", None), "bf16_products"):
            model.mlp_classify.bf16_products = True


def autocast_for(opt_lvl: int, device):
    """bf16 autocast around the stock encoders for --opt_lvl >= 1 on the GPU, else nothing."""
    if opt_lvl > 0 and device.type == "cuda":
        return torch.autocast("cuda", dtype=torch.bfloat16)
    return contextlib.nullcontext()


def sort_batch(images, questions, answers, ques_seq_lens, *extras):
    """Descending by question length, as packing requires (utils.py:33-45).  `extras` (e.g. the soft answer targets
    `answers`, `answer_scores` of a batch) are reordered alike and appended to the result."""
    ques_seq_lens, order = ques_seq_lens.sort(dim=0, descending=True)
    return (images[order], questions[order], answers[order], ques_seq_lens, *[e[order] for e in extras])


LOSSES = ("ce", "soft_ce", "bce")
ANSWER_SCORES = (0.3, 0.6, 0.9, 1.0)      # min(1, n / 3) for n = 1, 2, 3, >= 4 humans, as VQA v2's annotations are commonly scored


def check_loss(loss: str, num_answers: int = 10) -> None:
    """--loss: "ce" (the default: the reference's nn.CrossEntropyLoss on the majority answer), "soft_ce" or "bce" on the soft
    answer targets (loss.soft_target_loss); --num_answers: answer slots per sample, 1..16."""
    if loss not in LOSSES:
        raise ValueError("--loss must be one of %s, got %r" % (LOSSES, loss))
    if not 1 <= int(num_answers) <= 16:
        raise ValueError("--num_answers must be in 1..16, got %r" % (num_answers,))


OPTIMIZERS = ("torch", "hip")


def check_optimizer(optimizer: str, weight_decay: float = 0.0, clip_grad_norm=None) -> None:
    """--optimizer: "torch" (the default: the reference's torch.optim.Adam, main.py:180, untouched) or "hip" (optim.HipAdam: the
    fused HIP step).  --weight_decay (decoupled, AdamW) and --clip_grad_norm (global norm) exist on the HIP step only: the stock
    path stays what it is and does not grow a second implementation."""
    if optimizer not in OPTIMIZERS:
        raise ValueError("--optimizer must be one of %s, got %r" % (OPTIMIZERS, optimizer))
    if weight_decay < 0:
        raise ValueError("--weight_decay must be non-negative, got %r" % (weight_decay,))
    if clip_grad_norm is not None and not clip_grad_norm > 0:
        raise ValueError("--clip_grad_norm must be positive, got %r" % (clip_grad_norm,))
    if optimizer == "torch" and (weight_decay != 0 or clip_grad_norm is not None):
        raise ValueError("--weight_decay / --clip_grad_norm need --optimizer hip (the stock Adam path takes neither)")


def synthetic_answers(labels: torch.Tensor, num_answers: int, num_classes: int, seed: int):
    """Soft answer targets for `labels` (shape [...]): answers int32 [..., A] and answer_scores fp32 [..., A].  Slot 0 is
    (label, 1.0); every further slot is empty (-1) with probability 1/3, else a class U{0..num_classes-1} with a score from
    ANSWER_SCORES.  Drawn from a generator of its OWN (seeded by `seed`), so that asking for answers changes no bit of the
    image, question, length or label of any seed."""
    g = torch.Generator().manual_seed((seed * 2654435761 + 97) % (2 ** 63))
    shape = tuple(labels.shape) + (num_answers,)
    idx = torch.randint(0, num_classes, shape, generator=g)
    empty = torch.randint(0, 3, shape, generator=g) == 0
    score = torch.tensor(ANSWER_SCORES)[torch.randint(0, len(ANSWER_SCORES), shape, generator=g)]
    idx = torch.where(empty, torch.full_like(idx, -1), idx)
    score = torch.where(empty, torch.zeros_like(score), score)
    idx[..., 0] = labels
    score[..., 0] = 1.0
    return idx.to(torch.int32), score.to(torch.float32)


def synthetic_batch(batch_size: int, image_size, max_seq_len: int, vocab_size: int, num_classes: int,
                    seed: int, num_answers: int = 0) -> Dict[str, torch.Tensor]:
    """One batch shaped like VQADataset's output (dataloader.py:72): images N(0,1), token ids
    U{2..vocab-1} zero-padded to max_seq_len, lengths U{3..max} with at least one full-length
    question, labels U{0..num_classes-1}.  CPU tensors; lengths are NOT sorted (sort_batch does).
    num_answers = A > 0: also `answers` int32 [B,A] and `answer_scores` fp32 [B,A] (synthetic_answers; the other four keys
    keep their bits)."""
    g = torch.Generator().manual_seed(seed)
    H, W = image_size
    image = torch.randn(batch_size, 3, H, W, generator=g)
    lens = torch.randint(min(3, max_seq_len), max_seq_len + 1, (batch_size,), generator=g)
    lens[int(torch.randint(0, batch_size, (1,), generator=g))] = max_seq_len
    question = torch.randint(2, vocab_size, (batch_size, max_seq_len), generator=g)
    question = question * (torch.arange(max_seq_len)[None, :] < lens[:, None])
    label = torch.randint(0, num_classes, (batch_size,), generator=g)
    out = {"image": image, "question": question, "ques_len": lens, "label": label}
    if num_answers:
        out["answers"], out["answer_scores"] = synthetic_answers(label, num_answers, num_classes, seed)
    return out


class DevicePrefetcher:
    """Host -> device hand-off of the following batches while the current step computes
    (main.py:205-208 copies synchronously).  A worker thread pulls batches from the host iterator,
    stages them in pinned buffers (a ring of two sets, reused once their copy has completed) and queues
    the copies on a side stream; the consumer stream waits on the copy's event before it touches the
    tensors.  Lengths stay on the host (packing).  At most `depth` batches are in flight."""

    _END = object()

    def __init__(self, batches, device, channels_last: bool = False, depth: int = 2, preprocess=None):
        self.device = device
        self.cl = channels_last
        # file data (--preprocess hip): a batch's `image` is a preprocess.PackedBatch of decoded pixels; its bytes go through
        # the pinned ring, and `preprocess` (an ImagePreprocessor) queues its one launch on the side stream behind the copy
        self.preprocess = preprocess
        self.next = None
        if device.type != "cuda":
            self._it = iter(batches)
            self._q = None
            self._advance()
            return
        import queue
        import threading
        self.stream = torch.cuda.Stream(device)
        self._q = queue.Queue(maxsize=max(1, depth))
        self._err = None
        self._thread = threading.Thread(target=self._worker, args=(iter(batches),), daemon=True)
        self._thread.start()
        self._advance()

    def _worker(self, it):
        try:
            torch.cuda.set_device(self.device)
            ring = [{}, {}]                                       # pinned staging buffers + their last copy event
            for i, (image, question, ques_len, label, *extras) in enumerate(it):
                slot = ring[i & 1]
                if slot.get("event") is not None:
                    slot["event"].synchronize()                  # the previous copy out of this set is done

                def pin(name, t):
                    buf = slot.get(name)
                    if buf is None or buf.shape != t.shape or buf.dtype != t.dtype:
                        buf = torch.empty(t.shape, dtype=t.dtype).pin_memory()
                        slot[name] = buf
                    buf.copy_(t)
                    return buf

                def pin_bytes(name, t):                         # a 1-D buffer whose length differs batch to batch: grow only
                    buf = slot.get(name)
                    if buf is None or buf.numel() < t.numel():
                        buf = torch.empty(max(t.numel(), 2 * buf.numel() if buf is not None else 0), dtype=t.dtype).pin_memory()
                        slot[name] = buf
                    buf[:t.numel()].copy_(t)
                    return buf[:t.numel()]

                with torch.cuda.stream(self.stream):
                    if torch.is_tensor(image):
                        im = pin("image", image).to(self.device, non_blocking=True)
                        if self.cl:
                            im = im.contiguous(memory_format=torch.channels_last)
                    else:
                        packed = image.with_buf(pin_bytes("pixels", image.buf).to(self.device, non_blocking=True))
                        im = self.preprocess.launch(packed, channels_last=self.cl)
                    qu = pin("question", question).to(self.device, non_blocking=True)
                    la = pin("label", label).to(self.device, non_blocking=True)
                    ex = [pin("extra%d" % j, e).to(self.device, non_blocking=True) for j, e in enumerate(extras)]
                    ev = torch.cuda.Event()
                    ev.record(self.stream)
                slot["event"] = ev
                self._q.put((im, qu, ques_len, la, ev, *ex))
        except BaseException as e:                                # surfaced in the consumer thread
            self._err = e
        finally:
            self._q.put(self._END)

    def _advance(self):
        if self._q is None:
            try:
                image, question, ques_len, label, *extras = next(self._it)
                self.next = (image, question, ques_len, label, None, *extras)
            except StopIteration:
                self.next = None
            return
        item = self._q.get()
        if item is self._END:
            self.next = None
            if self._err is not None:
                raise self._err
        else:
            self.next = item

    def __iter__(self):
        return self

    def peek_image(self):
        """(image, copy-done event) of the batch the next __next__ will return, (None, None) at the
        end: lets the consumer queue work on that image on another stream behind the event."""
        if self.next is None:
            return None, None
        return self.next[0], self.next[4]

    def __next__(self):
        if self.next is None:
            raise StopIteration
        im, qu, ln, la, ev, *extras = self.next          # (extras: the soft answer targets, when the batches carry them)
        if ev is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            for t in (im, qu, la, *extras):
                t.record_stream(cur)
        self._advance()
        return (im, qu, ln, la, *extras)


class Trainer:
    """Owns model, Adam (lr, PyTorch defaults: main.py:180), loss and the gradient reducer.

    optimizer="torch" (default) is exactly ``torch.optim.Adam(model.parameters(), lr)``; optimizer="hip" is ``optim.HipAdam``
    -- the same arithmetic in one HIP launch on the step's stream -- and is what `weight_decay` (decoupled, AdamW) and
    `clip_grad_norm` (by the global norm of the averaged gradients: it runs behind the reducer; the norm of the last step stays
    on the device as ``trainer.optimizer.grad_norm``) need.

    feature_dropout=P > 0 (with dropout_seed): dropout on the attended features in front of the answer head, CUDA and
    opt_lvl 0 only (modules.set_feature_dropout; masks from dropout_seed + rank, nothing taken from torch's generators).

    Encoder run-ahead: when the image encoder is frozen (the reference default, main.py:67 /
    model.py:239-241) its output does not depend on the optimiser state, so ``step(...,
    next_image=...)`` launches the stock encoder for the NEXT batch on a second, high-priority HIP
    stream before it queues this step's own work.  The long MIOpen convolutions then overlap the
    many short, latency-bound kernels of the question encoder / co-attention / MLP / backward / Adam
    (and the RCCL all-reduce) instead of running in series with them.  Values are unchanged: the same
    modules see the same tensors, BatchNorm running statistics are updated in batch order on that
    stream."""

    def __init__(self, model: nn.Module, lr: float = 1e-4, device=None, opt_lvl: int = 0,
                 bucket_mb: float = 16.0, encoder_runahead: bool = True, graph: bool = False, static_hot_path: bool = True,
                 precision: str = "exact", loss: str = "ce", optimizer: str = "torch", weight_decay: float = 0.0,
                 clip_grad_norm=None, sentence_lstm=None, word_embedding=None, feature_dropout: float = 0.0,
                 dropout_seed: int = 0, encoder_eval=None, question_gru=None, fusion_head=None):
        check_loss(loss)
        if fusion_head is not None:                              # "stock" | "hip" (set_fusion_head); None: leave the model's
            if fusion_head == "hip" and opt_lvl > 0:
                raise ValueError("Trainer(fusion_head='hip') is not available with opt_lvl >= 1 (the reduced-precision mode)")
            set_fusion_head(model, fusion_head, rank_seed(dropout_seed, vdist.rank()))
        if question_gru is not None:                             # "stock" | "hip" (set_question_gru); None: leave the model's
            set_question_gru(model, question_gru)
        if encoder_eval is not None:                             # "stock" | "hip" (set_encoder_eval); None: leave the model's
            dev = device or next(model.parameters()).device
            if encoder_eval == "hip" and torch.device(dev).type != "cuda":
                raise ValueError("Trainer(encoder_eval='hip') needs a model on the GPU (the kernels have no CPU form)")
            if encoder_eval == "hip" and opt_lvl > 0:
                raise ValueError("Trainer(encoder_eval='hip') is not available with opt_lvl >= 1 (the reduced-precision mode)")
            set_encoder_eval(model, encoder_eval)
        if word_embedding is not None:                           # "stock" | "hip" (set_word_embedding); None: leave the model's
            set_word_embedding(model, word_embedding)
        if sentence_lstm is not None:                            # "stock" | "hip" (set_sentence_lstm); None: leave the model's
            set_sentence_lstm(model, sentence_lstm)
        check_optimizer(optimizer, weight_decay, clip_grad_norm)
        self.loss = loss                                         # "ce": int64 labels; "soft_ce" | "bce": step(..., targets=...)
        self.device = device or next(model.parameters()).device
        if feature_dropout:                                      # (refused before anything of the model is switched)
            if self.device.type != "cuda":
                raise ValueError("Trainer(feature_dropout > 0) needs a model on the GPU (the dropout has no CPU fallback)")
            if opt_lvl > 0:
                raise ValueError("Trainer(feature_dropout > 0) is not available with opt_lvl >= 1 (the reduced-precision mode)")
        self.model = model
        # Precision of the HIP path's fp32 products (include/coattn.h "Widths of the fp32 mode"): "exact" -- the default, the
        # reference's arithmetic (main.py --opt_lvl 0) -- is fp32-accurate products over fp32's range, the modules' and the
        # C-ABI's own default; "fast" is the opt-in tolerance mode (forward products on two FP16 pieces = 22 significand
        # bits, backward on two bf16 pieces = 16; inside the reference contract of 1e-4 for operands below 65,504 in
        # magnitude; every forward there folds its range report into a sticky accumulator, and check_range() -- called where
        # the loss is read -- falls back to exact when ANY step since the last check left the range).
        if precision not in ("fast", "exact"):
            raise ValueError("precision must be 'fast' or 'exact'")
        self.set_precision(precision)
        self.criterion = CrossEntropyLoss()      # nn.CrossEntropyLoss() semantics (main.py:94); fused HIP kernel on CUDA
        self.soft_criterion = SoftTargetLoss(loss) if loss != "ce" else None
        if optimizer == "hip":
            if self.device.type != "cuda":
                raise ValueError("Trainer(optimizer='hip') needs a model on the GPU (HipAdam has no CPU fallback)")
            from .optim import HipAdam
            self.optimizer = HipAdam(model.parameters(), lr, weight_decay=weight_decay, max_grad_norm=clip_grad_norm)
        else:
            self.optimizer = torch.optim.Adam(model.parameters(), lr)
        self.opt_lvl = opt_lvl
        set_reduced_precision(model, opt_lvl)                    # AMP: projections on the bf16 MFMA as well
        # feature_dropout > 0: dropout on the attended features in front of the answer head (dropout.py), its masks drawn on the
        # device from (dropout_seed + rank, step): data-parallel ranks draw different masks, torch's generators are not touched.
        # 0 (the default) leaves the model as it is.  The step counter is not part of a checkpoint.
        if feature_dropout:
            set_feature_dropout(model, feature_dropout, rank_seed(dropout_seed, vdist.rank()))
        # graph=True: co-attention + answer head + loss, forward and backward, replayed from one captured HIP graph
        # (graph.py): one host call instead of ~25 launches; same values bit for bit
        if graph and hasattr(model, "hot_path_graph") and self.device.type == "cuda":
            model.hot_path_graph = True
        self.reducer = vdist.GradReducer(model, bucket_mb=bucket_mb) if vdist.world_size() > 1 else None
        # Default on CUDA: the hot path as one autograd node over static buffers, calls issued eagerly (graph.py,
        # capture=False): half the host time of the module-by-module path, no graph-node gaps.  This trainer owns the step
        # (zero_grad -> backward -> optimiser), so the static gradient buffers may become param.grad directly -- unless a
        # gradient reducer needs autograd's post-accumulate hooks to fire (data-parallel runs).
        # VQA_HOT_PATH=modules restores the module-by-module path.
        if (static_hot_path and hasattr(model, "hot_path_static") and self.device.type == "cuda"
                and os.environ.get("VQA_HOT_PATH", "static") != "modules"):
            model.hot_path_static = True
            model.hot_path_direct_grads = self.reducer is None
        enc = getattr(model, "image_encoder", None)
        self.runahead = bool(encoder_runahead and self.device.type == "cuda" and enc is not None
                             and hasattr(model, "forward_features")
                             and not any(p.requires_grad for p in enc.parameters()))
        self.enc_stream = (torch.cuda.Stream(self.device, priority=int(os.environ.get("VQA_ENC_PRIORITY", "-1")))
                           if self.runahead else None)
        self._ahead = None                                       # (image, features, event) of the next batch
        self._resident = None                                    # last image batch consumed on the device

    def _autocast(self):
        return autocast_for(self.opt_lvl, self.device)

    def _queue_encoder(self, image, ready=None):
        """Queue the frozen image encoder for `image` on the encoder stream; returns (image, features,
        done-event).  `ready`: event after which `image` is valid (None: valid once the work queued on
        the current stream so far is done; nothing to wait for if the batch is the one just consumed).
        The encoder stream takes no other dependency on the step, so consecutive passes run back to back."""
        if ready is not None:
            self.enc_stream.wait_event(ready)
        elif image is not self._resident:
            self.enc_stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.enc_stream), torch.no_grad(), self._autocast():
            feats = self.model.image_encoder(image)
            ev = torch.cuda.Event()
            ev.record(self.enc_stream)
        image.record_stream(self.enc_stream)
        return image, feats, ev

    def _claim(self, queued):
        """Hand features queued on the encoder stream to the current stream (which waits for them here)."""
        _, feats, ev = queued
        main = torch.cuda.current_stream(self.device)
        main.wait_event(ev)
        feats.record_stream(main)
        return feats

    def step(self, image, question, ques_len, label, next_image=None, next_ready=None, targets=None) -> torch.Tensor:
        """One optimisation step on device-resident, length-sorted tensors; returns the loss.
        `next_image`: the following step's image batch (device-resident), if known; `next_ready`: the
        event that marks its host->device copy complete (DevicePrefetcher.peek_image).
        `targets` = (ans_idx int32 [B,A], ans_score fp32 [B,A]): what a Trainer(loss="soft_ce" | "bce") trains against
        (`label` is then not read); a Trainer(loss="ce") takes none."""
        if (targets is not None) != (self.loss != "ce"):
            raise ValueError("Trainer(loss=%r).step: %s" % (self.loss, "targets=(ans_idx, ans_score) needed" if targets is None
                                                           else "takes labels, not targets"))
        tk = dict(labels=label) if targets is None else dict(targets=tuple(targets), loss_kind=self.loss)
        if self.runahead:
            with self._autocast():
                mine, self._ahead = self._ahead, None
                if mine is not None and mine[0] is not image:
                    # queued for some other batch: drop it -- but its pass may still be running on the encoder stream
                    # and updates the same BatchNorm running statistics as the inline pass below: wait for it
                    torch.cuda.current_stream(self.device).wait_stream(self.enc_stream)
                    mine = None
                if mine is None:
                    with torch.no_grad():
                        inline = self.model.image_encoder(image)
                    # the inline pass updated the BatchNorm running statistics on this stream: the pass queued
                    # below for the next batch must come after it (batch order)
                    self.enc_stream.wait_stream(torch.cuda.current_stream(self.device))
                self._resident = image
                if next_image is not None:
                    self._ahead = self._queue_encoder(next_image, next_ready)
                # the question side is queued before the current stream waits for the image features; the loss comes
                # out of the answer head's own call (main.py:211 + :214 in one)
                logits, loss = self.model.forward_features((lambda: self._claim(mine)) if mine is not None else inline,
                                                           question, ques_len, **tk)
        else:
            with self._autocast():
                logits = self.model(image, question, ques_len)
            loss = self.criterion(logits.float(), label) if targets is None else self.soft_criterion(logits.float(), *targets)
        self.optimizer.zero_grad()
        if self.reducer is not None:
            self.reducer.prepare()
        loss.backward()
        if self.reducer is not None:
            self.reducer.finish()
        self.optimizer.step()
        return loss

    def step_features(self, features, question, ques_len, label, targets=None) -> torch.Tensor:
        """One optimisation step from already-encoded image features [B, N, d] (fp32, device-resident: the rows
        ``features.gather_features`` takes from a feature table) -- the body of `step` from ``forward_features`` on.  The
        image encoder is never called, so nothing runs ahead and its BatchNorm statistics stay as they are; the loss, the
        backward, the gradient reducer and the optimiser are `step`'s."""
        if (targets is not None) != (self.loss != "ce"):
            raise ValueError("Trainer(loss=%r).step_features: %s" % (self.loss, "targets=(ans_idx, ans_score) needed"
                                                                    if targets is None else "takes labels, not targets"))
        if not hasattr(self.model, "forward_features"):
            raise ValueError("step_features needs a co-attention model (forward_features); %s has no feature grid"
                             % type(self.model).__name__)
        tk = dict(labels=label) if targets is None else dict(targets=tuple(targets), loss_kind=self.loss)
        with self._autocast():
            logits, loss = self.model.forward_features(features, question, ques_len, **tk)
        self.optimizer.zero_grad()
        if self.reducer is not None:
            self.reducer.prepare()
        loss.backward()
        if self.reducer is not None:
            self.reducer.finish()
        self.optimizer.step()
        return loss

    def set_precision(self, precision: str) -> None:
        self.precision = precision
        set_products(self.model, precision)

    def check_range(self) -> bool:
        """Tolerance mode only: True if every operand of EVERY forward since the last check lay inside the FP16-piece range
        (the report is sticky: each tolerance-mode forward folds its status words into a per-device accumulator,
        _lib.fold_range).  If one did not (its pieces were clamped: that step's values were off, and the Adam updates made
        since are NOT rolled back), warn, switch this trainer to the exact mode for the following steps and return False.
        Data-parallel runs decide together: the flag is MAX-reduced over the group, so every rank switches in the same
        step.  Synchronises -- call it where the loss is read on the host."""
        if self.device.type != "cuda" or self.precision != "fast" or self.opt_lvl > 0:
            return True
        from . import _lib
        msg = None
        try:
            _lib.check_range()
        except _lib.RangeError as e:
            msg = str(e)
        bad = msg is not None
        if vdist.world_size() > 1:
            flag = torch.tensor([1.0 if bad else 0.0], device=self.device)
            torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MAX)
            if float(flag) > 0 and not bad:
                bad, msg = True, "another rank reported an operand outside the FP16-piece range"
        if bad:
            import warnings
            warnings.warn("vqa_amd.Trainer: %s -- continuing in the exact mode (steps since the last check ran on clamped "
                          "pieces and are not rolled back)" % msg)
            self.set_precision("exact")
            return False
        return True

    def check_labels(self) -> None:
        """Raise IndexError if a label of the last step lay outside [0, K) (the asynchronous HIP loss only sets a status
        word where nn.CrossEntropyLoss raises); synchronises -- call it where the loss is read on the host."""
        if self.device.type == "cuda":
            from . import head, loss
            head.check_labels()
            loss.check_labels()

    @torch.no_grad()
    def validate(self, batches, features: bool = False) -> Dict[str, float]:
        """Accuracy / mean CE under eval() (main.py:290-351, without its n_iters+1 / n_iters slip).
        With encoder run-ahead, an encoder pass queued for the next training batch is waited for first
        (its BatchNorm running-statistics update is then already included, i.e. one batch earlier than
        in the serial schedule); pass next_image=None on the step before validating to avoid that.
        Batches are (image, question, ques_len, label) or, with soft answer targets, (..., label, ans_idx, ans_score): the
        dict then gains `vqa_score` (the mean of min(1, t[pred]) over all samples, in [0, 1]: with one-hot targets it is
        `accuracy` / 100; on the GPU through coattn_vqa_score, summed on the device and read once), and `loss` is this trainer's own loss kind.
        features=True: the first element of a batch is the encoded image features [B, N, d] (the rows of a feature table),
        handed to ``model.forward_features``; the image encoder is not called."""
        if features and not hasattr(self.model, "forward_features"):
            raise ValueError("validate(features=True) needs a co-attention model (forward_features); %s has no feature grid"
                             % type(self.model).__name__)
        if self.enc_stream is not None:
            torch.cuda.current_stream(self.device).wait_stream(self.enc_stream)
        self.model.eval()
        n_ok = n = 0
        loss = 0.0
        score = None
        for image, question, ques_len, label, *targets in batches:
            logits = (self.model.forward_features(image, question, ques_len) if features
                      else self.model(image, question, ques_len))
            if self.loss != "ce":
                if not targets:
                    raise ValueError("Trainer(loss=%r).validate: the batches carry no answer targets" % self.loss)
                loss += float(self.soft_criterion(logits.float(), *targets))
            else:
                loss += float(self.criterion(logits.float(), label))
            n_ok += int((logits.argmax(1) == label).sum())
            n += label.numel()
            if targets:
                from . import loss as _loss
                if logits.is_cuda:
                    part = _loss.vqa_score_sum(logits.float(), *targets, row_score=False)[2]
                else:
                    part = _loss.vqa_score(logits.float(), *targets)[1].sum()
                score = part if score is None else score + part
        self.model.train()
        out = {"accuracy": 100.0 * n_ok / max(n, 1), "loss": loss / max(len(batches), 1)}
        if score is not None:
            out["vqa_score"] = float(score) / max(n, 1)          # (the one host read of the scores)
        return out


class SyntheticVQADataset(torch.utils.data.Dataset):
    """Samples shaped like VQADataset's (dataloader.py:72: {'image','question','ques_len','label'}) drawn from a seed per
    index: images N(0,1), token ids U{2..vocab-1} zero-padded to max_seq_len, lengths U{3..max}, labels U{0..K}.  Stands
    in for the dataset files this environment does not have; feeds the same DataLoader(batch_size, shuffle, drop_last,
    num_workers) as main.py:129-130."""

    def __init__(self, n_samples, image_size, max_seq_len, vocab_size, num_classes, seed, num_answers: int = 0,
                 images: bool = True):
        self.n, self.size, self.T, self.vocab, self.K, self.seed = n_samples, image_size, max_seq_len, vocab_size, num_classes, seed
        self.A = num_answers          # > 0: samples also carry `answers` int32 [A], `answer_scores` fp32 [A] (synthetic_answers)
        # images=False (a run on cached image features): the `image` slot carries the sample's index i -- the row of the feature
        # table -- and no image.  The label is drawn after the image from the same generator, so the image is still drawn, once
        # per index: the rest of the sample is kept and later epochs do not pay again.  Every other key keeps its bits.
        self.images = images
        self._memo = {}

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if not self.images:
            out = self._memo.get(i)
            if out is None:
                out = self._memo[i] = self._draw(i)
                out["image"] = torch.tensor(i, dtype=torch.int64)
            return dict(out)
        return self._draw(i)

    def _draw(self, i):
        g = torch.Generator().manual_seed(self.seed * 1000003 + i)
        n = int(torch.randint(min(3, self.T), self.T + 1, (1,), generator=g))
        q = torch.randint(2, self.vocab, (self.T,), generator=g) * (torch.arange(self.T) < n)
        out = {"image": torch.randn(3, *self.size, generator=g), "question": q, "ques_len": torch.tensor(n),
               "label": torch.randint(0, self.K, (), generator=g)}
        if self.A:
            out["answers"], out["answer_scores"] = synthetic_answers(out["label"], self.A, self.K, self.seed * 1000003 + i)
        return out


def build_parser():
    """The reference's command line (main.py:34-78; same names, types and meanings) plus what it lacks here: synthetic
    data, precision, data-parallel launch through the environment.  The dataset / vocabulary flags are the reference's and
    are read with --synthetic false (check_files); --synthetic true, the default, needs none of them."""
    ap = argparse.ArgumentParser(description="Visual Question Answering (MI355X co-attention path)")
    # Experiment params (main.py:37-41; not `required` here: synthetic runs need no directory)
    ap.add_argument("--mode", default="train", choices=["train", "test"])
    ap.add_argument("--expt_dir", type=str, default=None, help="root directory to save model & summaries")
    ap.add_argument("--expt_name", type=str, default="expt")
    ap.add_argument("--run_name", type=str, default="run")
    ap.add_argument("--model", default="attention", choices=["baseline", "attention", "bert", "attention_resnet", "attention_bert"])
    # Data params (main.py:44-48)
    ap.add_argument("--train_img", type=str, default=None)
    ap.add_argument("--train_file", type=str, default=None)
    ap.add_argument("--val_img", type=str, default=None)
    ap.add_argument("--val_file", type=str, default=None)
    ap.add_argument("--num_cls", "-K", type=int_min_two, default=1000)
    ap.add_argument("--vocab_file", type=str, default=None)
    # Training params (main.py:54-59)
    ap.add_argument("--batch_size", "-bs", type=int, default=8)
    ap.add_argument("--num_epochs", "-ep", type=int, default=1,
                    help="number of epochs (the reference's default is 50; an epoch here is --num_steps synthetic batches)")
    ap.add_argument("--learning_rate", "-lr", type=float, default=1e-4)
    ap.add_argument("--log_interval", type=int, default=10, help="interval size for logging training summaries")
    ap.add_argument("--save_interval", type=int, default=3000, help="save model after `n` weight update steps (main.py:260-263)")
    ap.add_argument("--val_size", type=int, default=0,
                    help="validation set size for evaluating accuracy (samples; the reference's default is 10000; 0 = no "
                         "validation: there is no --val_file here, the samples are synthetic)")
    ap.add_argument("--K_eval", type=int, default=1000)
    # Model params (main.py:65-67)
    ap.add_argument("--model_ckpt", type=str, default=None, help="resume training; e.g. model_1000.pth (inside the log directory, or a path)")
    ap.add_argument("--vgg_wts_path", type=str, default=None)
    ap.add_argument("--vgg_train", type=str2bool, default="false")
    # GPU params (main.py:72-73)
    ap.add_argument("--gpu_id", type=int, default=0, help="cuda:gpu_id of a single-process run (under a launcher LOCAL_RANK decides)")
    ap.add_argument("--opt_lvl", type=int, default=0, choices=[0, 1, 2, 3],
                    help="0 = fp32 (the parity mode; the reference's default is apex O1, which is CUDA-only); >= 1: bf16 autocast")
    # Misc params (main.py:76)
    ap.add_argument("--num_workers", type=int, default=0, help="number of worker processes of the DataLoader")
    # --- this build ---
    ap.add_argument("--num_steps", type=int, default=20, help="synthetic batches per epoch")
    ap.add_argument("--precision", default="exact", choices=["fast", "exact"],
                    help="fp32 products of the HIP path: fp32-accurate (default: the reference's --opt_lvl 0 arithmetic) or the "
                         "opt-in tolerance mode (include/coattn.h COATTN_FLAG_FAST16; range-checked at every --log_interval)")
    ap.add_argument("--synthetic", type=str2bool, default="true",
                    help="synthetic data (the default); false: the reference's dataset files -- --train_file / --train_img / "
                         "--vocab_file [--val_file / --val_img], see vqa_amd.data")
    ap.add_argument("--test_file", type=str, default=None, help="the test split's data file (predict.py, extract.py --split test)")
    ap.add_argument("--test_img", type=str, default=None, help="the test split's image directory")
    ap.add_argument("--preprocess", default=None, choices=list(PREPROCESS),
                    help="file data: where images are resized and normalised -- 'hip' (the default on a GPU): one HIP launch "
                         "per batch on the prefetcher's copy stream, the GPU receives the decoded uint8 pixels; 'host' (the "
                         "default on the CPU): PIL and a lookup table per image, the reference's transform")
    ap.add_argument("--vocab_size", type=int, default=10000)
    ap.add_argument("--max_seq_length", type=int, default=26)
    ap.add_argument("--image_size", type=int, default=0, help="override the model's image size (0 = registry)")
    ap.add_argument("--channels_last", type=str2bool, default="true",
                    help="run the stock image encoder in channels_last (MIOpen NHWC kernels)")
    ap.add_argument("--val_interval", type=int, default=0,
                    help="validate every this many steps (0: at --log_interval, as main.py:225-246, when --val_size > 0)")
    ap.add_argument("--val_batches", type=int, default=0, help="validation batches (overrides --val_size // --batch_size)")
    ap.add_argument("--save_path", type=str, default=None, help="also save the final state_dict here")
    ap.add_argument("--question_mask", type=str2bool, default="false",
                    help="co-attention over each question's first ques_len tokens only (a_q = 0 on pad tokens); default: "
                         "unmasked, as the reference (model.py:388).  Checkpoints hold only the state_dict, so the flag is not "
                         "recorded: give prediction the value the checkpoint was trained with (a mismatch goes undetected)")
    ap.add_argument("--affinity", default="reference", choices=["reference", "bilinear"],
                    help="co-attention affinity: 'reference' = tanh(Q V^T) as model.py:377 (W_b constructed, never trained); "
                         "'bilinear' = tanh(W_b(Q) V^T) as the published model, W_b trained.  Co-attention models only, not with "
                         "--opt_lvl >= 1.  Checkpoints hold only the state_dict (same keys for both), so the flag is not "
                         "recorded: give prediction the value the checkpoint was trained with (a mismatch goes undetected)")
    ap.add_argument("--co_attention", default="parallel", choices=["parallel", "alternating"],
                    help="co-attention form (Lu et al. 2016 section 3.3): 'parallel' = the reference's ParallelCoAttention; "
                         "'alternating' = three chained guided-attention steps (AlternatingCoAttention; its own state_dict "
                         "keys).  Co-attention models only, exact mode only: not with --affinity bilinear, --opt_lvl >= 1 or "
                         "--precision fast")
    ap.add_argument("--sentence_lstm", default="stock", choices=list(SENTENCE_LSTMS),
                    help="the question encoder's sentence LSTM: 'stock' = pack_padded_sequence -> nn.LSTM -> "
                         "pad_packed_sequence as the reference (model.py:286-296); 'hip' = the length-aware HIP forward / "
                         "backward on the same parameters (exact fp32, no packing, no host read of the lengths).  "
                         "Co-attention models only; a checkpoint does not depend on it")
    ap.add_argument("--question_gru", default="stock", choices=list(QUESTION_GRUS),
                    help="the baseline question encoder's GRU: 'stock' = pack_padded_sequence -> nn.GRU as the reference "
                         "(model.py:86-100; sorted lengths, read on the host); 'hip' = the length-aware HIP forward / backward on "
                         "the same parameters (exact fp32, no packing, no host read of the lengths, any order).  --model baseline "
                         "only; a checkpoint does not depend on it")
    ap.add_argument("--fusion_head", default="stock", choices=list(FUSION_HEADS),
                    help="the baseline model behind its two encoders (row norm, the two embeddings, the product, Linear -> "
                         "Dropout -> Tanh, the classifier): 'stock' = the nn modules as the reference (model.py:10-38); 'hip' = "
                         "four HIP launches forward and three backward on the same parameters (exact fp32; the dropout drawn "
                         "inside the head from --dropout_seed + rank, nothing from torch's generators).  --model baseline only, "
                         "not with --vgg_train true or --opt_lvl >= 1; a checkpoint does not depend on it")
    ap.add_argument("--encoder_eval", default="stock", choices=list(ENCODER_EVALS),
                    help="the frozen VGG's eval-mode groups (validation, predict.py, extract.py): stock (the default: every route as "
                         "it is) or hip (BatchNorm on running statistics + bias + ReLU + pool in one HIP launch per group, the first "
                         "group from the image; verified per shape against the stock kernels, same bits)")
    ap.add_argument("--word_embedding", default="stock", choices=list(WORD_EMBEDDINGS),
                    help="the question encoder's word level: 'stock' = nn.Embedding and PyTorch's embedding backward; 'hip' = "
                         "the HIP gather and its dense gradient in one launch each on the same parameter (fixed summation "
                         "order, no host read of the ids).  --model attention only; a checkpoint does not depend on it")
    ap.add_argument("--dropout", type=float, default=0.0,
                    help="feature dropout probability P in [0, 1) on the attended features q_l + v_l in front of the answer head "
                         "(Lu et al. 2016 use 0.5): one HIP launch per direction, the mask regenerated in the backward.  "
                         "Co-attention models only, not with --opt_lvl >= 1.  Prediction runs in eval mode and needs no flag.  "
                         "The checkpoint does not record the mask counter: a resumed run draws other masks than the "
                         "uninterrupted one would")
    ap.add_argument("--dropout_seed", type=int, default=0,
                    help="seed of the dropout masks (rank r of a data-parallel run uses seed + r); torch's generators are not "
                         "consumed, so images, questions, labels and weights keep their bits for every value")
    ap.add_argument("--loss", default="ce", choices=list(LOSSES),
                    help="'ce' = the reference's cross entropy on the majority answer; 'soft_ce' / 'bce' = soft cross entropy / "
                         "binary cross entropy with logits on the soft answer targets (up to --num_answers (answer, score) pairs "
                         "per sample; validation then reports the VQA score).  The checkpoint does not record it: give "
                         "prediction the value the checkpoint was trained with (with 'bce' its probabilities are sigmoids)")
    ap.add_argument("--num_answers", type=int, default=10, help="answer slots per sample of the soft targets (1..16)")
    ap.add_argument("--optimizer", default="torch", choices=list(OPTIMIZERS),
                    help="'torch' = torch.optim.Adam as the reference (main.py:180); 'hip' = the fused HIP Adam step (one launch "
                         "for all parameters; same arithmetic), which also takes --weight_decay and --clip_grad_norm")
    ap.add_argument("--weight_decay", type=float, default=0.0, help="decoupled weight decay (AdamW); --optimizer hip only")
    ap.add_argument("--clip_grad_norm", type=float, default=None,
                    help="clip the gradients to this global norm ahead of the update; --optimizer hip only")
    ap.add_argument("--image_features", type=str, default=None,
                    help="train from this feature table (python -m vqa_amd.extract --split train) instead of running the "
                         "frozen image encoder in the step: each batch's rows are gathered on the device.  The features are the "
                         "encoder's in eval mode (running statistics), as validation and prediction see them; the table's "
                         "sidecar must match the run (model, image size, split, seed, samples = --num_steps x --batch_size).  "
                         "Co-attention models only, not with --vgg_train true; {rank} in the path for data-parallel runs")
    ap.add_argument("--val_image_features", type=str, default=None,
                    help="the validation split's table (--split val); required when a run on --image_features validates")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_loss(args.loss, args.num_answers)
    check_optimizer(args.optimizer, args.weight_decay, args.clip_grad_norm)
    if args.mode == "test":
        raise NotImplementedError("TODO: test mode")          # as the reference, main.py:286-287
    files = not args.synthetic                                  # the reference's dataset files (vqa_amd.data)
    n_val = args.val_batches or args.val_size // args.batch_size
    vocab = None
    try:
        if files:
            check_files(args, "train", int(os.environ.get("WORLD_SIZE", "1")), validates=n_val > 0)
            vocab = file_vocab(args)                            # (the model below is built from its sizes)
        check_image_features(args, int(os.environ.get("WORLD_SIZE", "1")), validates=n_val > 0)
    except (ValueError, OSError) as e:
        raise SystemExit(str(e))

    rank, world, local = vdist.init_from_env()
    if torch.cuda.is_available():
        device = torch.device("cuda", local if "LOCAL_RANK" in os.environ else args.gpu_id)   # (main.py:80)
    else:
        device = torch.device("cpu")
    if device.type == "cuda":
        torch.cuda.set_device(device)
        # the step is GPU work; the host side only launches kernels and stages batches.  ATen's default of
        # one thread per logical CPU oversubscribes a containerised rank (measured: 39.7 vs 26.3 ms/step)
        torch.set_num_threads(max(1, min(4, usable_cpus())))
    try:
        check_encoder_eval(args.model, args.encoder_eval, args.channels_last, device.type, args.opt_lvl)
    except ValueError as e:
        raise SystemExit(str(e))
    torch.manual_seed(0)                                        # identical weights on every rank
    model, cfg = model_from_args(args)
    # log directory expt_dir/expt_name/run_name (main.py:110-114): checkpoints model_{step}.pth live there (main.py:260-263)
    log_dir = log_dir_of(args)
    if log_dir and rank == 0:
        os.makedirs(log_dir, exist_ok=True)
    if args.model_ckpt:
        model.load_state_dict(torch.load(checkpoint_path(args), map_location="cpu"))
    model.to(device)
    cl = args.channels_last and device.type == "cuda" and args.model.startswith("attention")
    if cl:
        model.image_encoder.to(memory_format=torch.channels_last)
    trainer = Trainer(model, args.learning_rate, device, args.opt_lvl, precision=args.precision, loss=args.loss,
                      optimizer=args.optimizer, weight_decay=args.weight_decay, clip_grad_norm=args.clip_grad_norm,
                      sentence_lstm=args.sentence_lstm, word_embedding=args.word_embedding, feature_dropout=args.dropout,
                      dropout_seed=args.dropout_seed, encoder_eval=args.encoder_eval, question_gru=args.question_gru,
                      fusion_head=args.fusion_head)
    n_ans = args.num_answers if args.loss != "ce" else 0
    size = (args.image_size, args.image_size) if args.image_size else cfg["image_size"]
    n_cls = args.num_cls + 1

    cached = bool(args.image_features)                           # the `image` slot of a batch then holds table rows' indices

    def table(path, split, seed, n_samples, ds=None):
        from .features import FeatureTable
        tab = FeatureTable.load(path.replace("{rank}", str(rank)), device)
        # (before the first step: a table of another run, or of another file list, is refused)
        if ds is not None:
            tab.check_files(args.model, size[0], split, ds.image_names)
        else:
            tab.check(args.model, size[0], split, seed, n_samples)
        return tab

    def loader(n_samples, seed):
        ds = SyntheticVQADataset(n_samples, size, args.max_seq_length, args.vocab_size, n_cls, seed, num_answers=n_ans,
                                 images=not cached)
        return torch.utils.data.DataLoader(ds, args.batch_size, shuffle=True, drop_last=True, num_workers=args.num_workers,
                                           generator=torch.Generator().manual_seed(seed))

    def sorted_host(batch):                                      # main.py:196-202
        extras = (batch["answers"], batch["answer_scores"]) if n_ans else ()
        if files:
            batch["image"] = file_images.host(batch["image"])    # the decoded pixels, packed (hip) or preprocessed (host)
        image, question, label, ques_len, *extras = sort_batch(batch["image"], batch["question"], batch["label"],
                                                               batch["ques_len"], *extras)
        return (image, question, ques_len, label, *extras)

    file_images = train_ds = val_ds = None
    if files:
        # an epoch is one pass over --train_file (shuffled, the last partial batch dropped: main.py:129-130)
        file_images = FileImages(args, size[0], device)
        train_ds = file_dataset(args, "train", vocab)
        train_loader = file_loader(train_ds, args, shuffle=True, seed=1234 + rank, drop_last=True)
        if rank == 0:
            print(json.dumps({"data": "files", "samples": len(train_ds), "images": len(train_ds.image_names),
                              "steps_per_epoch": len(train_loader), "preprocess": "none (cached features)" if cached else
                              file_images.mode, "note": "--num_steps is ignored: an epoch is one pass over --train_file"}))
        if len(train_loader) == 0:
            raise SystemExit("--train_file holds %d samples: fewer than one batch of %d" % (len(train_ds), args.batch_size))
    else:
        train_loader = loader(args.num_steps * args.batch_size, 1234 + rank)
    steps_per_epoch = len(train_loader)
    feats = table(args.image_features, "train", 1234 + rank, args.num_steps * args.batch_size, train_ds) if cached else None
    if files and n_val > 0:
        val_ds = file_dataset(args, "val", vocab)
    val_feats = (table(args.val_image_features, "val", 987654 + rank, n_val * args.batch_size, val_ds)
                 if cached and n_val > 0 else None)
    val = []
    if n_val > 0:
        val_batches = (file_loader(val_ds, args, shuffle=False) if files else loader(n_val * args.batch_size, 987654 + rank))
        for i, b in enumerate(val_batches):
            if i >= n_val:                                       # (file data: the first n_val batches of --val_file)
                break
            image, question, ques_len, label, *extras = sorted_host(b)
            # (file data: the pixels are resized and normalised here, in the layout the encoder runs in)
            image = file_images.device_images(image, cl and not cached) if files else image.to(device)
            if cached:
                image = val_feats.gather(image)                  # this batch's rows, gathered once
            elif cl and not files:
                image = image.contiguous(memory_format=torch.channels_last)
            val.append((image, question.to(device), ques_len, label.to(device), *[e.to(device) for e in extras]))
    val_every = args.val_interval or (args.log_interval if val else 0)

    t0 = time.time()
    step = 0
    for epoch in range(args.num_epochs):
        batches = DevicePrefetcher((sorted_host(b) for b in train_loader), device, cl and not cached,
                                   preprocess=file_images.hip if files else None)
        for image, question, ques_len, label, *extras in batches:
            validate_now = bool(val) and val_every > 0 and (step + 1) % val_every == 0
            if cached:                                           # `image`: the batch's row indices, on the device
                loss = trainer.step_features(feats.gather(image), question, ques_len, label,
                                             targets=tuple(extras) if extras else None)
            else:
                # no encoder run-ahead across a validation: its BatchNorm statistics must be those of this step
                nxt, ready = (None, None) if validate_now else batches.peek_image()
                loss = trainer.step(image, question, ques_len, label, next_image=nxt, next_ready=ready,
                                    targets=tuple(extras) if extras else None)
            if (step + 1) % args.log_interval == 0:
                trainer.check_labels()                           # (the host synchronises here anyway to read the loss)
                trainer.check_range()
                if cached and device.type == "cuda":
                    from .features import bad_indices
                    n_bad = bad_indices()
                    if n_bad:
                        raise IndexError("%d image indices lay outside the feature table (their rows were zeros)" % n_bad)
                if files and file_images.hip is not None:
                    from .preprocess import bad_images
                    n_bad = bad_images()
                    if n_bad:
                        raise ValueError("%d images were refused by the preprocessing launch (their pixels were zeros)" % n_bad)
                if rank == 0:
                    print(json.dumps({"epoch": epoch + 1, "step": step + 1, "steps_per_epoch": steps_per_epoch,
                                      "loss": round(float(loss), 5), "precision": trainer.precision,
                                      "pairs_per_s": round(world * args.batch_size * (step + 1) / (time.time() - t0), 2)}))
            if validate_now:
                m = trainer.validate(val, features=cached)
                if rank == 0:
                    print(json.dumps({"step": step + 1, "val_accuracy": round(m["accuracy"], 3), "val_loss": round(m["loss"], 5),
                                      **({"val_vqa_score": round(m["vqa_score"], 5)} if "vqa_score" in m else {})}))
            if (step + 1) % args.save_interval == 0 and log_dir and rank == 0:   # main.py:260-263
                torch.save(model.state_dict(), os.path.join(log_dir, "model_%d.pth" % (step + 1)))
            step += 1
    if args.save_path and rank == 0:
        torch.save(model.state_dict(), args.save_path)
    vdist.shutdown()


if __name__ == "__main__":
    main()

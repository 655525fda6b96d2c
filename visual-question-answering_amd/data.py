"""The reference's dataset files: data files of ``img_name \\t question \\t answer`` lines, an image directory and the vocabulary
pickle its ``prepare_data.py`` writes (utils.py:162-198) -- ``preprocess_text``, ``encode_question``, ``build_vocab`` /
``load_vocab`` and ``VQAFileDataset``, which yields the reference's sample keys (dataloader.py:72) with the image still a
decoded uint8 array: resizing and normalising are a batch's work (``vqa_amd.preprocess``), not a sample's.  DESIGN.md section
3.18.

``python -m vqa_amd.data vocab --train_file F --vocab_file V [--min_word_count 1] [-K 1000]`` writes the vocabulary.  The
step from the VQA annotation JSON to the data files stays with the reference's prepare_data.py.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import pickle
import string

import numpy as np
import torch

VOCAB_KEYS = ("word2idx", "idx2word", "label2idx", "idx2label", "max_seq_length")
PAD, UNKNOWN, UNKNOWN_LABEL = "<PAD>", "<UNKNOWN>", "UNKNOWN"
_NO_PUNCTUATION = str.maketrans("", "", string.punctuation)
IMAGE_MODES = ("pixels", "row")


def preprocess_text(text: str):
    """The reference's question cleaning (utils.py:48-73): commas become spaces, punctuation is stripped from every word, empty
    strings and the token ``s`` (what ``'s`` leaves) are dropped, the rest is lower-cased -- in that order, so ``S`` stays."""
    words = [w.translate(_NO_PUNCTUATION) for w in text.strip().replace(",", " ").split()]
    return [w.lower() for w in words if w != "" and w != "s"]


def encode_question(words, word2idx, max_seq_length: int):
    """(int64 [max_seq_length], ques_len): the ids of `words` (a string is cleaned first), <UNKNOWN> for a word outside the
    vocabulary, truncated and zero-padded; ques_len counts the non-zero ids (dataloader.py:58-65)."""
    if isinstance(words, str):
        words = preprocess_text(words)
    unk = word2idx[UNKNOWN]
    ids = np.zeros(int(max_seq_length), dtype=np.int64)
    head = [word2idx.get(w, unk) for w in words[:max_seq_length]]
    ids[:len(head)] = head
    return ids, int(np.count_nonzero(ids))


def read_lines(data_file: str):
    """[(img_name, question, answer)] of a data file; a line without three tab-separated fields raises with its number."""
    with open(data_file, "r") as fh:
        lines = fh.read().strip().split("\n")
    out = []
    for i, line in enumerate(lines):
        parts = line.strip().split("\t")
        if len(parts) != 3:
            raise ValueError("%s line %d: expected `img_name \\t question \\t answer`, got %d fields" % (data_file, i + 1, len(parts)))
        out.append((parts[0], parts[1].strip(), parts[2].strip()))
    return out


def build_vocab(train_file: str, min_word_count: int = 1, K: int = 1000) -> dict:
    """The vocabulary of a training file, with the reference's five keys (utils.py:76-159, 190-192): <PAD> = 0, <UNKNOWN> = 1,
    then the words seen at least `min_word_count` times in first-seen order; max_seq_length the longest cleaned question;
    labels `UNKNOWN` = 0, then the K most frequent answers, ties in first-seen order (a stable sort)."""
    word_count, answer_count, longest = {}, {}, 0
    for _, question, answer in read_lines(train_file):
        words = preprocess_text(question)
        for w in words:
            word_count[w] = word_count.get(w, 0) + 1
        longest = max(longest, len(words))
        answer_count[answer] = answer_count.get(answer, 0) + 1
    word2idx = {PAD: 0, UNKNOWN: 1}
    for w, n in word_count.items():
        if n >= min_word_count:
            word2idx[w] = len(word2idx)
    top = sorted(answer_count.items(), key=lambda kv: -kv[1])[:K]        # (stable: ties keep their first-seen order)
    labels = [UNKNOWN_LABEL] + [a for a, _ in top]
    label2idx = {a: i for i, a in enumerate(labels)}
    return {"word2idx": word2idx, "idx2word": {i: w for w, i in word2idx.items()}, "label2idx": label2idx,
            "idx2label": {i: a for i, a in enumerate(labels)}, "max_seq_length": longest}


def save_vocab(vocab: dict, vocab_file: str) -> None:
    with open(vocab_file, "wb") as fh:
        pickle.dump({k: vocab[k] for k in VOCAB_KEYS}, fh, protocol=pickle.HIGHEST_PROTOCOL)


def load_vocab(vocab_file: str) -> dict:
    """The vocabulary pickle, its five entries read BY KEY (the reference unpacks ``vocab.values()`` by position, main.py)."""
    with open(vocab_file, "rb") as fh:
        vocab = pickle.load(fh)
    missing = [k for k in VOCAB_KEYS if not isinstance(vocab, dict) or k not in vocab]
    if missing:
        raise ValueError("%s is no vocabulary file: it lacks %s" % (vocab_file, ", ".join(missing)))
    for k in (PAD, UNKNOWN):
        if k not in vocab["word2idx"]:
            raise ValueError("%s: word2idx lacks %s" % (vocab_file, k))
    if vocab["word2idx"][PAD] != 0 or UNKNOWN_LABEL not in vocab["label2idx"]:
        raise ValueError("%s: <PAD> must be id 0 and the labels must hold %s" % (vocab_file, UNKNOWN_LABEL))
    return {k: vocab[k] for k in VOCAB_KEYS}


def names_digest(names) -> str:
    """SHA-256 of the newline-joined image names: what a feature table of a file list records."""
    return hashlib.sha256("\n".join(names).encode("utf-8")).hexdigest()


def load_image(path: str) -> np.ndarray:
    """uint8 [h, w, 3]: a ``.npy`` file is read as it is (pre-decoded datasets), anything else through PIL, as RGB."""
    if path.endswith(".npy"):
        img = np.load(path, allow_pickle=False)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("%s: a .npy image must be uint8 [h, w, 3]; got %s %s" % (path, img.dtype, img.shape))
        return img
    try:
        from PIL import Image
    except ImportError as e:                              # pragma: no cover
        raise RuntimeError("decoding %s needs Pillow (PIL), which is not installed; .npy images need none" % path) from e
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


class VQAFileDataset(torch.utils.data.Dataset):
    """The samples of a data file: ``question`` int64 [T], ``ques_len``, ``label`` (an answer outside the table is UNKNOWN) as
    the reference's VQADataset yields them, and under ``image`` -- images="pixels": the decoded uint8 [h, w, 3] array;
    images="row": the index of the sample's image in ``image_names`` (the distinct names in first-seen order: the rows of a
    feature table), and no file is opened."""

    def __init__(self, data_file, img_dir, vocab, images="pixels"):
        if images not in IMAGE_MODES:
            raise ValueError("VQAFileDataset: images must be one of %s, got %r" % (IMAGE_MODES, images))
        if images == "pixels" and not img_dir:
            raise ValueError("VQAFileDataset: images='pixels' needs the image directory")
        self.data_file, self.img_dir, self.images = data_file, img_dir, images
        self.samples = read_lines(data_file)
        self.word2idx, self.label2idx, self.T = vocab["word2idx"], vocab["label2idx"], int(vocab["max_seq_length"])
        first = {}
        for name, _, _ in self.samples:
            first.setdefault(name, len(first))
        self.image_names = list(first)
        self.rows = [first[name] for name, _, _ in self.samples]

    def __len__(self):
        return len(self.samples)

    def words(self, i):
        return preprocess_text(self.samples[i][1])

    def load(self, name) -> np.ndarray:
        return load_image(os.path.join(self.img_dir, name))

    def __getitem__(self, i):
        name, question, answer = self.samples[i]
        ids, n = encode_question(question, self.word2idx, self.T)
        label = self.label2idx[answer if answer in self.label2idx else UNKNOWN_LABEL]
        image = self.load(name) if self.images == "pixels" else torch.tensor(self.rows[i], dtype=torch.int64)
        return {"image": image, "question": torch.from_numpy(ids), "ques_len": torch.tensor(n), "label": torch.tensor(label),
                "index": torch.tensor(i)}


class DistinctImages(torch.utils.data.Dataset):
    """The distinct images of a VQAFileDataset, in ``image_names`` order: what a feature table encodes, one row each."""

    def __init__(self, dataset: VQAFileDataset):
        self.ds = dataset

    def __len__(self):
        return len(self.ds.image_names)

    def __getitem__(self, r):
        return {"image": self.ds.load(self.ds.image_names[r]), "row": torch.tensor(r)}


def collate(samples, pack=None):
    """A list of samples -> a batch: the tensors stacked; ``image`` a list of uint8 arrays, or -- with ``pack``, an
    ImagePreprocessor's -- the PackedBatch of their pixels and descriptors, or the stacked row indices."""
    out = {k: torch.stack([s[k] for s in samples]) for k in samples[0] if k != "image"}
    first = samples[0]["image"]
    if torch.is_tensor(first):
        out["image"] = torch.stack([s["image"] for s in samples])
    else:
        images = [s["image"] for s in samples]
        out["image"] = pack(images) if pack is not None else images
    return out


def sort_batch(batch: dict) -> dict:
    """The batch in descending order of question length (utils.py:33-45).  A PackedBatch is permuted by its descriptor rows;
    its pixels stay where they are."""
    lens, order = batch["ques_len"].sort(dim=0, descending=True)
    out = {}
    for k, v in batch.items():
        if k == "ques_len":
            out[k] = lens
        elif isinstance(v, list):
            out[k] = [v[i] for i in order.tolist()]
        else:
            out[k] = v[order]                               # (a tensor, or a PackedBatch: its __getitem__ permutes)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="VQA dataset files")
    sub = ap.add_subparsers(dest="command", required=True)
    v = sub.add_parser("vocab", help="build the vocabulary pickle of a training file")
    v.add_argument("--train_file", required=True)
    v.add_argument("--vocab_file", required=True)
    v.add_argument("--min_word_count", type=int, default=1)
    v.add_argument("--num_cls", "-K", type=int, default=1000)
    args = ap.parse_args(argv)
    vocab = build_vocab(args.train_file, args.min_word_count, args.num_cls)
    save_vocab(vocab, args.vocab_file)
    print("vocab size %d, max sequence length %d, %d labels -> %s"
          % (len(vocab["word2idx"]), vocab["max_seq_length"], len(vocab["label2idx"]), args.vocab_file))


if __name__ == "__main__":
    main()

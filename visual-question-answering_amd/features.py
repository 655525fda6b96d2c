"""Cached image features: the frozen image encoder's output encoded once into a table (``python -m vqa_amd.extract``), and
the device-side data path that feeds a training or prediction step from it -- ``gather_features``: the rows of a batch in one
HIP launch of 16-byte copies (``csrc/features.hip``, ``coattn_features_gather`` of ``include/coattn.h``: indices read on the
device only, an index outside the table gives a zero row and is counted, a bf16 table is up-cast on the way), and
``FeatureTable``: the table on the device with the sidecar that says what it was made from.  DESIGN.md section 3.16.

The features are those of the encoder in eval mode (BatchNorm on its running statistics): what ``Trainer.validate`` and
``predict.py`` feed the model.  Batch-statistics features, tables larger than the device memory and a trainable encoder are
not offered.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import _lib

_IDX_DTYPES = {torch.int32: _lib.IDS_I32, torch.int64: _lib.IDS_I64}
_TABLE_DTYPES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}          # --features_dtype / the sidecar's "dtype"
SPLITS = ("train", "val", "test")
ENCODER_STATS = "running"                                          # the one kind of table there is (eval-mode BatchNorm)
_COPY_BYTES = 256 << 20                                            # host -> device pieces of FeatureTable.load


def supported(S, B, N, d, dtype=torch.float32) -> bool:
    """Does the HIP gather take this shape (include/coattn.h coattn_features_gather_supported)?  No GPU call."""
    return dtype in _TABLE_DTYPES and bool(_lib.load().coattn_features_gather_supported(S, B, N, d, _TABLE_DTYPES[dtype], 0))


_bad = {}                     # device index -> int32[1] counter the gathers add to


def _counter(dev):
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    c = _bad.get(key)
    if c is None:
        c = _bad[key] = torch.zeros(1, device=torch.device("cuda", key), dtype=torch.int32)
    return c


def bad_indices() -> int:
    """How many image indices outside [0, S) the gathers of this process have met (each gave a row of zeros) since the last
    call, over all devices; clears the count.  Synchronises every device it reads -- call it where the host reads the loss,
    not in the step."""
    total = 0
    for key, c in _bad.items():
        torch.cuda.synchronize(key)                              # (the whole device, not the current stream alone)
        total += int(c.item())
        c.zero_()
        torch.cuda.synchronize(key)                              # the clear lands before a gather on another stream adds
    return total


def gather_features(table, idx, out=None):
    """table [S, N, d] (fp32 or bfloat16, contiguous), idx [B] (integer) -> fp32 [B, N, d] = table[idx], bit for bit (bf16:
    the exact up-cast).  CUDA tensors take one launch of coattn_features_gather on the current stream: no host read of the
    indices, an index outside [0, S) gives a row of exact +0 and is counted (``bad_indices()``) where stock ``table[idx]``
    device-asserts; a shape the kernel does not take is an error, never another route.  CPU tensors take
    ``table[idx].float()``, where a bad index raises as torch does.  No gradient flows to the table: one that requires grad is
    refused.  `out`: a contiguous fp32 [B, N, d] buffer on the table's device to write into."""
    if table.requires_grad:
        raise RuntimeError("gather_features: the table requires grad; cached features carry no gradient (the encoder is frozen)")
    if table.dim() != 3 or table.dtype not in _TABLE_DTYPES:
        raise RuntimeError("gather_features takes an fp32 or bfloat16 [S, N, d] table; got %s %s" % (table.dtype, tuple(table.shape)))
    if idx.dim() != 1 or idx.is_floating_point() or idx.is_complex() or idx.dtype == torch.bool:
        raise RuntimeError("gather_features takes a 1-D integer idx; got %s %s" % (idx.dtype, tuple(idx.shape)))
    if table.device != idx.device:
        raise RuntimeError("gather_features: table on %s, idx on %s" % (table.device, idx.device))
    S, N, d = table.shape
    B = idx.numel()
    if out is not None and (tuple(out.shape) != (B, N, d) or out.dtype != torch.float32 or not out.is_contiguous()
                            or out.device != table.device):
        raise RuntimeError("gather_features: `out` must be a contiguous fp32 [B, N, d] tensor on the table's device")
    if not table.is_cuda:
        rows = table.detach()[idx.long()].float()
        if out is None:
            return rows
        out.copy_(rows)
        return out
    if not table.is_contiguous():
        raise RuntimeError("gather_features: the table must be contiguous (location-major [S, N, d])")
    if not supported(S, B, N, d, table.dtype):
        raise RuntimeError("gather_features (HIP): shape S=%d B=%d N=%d d=%d of %s not supported (B >= 1, N <= 4096, d <= 2048, "
                           "N*d a multiple of 4 for fp32 or 8 for bf16: coattn_features_gather_supported)"
                           % (S, B, N, d, table.dtype))
    if idx.dtype not in _IDX_DTYPES:
        idx = idx.to(torch.int64 if idx.element_size() == 8 else torch.int32)
    idx = idx.contiguous()
    if out is None:
        out = torch.empty((B, N, d), dtype=torch.float32, device=table.device)
    with _lib.on_device(table.device):
        _lib.bind("coattn_features_gather", table=table.detach(), table_dtype=_TABLE_DTYPES[table.dtype], idx=idx,
                  idx_dtype=_IDX_DTYPES[idx.dtype], out=out, bad_idx=_counter(table.device), S=S, B=B, N=N, d=d, flags=0,
                  stream=_lib.stream_ptr(table.device))()
    return out


def sidecar_path(path: str) -> str:
    """The JSON sidecar of the table file `path`: beside it, `.json` in place of a `.npy` suffix."""
    return (path[:-4] if path.endswith(".npy") else path) + ".json"


def abi_version() -> str:
    v = _lib.load().coattn_version()
    return "%d.%d.%d" % (v // 10000, v // 100 % 100, v % 100)


def make_meta(model_name, image_size, N, d, dtype, split, seed, S) -> dict:
    """What a table's sidecar records (`FeatureTable.check` compares the run against it)."""
    if dtype not in DTYPES:
        raise ValueError("features dtype must be one of %s, got %r" % (tuple(DTYPES), dtype))
    if split not in SPLITS:
        raise ValueError("split must be one of %s, got %r" % (SPLITS, split))
    side = int(round(N ** 0.5))
    return {"model": model_name, "image_size": int(image_size), "N": int(N), "d": int(d),
            "grid": [side, side] if side * side == N else [1, int(N)], "dtype": dtype, "split": split, "seed": int(seed),
            "S": int(S), "encoder_stats": ENCODER_STATS, "abi": abi_version()}


class FeatureTable:
    """A feature table on one device: ``data`` [S, N, d] (fp32 or bfloat16) and ``meta`` (`make_meta`).  On disk it is a
    ``.npy`` of fp32, or of uint16 holding the bf16 bits, and a JSON sidecar beside it."""

    def __init__(self, data, meta):
        if data.dim() != 3 or data.dtype not in _TABLE_DTYPES:
            raise ValueError("FeatureTable takes an fp32 or bfloat16 [S, N, d] tensor; got %s %s" % (data.dtype, tuple(data.shape)))
        meta = dict(meta)
        want = {"S": data.shape[0], "N": data.shape[1], "d": data.shape[2],
                "dtype": "bf16" if data.dtype == torch.bfloat16 else "fp32"}
        for k, v in want.items():
            if meta.get(k) != v:
                raise ValueError("FeatureTable: the sidecar's %s is %r, the data's is %r" % (k, meta.get(k), v))
        if meta.get("encoder_stats") != ENCODER_STATS:
            raise ValueError("FeatureTable: encoder_stats %r; only %r tables (the encoder in eval mode) are offered"
                             % (meta.get("encoder_stats"), ENCODER_STATS))
        self.data, self.meta = data.detach().contiguous(), meta

    def __len__(self):
        return self.data.shape[0]

    def save(self, path: str) -> None:
        host = self.data.cpu()
        arr = host.view(torch.int16).numpy().view(np.uint16) if host.dtype == torch.bfloat16 else host.numpy()
        with open(path, "wb") as fh:                              # (a file object: np.save appends no suffix)
            np.save(fh, arr)
        with open(sidecar_path(path), "w") as fh:
            json.dump(self.meta, fh, indent=1, sort_keys=True)

    @classmethod
    def load(cls, path: str, device="cpu") -> "FeatureTable":
        """Memory-map `path`, read its sidecar and copy the table to `device` once, in pieces (no second host copy).  On a
        GPU the table's bytes are first compared with the free device memory: a table that does not fit raises with both
        numbers in place of an out-of-memory error."""
        device = torch.device(device)
        with open(sidecar_path(path)) as fh:
            meta = json.load(fh)
        arr = np.load(path, mmap_mode="r")
        bf16 = meta.get("dtype") == "bf16"
        if arr.ndim != 3 or arr.dtype != (np.uint16 if bf16 else np.float32):
            raise ValueError("%s: a %s table is a 3-D .npy of %s; found %s %s" % (path, meta.get("dtype"),
                                                                                 "uint16" if bf16 else "float32", arr.dtype, arr.shape))
        if device.type == "cuda":
            free, total = torch.cuda.mem_get_info(device)
            if arr.nbytes > free:
                raise RuntimeError("%s: the table holds %d bytes, %s has %d bytes free (of %d): a table that does not fit the "
                                   "device memory is not offered" % (path, arr.nbytes, device, free, total))
        data = torch.empty(arr.shape, dtype=torch.bfloat16 if bf16 else torch.float32, device=device)
        raw = data.view(torch.int16) if bf16 else data
        rows = max(1, _COPY_BYTES // max(1, arr[0].nbytes))
        for lo in range(0, arr.shape[0], rows):
            piece = np.array(arr[lo:lo + rows])                  # (this piece alone leaves the map: a writable host copy)
            raw[lo:lo + rows].copy_(torch.from_numpy(piece.view(np.int16) if bf16 else piece))
        return cls(data, meta)

    def gather(self, idx, out=None):
        """fp32 [B, N, d]: the rows `idx` (on the table's device) -- `gather_features`."""
        return gather_features(self.data, idx, out)

    def check(self, model_name, image_size, split, seed, S) -> None:
        """Raise ValueError unless the table was made for this run; the message names the field that differs."""
        for field, mine in (("model", model_name), ("image_size", int(image_size)), ("split", split), ("seed", int(seed)),
                            ("S", int(S))):
            if self.meta.get(field) != mine:
                raise ValueError("feature table: %s is %r in the sidecar, %r in this run" % (field, self.meta.get(field), mine))

    def check_files(self, model_name, image_size, split, image_names) -> None:
        """The same for a table of file data (``extract.py --synthetic false``: one row per distinct image, in the order of
        ``VQAFileDataset.image_names``): the model, the image size, the split, and the file list -- its source, its length and
        the SHA-256 of its newline-joined names -- must be this run's."""
        from .data import names_digest
        for field, mine in (("model", model_name), ("image_size", int(image_size)), ("split", split), ("source", "files"),
                            ("images", len(image_names)), ("S", len(image_names)), ("names_sha256", names_digest(image_names))):
            if self.meta.get(field) != mine:
                raise ValueError("feature table: %s is %r in the sidecar, %r in this run" % (field, self.meta.get(field), mine))


def files_meta(meta: dict, image_names) -> dict:
    """`make_meta`'s record plus what a table of file data records besides: where its rows come from."""
    from .data import names_digest
    return {**meta, "source": "files", "images": len(image_names), "names_sha256": names_digest(image_names)}

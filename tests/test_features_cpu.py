"""Cached image features (include/coattn.h v0.20.0, vqa_amd.features, vqa_amd.extract, Trainer.step_features,
--image_features) as far as they go without a GPU: the declaration, the exports, the supported table, every argument error of
the entry point, the table's round trip through its files, the sidecar check, the image-free dataset, the command-line refusals
and the CPU route of the gather."""
import ctypes as C
import json
import re

import numpy as np
import pytest
import torch

import vqa_amd
from vqa_amd import _lib, extract as X, features as FT, predict as P, train as T

from tests._header import args as header_args, header


def _err():
    return _lib.load().coattn_last_error().decode()


def test_header_declares_exports_constants_and_version():
    hdr = header()
    for fn in ("coattn_features_gather_supported", "coattn_features_gather"):
        assert re.search(r"^int %s\(" % fn, hdr, re.M), fn
        assert fn in _lib.EXPORTS and hasattr(C.CDLL(_lib.LIB_PATH), fn), fn
    assert _lib.load().coattn_version() >= 2000
    for name in ("COATTN_FEATURES_THREADS", "COATTN_FEATURES_LOADS"):
        assert int(re.search(r"^#define %s (\d+)" % name, hdr, re.M).group(1)) >= 1
    assert vqa_amd.gather_features is FT.gather_features and vqa_amd.FeatureTable is FT.FeatureTable
    assert {"features", "gather_features", "FeatureTable"} <= set(vqa_amd.__all__)
    assert FT.abi_version() == "0.%d.%d" % divmod(_lib.load().coattn_version(), 100)


def test_tabled_signature_matches_the_header():
    fn = "coattn_features_gather"
    assert _lib.SIGNATURES[fn][-1][0] == "stream"                                # (names and types: tests/test_call_layer_cpu.py)
    names = [a.split()[-1] for a in header_args(header(), "coattn_features_gather_supported")]
    assert names == "S B N d table_dtype flags".split()
    assert len(_lib.load().coattn_features_gather_supported.argtypes) == 6


def test_supported_table_at_its_edges():
    sup = lambda S, B, N, d, dt=_lib.F32, fl=0: _lib.load().coattn_features_gather_supported(S, B, N, d, dt, fl)      # noqa: E731
    for N, d in ((49, 512), (196, 512), (49, 2048)):                              # cfg 2 and cfg 4
        assert sup(82000, 160, N, d) == 1 and sup(82000, 160, N, d, _lib.BF16) == 1
    assert sup(1, 1, 1, 4) == 1 and sup(1, 1, 1, 8, _lib.BF16) == 1 and sup(1, 1, 4, 1) == 1 and sup(1, 1, 8, 1, _lib.BF16) == 1
    for N, d, f32, bf in ((1, 1, 0, 0), (1, 2, 0, 0), (1, 4, 1, 0), (3, 4, 1, 0), (2, 4, 1, 1), (1, 12, 1, 0), (3, 8, 1, 1), (7, 6, 0, 0)):
        assert sup(5, 3, N, d) == f32 and sup(5, 3, N, d, _lib.BF16) == bf, (N, d)
    for d, ok in ((0, 0), (-8, 0), (2048, 1), (2056, 0), (4096, 0)):
        assert sup(5, 3, 1, d) == ok, d
    for N, ok in ((0, 0), (-1, 0), (4096, 1), (4097, 0)):
        assert sup(5, 3, N, 8) == ok, N
    for B, ok in ((-1, 0), (0, 0), (1, 1), (65536, 1), (2 ** 24 - 1, 1), (2 ** 24, 0), (2 ** 32 + 1, 0)):
        assert sup(5, B, 1, 8) == ok, B
    assert sup(5, 8191, 4096, 2048) == 1 and sup(5, 8192, 4096, 2048) == 0       # B x passes per row stays below 2^24
    for S, ok in ((-1, 0), (0, 0), (1, 1), (2 ** 40, 1)):
        assert sup(S, 3, 1, 8) == ok, S
    assert sup(5, 3, 1, 8, 2) == 0 and sup(5, 3, 1, 8, -1) == 0 and sup(5, 3, 1, 8, _lib.F32, 1) == 0
    assert sup(5, 3, 1, 8, _lib.F32, _lib.FLAG_FAST16) == 0
    assert FT.supported(5, 3, 49, 512) and FT.supported(5, 3, 49, 512, torch.bfloat16) and not FT.supported(5, 3, 49, 512, torch.float16)


def test_every_argument_error_is_minus_one_with_a_message_before_any_device_work():
    """Made-up pointers: a call that went on to touch them would fault; each error names what is wrong."""
    fake = lambda i: 0x10000 * (i + 1)                          # noqa: E731  (16-byte aligned, never dereferenced)
    base = dict(table=fake(0), table_dtype=_lib.F32, idx=fake(1), idx_dtype=_lib.IDS_I64, out=fake(2), bad_idx=fake(3), S=5, B=3,
                N=3, d=8, flags=0, stream=None)

    def call(**kw):
        c = _lib.bind("coattn_features_gather", **{**base, **kw})
        return c.fn(*c)

    for kw, word in ((dict(table=None), "null"), (dict(idx=None), "null"), (dict(out=None), "null"),
                     (dict(S=0), "non-positive"), (dict(S=-2), "non-positive"), (dict(B=0), "non-positive"),
                     (dict(B=-1), "non-positive"), (dict(N=0), "non-positive"), (dict(d=0), "non-positive"),
                     (dict(d=-8), "non-positive"),
                     (dict(flags=1), "flags"), (dict(flags=_lib.FLAG_FAST16), "flags"), (dict(flags=_lib.FLAG_BF16_IN), "flags"),
                     (dict(table_dtype=2), "table dtype"), (dict(table_dtype=-1), "table dtype"),
                     (dict(idx_dtype=2), "idx_dtype"), (dict(idx_dtype=-1), "idx_dtype"),
                     (dict(N=1, d=6), "not supported"), (dict(N=3, d=4, table_dtype=_lib.BF16), "not supported"),
                     (dict(N=1, d=4, table_dtype=_lib.BF16), "not supported"), (dict(d=2052), "not supported"),
                     (dict(N=4097), "not supported"), (dict(B=2 ** 24), "not supported"),
                     (dict(table=fake(0) + 4), "aligned"), (dict(table=fake(0) + 8), "aligned"), (dict(out=fake(2) + 4), "aligned"),
                     (dict(idx=fake(1) + 4), "aligned"), (dict(idx=fake(1) + 2, idx_dtype=_lib.IDS_I32), "aligned"),
                     (dict(bad_idx=fake(3) + 2), "aligned")):
        assert call(**kw) == -1 and word in _err(), (kw, _err())
    # what is allowed: no counter, and int32 indices at any 4-byte address -- checked on a call that is refused further on, so
    # that the made-up pointers are never reached
    assert call(bad_idx=None, out=None) == -1 and "null" in _err()
    assert call(idx=fake(1) + 4, idx_dtype=_lib.IDS_I32, out=None) == -1 and "null" in _err()


# ---- FeatureTable ---------------------------------------------------------------------------------------------------------
def _table(dtype, S=6, N=4, d=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    data = torch.randn(S, N, d, generator=g)
    data[0, 0, :4] = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0])
    data = data.to(FT.DTYPES[dtype])
    return FT.FeatureTable(data, FT.make_meta("attention", 64, N, d, dtype, "train", 1234, S))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
def test_save_load_round_trip_is_bit_for_bit(tmp_path, dtype):
    tab = _table(dtype)
    path = str(tmp_path / "feats.npy")
    tab.save(path)
    arr = np.load(path)
    assert arr.dtype == (np.uint16 if dtype == "bf16" else np.float32) and arr.shape == (6, 4, 8)
    side = json.load(open(FT.sidecar_path(path)))
    assert FT.sidecar_path(path) == str(tmp_path / "feats.json")
    assert side == {"model": "attention", "image_size": 64, "N": 4, "d": 8, "grid": [2, 2], "dtype": dtype, "split": "train",
                    "seed": 1234, "S": 6, "encoder_stats": "running", "abi": FT.abi_version()}
    back = FT.FeatureTable.load(path, "cpu")
    assert back.data.dtype == FT.DTYPES[dtype] and back.meta == tab.meta and len(back) == 6
    assert torch.equal(_bits(back.data), _bits(tab.data))
    small = FT._COPY_BYTES
    try:                                                          # the copy in pieces: one row at a time
        FT._COPY_BYTES = 1
        again = FT.FeatureTable.load(path, "cpu")
    finally:
        FT._COPY_BYTES = small
    assert torch.equal(_bits(again.data), _bits(tab.data))


def test_a_table_and_sidecar_that_disagree_are_refused(tmp_path):
    tab = _table("fp32")
    path = str(tmp_path / "t.npy")
    tab.save(path)
    for field, value in (("S", 7), ("N", 5), ("d", 16), ("dtype", "bf16"), ("encoder_stats", "batch")):
        side = dict(tab.meta, **{field: value})
        json.dump(side, open(FT.sidecar_path(path), "w"))
        with pytest.raises(ValueError, match=field if field != "dtype" else "table"):
            FT.FeatureTable.load(path, "cpu")
    with pytest.raises(ValueError, match="fp32 or bfloat16"):
        FT.FeatureTable(torch.zeros(2, 2, 8, dtype=torch.float16), tab.meta)
    with pytest.raises(ValueError, match="dtype"):
        FT.make_meta("attention", 64, 4, 8, "fp16", "train", 1, 2)
    with pytest.raises(ValueError, match="split"):
        FT.make_meta("attention", 64, 4, 8, "fp32", "dev", 1, 2)
    assert FT.make_meta("attention", 64, 6, 8, "fp32", "val", 1, 2)["grid"] == [1, 6]


def test_check_names_each_mismatching_field():
    tab = _table("fp32")
    ok = dict(model_name="attention", image_size=64, split="train", seed=1234, S=6)
    tab.check(**ok)
    for field, key, value in (("model", "model_name", "attention_resnet"), ("image_size", "image_size", 448),
                              ("split", "split", "val"), ("seed", "seed", 1235), ("S", "S", 8)):
        with pytest.raises(ValueError, match=r"feature table: %s is " % field):
            tab.check(**dict(ok, **{key: value}))


# ---- the dataset without images ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (1234, 987654, P.TEST_SEED))
@pytest.mark.parametrize("num_answers", (0, 3))
def test_dataset_without_images_keeps_every_other_bit(seed, num_answers):
    full = T.SyntheticVQADataset(40, (8, 8), 26, 50, 11, seed, num_answers=num_answers)
    lean = T.SyntheticVQADataset(40, (8, 8), 26, 50, 11, seed, num_answers=num_answers, images=False)
    assert len(lean) == 40
    for i in (0, 1, 7, 39, 7):                                   # (7 twice: the second read comes from the memo)
        a, b = full[i], lean[i]
        assert a.keys() == b.keys() and a["image"].shape == (3, 8, 8)
        assert b["image"].dtype == torch.int64 and b["image"].shape == () and int(b["image"]) == i
        for k in a.keys() - {"image"}:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (i, k)
    batch = next(iter(torch.utils.data.DataLoader(lean, 4, shuffle=False)))
    assert batch["image"].tolist() == [0, 1, 2, 3]
    im, qu, la, ln = T.sort_batch(batch["image"], batch["question"], batch["label"], batch["ques_len"])
    assert sorted(im.tolist()) == [0, 1, 2, 3] and all(torch.equal(qu[j], full[int(im[j])]["question"]) for j in range(4))
    assert extract_seeds() == (1234, 1237, 987654, 987655, P.TEST_SEED, P.TEST_SEED)


def extract_seeds():
    return (X.split_seed("train"), X.split_seed("train", 3), X.split_seed("val"), X.split_seed("val", 1), X.split_seed("test"),
            X.split_seed("test", 5))


# ---- command lines ----------------------------------------------------------------------------------------------------------
def _args(*argv):
    return T.build_parser().parse_args(list(argv))


def test_the_flags_parse_in_the_three_clis():
    for mod in (T, P, X):
        a = mod.build_parser().parse_args([])
        assert a.image_features is None and a.val_image_features is None
        assert mod.build_parser().parse_args(["--image_features", "t.npy"]).image_features == "t.npy"
    a = X.build_parser().parse_args([])
    assert (a.split, a.samples, a.features_dtype, a.out) == ("train", 0, "fp32", None)
    a = X.build_parser().parse_args(["--split", "val", "--samples", "8", "--features_dtype", "bf16", "--out", "o.npy"])
    assert (a.split, a.samples, a.features_dtype, a.out) == ("val", 8, "bf16", "o.npy")
    for bad in (["--split", "dev"], ["--features_dtype", "fp16"]):
        with pytest.raises(SystemExit):
            X.build_parser().parse_args(bad)


def test_check_image_features_refusals():
    T.check_image_features(_args())                              # no table: nothing to check
    T.check_image_features(_args("--image_features", "t.npy"))
    T.check_image_features(_args("--image_features", "t.npy", "--val_image_features", "v.npy"), validates=True)
    T.check_image_features(_args("--image_features", "t{rank}.npy", "--val_image_features", "v{rank}.npy"), world=8, validates=True)
    for model in ("attention", "attention_resnet", "attention_bert"):
        T.check_image_features(_args("--model", model, "--image_features", "t.npy"))
    for argv, kw, word in ((["--image_features", "t.npy", "--vgg_train", "true"], {}, "--vgg_train"),
                           (["--image_features", "t.npy", "--model", "baseline"], {}, "co-attention models"),
                           (["--image_features", "t.npy", "--model", "bert"], {}, "co-attention models"),
                           (["--image_features", "t.npy"], dict(validates=True), "--val_image_features"),
                           (["--val_image_features", "v.npy"], {}, "needs --image_features"),
                           (["--image_features", "t.npy"], dict(world=2), "{rank}"),
                           (["--image_features", "t{rank}.npy", "--val_image_features", "v.npy"], dict(world=2, validates=True),
                            "--val_image_features with WORLD_SIZE")):
        with pytest.raises(ValueError, match=re.escape(word)):
            T.check_image_features(_args(*argv), **kw)


def test_train_cli_refuses_before_anything_is_built(monkeypatch):
    monkeypatch.setattr(T, "model_from_args", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a model was built")))
    for argv, word in ((["--image_features", "t.npy", "--vgg_train", "true"], "--vgg_train"),
                       (["--image_features", "t.npy", "--model", "baseline"], "co-attention models"),
                       (["--image_features", "t.npy", "--val_size", "16"], "--val_image_features"),
                       (["--image_features", "t.npy", "--val_batches", "2"], "--val_image_features")):
        with pytest.raises(SystemExit, match=re.escape(word)):
            T.main(argv)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match=re.escape("{rank}")):
        T.main(["--image_features", "t.npy"])


def test_predict_and_extract_clis_refuse(monkeypatch, tmp_path, capsys):
    monkeypatch.setattr(T, "model_from_args", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a model was built")))
    for argv, word in ((["--image_features", "t.npy", "--model", "baseline"], "co-attention models"),
                       (["--image_features", "t.npy", "--vgg_train", "true"], "--vgg_train"),
                       (["--image_features", "t.npy", "--val_image_features", "v.npy"], "--val_image_features")):
        with pytest.raises(SystemExit):
            P.main(["--model_ckpt", "x.pth"] + argv)
        assert word in capsys.readouterr().err
    for argv, word in ((["--model", "baseline", "--samples", "4", "--out", "o.npy"], "co-attention"),
                       (["--samples", "0", "--out", "o.npy"], "--samples"), (["--samples", "4"], "--out")):
        with pytest.raises(SystemExit):
            X.main(argv)
        assert word in capsys.readouterr().err


def test_trainer_methods_refuse_what_they_cannot_take():
    tr = T.Trainer(T.build_model("attention", 50, 10), 1e-4, torch.device("cpu"))
    with pytest.raises(ValueError, match="takes labels, not targets"):
        tr.step_features(torch.zeros(2, 4, 512), torch.zeros(2, 26, dtype=torch.int64), torch.tensor([3, 3]), torch.zeros(2, dtype=torch.int64),
                         targets=(None, None))

    class Plain(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Linear(2, 2)

    tr = T.Trainer(Plain(), 1e-4, torch.device("cpu"))
    with pytest.raises(ValueError, match="forward_features"):
        tr.step_features(None, None, None, None)
    with pytest.raises(ValueError, match="forward_features"):
        tr.validate([], features=True)


# ---- the CPU route of the gather ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
def test_gather_features_on_cpu_tensors_is_torch_indexing(dtype):
    tab = _table(dtype)
    idx = torch.tensor([5, 0, 0, 3])
    want = tab.data[idx].float()
    got = FT.gather_features(tab.data, idx)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(tab.gather(idx.to(torch.int32)).view(torch.int32), want.view(torch.int32))
    out = torch.empty(4, 4, 8)
    assert FT.gather_features(tab.data, idx, out) is out and torch.equal(out.view(torch.int32), want.view(torch.int32))
    for bad in (torch.tensor([6]), torch.tensor([-7])):
        with pytest.raises(IndexError):
            FT.gather_features(tab.data, bad)
    assert FT.bad_indices() == 0                                 # (the counter belongs to the device route)


def test_gather_features_refuses_a_table_with_grad_and_wrong_arguments():
    t = torch.randn(3, 2, 8)
    with pytest.raises(RuntimeError, match="requires grad"):
        FT.gather_features(t.clone().requires_grad_(True), torch.tensor([0]))
    for table, idx, out, word in ((t[0], torch.tensor([0]), None, "table"), (t.half(), torch.tensor([0]), None, "table"),
                                  (t, torch.tensor([0.0]), None, "integer idx"), (t, torch.tensor([[0]]), None, "integer idx"),
                                  (t, torch.tensor([True]), None, "integer idx"),
                                  (t, torch.tensor([0]), torch.empty(2, 2, 8), "`out`"),
                                  (t, torch.tensor([0]), torch.empty(1, 2, 8, dtype=torch.float64), "`out`")):
        with pytest.raises(RuntimeError, match=word):
            FT.gather_features(table, idx, out)
    assert not FT.gather_features(t, torch.tensor([1, 1])).requires_grad

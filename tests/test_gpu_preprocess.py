"""GPU: image preprocessing (csrc/preprocess.hip, include/coattn_ext.h v0.23.0, vqa_amd.preprocess, the file-data command
lines) -- the C-ABI against the numpy restatement of tests/_preprocess.py plus the lookup table, bit pattern for bit pattern, at
the smallest shapes that reach each branch; every buffer at its exact size inside marker-filled arenas; bad descriptors; the
Python layer against the C-ABI; train.py, extract.py and predict.py on a dataset written into tmp_path."""
import json

import numpy as np
import pytest
import torch

from vqa_amd import _lib, preprocess as PP

from tests import _preprocess as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROWS = R.constants()["ROWS"]
MIXED = ((37, 23), (5, 7), (28, 28), (1, 1), (23, 50))


def _same(got, want):
    want = R.bits_of(want)
    assert got.shape == want.shape
    assert np.array_equal(got, want), R.diff(got, want)


def _check(sizes, S, **kw):
    r = R.run_images(R.images(sizes), S, **kw)
    assert r["bad"] == 0
    _same(r["bits"], R.reference_of(tuple(sizes), S))
    return r


@pytest.mark.parametrize("h,w,S", ((37, 23, 14), (5, 7, 14), (28, 28, 28), (1, 1, 14), (1, 9, 14), (9, 1, 14)),
                         ids=lambda v: str(v))
def test_downscale_upscale_identity_and_one_pixel_sources(h, w, S):
    _check(((h, w),), S)


@pytest.mark.parametrize("align,lead", ((16, 0), (1, 0), (1, 1), (1, 2)))
def test_every_residue_of_a_row_start(align, lead):
    """Rows of 3 w bytes for 3 w mod 16 in {0, 3, 5, 9, 15, 1, 8}; packed back to back (align = 1) behind `lead` bytes, image
    and row starts take every residue."""
    widths = (16, 1, 7, 3, 5, 11, 8)
    assert sorted((3 * w) % 16 for w in widths) == [0, 1, 3, 5, 8, 9, 15]
    _check(tuple((6 + i, w) for i, w in enumerate(widths)), 14, align=align, lead=lead)


@pytest.mark.parametrize("S", (ROWS - 1, ROWS, ROWS + 1, 2 * ROWS, 2 * ROWS + 1))
def test_band_edges(S):
    _check(((50, 41), (7, 9)), S)


def _limit(S):
    lib = _lib.load()
    lo, hi = 1, R.constants()["MAX_IN"]
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if lib.coattn_preprocess_supported(1, S, mid, 2) else (lo, mid - 1)
    return lo


@pytest.mark.parametrize("S", (14, 28))
def test_the_largest_downscale_the_lds_takes_and_one_past_it(S):
    """S = 14: one band, the whole source in LDS; S = 28: two bands, each with a window of its own.  One row more is refused
    before any device work: nothing is written."""
    h = _limit(S)
    assert 2000 < h < R.constants()["MAX_IN"] and not _lib.load().coattn_preprocess_supported(1, S, h + 1, 2)
    _check(((h, 2),), S)
    imgs = R.images(((h + 1, 2),))
    r = R.run_images(imgs, S, expect_rc=-1)
    assert "not supported" in r["err"] and r["bad"] == 0
    assert (r["words"] == R.MARK_BITS).all()
    # the same image under a max_h the LDS takes: its descriptor is beyond the launch's limit -> a bad image, zeros
    r = R.run_images(imgs, S, max_h=h)
    assert r["bad"] == 1 and not r["bits"].any()


@pytest.mark.parametrize("sizes", (MIXED[:1], MIXED), ids=("B1", "B5"))
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_mixed_sizes_in_every_output_layout(layout, sizes):
    _check(sizes, 20, layout=layout)


def test_wider_tables_and_wider_limits_change_nothing():
    _check(MIXED, 20, extra_taps=3)
    _check(MIXED, 20, max_h=480, max_w=8192)


def test_the_counter_may_be_null_and_is_added_to():
    _check(MIXED[:2], 14, bad=False)
    r = R.run_images(R.images(MIXED[:2]), 14, bad_start=7)
    assert r["bad"] == 7


def test_two_calls_give_identical_bits():
    a, b = _check(MIXED, 20), _check(MIXED, 20)
    assert np.array_equal(a["bits"], b["bits"])


BAD = {"h = 0": dict(h=0), "w = 0": dict(w=0), "h < 0": dict(h=-3), "h above max_h": dict(h=38), "w above max_w": dict(w=51),
       "offset < 0": dict(offset=-16), "extent past the pixels": "extent", "offset past the pixels": dict(offset=1 << 40),
       "tab_x past the table": "tab_x", "tab_y < 0": dict(tab_y=-1), "taps_x = 0": dict(taps_x=0),
       "taps_y above the limit": dict(taps_y=R.constants()["MAX_TAPS"] + 1), "tab_y past the table": "tab_y"}


@pytest.mark.parametrize("kind", sorted(BAD))
def test_a_bad_descriptor_gives_a_zero_image_and_is_counted(kind):
    S, sizes = 20, ((37, 23), (23, 50), (28, 28))
    imgs = R.images(sizes)
    pixels, desc, coef = R.pack(imgs, S)
    want = R.reference_of(sizes, S).copy()
    edit, kw = BAD[kind], {}
    if edit == "extent":                                         # the last image's extent runs one byte past the buffer
        i, kw = 2, dict(pixel_bytes=pixels.size - 1)
    elif edit in ("tab_x", "tab_y"):                             # the table that lies last in coef ends one element past it
        i = int(np.argmax(desc[edit]))
        kw = dict(coef_count=coef.size - 1)
    else:
        i = 1
        for k, v in edit.items():
            desc[k][i] = v
    want[i] = 0
    r = R.run(pixels, desc, coef, S, 37, 50, bad_start=2, **kw)
    assert r["bad"] == 3
    _same(r["bits"], want)
    assert not r["bits"][i].any()                                # +0.0, every bit


def test_two_bad_images_in_channels_last():
    S, sizes = 14, MIXED
    pixels, desc, coef = R.pack(R.images(sizes), S)
    desc["w"][0], desc["offset"][4] = 0, pixels.size
    want = R.reference_of(sizes, S).copy()
    want[0] = want[4] = 0
    r = R.run(pixels, desc, coef, S, 37, 50, layout="nhwc")
    assert r["bad"] == 2
    _same(r["bits"], want)


def test_the_shipped_size_from_camera_shaped_sources():
    _check(((480, 640), (640, 480)), 224)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def test_image_preprocessor_equals_the_c_abi():
    S, sizes = 20, MIXED
    imgs = R.images(sizes)
    want = R.run_images(imgs, S)["bits"]
    pre = PP.ImagePreprocessor(S, device=DEV)
    assert np.array_equal(_bits(pre.lut), R.bits_of(R.lut()))
    out = pre(imgs)
    assert out.shape == (5, 3, S, S) and out.is_contiguous() and np.array_equal(_bits(out), want)
    cl = pre([torch.from_numpy(np.array(i)) for i in imgs], channels_last=True)
    assert cl.is_contiguous(memory_format=torch.channels_last) and np.array_equal(_bits(cl), want)
    big = torch.full((5, 4, S + 3, S + 5), float("nan"), device=DEV)
    view = big[:, 1:, 2:2 + S, 3:3 + S]
    assert pre(imgs, out=view) is view and np.array_equal(_bits(view), want)
    assert bool(torch.isnan(big[:, 0]).all()) and bool(torch.isnan(big[:, :, :2]).all()) and bool(torch.isnan(big[..., :3]).all())
    # an already packed batch, permuted by its descriptor rows: the pixels stay where they are
    packed = pre.pack(imgs)
    pix = packed.buf[packed.pix_off:].clone()
    order = torch.tensor([3, 0, 4, 2, 1])
    assert packed[order] is packed and packed.sizes == [sizes[i] for i in order.tolist()]
    assert torch.equal(packed.buf[packed.pix_off:], pix)
    assert np.array_equal(_bits(pre(packed)), want[order.numpy()])
    assert np.array_equal(_bits(pre.launch(packed.to(DEV))), want[order.numpy()])
    assert PP.bad_images() == 0
    # the host route gives the same bits (where Pillow is installed)
    try:
        host = PP.preprocess_host(imgs, S)
    except RuntimeError:
        host = None
    if host is not None:
        assert np.array_equal(_bits(host), want)


def test_the_hip_route_refuses_cpu_tensors_and_counts_bad_images():
    S = 14
    pre = PP.ImagePreprocessor(S, device=DEV)
    imgs = R.images(MIXED[:3])
    packed = pre.pack(imgs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pre.launch(packed)
    with pytest.raises(RuntimeError, match="out must be"):
        pre(imgs, out=torch.empty(3, 3, S, S))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.ImagePreprocessor(S, device="cpu")
    PP.bad_images()
    packed.desc()["h"][1] = 0
    out = pre(packed)
    want = R.reference_of(MIXED[:3], S).copy()
    want[1] = 0
    assert np.array_equal(_bits(out), R.bits_of(want))
    assert PP.bad_images() == 1 and PP.bad_images() == 0


# ---- end to end: the command lines on a dataset in tmp_path -----------------------------------------------------------------------
# 12 .npy images of four sizes, 24 lines (every image twice), a vocabulary with K = 4 answers; --image_size 64, --batch_size 4
S_E2E = 64


@pytest.fixture
def repeatable_convolutions():
    """MIOpen's deterministic solvers for the routes compared here (the default ones do not repeat their own bits: see
    tests/test_gpu_cached_features.py); where a route still differs from its own second run, that spread is the tolerance."""
    old, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    yield
    torch.backends.cudnn.deterministic = old


def _argv(fx, *more):
    return ["--synthetic", "false", "--model", "attention", "--num_cls", "4", "--image_size", str(S_E2E), "--batch_size", "4",
            "--vocab_file", fx["vocab_file"], *more]


def _train_argv(fx, *more):
    return _argv(fx, "--train_file", fx["data_file"], "--train_img", fx["img_dir"], *more)


def _records(capsys):
    return [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]


def _reference_images(fx, names):
    imgs = [np.load(fx["img_dir"] + "/" + n) for n in names]
    return torch.from_numpy(R.reference(imgs, S_E2E))


def _hand_steps(fx, argv, n_steps):
    """What train.main does for its first `n_steps` steps, spelled out on the restatement's images: the model of the command
    line from seed 0, the DataLoader's shuffle of seed 1234, batches sorted by question length, Trainer.step."""
    from vqa_amd import data as D, train as T
    args = T.build_parser().parse_args(argv)
    vocab = T.file_vocab(args)
    torch.manual_seed(0)
    model, _ = T.model_from_args(args)
    model.to(DEV)
    model.image_encoder.to(memory_format=torch.channels_last)
    tr = T.Trainer(model, args.learning_rate, DEV)
    ds = D.VQAFileDataset(fx["data_file"], fx["img_dir"], vocab)
    # (the batches' sample indices from a DataLoader of the same seed over the same lines, without their images)
    rows = D.VQAFileDataset(fx["data_file"], None, vocab, images="row")
    order = [b["index"].tolist() for b in T.file_loader(rows, args, shuffle=True, seed=1234, drop_last=True)]
    assert len(order) == 6 and sorted(i for b in order for i in b) == list(range(24)) and order[0] != [0, 1, 2, 3]
    losses = []
    for s in range(n_steps):
        idx = order[s]
        samples = [ds[i] for i in idx]
        image = _reference_images(fx, [fx["lines"][i][0] for i in idx])
        b = D.collate(samples)
        im, qu, la, ln = T.sort_batch(image, b["question"], b["label"], b["ques_len"])
        im = im.to(DEV).contiguous(memory_format=torch.channels_last)
        losses.append(float(tr.step(im, qu.to(DEV), ln, la.to(DEV))))
    return losses


def test_train_on_files_takes_the_steps_written_out_by_hand(tmp_path, capsys, repeatable_convolutions):
    """Two steps of `train.py --synthetic false` (the prefetcher copies the packed pixels and queues the HIP launch on its side
    stream) against Trainer.step on the restatement's images.  The log rounds a loss to 5 decimals (5e-6); beyond that the CLI
    may differ from the hand-written steps by what those differ from their own second run."""
    from vqa_amd import train as T
    fx = R.write_fixture(str(tmp_path))
    argv = _train_argv(fx, "--log_interval", "1", "--num_epochs", "1")
    T.main(argv)
    recs = _records(capsys)
    assert recs[0]["data"] == "files" and recs[0]["preprocess"] == "hip" and recs[0]["steps_per_epoch"] == 6
    cli = [r["loss"] for r in recs if "loss" in r]
    assert len(cli) == 6
    first, second = _hand_steps(fx, argv, 2), _hand_steps(fx, argv, 2)
    print("train on files: cli", cli[:2], "by hand", first, second)
    for c, a, b in zip(cli, first, second):
        assert abs(c - a) <= 5.1e-6 + abs(a - b), (cli, first, second)
    assert PP.bad_images() == 0


def test_extract_train_from_the_table_and_predict(tmp_path, capsys, monkeypatch, repeatable_convolutions):
    from vqa_amd import extract as X, features as FT, predict as P, train as T
    from vqa_amd.coattention import native_features
    fx = R.write_fixture(str(tmp_path))
    table = str(tmp_path / "train_feats.npy")
    meta = X.main(_train_argv(fx, "--split", "train", "--out", table))
    names = [n for i, n in enumerate(l[0] for l in fx["lines"]) if n not in [m[0] for m in fx["lines"][:i]]]
    assert meta["source"] == "files" and meta["images"] == meta["S"] == 12 and len(names) == 12
    tab = FT.FeatureTable.load(table, DEV)
    tab.check_files("attention", S_E2E, "train", names)
    # one row per distinct image, in first-seen order: the encoder (eval mode, batches of 4 as the extractor ran) on the
    # restatement's image; compared within what the encoder differs from its own second pass (nothing, on these solvers)
    args = T.build_parser().parse_args(_train_argv(fx))
    T.file_vocab(args)
    torch.manual_seed(0)
    model, _ = T.model_from_args(args)
    model.to(DEV).eval()
    model.image_encoder.to(memory_format=torch.channels_last)
    image = _reference_images(fx, names).to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        passes = [torch.cat([native_features(model.image_encoder(image[i:i + 4])) for i in range(0, 12, 4)]) for _ in range(2)]
    spread = float((passes[0] - passes[1]).abs().max())
    print("extract on files: spread of two encoder passes", spread, "table against them", float((tab.data - passes[0]).abs().max()))
    assert tab.data.shape == passes[0].shape and float((tab.data - passes[0]).abs().max()) <= spread
    # train.py --image_features on that table: rows, never an image file, never the encoder in the step
    capsys.readouterr()
    monkeypatch.setattr(T.Trainer, "step", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the image route ran")))
    run = _argv(fx, "--train_file", fx["data_file"], "--image_features", table, "--log_interval", "1")
    T.main(run)
    recs = _records(capsys)
    losses = [r["loss"] for r in recs if "loss" in r]
    assert recs[0]["preprocess"].startswith("none") and len(losses) == 6 and all(np.isfinite(x) and x > 0 for x in losses)
    # a table of another file list is refused before the first step, and the message names the field
    other = str(tmp_path / "other.txt")
    open(other, "w").write("".join("\t".join(l) + "\n" for l in fx["lines"][2:]))
    monkeypatch.setattr(T.Trainer, "step_features", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a step ran")))
    with pytest.raises(ValueError, match="feature table: names_sha256 is"):
        T.main(_argv(fx, "--train_file", other, "--image_features", table))
    monkeypatch.undo()
    # predict.py on the files: answers as strings
    ckpt, preds = str(tmp_path / "net.pth"), str(tmp_path / "preds.jsonl")
    torch.manual_seed(0)
    torch.save(T.model_from_args(args)[0].state_dict(), ckpt)
    summary = P.main(_argv(fx, "--test_file", fx["data_file"], "--test_img", fx["img_dir"], "--model_ckpt", ckpt, "--predictions",
                           preds, "--topk", "3"))
    recs = [json.loads(line) for line in open(preds)]
    assert summary["samples"] == 24 and len(recs) == 24
    labels = set(fx["vocab"]["label2idx"])
    for i, r in enumerate(recs):
        name, question, _ = fx["lines"][i]
        assert r["index"] == i and r["image"] == name and r["question"] == [w for w in r["question"] if w] and len(r["answers"]) == 3
        assert set(r["answers"]) <= labels and r["answers"] == [fx["vocab"]["idx2label"][t] for t in r["top"]]
    assert recs[0]["question"] == ["what", "color", "is", "the", "cat"]
    assert PP.bad_images() == 0

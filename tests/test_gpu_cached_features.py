"""GPU: cached image features (csrc/features.hip, include/coattn.h v0.20.0, vqa_amd.features / extract, Trainer.step_features,
--image_features) -- the gather's C-ABI against the numpy oracle of tests/_features.py bit for bit, the Python layer against
the C-ABI, the extractor against the encoder it caches, the trainer's cached step against hand-written steps, and the evaluation
routes (validate, predict.py) on a table against the same routes on images."""
import copy
import json

import numpy as np
import pytest
import torch

from vqa_amd import extract as X, features as FT, predict as P, train as T
from vqa_amd.coattention import native_features
from vqa_amd.dropout import rank_seed

from tests import _features as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SMALL = ["--num_cls", "10", "--image_size", "64", "--vocab_size", "50"]      # the sizes tests/test_gpu_net.py runs the encoder at


# ---- the C-ABI against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: "S%d_B%d_N%d_d%d" % s)
@pytest.mark.parametrize("kind", ("int32", "int64"))
@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
def test_gather_is_table_of_idx_bit_for_bit(dtype, kind, shape):
    S, B, N, d = shape
    bits, idx = F.table_bits(dtype, S, N, d), F.indices(S, B)
    want, n_bad = F.oracle(bits, idx, dtype)
    r = F.run(bits, idx, dtype, kind)
    assert n_bad == 0 and r["bad"] == 0 and F.same(r["out"], want)


@pytest.mark.parametrize("over", (-1, 0, 1), ids=("one_vector_under_a_pass", "a_pass", "one_vector_over_a_pass"))
@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
def test_rows_at_the_edge_of_a_workgroup_pass(dtype, over):
    """A row of exactly the elements one workgroup copies (COATTN_FEATURES_THREADS x COATTN_FEATURES_LOADS 16-byte vectors), one
    16-byte vector less and one more: the last takes a second workgroup with a single live lane."""
    vec = F.TABLE[dtype][2]
    row = F.pass_elements(dtype) + over * vec
    S, B, N, d = 3, 4, row // vec, vec
    assert N * d == row and N <= 4096
    bits, idx = F.table_bits(dtype, S, N, d, seed=1), np.array([2, 0, 1, 2])
    r = F.run(bits, idx, dtype, "int32")
    assert r["bad"] == 0 and F.same(r["out"], F.oracle(bits, idx, dtype)[0])


@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
def test_repeated_indices(dtype):
    bits, idx = F.table_bits(dtype, 5, 3, 8), np.array([2, 2, 0, 2, 0, 4, 4])
    r = F.run(bits, idx, dtype)
    assert r["bad"] == 0 and F.same(r["out"], F.oracle(bits, idx, dtype)[0])
    assert F.same(r["out"][0], r["out"][1]) and F.same(r["out"][0], r["out"][3])


@pytest.mark.parametrize("kind", ("int32", "int64"))
@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
def test_indices_outside_the_table_give_zero_rows_and_an_exact_count(dtype, kind):
    S, N, d = 7, 49, 64
    bits = F.table_bits(dtype, S, N, d)
    bad = [-1, S] + ([2 ** 32 + 1, -2 ** 40, 2 ** 63 - 1] if kind == "int64" else [2 ** 31 - 1, -2 ** 31])
    idx = []
    for k, b in enumerate(bad):                                  # every bad index between two good neighbours
        idx += [k % S, b]
    idx = np.array(idx + [S - 1], dtype=np.int64)
    want, n_bad = F.oracle(bits, idx, dtype)
    assert n_bad == len(bad)
    r = F.run(bits, idx, dtype, kind)
    assert r["bad"] == n_bad and F.same(r["out"], want)
    assert not r["out"][1::2].any() and all(r["out"][j].any() for j in range(0, len(idx), 2))     # +0 rows; the neighbours live
    assert F.same(F.run(bits, idx, dtype, kind, bad=False)["out"], want)                             # the counter may be NULL


def test_special_bit_patterns_come_out_with_their_bits():
    f32 = np.array([0x7fc00000, 0x7fc00001, 0xffc12345, 0x7f800001, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x80000000,
                    0x00000000, 0x7f7fffff, 0x00800000], dtype=np.uint32)
    bf = np.array([0x7fc0, 0x7fc1, 0xffff, 0x7f81, 0x7f80, 0xff80, 0x0001, 0x807f, 0x8000, 0x0000, 0x7f7f, 0x0080, 0x3f80, 0xbf80,
                   0x7fff, 0x0040], dtype=np.uint16)
    for dtype, pat in (("fp32", f32), ("bf16", bf)):
        bits = np.stack([pat.reshape(1, -1), pat[::-1].reshape(1, -1)])            # [2, 1, d]
        idx = np.array([1, 0, 1])
        r = F.run(bits, idx, dtype)
        want = F.oracle(bits, idx, dtype)[0]
        assert F.same(r["out"], want)
        if dtype == "bf16":
            assert int(want[1, 0, 2]) == 0xffff0000 and int(want[1, 0, 6]) == 0x00010000


def test_offsets_past_two_to_the_31_elements():
    """A bf16 table of 85,600 rows of 25,088 elements: 2.147e9 elements (past 2^31) and 4.295e9 bytes (past 2^32).  Only the first
    and the last row are written; both are gathered, with a bad index between them."""
    S, N, d = 85600, 49, 512
    assert S * N * d > 2 ** 31 and 2 * S * N * d > 2 ** 32
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < 6e9:
        pytest.skip("%.1f GB of device memory free; the 64-bit-offset case takes 4.3 GB (needs 6 GB)" % (free / 1e9))
    table = torch.empty((S, N, d), dtype=torch.bfloat16, device=DEV)
    g = torch.Generator().manual_seed(3)
    first, last = torch.randn(N, d, generator=g).to(torch.bfloat16), torch.randn(N, d, generator=g).to(torch.bfloat16)
    table[0], table[S - 1] = first.to(DEV), last.to(DEV)
    out = FT.gather_features(table, torch.tensor([S - 1, S, 0], device=DEV))
    torch.cuda.synchronize()
    del table
    assert FT.bad_indices() == 1
    assert F.same(out[0].cpu(), last.float()) and F.same(out[2].cpu(), first.float()) and not out[1].view(torch.int32).any()


# ---- the Python layer against the C-ABI runner --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("int32", "int64"))
@pytest.mark.parametrize("dtype", ("fp32", "bf16"))
def test_gather_features_and_the_table_have_the_runners_bits(dtype, kind):
    S, B, N, d = 7, 33, 49, 64
    bits = F.table_bits(dtype, S, N, d)
    idx = F.indices(S, B).copy()
    idx[[3, 20]] = [S, -1]
    r = F.run(bits, idx, dtype, kind)
    host = torch.from_numpy(bits.view(np.int16 if dtype == "bf16" else np.int32).copy())
    data = host.view(torch.bfloat16 if dtype == "bf16" else torch.float32).to(DEV)
    assert FT.bad_indices() == 0
    tidx = torch.from_numpy(idx).to(F.IDX[kind][0]).to(DEV)
    got = FT.gather_features(data, tidx)
    assert got.dtype == torch.float32 and got.shape == (B, N, d) and F.same(got, r["out"])
    assert FT.bad_indices() == 2 and FT.bad_indices() == 0      # read and reset
    tab = FT.FeatureTable(data, FT.make_meta("attention", 224, N, d, dtype, "train", 1234, S))
    out = torch.full((B, N, d), float("nan"), device=DEV)
    assert tab.gather(tidx, out) is out and F.same(out, r["out"]) and FT.bad_indices() == 2
    assert F.same(tab.gather(tidx.to(torch.int16)), r["out"]) and FT.bad_indices() == 2        # another integer type is cast
    with pytest.raises(RuntimeError, match="requires grad"):
        FT.gather_features(data.float().clone().requires_grad_(True), tidx)
    with pytest.raises(RuntimeError, match="not supported"):
        FT.gather_features(torch.zeros(2, 1, 6, device=DEV), tidx)                            # no quiet other route
    with pytest.raises(RuntimeError, match="contiguous"):
        FT.gather_features(data.float().transpose(1, 2), tidx)


def test_load_puts_the_table_on_the_device_and_refuses_one_that_does_not_fit(tmp_path, monkeypatch):
    data = torch.randn(6, 4, 8).to(torch.bfloat16)
    tab = FT.FeatureTable(data, FT.make_meta("attention", 64, 4, 8, "bf16", "val", 987654, 6))
    path = str(tmp_path / "t.npy")
    tab.save(path)
    dev = FT.FeatureTable.load(path, DEV)
    assert dev.data.device == DEV and torch.equal(dev.data.cpu().view(torch.int16), data.view(torch.int16))
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a: (100, 1000))
    with pytest.raises(RuntimeError, match=r"holds 384 bytes.* 100 bytes free \(of 1000\)"):
        FT.FeatureTable.load(path, DEV)


# ---- the extractor ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def repeatable_convolutions():
    """The image routes the tables are compared with run their convolutions on MIOpen's deterministic solvers, as the extractor
    does.  On the default solvers the eval-mode encoder does not repeat its own bits (measured on an MI355X at 64 px, batch 4
    and 8, six passes over one batch: 47 % of the feature elements differ between two passes, by up to 1.1e-8 at a scale of
    2.5e-2, from the third convolution on; Trainer.validate's loss over the same 16 samples came out as 2.403187870979309 and
    2.4031877517700195), so no route could be held to it exactly; on the deterministic ones six passes are identical,
    whatever the order of the samples inside the batch."""
    old, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    yield
    torch.backends.cudnn.deterministic = old


def _eval_model(argv, ckpt=None):
    """The model as train.py / extract.py build it for `argv`, on the GPU with a channels_last encoder, in eval mode."""
    args = T.build_parser().parse_args(argv)
    torch.manual_seed(0)
    model, _ = T.model_from_args(args)
    if ckpt:
        model.load_state_dict(torch.load(ckpt, map_location="cpu"))
    model.to(DEV)
    model.image_encoder.to(memory_format=torch.channels_last)
    return model.eval()


def _first_diff(a, b):
    d = (a.float() - b.float()).abs()
    return "max |a - b| = %.3e over %d differing elements of %d" % (float(d.max()), int((a != b).sum()), a.numel())


def test_extractor_writes_the_eval_mode_encoders_features(tmp_path, capsys, repeatable_convolutions):
    argv = ["--model", "attention", "--batch_size", "4"] + SMALL
    paths = {}
    for dtype in ("fp32", "bf16"):
        paths[dtype] = str(tmp_path / (dtype + ".npy"))
        meta = X.main(argv + ["--split", "train", "--samples", "8", "--features_dtype", dtype, "--out", paths[dtype]])
        assert (meta["S"], meta["N"], meta["d"], meta["grid"], meta["split"], meta["seed"], meta["dtype"], meta["image_size"]) \
            == (8, 4, 512, [2, 2], "train", 1234, dtype, 64)
    capsys.readouterr()
    model = _eval_model(argv)
    ds = T.SyntheticVQADataset(8, (64, 64), 26, 50, 11, 1234)
    want = []
    with torch.no_grad():
        for b in torch.utils.data.DataLoader(ds, 4, shuffle=False):
            x = b["image"].to(DEV).contiguous(memory_format=torch.channels_last)
            want.append(native_features(model.image_encoder(x)).clone())
    want = torch.cat(want)
    f32 = FT.FeatureTable.load(paths["fp32"], DEV)
    bf = FT.FeatureTable.load(paths["bf16"], DEV)
    f32.check("attention", 64, "train", 1234, 8)
    print("extractor fp32:", _first_diff(f32.data, want), "| bf16:", _first_diff(bf.data, want.to(torch.bfloat16)))
    assert f32.data.shape == (8, 4, 512) and float(want.abs().max()) > 0
    assert torch.equal(f32.data, want)
    assert torch.equal(bf.data.view(torch.int16), want.to(torch.bfloat16).view(torch.int16))


# ---- the trainer --------------------------------------------------------------------------------------------------------------
def _running_means(net):
    return [m.running_mean.clone() for m in net.image_encoder.modules() if isinstance(m, torch.nn.BatchNorm2d)]


@pytest.mark.parametrize("route", ("defaults", "hip"))
def test_three_cached_steps_are_three_hand_written_steps(route):
    """Trainer.step_features on rows gathered from a table against forward_features(table[idx].float(), labels=...) ->
    zero_grad -> backward -> the same optimiser on a second model with equal initial weights (and the hot-path switches the
    Trainer sets): the same loss bits every step, every parameter equal afterwards, and the image encoder never ran."""
    hip = route == "hip"
    torch.manual_seed(0)
    net0 = T.build_model("attention", 100, 10)
    g = torch.Generator().manual_seed(11)
    table = torch.randn(12, 4, 512, generator=g).to(DEV)         # 64 px: a 2 x 2 grid
    tab = FT.FeatureTable(table, FT.make_meta("attention", 64, 4, 512, "fp32", "train", 1234, 12))
    ds = T.SyntheticVQADataset(12, (64, 64), 26, 100, 11, 1234, images=False)
    batches = []
    for b in torch.utils.data.DataLoader(ds, 4, shuffle=False):
        idx, qu, la, ln = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
        batches.append((idx.to(DEV), qu.to(DEV), ln, la.to(DEV)))
    assert len(batches) == 3

    net_a = copy.deepcopy(net0).to(DEV)
    kw = dict(sentence_lstm="hip", word_embedding="hip", optimizer="hip", feature_dropout=0.5) if hip else {}
    tr = T.Trainer(net_a, 1e-4, DEV, **kw)
    before = _running_means(net_a)
    assert len(before) == 8
    net_a.image_encoder.register_forward_hook(lambda *a: (_ for _ in ()).throw(AssertionError("the image encoder ran")))
    losses_a = [tr.step_features(tab.gather(idx), qu, ln, la).detach().clone() for idx, qu, ln, la in batches]

    net_b = copy.deepcopy(net0).to(DEV)
    net_b.hot_path_static, net_b.hot_path_direct_grads = net_a.hot_path_static, net_a.hot_path_direct_grads
    if hip:
        from vqa_amd.optim import HipAdam
        T.set_sentence_lstm(net_b, "hip")
        T.set_word_embedding(net_b, "hip")
        T.set_feature_dropout(net_b, 0.5, rank_seed(0, 0))
        opt = HipAdam(net_b.parameters(), 1e-4)
    else:
        opt = torch.optim.Adam(net_b.parameters(), 1e-4)
    losses_b = []
    for idx, qu, ln, la in batches:
        _, loss = net_b.forward_features(table[idx].float(), qu, ln, labels=la)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses_b.append(loss.detach().clone())
    torch.cuda.synchronize()
    print("cached steps", route, [float(x) for x in losses_a], [float(x) for x in losses_b])
    for a, b in zip(losses_a, losses_b):
        assert torch.isfinite(a) and F.same(a.reshape(1), b.reshape(1))
    assert losses_a[0] != losses_a[2]
    for (name, p), q in zip(net_a.named_parameters(), net_b.parameters()):
        assert torch.equal(p, q), name
    for x, y in zip(before, _running_means(net_a)):
        assert torch.equal(x, y)
    assert FT.bad_indices() == 0


# ---- evaluation: a table against images -----------------------------------------------------------------------------------------
def _checkpoint(tmp_path):
    torch.manual_seed(5)
    ckpt = str(tmp_path / "net.pth")
    torch.save(T.build_model("attention", 50, 10).state_dict(), ckpt)
    return ckpt


def test_validate_on_a_table_is_validate_on_the_images(tmp_path, capsys, repeatable_convolutions):
    """Trainer.validate over image batches and validate(..., features=True) over the fp32 rows the extractor wrote for the same
    samples, same batch partition and order.  The image route is run twice first: where it repeats its own results exactly
    (on the deterministic solvers the encoder in eval mode is a fixed function at a fixed batch shape: `repeatable_convolutions`)
    the table route must equal it exactly; where it does not, the table route must lie within the spread of the two image runs."""
    ckpt = _checkpoint(tmp_path)
    argv = ["--model", "attention", "--batch_size", "8", "--model_ckpt", ckpt] + SMALL
    path = str(tmp_path / "val.npy")
    X.main(argv + ["--split", "val", "--samples", "16", "--out", path])
    capsys.readouterr()
    model = _eval_model(argv, ckpt)
    tr = T.Trainer(model, 1e-4, DEV)
    tab = FT.FeatureTable.load(path, DEV)
    tab.check("attention", 64, "val", 987654, 16)
    images, rows = [], []
    for kind, out in ((True, images), (False, rows)):
        ds = T.SyntheticVQADataset(16, (64, 64), 26, 50, 11, 987654, images=kind)
        for b in torch.utils.data.DataLoader(ds, 8, shuffle=False):
            im, qu, la, ln = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
            im = im.to(DEV).contiguous(memory_format=torch.channels_last) if kind else tab.gather(im.to(DEV))
            out.append((im, qu.to(DEV), ln, la.to(DEV)))
    first, second = tr.validate(images), tr.validate(images)
    cached = tr.validate(rows, features=True)
    print("validate: images", first, "images again", second, "table", cached)
    assert FT.bad_indices() == 0 and model.training
    for k in first:
        spread = abs(first[k] - second[k])
        assert abs(cached[k] - first[k]) <= spread, (k, first, second, cached)      # (spread 0: exact equality)


def test_predict_writes_the_same_files_from_a_table(tmp_path, capsys, repeatable_convolutions):
    """predict.py on images (twice) and on the extractor's fp32 table of the test split: the same JSONL text and the same
    maps.npz arrays -- exactly where the image route repeats itself (`repeatable_convolutions`), else within the spread of its
    two runs (on the default solvers two image runs gave probabilities 1.5e-8 apart)."""
    ckpt = _checkpoint(tmp_path)
    argv = ["--model", "attention", "--batch_size", "8", "--model_ckpt", ckpt] + SMALL
    path = str(tmp_path / "test.npy")
    X.main(argv + ["--split", "test", "--samples", "16", "--out", path])
    got = {}
    for run, extra in (("images", []), ("again", []), ("table", ["--image_features", path])):
        preds, maps = str(tmp_path / (run + ".jsonl")), str(tmp_path / (run + ".npz"))
        summary = P.main(argv + ["--test_size", "16", "--predictions", preds, "--attention_maps", maps] + extra)
        z = np.load(maps)
        got[run] = (open(preds).read(), {k: z[k] for k in z.files}, summary)
    capsys.readouterr()
    assert got["table"][2]["samples"] == 16 and sorted(got["table"][1]) == ["a_q", "a_v", "index", "ques_len"]
    repeatable = got["images"][0] == got["again"][0] and all(np.array_equal(got["images"][1][k], got["again"][1][k])
                                                             for k in got["images"][1])
    print("predict: the image route repeats itself:", repeatable)
    if repeatable:
        assert got["table"][0] == got["images"][0]
        for k, v in got["images"][1].items():
            assert np.array_equal(got["table"][1][k], v), k
        return
    for k, v in got["images"][1].items():
        spread = np.abs(v.astype(np.float64) - got["again"][1][k]).max()
        assert np.abs(v.astype(np.float64) - got["table"][1][k]).max() <= spread, (k, spread)
    recs = {run: [json.loads(line) for line in got[run][0].splitlines()] for run in got}
    for a, b, c in zip(recs["images"], recs["again"], recs["table"]):
        assert (a["index"], a["label"]) == (c["index"], c["label"])
        spread = max(abs(x - y) for x, y in zip(a["prob"], b["prob"]))
        assert max(abs(x - y) for x, y in zip(a["prob"], c["prob"])) <= spread, (a, b, c)


def test_predict_refuses_a_table_of_another_split(tmp_path, capsys):
    ckpt = _checkpoint(tmp_path)
    argv = ["--model", "attention", "--batch_size", "8", "--model_ckpt", ckpt] + SMALL
    tab = FT.FeatureTable(torch.zeros(16, 4, 512), FT.make_meta("attention", 64, 4, 512, "fp32", "val", 987654, 16))
    tab.save(str(tmp_path / "val.npy"))
    with pytest.raises(SystemExit):
        P.main(argv + ["--test_size", "16", "--image_features", str(tmp_path / "val.npy")])
    assert "split is 'val'" in capsys.readouterr().err


# ---- train.py --image_features --------------------------------------------------------------------------------------------------
def test_train_cli_runs_from_tables_and_refuses_a_table_of_another_run(tmp_path, capsys, monkeypatch):
    argv = ["--model", "attention", "--batch_size", "4"] + SMALL
    train, val = str(tmp_path / "train.npy"), str(tmp_path / "val.npy")
    X.main(argv + ["--split", "train", "--samples", "16", "--out", train])
    X.main(argv + ["--split", "val", "--samples", "8", "--features_dtype", "bf16", "--out", val])
    capsys.readouterr()
    run = argv + ["--num_steps", "4", "--log_interval", "1", "--image_features", train]
    monkeypatch.setattr(T.Trainer, "step", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the image route ran")))
    T.main(run + ["--val_image_features", val, "--val_batches", "2", "--val_interval", "4"])
    lines = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    losses = [rec["loss"] for rec in lines if "loss" in rec]
    assert len(losses) == 4 and all(np.isfinite(x) and x > 0 for x in losses)
    assert [rec for rec in lines if "val_loss" in rec] and np.isfinite([rec for rec in lines if "val_loss" in rec][0]["val_loss"])
    # a sidecar of another split, and of another number of samples: refused before the first step
    monkeypatch.setattr(T.Trainer, "step_features", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a step ran")))
    side = json.load(open(FT.sidecar_path(train)))
    for field, value in (("split", "val"), ("S", 12)):
        json.dump(dict(side, **{field: value}), open(FT.sidecar_path(train), "w"))
        with pytest.raises(ValueError, match=("feature table: %s is " % field) if field == "split" else r"\bS\b"):
            T.main(run)
    json.dump(side, open(FT.sidecar_path(train), "w"))
    with pytest.raises(ValueError, match="feature table: S is 16"):
        T.main(argv + ["--num_steps", "3", "--image_features", train])

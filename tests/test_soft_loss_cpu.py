"""Soft answer targets (include/coattn.h v0.12.0) without a GPU: the C-ABI declarations, exports and argument errors, the
synthetic answers (which must not disturb a bit of the existing keys), the stock-op fallback of ``SoftTargetLoss`` against the
float64 oracle of tests/_soft_loss.py, and the command lines."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from oracle import coattn_oracle as O
from tests import _soft_loss as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "coattn.h")
NEW = ("coattn_soft_loss_forward", "coattn_vqa_score", "coattn_head_forward_soft")
COMMON = ["--num_cls", "4", "--batch_size", "4", "--image_size", "64", "--vocab_size", "50", "--max_seq_length", "8"]


def test_header_declares_exports_and_version():
    from vqa_amd import _lib
    hdr = open(HDR).read()
    for fn in NEW:
        assert re.search(r"\bint %s\(" % fn, hdr), fn
        assert fn in _lib.EXPORTS
    assert re.search(r"#define COATTN_LOSS_SOFT_CE 1\b", hdr) and re.search(r"#define COATTN_LOSS_BCE 2\b", hdr)
    assert (_lib.LOSS_SOFT_CE, _lib.LOSS_BCE) == (SL.SOFT_CE, SL.BCE) == (1, 2)
    lib = C.CDLL(_lib.LIB_PATH)
    for fn in NEW:
        assert hasattr(lib, fn), fn
    assert _lib.load().coattn_version() >= 1200
    # the header states that the hard-label backward / status serve the soft forward
    assert "coattn_head_backward and coattn_head_status serve both unchanged" in hdr


def test_argument_errors_return_before_any_device_work():
    """A outside 1..16, an unknown kind and NULL pointers are -1 with a message; nothing is launched (no GPU here)."""
    from vqa_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(64)                      # any non-NULL address: the checks come first, nothing dereferences it
    def soft(A=10, kind=1, logits=one, idx=one, sc=one, loss=one, ws=one):
        return lib.coattn_soft_loss_forward(logits, idx, sc, A, kind, loss, None, ws, 4, 7, _lib.F32, None)
    for bad in (dict(A=0), dict(A=17), dict(A=-3)):
        assert soft(**bad) == -1 and b"1..16" in lib.coattn_last_error()
    for bad in (dict(kind=0), dict(kind=3)):
        assert soft(**bad) == -1 and b"kind" in lib.coattn_last_error()
    for bad in (dict(logits=None), dict(idx=None), dict(sc=None), dict(loss=None), dict(ws=None)):
        assert soft(**bad) == -1 and b"null" in lib.coattn_last_error()
    assert lib.coattn_soft_loss_forward(one, one, one, 10, 1, one, None, one, 0, 7, _lib.F32, None) == -1

    def score(A=10, logits=one, idx=one, sc=one, pred=one, total=one, ws=one):
        return lib.coattn_vqa_score(logits, idx, sc, A, pred, None, total, ws, 4, 7, _lib.F32, None)
    assert score(A=0) == -1 and score(A=17) == -1 and b"1..16" in lib.coattn_last_error()
    for bad in (dict(logits=None), dict(idx=None), dict(sc=None), dict(pred=None), dict(total=None), dict(ws=None)):
        assert score(**bad) == -1 and b"null" in lib.coattn_last_error()

    rows = (C.c_void_p * 3)(64, 64, 64)
    hp = _lib.HeadParams(*([64] * 8))
    def head(A=10, kind=2, idx=one, sc=one, loss=one, flags=0):
        return lib.coattn_head_forward_soft(rows, rows, C.byref(hp), idx, sc, A, kind, one, loss, one, 4, 32, 32, 7, _lib.F32,
                                            flags, None)
    assert head(A=17) == -1 and b"1..16" in lib.coattn_last_error()
    assert head(kind=5) == -1 and b"kind" in lib.coattn_last_error()
    assert head(idx=None) == -1 and head(sc=None) == -1 and head(loss=None) == -1
    assert head(flags=1 | _lib.FLAG_BF16_PROJ) == -1 and b"COATTN_HEAD_PERSISTENT" in lib.coattn_last_error()


@pytest.mark.parametrize("seed", [1, 7, 1234])
def test_synthetic_answers_leave_the_existing_keys_bit_identical(seed):
    from vqa_amd import train as T
    K, A = 11, 10
    a = T.synthetic_batch(6, (8, 8), 12, 100, K, seed=seed)
    b = T.synthetic_batch(6, (8, 8), 12, 100, K, seed=seed, num_answers=A)
    assert set(a) == {"image", "question", "ques_len", "label"} and set(b) == set(a) | {"answers", "answer_scores"}
    for k in a:
        assert torch.equal(a[k], b[k]), k
    idx, sc = b["answers"], b["answer_scores"]
    assert idx.dtype == torch.int32 and sc.dtype == torch.float32 and tuple(idx.shape) == tuple(sc.shape) == (6, A)
    assert torch.equal(idx[:, 0].long(), b["label"]) and bool((sc[:, 0] == 1.0).all())
    assert int(idx.min()) >= -1 and int(idx.max()) < K and bool((idx == -1).any())
    allowed = torch.tensor(T.ANSWER_SCORES)
    assert bool(torch.isin(sc[idx >= 0], allowed).all()) and bool((sc[idx < 0] == 0).all())
    # the dataset form: per-sample [A] vectors, the four keys of every index unchanged
    d0 = T.SyntheticVQADataset(5, (8, 8), 12, 100, K, seed)
    d1 = T.SyntheticVQADataset(5, (8, 8), 12, 100, K, seed, num_answers=A)
    for i in range(5):
        s0, s1 = d0[i], d1[i]
        for k in s0:
            assert torch.equal(s0[k], s1[k]), (i, k)
        assert tuple(s1["answers"].shape) == (A,) and s1["answers"].dtype == torch.int32
        assert int(s1["answers"][0]) == int(s1["label"]) and float(s1["answer_scores"][0]) == 1.0
        assert int(s1["answers"].min()) >= -1 and int(s1["answers"].max()) < K


@pytest.mark.parametrize("kind", ["soft_ce", "bce"])
def test_cpu_fallback_equals_the_oracle_in_float64(kind):
    from vqa_amd.loss import SoftTargetLoss
    B, K, A = 37, 101, 10
    idx, sc = SL.make_targets(B, K, A, seed=5)
    assert bool((idx == -1).all(1).any()) and bool((idx[:, 0] == idx[:, 1]).any())     # empty rows and duplicates are in
    for scale in (0.5, 3.0, 30.0):
        z = torch.from_numpy(O.hash_normal((B, K), 3, scale))
        ref, gref = SL.loss_and_grad(z, idx, sc, kind, upstream=2.5)
        zg = z.clone().requires_grad_(True)
        got = SoftTargetLoss(kind)(zg, idx, sc)
        (2.5 * got).backward()
        assert got.dtype == torch.float64
        assert abs(got.item() - ref.item()) <= 1e-12 * max(1.0, abs(ref.item()))
        assert (zg.grad - gref).abs().max().item() <= 1e-12
    # the anchor: one-hot targets make the soft cross entropy the reference's cross entropy
    lab = torch.from_numpy((O.hash_uniform(B, 4) * K).astype("int64")).clamp_(0, K - 1)
    z = torch.from_numpy(O.hash_normal((B, K), 6, 3.0))
    if kind == "soft_ce":
        ce = torch.nn.functional.cross_entropy(z, lab)
        assert abs(SoftTargetLoss(kind)(z, *SL.one_hot_targets(lab, 3)).item() - ce.item()) <= 1e-12
    # a NaN in an empty slot's score is not read; a huge logit stays finite
    sc2 = sc.clone()
    sc2[idx < 0] = float("nan")
    z[0, 5] = 8.0e4
    assert torch.equal(SoftTargetLoss(kind)(z, idx, sc2), SoftTargetLoss(kind)(z, idx, sc))
    assert bool(torch.isfinite(SoftTargetLoss(kind)(z, idx, sc)))
    with pytest.raises(ValueError):
        SoftTargetLoss("hinge")
    bad = idx.clone()
    bad[3, 2] = K
    with pytest.raises(IndexError):
        SoftTargetLoss(kind)(z, bad, sc)


def test_cpu_vqa_score_follows_the_oracle():
    from vqa_amd.loss import vqa_score
    B, K, A = 23, 17, 6
    idx, sc = SL.make_targets(B, K, A, seed=9)
    z = torch.from_numpy(O.hash_normal((B, K), 8, 2.0)).float()
    z[2, 4] = z[2, 9] = z[2].max() + 1.0            # a tie: the first index wins
    pred, rows, mean = vqa_score(z, idx, sc)
    p_ref, r_ref, m_ref = SL.score(z, idx, sc)
    assert pred.tolist() == p_ref.tolist() and int(pred[2]) == 4
    assert torch.equal(rows, r_ref.float()) and abs(float(mean) - float(m_ref)) < 1e-6


def test_command_lines_parse_loss_and_refuse_labels_with_targets():
    from vqa_amd import predict as Pr
    from vqa_amd import train as T
    from vqa_amd.modules import MLPClassifier
    ap = T.build_parser()
    assert ap.parse_args([]).loss == "ce" and ap.parse_args([]).num_answers == 10
    for kind in ("ce", "soft_ce", "bce"):
        assert ap.parse_args(["--loss", kind]).loss == kind
        assert Pr.build_parser().parse_args(["--loss", kind, "--num_answers", "4"]).num_answers == 4
    with pytest.raises(SystemExit):
        ap.parse_args(["--loss", "hinge"])
    with pytest.raises(ValueError, match="num_answers"):
        T.check_loss("bce", 17)
    with pytest.raises(ValueError):
        T.Trainer(T.build_model("baseline", 20, 3), loss="hinge")
    head = MLPClassifier(8, 8, 5)
    v = [torch.randn(2, 8) for _ in range(3)]
    tg = SL.one_hot_targets(torch.tensor([1, 2]), 3)
    with pytest.raises(ValueError, match="labels or targets"):
        head.forward_loss(v, v, torch.tensor([1, 2]), targets=tg)
    from vqa_amd.head import answer_head
    with pytest.raises(ValueError, match="not both"):
        answer_head(v, v, *head._params(), labels=torch.tensor([1, 2]), targets=tg)
    net = T.build_model("attention", 20, 4)
    with pytest.raises(ValueError, match="not both"):
        net.forward_features(torch.zeros(2, 4, 512), torch.ones(2, 3, dtype=torch.long), torch.tensor([3, 3]),
                             labels=torch.tensor([1, 2]), targets=tg)
    # the stock head on CPU tensors takes targets too (loss = the stock-op formula)
    logits, loss = head.forward_loss(v, v, targets=tg, loss_kind="bce")
    assert abs(loss.item() - SL.loss(logits.detach().double(), *tg, "bce").item()) < 1e-5
    # a soft-target trainer needs targets, a label trainer refuses them
    tr = T.Trainer(T.build_model("baseline", 20, 3), loss="soft_ce")
    b = T.synthetic_batch(2, (64, 64), 6, 20, 4, seed=1, num_answers=3)
    im, qu, la, ln, ai, sc = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"], b["answers"], b["answer_scores"])
    with pytest.raises(ValueError, match="targets"):
        tr.step(im, qu, ln, la)
    with pytest.raises(ValueError, match="labels, not targets"):
        T.Trainer(T.build_model("baseline", 20, 3)).step(im, qu, ln, la, targets=(ai, sc))


@pytest.mark.parametrize("kind", ["soft_ce", "bce"])
def test_baseline_trains_validates_and_predicts_on_the_cpu(kind, tmp_path, capsys):
    from vqa_amd import predict as Pr
    from vqa_amd import train as T
    ckpt = str(tmp_path / "m.pth")
    T.main(["--model", "baseline", "--num_steps", "2", "--log_interval", "1", "--save_path", ckpt, "--loss", kind,
            "--num_answers", "5", "--val_batches", "1", "--val_interval", "2"] + COMMON)
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines() if l.startswith("{")]
    steps = [l for l in lines if "loss" in l]
    assert len(steps) == 2 and all(l["loss"] == l["loss"] and l["loss"] > 0 for l in steps)
    val = [l for l in lines if "val_loss" in l]
    assert len(val) == 1 and 0.0 <= val[0]["val_vqa_score"] <= 1.0
    S = 6
    preds = str(tmp_path / "p.jsonl")
    summary = Pr.main(["--model", "baseline", "--model_ckpt", ckpt, "--test_size", str(S), "--topk", "2", "--loss", kind,
                       "--num_answers", "5", "--predictions", preds] + COMMON)
    recs = [json.loads(l) for l in open(preds)]
    assert len(recs) == S and all(0.0 <= r["score"] <= 1.0 for r in recs)
    assert summary["vqa_score"] == pytest.approx(sum(r["score"] for r in recs) / S, abs=1e-5)
    ds = T.SyntheticVQADataset(S, (64, 64), 8, 50, 5, Pr.TEST_SEED, num_answers=5)
    for i, r in enumerate(recs):                                     # score = min(1, target of the top answer)
        s = ds[i]
        t = SL.dense(s["answers"][None], s["answer_scores"][None], 5)[0]
        assert r["score"] == pytest.approx(min(1.0, float(t[r["top"][0]])), abs=1e-6)
        if kind == "bce":
            assert all(0.0 < p < 1.0 for p in r["prob"])

"""predict.py (inference of a trained checkpoint, with the co-attention maps) and the C-ABI's coattn_infer, on the CPU:
the baseline model end to end, the command line's refusals, and the library's declaration / export / version."""
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COMMON = ["--num_cls", "4", "--batch_size", "4", "--image_size", "64", "--vocab_size", "50", "--max_seq_length", "8"]


def _train_baseline(tmp_path, capsys):
    from vqa_amd import train as T
    ckpt = str(tmp_path / "baseline.pth")
    T.main(["--model", "baseline", "--num_steps", "2", "--log_interval", "1", "--save_path", ckpt] + COMMON)
    capsys.readouterr()
    return ckpt


def test_predict_baseline_records_summary_and_plain_forward(tmp_path, capsys):
    from vqa_amd import predict as Pr
    from vqa_amd import train as T
    ckpt = _train_baseline(tmp_path, capsys)
    S = 10                                                    # (two full batches and a partial one: drop_last=False)
    preds = str(tmp_path / "preds.jsonl")
    summary = Pr.main(["--model", "baseline", "--model_ckpt", ckpt, "--test_size", str(S), "--topk", "3",
                       "--predictions", preds] + COMMON)
    line = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines() if l.startswith("{")]
    assert line == [summary]
    assert set(summary) == {"samples", "accuracy", "top3_accuracy", "loss", "pairs_per_s"} and summary["samples"] == S
    recs = [json.loads(l) for l in open(preds)]
    assert sorted(r["index"] for r in recs) == list(range(S))            # every sample once, in dataset order
    assert [r["index"] for r in recs] == list(range(S))
    for r in recs:
        assert len(r["top"]) == 3 and len(set(r["top"])) == 3
        p = r["prob"]
        assert all(0.0 < x <= 1.0 for x in p) and p == sorted(p, reverse=True) and sum(p) <= 1.0 + 1e-6
    hit1 = sum(r["top"][0] == r["label"] for r in recs) / S
    hitk = sum(r["label"] in r["top"] for r in recs) / S
    assert summary["accuracy"] == pytest.approx(100.0 * hit1, abs=1e-3)
    assert summary["top3_accuracy"] == pytest.approx(100.0 * hitk, abs=1e-3) and hitk >= hit1
    # a plain model(...) pass over the same samples, in dataset order, one at a time (no sorting needed)
    args = T.build_parser().parse_args(["--model", "baseline"] + COMMON)
    torch.manual_seed(0)
    model, _ = T.model_from_args(args)
    model.load_state_dict(torch.load(ckpt, map_location="cpu"))
    model.eval()
    ds = T.SyntheticVQADataset(S, (64, 64), 8, 50, 5, Pr.TEST_SEED)
    ok = 0
    losses = []
    with torch.no_grad():
        for i in range(S):
            s = ds[i]
            logits = model(s["image"][None], s["question"][None], s["ques_len"][None])
            ok += int(int(logits.argmax(1)) == int(s["label"]))
            losses.append(float(torch.nn.functional.cross_entropy(logits, s["label"][None])))
            assert int(s["label"]) == recs[i]["label"]
    assert summary["accuracy"] == pytest.approx(100.0 * ok / S, abs=1e-3)
    assert summary["loss"] == pytest.approx(sum(losses) / S, rel=1e-4, abs=1e-5)


def test_predict_refuses_without_checkpoint_and_maps_of_baseline(tmp_path, capsys):
    from vqa_amd import predict as Pr
    with pytest.raises(SystemExit) as e:
        Pr.main(["--model", "baseline", "--test_size", "4"] + COMMON)
    assert e.value.code == 2 and "--model_ckpt" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        Pr.main(["--model", "baseline", "--model_ckpt", str(tmp_path / "x.pth"), "--attention_maps",
                 str(tmp_path / "m.npz")] + COMMON)
    assert e.value.code == 2 and "--attention_maps" in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "m.npz")


def test_predict_refuses_multi_process(tmp_path, capsys, monkeypatch):
    from vqa_amd import predict as Pr
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        Pr.main(["--model", "baseline", "--model_ckpt", str(tmp_path / "x.pth")] + COMMON)
    assert e.value.code == 2 and "one process" in capsys.readouterr().err


def test_c_abi_declares_and_exports_coattn_infer():
    from vqa_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "coattn.h")).read()
    assert re.search(r"\bint\s+coattn_infer\s*\(", hdr)
    assert "coattn_infer" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "coattn_infer")
    assert lib.coattn_version() >= 700

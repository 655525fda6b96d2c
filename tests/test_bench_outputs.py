"""bench.py's plain run and --dump-outputs: the headline line alone, exactly --steps timed steps, and the arrays of the last
timed step written within their budget, the same positions from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Wide(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.big = torch.nn.Parameter(torch.randn(4096, 2048, generator=g))
        self.small = torch.nn.Parameter(torch.randn(7, generator=g))
        self.frozen = torch.nn.Parameter(torch.randn(5000), requires_grad=False)
        self.big.grad = torch.randn(4096, 2048, generator=g)
        self.small.grad = torch.randn(7, generator=g)


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 40 * 2 ** 20)        # below the 64 MiB of the whole set: forces the sample
    m = _Wide()
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), m, torch.tensor(2.5))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grad.big.npy", "grad.small.npy", "loss.npy", "param.big.npy", "param.small.npy"]
    total = sum(os.path.getsize(tmp_path / "a" / n) for n in names)
    assert total <= 40 * 2 ** 20 + 1024 * len(names)
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b), n
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == 2.5
    assert np.array_equal(np.load(tmp_path / "a" / "param.small.npy"), m.small.detach().numpy())       # small: whole
    big = np.load(tmp_path / "a" / "param.big.npy")
    assert big.ndim == 1 and 0.3 * m.big.numel() < big.size < 0.7 * m.big.numel()
    assert np.isin(big, m.big.detach().numpy().reshape(-1)).all()
    # under the budget nothing is sampled and shapes are kept
    bench.dump_outputs(str(tmp_path / "c"), torch.nn.Linear(3, 2), torch.tensor(1.0))
    assert np.load(tmp_path / "c" / "param.weight.npy").shape == (2, 3)


def _seed_files():
    import bench
    return sorted(f for f in os.listdir(bench.MIOPEN_DB_SEED) if f.endswith(".txt"))


def test_miopen_seed_goes_to_the_user_database_not_the_repository(tmp_path, monkeypatch):
    import bench
    assert _seed_files()
    before = sorted(os.listdir(ROOT))
    # MIOpen's default user database under the home directory
    monkeypatch.delenv("MIOPEN_USER_DB_PATH", raising=False)
    monkeypatch.setenv("HOME", str(tmp_path / "home"))
    bench.seed_miopen_db()
    assert "MIOPEN_USER_DB_PATH" not in os.environ
    db = tmp_path / "home" / ".config" / "miopen"
    assert sorted(os.listdir(db)) == _seed_files()
    for f in _seed_files():
        assert (db / f).read_bytes() == open(os.path.join(bench.MIOPEN_DB_SEED, f), "rb").read()
    # a chosen user database; a record file already there is left as it is
    own = tmp_path / "own"
    own.mkdir()
    (own / _seed_files()[0]).write_text("mine\n")
    monkeypatch.setenv("MIOPEN_USER_DB_PATH", str(own))
    bench.seed_miopen_db()
    assert os.environ["MIOPEN_USER_DB_PATH"] == str(own) and (own / _seed_files()[0]).read_text() == "mine\n"
    assert sorted(os.listdir(ROOT)) == before


def test_miopen_seed_falls_back_to_a_temporary_database(tmp_path, monkeypatch):
    import bench
    blocker = tmp_path / "not_a_dir"
    blocker.write_text("")
    monkeypatch.delenv("MIOPEN_USER_DB_PATH", raising=False)
    monkeypatch.delenv("MIOPEN_CUSTOM_CACHE_DIR", raising=False)
    monkeypatch.setenv("HOME", str(blocker))            # ~/.config/miopen cannot be created
    bench.seed_miopen_db()
    d = os.environ["MIOPEN_USER_DB_PATH"]
    try:
        assert not d.startswith(ROOT) and sorted(os.listdir(d)) == _seed_files()
        assert os.environ["MIOPEN_CUSTOM_CACHE_DIR"] == os.path.join(d, "cache")
    finally:
        import shutil
        shutil.rmtree(d, ignore_errors=True)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_bench_line_steps_and_dump(tmp_path):
    out_dir = tmp_path / "out"
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    # a fresh child: the test process has touched the GPU and must not exec or fork into GPU work itself
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "16", "--dump-outputs", str(out_dir)], env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=500, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "QA-pairs/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["metric"].startswith("QA-pairs/sec") and out["ms_per_step"] > 0
    assert abs(out["value"] - 16 / (out["ms_per_step"] * 1e-3)) < 0.01 * out["value"]
    for k in ("value_fast16", "roofline", "hot_path", "config4", "config5", "cpu_baseline"):      # --full only
        assert k not in out, k
    names = os.listdir(out_dir)
    assert "loss.npy" in names and "grad.co_attention.W_v.weight.npy" in names and "param.mlp_classify.W_h.weight.npy" in names
    assert sum(os.path.getsize(out_dir / n) for n in names) <= 64 * 10 ** 6
    loss = np.load(out_dir / "loss.npy")
    assert loss.dtype == np.float32 and np.isfinite(loss).all() and loss[0] > 0
    g = np.load(out_dir / "grad.co_attention.W_v.weight.npy")
    assert np.isfinite(g).all() and np.abs(g).max() > 0

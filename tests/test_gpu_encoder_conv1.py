"""The frozen encoder's first convolution (3 -> 64 channels, 3x3, padding 1) with its BatchNorm statistics riding along
(include/coattn.h v0.16.0, csrc/encoder.hip conv1_stats_miopen_kernel, vqa_amd/encoder.py conv1_bn_exact_or_stock): the values
against float64 within the bound of a 28-term fp32 chain, the statistics bit for bit against coattn_bn_exact_forward on the
kernel's own x, the stock convolution's bits at the benchmark's shape, and the route."""
import copy
import ctypes as C
import functools
import os
import subprocess
import sys
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-5, 0.1
BENCH = (160, 224, 224)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda:0")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))


# ---- the shape list, from the geometry rule -----------------------------------------------------------------------------------
# (g: the BatchNorm geometry of the convolution's output; the kernel's wave owns 32 consecutive pixels whatever g1 is)
PROPERTIES = {
    "a pixel group wraps an image row (W not a multiple of g1)": lambda g, B, H, W: W % g["g1"] != 0 and H >= 2 and H * W > g["g1"],
    "a masked tail of pixels": lambda g, B, H, W: (H * W) % g["g1"] != 0,
    "whole pixel groups of the last wave lie past the end": lambda g, B, H, W: 1 <= (H * W) % 32 <= 32 - g["g1"],
    "every pixel on the border (H = W = 2)": lambda g, B, H, W: H == 2 and W == 2,
    "odd H and odd W": lambda g, B, H, W: H % 2 == 1 and W % 2 == 1 and H >= 3 and W >= 3,
    "g1 = 8": lambda g, B, H, W: g["g1"] == 8,
    "g1 = 16": lambda g, B, H, W: g["g1"] == 16,
    "one sample (nothing to prefetch)": lambda g, B, H, W: B == 1,
    "three samples": lambda g, B, H, W: B == 3,
    "more than one workgroup": lambda g, B, H, W: H * W > 32,
}


@functools.lru_cache(maxsize=None)
def shape_list():
    """For each property the covered (B, H, W) of smallest B H W that has it, B in {1, 2, 3}, candidates in order of B H W, then
    B, then H.  H, W <= 48 -- except for g1 = 16: at 64 channels MIOpen's geometry has it from H W = 2560 on, above 48 x 48,
    so that property alone looks up to 64 (found: 1 x 40 x 64, 655 KB of output)."""
    from vqa_amd import encoder
    shapes = []
    for name, has in PROPERTIES.items():
        top = 65 if name == "g1 = 16" else 49
        cands = sorted((B * H * W, B, H, W) for B in (1, 2, 3) for H in range(1, top) for W in range(H, top))
        for _, B, H, W in cands:
            g = encoder.exact_geometry(B, H, W, 64)
            if g is not None and H >= 2 and has(g, B, H, W):
                if (B, H, W) not in shapes:
                    shapes.append((B, H, W))
                break
        else:
            raise AssertionError(name)
    return tuple(shapes)


def test_the_shape_list_has_every_property():
    from vqa_amd import _lib, encoder
    shapes = shape_list()
    for name, has in PROPERTIES.items():
        assert any(has(encoder.exact_geometry(B, H, W, 64), B, H, W) for B, H, W in shapes), name
    lib = _lib.load()
    assert all(lib.coattn_conv1_bn_exact_supported(B, H, W, 3, 64, 1, _lib.F32) == 1 for B, H, W in shapes)
    assert all(B * H * W * 64 * 4 <= 2 ** 21 for B, H, W in shapes)


# ---- inputs and the raw call ----------------------------------------------------------------------------------------------------
KINDS = ("normal", "mixed magnitude", "subnormal", "near 1e19", "NaN and inf", "negative zero")


def _inputs(shape, kind, seed):
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, 3, H, W, generator=g)
    w = torch.randn(64, 3, 3, 3, generator=g) * 0.2
    if kind == "mixed magnitude":
        img *= 10.0 ** torch.randint(-4, 5, img.shape, generator=g).float()
        w *= 10.0 ** torch.randint(-2, 3, w.shape, generator=g).float()
    elif kind == "subnormal":
        img *= 1e-41
        w *= 5.0
    elif kind == "near 1e19":
        img *= 1e19
    elif kind == "NaN and inf":
        img[0, 1, 0, 0] = float("nan")
        img[B - 1, 2, H - 1, W - 1] = float("inf")
        img[B // 2, 0, H // 2, 1] = float("-inf")
    elif kind == "negative zero":
        img[:, :, ::2] = -0.0
        w[::2] = -w[::2].abs()
        w[5] = -0.0
    return _cl(img.to(_dev())), _cl(w.to(_dev()))


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [t.to(_dev()) for t in (0.5 + torch.rand(64, generator=g), 0.5 * torch.randn(64, generator=g),
                                   torch.randn(64, generator=g), 0.5 + torch.rand(64, generator=g))]


def _raw(img, w, params, pool):
    """(x, y, running_mean, running_var, save_mean, save_invstd) of coattn_conv1_bn_exact_forward on clones of the statistics."""
    from vqa_amd import encoder
    gamma, beta, rm, rv = params
    rm, rv = rm.clone(), rv.clone()
    x, y, mean, invstd = encoder._conv1_raw(img, w, gamma, beta, rm, rv, MOMENTUM, EPS, pool, True)
    return x, y, rm, rv, mean, invstd


# ---- values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("normal", "mixed magnitude", "near 1e19"))
def test_values_against_float64(kind):
    """|x - ref| <= 28 * 2^-24 * sum |w v| per element: the bound of a 28-term fp32 chain of fused multiply-adds (each step rounds
    once, by at most 2^-24 of a partial sum that never exceeds sum |w v|)."""
    for n, shape in enumerate(shape_list()):
        img, w = _inputs(shape, kind, 10 + n)
        x = _raw(img, w, _params(n), False)[0]
        ref = F.conv2d(img.double(), w.double(), None, 1, 1)
        mag = F.conv2d(img.double().abs(), w.double().abs(), None, 1, 1)
        err = (x.double() - ref).abs()
        bound = 28 * 2.0 ** -24 * mag
        worst = float((err / bound.clamp_min(1e-300)).max())
        print("conv1 %s %s: max err / bound = %.3f" % (kind, shape, worst))
        assert bool((err <= bound).all()), (kind, shape, worst)
        assert x.is_contiguous(memory_format=torch.channels_last)


def test_x_in_the_workspace_is_the_same_x():
    """x_out = NULL keeps x in the workspace: y and the statistics are those of the call that returns x."""
    from vqa_amd import encoder
    for shape in shape_list()[:3]:
        img, w = _inputs(shape, "normal", 3)
        gamma, beta, rm, rv = _params(4)
        want = _raw(img, w, (gamma, beta, rm, rv), True)
        rm1, rv1 = rm.clone(), rv.clone()
        _, y, mean, invstd = encoder._conv1_raw(img, w, gamma, beta, rm1, rv1, MOMENTUM, EPS, True, False)
        for a, b in zip((y, rm1, rv1, mean, invstd), want[1:]):
            assert torch.equal(a, b), shape


# ---- the statistics ride along: bit for bit, on every shape -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_statistics_are_bn_exact_on_the_kernels_own_x(kind):
    from vqa_amd import encoder
    for n, shape in enumerate(shape_list()):
        img, w = _inputs(shape, kind, 30 + n)
        for pool in (True, False):
            params = _params(50 + n)
            x, y, rm, rv, mean, invstd = _raw(img, w, params, pool)
            gamma, beta, rm0, rv0 = params
            rm0, rv0 = rm0.clone(), rv0.clone()
            want_y, want_mean, want_invstd = encoder._bn_exact_raw(x, gamma, beta, rm0, rv0, MOMENTUM, EPS, pool)
            for name, a, b in (("y", y, want_y), ("running_mean", rm, rm0), ("running_var", rv, rv0), ("save_mean", mean, want_mean),
                               ("save_invstd", invstd, want_invstd)):
                assert _same(a, b), (kind, shape, pool, name)
            if kind == "NaN and inf":
                assert torch.isnan(x).any() and torch.isnan(mean).any()


def test_guard_bands():
    """x, y and the workspace carved out of larger buffers filled with a marker: not a word outside them changes, every word of
    x and y is written."""
    from vqa_amd import _lib
    lib = _lib.load()
    for shape in shape_list():
        B, H, W = shape
        img, w = _inputs(shape, "normal", 5)
        gamma, beta, rm, rv = _params(6)
        nx, ny, nws, pad, marker = B * 64 * H * W, B * 64 * (H // 2) * (W // 2), lib.coattn_conv1_bn_exact_workspace_bytes(B, H, W, 0) // 4, 4096, 12345.5
        big = [torch.full((pad + n + pad,), marker, device=_dev()) for n in (nx, ny, nws)]
        save = torch.full((2, 64), marker, device=_dev())
        big[0][pad:pad + nx] = float("nan")
        big[1][pad:pad + ny] = float("nan")
        rc = lib.coattn_conv1_bn_exact_forward(_lib.ptr(img), _lib.ptr(w), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(rm), _lib.ptr(rv),
                                               MOMENTUM, EPS, _lib.ptr(big[0][pad:]), _lib.ptr(big[1][pad:]), _lib.ptr(save[0]),
                                               _lib.ptr(save[1]), _lib.ptr(big[2][pad:]), B, H, W, 3, 64, 1, _lib.F32,
                                               C.c_void_p(_lib.stream_ptr(img.device)))
        _lib.check(rc, "coattn_conv1_bn_exact_forward")
        torch.cuda.synchronize()
        for b, n in zip(big, (nx, ny, nws)):
            assert (b[:pad] == marker).all() and (b[pad + n:] == marker).all(), shape
        assert not torch.isnan(big[0]).any() and not torch.isnan(big[1]).any() and not (save == marker).any(), shape


# ---- the stock bits where the benchmark needs them ----------------------------------------------------------------------------------
def _first_group(seed=0, pool=True):
    torch.manual_seed(seed)
    mods = [torch.nn.Conv2d(3, 64, 3, padding=1), torch.nn.BatchNorm2d(64, eps=EPS, momentum=MOMENTUM), torch.nn.ReLU(inplace=True)]
    if pool:
        mods.append(torch.nn.MaxPool2d(2, 2))
    return torch.nn.Sequential(*mods).to(_dev()).to(memory_format=torch.channels_last).requires_grad_(False)


def _default_env(monkeypatch):
    """The default switches -- and deterministic convolution algorithms, as tests/test_gpu_encoder_exact.py sets them: two runs of
    the stock kernels are comparable bit for bit only then."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    for name in ("VQA_ENCODER_FUSED", "VQA_ENCODER_EXACT_BN", "VQA_ENCODER_EXACT_CONV1", "VQA_ENCODER_REWRITE"):
        monkeypatch.delenv(name, raising=False)


def _forget(monkeypatch):
    from vqa_amd import encoder
    monkeypatch.setattr(encoder, "_exact", {})


class _Spy:
    def __init__(self, monkeypatch, name):
        from vqa_amd import encoder
        self.calls, real = 0, getattr(encoder, name)

        def counted(*a, **k):
            self.calls += 1
            return real(*a, **k)
        monkeypatch.setattr(encoder, name, counted)

    def take(self):
        n, self.calls = self.calls, 0
        return n


def _bench_shape_check():
    """Runs in a process of its own (below): 160 x 3 x 224 x 224 under the benchmark's own MIOpen find records."""
    import bench
    bench.seed_miopen_db()
    from vqa_amd import encoder
    from vqa_amd.modules import run_conv_bn_stack
    for name in ("VQA_ENCODER_FUSED", "VQA_ENCODER_EXACT_BN", "VQA_ENCODER_EXACT_CONV1", "VQA_ENCODER_REWRITE"):
        os.environ.pop(name, None)
    B, H, W = BENCH
    calls, real = [0], encoder._conv1_raw

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    def take():
        n, calls[0] = calls[0], 0
        return n
    encoder._conv1_raw = counted
    seq = _first_group(1)
    stock = copy.deepcopy(seq)
    g = torch.Generator(device=_dev()).manual_seed(7)
    img = _cl(torch.randn(B, 3, H, W, device=_dev(), generator=g))
    with torch.no_grad():
        z = F.conv2d(img, seq[0].weight, None, 1, 1)
        x = _raw(img, seq[0].weight, [seq[1].weight, seq[1].bias, seq[1].running_mean, seq[1].running_var], True)[0]
        assert torch.equal(x, z), "x is not the stock convolution's: %d elements differ" % int((x != z).sum())
        del x, z
        take()
        os.environ["VQA_ENCODER_EXACT_CONV1"] = "0"
        wants = [run_conv_bn_stack(stock, img) for _ in range(3)]
        assert take() == 0
        del os.environ["VQA_ENCODER_EXACT_CONV1"]
        first = run_conv_bn_stack(seq, img)                                  # compares
        state = encoder.exact_report()[(0, B, 64, H, W, True)]
        assert state["verified"] and state["conv1"] == {"verified": True, "first_difference": None}, state
        assert take() == 1 and torch.equal(first, wants[0])
        del first
        second = run_conv_bn_stack(seq, img)                                 # the route
        assert take() == 1 and torch.equal(second, wants[1])
        del second
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            third = run_conv_bn_stack(seq, img)
        side.synchronize()
        assert take() == 1 and torch.equal(third, wants[2])
    for k, v in seq.state_dict().items():
        assert torch.equal(v, stock.state_dict()[k]), k
    assert int(seq[1].num_batches_tracked) == 3
    print("bench shape ok")


def _bench_trainer_check():
    """Runs in the same process of its own, behind _bench_shape_check (the shape is verified by then): three Trainer steps at
    the benchmark's image shape with the route on and off.  Every convolution shape of the run is in the seeded find records, so
    MIOpen's solvers are the same in both runs."""
    from vqa_amd import encoder
    from vqa_amd import train as T
    from vqa_amd.modules import HierarchicalCoAttentionNet
    B, H, W = BENCH
    dev = _dev()
    calls, real = [0], encoder._conv1_raw

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    encoder._conv1_raw = counted
    qp = dict(vocab_size=60, word_emb_dim=512, hidden_dim=512)
    torch.manual_seed(3)
    net0 = HierarchicalCoAttentionNet(qp, dict(is_trainable=False, weights_path=None), K=11)
    batches = []
    for s in range(3):
        b = T.synthetic_batch(B, (H, W), 26, 60, 11, seed=70 + s)
        image, question, label, lens = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
        batches.append((_cl(image.to(dev)), question.to(dev), lens, label.to(dev)))
    runs = {}
    for route in ("0", "1"):
        os.environ["VQA_ENCODER_EXACT_CONV1"] = route
        net = copy.deepcopy(net0).to(dev)
        net.image_encoder.to(memory_format=torch.channels_last)
        tr = T.Trainer(net, 1e-3, dev)
        losses, per_step = [], []
        for i, bt in enumerate(batches):
            nxt = batches[i + 1][0] if i + 1 < len(batches) else None
            losses.append(tr.step(*bt, next_image=nxt).detach().clone())
            torch.cuda.synchronize()
            per_step.append(calls[0])
        runs[route] = (torch.stack(losses).cpu(), {k: v.detach().cpu() for k, v in net.state_dict().items()})
        # one encoder pass per batch, each through the binding when the route is on (the shape was verified above; a batch's
        # pass may run a step ahead)
        assert (per_step == [0, 0, 0]) if route == "0" else (per_step[0] >= 1 and per_step[2] == 3), (route, per_step)
        calls[0] = 0
    del os.environ["VQA_ENCODER_EXACT_CONV1"]
    state = encoder.exact_report()[(0, B, 64, H, W, True)]["conv1"]
    assert state == {"verified": True, "first_difference": None}, state
    assert torch.equal(runs["1"][0], runs["0"][0]), (runs["1"][0].tolist(), runs["0"][0].tolist())
    for k, v in runs["0"][1].items():
        assert _same(runs["1"][1][k].float(), v.float()), k
    print("bench trainer ok")


@functools.lru_cache(maxsize=None)
def _bench_process(db_dir):
    """One process of its own for both checks at the benchmark's shape, 160 x 3 x 224 x 224 -- the one shape at which MIOpen's
    solver is the benchmark's, so its MIOpen user database is a fresh directory holding the benchmark's find records
    (bench.seed_miopen_db), as a benchmark run on a clean machine has it; in the suite's own process MIOpen would choose by
    whatever records earlier tests left."""
    env = dict(os.environ, MIOPEN_USER_DB_PATH=db_dir)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--bench-shape"], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    return r.stdout


def test_stock_bits_at_the_benchmarks_shape(tmp_path_factory):
    """x is the stock convolution's, the whole group the stock chain's, the route's own comparison says verified, and a second
    call and a call on a side stream give the same bits."""
    out = _bench_process(str(tmp_path_factory.getbasetemp() / "conv1_miopen_db"))
    assert "bench shape ok" in out, out[-3000:]


def test_trainer_keeps_the_stock_trajectory(tmp_path_factory):
    """Three Trainer steps at the benchmark's image shape, where the route is verified and taken (the binding is called on every
    step), with the route on and off: equal losses and parameters."""
    out = _bench_process(str(tmp_path_factory.getbasetemp() / "conv1_miopen_db"))
    assert "bench trainer ok" in out, out[-3000:]


# ---- the route ----------------------------------------------------------------------------------------------------------------------
SMALL = (2, 6, 8)


def _small_image(seed=3):
    B, H, W = SMALL
    return _cl(torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed)).to(_dev()))


def test_routes_that_stay_stock(monkeypatch):
    """Nothing of these reaches the binding, not even to compare."""
    from vqa_amd import encoder
    from vqa_amd.modules import run_conv_bn_stack
    _default_env(monkeypatch)
    _forget(monkeypatch)
    raw_spy = _Spy(monkeypatch, "_conv1_raw")
    img = _small_image()

    def stays(seq, x=img):
        ref = copy.deepcopy(seq)
        got = run_conv_bn_stack(seq, x)
        assert raw_spy.take() == 0
        monkeypatch.setenv("VQA_ENCODER_REWRITE", "0")
        want = ref(x)
        monkeypatch.delenv("VQA_ENCODER_REWRITE")
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-5)               # (the bias fold moves roundings, as it always did)

    seq = _first_group(2)
    seq[0].weight.requires_grad_(True)
    stays(seq)                                                               # a trainable convolution
    seq = _first_group(2)
    seq[1].weight.requires_grad_(True)
    stays(seq)                                                               # a trainable BatchNorm
    seq = _first_group(2)
    seq[1].eval()
    stays(seq)                                                               # eval mode
    for conv in (torch.nn.Conv2d(3, 128, 3, padding=1), torch.nn.Conv2d(3, 64, 5, padding=2), torch.nn.Conv2d(3, 64, 3, stride=2, padding=1),
                 torch.nn.Conv2d(3, 64, 3, padding=1, padding_mode="reflect")):
        seq = _first_group(2)
        seq[0] = conv.to(_dev()).to(memory_format=torch.channels_last).requires_grad_(False)
        if conv.out_channels != 64:
            seq[1] = torch.nn.BatchNorm2d(conv.out_channels).to(_dev()).requires_grad_(False)
        stays(seq)
    seq = _first_group(2)                                                    # a misaligned parameter view
    flat = torch.zeros(2 * 64 + 1, device=_dev())
    flat[1:65], flat[65:129] = seq[1].running_mean, seq[1].running_var
    seq[1].running_mean, seq[1].running_var = flat[1:65], flat[65:129]
    assert seq[1].running_mean.data_ptr() % 16 == 4
    stays(seq)
    seq = _first_group(2)                                                    # NCHW weights
    seq[0].weight.data = seq[0].weight.data.contiguous()
    stays(seq)
    for name, value in (("VQA_ENCODER_EXACT_CONV1", "0"), ("VQA_ENCODER_EXACT_BN", "0"), ("VQA_ENCODER_REWRITE", "0"),
                        ("VQA_ENCODER_FUSED", "0")):
        monkeypatch.setenv(name, value)
        run_conv_bn_stack(_first_group(2), img)
        assert raw_spy.take() == 0, name
        monkeypatch.delenv(name)
    # a group that is not the first is never taken, whatever its convolution is
    head = torch.nn.Conv2d(64, 3, 3, padding=1).to(_dev()).to(memory_format=torch.channels_last).requires_grad_(False)
    run_conv_bn_stack(torch.nn.Sequential(head, *_first_group(4)), _cl(torch.randn(2, 64, 6, 8, device=_dev())))
    assert raw_spy.take() == 0
    assert all("conv1" not in v for v in encoder.exact_report().values())
    run_conv_bn_stack(_first_group(2), img)                                  # and the plain first group does reach it: it compares
    assert raw_spy.take() == 1 and "conv1" in encoder.exact_report()[(0, 2, 64, 6, 8, True)]


def test_a_mismatch_warns_once_and_stays_stock(monkeypatch):
    from vqa_amd import encoder
    from vqa_amd.modules import run_conv_bn_stack
    _default_env(monkeypatch)
    _forget(monkeypatch)
    raw_spy = _Spy(monkeypatch, "_conv1_raw")
    real = encoder._differs
    B, H, W = SMALL
    monkeypatch.setattr(encoder, "_differs", lambda a, b: real(a, b) | (a.numel() == B * 64 * H * W))     # "x differs"
    seq = _first_group(5)
    ref = copy.deepcopy(seq)
    img = _small_image(6)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(3):
            got = run_conv_bn_stack(seq, img)
            monkeypatch.setenv("VQA_ENCODER_EXACT_CONV1", "0")
            want = run_conv_bn_stack(ref, img)
            monkeypatch.delenv("VQA_ENCODER_EXACT_CONV1")
            assert torch.equal(got, want)
    mine = [w for w in caught if "first convolution" in str(w.message)]
    assert len(mine) == 1 and "B=2 H=6 W=8 pool=1" in str(mine[0].message) and "(x differs)" in str(mine[0].message)
    assert raw_spy.take() == 1                                               # the comparison, never again
    assert encoder.exact_report()[(0, B, 64, H, W, True)]["conv1"] == {"verified": False, "first_difference": "x"}
    for k, v in seq.state_dict().items():
        assert torch.equal(v, ref.state_dict()[k]), k


def test_the_first_call_inside_a_capture_does_not_verify(monkeypatch):
    from vqa_amd import encoder
    _default_env(monkeypatch)
    _forget(monkeypatch)
    raw_spy = _Spy(monkeypatch, "_conv1_raw")
    seq = _first_group(7, pool=False)
    ref = copy.deepcopy(seq)
    img = _small_image(8)
    assert encoder.conv1_modules_fusable(seq[0], seq[1], None, img)
    with torch.no_grad():
        want = F.relu(ref[1](F.conv2d(img, ref[0].weight, None, 1, 1)))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = encoder.conv1_bn_exact_or_stock(img, seq[0], seq[1], None)
    assert encoder.exact_report() == {} and raw_spy.take() == 0
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, want)
    encoder.conv1_bn_exact_or_stock(img, seq[0], seq[1], None)               # outside: compared and remembered
    assert raw_spy.take() == 1 and "conv1" in encoder.exact_report()[(0, SMALL[0], 64, SMALL[1], SMALL[2], False)]


if __name__ == "__main__" and sys.argv[1:] == ["--bench-shape"]:
    sys.path.insert(0, ROOT)
    _bench_shape_check()
    _bench_trainer_check()

"""The frozen encoder in eval mode on the one-launch HIP passes (include/coattn_ext.h v0.24.0: coattn_bn_eval_forward,
coattn_conv1_bn_eval_forward; vqa_amd/encoder.py bn_eval, conv1_bn_eval and their *_or_stock routes; --encoder_eval hip).  The
oracle is the stock chain on the same tensors on the same device (tests/_encoder_eval.py); every comparison is bit for bit."""
import copy
import functools
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                                           # (the child process of the benchmark's shape, below)
    sys.path.insert(0, ROOT)

from tests import _encoder_eval as E  # noqa: E402

pytestmark = pytest.mark.gpu

BENCH = (160, 224, 224)
MARKER, PAD = 12345.5, 4096
SWITCHES = ("VQA_ENCODER_FUSED", "VQA_ENCODER_EXACT_BN", "VQA_ENCODER_EXACT_CONV1", "VQA_ENCODER_REWRITE",
            "VQA_ENCODER_CONV1_RECOMPUTE")


def _arena(n):
    """A marker-filled buffer with n NaN words in the middle: y is carved out of it."""
    big = torch.full((PAD + n + PAD,), MARKER, device=E.dev())
    big[PAD:PAD + n] = float("nan")
    return big


def _check_arena(big, n, may_hold_nan, what):
    assert (big[:PAD] == MARKER).all() and (big[PAD + n:] == MARKER).all(), ("written outside y", what)
    if not may_hold_nan:
        assert not torch.isnan(big[PAD:PAD + n]).any(), ("a word of y was not written", what)


# ---- coattn_bn_eval_forward against the stock chain -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,eps", E.KINDS)
@pytest.mark.parametrize("C", E.CHANNELS)
def test_bn_eval_has_the_stock_chains_bits(C, kind, eps):
    seen_nan_window = False
    for n, shape in enumerate(E.SHAPES):
        x, bias, gamma, beta, rm, rv, eps = E.operands(C, shape, kind, 100 * C + n, eps)
        keep = [t.clone() for t in (x, bias, gamma, beta, rm, rv)]
        B, H, W = shape
        for pool in (False, True):
            for relu in (False, True):
                for b in (None, bias):
                    want = E.oracle(x, b, gamma, beta, rm, rv, eps, pool, relu)
                    ny = E.out_numel(B, C, H, W, pool)
                    big = _arena(ny)
                    E.bn_eval_into(big[PAD:], x, b, gamma, beta, rm, rv, eps, pool, relu)
                    got = E.as_nchw(big[PAD:PAD + ny], B, C, H, W, pool)
                    what = (C, kind, eps, shape, pool, relu, b is not None)
                    assert E.same(got, want), (what, int((torch.nan_to_num(got, nan=-1.) != torch.nan_to_num(want, nan=-1.)).sum()))
                    # the NaN-filled y: a NaN result may stand where the oracle has one, nowhere else (checked by `same`)
                    _check_arena(big, ny, True, what)
                    if kind == "NaN and inf" and pool and H * W > 4:
                        nan = torch.isnan(got)
                        seen_nan_window |= bool(nan.any() and not nan[1:].any() and int(nan.sum()) == 1)
        for t, k in zip((x, bias, gamma, beta, rm, rv), keep):
            assert E.same(t, k)                                      # every input is read only, the running statistics too
    if kind == "NaN and inf":
        assert seen_nan_window                                       # one sample's NaN: its own window of its own channel, no other


def test_what_the_variance_operands_are():
    """The "variances" kind holds what it says, for the eps it is run with: a zero, a negative and a huge variance, and sums with
    eps that are subnormal or cancel to zero."""
    tiny = float(torch.finfo(torch.float32).tiny)
    for eps, want_subnormal in ((E.EPS, False), (1e-40, True)):
        rv = E.operands(64, (1, 2, 2), "variances", 0, eps)[5]
        a = (rv + torch.tensor(eps, dtype=torch.float32, device=rv.device)).abs()
        assert (rv == 0).any() and (rv < 0).any() and (rv >= 1e30).any()
        assert bool(((a > 0) & (a < tiny)).any()) == want_subnormal
        if not want_subnormal:
            assert (a == 0).any()                                    # var = -eps: rsqrt(0) = inf


@pytest.mark.parametrize("pool", (False, True))
def test_the_second_trip_of_the_grid_stride_loop(pool):
    """The smallest shape (tests/_encoder_eval.second_trip_shape, from the launcher's grid cap) at which the capped grid goes round
    its loop a second time and ends in a partial tail."""
    C = 64
    shape = E.second_trip_shape(C, pool)
    B, H, W = shape
    x, bias, gamma, beta, rm, rv, eps = E.operands(C, shape, "normal", 7)
    want = E.oracle(x, bias, gamma, beta, rm, rv, eps, pool, True)
    ny = E.out_numel(B, C, H, W, pool)
    big = _arena(ny)
    E.bn_eval_into(big[PAD:], x, bias, gamma, beta, rm, rv, eps, pool, True)
    assert E.same(E.as_nchw(big[PAD:PAD + ny], B, C, H, W, pool), want), shape
    _check_arena(big, ny, False, shape)


def test_a_second_call_and_a_side_stream_give_the_same_bits():
    for C, shape in ((64, (2, 5, 7)), (512, (3, 8, 6))):
        x, bias, gamma, beta, rm, rv, eps = E.operands(C, shape, "mixed magnitude", 3)
        B, H, W = shape
        for pool in (False, True):
            ny = E.out_numel(B, C, H, W, pool)
            ys = [torch.empty(ny, device=E.dev()) for _ in range(3)]
            E.bn_eval_into(ys[0], x, bias, gamma, beta, rm, rv, eps, pool, True)
            E.bn_eval_into(ys[1], x, bias, gamma, beta, rm, rv, eps, pool, True)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                E.bn_eval_into(ys[2], x, bias, gamma, beta, rm, rv, eps, pool, True)
            side.synchronize()
            torch.cuda.current_stream().wait_stream(side)
            assert E.same(ys[0], ys[1]) and E.same(ys[0], ys[2]), (C, shape, pool)


def test_the_module_form_moves_no_buffer():
    from vqa_amd import encoder
    C, shape = 128, (2, 5, 7)
    x, bias, gamma, beta, rm, rv, eps = E.operands(C, shape, "normal", 11)
    bn = torch.nn.BatchNorm2d(C, eps=eps).to(E.dev()).eval().requires_grad_(False)
    bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    bn.num_batches_tracked.fill_(5)
    before = copy.deepcopy(bn.state_dict())
    for pool in (False, True):
        for b in (None, bias):
            got = encoder.bn_eval(x, bn, conv_bias=b, pool=pool)
            assert got.is_contiguous(memory_format=torch.channels_last)
            assert E.same(got, E.oracle(x, b, gamma, beta, rm, rv, eps, pool, True))
    for k, v in bn.state_dict().items():
        assert torch.equal(v, before[k]), k
    with pytest.raises(ValueError, match="eval mode"):
        encoder.bn_eval(x, copy.deepcopy(bn).train())
    with pytest.raises(ValueError, match="channels_last"):
        encoder.bn_eval(x.contiguous(), bn)


# ---- coattn_conv1_bn_eval_forward against the project's own verified pieces -----------------------------------------------------------
def test_the_conv1_shape_list_has_every_property():
    from vqa_amd import _lib
    shapes = E.conv1_shapes()
    print("conv1 eval shapes:", shapes)
    for name, has in E.CONV1_PROPERTIES.items():
        assert any(has(B, H, W) for B, H, W in shapes), name
    lib = _lib.load()
    for pool in (0, 1):
        assert all(lib.coattn_conv1_bn_exact_supported(B, H, W, 3, 64, pool, _lib.F32) == 1 and
                   lib.coattn_conv1_bn_eval_supported(B, H, W, 3, 64, pool, _lib.F32) == 1 for B, H, W in shapes)
    assert {B for B, _, _ in shapes} >= {1, E.chunk(), E.chunk() + 1}
    assert all(B * H * W * 64 * 4 <= 2 ** 22 for B, H, W in shapes)


@functools.lru_cache(maxsize=None)
def _conv1_x(shape, kind, seed):
    """(image, weight, x): x the convolution output coattn_conv1_bn_exact_forward stores, which tests/test_gpu_encoder_conv1.py pins
    to the stock convolution's bits.  Computed once per case and left unchanged."""
    from vqa_amd import encoder
    img, w = E.conv1_operands(shape, kind, seed)
    ones, zeros = torch.ones(64, device=E.dev()), torch.zeros(64, device=E.dev())
    x, _, _, _ = encoder._conv1_raw(img, w, ones, zeros, zeros.clone(), ones.clone(), 0.1, E.EPS, False, True)
    return img, w, x


@pytest.mark.parametrize("kind", ("normal", "mixed magnitude", "NaN and inf"))
def test_conv1_eval_is_bn_eval_of_the_stored_convolution(kind):
    seen_mix = False
    for n, shape in enumerate(E.conv1_shapes()):
        img, w, x = _conv1_x(shape, kind, 40 + n)
        B, H, W = shape
        # the per-channel operands alternate between the shapes: mixed magnitudes, the variance cases, and those with a tiny eps
        _, bias, gamma, beta, rm, rv, eps = E.operands(64, (1, 2, 2), "variances" if n % 2 else "mixed magnitude", 60 + n,
                                                       1e-40 if n % 4 == 3 else E.EPS)
        for pool in (True, False):
            for b in (None, bias):
                ny = E.out_numel(B, 64, H, W, pool)
                want = torch.empty(ny, device=E.dev())
                E.bn_eval_into(want, x, b, gamma, beta, rm, rv, eps, pool, True)
                big = _arena(ny)
                E.conv1_eval_into(big[PAD:], img, w, b, gamma, beta, rm, rv, eps, pool)
                what = (kind, shape, pool, b is not None)
                assert E.same(big[PAD:PAD + ny], want), what
                _check_arena(big, ny, True, what)
                if kind == "NaN and inf":
                    assert torch.isnan(want).any()
                    seen_mix |= not bool(torch.isnan(want).all())    # (a 2 x 2 image is all NaN: every window sees the NaN pixel)
    assert seen_mix or kind != "NaN and inf"


def test_conv1_eval_second_call_side_stream_and_module_form():
    from vqa_amd import encoder
    shape = E.conv1_shapes()[-1]
    img, w = E.conv1_operands(shape, "mixed magnitude", 5)
    B, H, W = shape
    _, bias, gamma, beta, rm, rv, eps = E.operands(64, (1, 2, 2), "normal", 9)
    conv = torch.nn.Conv2d(3, 64, 3, padding=1).to(E.dev()).to(memory_format=torch.channels_last).requires_grad_(False)
    conv.weight.copy_(w), conv.bias.copy_(bias)
    bn = torch.nn.BatchNorm2d(64, eps=eps).to(E.dev()).eval().requires_grad_(False)
    bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    before = copy.deepcopy(bn.state_dict())
    for pool in (True, False):
        ny = E.out_numel(B, 64, H, W, pool)
        ys = [torch.empty(ny, device=E.dev()) for _ in range(3)]
        E.conv1_eval_into(ys[0], img, w, bias, gamma, beta, rm, rv, eps, pool)
        E.conv1_eval_into(ys[1], img, w, bias, gamma, beta, rm, rv, eps, pool)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            E.conv1_eval_into(ys[2], img, w, bias, gamma, beta, rm, rv, eps, pool)
        side.synchronize()
        torch.cuda.current_stream().wait_stream(side)
        assert E.same(ys[0], ys[1]) and E.same(ys[0], ys[2]), pool
        got = encoder.conv1_bn_eval(img, conv, bn, pool)
        assert got.is_contiguous(memory_format=torch.channels_last) and E.same(got, E.as_nchw(ys[0], B, 64, H, W, pool))
    for k, v in bn.state_dict().items():
        assert torch.equal(v, before[k]), k


# ---- the route ----------------------------------------------------------------------------------------------------------------------------
def _default_env(monkeypatch):
    from vqa_amd import encoder
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(encoder, "_eval", {})


def _features(seed=0):
    """A VGG11-bn `features` stack with running statistics that are not the initial ones, frozen, channels_last, in eval mode."""
    from vqa_amd.modules import vgg11_bn_features
    torch.manual_seed(seed)
    seq = vgg11_bn_features()
    for m in seq:
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.3), m.running_var.uniform_(0.5, 1.5), m.weight.data.uniform_(0.5, 1.5), m.bias.data.normal_(0, 0.2)
    return seq.to(E.dev()).to(memory_format=torch.channels_last).requires_grad_(False).eval()


def _image(B=3, S=64, seed=1):
    return E.cl(torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(seed)).to(E.dev()))


class _Count:
    """Counts the calls of owner.name for the life of the monkeypatch."""

    def __init__(self, monkeypatch, owner, name):
        self.calls, real = 0, getattr(owner, name)

        def counted(*a, **k):
            self.calls += 1
            return real(*a, **k)
        monkeypatch.setattr(owner, name, counted)

    def take(self):
        n, self.calls = self.calls, 0
        return n


def test_the_vgg_stack_under_hip_is_the_stock_stack(monkeypatch):
    from vqa_amd import encoder
    from vqa_amd.modules import run_conv_bn_stack
    _default_env(monkeypatch)
    seq = _features()
    before = copy.deepcopy(seq.state_dict())
    img = _image()
    bn_calls = _Count(monkeypatch, torch.nn.BatchNorm2d, "forward")
    pool_calls = _Count(monkeypatch, encoder, "relu_pool")
    one = _Count(monkeypatch, encoder, "_conv1_eval_raw")
    with torch.no_grad(), warnings.catch_warnings():
        # no BatchNorm shape may differ: the map is elementwise.  The first group's one-launch form may: away from the benchmark's
        # shape MIOpen may run the first convolution on a solver of another summation order (tests/test_gpu_encoder_conv1.py)
        warnings.filterwarnings("error", message="encoder: bn_eval")
        warnings.filterwarnings("ignore", message="encoder: the one-launch")
        want = seq(img)
        assert bn_calls.take() == 8
        stock = run_conv_bn_stack(seq, img)                          # the default: today's route, five relu_pool calls
        assert E.same(stock, want) and bn_calls.take() == 8 and pool_calls.take() == 5 and encoder.eval_report() == {}
        first = run_conv_bn_stack(seq, img, "hip")                   # every group compared
        assert bn_calls.take() == 8 and one.take() == 1
        report = encoder.eval_report()
        print("eval report:", json.dumps({str(k): v for k, v in report.items()}))
        assert len(report) == 8
        for key, entry in report.items():
            assert entry["verified"] and entry["first_difference"] is None and entry["bias"] in ("kernel", "convolution"), (key, entry)
        conv1 = report[(0, 3, 64, 64, 64, True, 3)]["conv1"]         # the first group's verdict is recorded either way
        assert conv1 in ({"verified": True, "first_difference": None}, {"verified": False, "first_difference": "y"})
        assert sum("conv1" in e for e in report.values()) == 1
        pool_calls.take()
        second = run_conv_bn_stack(seq, img, "hip")                  # the route: no stock BatchNorm, no separate pool pass
        assert bn_calls.take() == 0 and pool_calls.take() == 0 and one.take() == (1 if conv1["verified"] else 0)
        third = run_conv_bn_stack(seq, img, "hip")
    for got in (first, second, third):
        assert E.same(got, want)
    assert float(want.abs().max()) > 0 and want.shape == (3, 512, 2, 2)
    for k, v in seq.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_the_bias_goes_into_the_kernel_only_where_the_convolutions_agree(monkeypatch):
    """Groups 2 - 8: under deterministic solvers the verdict of conv2d(x, w, None) + b == conv2d(x, w, b) is recorded and the route
    issues the convolution accordingly; without them the convolution keeps its bias."""
    from vqa_amd import encoder
    _default_env(monkeypatch)
    seq = _features(2)
    conv, bn, pool = seq[4], seq[5], seq[7]
    x = E.cl(torch.randn(3, 64, 16, 16, generator=torch.Generator().manual_seed(4)).to(E.dev()))
    key = (0, 3, 128, 16, 16, True, 64)
    with torch.no_grad():
        want = F.relu(pool(bn(conv(x))))
        equal = E.same(F.conv2d(x, conv.weight, None, 1, 1) + conv.bias.view(1, -1, 1, 1), conv(x))
        convs = _Count(monkeypatch, F, "conv2d")
        first = encoder.bn_eval_or_stock(x, conv, bn, pool)
        entry = encoder.eval_report()[key]
        assert entry["verified"] and entry["bias"] == ("kernel" if equal else "convolution"), (entry, equal)
        convs.take()
        seen = []
        real = encoder.bn_eval
        monkeypatch.setattr(encoder, "bn_eval", lambda z, b, conv_bias=None, pool=False: seen.append(conv_bias) or real(z, b, conv_bias, pool))
        second = encoder.bn_eval_or_stock(x, conv, bn, pool)
        assert len(seen) == 1 and (seen[0] is conv.bias) == equal
        assert E.same(first, want) and E.same(second, want)
        # without deterministic solvers nothing is known about the next call's solver: the convolution keeps its bias
        monkeypatch.setattr(encoder, "_eval", {})
        monkeypatch.setattr(torch.backends.cudnn, "deterministic", False)
        encoder.bn_eval_or_stock(x, conv, bn, pool)
        assert encoder.eval_report()[key]["bias"] == "convolution"
        encoder.bn_eval_or_stock(x, conv, bn, pool)
        assert seen[-1] is None
    print("bias in the kernel:", equal)


def test_a_shape_made_to_differ_stays_stock_and_warns_once(monkeypatch):
    from vqa_amd import encoder
    from vqa_amd.modules import run_conv_bn_stack
    _default_env(monkeypatch)
    seq = torch.nn.Sequential(*list(_features(3))[:8])
    img = _image(2, 16, 5)
    B, H, W = 2, 16, 16
    real = encoder._differs
    # "y differs" for the first group's pooled output, whoever computed it
    monkeypatch.setattr(encoder, "_differs", lambda a, b: real(a, b) | (a.numel() == B * 64 * (H // 2) * (W // 2)))
    raw, one = _Count(monkeypatch, encoder, "_bn_eval_raw"), _Count(monkeypatch, encoder, "_conv1_eval_raw")
    with torch.no_grad():
        want = seq(img)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            outs = [run_conv_bn_stack(seq, img, "hip") for _ in range(3)]
    texts = [str(w.message) for w in caught]
    assert sum("bn_eval does not reproduce" in t for t in texts) == 1 and sum("one-launch eval-mode first group" in t for t in texts) == 1
    assert len(texts) == 2, texts
    report = encoder.eval_report()
    first = report[(0, B, 64, H, W, True, 3)]
    assert not first["verified"] and first["first_difference"] == "y" and first["conv1"] == {"verified": False, "first_difference": "y"}
    assert report[(0, B, 128, H // 2, W // 2, True, 64)]["verified"]
    for got in outs:
        assert E.same(got, want)
    # the first pass compared (both forms of group 1, one or two of group 2); afterwards group 1 is stock, group 2 on its route
    # (both groups compared with the bias outside and inside the kernel: the solvers are deterministic)
    assert one.take() == 1 and raw.take() == 2 + 2 + 2


def test_a_capturing_stream_runs_stock_and_remembers_nothing(monkeypatch):
    from vqa_amd import encoder
    _default_env(monkeypatch)
    seq = _features(4)
    conv, bn, relu, pool = seq[0], seq[1], seq[2], seq[3]
    img = _image(2, 16, 6)
    raw, one = _Count(monkeypatch, encoder, "_bn_eval_raw"), _Count(monkeypatch, encoder, "_conv1_eval_raw")
    with torch.no_grad():
        want = F.relu(pool(bn(conv(img))))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = encoder.conv1_bn_eval_or_stock(img, conv, bn, pool)
        assert encoder.eval_report() == {} and raw.take() == 0 and one.take() == 0
        graph.replay()
        torch.cuda.synchronize()
        assert E.same(y, want)
        encoder.conv1_bn_eval_or_stock(img, conv, bn, pool)          # outside: compared and remembered
    assert one.take() == 1 and "conv1" in encoder.eval_report()[(0, 2, 64, 16, 16, True, 3)]


def test_train_mode_under_hip_takes_todays_routes(monkeypatch):
    from vqa_amd import encoder
    from vqa_amd.modules import run_conv_bn_stack
    _default_env(monkeypatch)
    monkeypatch.setattr(encoder, "_exact", {})
    a, b = _features(5).train(), _features(5).train()
    img = _image(2, 32, 7)
    asked, real = [], encoder._lib.bind
    monkeypatch.setattr(encoder._lib, "bind", lambda name, **kw: asked.append(name) or real(name, **kw))
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(2):
            monkeypatch.setattr(encoder, "_exact", {})               # (both runs compare their shapes: the same calls)
            got = run_conv_bn_stack(a, img, "hip")
            n_hip, asked[:] = list(asked), []
            monkeypatch.setattr(encoder, "_exact", {})
            want = run_conv_bn_stack(b, img)
            n_stock, asked[:] = list(asked), []
            assert E.same(got, want) and n_hip == n_stock and not any("eval" in n for n in n_hip)
    assert encoder.eval_report() == {}
    for (k, v), w in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(v, w), k
    # NCHW, autocast and a trainable encoder stay on the stock lines in eval mode too
    with torch.no_grad():
        x = _image(2, 32, 8).contiguous()
        nchw = _features(6).to(memory_format=torch.contiguous_format)
        assert E.same(run_conv_bn_stack(nchw, x, "hip"), nchw(x))
        assert encoder.eval_report() == {} and not any("eval" in n for n in asked)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            run_conv_bn_stack(_features(6), _image(2, 32, 8), "hip")
    assert encoder.eval_report() == {} and not any("eval" in n for n in asked)
    run_conv_bn_stack(_features(6).requires_grad_(True), _image(2, 32, 8), "hip")
    assert encoder.eval_report() == {} and not any("eval" in n for n in asked)


# ---- the benchmark's shape, in a process of its own --------------------------------------------------------------------------------------
def _bench_shape_check():
    """160 x 3 x 224 x 224 under the benchmark's own MIOpen find records.  On the default solvers, which are the benchmark's, the
    one-launch first group verifies against the stock convolution and chain and its route gives their bits.  On the deterministic
    solvers (extract.py's) PyTorch runs the first convolution on another algorithm, of another summation order: there every
    BatchNorm group verifies with the bias inside the kernel, the first group's verdict is recorded either way, and the whole
    stack gives the stock stack's bits."""
    import bench
    bench.seed_miopen_db()
    from vqa_amd import encoder
    from vqa_amd.modules import run_conv_bn_stack
    for name in SWITCHES:
        os.environ.pop(name, None)
    B, H, W = BENCH
    seq = _features(1)
    g = torch.Generator(device=E.dev()).manual_seed(7)
    img = E.cl(torch.randn(B, 3, H, W, device=E.dev(), generator=g))
    calls, real = [0], encoder._conv1_eval_raw

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    encoder._conv1_eval_raw = counted
    key = (0, B, 64, H, W, True, 3)
    with torch.no_grad():
        torch.backends.cudnn.deterministic = False
        group = torch.nn.Sequential(*list(seq)[:4])
        want = run_conv_bn_stack(group, img)
        first = run_conv_bn_stack(group, img, "hip")
        entry = encoder.eval_report()[key]
        assert entry["verified"] and entry["bias"] == "convolution", entry
        assert entry["conv1"] == {"verified": True, "first_difference": None}, entry
        second = run_conv_bn_stack(group, img, "hip")
        assert calls[0] == 2 and E.same(first, want) and E.same(second, want)
        del first, second, want
        torch.backends.cudnn.deterministic = True
        encoder._eval.clear()
        want = run_conv_bn_stack(seq, img)
        first = run_conv_bn_stack(seq, img, "hip")
        report = encoder.eval_report()
        assert len(report) == 8 and all(e["verified"] for e in report.values()), report
        assert "conv1" in report[key], report
        second = run_conv_bn_stack(seq, img, "hip")
    assert E.same(first, want) and E.same(second, want)
    print("bias:", {str(k): v["bias"] for k, v in report.items()}, "conv1 on the deterministic solvers:", report[key]["conv1"])
    print("bench shape ok")


@functools.lru_cache(maxsize=None)
def _bench_process(db_dir):
    env = dict(os.environ, MIOPEN_USER_DB_PATH=db_dir)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--bench-shape"], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    return r.stdout


def test_every_group_verifies_at_the_benchmarks_shape(tmp_path_factory):
    out = _bench_process(str(tmp_path_factory.getbasetemp() / "encoder_eval_miopen_db"))
    assert "bench shape ok" in out, out[-3000:]


# ---- end to end: --encoder_eval hip against stock, deterministic solvers ------------------------------------------------------------------
SMALL = ["--num_cls", "10", "--image_size", "64", "--vocab_size", "50"]


@pytest.fixture
def deterministic(monkeypatch):
    _default_env(monkeypatch)


def _checkpoint(tmp_path):
    from vqa_amd import train as T
    torch.manual_seed(5)
    net = T.build_model("attention", 50, 10)
    for m in net.image_encoder.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.3), m.running_var.uniform_(0.5, 1.5)
    ckpt = str(tmp_path / "net.pth")
    torch.save(net.state_dict(), ckpt)
    return ckpt


def test_validate_returns_equal_dicts(tmp_path, deterministic):
    from vqa_amd import encoder, train as T
    ckpt = _checkpoint(tmp_path)
    batches = []
    ds = T.SyntheticVQADataset(16, (64, 64), 26, 50, 11, 987654)
    for b in torch.utils.data.DataLoader(ds, 8, shuffle=False):
        im, qu, la, ln = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
        batches.append((E.cl(im.to(E.dev())), qu.to(E.dev()), ln, la.to(E.dev())))
    got = {}
    for impl in ("stock", "hip"):
        torch.manual_seed(0)
        net = T.build_model("attention", 50, 10)
        net.load_state_dict(torch.load(ckpt, map_location="cpu"))
        net.to(E.dev())
        net.image_encoder.to(memory_format=torch.channels_last)
        tr = T.Trainer(net, 1e-4, E.dev(), encoder_eval=impl)
        assert net.image_encoder.eval_impl == impl
        got[impl] = [tr.validate(batches) for _ in range(2)]
    assert len(encoder.eval_report()) == 8 and all(e["verified"] for e in encoder.eval_report().values())
    print("validate:", got)
    assert got["hip"][0] == got["hip"][1] == got["stock"][0] == got["stock"][1]


def test_predict_and_extract_write_the_same_files(tmp_path, capsys, deterministic):
    from vqa_amd import encoder, extract as X, predict as P
    ckpt = _checkpoint(tmp_path)
    argv = ["--model", "attention", "--batch_size", "8", "--model_ckpt", ckpt] + SMALL
    got = {}
    for impl in ("stock", "hip"):
        preds, maps, table = (str(tmp_path / (impl + ext)) for ext in (".jsonl", ".npz", ".npy"))
        P.main(argv + ["--test_size", "16", "--predictions", preds, "--attention_maps", maps, "--encoder_eval", impl])
        X.main(argv + ["--split", "val", "--samples", "16", "--out", table, "--encoder_eval", impl])
        z = np.load(maps)
        side = [f for f in sorted(os.listdir(tmp_path)) if f.startswith(impl + ".") and f not in (impl + ".jsonl", impl + ".npz", impl + ".npy")]
        got[impl] = (open(preds).read(), {k: z[k] for k in z.files}, open(table, "rb").read(),
                     [open(str(tmp_path / f), "rb").read() for f in side])
    capsys.readouterr()
    assert len(encoder.eval_report()) == 8 and all(e["verified"] for e in encoder.eval_report().values())
    assert got["hip"][0] == got["stock"][0] and len(got["hip"][0]) > 0
    for k, v in got["stock"][1].items():
        assert np.array_equal(got["hip"][1][k], v), k
    assert got["hip"][2] == got["stock"][2]                          # the feature table, byte for byte
    assert got["hip"][3] == got["stock"][3] and len(got["stock"][3]) >= 1      # and its sidecar: no field says which route wrote it


if __name__ == "__main__" and sys.argv[1:] == ["--bench-shape"]:
    _bench_shape_check()

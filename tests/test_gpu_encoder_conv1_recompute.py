"""The frozen encoder's first group with its convolution computed twice and never stored (include/coattn.h v0.22.0,
coattn_conv1_bn_recompute_forward; csrc/encoder.hip conv1_stats_miopen_kernel<D, false> and conv1_norm_pool_kernel;
vqa_amd/encoder.py _conv1_recompute_raw).  The yardstick is the entry that stores the convolution output,
coattn_conv1_bn_exact_forward, which tests/test_gpu_encoder_conv1.py pins to the stock kernels' bits: every result of the new
entry is compared with it bit for bit."""
import copy
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
SWITCHES = ("VQA_ENCODER_FUSED", "VQA_ENCODER_EXACT_BN", "VQA_ENCODER_EXACT_CONV1", "VQA_ENCODER_REWRITE",
            "VQA_ENCODER_CONV1_RECOMPUTE")


def _dev():
    return torch.device("cuda:0")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _same(a, b):
    """Equal bits up to a NaN's payload: NaNs in the same places, and -0 is not +0."""
    if not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    a, b = torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0)
    return torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))


def _chunk():
    from vqa_amd import _lib
    return _lib.CONV1_RECOMPUTE_CHUNK


# ---- the shape list, by rule ------------------------------------------------------------------------------------------------------
# g: the BatchNorm geometry of the convolution's output (pass A owns 32 consecutive pixels per wave whatever g1 is); pass B's
# pooled tile is 2 image rows x 16 columns = 8 pooled columns, its workgroup takes _chunk() samples
PROPERTIES = {
    "Wo is not a multiple of 8 (a masked window)": lambda g, B, H, W: (W // 2) % 8 != 0 and W // 2 > 8,
    "Wo < 8": lambda g, B, H, W: W // 2 < 8,
    "odd W (the last column is never read for a pooled output)": lambda g, B, H, W: W % 2 == 1 and W >= 3,
    "odd H (the last row is never read for a pooled output)": lambda g, B, H, W: H % 2 == 1 and H >= 3,
    "H = W = 2": lambda g, B, H, W: H == 2 and W == 2,
    "more than one tile row and more than one column block": lambda g, B, H, W: H // 2 >= 2 and W // 2 > 8,
    "a pixel group wraps an image row (pass A)": lambda g, B, H, W: W % g["g1"] != 0 and H >= 2 and H * W > g["g1"],
    "a masked tail of pixels (pass A)": lambda g, B, H, W: (H * W) % g["g1"] != 0 and (H * W) % 32 != 0,
    "g1 = 8": lambda g, B, H, W: g["g1"] == 8,
    "g1 = 16": lambda g, B, H, W: g["g1"] == 16,
    "B = 1": lambda g, B, H, W: B == 1,
    "B = 2": lambda g, B, H, W: B == 2,
    "B = 3": lambda g, B, H, W: B == 3,
    "B crosses pass B's sample chunk by one": lambda g, B, H, W: B == _chunk() + 1,
}


@functools.lru_cache(maxsize=None)
def shape_list():
    """For each property the covered (B, H, W) of smallest B H W that has it, B in {1, 2, 3}, H <= W <= 48, candidates in order of
    B H W, then B, then H -- the rule of tests/test_gpu_encoder_conv1.py, with its one exception (g1 = 16 begins at H W = 2560:
    that property looks up to 64) and one more: the B that crosses the sample chunk is the chunk + 1, above 3."""
    from vqa_amd import encoder
    shapes = []
    for name, has in PROPERTIES.items():
        top = 65 if name == "g1 = 16" else 49
        batches = (_chunk() + 1,) if "chunk" in name else (1, 2, 3)
        cands = sorted((B * H * W, B, H, W) for B in batches for H in range(2, top) for W in range(H, top))
        for _, B, H, W in cands:
            g = encoder.exact_geometry(B, H, W, 64)
            if g is not None and has(g, B, H, W):
                if (B, H, W) not in shapes:
                    shapes.append((B, H, W))
                break
        else:
            raise AssertionError(name)
    return tuple(shapes)


def test_the_shape_list_has_every_property():
    from vqa_amd import _lib, encoder
    shapes = shape_list()
    print("shapes:", shapes)
    for name, has in PROPERTIES.items():
        assert any(has(encoder.exact_geometry(B, H, W, 64), B, H, W) for B, H, W in shapes), name
    lib = _lib.load()
    for pool in (0, 1):
        assert all(lib.coattn_conv1_bn_exact_supported(B, H, W, 3, 64, pool, _lib.F32) == 1 for B, H, W in shapes)
    assert all(B * H * W * 64 * 4 <= 2 ** 21 for B, H, W in shapes)


# ---- inputs and the two raw calls ---------------------------------------------------------------------------------------------------
KINDS = ("normal", "mixed magnitude", "subnormal", "near 1e19", "NaN and inf", "negative zero", "zeros of both signs and NaN in a window")


def _inputs(shape, kind, seed):
    """The input kinds of tests/test_gpu_encoder_conv1.py; the last one is made by _params."""
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


def _params(seed, kind="normal"):
    g = torch.Generator().manual_seed(seed)
    gamma, beta = 0.5 + torch.rand(64, generator=g), 0.5 * torch.randn(64, generator=g)
    if kind == "negative zero":
        gamma[1::4] = -gamma[1::4]                                             # (a negative gamma: the map goes before the maximum)
    if kind == "zeros of both signs and NaN in a window":
        # gamma * z underflows to a zero with z's sign, so a window's members are +0 and -0 (beta = +0: +0 + -0 = +0; beta = -0 keeps
        # the product's sign) and the maximum's answer depends on the order its members enter; gamma = inf, beta = -inf gives
        # NaN where z > 0 and -inf where z < 0: NaNs and numbers in one window without a NaN in the statistics
        gamma[0:8:2], gamma[1:8:2], beta[0:4], beta[4:8] = 1e-45, -1e-45, 0.0, -0.0
        gamma[8:12], beta[8:12] = float("inf"), float("-inf")
        gamma[12:16], beta[12:16] = float("-inf"), float("inf")
    return [t.to(_dev()) for t in (gamma, beta, torch.randn(64, generator=g), 0.5 + torch.rand(64, generator=g))]


def _stored(img, w, params, pool):
    """(y, running_mean, running_var, save_mean, save_invstd, x) of coattn_conv1_bn_exact_forward on clones of the statistics."""
    from vqa_amd import encoder
    gamma, beta, rm, rv = params
    rm, rv = rm.clone(), rv.clone()
    x, y, mean, invstd = encoder._conv1_raw(img, w, gamma, beta, rm, rv, MOMENTUM, EPS, pool, True)
    return y, rm, rv, mean, invstd, x


def _recompute(img, w, params, pool):
    """(y, running_mean, running_var, save_mean, save_invstd) of coattn_conv1_bn_recompute_forward on clones of the statistics."""
    from vqa_amd import encoder
    gamma, beta, rm, rv = params
    rm, rv = rm.clone(), rv.clone()
    y, mean, invstd = encoder._conv1_recompute_raw(img, w, gamma, beta, rm, rv, MOMENTUM, EPS, pool)
    return y, rm, rv, mean, invstd


NAMES = ("y", "running_mean", "running_var", "save_mean", "save_invstd")


# ---- bit equality with the stored form, on every shape ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_bits_are_the_stored_forms(kind):
    seen_zero_pair = seen_nan_mix = False
    for n, shape in enumerate(shape_list()):
        img, w = _inputs(shape, kind, 30 + n)
        for pool in (True, False):
            params = _params(50 + n, kind)
            want = _stored(img, w, params, pool)
            got = _recompute(img, w, params, pool)
            for name, a, b in zip(NAMES, got, want):
                assert _same(a, b), (kind, shape, pool, name, int((torch.nan_to_num(a, nan=-1.0) != torch.nan_to_num(b, nan=-1.0)).sum()))
            assert got[0].shape == want[0].shape and got[0].is_contiguous(memory_format=torch.channels_last)
            if kind == "NaN and inf":
                assert torch.isnan(got[3]).any()
            if kind.startswith("zeros of both signs") and pool:
                # what the windows hold, from the stored form's x: members of both zero signs, and NaN beside a number
                x, (gamma, beta) = want[5], params[:2]
                t = gamma.view(1, -1, 1, 1) * ((x - want[3].view(1, -1, 1, 1)) * want[4].view(1, -1, 1, 1)) + beta.view(1, -1, 1, 1)
                H2, W2 = shape[1] // 2 * 2, shape[2] // 2 * 2
                win = F.unfold(t[:, :, :H2, :W2].reshape(-1, 1, H2, W2), 2, stride=2)               # [B C, 4, windows]
                zero, neg = win == 0, torch.signbit(win)
                seen_zero_pair |= bool(((zero & neg).any(1) & (zero & ~neg).any(1)).any())
                seen_nan_mix |= bool((torch.isnan(win).any(1) & (~torch.isnan(win)).any(1)).any())
    if kind.startswith("zeros of both signs"):
        assert seen_zero_pair and seen_nan_mix, (seen_zero_pair, seen_nan_mix)


def test_guard_bands():
    """y and the workspace carved out of larger buffers filled with a marker: not a word outside them changes, every word of y is
    written, and the workspace is the partials alone."""
    from vqa_amd import _lib
    lib = _lib.load()
    for shape in shape_list():
        B, H, W = shape
        img, w = _inputs(shape, "normal", 5)
        assert lib.coattn_conv1_bn_recompute_workspace_bytes(B, H, W) == lib.coattn_conv1_bn_exact_workspace_bytes(B, H, W, 0)
        for pool in (1, 0):
            gamma, beta, rm, rv = _params(6)
            ny = B * 64 * (H // 2) * (W // 2) if pool else B * 64 * H * W
            nws, pad, marker = lib.coattn_conv1_bn_recompute_workspace_bytes(B, H, W) // 4, 4096, 12345.5
            big = [torch.full((pad + n + pad,), marker, device=_dev()) for n in (ny, nws)]
            save = torch.full((2, 64), marker, device=_dev())
            big[0][pad:pad + ny] = float("nan")
            _lib.bind("coattn_conv1_bn_recompute_forward", image=img, weight=w, gamma=gamma, beta=beta, running_mean=rm,
                      running_var=rv, momentum=MOMENTUM, eps=EPS, y=big[0][pad:], save_mean=save[0], save_invstd=save[1],
                      ws=big[1][pad:], B=B, H=H, W=W, Cin=3, Cout=64, pool=pool, dtype=_lib.F32,
                      stream=_lib.stream_ptr(img.device))()
            torch.cuda.synchronize()
            for b, n in zip(big, (ny, nws)):
                assert (b[:pad] == marker).all() and (b[pad + n:] == marker).all(), (shape, pool)
            assert not torch.isnan(big[0]).any() and not (save == marker).any(), (shape, pool)
            want = _stored(img, w, _params(6), bool(pool))[0]
            assert torch.equal(big[0][pad:pad + ny], want.permute(0, 2, 3, 1).reshape(-1)), (shape, pool)


def test_a_second_call_and_a_side_stream_give_the_same_bits():
    for n, shape in enumerate(shape_list()[:4] + shape_list()[-1:]):
        img, w = _inputs(shape, "mixed magnitude", 70 + n)
        for pool in (True, False):
            params = _params(80 + n)
            first = _recompute(img, w, params, pool)
            second = _recompute(img, w, params, pool)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                third = _recompute(img, w, params, pool)
            side.synchronize()
            torch.cuda.current_stream().wait_stream(side)
            for name, a, b, c in zip(NAMES, first, second, third):
                assert _same(a, b) and _same(a, c), (shape, pool, name)


# ---- the route ----------------------------------------------------------------------------------------------------------------------
SMALL = (2, 6, 8)


def _first_group(seed=0, pool=True):
    torch.manual_seed(seed)
    mods = [torch.nn.Conv2d(3, 64, 3, padding=1), torch.nn.BatchNorm2d(64, eps=EPS, momentum=MOMENTUM), torch.nn.ReLU(inplace=True)]
    if pool:
        mods.append(torch.nn.MaxPool2d(2, 2))
    return torch.nn.Sequential(*mods).to(_dev()).to(memory_format=torch.channels_last).requires_grad_(False)


def _default_env(monkeypatch):
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


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


def _small_image(seed=3):
    B, H, W = SMALL
    return _cl(torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed)).to(_dev()))


def test_a_shape_that_does_not_verify_never_reaches_the_new_binding(monkeypatch):
    """The stored form is compared first; where it differs from the stock kernels (here: made to, as
    tests/test_gpu_encoder_conv1.py makes it) the recompute form is not even run, and the shape stays stock."""
    from vqa_amd import encoder
    from vqa_amd.modules import run_conv_bn_stack
    _default_env(monkeypatch)
    monkeypatch.setattr(encoder, "_exact", {})
    new_spy, raw_spy = _Spy(monkeypatch, "_conv1_recompute_raw"), _Spy(monkeypatch, "_conv1_raw")
    real = encoder._differs
    B, H, W = SMALL
    monkeypatch.setattr(encoder, "_differs", lambda a, b: real(a, b) | (a.numel() == B * 64 * H * W))     # "x differs"
    seq = _first_group(5)
    ref = copy.deepcopy(seq)
    img = _small_image(6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(3):
            got = run_conv_bn_stack(seq, img)
            monkeypatch.setenv("VQA_ENCODER_EXACT_CONV1", "0")
            want = run_conv_bn_stack(ref, img)
            monkeypatch.delenv("VQA_ENCODER_EXACT_CONV1")
            assert torch.equal(got, want)
    assert new_spy.take() == 0 and raw_spy.take() == 1
    entry = encoder.exact_report()[(0, B, 64, H, W, True)]
    assert entry["conv1"] == {"verified": False, "first_difference": "x"} and "conv1_recompute" not in entry


def test_the_small_shape_without_interference(monkeypatch):
    """The recompute form is compared exactly when the stored form matched, once, and runs afterwards only if it matched too."""
    from vqa_amd import encoder
    from vqa_amd.modules import run_conv_bn_stack
    _default_env(monkeypatch)
    monkeypatch.setattr(encoder, "_exact", {})
    new_spy, raw_spy = _Spy(monkeypatch, "_conv1_recompute_raw"), _Spy(monkeypatch, "_conv1_raw")
    seq = _first_group(2)
    img = _small_image()
    B, H, W = SMALL
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        run_conv_bn_stack(seq, img)
        entry = encoder.exact_report()[(0, B, 64, H, W, True)]
        print("small shape:", entry)
        assert raw_spy.take() == 1 and new_spy.take() == (1 if entry["conv1"]["verified"] else 0)
        assert ("conv1_recompute" in entry) == entry["conv1"]["verified"]
        run_conv_bn_stack(seq, img)
    route = entry["conv1"]["verified"]
    assert raw_spy.take() == (1 if route else 0)
    assert new_spy.take() == (1 if route and entry["conv1_recompute"]["verified"] else 0)


def test_the_switch_keeps_the_stored_form(monkeypatch):
    """VQA_ENCODER_CONV1_RECOMPUTE=0: _conv1_raw(..., want_x=False) and bn_exact with conv call the stored entry, with the same
    bits; unset, they call the new one."""
    from vqa_amd import encoder
    _default_env(monkeypatch)
    new_spy = _Spy(monkeypatch, "_conv1_recompute_raw")
    seq = _first_group(9)
    img = _small_image(10)
    results = {}
    for value in ("0", None, "1"):
        if value is None:
            monkeypatch.delenv("VQA_ENCODER_CONV1_RECOMPUTE", raising=False)
        else:
            monkeypatch.setenv("VQA_ENCODER_CONV1_RECOMPUTE", value)
        assert encoder.conv1_recompute_enabled() == (value != "0")
        bn = copy.deepcopy(seq[1])
        x, y, mean, invstd = encoder._conv1_raw(img, seq[0].weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, MOMENTUM, EPS,
                                                True, False)
        assert x is None and new_spy.take() == (0 if value == "0" else 1)
        y2 = encoder.bn_exact(img, copy.deepcopy(seq[1]), True, conv=seq[0])
        assert new_spy.take() == (0 if value == "0" else 1) and torch.equal(y2, y)
        results[value] = (y, mean, invstd, bn.running_mean, bn.running_var)
        # want_x is always the stored form, and `recompute` overrides the switch
        assert encoder._conv1_raw(img, seq[0].weight, bn.weight, bn.bias, bn.running_mean.clone(), bn.running_var.clone(), MOMENTUM,
                                  EPS, True, True)[0] is not None and new_spy.take() == 0
        encoder.bn_exact(img, copy.deepcopy(seq[1]), True, conv=seq[0], recompute=False)
        assert new_spy.take() == 0
    for value in (None, "1"):
        for a, b in zip(results[value], results["0"]):
            assert _same(a, b), value


def test_a_shape_verified_with_the_switch_off_is_compared_again(monkeypatch):
    """What runs is what was compared: a shape verified under VQA_ENCODER_CONV1_RECOMPUTE=0 holds no verdict on the recompute form,
    so the first call with the switch on compares again (made to match here: only the bookkeeping is under test)."""
    from vqa_amd import encoder
    _default_env(monkeypatch)
    monkeypatch.setattr(encoder, "_exact", {})
    monkeypatch.setattr(encoder, "_differs", lambda a, b: torch.zeros((), dtype=torch.bool, device=a.device))
    new_spy, raw_spy = _Spy(monkeypatch, "_conv1_recompute_raw"), _Spy(monkeypatch, "_conv1_raw")
    seq = _first_group(11)
    img = _small_image(12)
    key = (0, SMALL[0], 64, SMALL[1], SMALL[2], True)
    monkeypatch.setenv("VQA_ENCODER_CONV1_RECOMPUTE", "0")
    encoder.conv1_bn_exact_or_stock(img, seq[0], seq[1], seq[3])
    assert (raw_spy.take(), new_spy.take()) == (1, 0) and "conv1_recompute" not in encoder.exact_report()[key]
    encoder.conv1_bn_exact_or_stock(img, seq[0], seq[1], seq[3])              # the route: the stored form
    assert (raw_spy.take(), new_spy.take()) == (1, 0)
    monkeypatch.delenv("VQA_ENCODER_CONV1_RECOMPUTE")
    encoder.conv1_bn_exact_or_stock(img, seq[0], seq[1], seq[3])              # compared again, both forms
    assert (raw_spy.take(), new_spy.take()) == (1, 1)
    assert encoder.exact_report()[key]["conv1_recompute"] == {"verified": True, "first_difference": None}
    encoder.conv1_bn_exact_or_stock(img, seq[0], seq[1], seq[3])              # the route: the recompute form
    assert (raw_spy.take(), new_spy.take()) == (1, 1)


# ---- the benchmark's shape, in a process of its own ------------------------------------------------------------------------------------
def _bench_shape_check():
    """160 x 3 x 224 x 224 under the benchmark's own MIOpen find records: the route verifies both forms, and its output is the stock
    chain's."""
    import bench
    bench.seed_miopen_db()
    from vqa_amd import encoder
    from vqa_amd.modules import run_conv_bn_stack
    for name in SWITCHES:
        os.environ.pop(name, None)
    B, H, W = BENCH
    calls, real = [0], encoder._conv1_recompute_raw

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    def take():
        n, calls[0] = calls[0], 0
        return n
    encoder._conv1_recompute_raw = counted
    seq = _first_group(1)
    stock = copy.deepcopy(seq)
    g = torch.Generator(device=_dev()).manual_seed(7)
    img = _cl(torch.randn(B, 3, H, W, device=_dev(), generator=g))
    with torch.no_grad():
        os.environ["VQA_ENCODER_EXACT_CONV1"] = "0"
        wants = [run_conv_bn_stack(stock, img) for _ in range(3)]
        assert take() == 0
        del os.environ["VQA_ENCODER_EXACT_CONV1"]
        first = run_conv_bn_stack(seq, img)                                  # compares both forms
        state = encoder.exact_report()[(0, B, 64, H, W, True)]
        assert state["verified"] and state["conv1"] == {"verified": True, "first_difference": None}, state
        assert state["conv1_recompute"] == {"verified": True, "first_difference": None}, state
        assert take() == 1 and torch.equal(first, wants[0])
        del first
        second = run_conv_bn_stack(seq, img)                                 # the route: the recompute form
        assert take() == 1 and torch.equal(second, wants[1])
        del second
        os.environ["VQA_ENCODER_CONV1_RECOMPUTE"] = "0"
        third = run_conv_bn_stack(seq, img)                                  # the route: the stored form
        del os.environ["VQA_ENCODER_CONV1_RECOMPUTE"]
        assert take() == 0 and torch.equal(third, wants[2])
    for k, v in seq.state_dict().items():
        assert torch.equal(v, stock.state_dict()[k]), k
    print("bench shape ok")


def _bench_trainer_check():
    """Behind _bench_shape_check (both forms are verified by then): three Trainer steps at the benchmark's image shape with the
    recompute form on and off."""
    from vqa_amd import encoder
    from vqa_amd import train as T
    from vqa_amd.modules import HierarchicalCoAttentionNet
    B, H, W = BENCH
    dev = _dev()
    calls, real = [0], encoder._conv1_recompute_raw

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    encoder._conv1_recompute_raw = counted
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
        os.environ["VQA_ENCODER_CONV1_RECOMPUTE"] = route
        net = copy.deepcopy(net0).to(dev)
        net.image_encoder.to(memory_format=torch.channels_last)
        tr = T.Trainer(net, 1e-3, dev)
        losses = []
        for i, bt in enumerate(batches):
            nxt = batches[i + 1][0] if i + 1 < len(batches) else None
            losses.append(tr.step(*bt, next_image=nxt).detach().clone())
        torch.cuda.synchronize()
        runs[route] = (torch.stack(losses).cpu(), {k: v.detach().cpu() for k, v in net.state_dict().items()})
        assert calls[0] == (0 if route == "0" else 3), (route, calls[0])      # one encoder pass per batch
        calls[0] = 0
    del os.environ["VQA_ENCODER_CONV1_RECOMPUTE"]
    assert torch.equal(runs["1"][0], runs["0"][0]), (runs["1"][0].tolist(), runs["0"][0].tolist())
    for k, v in runs["0"][1].items():
        assert _same(runs["1"][1][k].float(), v.float()), k
    print("bench trainer ok")


@functools.lru_cache(maxsize=None)
def _bench_process(db_dir):
    """One process of its own for both checks at the benchmark's shape, its MIOpen user database a fresh directory holding the
    benchmark's find records (bench.seed_miopen_db): the pattern of tests/test_gpu_encoder_conv1.py."""
    env = dict(os.environ, MIOPEN_USER_DB_PATH=db_dir)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--bench-shape"], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    return r.stdout


def test_both_forms_verify_at_the_benchmarks_shape(tmp_path_factory):
    out = _bench_process(str(tmp_path_factory.getbasetemp() / "conv1_recompute_miopen_db"))
    assert "bench shape ok" in out, out[-3000:]


def test_trainer_steps_are_equal_with_recompute_on_and_off(tmp_path_factory):
    out = _bench_process(str(tmp_path_factory.getbasetemp() / "conv1_recompute_miopen_db"))
    assert "bench trainer ok" in out, out[-3000:]


if __name__ == "__main__" and sys.argv[1:] == ["--bench-shape"]:
    sys.path.insert(0, ROOT)
    _bench_shape_check()
    _bench_trainer_check()

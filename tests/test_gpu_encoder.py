"""The frozen encoder's train-mode BatchNorm + ReLU + 2x2 max-pool on the GPU (include/coattn.h v0.14.0, csrc/encoder.hip,
vqa_amd/encoder.py): values against a float64 chain with the stock fp32 chain's own error as the yardstick, memory
isolation, repeatability, NaN, stream, offsets past 2^31 bytes, and the encoder / trainer level routes."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-5, 0.1
# (B, C, H, W, pool, input mean, input std)
CASES = ((2, 64, 4, 4, True, 0.0, 1.0),
         (3, 16, 5, 7, True, 0.0, 1.0),          # odd sides: floor mode drops the last row and column
         (1, 128, 2, 2, True, 0.0, 1.0),         # one output pixel
         (6, 512, 6, 6, False, 0.0, 1.0),
         (2, 256, 3, 3, False, 0.0, 1.0),
         (5, 64, 9, 11, True, 0.0, 1.0),         # rows that are no multiple of any tile
         (4, 64, 32, 32, True, 30.0, 0.5),       # ten statistics workgroups; |mean| >> std
         (5, 64, 9, 11, True, 1000.0, 3.0))


def _dev():
    return torch.device("cuda:0")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def make_inputs(idx, batches=1):
    """x batches (channels_last fp32), gamma (channel 0 negative), beta, conv bias (odd cases only); channel 1 is constant."""
    B, Ch, H, W, pool, mean, std = CASES[idx]
    g = torch.Generator().manual_seed(100 + idx)
    gamma = 0.5 + torch.rand(Ch, generator=g)
    gamma[0] = -gamma[0]
    beta = 0.5 * torch.randn(Ch, generator=g)
    bias = torch.randn(Ch, generator=g).to(_dev()) if idx % 2 else None
    xs = []
    for _ in range(batches):                       # (drawn last: the first batch does not depend on how many follow)
        x = mean + std * torch.randn(B, Ch, H, W, generator=g)
        x[:, 1] = mean + 0.5
        xs.append(_cl(x.to(_dev())))
    return xs, gamma.to(_dev()), beta.to(_dev()), bias


def chain(x, gamma, beta, pool, dtype):
    """batch_norm (batch statistics) -> max_pool2d(2, 2) if pooled -> relu, in `dtype`, on the device."""
    t = F.batch_norm(x.to(dtype), None, None, gamma.to(dtype), beta.to(dtype), True, 0.0, EPS)
    if pool:
        t = F.max_pool2d(t, 2, 2)
    return F.relu(t)


def make_bn(Ch, gamma, beta, dtype=torch.float32, seed=7):
    bn = torch.nn.BatchNorm2d(Ch, eps=EPS, momentum=MOMENTUM).to(_dev(), dtype)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(torch.randn(Ch, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(Ch, generator=g))
    for p in bn.parameters():
        p.requires_grad = False
    return bn.train()


def bound(stock, ref64):
    """2 max|stock - ref64| + 2^-22 max|ref64|: the stock chain's own error, a factor 2 for one differently-ordered rounding,
    and a floor for a stock chain that happens to be exact."""
    return 2.0 * (stock.double() - ref64).abs().max().item() + 2.0 ** -22 * ref64.abs().max().item()


def err(y, ref64):
    return (y.double() - ref64).abs().max().item()


@functools.lru_cache(maxsize=None)
def references(idx):
    """(ref64, stock) of the case's first batch, computed once and not modified by the tests that share them."""
    xs, gamma, beta, _ = make_inputs(idx)
    pool = CASES[idx][4]
    return chain(xs[0], gamma, beta, pool, torch.float64), chain(xs[0], gamma, beta, pool, torch.float32)


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_parity_with_the_float64_chain(idx):
    from vqa_amd import encoder
    B, Ch, H, W, pool, _, _ = CASES[idx]
    xs, gamma, beta, bias = make_inputs(idx, batches=3)
    ref64, stock = references(idx)
    bn = make_bn(Ch, gamma, beta)
    stats = torch.full((2, Ch), float("nan"), device=_dev())
    y = encoder.bn_relu_pool(xs[0], bn, conv_bias=bias, pool=pool, stats_out=stats)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    assert tuple(y.shape) == (B, Ch, Ho, Wo) and y.dtype == torch.float32
    assert y.stride() == (Ho * Wo * Ch, 1, Wo * Ch, Ch)
    e, lim = err(y, ref64), bound(stock, ref64)
    print("case", CASES[idx], "y err %.3e stock err %.3e bound %.3e" % (e, err(stock, ref64), lim))
    assert e <= lim
    assert torch.isfinite(y).all()                                           # the constant channel included
    # the batch statistics: float64 against torch's fp32 reduction
    x64 = xs[0].double()
    var64, mean64 = torch.var_mean(x64, dim=(0, 2, 3), unbiased=False)
    var32, mean32 = torch.var_mean(xs[0], dim=(0, 2, 3), unbiased=False)
    for name, got, want, stk in (("mean", stats[0], mean64, mean32), ("var", stats[1], var64, var32)):
        e, lim = err(got, want), bound(stk, want)
        print("  %s err %.3e bound %.3e" % (name, e, lim))
        assert e <= lim, name
    # running statistics after three different batches, against stock BatchNorm2d modules fed conv output + bias
    stock_bn, ref_bn = make_bn(Ch, gamma, beta), make_bn(Ch, gamma, beta, torch.float64)
    shift = 0 if bias is None else bias.view(1, -1, 1, 1)
    for k, x in enumerate(xs):
        if k:
            encoder.bn_relu_pool(x, bn, conv_bias=bias, pool=pool)
        stock_bn(_cl(x + shift))
        ref_bn(x.double() + (0 if bias is None else shift.double()))
    for name in ("running_mean", "running_var"):
        got, want, stk = getattr(bn, name), getattr(ref_bn, name), getattr(stock_bn, name)
        e, lim = err(got, want), bound(stk, want)
        print("  %s err %.3e bound %.3e" % (name, e, lim))
        assert e <= lim, name
    assert int(bn.num_batches_tracked) == int(stock_bn.num_batches_tracked) == 3


def _raw_call(x, gamma, beta, bias, rm, rv, y, stats, ws, pool, stream=None):
    from vqa_amd import _lib
    B, Ch, H, W = x.shape
    rc = _lib.load().coattn_bn_relu_pool_forward(_lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(bias), _lib.ptr(rm),
                                                 _lib.ptr(rv), MOMENTUM, EPS, _lib.ptr(y), _lib.ptr(stats), _lib.ptr(ws),
                                                 B, H, W, Ch, int(pool), 1, _lib.F32,
                                                 C.c_void_p(_lib.stream_ptr(x.device) if stream is None else stream))
    _lib.check(rc, "coattn_bn_relu_pool_forward")


@pytest.mark.parametrize("idx", (1, 4, 5, 6))
def test_guard_bands(idx):
    """y and the workspace are carved out of larger buffers filled with a marker: not a word outside them changes, every word
    of y is written, and the inputs stay what they were."""
    from vqa_amd import _lib
    B, Ch, H, W, pool, _, _ = CASES[idx]
    xs, gamma, beta, bias = make_inputs(idx)
    x = xs[0]
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    ny, nws, pad = B * Ch * Ho * Wo, (_lib.load().coattn_bn_workspace_bytes(B, H, W, Ch) + 3) // 4, 4096
    marker = 12345.5
    ybig = torch.full((pad + ny + pad,), marker, device=_dev())
    wsbig = torch.full((pad + nws + pad,), marker, device=_dev())
    small = torch.full((6, pad + Ch + pad), marker, device=_dev())      # gamma, beta, rm, rv and the two rows of stats_out
    small[0, pad:pad + Ch], small[1, pad:pad + Ch] = gamma, beta
    small[2, pad:pad + Ch], small[3, pad:pad + Ch] = 0.0, 1.0
    stats = small[4:6, pad:pad + Ch]
    keep = [t.clone() for t in (x, gamma, beta)] + ([bias.clone()] if bias is not None else [])
    y = ybig[pad:pad + ny]
    y.fill_(float("nan"))
    _raw_call(x, small[0, pad:], small[1, pad:], bias, small[2, pad:], small[3, pad:], y, None, wsbig[pad:], pool)
    torch.cuda.synchronize()
    for big, n in ((ybig, ny), (wsbig, nws)):
        assert (big[:pad] == marker).all() and (big[pad + n:] == marker).all()
    assert (small[:, :pad] == marker).all() and (small[:, pad + Ch:] == marker).all()
    assert (stats == marker).all()                                        # stats_out was NULL
    assert torch.equal(small[0, pad:pad + Ch], gamma) and torch.equal(small[1, pad:pad + Ch], beta)
    assert not torch.isnan(y).any()
    for t, k in zip((x, gamma, beta, bias), keep):
        assert torch.equal(t, k)
    ref64, stock = references(idx)
    got = y.view(B, Ho, Wo, Ch).permute(0, 3, 1, 2)
    assert err(got, ref64) <= bound(stock, ref64)


def test_two_calls_give_the_same_bits():
    from vqa_amd import encoder
    for idx in (6, 3):
        B, Ch, H, W, pool, _, _ = CASES[idx]
        xs, gamma, beta, bias = make_inputs(idx)
        outs = []
        for _ in range(2):
            bn = make_bn(Ch, gamma, beta)
            stats = torch.zeros(2, Ch, device=_dev())
            y = encoder.bn_relu_pool(xs[0], bn, conv_bias=bias, pool=pool, stats_out=stats)
            outs.append((y, stats, bn.running_mean.clone(), bn.running_var.clone()))
        for a, b in zip(*outs):
            assert torch.equal(a, b)


@pytest.mark.parametrize("pool", (True, False))
def test_nan_propagates_as_in_the_stock_chain(pool):
    from vqa_amd import encoder
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 64, 8, 8, generator=g)
    x[1, 3, 2, 1] = float("nan")
    x = _cl(x.to(_dev()))
    gamma, beta = (0.5 + torch.rand(64, generator=g)).to(_dev()), torch.randn(64, generator=g).to(_dev())
    stock = chain(x, gamma, beta, pool, torch.float32)
    y = encoder.bn_relu_pool(x, make_bn(64, gamma, beta), pool=pool)
    assert torch.equal(torch.isnan(y), torch.isnan(stock))
    assert torch.isnan(y[:, 3]).all() and not torch.isnan(y[:, :3]).any() and not torch.isnan(y[:, 4:]).any()


def test_runs_on_the_current_side_stream():
    """x is written late on a side stream (behind milliseconds of matmuls); the call made under that stream must see it.  Only
    the side stream is synchronised."""
    from vqa_amd import encoder
    idx = 6
    B, Ch, H, W, pool, _, _ = CASES[idx]
    xs, gamma, beta, bias = make_inputs(idx)
    src = xs[0]
    bn0, bn1 = make_bn(Ch, gamma, beta), make_bn(Ch, gamma, beta)
    want = encoder.bn_relu_pool(src, bn0, conv_bias=bias, pool=pool)
    x = _cl(torch.zeros_like(src))
    a = torch.randn(4096, 4096, device=_dev()) / 64.0
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = a
        for _ in range(6):
            t = t @ a
        x.copy_(src)
        y = encoder.bn_relu_pool(x, bn1, conv_bias=bias, pool=pool)
    side.synchronize()
    assert torch.equal(y, want)
    assert torch.equal(bn1.running_mean, bn0.running_mean) and torch.equal(bn1.running_var, bn0.running_var)
    assert torch.isfinite(t).all()


def test_byte_offsets_past_2_31():
    """x = [1, 64, 2, 2^22 + 2]: 2^29 + 256 elements, 2.147 GB, so byte offsets pass 2^31 while the shape is still supported.
    The whole pooled y and, on their own, its last 1000 pixels meet the parity bound.  A float64 copy of x would cost 4 GB:
    the float64 chain is formed in slices along W from float64 statistics that are summed in slices too; the stock fp32
    chain (whole tensor) supplies the bound's error term as in the parity test."""
    from vqa_amd import encoder
    Ch, H, W = 64, 2, 2 ** 22 + 2
    g = torch.Generator(device=_dev()).manual_seed(11)
    xp = torch.randn(1, H, W, Ch, device=_dev(), generator=g)               # physical NHWC
    x = xp.permute(0, 3, 1, 2)
    assert x.is_contiguous(memory_format=torch.channels_last) and x.numel() * 4 > 2 ** 31
    gamma = 0.5 + torch.rand(Ch, device=_dev(), generator=g)
    gamma[0] = -gamma[0]
    beta = torch.randn(Ch, device=_dev(), generator=g)
    y = encoder.bn_relu_pool(x, make_bn(Ch, gamma, beta), pool=True)
    Wo = W // 2
    assert tuple(y.shape) == (1, Ch, 1, Wo) and y.stride() == (Wo * Ch, 1, Wo * Ch, Ch)
    stock = chain(x, gamma, beta, True, torch.float32)
    step = 2 ** 19
    edges = list(range(0, W, step)) + [W]                                   # even edges: windows do not straddle slices
    s = torch.zeros(Ch, device=_dev(), dtype=torch.float64)
    q = torch.zeros_like(s)
    for w0, w1 in zip(edges[:-1], edges[1:]):
        xc = xp[0, :, w0:w1].double()
        s += xc.sum(dim=(0, 1))
        q += (xc * xc).sum(dim=(0, 1))
    n = float(H * W)
    mean = s / n
    scale = gamma.double() / torch.sqrt(q / n - mean * mean + EPS)
    yp, sp = y.permute(0, 2, 3, 1)[0, 0], stock.permute(0, 2, 3, 1)[0, 0]   # [Wo, C] views

    def errors(w0, w1):
        """(y error, stock error, max|ref64|) over the input columns [w0, w1), both even"""
        t = (xp[0, :, w0:w1].double() - mean) * scale + beta.double()
        r = torch.relu(t.view(H, (w1 - w0) // 2, 2, Ch).amax(dim=(0, 2)))
        return ((yp[w0 // 2:w1 // 2].double() - r).abs().max().item(), (sp[w0 // 2:w1 // 2].double() - r).abs().max().item(),
                r.abs().max().item())

    e_y = e_s = m = 0.0
    for w0, w1 in zip(edges[:-1], edges[1:]):
        a, b, c = errors(w0, w1)
        e_y, e_s, m = max(e_y, a), max(e_s, b), max(m, c)
    tail_y, tail_s, tail_m = errors(W - 2000, W)
    print("whole: y err %.3e stock err %.3e; last 1000 pixels: y err %.3e stock err %.3e; max|y - stock| %.3e"
          % (e_y, e_s, tail_y, tail_s, (y - stock).abs().max().item()))
    assert e_y <= 2.0 * e_s + 2.0 ** -22 * m
    assert tail_y <= 2.0 * tail_s + 2.0 ** -22 * tail_m


class _Spy:
    def __init__(self, monkeypatch, name="bn_relu_pool"):
        from vqa_amd import encoder
        self.calls, real = 0, getattr(encoder, name)

        def counted(*a, **k):
            self.calls += 1
            return real(*a, **k)
        monkeypatch.setattr(encoder, name, counted)

    def take(self):
        n, self.calls = self.calls, 0
        return n


def _encoder(trainable=False, seed=0):
    from vqa_amd.modules import ImageCoAttentionEncoder
    torch.manual_seed(seed)
    return ImageCoAttentionEncoder(is_trainable=trainable, weights_path=None).to(_dev())


@pytest.mark.parametrize("B,side", ((4, 64), (3, 100)))                   # 100 -> 50 -> 25 -> 12 -> 6 -> 3: floor mode on the way
def test_encoder_matches_the_stock_route(monkeypatch, B, side):
    spy = _Spy(monkeypatch)
    enc = _encoder().to(memory_format=torch.channels_last)
    ref = copy.deepcopy(enc)
    g = torch.Generator().manual_seed(side)
    for _ in range(3):
        x = _cl(torch.randn(B, 3, side, side, generator=g).to(_dev()))
        monkeypatch.setenv("VQA_ENCODER_FUSED", "0")
        want = ref(x)
        assert spy.take() == 0
        monkeypatch.setenv("VQA_ENCODER_FUSED", "1")
        got = enc(x)
        assert spy.take() == 8
        assert got.shape == want.shape and got.stride() == want.stride()
        tol = 2e-3 * want.abs().max().item()
        print("features differ by %.3e (tolerance %.3e)" % ((got - want).abs().max().item(), tol))
        assert (got - want).abs().max().item() <= tol
    bufs, ref_bufs = dict(enc.named_buffers()), dict(ref.named_buffers())
    assert len(bufs) == 24
    for k, v in bufs.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref_bufs[k]) == 3
        else:
            assert (v - ref_bufs[k]).abs().max().item() <= tol, k


def test_encoder_routes_that_stay_stock(monkeypatch):
    spy = _Spy(monkeypatch)
    monkeypatch.setenv("VQA_ENCODER_FUSED", "1")
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(_dev())
    _encoder()(x)                                                            # NCHW weights and input
    assert spy.take() == 0
    enc = _encoder().to(memory_format=torch.channels_last)
    enc(_cl(x))
    assert spy.take() == 8
    enc.eval()
    enc(_cl(x))
    assert spy.take() == 0
    enc.train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        enc(_cl(x))
    assert spy.take() == 0
    trainable = _encoder(trainable=True).to(memory_format=torch.channels_last)
    out = trainable(_cl(x))
    assert spy.take() == 0 and out.requires_grad


def test_runahead_with_a_channels_last_encoder(monkeypatch):
    """tests/test_gpu_net.py::test_encoder_runahead_is_value_preserving's schedule and tolerances with the encoder and the
    image batches in channels_last: the fused passes run on the encoder stream one step ahead."""
    from vqa_amd import train as T
    from vqa_amd.modules import HierarchicalCoAttentionNet
    spy = _Spy(monkeypatch)
    monkeypatch.setenv("VQA_ENCODER_FUSED", "1")
    dev = _dev()
    qp = dict(vocab_size=60, word_emb_dim=512, hidden_dim=512)
    torch.manual_seed(3)
    net0 = HierarchicalCoAttentionNet(qp, dict(is_trainable=False, weights_path=None), K=11)
    batches = []
    for s in range(5):
        b = T.synthetic_batch(6, (96, 96), 26, 60, 11, seed=50 + s)
        image, question, label, lens = T.sort_batch(b["image"], b["question"], b["label"], b["ques_len"])
        batches.append((_cl(image.to(dev)), question.to(dev), lens, label.to(dev)))
    runs = {}
    for ahead in (False, True):
        net = copy.deepcopy(net0).to(dev)
        net.image_encoder.to(memory_format=torch.channels_last)
        tr = T.Trainer(net, 1e-3, dev, encoder_runahead=ahead)
        assert tr.runahead == ahead
        losses = []
        for i, bt in enumerate(batches):
            nxt = batches[i + 1][0] if i + 1 < len(batches) else None
            losses.append(float(tr.step(*bt, next_image=nxt).detach()))
        torch.cuda.synchronize()
        assert spy.take() == 8 * len(batches)
        runs[ahead] = (losses, {k: v.detach().cpu() for k, v in net.state_dict().items()})
    print("losses", runs[False][0], runs[True][0])
    assert np.allclose(runs[False][0], runs[True][0], rtol=1e-4, atol=0)
    for k, v in runs[False][1].items():
        if k.startswith("image_encoder."):
            assert torch.allclose(v.float(), runs[True][1][k].float(), rtol=1e-4, atol=1e-5), k


# ---- the exact pool + ReLU pass (the default route) ----------------------------------------------------------------------
POOL_CASES = ((2, 64, 4, 4), (3, 16, 5, 7), (1, 128, 2, 2), (5, 64, 9, 11), (2, 512, 6, 6), (4, 64, 64, 64), (3, 256, 33, 35))


@pytest.mark.parametrize("shape", POOL_CASES)
def test_relu_pool_has_the_stock_kernels_bits(shape):
    """max and ReLU are exact: torch.equal against max_pool2d + relu, NaNs in the same places, the input untouched."""
    from vqa_amd import encoder
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g)
    x[0, 1, 0, 1] = float("nan")
    x[-1, 2, 1, 0] = float("inf")
    x = _cl(x.to(_dev()))
    keep = x.clone()
    want = F.relu(F.max_pool2d(x, 2, 2))
    y = encoder.relu_pool(x)
    B, Ch, H, W = shape
    assert tuple(y.shape) == (B, Ch, H // 2, W // 2) and y.stride() == ((H // 2) * (W // 2) * Ch, 1, (W // 2) * Ch, Ch)
    assert torch.equal(torch.isnan(y), torch.isnan(want)) and torch.isnan(y).any()
    assert torch.equal(torch.nan_to_num(y, nan=-1.0), torch.nan_to_num(want, nan=-1.0))
    assert torch.equal(torch.nan_to_num(x, nan=-1.0), torch.nan_to_num(keep, nan=-1.0))


def test_relu_pool_guard_bands_and_offsets_past_2_31():
    from vqa_amd import _lib
    Ch, H, W = 64, 2, 2 ** 22 + 2
    xp = torch.randn(1, H, W, Ch, device=_dev(), generator=torch.Generator(device=_dev()).manual_seed(3))
    x = xp.permute(0, 3, 1, 2)
    ny, pad, marker = (W // 2) * Ch, 4096, 12345.5
    ybig = torch.full((pad + ny + pad,), marker, device=_dev())
    y = ybig[pad:pad + ny]
    y.fill_(float("nan"))
    _lib.check(_lib.load().coattn_relu_pool_forward(_lib.ptr(x), _lib.ptr(y), 1, H, W, Ch, _lib.F32,
                                                    C.c_void_p(_lib.stream_ptr(x.device))), "coattn_relu_pool_forward")
    torch.cuda.synchronize()
    assert (ybig[:pad] == marker).all() and (ybig[pad + ny:] == marker).all()
    want = F.relu(F.max_pool2d(x, 2, 2)).permute(0, 2, 3, 1).reshape(-1)
    assert torch.equal(y, want)


def test_default_route_is_the_exact_pool_pass_only(monkeypatch):
    """Without VQA_ENCODER_FUSED the encoder takes relu_pool for its five pools and never the BatchNorm kernels; every pool
    output has the stock bits, so the features agree with the all-stock route as two stock passes do."""
    bn_spy, pool_spy = _Spy(monkeypatch), _Spy(monkeypatch, "relu_pool")
    monkeypatch.delenv("VQA_ENCODER_FUSED", raising=False)
    enc = _encoder().to(memory_format=torch.channels_last)
    ref = copy.deepcopy(enc)
    x = _cl(torch.randn(3, 3, 100, 100, generator=torch.Generator().manual_seed(2)).to(_dev()))
    got = enc(x)
    assert (bn_spy.take(), pool_spy.take()) == (0, 5)
    monkeypatch.setenv("VQA_ENCODER_FUSED", "0")
    want = ref(x)
    assert (bn_spy.take(), pool_spy.take()) == (0, 0)
    assert got.shape == want.shape and got.stride() == want.stride()
    assert (got - want).abs().max().item() <= 2e-3 * want.abs().max().item()
    monkeypatch.delenv("VQA_ENCODER_FUSED")
    _encoder()(x.contiguous())                                              # NCHW
    assert pool_spy.take() == 0
    enc.eval()
    enc(x)
    assert pool_spy.take() == 5                                              # (eval mode: the pool pass does not depend on BatchNorm)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        enc(x)
    assert pool_spy.take() == 0
    out = _encoder(trainable=True).to(memory_format=torch.channels_last)(x)
    assert pool_spy.take() == 0 and out.requires_grad

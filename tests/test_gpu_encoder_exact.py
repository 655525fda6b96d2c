"""The frozen encoder's BatchNorm + ReLU + 2x2 max-pool with the STOCK kernels' bits (include/coattn.h v0.15.0, csrc/encoder.hip,
vqa_amd/encoder.py bn_exact).  Every comparison is torch.equal (NaNs in the same places first) against the stock chain on
channels_last fp32: nn.BatchNorm2d in train mode, then F.relu, or F.relu(F.max_pool2d(., 2, 2)); the saved statistics against
torch.miopen_batch_norm's."""
import copy
import functools
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-5, 0.1
CHANNELS = (64, 128, 256, 512)
CAP_BYTES = 512 * 2 ** 20


def _dev():
    return torch.device("cuda:0")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _same_layout(a, b):
    """Equal shapes, and equal strides wherever the size is above 1 (the stride of a dimension of size 1 is arbitrary)."""
    return a.shape == b.shape and all(sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()) if n > 1)


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))


# ---- the shape list, from the geometry rule -----------------------------------------------------------------------------
PROPERTIES = {
    "more than one sample per thread": lambda g, B, H, W, Ch: g["samples_per_thread"] > 1,
    "the final kernel's strided loop makes a second trip": lambda g, B, H, W, Ch: g["pixel_groups"] > g["f1"],
    "more than one workgroup along C": lambda g, B, H, W, Ch: Ch // g["vec"] > g["g0"],
    "a masked tail of pixels": lambda g, B, H, W, Ch: (H * W) % g["g1"] != 0,
    "odd H and odd W": lambda g, B, H, W, Ch: H % 2 == 1 and W % 2 == 1,
}


@functools.lru_cache(maxsize=None)
def shape_list():
    """For each C and each property the covered (B, C, H, W) of smallest B H W that has it (H, W >= 2: every shape is also
    pooled), candidates in order of B H W, then B, then H.  "More than one workgroup along C" depends on C alone (C / 4 > 16):
    C = 64 has no such shape and the three other C have it in every shape.  Smallest size found: every property but the
    second trip is met at B H W <= 15 (a few KiB); the second trip needs H W > 8 g1^2, 514 pixels at C <= 256 (513 = 1 modulo
    8 is not covered) and 2050 at C = 512 (4.2 MB) -- far below the 512 MiB cap."""
    from vqa_amd import encoder
    cands = sorted(((B * H * W, B, H, W) for B in (1, 2, 3) for H in range(2, 49) for W in range(H, 49)))
    shapes = []
    for Ch in CHANNELS:
        for name, has in PROPERTIES.items():
            for _, B, H, W in cands:
                g = encoder.exact_geometry(B, H, W, Ch)
                if g is not None and has(g, B, H, W, Ch) and B * H * W * Ch * 4 <= CAP_BYTES:
                    if (B, Ch, H, W) not in shapes:
                        shapes.append((B, Ch, H, W))
                    break
            else:
                assert name == "more than one workgroup along C" and Ch == 64, (Ch, name)
    return tuple(shapes)


def test_the_shape_list_has_every_property():
    from vqa_amd import encoder
    shapes = shape_list()
    for Ch in CHANNELS:
        mine = [(s, encoder.exact_geometry(s[0], s[2], s[3], Ch)) for s in shapes if s[1] == Ch]
        for name, has in PROPERTIES.items():
            if not (name == "more than one workgroup along C" and Ch == 64):
                assert any(has(g, s[0], s[2], s[3], Ch) for s, g in mine), (Ch, name)
    assert {encoder.exact_geometry(s[0], s[2], s[3], s[1])["g1"] for s in shapes} == {8, 16}   # both workgroup shapes
    assert all(s[0] * s[1] * s[2] * s[3] * 4 <= CAP_BYTES for s in shapes)


# ---- the two chains -------------------------------------------------------------------------------------------------------
def _params(Ch, seed, gamma=None):
    g = torch.Generator().manual_seed(seed)
    gamma = 0.5 + torch.rand(Ch, generator=g) if gamma is None else gamma
    return gamma.to(_dev()), (0.5 * torch.randn(Ch, generator=g)).to(_dev()), torch.randn(Ch, generator=g).to(_dev()), \
        (0.5 + torch.rand(Ch, generator=g)).to(_dev())


def _bn(Ch, params):
    gamma, beta, rm, rv = params
    bn = torch.nn.BatchNorm2d(Ch, eps=EPS, momentum=MOMENTUM).to(_dev())
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    return bn.train().requires_grad_(False)


def compare(xs, Ch, pool, params):
    """The stock chain and bn_exact over the batches `xs`, each on its own BatchNorm2d: y of every call, the saved statistics
    of every call and the running statistics after the last must be the stock ones'."""
    from vqa_amd import encoder
    stock, mine = _bn(Ch, params), _bn(Ch, params)
    for i, x in enumerate(xs):
        keep = x.clone()
        rm, rv = stock.running_mean.clone(), stock.running_var.clone()
        _, save_mean, save_invstd = torch.miopen_batch_norm(x, stock.weight, stock.bias, rm, rv, True, MOMENTUM, EPS)
        z = stock(x)
        want = F.relu(F.max_pool2d(z, 2, 2)) if pool else F.relu(z)
        got, mean, invstd = encoder._bn_exact_raw(x, mine.weight, mine.bias, mine.running_mean, mine.running_var, MOMENTUM, EPS,
                                                  pool)
        assert _same_layout(got, want)
        for name, a, b in (("y", got, want), ("save_mean", mean, save_mean), ("save_invstd", invstd, save_invstd),
                           ("running_mean", mine.running_mean, stock.running_mean),
                           ("running_var", mine.running_var, stock.running_var), ("x", x, keep)):
            assert _same(a, b), (name, "call %d" % i, tuple(x.shape), pool)
    return got, mine


def _batches(shape, seed, n=3, mean=0.0, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return [_cl((mean + std * torch.randn(*shape, generator=g)).to(_dev())) for _ in range(n)]


def test_bits_on_every_listed_shape():
    """Three consecutive calls on fresh inputs, with and without the pool, on every shape of the list: the running statistics
    compound.  Every listed shape must also come out verified by the route's own comparison."""
    from vqa_amd import encoder
    for shape in shape_list():
        B, Ch, H, W = shape
        for pool in (True, False):
            compare(_batches(shape, B + H + W), Ch, pool, _params(Ch, Ch + H))
            bn = _bn(Ch, _params(Ch, 1))
            encoder.bn_exact_or_stock(_batches(shape, 5, n=1)[0], bn, torch.nn.MaxPool2d(2, 2) if pool else None)
            state = encoder.exact_report()[(0, B, Ch, H, W, pool)]
            assert state["verified"] and state["first_difference"] is None, (shape, pool, state)


def _separating_shapes():
    shapes = shape_list()
    return (next(s for s in shapes if s[1] == 128), next(s for s in reversed(shapes) if s[1] == 256), shapes[0])


@pytest.mark.parametrize("kind", ("mean 1000, std 3", "a constant channel", "negative and zero gamma", "subnormal", "near 1e19",
                                  "one huge and one subnormal channel", "one NaN and one inf"))
def test_inputs_that_separate_the_candidates(kind):
    """fused or unfused multiply-adds, the contraction of the running-variance update, the denormal mode, the reciprocal square
    root and max's treatment of a NaN variance each change a bit on one of these."""
    for n, shape in enumerate(_separating_shapes()):
        B, Ch, H, W = shape
        gamma = None
        xs = _batches(shape, 40 + n, mean=1000.0 if kind.startswith("mean") else 0.0, std=3.0 if kind.startswith("mean") else 1.0)
        for x in xs:
            if kind == "a constant channel":
                x[:, 1] = 2.5
                x[:, 5] = 0.0
            elif kind == "subnormal":
                x.mul_(1e-41)
            elif kind == "near 1e19":
                x.mul_(1e19)
            elif kind.startswith("one huge"):
                x[:, 2] *= 1e19
                x[:, 7] *= 1e-41
            elif kind.startswith("one NaN"):
                x[0, 3, 0, 0] = float("nan")
                x[B - 1, 9, H - 1, W - 1] = float("inf")
                x[0, 11, 1, 1] = float("-inf")
        if kind.startswith("negative"):
            gamma = torch.randn(Ch, generator=torch.Generator().manual_seed(9))
            gamma[::3] = 0.0
        for pool in (True, False):
            y, bn = compare(xs, Ch, pool, _params(Ch, 3, gamma))
            if kind == "a constant channel":
                assert torch.equal(y[:, 5], torch.relu(bn.bias[5]).expand_as(y[:, 5]))       # the variance clamps to 0: y = beta
            if kind.startswith("one NaN"):
                assert torch.isnan(y[:, 3]).all() and not torch.isnan(y[:, 4]).any()


# ---- the route ------------------------------------------------------------------------------------------------------------
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


def _encoder(trainable=False, seed=0):
    from vqa_amd.modules import ImageCoAttentionEncoder
    torch.manual_seed(seed)
    return ImageCoAttentionEncoder(is_trainable=trainable, weights_path=None).to(_dev())


def _default_env(monkeypatch):
    """The default switches -- and deterministic convolution algorithms: the references below are second runs of the stock
    convolutions, which are comparable bit for bit only then."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    monkeypatch.delenv("VQA_ENCODER_FUSED", raising=False)
    monkeypatch.delenv("VQA_ENCODER_EXACT_BN", raising=False)


def _forget(monkeypatch):
    """A fresh per-shape record for this test (the record is the process's)."""
    from vqa_amd import encoder
    monkeypatch.setattr(encoder, "_exact", {})


def test_encoder_route_has_the_stock_bits(monkeypatch):
    """B = 5 at 88 x 104 px: 88 -> 44 -> 22 -> 11 -> 5 -> 2 and 104 -> 52 -> 26 -> 13 -> 6 -> 3, floor mode on the way; all eight
    layers are covered (a square odd side is not: its H W is 1 modulo 8)."""
    from vqa_amd import encoder
    _default_env(monkeypatch)
    _forget(monkeypatch)
    exact_spy, pool_spy, old_spy = _Spy(monkeypatch, "bn_exact"), _Spy(monkeypatch, "relu_pool"), _Spy(monkeypatch, "bn_relu_pool")
    enc = _encoder().to(memory_format=torch.channels_last)
    ref = copy.deepcopy(enc)
    g = torch.Generator().manual_seed(88)
    for step in range(3):
        x = _cl(torch.randn(5, 3, 88, 104, generator=g).to(_dev()))
        monkeypatch.setenv("VQA_ENCODER_FUSED", "0")
        want = ref(x)
        assert (exact_spy.take(), pool_spy.take()) == (0, 0)
        monkeypatch.delenv("VQA_ENCODER_FUSED")
        got = enc(x)
        # the first forward compares: the stock chain's result, relu_pool on the five pools; then bn_exact on every layer
        assert (exact_spy.take(), pool_spy.take(), old_spy.take()) == ((0, 5, 0) if step == 0 else (8, 0, 0))
        assert _same_layout(got, want)
        assert torch.equal(got, want), "step %d" % step
    report = encoder.exact_report()
    assert len(report) == 8 and all(v["verified"] and v["geometry"] for v in report.values())
    bufs, ref_bufs = dict(enc.named_buffers()), dict(ref.named_buffers())
    assert len(bufs) == 24
    for k, v in bufs.items():
        assert torch.equal(v, ref_bufs[k]), k
        assert not k.endswith("num_batches_tracked") or int(v) == 3


def test_routes_that_stay_stock(monkeypatch):
    from vqa_amd import encoder
    _default_env(monkeypatch)
    _forget(monkeypatch)
    exact_spy, route_spy = _Spy(monkeypatch, "bn_exact"), _Spy(monkeypatch, "bn_exact_or_stock")
    x = _cl(torch.randn(5, 3, 88, 104, generator=torch.Generator().manual_seed(1)).to(_dev()))
    enc = _encoder().to(memory_format=torch.channels_last)
    enc(x), enc(x)
    assert (exact_spy.take(), route_spy.take()) == (8, 16)
    monkeypatch.setenv("VQA_ENCODER_EXACT_BN", "0")
    enc(x)
    assert (exact_spy.take(), route_spy.take()) == (0, 0)
    monkeypatch.delenv("VQA_ENCODER_EXACT_BN")
    for value in ("0", "1"):
        monkeypatch.setenv("VQA_ENCODER_FUSED", value)
        enc(x)
        assert (exact_spy.take(), route_spy.take()) == (0, 0)
    monkeypatch.delenv("VQA_ENCODER_FUSED")
    _encoder()(x.contiguous())                                              # NCHW weights and input
    enc.eval()
    enc(x)
    enc.train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        enc(x)
    out = _encoder(trainable=True).to(memory_format=torch.channels_last)(x)
    assert out.requires_grad and (exact_spy.take(), route_spy.take()) == (0, 0)
    # a shape outside the rule: H W C = 160000 lies in the band where MIOpen's geometry was never observed
    z = _cl(torch.randn(2, 64, 50, 50, generator=torch.Generator().manual_seed(2)).to(_dev()))
    bn = _bn(64, _params(64, 4))
    assert encoder.exact_geometry(2, 50, 50, 64) is None and not encoder.exact_output_fusable(z, bn, True)
    with pytest.raises(ValueError, match="covers"):
        encoder.bn_exact(z, bn, True)
    assert exact_spy.take() == 1                                             # (the refused call)
    conv = torch.nn.Conv2d(64, 64, 3, padding=1).to(_dev()).to(memory_format=torch.channels_last).requires_grad_(False)
    seq = torch.nn.Sequential(conv, bn, torch.nn.ReLU(inplace=True), torch.nn.MaxPool2d(2, 2))
    from vqa_amd.modules import run_conv_bn_stack
    run_conv_bn_stack(seq, z), run_conv_bn_stack(seq, z)
    assert (exact_spy.take(), route_spy.take()) == (0, 0) and encoder.exact_report().keys() == report_keys_of(5, 88, 104)


def test_misaligned_parameters_stay_stock(monkeypatch):
    """BatchNorm2d buffers that are views at a 4-byte offset (a flattened buffer, say): the kernels want 16-byte alignment, so
    the layer falls back to the stock chain instead of raising, and nothing is compared or remembered."""
    from vqa_amd import encoder
    from vqa_amd.modules import run_conv_bn_stack
    _default_env(monkeypatch)
    _forget(monkeypatch)
    exact_spy, route_spy = _Spy(monkeypatch, "bn_exact"), _Spy(monkeypatch, "bn_exact_or_stock")
    bn, ref = _bn(64, _params(64, 4)), _bn(64, _params(64, 4))
    flat = torch.zeros(2 * 64 + 1, device=_dev())
    flat[1:65], flat[65:129] = bn.running_mean, bn.running_var
    bn.running_mean, bn.running_var = flat[1:65], flat[65:129]
    assert bn.running_mean.data_ptr() % 16 == 4
    conv = torch.nn.Conv2d(64, 64, 3, padding=1).to(_dev()).to(memory_format=torch.channels_last).requires_grad_(False)
    relu, pool = torch.nn.ReLU(inplace=True), torch.nn.MaxPool2d(2, 2)
    z = _batches((3, 64, 6, 6), 2, n=1)[0]
    assert encoder.exact_output_fusable(z, ref, True) and not encoder.exact_output_fusable(z, bn, True)
    for _ in range(2):
        got = run_conv_bn_stack(torch.nn.Sequential(conv, bn, relu, pool), z)
        monkeypatch.setenv("VQA_ENCODER_EXACT_BN", "0")
        want = run_conv_bn_stack(torch.nn.Sequential(conv, ref, relu, pool), z)
        monkeypatch.delenv("VQA_ENCODER_EXACT_BN")
        assert torch.equal(got, want)
    assert (exact_spy.take(), route_spy.take()) == (0, 0) and encoder.exact_report() == {}
    assert torch.equal(bn.running_mean, ref.running_mean) and torch.equal(bn.running_var, ref.running_var)


def report_keys_of(B, H, W):
    keys = set()
    for ch, pool in ((64, True), (128, True), (256, False), (256, True), (512, False), (512, True), (512, False), (512, True)):
        keys.add((0, B, ch, H, W, pool))
        H, W = (H // 2, W // 2) if pool else (H, W)
    return keys


def test_a_mismatch_warns_once_and_stays_stock(monkeypatch):
    from vqa_amd import encoder
    _default_env(monkeypatch)
    _forget(monkeypatch)
    exact_spy = _Spy(monkeypatch, "bn_exact")
    real = encoder._differs
    monkeypatch.setattr(encoder, "_differs", lambda a, b: real(a, b) | (a.numel() == 128))     # "the [C] tensors differ"
    shape = (3, 128, 6, 6)
    x = _batches(shape, 1, n=1)[0]
    bn, ref = _bn(128, _params(128, 2)), _bn(128, _params(128, 2))
    pool = torch.nn.MaxPool2d(2, 2)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(3):
            got = encoder.bn_exact_or_stock(x, bn, pool)
            assert torch.equal(got, F.relu(F.max_pool2d(ref(x), 2, 2)))
    mine = [w for w in caught if "bn_exact" in str(w.message)]
    assert len(mine) == 1 and "B=3 C=128 H=6 W=6 pool=1" in str(mine[0].message) and "running_mean" in str(mine[0].message)
    assert exact_spy.take() == 0
    assert encoder.exact_report()[(0, 3, 128, 6, 6, True)] == {"verified": False, "first_difference": "running_mean",
                                                              "geometry": encoder.exact_geometry(3, 6, 6, 128)}
    assert torch.equal(bn.running_mean, ref.running_mean) and torch.equal(bn.running_var, ref.running_var)


def test_the_first_call_inside_a_capture_does_not_verify(monkeypatch):
    from vqa_amd import encoder
    _default_env(monkeypatch)
    _forget(monkeypatch)
    exact_spy = _Spy(monkeypatch, "bn_exact")
    shape = (3, 128, 6, 6)
    x = _batches(shape, 1, n=1)[0]
    bn, ref = _bn(128, _params(128, 2)), _bn(128, _params(128, 2))
    want = F.relu(ref(x))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = encoder.bn_exact_or_stock(x, bn, None)
    assert encoder.exact_report() == {} and exact_spy.take() == 0
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, want)
    encoder.bn_exact_or_stock(x, bn, None)                                   # outside: compared and remembered
    assert encoder.exact_report()[(0, 3, 128, 6, 6, False)]["verified"]


# ---- streams, repeats, bounds -----------------------------------------------------------------------------------------------
def test_two_calls_and_a_side_stream_give_the_same_bits():
    """x is written late on a side stream (behind milliseconds of matmuls); the call made under that stream must see it.  Only
    the side stream is synchronised."""
    from vqa_amd import encoder
    shape = next(s for s in reversed(shape_list()) if s[1] == 256)
    B, Ch, H, W = shape
    src = _batches(shape, 7, n=1)[0]
    params = _params(Ch, 8)
    bns = [_bn(Ch, params) for _ in range(3)]
    want = encoder.bn_exact(src, bns[0], True)
    again = encoder.bn_exact(src, bns[1], True)
    assert torch.equal(again, want) and torch.equal(bns[0].running_var, bns[1].running_var)
    x = _cl(torch.zeros_like(src))
    a = torch.randn(4096, 4096, device=_dev()) / 64.0
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = a
        for _ in range(6):
            t = t @ a
        x.copy_(src)
        y = encoder.bn_exact(x, bns[2], True)
    side.synchronize()
    assert torch.equal(y, want)
    assert torch.equal(bns[2].running_mean, bns[0].running_mean) and torch.equal(bns[2].running_var, bns[0].running_var)
    assert int(bns[2].num_batches_tracked) == 1 and torch.isfinite(t).all()


@pytest.mark.parametrize("pool", (True, False))
def test_guard_bands(pool):
    """y, the saved statistics and the workspace are carved out of larger buffers filled with a marker: not a word outside them
    changes and every word of y is written."""
    import ctypes as C
    from vqa_amd import _lib
    lib = _lib.load()
    for shape in _separating_shapes()[:2]:
        B, Ch, H, W = shape
        x = _batches(shape, 3, n=1)[0]
        gamma, beta, rm, rv = _params(Ch, 6)
        Ho, Wo = (H // 2, W // 2) if pool else (H, W)
        ny, nws, pad, marker = B * Ch * Ho * Wo, lib.coattn_bn_exact_workspace_bytes(B, H, W, Ch) // 4, 4096, 12345.5
        ybig = torch.full((pad + ny + pad,), marker, device=_dev())
        wsbig = torch.full((pad + nws + pad,), marker, device=_dev())
        small = torch.full((4, pad + Ch + pad), marker, device=_dev())       # running_mean, running_var, save_mean, save_invstd
        small[0, pad:pad + Ch], small[1, pad:pad + Ch] = rm, rv
        y = ybig[pad:pad + ny]
        y.fill_(float("nan"))
        rc = lib.coattn_bn_exact_forward(_lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(small[0, pad:]),
                                         _lib.ptr(small[1, pad:]), MOMENTUM, EPS, _lib.ptr(y), _lib.ptr(small[2, pad:]),
                                         _lib.ptr(small[3, pad:]), _lib.ptr(wsbig[pad:]), B, H, W, Ch, int(pool), 1, _lib.F32,
                                         C.c_void_p(_lib.stream_ptr(x.device)))
        _lib.check(rc, "coattn_bn_exact_forward")
        torch.cuda.synchronize()
        for big, n in ((ybig, ny), (wsbig, nws)):
            assert (big[:pad] == marker).all() and (big[pad + n:] == marker).all()
        assert (small[:, :pad] == marker).all() and (small[:, pad + Ch:] == marker).all()
        assert not torch.isnan(y).any() and not (small[:, pad:pad + Ch] == marker).any() and not (wsbig[pad:pad + nws] == marker).any()
        z = F.batch_norm(x, rm.clone(), rv.clone(), gamma, beta, True, MOMENTUM, EPS)
        want = F.relu(F.max_pool2d(z, 2, 2)) if pool else F.relu(z)
        assert torch.equal(y.view(B, Ho, Wo, Ch).permute(0, 3, 1, 2), want)


def test_byte_offsets_past_2_31():
    """x = [16, 64, 2, 262200]: 2^29 + 114688 elements, 2.148 GB, so byte offsets pass 2^31 while the shape is still covered
    (32775 pixel groups of 16, sixteen samples per thread).  Everything the stock chain returns, bit for bit."""
    from vqa_amd import encoder
    B, Ch, H, W = 16, 64, 2, 262200
    g = encoder.exact_geometry(B, H, W, Ch)
    assert g is not None and g["pixel_groups"] == 32775 and B * Ch * H * W * 4 > 2 ** 31
    xp = torch.randn(B, H, W, Ch, device=_dev(), generator=torch.Generator(device=_dev()).manual_seed(11))
    x = xp.permute(0, 3, 1, 2)
    assert x.is_contiguous(memory_format=torch.channels_last)
    compare([x], Ch, True, _params(Ch, 12))


# ---- the trainer ------------------------------------------------------------------------------------------------------------
def test_trainer_keeps_the_stock_trajectory(monkeypatch):
    """Five steps of tests/test_gpu_encoder.py::test_runahead_with_a_channels_last_encoder's schedule under the default
    environment, with and without run-ahead, against the same schedule with VQA_ENCODER_EXACT_BN=0: the same bits."""
    from vqa_amd import train as T
    from vqa_amd.modules import HierarchicalCoAttentionNet
    _default_env(monkeypatch)
    _forget(monkeypatch)
    exact_spy = _Spy(monkeypatch, "bn_exact")
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
    for exact in ("0", "1"):
        monkeypatch.setenv("VQA_ENCODER_EXACT_BN", exact)
        for ahead in (False, True):
            net = copy.deepcopy(net0).to(dev)
            net.image_encoder.to(memory_format=torch.channels_last)
            tr = T.Trainer(net, 1e-3, dev, encoder_runahead=ahead)
            losses = []
            for i, bt in enumerate(batches):
                nxt = batches[i + 1][0] if i + 1 < len(batches) else None
                losses.append(tr.step(*bt, next_image=nxt).detach().clone())
            torch.cuda.synchronize()
            runs[exact, ahead] = (torch.stack(losses).cpu(), {k: v.detach().cpu() for k, v in net.state_dict().items()})
        calls = exact_spy.take()
        assert calls == (0 if exact == "0" else 8 * (2 * len(batches) - 1)), calls           # (the first pass of all compares)
    for ahead in (False, True):
        assert torch.equal(runs["1", ahead][0], runs["0", ahead][0]), ahead
        for k, v in runs["0", ahead][1].items():
            assert _same(runs["1", ahead][1][k].float(), v.float()), (ahead, k)

"""The eval-mode encoder passes (include/coattn_ext.h v0.24.0): the raw calls on explicit tensors, the stock-chain oracle, the
operand kinds and the shape lists shared by tests/test_encoder_eval_cpu.py and tests/test_gpu_encoder_eval.py."""
import functools

import torch
import torch.nn.functional as F

EPS = 1e-5
# the launcher of coattn_bn_eval_forward (csrc/encoder.hip: kMaxNormBlocks workgroups of kThreads threads, 4 output vectors of 16
# bytes per thread and trip without the pool, 2 with it)
MAX_BLOCKS, THREADS, PER_THREAD = 4096, 256, {False: 4, True: 2}
CHANNELS = (64, 128, 256, 512)
SHAPES = ((1, 2, 2), (2, 5, 7), (3, 8, 6))


def dev():
    return torch.device("cuda:0")


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def same(a, b):
    """Equal bits up to a NaN's payload: NaNs in the same places, and -0 is not +0."""
    if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    a, b = torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0)
    return torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))


def second_trip_shape(C, pool):
    """The smallest (B, H, W) with B = 1 and W = 16 (32 with the pool) whose output takes the capped grid round its loop a second
    time, with a partial tail: one output pixel row more than a full trip holds."""
    per_trip = MAX_BLOCKS * THREADS * PER_THREAD[pool]               # output vectors of one trip of the whole grid
    wo = 16
    rows = per_trip // (wo * (C // 4)) + 1
    assert per_trip < rows * wo * (C // 4) < 2 * per_trip and (rows * wo * (C // 4)) % (THREADS * PER_THREAD[pool]) != 0
    return (1, 2 * rows, 2 * wo) if pool else (1, rows, wo)


def operands(C, shape, kind, seed, eps=EPS):
    """(x, conv_bias, gamma, beta, running_mean, running_var, eps) on the device, x channels_last."""
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    gamma, beta = 0.5 + torch.rand(C, generator=g), 0.5 * torch.randn(C, generator=g)
    gamma[1::4] = -gamma[1::4]                                       # (a negative gamma: the map goes before the maximum)
    rm, rv = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    bias = torch.randn(C, generator=g)
    if kind == "mixed magnitude":
        x *= 10.0 ** torch.randint(-4, 5, x.shape, generator=g).float()
        rm *= 10.0 ** torch.randint(-3, 4, rm.shape, generator=g).float()
        bias *= 10.0 ** torch.randint(-3, 4, bias.shape, generator=g).float()
    elif kind == "NaN and inf":
        x[0, 1, 0, 0] = float("nan")                                 # one sample's NaN stays in its window
        x[B - 1, 2, H - 1, W - 1] = float("inf")
        x[B // 2, 0, H // 2, 1] = float("-inf")
        x[0, 5] = -0.0
    elif kind == "variances":
        # 0, negative (the fabs), huge, var + eps subnormal (with the eps below) and var + eps cancelling to 0 and to a tiny number
        rv[0:16:8], rv[1:16:8], rv[2:16:8], rv[3:16:8] = 0.0, -0.75, 1e30, 3e-41
        rv[4:16:8], rv[5:16:8], rv[6:16:8] = -eps, -1e-41, 1e-38
        rm[7] = 0.0
        x[:, 7, ::2] = -0.0                                           # (x - 0 keeps the zero's sign: no bias may be added as + 0)
    else:
        assert kind == "normal", kind
    return [cl(x.to(dev()))] + [t.to(dev()) for t in (bias, gamma, beta, rm, rv)] + [eps]


KINDS = (("normal", EPS), ("mixed magnitude", EPS), ("NaN and inf", EPS), ("variances", EPS), ("variances", 1e-40))


def oracle(x, bias, gamma, beta, rm, rv, eps, pool, relu):
    """The stock chain on the same tensors: the exact bias add, F.batch_norm on the running statistics, the pool, the ReLU."""
    z = x if bias is None else x + bias.view(1, -1, 1, 1)
    t = F.batch_norm(cl(z), rm, rv, gamma, beta, False, 0.0, eps)
    assert t.is_contiguous(memory_format=torch.channels_last)
    if pool:
        t = F.max_pool2d(t, 2, 2)
    return torch.relu_(t) if relu else t


def bn_eval_into(y_flat, x, bias, gamma, beta, rm, rv, eps, pool, relu):
    """coattn_bn_eval_forward writing at y_flat (a 1-d fp32 view whose first element is y's)."""
    from vqa_amd import _lib
    B, C, H, W = x.shape
    _lib.bind("coattn_bn_eval_forward", x=x, conv_bias=bias, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, eps=eps,
              y=y_flat, B=B, H=H, W=W, C=C, pool=int(pool), relu=int(relu), dtype=_lib.F32, stream=_lib.stream_ptr(x.device))()


def conv1_eval_into(y_flat, image, weight, bias, gamma, beta, rm, rv, eps, pool):
    from vqa_amd import _lib
    B, _, H, W = image.shape
    _lib.bind("coattn_conv1_bn_eval_forward", image=image, weight=weight, conv_bias=bias, gamma=gamma, beta=beta, running_mean=rm,
              running_var=rv, eps=eps, y=y_flat, B=B, H=H, W=W, Cin=3, Cout=64, pool=int(pool), dtype=_lib.F32,
              stream=_lib.stream_ptr(image.device))()


def out_numel(B, C, H, W, pool):
    return B * C * (H // 2) * (W // 2) if pool else B * C * H * W


def as_nchw(flat, B, C, H, W, pool):
    """The [B,C,Ho,Wo] channels_last view of the kernel's flat [B][Ho][Wo][C] output."""
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    return flat.view(B, Ho, Wo, C).permute(0, 3, 1, 2)


# ---- the first group's shape list, by rule (as tests/test_gpu_encoder_conv1_recompute.py builds its own) -----------------------------
def chunk():
    from vqa_amd import _lib
    return _lib.CONV1_RECOMPUTE_CHUNK


CONV1_PROPERTIES = {
    "B = 1": lambda B, H, W: B == 1,
    "B = the sample chunk": lambda B, H, W: B == chunk(),
    "B crosses the sample chunk by one": lambda B, H, W: B == chunk() + 1,
    "Wo is not a multiple of 8 and above it (a masked window in the last column block)": lambda B, H, W: (W // 2) % 8 != 0 and W // 2 > 8,
    "Wo < 8": lambda B, H, W: W // 2 < 8,
    "odd W": lambda B, H, W: W % 2 == 1 and W >= 3,
    "odd H": lambda B, H, W: H % 2 == 1 and H >= 3,
    "H = W = 2": lambda B, H, W: H == 2 and W == 2,
    "more than one tile row and more than one column block": lambda B, H, W: H // 2 >= 2 and W // 2 > 8,
    "the chunk edge on more than one tile row and column block, with a masked window": lambda B, H, W: (
        B == chunk() + 1 and H // 2 >= 2 and W // 2 > 8 and (W // 2) % 8 != 0),
    "H W is not a multiple of 32 and above it (a masked tail of the unpooled tile)": lambda B, H, W: (H * W) % 32 != 0 and H * W > 32,
}


@functools.lru_cache(maxsize=None)
def conv1_shapes():
    """For each property the (B, H, W) of smallest B H W that has it and that coattn_conv1_bn_exact_forward, the yardstick, covers:
    B in {1, chunk, chunk + 1}, H <= W <= 48, candidates in order of B H W, then B, then H."""
    from vqa_amd import _lib
    lib = _lib.load()
    shapes = []
    for name, has in CONV1_PROPERTIES.items():
        batches = (chunk(),) if name == "B = the sample chunk" else (chunk() + 1,) if "crosses" in name else (1, chunk(), chunk() + 1)
        cands = sorted((B * H * W, B, H, W) for B in batches for H in range(2, 49) for W in range(H, 49))
        for _, B, H, W in cands:
            if has(B, H, W) and lib.coattn_conv1_bn_exact_supported(B, H, W, 3, 64, 1, _lib.F32):
                if (B, H, W) not in shapes:
                    shapes.append((B, H, W))
                break
        else:
            raise AssertionError(name)
    return tuple(shapes)


def conv1_operands(shape, kind, seed):
    """(image, weight) on the device, both channels_last."""
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, 3, H, W, generator=g)
    w = torch.randn(64, 3, 3, 3, generator=g) * 0.2
    if kind == "mixed magnitude":
        img *= 10.0 ** torch.randint(-4, 5, img.shape, generator=g).float()
    elif kind == "NaN and inf":
        img[0, 1, 0, 0] = float("nan")
        img[B - 1, 2, H - 1, W - 1] = float("inf")
        img[B // 2, 0, H // 2, 1] = float("-inf")
    return cl(img.to(dev())), cl(w.to(dev()))

"""The frozen encoder's BatchNorm + ReLU + max-pool call (include/coattn.h v0.14.0, csrc/encoder.hip) without a GPU: the
C-ABI's declarations and exports, the supported-shape rule, argument errors that return before any device work, and
run_conv_bn_stack keeping CPU tensors on the stock modules."""
import ctypes as C
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "coattn.h")
NEW = ("coattn_bn_supported", "coattn_bn_workspace_bytes", "coattn_bn_relu_pool_forward", "coattn_relu_pool_forward")
# (C, H = W) of the eight convolution outputs of VGG11-bn at 224 px; twice the side at 448 px
VGG_LAYERS = ((64, 224), (128, 112), (256, 56), (256, 56), (512, 28), (512, 28), (512, 14), (512, 14))


def test_header_exports_and_version_agree():
    from vqa_amd import _lib
    hdr = open(HDR).read()
    assert re.search(r"^int coattn_bn_supported\(", hdr, re.M)
    assert re.search(r"^size_t coattn_bn_workspace_bytes\(", hdr, re.M)
    assert re.search(r"^int coattn_bn_relu_pool_forward\(", hdr, re.M)
    assert re.search(r"^int coattn_relu_pool_forward\(", hdr, re.M)
    raw = C.CDLL(_lib.LIB_PATH)
    for fn in NEW:
        assert fn in _lib.EXPORTS and hasattr(raw, fn), fn
    assert _lib.load().coattn_version() >= 1400
    # the argument list of the binding is the header's
    decl = re.search(r"^int coattn_bn_relu_pool_forward\(([^;]*)\);", hdr, re.M).group(1)
    kinds = [C.c_double if a.strip().startswith("double") else C.c_int if a.strip().startswith("int") else C.c_void_p
             for a in decl.split(",")]
    assert _lib.load().coattn_bn_relu_pool_forward.argtypes == kinds


def test_supported_shapes():
    from vqa_amd import _lib
    lib = _lib.load()
    for scale in (1, 2):
        for i, (ch, side) in enumerate(VGG_LAYERS):
            pool = int(i in (0, 1, 3, 5, 7))
            assert lib.coattn_bn_supported(160, side * scale, side * scale, ch, pool, _lib.F32) == 1, (ch, side * scale)
            assert lib.coattn_bn_workspace_bytes(160, side * scale, side * scale, ch) > 16 * ch
    assert lib.coattn_bn_supported(4, 8, 8, 6, 0, _lib.F32) == 0
    assert lib.coattn_bn_supported(4, 8, 8, 24, 0, _lib.F32) == 0
    assert lib.coattn_bn_supported(4, 8, 8, 1024, 0, _lib.F32) == 0
    assert lib.coattn_bn_supported(1, 1, 1, 64, 0, _lib.F32) == 0                     # B H W = 1: no variance
    assert lib.coattn_bn_supported(1, 1, 2, 64, 0, _lib.F32) == 1
    assert lib.coattn_bn_supported(1, 2, 2 ** 22 + 2, 64, 1, _lib.F32) == 1          # 2^29 + 256 elements
    assert lib.coattn_bn_supported(1, 4, 2 ** 22, 128, 0, _lib.F32) == 0             # B H W C = 2^31
    assert lib.coattn_bn_supported(2 ** 20, 2 ** 20, 2 ** 20, 16, 0, _lib.F32) == 0  # (and no 64-bit wrap-around)
    assert lib.coattn_bn_supported(4, 1, 8, 64, 1, _lib.F32) == 0                     # a pool needs two rows
    assert lib.coattn_bn_supported(4, 8, 1, 64, 1, _lib.F32) == 0
    assert lib.coattn_bn_supported(4, 1, 8, 64, 0, _lib.F32) == 1
    assert lib.coattn_bn_supported(4, 8, 8, 64, 0, _lib.BF16) == 0
    assert lib.coattn_bn_workspace_bytes(4, 8, 8, 24) == 0 and b"supported" in lib.coattn_last_error()


def test_workspace_partials_stay_small():
    """The per-workgroup partials (16 bytes per channel, written and read back) stay at or below 2 % of the layer."""
    from vqa_amd import _lib
    lib = _lib.load()
    for ch, side in VGG_LAYERS:
        layer = 160 * side * side * ch * 4
        partials = lib.coattn_bn_workspace_bytes(160, side, side, ch) - 16 * ch
        assert 0 < 2 * partials <= 0.02 * layer, (ch, side, partials, layer)


def test_argument_errors_return_before_any_device_work():
    """Each is negative with a message; nothing is launched (there is no GPU here, and the pointers are made up)."""
    from vqa_amd import _lib
    lib = _lib.load()

    def call(x=4096, B=2, H=4, W=4, ch=64, pool=1, dtype=_lib.F32, momentum=0.1, eps=1e-5, ws=1 << 20, y=1 << 16):
        p = [C.c_void_p(v) if v else None for v in (x, 256, 512, 0, 768, 1024)]
        return lib.coattn_bn_relu_pool_forward(*p, momentum, eps, C.c_void_p(y) if y else None, None,
                                               C.c_void_p(ws) if ws else None, B, H, W, ch, pool, 1, dtype, None)

    def failed(rc, word):
        return rc < 0 and word in lib.coattn_last_error()

    assert failed(call(B=0), b"B=0")
    assert failed(call(x=0), b"null")
    assert failed(call(y=0), b"null") and failed(call(ws=0), b"null")
    assert failed(call(ch=24), b"supported") and failed(call(H=1), b"supported") and failed(call(dtype=_lib.BF16), b"supported")
    assert failed(call(x=4100), b"aligned") and failed(call(ws=(1 << 20) + 8), b"aligned")
    assert failed(call(x=1 << 16), b"must not be x")
    assert failed(call(momentum=1.5), b"momentum") and failed(call(momentum=float("nan")), b"momentum")
    assert failed(call(eps=0.0), b"eps")

    def pool_call(x=4096, y=1 << 16, B=2, H=4, W=4, ch=64, dtype=_lib.F32):
        return lib.coattn_relu_pool_forward(C.c_void_p(x) if x else None, C.c_void_p(y) if y else None, B, H, W, ch, dtype, None)

    assert failed(pool_call(B=0), b"B=0") and failed(pool_call(x=0), b"null") and failed(pool_call(y=0), b"null")
    assert failed(pool_call(H=1), b"supported") and failed(pool_call(ch=24), b"supported")
    assert failed(pool_call(dtype=_lib.BF16), b"supported")
    assert failed(pool_call(y=(1 << 16) + 4), b"aligned") and failed(pool_call(y=4096), b"must not be x")


def test_cpu_tensors_never_reach_the_fused_route(monkeypatch):
    from vqa_amd import encoder
    from vqa_amd.modules import ImageCoAttentionEncoder, run_conv_bn_stack
    calls = []
    for name in ("bn_relu_pool", "relu_pool"):
        monkeypatch.setattr(encoder, name, lambda *a, **k: calls.append(a) or (_ for _ in ()).throw(AssertionError("fused")))
    torch.manual_seed(0)
    enc = ImageCoAttentionEncoder(is_trainable=False, weights_path=None)
    x = torch.randn(2, 3, 32, 32)
    for fmt in (torch.contiguous_format, torch.channels_last):
        with torch.no_grad():
            y = run_conv_bn_stack(enc.vgg11_encoder, x.contiguous(memory_format=fmt))
        assert y.shape == (2, 512, 1, 1)
    assert enc(x).shape == (2, 1, 512)
    monkeypatch.setenv("VQA_ENCODER_FUSED", "1")
    assert enc(x).shape == (2, 1, 512)
    assert calls == []


def test_mode_switch(monkeypatch):
    from vqa_amd import encoder
    monkeypatch.delenv("VQA_ENCODER_FUSED", raising=False)
    assert encoder.mode() == "pool"
    for value, want in (("0", "stock"), ("1", "bn"), ("", "pool")):
        monkeypatch.setenv("VQA_ENCODER_FUSED", value)
        assert encoder.mode() == want


def test_pool_recognition():
    from vqa_amd import encoder
    nn = torch.nn
    assert encoder.pool_is_2x2(nn.MaxPool2d(2, 2)) and encoder.pool_is_2x2(nn.MaxPool2d(2)) and encoder.pool_is_2x2(nn.MaxPool2d((2, 2), (2, 2)))
    for bad in (nn.MaxPool2d(3, 2), nn.MaxPool2d(2, 1), nn.MaxPool2d(2, 2, padding=1), nn.MaxPool2d(2, 2, ceil_mode=True),
                nn.MaxPool2d(2, 2, dilation=2), nn.MaxPool2d(2, 2, return_indices=True), nn.MaxPool2d((2, 1), (2, 1))):
        assert not encoder.pool_is_2x2(bad), bad

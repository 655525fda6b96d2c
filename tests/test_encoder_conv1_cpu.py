"""The frozen encoder's first convolution with its BatchNorm statistics riding along (include/coattn.h v0.16.0, csrc/encoder.hip)
without a GPU: the C-ABI's answers and argument checks, and the route, which a CPU tensor never takes."""
import ctypes as C

import pytest
import torch

NEW = ("coattn_conv1_bn_exact_supported", "coattn_conv1_bn_exact_workspace_bytes", "coattn_conv1_bn_exact_forward",
       "coattn_conv1_probe")


def test_exports_and_version():
    from vqa_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for fn in NEW:
        assert fn in _lib.EXPORTS and hasattr(raw, fn), fn
    lib = _lib.load()
    assert lib.coattn_version() >= 1600
    assert lib.coattn_conv1_bn_exact_workspace_bytes.restype is C.c_size_t


def test_supported_answers_0_for_each_unsupported_argument():
    from vqa_amd import _lib
    lib = _lib.load()
    ok = lib.coattn_conv1_bn_exact_supported
    assert ok(160, 224, 224, 3, 64, 1, _lib.F32) == 1 and ok(2, 6, 7, 3, 64, 0, _lib.F32) == 1
    assert ok(160, 224, 224, 4, 64, 1, _lib.F32) == 0                        # Cin
    assert ok(160, 224, 224, 3, 128, 1, _lib.F32) == 0 and ok(160, 224, 224, 3, 32, 1, _lib.F32) == 0      # Cout
    assert ok(160, 224, 224, 3, 64, 1, _lib.BF16) == 0                       # dtype
    assert ok(0, 224, 224, 3, 64, 1, _lib.F32) == 0 and ok(1025, 8, 8, 3, 64, 0, _lib.F32) == 0            # B
    assert ok(2, 50, 50, 3, 64, 0, _lib.F32) == 0                            # H W 64 = 160000: the geometry's unobserved band
    assert ok(2, 3, 3, 3, 64, 0, _lib.F32) == 0                              # H W = 1 modulo 8
    assert ok(2, 1, 16, 3, 64, 0, _lib.F32) == 1 and ok(2, 1, 16, 3, 64, 1, _lib.F32) == 0                 # a pool needs H >= 2
    assert ok(1, 4, 2 ** 23, 3, 64, 0, _lib.F32) == 0                        # B H W 64 = 2^31
    # where the BatchNorm geometry answers, and only there
    for B, H, W in ((1, 2, 2), (3, 7, 9), (2, 48, 50), (2, 50, 52), (5, 88, 104), (2, 5, 5)):
        assert ok(B, H, W, 3, 64, 0, _lib.F32) == (1 if lib.coattn_bn_exact_geometry(B, H, W, 64, _lib.F32, None) else 0), (B, H, W)


def test_workspace_bytes():
    from vqa_amd import _lib, encoder
    lib = _lib.load()
    g = encoder.exact_geometry(160, 224, 224, 64)
    partial = g["pixel_groups"] * 64 * 8
    assert lib.coattn_conv1_bn_exact_workspace_bytes(160, 224, 224, 0) == (partial + 255) // 256 * 256
    assert (lib.coattn_conv1_bn_exact_workspace_bytes(160, 224, 224, 1)
            == (partial + 255) // 256 * 256 + 160 * 224 * 224 * 64 * 4)
    assert lib.coattn_conv1_bn_exact_workspace_bytes(2, 50, 50, 1) == 0 and b"covered" in lib.coattn_last_error()


def test_argument_errors_come_before_any_gpu_call():
    """Host pointers that are never dereferenced: every refusal is -1 with a message, before a HIP call."""
    from vqa_amd import _lib
    lib = _lib.load()
    p = C.c_void_p

    def call(image=4096, weight=8192, gamma=512, beta=768, rm=1024, rv=1280, momentum=0.1, eps=1e-5, x=1 << 20, y=1 << 21,
             mean=1536, invstd=1792, ws=1 << 22, B=2, H=6, W=7, Cin=3, Cout=64, pool=1, dtype=_lib.F32):
        return lib.coattn_conv1_bn_exact_forward(p(image), p(weight), p(gamma), p(beta), p(rm), p(rv), momentum, eps, p(x), p(y),
                                                 p(mean), p(invstd), p(ws), B, H, W, Cin, Cout, pool, dtype, p(0))

    for kw, word in ((dict(Cin=4), b"covered"), (dict(Cout=128), b"covered"), (dict(dtype=_lib.BF16), b"covered"),
                     (dict(H=50, W=50), b"covered"), (dict(B=0), b">= 1"), (dict(H=1, W=16), b"covered"),
                     (dict(image=0), b"null"), (dict(weight=0), b"null"), (dict(y=0), b"null"), (dict(ws=0), b"null"),
                     (dict(gamma=0), b"null"), (dict(mean=0), b"null"),
                     (dict(y=(1 << 21) + 4), b"aligned"), (dict(x=(1 << 20) + 8), b"aligned"), (dict(rm=1028), b"aligned"),
                     (dict(image=4098), b"aligned"), (dict(weight=8193), b"aligned"), (dict(ws=(1 << 22) + 4), b"aligned"),
                     (dict(x=1 << 21), b"three buffers"), (dict(y=4096), b"three buffers"),
                     (dict(momentum=1.5), b"momentum"), (dict(eps=0.0), b"eps")):
        assert call(**kw) == -1, kw
        assert word in lib.coattn_last_error(), (kw, lib.coattn_last_error())
    assert lib.coattn_conv1_probe(p(4096), p(8192), p(1 << 20), p(1 << 22), 2, 6, 7, 14, 0, 1, 0, p(0)) == -1
    assert lib.coattn_conv1_probe(p(4096), p(8192), p(1 << 20), p(1 << 22), 2, 50, 50, 0, 0, 1, 0, p(0)) == -1
    assert lib.coattn_conv1_probe(p(4096), p(8192), p(0), p(1 << 22), 2, 6, 7, 0, 0, 1, 0, p(0)) == -1


def _first_group(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 64, 3, padding=1), torch.nn.BatchNorm2d(64), torch.nn.ReLU(inplace=True),
                               torch.nn.MaxPool2d(2, 2)).requires_grad_(False)


def test_on_cpu_the_route_is_never_taken(monkeypatch):
    import copy
    from vqa_amd import encoder
    from vqa_amd.modules import run_conv_bn_stack
    calls = []
    monkeypatch.setattr(encoder, "conv1_bn_exact_or_stock", lambda *a, **k: calls.append(a) or (_ for _ in ()).throw(AssertionError))
    seq = _first_group()
    ref = copy.deepcopy(seq)
    x = torch.randn(2, 3, 6, 8).contiguous(memory_format=torch.channels_last)
    seq.to(memory_format=torch.channels_last)
    assert not encoder.conv1_modules_fusable(seq[0], seq[1], seq[3], x)
    assert not encoder.conv1_inputs_fusable(x, seq[0], seq[1], True)
    got, want = run_conv_bn_stack(seq, x), ref(x)
    assert calls == [] and torch.allclose(got, want, rtol=1e-5, atol=1e-6)     # (the bias fold: equal to rounding, as today)
    for k, v in seq.state_dict().items():
        assert torch.allclose(v.float(), ref.state_dict()[k].float(), rtol=1e-5, atol=1e-6), k
    assert encoder.exact_report() == {} or all("verified" in v for v in encoder.exact_report().values())


def test_bn_exact_with_conv_refuses_a_cpu_tensor():
    from vqa_amd import encoder
    seq = _first_group().to(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match="with conv"):
        encoder.bn_exact(torch.randn(2, 3, 6, 8).contiguous(memory_format=torch.channels_last), seq[1], True, conv=seq[0])


def test_the_switches(monkeypatch):
    from vqa_amd import encoder
    for name in ("VQA_ENCODER_FUSED", "VQA_ENCODER_EXACT_BN", "VQA_ENCODER_EXACT_CONV1"):
        monkeypatch.delenv(name, raising=False)
    assert encoder.conv1_enabled()
    for name, value in (("VQA_ENCODER_EXACT_CONV1", "0"), ("VQA_ENCODER_EXACT_BN", "0"), ("VQA_ENCODER_FUSED", "0"),
                        ("VQA_ENCODER_FUSED", "1")):
        monkeypatch.setenv(name, value)
        assert not encoder.conv1_enabled(), name
        monkeypatch.delenv(name)
    assert encoder.conv1_enabled()

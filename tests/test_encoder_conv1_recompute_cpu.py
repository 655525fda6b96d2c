"""The frozen encoder's first group with its convolution computed twice and never stored (include/coattn.h v0.22.0,
csrc/encoder.hip) without a GPU: the exports, the tabled signature against the header, the C-ABI's answers and argument checks,
the switch, and the map from the MFMA's row slots to the pooling windows of a tile, restated in Python."""
import ctypes as C
import re

import torch

from tests._header import args as header_args, header

NEW = ("coattn_conv1_bn_recompute_workspace_bytes", "coattn_conv1_bn_recompute_forward")
FORWARD = "coattn_conv1_bn_recompute_forward"


def test_exports_and_version():
    from vqa_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for fn in NEW:
        assert fn in _lib.EXPORTS and hasattr(raw, fn), fn
    lib = _lib.load()
    assert lib.coattn_version() >= 2200
    assert lib.coattn_conv1_bn_recompute_workspace_bytes.restype is C.c_size_t


def test_the_tabled_signature_and_the_chunk_match_the_header():
    from vqa_amd import _lib
    hdr = header()
    sig = _lib.SIGNATURES[FORWARD]                                               # (held against the header: tests/test_call_layer_cpu.py)
    assert sig[-1][0] == "stream"
    # the stored entry's arguments without x_out, in its order
    stored = [a.rsplit(" ", 1)[1] for a in header_args(hdr, "coattn_conv1_bn_exact_forward")]
    assert [n for n in stored if n != "x_out"] == [n for n, _ in sig]
    ws = re.search(r"^size_t coattn_conv1_bn_recompute_workspace_bytes\(([^;]*)\);", hdr, re.M).group(1)
    assert [a.split()[-1] for a in ws.split(",")] == ["B", "H", "W"]
    assert len(_lib.load().coattn_conv1_bn_recompute_workspace_bytes.argtypes) == 3
    assert int(re.search(r"^#define COATTN_CONV1_RECOMPUTE_CHUNK (\d+)", hdr, re.M).group(1)) == _lib.CONV1_RECOMPUTE_CHUNK >= 1


def test_workspace_bytes_are_the_partials_alone():
    from vqa_amd import _lib, encoder
    lib = _lib.load()
    size = lib.coattn_conv1_bn_recompute_workspace_bytes
    g = encoder.exact_geometry(160, 224, 224, 64)
    assert size(160, 224, 224) == (g["pixel_groups"] * 64 * 8 + 255) // 256 * 256 < 2 ** 22
    for B, H, W in ((1, 2, 2), (3, 7, 9), (2, 48, 50), (9, 2, 2)):
        assert size(B, H, W) == lib.coattn_conv1_bn_exact_workspace_bytes(B, H, W, 0) > 0, (B, H, W)
    assert size(2, 50, 50) == 0 and b"covered" in lib.coattn_last_error()


def test_argument_errors_come_before_any_gpu_call():
    """Host pointers that are never dereferenced: every refusal is -1 with a message, before a HIP call."""
    from vqa_amd import _lib
    lib = _lib.load()
    base = dict(image=4096, weight=8192, gamma=512, beta=768, running_mean=1024, running_var=1280, momentum=0.1, eps=1e-5, y=1 << 21,
                save_mean=1536, save_invstd=1792, ws=1 << 22, B=2, H=6, W=7, Cin=3, Cout=64, pool=1, dtype=_lib.F32, stream=0)
    for kw, word in ((dict(Cin=4), b"covered"), (dict(Cout=128), b"covered"), (dict(dtype=_lib.BF16), b"covered"),
                     (dict(H=50, W=50), b"covered"), (dict(B=0), b">= 1"), (dict(H=1, W=16), b"covered"), (dict(B=1025), b"covered"),
                     (dict(image=0), b"null"), (dict(weight=0), b"null"), (dict(y=0), b"null"), (dict(ws=0), b"null"),
                     (dict(gamma=0), b"null"), (dict(beta=0), b"null"), (dict(save_mean=0), b"null"), (dict(save_invstd=0), b"null"),
                     (dict(running_mean=0), b"null"), (dict(running_var=0), b"null"),
                     (dict(y=(1 << 21) + 4), b"aligned"), (dict(running_mean=1028), b"aligned"), (dict(save_invstd=1800), b"aligned"),
                     (dict(image=4098), b"aligned"), (dict(weight=8193), b"aligned"), (dict(ws=(1 << 22) + 4), b"aligned"),
                     (dict(y=4096), b"two buffers"),
                     (dict(momentum=1.5), b"momentum"), (dict(momentum=-0.1), b"momentum"), (dict(eps=0.0), b"eps")):
        call = _lib.bind(FORWARD, **{**base, **kw})
        assert call.fn(*call) == -1, kw
        assert word in lib.coattn_last_error() and b"conv1_bn_recompute_forward" in lib.coattn_last_error(), (kw, lib.coattn_last_error())


def test_the_switch(monkeypatch):
    from vqa_amd import encoder
    monkeypatch.delenv("VQA_ENCODER_CONV1_RECOMPUTE", raising=False)
    assert encoder.conv1_recompute_enabled()
    monkeypatch.setenv("VQA_ENCODER_CONV1_RECOMPUTE", "0")
    assert not encoder.conv1_recompute_enabled() and encoder.conv1_enabled()     # (the stored form, not the stock kernels)
    monkeypatch.setenv("VQA_ENCODER_CONV1_RECOMPUTE", "1")
    assert encoder.conv1_recompute_enabled()


def test_on_cpu_nothing_reaches_the_binding(monkeypatch):
    from vqa_amd import encoder
    from vqa_amd.modules import run_conv_bn_stack
    monkeypatch.setattr(encoder, "_conv1_recompute_raw", lambda *a, **k: (_ for _ in ()).throw(AssertionError))
    torch.manual_seed(0)
    seq = torch.nn.Sequential(torch.nn.Conv2d(3, 64, 3, padding=1), torch.nn.BatchNorm2d(64), torch.nn.ReLU(inplace=True),
                              torch.nn.MaxPool2d(2, 2)).requires_grad_(False).to(memory_format=torch.channels_last)
    y = run_conv_bn_stack(seq, torch.randn(2, 3, 6, 8).contiguous(memory_format=torch.channels_last))
    assert y.shape == (2, 64, 3, 4)


# ---- the pooled tile: conv1_norm_pool_kernel<D, true>'s map, restated -----------------------------------------------------------------
def _slot_pixel(q):
    """(tile row, tile column) of the pixel whose terms the lane with p = q loads: window q >> 2, member q & 3."""
    return (q >> 1) & 1, 2 * (q >> 2) + (q & 1)


def _register_slot(v, g):
    """The MFMA row of accumulator register v in lane half g (v_mfma_f32_32x32x2_f32's D layout): 8 (v >> 2) + 4 g + (v & 3)."""
    return 8 * (v >> 2) + 4 * g + (v & 3)


def test_the_32_slots_are_the_32_pixels_of_the_tile():
    pixels = [_slot_pixel(q) for q in range(32)]
    assert sorted(pixels) == [(r, c) for r in range(2) for c in range(16)]


def test_a_lanes_four_registers_are_one_window_in_the_pool_kernels_member_order():
    """bn_relu_pool_kernel reads a window as v[0] = (0, 0), v[1] = (0, 1) (one pixel on), v[2] = (1, 0) (one row on), v[3] = (1, 1) and
    takes max(max(v0, v1), max(v2, v3)); conv1_norm_pool_kernel hands window_max1 the registers 4 b .. 4 b + 3 in that order."""
    order = [(0, 0), (0, 1), (1, 0), (1, 1)]
    windows = set()
    for g in range(2):
        for b in range(4):
            window = 2 * b + g                                               # the pooled column the kernel stores register group b to
            members = [_slot_pixel(_register_slot(4 * b + r, g)) for r in range(4)]
            assert members == [(dy, 2 * window + dx) for dy, dx in order], (g, b, members)
            windows.add(window)
    assert windows == set(range(8))
    # the two lane halves of a store are adjacent pooled pixels: two whole 128-byte lines
    assert all((2 * b + 1) - (2 * b + 0) == 1 for b in range(4))


def test_the_grid_covers_every_pooled_pixel_once():
    """Tile t = (ho, cb) with cbs = ceil(Wo / 8); window wo = 8 cb + 2 b + g is stored iff wo < Wo; floor mode never reads past
    2 Ho x 2 Wo."""
    for H, W in ((2, 2), (5, 7), (6, 18), (7, 35), (224, 224)):
        Ho, Wo = H // 2, W // 2
        cbs = (Wo + 7) // 8
        stored = {}
        for t in range(Ho * cbs):
            ho, cb = divmod(t, cbs)
            for g in range(2):
                for b in range(4):
                    wo = 8 * cb + 2 * b + g
                    if wo < Wo:
                        stored[(ho, wo)] = stored.get((ho, wo), 0) + 1
                        for r in range(4):
                            dy, col = _slot_pixel(_register_slot(4 * b + r, g))
                            assert 2 * ho + dy < 2 * Ho <= H and 16 * cb + col < 2 * Wo <= W
        assert stored == {(ho, wo): 1 for ho in range(Ho) for wo in range(Wo)}, (H, W)

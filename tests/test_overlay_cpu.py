"""Attention overlays (include/coattn.h v0.21.0, vqa_amd.overlay, predict.py --attention_overlays) as far as they go without a
GPU: the declaration, the exports, the supported table, every argument error of the entry point, the tests' own oracle pinned
against torch's bilinear interpolation in float64, the PNG writer, the sheet and the command-line refusals."""
import ctypes as C
import re
import struct
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vqa_amd
from vqa_amd import _lib, overlay as OV, predict as P, train as T

from tests import _overlay as O
from tests._header import args as header_args, header


def _err():
    return _lib.load().coattn_last_error().decode()


# ---- header and exports ---------------------------------------------------------------------------------------------------------
def test_header_declares_exports_constants_and_version():
    hdr = header()
    for fn in ("coattn_overlay_supported", "coattn_overlay_render"):
        assert re.search(r"^int %s\(" % fn, hdr, re.M), fn
        assert fn in _lib.EXPORTS and hasattr(C.CDLL(_lib.LIB_PATH), fn), fn
    assert _lib.load().coattn_version() >= 2100
    for name, value in (("COATTN_OVERLAY_HEAT", _lib.OVERLAY_HEAT), ("COATTN_OVERLAY_MASK", _lib.OVERLAY_MASK)):
        assert int(re.search(r"^#define %s (\d+)" % name, hdr, re.M).group(1)) == value
    assert _lib.OVERLAY_HEAT != _lib.OVERLAY_MASK and OV.MODES == {"heat": _lib.OVERLAY_HEAT, "mask": _lib.OVERLAY_MASK}
    rows, threads = O.constants()
    assert rows >= 1 and threads >= 64 and threads % 64 == 0
    assert vqa_amd.overlay is OV and vqa_amd.render_attention is OV.render_attention
    assert {"overlay", "render_attention"} <= set(vqa_amd.__all__)
    # the arithmetic is written into the header
    for phrase in ("r = 1.0f / mx", "src = ((float)y + 0.5f) * sy - 0.5f", "g = floor + (1-floor)*u", "k = (int)(u*255 + 0.5f)",
                   "cell t = (x*T) / W"):
        assert phrase in hdr, phrase


def test_the_struct_and_the_tabled_signature_match_the_header():
    hdr = header()
    body = re.search(r"typedef struct coattn_overlay_params \{(.*?)\} coattn_overlay_params;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(const void\*|float)\s+(\w+)(\[3\])?;", body, re.M)
    assert [(n, t, bool(a)) for t, n, a in fields] == [("mean", "float", True), ("std", "float", True), ("alpha", "float", False),
                                                       ("floor", "float", False), ("lut", "const void*", False)]
    assert [(n, t) for n, t in _lib.OverlayParams._fields_] == [("mean", C.c_float * 3), ("std", C.c_float * 3), ("alpha", C.c_float),
                                                               ("floor", C.c_float), ("lut", C.c_void_p)]
    fn = "coattn_overlay_render"
    assert _lib.SIGNATURES[fn][-1][0] == "stream"                                # (names and types: tests/test_call_layer_cpu.py)
    names = [a.split()[-1] for a in header_args(hdr, "coattn_overlay_supported")]
    assert names == "B L H W Gh Gw T strip_h mode".split()
    assert len(_lib.load().coattn_overlay_supported.argtypes) == 9


def test_supported_table_at_its_edges():
    base = dict(B=2, L=3, H=224, W=224, Gh=7, Gw=7, T=26, strip_h=32, mode=_lib.OVERLAY_HEAT)

    def sup(**kw):
        a = {**base, **kw}
        return _lib.load().coattn_overlay_supported(*[a[k] for k in "B L H W Gh Gw T strip_h mode".split()])

    assert sup() == 1 and sup(mode=_lib.OVERLAY_MASK) == 1 and sup(B=160, H=448, W=448, Gh=14, Gw=14) == 1
    for kw, ok in ((dict(B=0), 0), (dict(B=-1), 0), (dict(B=1), 1), (dict(B=65536), 1),
                   (dict(L=0), 0), (dict(L=1), 1), (dict(L=8), 1), (dict(L=9), 0),
                   (dict(H=0), 0), (dict(H=1), 1), (dict(H=4096), 1), (dict(H=4097), 0), (dict(H=3, Gh=14), 1),
                   (dict(W=0), 0), (dict(W=4, T=4), 1), (dict(W=4096), 1), (dict(W=4100), 0), (dict(W=222), 0), (dict(W=226), 0),
                   (dict(W=225), 0), (dict(W=228), 1),
                   (dict(Gh=0), 0), (dict(Gh=1), 1), (dict(Gh=64), 1), (dict(Gh=65), 0),
                   (dict(Gw=0), 0), (dict(Gw=1), 1), (dict(Gw=64), 1), (dict(Gw=65), 0),
                   (dict(T=0), 0), (dict(T=1), 1), (dict(T=224), 1), (dict(T=225), 0), (dict(W=4096, T=4096), 1),
                   (dict(strip_h=0, T=0), 1), (dict(strip_h=0, T=100000), 1), (dict(strip_h=-1), 0), (dict(strip_h=1), 1),
                   (dict(strip_h=4096), 1), (dict(strip_h=4097), 0),
                   (dict(mode=2), 0), (dict(mode=-1), 0)):
        assert sup(**kw) == ok, kw
    rows = O.constants()[0]
    bands = (1 + rows - 1) // rows                                               # B times the bands of a sample stays below 2^31
    assert sup(B=2 ** 31 - 1, H=1, strip_h=0) == (1 if bands == 1 else 0) and sup(B=2 ** 31 - 1, H=4096, strip_h=0) == 0
    assert OV.supported(2, 3, 224, 224, 7, 7, 26, 32) and OV.supported(2, 3, 224, 224, 7, 7, mode="mask")
    assert not OV.supported(2, 3, 224, 222, 7, 7) and not OV.supported(2, 3, 224, 224, 7, 7, mode="jet")


def test_every_argument_error_is_minus_one_with_a_message_before_any_device_work():
    """Made-up pointers: a call that went on to touch them would fault; each error names what is wrong."""
    fake = lambda i: 0x10000 * (i + 1)                          # noqa: E731  (16-byte aligned, never dereferenced)
    par = dict(mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25), alpha=0.6, floor=0.3, lut=fake(7))
    base = dict(image=fake(0), sB=3 * 8 * 8, sC=64, sH=8, sW=1, a_v=fake(1), a_q=fake(2), q_len=fake(3), out=fake(4),
                bad_maps=fake(5), B=2, L=3, H=8, W=8, Gh=2, Gw=2, T=5, strip_h=2, mode=_lib.OVERLAY_HEAT, stream=None)

    def call(p=None, **kw):
        pp = {**par, **(p or {})}
        st = _lib.OverlayParams((C.c_float * 3)(*pp["mean"]), (C.c_float * 3)(*pp["std"]), pp["alpha"], pp["floor"], pp["lut"])
        c = _lib.bind("coattn_overlay_render", **{**base, "p": st, **kw})
        return c.fn(*c)

    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(mode=2), "mode"), (dict(mode=-1), "mode"),
                     (dict(B=0), "non-positive"), (dict(L=0), "non-positive"), (dict(H=0), "non-positive"), (dict(W=-4), "non-positive"),
                     (dict(Gh=0), "non-positive"), (dict(Gw=-1), "non-positive"),
                     (dict(strip_h=-1), "negative strip_h"), (dict(a_q=None), "needs a_q"),
                     (dict(L=9), "not supported"), (dict(H=4097), "not supported"), (dict(W=4100), "not supported"),
                     (dict(W=6), "not supported"), (dict(Gh=65), "not supported"), (dict(Gw=65), "not supported"),
                     (dict(T=0), "not supported"), (dict(T=9), "not supported"), (dict(strip_h=4097), "not supported"),
                     (dict(image=None), "null"), (dict(a_v=None), "null"), (dict(out=None), "null"), (dict(p=None), "null"),
                     (dict(p=dict(alpha=-0.1)), "alpha"), (dict(p=dict(alpha=1.5)), "alpha"), (dict(p=dict(alpha=nan)), "alpha"),
                     (dict(p=dict(floor=-1e-3)), "floor"), (dict(p=dict(floor=1.001)), "floor"), (dict(p=dict(floor=nan)), "floor"),
                     (dict(p=dict(std=(0.2, 0.0, 0.2))), "std[1]"), (dict(p=dict(std=(inf, 0.2, 0.2))), "std[0]"),
                     (dict(p=dict(std=(0.2, 0.2, nan))), "std[2]"), (dict(p=dict(mean=(0.5, nan, 0.5))), "mean[1]"),
                     (dict(p=dict(lut=None)), "lut"),
                     (dict(out=fake(4) + 4), "aligned"), (dict(out=fake(4) + 8), "aligned"), (dict(image=fake(0) + 4), "aligned"),
                     (dict(image=fake(0) + 8), "aligned"), (dict(image=fake(0) + 2, sW=3, sC=1, sH=24), "aligned"),
                     (dict(a_v=fake(1) + 2), "aligned"), (dict(a_q=fake(2) + 1), "aligned"), (dict(q_len=fake(3) + 2), "aligned"),
                     (dict(bad_maps=fake(5) + 2), "aligned"), (dict(p=dict(lut=fake(7) + 2)), "aligned")):
        if "p" in kw and kw["p"] is None:
            c = _lib.bind("coattn_overlay_render", **{**base, "p": None})
            rc = c.fn(*c)
        else:
            rc = call(**kw)
        assert rc == -1 and word in _err(), (kw, _err())
    # what is allowed, checked on calls that are refused further on, so that the made-up pointers are never reached: no counter,
    # no lengths, no lut in the mask mode, T and a_q ignored without a strip, a strided image at a 4-byte address
    assert call(bad_maps=None, q_len=None, out=None) == -1 and "null" in _err()
    assert call(p=dict(lut=None), mode=_lib.OVERLAY_MASK, out=None) == -1 and "null" in _err()
    assert call(strip_h=0, a_q=None, T=0, out=None) == -1 and "null" in _err()
    assert call(image=fake(0) + 4, sW=3, sC=1, sH=24, out=fake(4) + 4) == -1 and "out" in _err() and "aligned" in _err()
    assert call(image=fake(0) + 4, sH=9, sC=72, sB=216, out=None) == -1 and "null" in _err()      # sW = 1, odd rows: element loads


def test_render_attention_refuses_cpu_tensors_and_wrong_arguments():
    im, av, aq = torch.zeros(2, 3, 8, 8), torch.zeros(3, 2, 4), torch.zeros(3, 2, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OV.render_attention(im, av, aq)
    with pytest.raises(RuntimeError, match="GPU"):
        OV.default_lut("cpu")
    for args, kw, exc, word in (((im, torch.zeros(3, 2, 5)), {}, ValueError, "square"),
                                ((im, av), dict(grid=(2, 3)), ValueError, "grid 2x3"),
                                ((im, av), dict(strip=4), ValueError, "needs a_q"),
                                ((im, av, aq), dict(strip=-1), ValueError, "strip"),
                                ((im, av, aq), dict(mode="jet"), ValueError, "mode"),
                                ((im.double(), av), {}, RuntimeError, "image"), ((im[:, :2], av), {}, RuntimeError, "image"),
                                ((im, av[:, :1]), {}, RuntimeError, "image attention"), ((im, av.half()), {}, RuntimeError, "image attention"),
                                ((im, av, aq[:2]), {}, RuntimeError, "question attention"),
                                ((im, av, aq, torch.zeros(2)), {}, RuntimeError, "ques_len"),
                                ((im, av, aq, torch.zeros(3, dtype=torch.int64)), {}, RuntimeError, "ques_len")):
        with pytest.raises(exc, match=word):
            OV.render_attention(*args, **kw)
    assert OV.bad_maps() == 0                                    # (no device, no counter)


# ---- the oracle itself ----------------------------------------------------------------------------------------------------------
UPSAMPLE = ((7, 7, 224, 224), (14, 14, 448, 448), (7, 7, 225, 223), (3, 5, 17, 31), (1, 1, 4, 4), (2, 3, 2, 3), (14, 14, 13, 9),
            (16, 16, 448, 448))                                                  # (Gh, Gw, H, W)


@pytest.mark.parametrize("shape", UPSAMPLE, ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_the_oracles_upsampling_is_torchs_bilinear_in_float64(shape):
    """Bound 8 max(Gh, Gw) 2^-24 max|m|: the source coordinate carries three roundings of a value below G, so each weight errs
    by a few G 2^-24; two axes and six product roundings stay under it.  The bytes of the mask mode differ from the float64
    pipeline's by one code value at the most (only a rounding edge can flip)."""
    Gh, Gw, H, W = shape
    g = torch.Generator().manual_seed(8200 + Gh * Gw + H)
    a = torch.softmax(torch.randn(Gh * Gw, generator=g) * 3, 0).numpy()
    m, bad = O.normalise(a)
    assert not bad and m.dtype == np.float32 and m.max() <= 1
    u = O.upsample(m.reshape(Gh, Gw), H, W)
    assert u.dtype == np.float32 and u.shape == (H, W) and u.min() >= 0 and u.max() <= 1
    ref = F.interpolate(torch.from_numpy(m.astype(np.float64)).view(1, 1, Gh, Gw), size=(H, W), mode="bilinear",
                        align_corners=False)[0, 0].numpy()
    err, bound = np.abs(u.astype(np.float64) - ref).max(), 8 * max(Gh, Gw) * 2.0 ** -24 * float(m.max())
    print("upsample %s: max error %.3e = %.2f of the bound" % (shape, err, err / bound))
    assert err <= bound
    image = (torch.randn(1, 3, H, W, generator=g) * 0.25 + 0.5).numpy()
    got = O.oracle(image, a.reshape(1, 1, -1), None, None, Gh, Gw, "mask", 0)[0][0, 1]
    m64 = a.astype(np.float64) / float(a.max())
    u64 = F.interpolate(torch.from_numpy(m64).view(1, 1, Gh, Gw), size=(H, W), mode="bilinear", align_corners=False)[0, 0].numpy()
    x64 = np.clip(image[0].astype(np.float64) * np.float32(O.STD).astype(np.float64)[:, None, None]
                  + np.float32(O.MEAN).astype(np.float64)[:, None, None], 0, 1).transpose(1, 2, 0)
    g64 = float(np.float32(O.FLOOR)) + (1 - float(np.float32(O.FLOOR))) * u64
    want = np.floor(np.clip(x64 * g64[:, :, None], 0, 1) * 255 + 0.5).astype(np.int32)
    delta = np.abs(got.astype(np.int32) - want)
    print("mask bytes %s: %d of %d differ from the float64 pipeline" % (shape, int((delta != 0).sum()), delta.size))
    assert delta.max() <= 1


@pytest.mark.parametrize("G,extent", ((7, 224), (14, 448)))
def test_the_weights_of_an_integer_ratio_are_exact(G, extent):
    i0, i1, w0, w1 = O.axis(G, extent)
    k = extent // G
    for y in range(extent):
        src = max((y + 0.5) / k - 0.5, 0.0)                      # exact in binary: k = 32
        lo = min(int(src), G - 1)
        assert (i0[y], i1[y]) == (lo, min(lo + 1, G - 1)) and float(w1[y]) == src - lo and float(w0[y]) == 1 - (src - lo)
    assert w0.dtype == w1.dtype == np.float32


def test_the_oracles_normalisation_names_every_bad_map():
    ok = np.array([0.25, 0.5, 0.125, 0.125], dtype=np.float32)
    m, bad = O.normalise(ok)
    assert not bad and m.tolist() == [0.5, 1.0, 0.25, 0.25]
    for spoiled in ([0.25, np.nan, 0.5], [np.inf, 0.5], [0.5, -np.inf], [0.5, -1e-30], [0.0, 0.0], [1e-40, 2e-40]):
        m, bad = O.normalise(np.array(spoiled, dtype=np.float32))
        assert bad and not m.any(), spoiled
    assert not O.normalise(np.array([3e-39, 0.0], dtype=np.float32))[1]          # a denormal maximum whose reciprocal is finite
    assert not O.normalise(np.array([-0.0, 1.0], dtype=np.float32))[1]           # -0 is not negative


# ---- PNG and sheet ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((1, 1), (5, 7), (64, 100)))
def test_write_png_round_trips(tmp_path, shape):
    g = torch.Generator().manual_seed(8300)
    px = torch.randint(0, 256, shape + (3,), generator=g, dtype=torch.uint8)
    px[0, 0] = torch.tensor([0, 255, 128], dtype=torch.uint8)
    path = str(tmp_path / "a.png")
    OV.write_png(path, px)
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and raw[12:16] == b"IHDR" and raw[-8:-4] == b"IEND"
    assert struct.unpack(">II", raw[16:24]) == (shape[1], shape[0])
    idat = raw.index(b"IDAT")
    n = struct.unpack(">I", raw[idat - 4:idat])[0]
    assert len(zlib.decompress(raw[idat + 4:idat + 4 + n])) == shape[0] * (1 + 3 * shape[1])
    assert np.array_equal(O.read_png(path), px.numpy())
    OV.write_png(path, px.numpy())                               # an array as well
    assert np.array_equal(O.read_png(path), px.numpy())
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(path) as im:
            assert im.mode == "RGB" and im.size == (shape[1], shape[0]) and np.array_equal(np.asarray(im), px.numpy())
    for bad in (px.numpy().astype(np.int32), px.numpy()[:, :, :2], px.numpy()[0]):
        with pytest.raises(ValueError, match="uint8"):
            OV.write_png(path, bad)


def test_sheet_lays_the_panels_side_by_side():
    panels = torch.arange(4 * 5 * 6 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).view(4, 5, 6, 3)
    s = OV.sheet(panels)
    assert tuple(s.shape) == (5, 24, 3) and s.dtype == torch.uint8
    for p in range(4):
        assert torch.equal(s[:, 6 * p:6 * p + 6], panels[p])
    assert np.array_equal(OV.sheet(panels.numpy()), s.numpy())
    with pytest.raises(ValueError, match="panels"):
        OV.sheet(panels[0])


def test_default_lut_values():
    lut = OV.lut_values()
    assert lut.shape == (256, 3) and lut.dtype == np.float32 and lut.min() == 0 and lut.max() == 1
    assert lut[0].tolist() == [0, 0, 1] and lut[255].tolist() == [1, 1, 0]      # blue -> red -> yellow
    assert (np.diff(lut[:, 0]) >= 0).all() and (np.diff(lut[:, 1]) >= 0).all() and (np.diff(lut[:, 2]) <= 0).all()
    assert abs(float(lut[128, 0]) - 1) < 1e-6 and float(lut[127, 1]) == 0


# ---- predict.py -----------------------------------------------------------------------------------------------------------------
def test_the_parsers_defaults():
    a = P.build_parser().parse_args([])
    assert (a.attention_overlays, a.overlay_mode, a.overlay_samples, a.overlay_alpha, a.overlay_floor, a.image_mean, a.image_std,
            a.overlay_strip) == (None, "heat", 16, 0.6, 0.3, None, None, 32)
    assert (a.predictions, a.topk, a.attention_maps, a.test_size) == (None, 5, None, 1000)      # the flags there were
    a = P.build_parser().parse_args(["--attention_overlays", "d", "--overlay_mode", "mask", "--overlay_samples", "0", "--image_mean",
                                     "0.1", "0.2", "0.3", "--image_std", "1", "2", "3", "--overlay_strip", "0"])
    assert (a.attention_overlays, a.overlay_mode, a.overlay_samples, a.image_mean, a.image_std, a.overlay_strip) \
        == ("d", "mask", 0, [0.1, 0.2, 0.3], [1.0, 2.0, 3.0], 0)
    assert not hasattr(T.build_parser().parse_args([]), "attention_overlays")   # prediction's flag, not training's
    for bad in (["--overlay_mode", "jet"], ["--image_mean", "0.1", "0.2"]):
        with pytest.raises(SystemExit):
            P.build_parser().parse_args(bad)


def test_predict_refuses_before_anything_is_built(monkeypatch, tmp_path, capsys):
    monkeypatch.setattr(T, "model_from_args", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a model was built")))
    out = str(tmp_path / "sheets")
    for argv, word in ((["--model", "baseline"], "has no attention maps"), (["--model", "bert"], "has no attention maps"),
                       (["--image_features", "t.npy"], "has no pixels"), (["--overlay_samples", "-1"], "--overlay_samples"),
                       (["--overlay_strip", "-2"], "--overlay_strip"), (["--overlay_alpha", "1.5"], "[0, 1]"),
                       (["--overlay_floor", "-0.5"], "[0, 1]")):
        with pytest.raises(SystemExit):
            P.main(["--model_ckpt", "x.pth", "--attention_overlays", out] + argv)
        assert word in capsys.readouterr().err, argv
    assert not (tmp_path / "sheets").exists()

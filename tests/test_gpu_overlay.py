"""GPU: attention overlays (csrc/overlay.hip, include/coattn.h v0.21.0, vqa_amd.overlay, predict.py --attention_overlays) --
the render's C-ABI against the numpy oracle of tests/_overlay.py byte for byte in both modes, every layout of the image, bad
maps and bad pixels, the question strip, the Python layer against the C-ABI, and predict.py's files against the Python layer."""
import json

import numpy as np
import pytest
import torch

from vqa_amd import overlay as OV, predict as P, train as T

from tests import _overlay as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROWS, THREADS = O.constants()
# (B, L, H, W, Gh, Gw, T, strip): the smallest that reach each branch
SHAPES = ((1, 1, 4, 4, 1, 1, 1, 0),
          (2, 3, 224, 224, 7, 7, 26, 32),                       # the shipped grid
          (1, 3, 28, 56, 14, 14, 26, 8),                        # stands for 448 px; the ratio differs between the axes
          (3, 2, 20, 36, 7, 5, 5, 3),                           # a non-integer ratio
          (1, 1, 12, 12, 14, 14, 3, 1),                         # downsampling
          (1, 2, ROWS - 1, 8, 3, 2, 4, 2), (1, 2, ROWS, 8, 3, 2, 4, 2), (1, 2, ROWS + 1, 8, 3, 2, 4, 2),
          (1, 2, ROWS + 1, 8, 3, 2, 4, 0),
          (1, 1, 3, THREADS * 4 + 4, 2, 3, 7, 1),               # one vector past a full workgroup pass
          (1, 8, 8, 8, 3, 3, 5, 2),                             # L = 8
          (1, 2, 8, 16, 2, 2, 16, 2),                           # T = W
          (1, 4, 16, 16, 64, 64, 3, 1), (1, 8, 12, 12, 64, 64, 3, 0))      # 64 KB and 128 KB of maps in LDS (the raised limit)
MODES = ("heat", "mask")
SMALLISH = (3, 2, 20, 36, 7, 5, 5, 3)


def _id(s):
    return "B%d_L%d_%dx%d_g%dx%d_T%d_s%d" % s


def _same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), O.diff(got, want)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("mode", MODES)
def test_bytes_equal_the_oracles(mode, shape):
    r, want, n_bad = O.run_case(shape, mode)
    assert n_bad == 0 and r["bad"] == 0
    _same(r["out"], want)


@pytest.mark.parametrize("shape", (SMALLISH, (1, 3, 28, 56, 14, 14, 26, 8)), ids=_id)
@pytest.mark.parametrize("layout", ("nhwc", "pad4", "pad1"))
@pytest.mark.parametrize("mode", MODES)
def test_every_image_layout_gives_the_contiguous_images_bytes(mode, layout, shape):
    base, want, _ = O.run_case(shape, mode)
    r, _, _ = O.run_case(shape, mode, layout=layout)
    _same(r["out"], want)
    _same(r["out"], base["out"])


def test_no_lengths_and_no_question_maps():
    for mode in MODES:
        r, want, _ = O.run_case(SMALLISH, mode, lens=False)                      # q_len = NULL: every row has T entries
        _same(r["out"], want)
        image, a_v, a_q, _ = O.case(*SMALLISH[:7])
        lut = O.default_lut()
        r = O.run(image, a_v, None, None, 7, 5, mode, 0, lut=lut)                # a_q = NULL, strip_h = 0
        _same(r["out"], O.oracle(image, a_v, None, None, 7, 5, mode, 0, lut=lut)[0])
        full = O.run(image, a_v, a_q, None, 7, 5, mode, 3, lut=lut)["out"]       # the panels above a strip are those without one
        _same(full[:, :, :20], r["out"])
        assert O.run(image, a_v, a_q, None, 7, 5, mode, 0, lut=lut, bad=False)["rc"] == 0     # a_q given and ignored; no counter


def test_repeats_its_bytes():
    for mode in MODES:
        a, _, _ = O.run_case((2, 3, 224, 224, 7, 7, 26, 32), mode)
        b, _, _ = O.run_case((2, 3, 224, 224, 7, 7, 26, 32), mode)
        _same(a["out"], b["out"])


def test_panel_zero_is_the_denormalised_image():
    image = O.case(*SMALLISH[:7])[0]
    r, _, _ = O.run_case(SMALLISH, "mask")
    x = image.astype(np.float32) * np.float32(O.STD)[None, :, None, None] + np.float32(O.MEAN)[None, :, None, None]
    want = (np.clip(x, 0, 1).astype(np.float32) * np.float32(255) + np.float32(0.5)).astype(np.int32).transpose(0, 2, 3, 1)
    assert 0 in want and 255 in want                                             # both sides of the clamp are taken
    _same(r["out"][:, 0, :20], want.astype(np.uint8))
    assert not r["out"][:, 0, 20:].any()                                         # its strip rows are 0


# ---- bad maps and bad pixels ----------------------------------------------------------------------------------------------------
def _spoil(a, kind):
    a = a.copy()
    if kind == "nan":
        a[min(3, a.size - 1)] = np.nan
    elif kind == "inf":
        a[0] = np.inf
    elif kind == "negative":
        a[-1] = -1e-3
    elif kind == "zero":
        a[:] = 0
    elif kind == "denormal":
        a[:] = np.float32(1e-41) * np.arange(1, a.size + 1, dtype=np.float32)    # 1 / max overflows
        with np.errstate(over="ignore"):
            assert np.isinf(np.float32(1) / a.max()) and a.max() > 0
    return a


@pytest.mark.parametrize("kind", ("nan", "inf", "negative", "zero", "denormal"))
@pytest.mark.parametrize("mode", MODES)
def test_a_bad_map_is_drawn_as_zeros_and_counted_and_touches_no_other_panel(mode, kind):
    B, L, H, W, Gh, Gw, T, strip = SMALLISH
    image, a_v, a_q, q_len = O.case(B, L, H, W, Gh, Gw, T)
    lut = O.default_lut()
    clean = O.run(image, a_v, a_q, q_len, Gh, Gw, mode, strip, lut=lut)
    assert clean["bad"] == 0
    zero_v = O.oracle(image, np.zeros_like(a_v), a_q, q_len, Gh, Gw, mode, strip, lut=lut)[0]
    spoiled = a_v.copy()
    spoiled[1, 2], spoiled[0, 0] = _spoil(a_v[1, 2], kind), _spoil(a_v[0, 0], kind)
    r = O.run(image, spoiled, a_q, q_len, Gh, Gw, mode, strip, lut=lut, bad_start=5)
    want, n_bad = O.oracle(image, spoiled, a_q, q_len, Gh, Gw, mode, strip, lut=lut)
    assert n_bad == 2 and r["bad"] == 5 + 2                                       # added to what the counter held
    _same(r["out"], want)
    for b in range(B):
        for p in range(L + 1):
            if (p - 1, b) in ((1, 2), (0, 0)):
                _same(r["out"][b, p, :H], zero_v[b, p, :H])                       # the m = 0 picture
                _same(r["out"][b, p, H:], clean["out"][b, p, H:])                 # its strip is a_q's
            else:
                _same(r["out"][b, p], clean["out"][b, p])
    # the same for a row of a_q (over its first len entries: one spoiled past the length does not count)
    n = [min(max(int(x), 1), T) for x in q_len]
    spoiled_q = a_q.copy()
    spoiled_q[1, 1, :n[1]] = _spoil(a_q[1, 1, :n[1]], kind)
    if n[0] < T:
        spoiled_q[0, 0, n[0]:] = np.nan
    r = O.run(image, a_v, spoiled_q, q_len, Gh, Gw, mode, strip, lut=lut)
    want, n_bad = O.oracle(image, a_v, spoiled_q, q_len, Gh, Gw, mode, strip, lut=lut)
    assert n_bad == 1 and r["bad"] == 1
    _same(r["out"], want)
    keep = np.ones(r["out"].shape[:3], dtype=bool)
    keep[1, 2, H:] = False
    _same(r["out"][keep], clean["out"][keep])
    cells = r["out"][1, 2, H:]
    live = (np.arange(W) * T) // W < n[1]
    colour = (np.clip(lut[0], 0, 1) * 255 + 0.5).astype(np.uint8) if mode == "heat" else np.zeros(3, np.uint8)
    assert (cells[:, live] == colour).all() and not cells[:, ~live].any()


@pytest.mark.parametrize("mode", MODES)
def test_a_bad_pixel_changes_its_own_three_bytes_per_panel(mode):
    B, L, H, W, Gh, Gw, T, strip = SMALLISH
    image, a_v, a_q, q_len = O.case(B, L, H, W, Gh, Gw, T)
    lut = O.default_lut()
    clean = O.run(image, a_v, a_q, q_len, Gh, Gw, mode, strip, lut=lut)["out"]
    spoiled = image.copy()
    spots = {(0, 0, 0, 0): np.nan, (1, 1, 7, 13): 1e30, (2, 2, 19, 35): -1e30, (1, 0, 8, 5): np.inf}      # (b, c, y, x)
    for k, v in spots.items():
        spoiled[k] = v
    r = O.run(spoiled, a_v, a_q, q_len, Gh, Gw, mode, strip, lut=lut)
    assert r["bad"] == 0
    _same(r["out"], O.oracle(spoiled, a_v, a_q, q_len, Gh, Gw, mode, strip, lut=lut)[0])
    touched = np.zeros(clean.shape[:1] + clean.shape[2:4], dtype=bool)
    for b, _, y, x in spots:
        touched[b, y, x] = True
    changed = (r["out"] != clean).any(axis=(1, 4))
    assert not (changed & ~touched).any()
    assert r["out"][0, 0, 0, 0, 0] == 0 and r["out"][1, 0, 7, 13, 1] == 255 and r["out"][2, 0, 19, 35, 2] == 0     # NaN -> 0


# ---- the question strip ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_strip_cells_lengths_and_clamps(mode):
    B, L, H, W, Gh, Gw, T, strip = 4, 2, 4, 36, 2, 2, 5, 2
    image, a_v, a_q, _ = O.case(B, L, H, W, Gh, Gw, T, seed=2)
    lut = O.default_lut()
    lens = np.array([3, 0, T + 5, T])
    r = O.run(image, a_v, a_q, lens, Gh, Gw, mode, strip, lut=lut)
    _same(r["out"], O.oracle(image, a_v, a_q, lens, Gh, Gw, mode, strip, lut=lut)[0])
    clamped = O.run(image, a_v, a_q, np.array([3, 1, T, T]), Gh, Gw, mode, strip, lut=lut)
    _same(r["out"], clamped["out"])                                              # 0 == 1 and T + 5 == T
    t = (np.arange(W) * T) // W
    assert t[7] == 0 and t[8] == 1 and t[-1] == T - 1                            # 36 / 5: the cells are 8, 7, 7, 7, 7 wide
    for b, n in enumerate((3, 1, T, T)):
        for l in range(L):
            cells = r["out"][b, 1 + l, H:]
            assert (cells == cells[:1]).all()                                    # every strip row alike
            assert not cells[:, t >= n].any()
            for c in range(n):
                assert (cells[0, t == c] == cells[0, t == c][0]).all()           # one colour per cell
            peak = int(np.argmax(a_q[l, b, :n]))                                 # the row's maximum is drawn at full scale
            full = (np.clip(lut[255], 0, 1) * 255 + 0.5).astype(np.uint8) if mode == "heat" else np.full(3, 255, np.uint8)
            assert (cells[0, t == peak] == full).all()


# ---- the Python layer -------------------------------------------------------------------------------------------------------------
def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.array(a)).to(DEV) for a in arrays]


@pytest.mark.parametrize("mode", MODES)
def test_render_attention_is_the_c_abi_run(mode):
    B, L, H, W, Gh, Gw, T, strip = SMALLISH
    image, a_v, a_q, q_len = O.case(B, L, H, W, Gh, Gw, T)
    kw = dict(alpha=O.ALPHA, floor=O.FLOOR, mean=O.MEAN, std=O.STD)
    want = O.run(image, a_v, a_q, q_len, Gh, Gw, mode, strip, lut=O.default_lut())["out"]
    im, av, aq = _dev(image, a_v, a_q)
    for lens in (torch.from_numpy(q_len.copy()), torch.from_numpy(q_len.astype(np.int32)).to(DEV), torch.from_numpy(q_len.astype(np.int16))):
        got = OV.render_attention(im, av, aq, lens, grid=(Gh, Gw), mode=mode, strip=strip, **kw)
        assert got.dtype == torch.uint8 and got.device == im.device and tuple(got.shape) == (B, L + 1, H + strip, W, 3)
        _same(got.cpu().numpy(), want)
    _same(OV.render_attention(im.contiguous(memory_format=torch.channels_last), av, aq, torch.from_numpy(q_len.copy()), grid=(Gh, Gw),
                              mode=mode, strip=strip, **kw).cpu().numpy(), want)
    with pytest.raises(ValueError, match="square"):
        OV.render_attention(im, av, aq, mode=mode, **kw)                          # 35 locations and no grid
    user = O.user_lut()
    got = OV.render_attention(im, av, aq, None, grid=(Gh, Gw), mode=mode, strip=strip, lut=_dev(user)[0], **kw)
    _same(got.cpu().numpy(), O.run(image, a_v, a_q, None, Gh, Gw, mode, strip, lut=user)["out"])
    if mode == "heat":
        assert not np.array_equal(got.cpu().numpy()[:, 1:], want[:, 1:])
    # a square grid is found; the defaults are ImageNet's normalisation, alpha 0.6, floor 0.3 and no strip
    image, a_v, a_q, q_len = O.case(1, 3, 28, 56, 14, 14, 26)
    im, av, aq = _dev(image, a_v, a_q)
    got = OV.render_attention(im, av, aq, mode=mode)
    _same(got.cpu().numpy(), O.run(image, a_v, None, None, 14, 14, mode, 0, alpha=0.6, floor=0.3, mean=OV.IMAGENET_MEAN,
                                   std=OV.IMAGENET_STD, lut=O.default_lut())["out"])
    assert OV.bad_maps() == 0
    assert OV.default_lut(DEV) is OV.default_lut(DEV) and np.array_equal(OV.default_lut(DEV).cpu().numpy(), OV.lut_values())


def test_bad_maps_reads_and_clears_the_counter():
    image, a_v, a_q, q_len = O.case(*SMALLISH[:7])
    spoiled = a_v.copy()
    spoiled[0, 1, 4], spoiled[1, 2, :] = np.nan, 0
    im, av, aq = _dev(image, spoiled, a_q)
    assert OV.bad_maps() == 0
    OV.render_attention(im, av, aq, grid=(7, 5), strip=3)
    OV.render_attention(im, av, grid=(7, 5), mode="mask")
    assert OV.bad_maps() == 4 and OV.bad_maps() == 0


# ---- predict.py --attention_overlays ------------------------------------------------------------------------------------------------
@pytest.fixture
def repeatable_convolutions():
    """Two prediction runs are compared bit for bit: the encoder's convolutions run on the deterministic solvers (on the default
    ones the eval-mode encoder does not repeat its own bits: tests/test_gpu_cached_features.py)."""
    old, torch.backends.cudnn.deterministic = torch.backends.cudnn.deterministic, True
    yield
    torch.backends.cudnn.deterministic = old


@pytest.mark.parametrize("co_attention", ("parallel", "alternating"))
def test_predict_writes_the_sheets_render_attention_gives(tmp_path, capsys, repeatable_convolutions, co_attention):
    """A two-step-trained checkpoint (trained at 64 px: the encoder is convolutional; the command line has no flag for the
    embedding and hidden sizes, so they are the registry's), predicted at 224 px over 5 samples in batches of 2 with overlays of
    the first 3."""
    ckpt = str(tmp_path / "net.pth")
    model = ["--model", "attention", "--co_attention", co_attention, "--num_cls", "10", "--vocab_size", "50", "--batch_size", "2"]
    T.main(model + ["--image_size", "64", "--num_steps", "2", "--log_interval", "2", "--save_path", ckpt])
    argv = model + ["--image_size", "224", "--model_ckpt", ckpt, "--test_size", "5"]
    out = {}
    for run, extra in (("plain", []), ("drawn", ["--attention_overlays", str(tmp_path / "sheets"), "--overlay_samples", "3"])):
        preds, maps = str(tmp_path / (run + ".jsonl")), str(tmp_path / (run + ".npz"))
        P.main(argv + ["--predictions", preds, "--attention_maps", maps] + extra)
        z = np.load(maps)
        out[run] = (open(preds).read(), {k: z[k] for k in z.files})
    capsys.readouterr()
    assert OV.bad_maps() == 0
    assert out["plain"][0] == out["drawn"][0] and out["plain"][1].keys() == out["drawn"][1].keys()
    for k, v in out["plain"][1].items():
        assert v.dtype == out["drawn"][1][k].dtype and v.tobytes() == out["drawn"][1][k].tobytes(), k
    files = sorted(p.name for p in (tmp_path / "sheets").iterdir())
    assert files == ["index.json"] + ["sample_%06d.png" % i for i in range(3)]
    records = [json.loads(line) for line in out["drawn"][0].splitlines()]
    index = json.load(open(str(tmp_path / "sheets" / "index.json")))
    z = out["drawn"][1]
    ds = T.SyntheticVQADataset(5, (224, 224), 26, 50, 11, P.TEST_SEED)
    S, L, Gh, Gw = z["a_v"].shape
    assert (S, L) == (5, 3) and z["a_q"].shape == (5, 3, 26)
    for i, entry in enumerate(index):
        rec = records[i]
        assert entry["index"] == i == rec["index"] and entry["file"] == "sample_%06d.png" % i
        assert (entry["label"], entry["top"], entry["prob"]) == (rec["label"], rec["top"], rec["prob"])
        assert entry["ques_len"] == int(z["ques_len"][i]) and entry["question"] == ds[i]["question"].tolist()
        a_v = torch.from_numpy(z["a_v"][i].reshape(L, 1, Gh * Gw)).to(DEV)
        a_q = torch.from_numpy(z["a_q"][i].reshape(L, 1, 26)).to(DEV)
        want = OV.sheet(OV.render_attention(ds[i]["image"][None].to(DEV), a_v, a_q, strip=32)[0]).cpu().numpy()
        got = O.read_png(str(tmp_path / "sheets" / entry["file"]))
        assert got.shape == (224 + 32, 4 * 224, 3)
        _same(got, want)
    assert OV.bad_maps() == 0

"""Image preprocessing and the dataset files, on the CPU: the numpy restatement of include/coattn_ext.h's contract
(tests/_preprocess.py) against Pillow and against Pillow's recorded bytes, the package's tables against the restatement, the
second signature table against the second header, the text rules against the reference's utils.py, the dataset on a fixture in
tmp_path, and the command lines' refusals."""
import ctypes as C
import importlib.util
import os
import pickle
import re
import sys
import types

import numpy as np
import pytest
import torch

import vqa_amd  # noqa: F401
from tests import _preprocess as R
from tests._header import args as header_args, declared
from vqa_amd import _lib, data as D, preprocess as PP, train as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preprocess_pil.npz")
REFERENCE = "/root/reference"


# ---- the contract -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,S", R.PIL_SHAPES, ids=lambda v: str(v))
def test_the_restatement_gives_pillows_bytes(h, w, S):
    Image = pytest.importorskip("PIL.Image")
    img = np.ascontiguousarray(R.image(h, w))
    want = np.asarray(Image.fromarray(img).resize((S, S), Image.BILINEAR))
    got = R.resize_u8(img, S)
    assert got.shape == want.shape == (S, S, 3) and int((got != want).sum()) == 0


def test_the_restatement_gives_pillows_recorded_bytes():
    z = np.load(GOLDEN)
    shapes = z["shapes"]
    assert len(shapes) >= 5
    for i, (h, w, S) in enumerate(shapes.tolist()):
        img, want = z["in_%d" % i], z["out_%d" % i]
        assert img.shape == (h, w, 3) and want.shape == (S, S, 3) and h <= 64 and w <= 64 and S in (14, 28)
        assert int((R.resize_u8(img, S) != want).sum()) == 0, (h, w, S)


def test_the_lookup_table_has_torchs_bits():
    lut = PP.lut_values()
    assert lut.shape == (3, 256) and lut.dtype == torch.float32
    assert np.array_equal(R.bits_of(lut.numpy()), R.bits_of(R.lut()))
    # ToTensor + Normalize as torchvision spells them: uint8 -> float().div(255), then sub_(mean[:, None, None]).div_(std[...])
    x = torch.arange(256, dtype=torch.uint8).reshape(1, 256, 1).expand(3, 256, 1).float().div(255)
    mean = torch.as_tensor(PP.IMAGENET_MEAN, dtype=torch.float32).view(-1, 1, 1)
    std = torch.as_tensor(PP.IMAGENET_STD, dtype=torch.float32).view(-1, 1, 1)
    assert np.array_equal(R.bits_of(x.clone().sub_(mean).div_(std).reshape(3, 256).numpy()), R.bits_of(lut.numpy()))
    other = PP.lut_values((0.1, 0.2, 0.3), (0.5, 2.0, 1.0))
    assert np.array_equal(R.bits_of(other.numpy()), R.bits_of(R.lut((0.1, 0.2, 0.3), (0.5, 2.0, 1.0))))
    with pytest.raises(ValueError, match="std"):
        PP.lut_values(std=(1.0, 0.0, 1.0))


@pytest.mark.parametrize("n_in,S", sorted({(n, S) for h, w, S in R.PIL_SHAPES for n in (h, w)} | {(3827, 14), (2, 448)}))
def test_the_packages_tables_are_the_restatements(n_in, S):
    tab = PP.axis_table(n_in, S)
    want = R.table(n_in, S)
    assert tab.dtype == np.int32 and tab.shape == want.shape and np.array_equal(tab, want)
    lo, n = tab[:, 0], tab[:, 1]
    assert (lo >= 0).all() and (n >= 1).all() and (lo + n <= n_in).all() and (tab[:, 2:].sum(1) > 0).all()
    assert abs(int(tab[:, 2:].sum(1).max()) - (1 << 22)) <= tab.shape[1]          # the taps sum to 2^22 but for their rounding


def test_pack_lays_a_batch_out_as_the_header_says():
    imgs = R.images(((37, 23), (5, 7), (28, 28), (5, 23)))
    pre = PP.ImagePreprocessor.__new__(PP.ImagePreprocessor)                     # (no device: the host side alone)
    pre.S, pre._tables = 14, {}
    p = pre.pack(imgs)
    assert p.B == 4 and p.sizes == [(37, 23), (5, 7), (28, 28), (5, 23)] and (p.max_h, p.max_w) == (37, 28)
    assert p.desc_off % 16 == 0 and p.coef_off % 16 == 0 and p.pix_off % 16 == 0 and p.buf.numel() == p.pix_off + p.pix_bytes
    raw = p.buf.numpy()
    coef = raw[p.coef_off:p.coef_off + 4 * p.coef_count].view(np.int32)
    for d, img in zip(p.desc(), imgs):
        h, w, _ = img.shape
        assert (d["h"], d["w"]) == (h, w) and d["offset"] % 16 == 0 and d["offset"] + 3 * h * w <= p.pix_bytes
        assert np.array_equal(raw[p.pix_off + d["offset"]:p.pix_off + d["offset"] + 3 * h * w], img.reshape(-1))
        for tab, taps, n_in in ((d["tab_x"], d["taps_x"], w), (d["tab_y"], d["taps_y"], h)):
            want = R.table(n_in, 14)
            assert taps == want.shape[1] - 2 and np.array_equal(coef[tab:tab + want.size].reshape(want.shape), want)
    assert p.coef_count == sum(R.table(n, 14).size for n in (5, 7, 23, 28, 37))     # one table per distinct size
    before = raw[p.pix_off:].copy()
    assert p[torch.tensor([2, 0, 3, 1])] is p and p.sizes == [(28, 28), (37, 23), (5, 23), (5, 7)]
    assert [int(h) for h in p.desc()["h"]] == [28, 37, 5, 5] and np.array_equal(raw[p.pix_off:], before)
    with pytest.raises(ValueError, match="permutation"):
        p.permute([0, 0, 1, 2])
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            pre.pack([bad])
    with pytest.raises(ValueError, match="empty"):
        pre.pack([])


def test_preprocess_host_is_the_restatement():
    pytest.importorskip("PIL")
    sizes = ((37, 23), (5, 7), (1, 1))
    out = PP.preprocess_host(R.images(sizes), 14)
    assert out.shape == (3, 3, 14, 14) and out.dtype == torch.float32
    assert np.array_equal(R.bits_of(out.numpy()), R.bits_of(R.reference_of(sizes, 14)))


# ---- supported, and what is refused ---------------------------------------------------------------------------------------------
def test_supported_and_every_refusal():
    lib = _lib.load()
    assert lib.coattn_version() >= 2300
    k = R.constants()
    assert k["ROWS"] == _lib.PREPROCESS_ROWS and k["MAX_TAPS"] == _lib.PREPROCESS_MAX_TAPS and k["THREADS"] % 64 == 0
    ok = lib.coattn_preprocess_supported
    assert ok(160, 224, 640, 640) and ok(160, 448, 640, 640) and ok(1, 1, 1, 1) and ok(1, k["MAX_S"], 1, k["MAX_IN"])
    assert PP.supported(160, 224, 480, 640) and not PP.supported(160, 224, 4096, 640)
    for B, S, h, w in ((0, 224, 8, 8), (1, 0, 8, 8), (1, k["MAX_S"] + 1, 8, 8), (1, 14, 0, 8), (1, 14, 8, 0),
                       (1, 14, k["MAX_IN"] + 1, 8), (1, 14, 8, k["MAX_IN"] + 1), (1, 224, k["MAX_IN"], 8)):
        assert not ok(B, S, h, w), (B, S, h, w)
    # the LDS rule of the header: 3072 + 16 ceil(3 S rows / 16) <= 163840, monotone in max_h; the width is not limited by it
    for S in (14, 28, 224, 448):
        hs = [h for h in range(1, k["MAX_IN"] + 1, 7) if ok(1, S, h, 8)]
        top = max(hs)
        assert hs == list(range(1, top + 1, 7)) and ok(1, S, top, k["MAX_IN"])
        s = (top + 7) / S
        rows = min(top + 7, int((k["ROWS"] - 1) * s + 2 * max(s, 1.0) + 1) + 1)
        assert 3072 + 16 * -(-3 * S * rows // 16) > 163840
    call = dict(pixels=1 << 20, pixel_bytes=64, desc=1 << 21, coef=1 << 22, coef_count=64, lut=1 << 23, out=1 << 24, sB=1, sC=1,
                sH=1, sW=1, B=1, S=14, max_h=8, max_w=8, stream=0)
    for edit, text in ((dict(S=0), "not supported"), (dict(max_h=5000), "not supported"), (dict(pixels=0), "null"),
                       (dict(desc=0), "null"), (dict(coef=0), "null"), (dict(lut=0), "null"), (dict(out=0), "null"),
                       (dict(pixel_bytes=0), "positive"), (dict(coef_count=0), "positive"), (dict(desc=(1 << 21) + 4), "aligned"),
                       (dict(coef=(1 << 22) + 2), "aligned"), (dict(out=(1 << 24) + 1), "aligned"),
                       (dict(bad_images=(1 << 25) + 2), "aligned")):
        rc = _lib.bind("coattn_preprocess_images", **{**call, **edit}).code()       # (refused before any device work)
        assert rc == -1 and text in lib.coattn_last_error().decode(), (edit, lib.coattn_last_error())


# ---- the second table against the second header -----------------------------------------------------------------------------------
SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "long long": C.c_int64, "double": C.c_double, "float": C.c_float,
           "size_t": C.c_size_t}
POINTERS = {"void": C.c_void_p, "int32_t": C.c_void_p, "size_t": C.POINTER(C.c_size_t), "float": C.POINTER(C.c_float),
            "int": C.POINTER(C.c_int), "char": C.c_char_p}
RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}


def test_the_second_table_is_the_second_header():
    hdr = R.ext_header()
    decl = declared(hdr)
    assert list(_lib.EXT_SIGNATURES) == list(decl) == list(_lib.EXT_EXPORTS) and len(decl) >= 2      # names, in the header's order
    assert set(re.findall(r"^[a-z][^\n(]*\b(coattn_\w+)\(", hdr, re.M)) == set(decl)               # no declaration escapes
    assert set(_lib.EXT_RESTYPES) == {n for n, ret in decl.items() if ret != "int"}
    lib = _lib.load()
    for name, sig in _lib.EXT_SIGNATURES.items():
        declared_args = [a.rsplit(" ", 1) for a in header_args(hdr, name)]
        assert [n for n, _ in sig] == [n for _, n in declared_args], name
        for (n, ctype), (ctext, _) in zip(sig, declared_args):
            base = ctext.replace("const", "").replace("*", "").strip()
            assert ctype is (POINTERS[base] if "*" in ctext else SCALARS[base]), (name, n, ctext, ctype)
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [t for _, t in sig]
        assert fn.restype is RETURNS[decl[name]] is _lib.EXT_RESTYPES.get(name, C.c_int)
    # the first table is what it was: the 78 functions of 0.22.0, none of them the new ones
    assert len(_lib.EXPORTS) == len(_lib.SIGNATURES) == 78 and not set(_lib.EXPORTS) & set(_lib.EXT_EXPORTS)
    fields = re.search(r"typedef struct coattn_preprocess_desc \{(.*?)\} coattn_preprocess_desc;", hdr, re.S).group(1)
    names = [n for line in re.sub(r"/\*.*?\*/", "", fields, flags=re.S).split(";") for n in line.replace(",", " ").split()
             if n not in ("long", "int")]
    assert [f for f, _ in _lib.PreprocessDesc._fields_] == names == list(R.DESC.names) == list(PP.DESC_DTYPE.names)
    assert C.sizeof(_lib.PreprocessDesc) == R.DESC.itemsize == 32


def test_bind_and_replace_serve_the_second_table():
    t = torch.zeros(64)
    kw = dict(pixels=t, pixel_bytes=64, desc=t, coef=t, coef_count=16, lut=t, out=t, sB=1, sC=2, sH=3, sW=4, B=1, S=14,
              max_h=8, max_w=9)
    call = _lib.bind("coattn_preprocess_images", **kw)
    assert call.name == "coattn_preprocess_images" and len(call) == len(_lib.EXT_SIGNATURES[call.name]) - 1
    assert call[11] is None and tuple(call[7:11]) == (1, 2, 3, 4) and tuple(call[12:]) == (1, 14, 8, 9)
    again = call.replace(bad_images=t, stream=0x7f00)
    assert again[11].value == t.data_ptr() and again[-1].value == 0x7f00 and len(again) == len(call) + 1
    with pytest.raises(TypeError, match="max_d"):
        _lib.bind("coattn_preprocess_images", max_d=1, **kw)
    with pytest.raises(TypeError, match="missing argument 'lut'"):
        _lib.bind("coattn_preprocess_images", **{k: v for k, v in kw.items() if k != "lut"})


# ---- the text rules against the reference's ---------------------------------------------------------------------------------------
def _reference_utils():
    path = os.path.join(REFERENCE, "utils.py")
    if not os.path.isfile(path):
        pytest.skip("the reference is not present")
    if "matplotlib" not in sys.modules and importlib.util.find_spec("matplotlib") is None:
        sys.modules["matplotlib"] = types.ModuleType("matplotlib")
        sys.modules["matplotlib.pyplot"] = sys.modules["matplotlib"].pyplot = types.ModuleType("matplotlib.pyplot")
    sys.dont_write_bytecode = True                               # the reference tree is read-only
    spec = importlib.util.spec_from_file_location("_vqa_ref_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TEXTS = ("What color is the cat?", "Is this a dog, or a cat", "How many people's hats are there?", "  what,is,on the table  ",
         "S s 's it's U.S.A.", "", " , ,", "Man sleeping next to a cat on a bed.", "don't \"quote\" (this) -- ok?! #1 50%",
         "TAB\there and\nnewline", "ünïcode ¿qué?")


def test_text_rules_and_vocabulary_equal_the_references(tmp_path):
    U = _reference_utils()
    for text in TEXTS:
        assert D.preprocess_text(text) == U.preprocess_text(text), text
    fx = R.write_fixture(str(tmp_path))
    lines = open(fx["data_file"]).read().strip().split("\n")
    for min_count, K in ((1, 4), (2, 3), (1, 100), (3, 1)):
        mine = D.build_vocab(fx["data_file"], min_count, K)
        word2idx, idx2word, longest = U.build_vocab(lines, min_count)
        label2idx, idx2label = U.build_answer(lines, K)
        assert mine == {"word2idx": word2idx, "idx2word": idx2word, "label2idx": label2idx, "idx2label": idx2label,
                        "max_seq_length": longest}
        assert list(mine["word2idx"]) == list(word2idx) and list(mine["label2idx"]) == list(label2idx)      # the order too
    vocab = fx["vocab"]
    for _, question, _ in fx["lines"]:
        for T_ in (vocab["max_seq_length"], 3):
            words = U.preprocess_text(question)
            ids = [vocab["word2idx"][w] if w in vocab["word2idx"] else vocab["word2idx"]["<UNKNOWN>"] for w in words]
            want = U.pad_sequences(ids, T_)
            got, n = D.encode_question(question, vocab["word2idx"], T_)
            assert np.array_equal(got, want) and got.dtype == np.int64 and n == int(sum(1 - np.equal(want, 0)))


def test_text_rules_without_the_reference():
    assert D.preprocess_text("Man sleeping next to a cat on a bed.") == ["man", "sleeping", "next", "to", "a", "cat", "on", "a", "bed"]
    assert D.preprocess_text("How many people's hats, are there?") == ["how", "many", "peoples", "hats", "are", "there"]
    assert D.preprocess_text("it 's S s") == ["it", "s"]                           # `s` is dropped before lower-casing: `S` stays
    ids, n = D.encode_question("a zebra cat", {"<PAD>": 0, "<UNKNOWN>": 1, "a": 2, "cat": 3}, 5)
    assert ids.tolist() == [2, 1, 3, 0, 0] and n == 3
    ids, n = D.encode_question(["a", "cat", "a", "cat"], {"<PAD>": 0, "<UNKNOWN>": 1, "a": 2, "cat": 3}, 3)
    assert ids.tolist() == [2, 3, 2] and n == 3


# ---- the dataset ------------------------------------------------------------------------------------------------------------------
def test_vocabulary_file_round_trip_and_refusals(tmp_path):
    fx = R.write_fixture(str(tmp_path))
    v = fx["vocab"]
    assert v["word2idx"]["<PAD>"] == 0 and v["word2idx"]["<UNKNOWN>"] == 1 and v["label2idx"]["UNKNOWN"] == 0
    assert len(v["label2idx"]) == 5 and v["idx2label"][1] == "yes"              # the most frequent answer leads
    assert list(v["word2idx"])[2:5] == ["what", "color", "is"]                  # first-seen order
    # the reference writes the five keys in another order than it unpacks them by position: by key it does not matter
    shuffled = {k: v[k] for k in ("max_seq_length", "idx2label", "word2idx", "label2idx", "idx2word")}
    path = str(tmp_path / "shuffled.pkl")
    pickle.dump(shuffled, open(path, "wb"))
    assert D.load_vocab(path) == v and list(D.load_vocab(path)) == list(D.VOCAB_KEYS)
    pickle.dump({k: v[k] for k in D.VOCAB_KEYS[:4]}, open(path, "wb"))
    with pytest.raises(ValueError, match="max_seq_length"):
        D.load_vocab(path)
    out = str(tmp_path / "cli.pkl")
    D.main(["vocab", "--train_file", fx["data_file"], "--vocab_file", out, "-K", "4"])
    assert D.load_vocab(out) == v


def test_dataset_collate_and_sorting(tmp_path):
    fx = R.write_fixture(str(tmp_path))
    vocab = D.load_vocab(fx["vocab_file"])
    ds = D.VQAFileDataset(fx["data_file"], fx["img_dir"], vocab)
    assert len(ds) == 24 and len(ds.image_names) == 12 and ds.image_names[:3] == ["img_00.npy", "img_05.npy", "img_10.npy"]
    for i in (0, 7, 23):
        name, question, answer = fx["lines"][i]
        s = ds[i]
        assert np.array_equal(s["image"], np.load(os.path.join(fx["img_dir"], name))) and s["image"].dtype == np.uint8
        ids, n = D.encode_question(question, vocab["word2idx"], vocab["max_seq_length"])
        assert s["question"].tolist() == ids.tolist() and int(s["ques_len"]) == n and s["question"].dtype == torch.int64
        assert int(s["label"]) == vocab["label2idx"].get(answer, 0) and int(s["index"]) == i
    assert any(a not in vocab["label2idx"] for _, _, a in fx["lines"])          # (an answer outside the table occurs)
    rows = D.VQAFileDataset(fx["data_file"], None, vocab, images="row")
    assert [int(rows[i]["image"]) for i in range(24)] == [ds.image_names.index(l[0]) for l in fx["lines"]]
    distinct = D.DistinctImages(ds)
    assert len(distinct) == 12 and np.array_equal(distinct[1]["image"], np.load(os.path.join(fx["img_dir"], "img_05.npy")))
    batch = D.collate([ds[i] for i in (3, 4, 5, 6)])
    assert isinstance(batch["image"], list) and batch["question"].shape == (4, vocab["max_seq_length"])
    pre = PP.ImagePreprocessor.__new__(PP.ImagePreprocessor)
    pre.S, pre._tables = 16, {}
    packed = D.collate([ds[i] for i in (3, 4, 5, 6)], pack=pre.pack)
    pix = packed["image"].buf[packed["image"].pix_off:].clone()
    sizes = list(packed["image"].sizes)
    s = D.sort_batch(packed)
    order = torch.argsort(batch["ques_len"], descending=True, stable=False)
    assert s["ques_len"].tolist() == sorted(batch["ques_len"].tolist(), reverse=True)
    assert sorted(s["index"].tolist()) == [3, 4, 5, 6] and s["image"].sizes == [sizes[[3, 4, 5, 6].index(i)] for i in s["index"].tolist()]
    assert torch.equal(s["image"].buf[s["image"].pix_off:], pix) and len(order) == 4      # descriptor rows moved, pixels did not
    for i, j in enumerate(s["index"].tolist()):
        assert s["question"][i].tolist() == ds[j]["question"].tolist() and int(s["label"][i]) == int(ds[j]["label"])
    # train.sort_batch takes the packed images as it takes a tensor of them
    again = D.collate([ds[i] for i in (3, 4, 5, 6)], pack=pre.pack)
    im, qu, la, ln = T.sort_batch(again["image"], again["question"], again["label"], again["ques_len"])
    assert im is again["image"] and im.sizes == s["image"].sizes and torch.equal(qu, s["question"])
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("img_00.npy\tonly two fields\n")
    with pytest.raises(ValueError, match="line 1"):
        D.VQAFileDataset(bad, fx["img_dir"], vocab)
    np.save(os.path.join(fx["img_dir"], "grey.npy"), np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        D.load_image(os.path.join(fx["img_dir"], "grey.npy"))


def test_a_png_is_decoded_through_pil(tmp_path):
    pytest.importorskip("PIL")
    from vqa_amd.overlay import write_png
    img = np.ascontiguousarray(R.image(9, 6))
    write_png(str(tmp_path / "a.png"), img)
    assert np.array_equal(D.load_image(str(tmp_path / "a.png")), img)


# ---- the command lines --------------------------------------------------------------------------------------------------------
def _args(fx, *more):
    return ["--synthetic", "false", "--train_file", fx["data_file"], "--train_img", fx["img_dir"], "--vocab_file",
            fx["vocab_file"], "--num_cls", "4", *more]


def test_command_line_refusals(tmp_path):
    from vqa_amd import extract as E, predict as P
    fx = R.write_fixture(str(tmp_path))
    ap = T.build_parser()
    assert ap.parse_args([]).synthetic is True and ap.parse_args([]).preprocess is None
    a = ap.parse_args(_args(fx))
    T.check_files(a)
    vocab = T.file_vocab(a)
    assert (a.vocab_size, a.max_seq_length) == (len(vocab["word2idx"]), vocab["max_seq_length"])
    for drop, text in (("--train_file", "--train_file"), ("--train_img", "--train_img"), ("--vocab_file", "--vocab_file")):
        argv = _args(fx)
        i = argv.index(drop)
        with pytest.raises(ValueError, match=text):
            T.check_files(ap.parse_args(argv[:i] + argv[i + 2:]))
    with pytest.raises(ValueError, match="--val_file"):
        T.check_files(a, validates=True)
    for loss in ("soft_ce", "bce"):
        with pytest.raises(ValueError, match="one answer per line"):
            T.check_files(ap.parse_args(_args(fx, "--loss", loss)))
    with pytest.raises(ValueError, match="tokeniser"):
        T.check_files(ap.parse_args(_args(fx, "--model", "attention_bert")))
    with pytest.raises(ValueError, match="WORLD_SIZE"):
        T.check_files(a, world=2)
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="no CPU fallback"):
            T.check_files(ap.parse_args(_args(fx, "--preprocess", "hip")))
    with pytest.raises(SystemExit):
        ap.parse_args(_args(fx, "--preprocess", "gpu"))
    with pytest.raises(ValueError, match="5 labels.*--num_cls 7 needs 8"):
        T.file_vocab(ap.parse_args(_args(fx)[:-1] + ["7"]))
    # cached features need no image directory
    argv = _args(fx, "--image_features", "t.npy")
    i = argv.index("--train_img")
    T.check_files(ap.parse_args(argv[:i] + argv[i + 2:]))
    # the commands themselves: train.py exits with the message, predict.py and extract.py likewise
    with pytest.raises(SystemExit, match="--train_file"):
        T.main(["--synthetic", "false"])
    with pytest.raises(SystemExit, match="one answer per line"):
        T.main(_args(fx, "--loss", "bce"))
    with pytest.raises(SystemExit, match="needs 8"):
        T.main(_args(fx)[:-1] + ["7"])
    with pytest.raises(SystemExit):
        P.main(["--synthetic", "false", "--model_ckpt", "x.pth", "--vocab_file", fx["vocab_file"]])       # no --test_file
    with pytest.raises(SystemExit, match="--val_file"):
        E.main(_args(fx, "--split", "val", "--out", str(tmp_path / "t.npy")))


def test_a_feature_table_of_another_file_list_is_refused():
    from vqa_amd import features as FT
    names = ["a.npy", "b.npy", "c.npy"]
    meta = FT.files_meta(FT.make_meta("attention", 64, 4, 8, "fp32", "train", 0, 3), names)
    assert meta["source"] == "files" and meta["images"] == 3 and meta["names_sha256"] == D.names_digest(names)
    assert set(meta) == set(FT.make_meta("attention", 64, 4, 8, "fp32", "train", 0, 3)) | {"source", "images", "names_sha256"}
    tab = FT.FeatureTable(torch.zeros(3, 4, 8), meta)
    tab.check_files("attention", 64, "train", names)
    for kw, field in ((dict(model_name="attention_resnet"), "model"), (dict(image_size=32), "image_size"), (dict(split="val"), "split"),
                      (dict(image_names=names[:2]), "images"), (dict(image_names=["a.npy", "c.npy", "b.npy"]), "names_sha256")):
        call = dict(model_name="attention", image_size=64, split="train", image_names=names)
        with pytest.raises(ValueError, match="feature table: %s is" % field):
            tab.check_files(**{**call, **kw})
    synthetic = FT.FeatureTable(torch.zeros(3, 4, 8), FT.make_meta("attention", 64, 4, 8, "fp32", "train", 1234, 3))
    with pytest.raises(ValueError, match="source"):
        synthetic.check_files("attention", 64, "train", names)


def test_train_runs_on_files_through_the_host_route(tmp_path, capsys):
    """One epoch of two steps on the CPU with --preprocess host; the co-attention itself has no CPU route, so the baseline."""
    pytest.importorskip("PIL")
    import json
    fx = R.write_fixture(str(tmp_path))
    T.main(_args(fx, "--model", "baseline", "--preprocess", "host", "--image_size", "32", "--batch_size", "12", "--log_interval", "1",
                 "--num_steps", "7"))
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().split("\n")]
    assert lines[0]["data"] == "files" and lines[0]["samples"] == 24 and lines[0]["images"] == 12 and lines[0]["steps_per_epoch"] == 2
    assert lines[0]["preprocess"] == "host" and [l["step"] for l in lines[1:]] == [1, 2]           # (--num_steps is ignored)
    assert all(l["loss"] > 0 for l in lines[1:])

"""Image preprocessing (coattn_preprocess_images; csrc/preprocess.hip) for the tests: the oracle -- the arithmetic that
include/coattn_ext.h states, restated in numpy, never the code under test --, the cases, packers that lay a batch out for the
C-ABI by hand, and a ctypes runner that puts every device buffer of a call at its exact size inside a marker-filled byte arena
with the output pre-filled with a marker."""
import ctypes as C
import functools
import os
import re

import numpy as np
import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
GUARD, GUARD_BYTE = 256, 0xA5                    # bytes on each side of an arena's body, and what they hold
MARK_BITS = 0x7FC0BEEF                           # what the output holds before the call: a NaN no lookup table contains
# (H, W, S) of the contract's eleven checks against Pillow
PIL_SHAPES = ((480, 640, 224), (640, 480, 224), (427, 640, 448), (100, 37, 224), (7, 5, 14), (224, 224, 224), (1, 1, 14),
              (333, 500, 224), (500, 375, 448), (13, 600, 28), (225, 223, 224))


def ext_header():
    from vqa_amd import _lib
    return open(os.path.join(os.path.dirname(_lib.CSRC.rstrip("/")), "..", "include", "coattn_ext.h")).read()


@functools.lru_cache(None)
def constants():
    """{"ROWS": 16, "THREADS": 256, "MAX_S": ..., "MAX_IN": ..., "MAX_TAPS": ...} as include/coattn_ext.h defines them."""
    return {n: int(v) for n, v in re.findall(r"^#define COATTN_PREPROCESS_(\w+) (\d+)", ext_header(), re.M)}


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def coefficients(n_in, S):
    """(lo int64 [S], n int64 [S], K int64 [S, taps]) of an axis of n_in samples resampled to S, in IEEE double."""
    scale = np.float64(n_in) / np.float64(S)
    fs = max(scale, np.float64(1.0))
    support, ss = fs, np.float64(1.0) / fs
    center = (np.arange(S, dtype=np.float64) + 0.5) * scale
    lo = np.maximum(0, np.trunc(center - support + 0.5).astype(np.int64))
    hi = np.minimum(n_in, np.trunc(center + support + 0.5).astype(np.int64))
    n = hi - lo
    taps = int(n.max())
    j = np.arange(taps, dtype=np.float64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs((j + lo[:, None] - center[:, None] + 0.5) * ss))
    w = np.where(j < n[:, None], w, 0.0)
    ww = np.zeros(S, dtype=np.float64)
    for t in range(taps):                                    # left to right (np.sum adds pairwise); a masked tap adds +0.0
        ww = ww + w[:, t]
    k = w / ww[:, None]
    K = np.trunc(0.5 + k * np.float64(1 << 22)).astype(np.int64)
    K = np.where(j < n[:, None], K, 0)
    for a in (lo, n, K):
        a.setflags(write=False)
    return lo, n, K


def _pass(p, n_in, S):
    """uint8 [n_in, ...] -> uint8 [S, ...]: one pass along axis 0."""
    lo, n, K = coefficients(n_in, S)
    acc = np.full((S,) + p.shape[1:], 1 << 21, dtype=np.int64)
    tail = (1,) * (p.ndim - 1)
    for t in range(K.shape[1]):
        idx = np.minimum(lo + t, n_in - 1)                   # (a masked tap has K = 0)
        acc += K[:, t].reshape((S,) + tail) * p[idx].astype(np.int64)
    assert int(acc.max()) < 2 ** 31 and int(acc.min()) >= 0  # the sums fit in int32
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def resize_u8(img, S):
    """uint8 [h, w, 3] -> uint8 [S, S, 3]: the horizontal pass over every source row, a uint8, then the vertical pass."""
    h, w, _ = img.shape
    t = _pass(np.ascontiguousarray(img.transpose(1, 0, 2)), w, S).transpose(1, 0, 2)      # [h, S, 3]
    return _pass(np.ascontiguousarray(t), h, S)


def lut(mean=MEAN, std=STD):
    """float32 [3, 256] by torch's div / sub / div, one channel and one Python scalar at a time."""
    x = torch.arange(256).float().div(255)
    return np.stack([x.sub(m).div(s).numpy() for m, s in zip(mean, std)]).astype(np.float32)


def reference(images, S, table=None):
    """float32 [B, 3, S, S]: resize_u8 and the lookup table."""
    table = lut() if table is None else table
    out = np.empty((len(images), 3, S, S), dtype=np.float32)
    for b, img in enumerate(images):
        u = resize_u8(img, S)
        for c in range(3):
            out[b, c] = table[c][u[:, :, c]]
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def image(h, w, seed=0):
    """A read-only uint8 [h, w, 3]: smooth ramps plus noise, with runs of 0 and 255 (both ends of the clip)."""
    g = np.random.default_rng(9000 + 131 * h + 17 * w + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(yy * 7 + xx * 3) % 256, (yy * 2 + xx * 11 + 40) % 256, (yy * xx + seed) % 256], 2)
    img = np.clip(base + g.integers(-40, 41, size=(h, w, 3)), 0, 255).astype(np.uint8)
    img[g.random((h, w)) < 0.1] = 255
    img[g.random((h, w)) < 0.1] = 0
    img.setflags(write=False)
    return img


def images(sizes, seed=0):
    return [image(h, w, seed + i) for i, (h, w) in enumerate(sizes)]


@functools.lru_cache(None)
def reference_of(sizes, S, seed=0):
    """reference(images(sizes, seed), S), computed once and read-only."""
    out = reference(images(sizes, seed), S)
    out.setflags(write=False)
    return out


# ---- packing by hand ------------------------------------------------------------------------------------------------------------
DESC = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("tab_x", "<i4"), ("tab_y", "<i4"), ("taps_x", "<i4"),
                 ("taps_y", "<i4")])


def table(n_in, S, taps=None):
    """int32 [S, 2 + taps]: lo, n, the taps zero-padded to `taps` (default: the widest row)."""
    lo, n, K = coefficients(n_in, S)
    taps = K.shape[1] if taps is None else taps
    tab = np.zeros((S, 2 + taps), dtype=np.int32)
    tab[:, 0], tab[:, 1], tab[:, 2:2 + K.shape[1]] = lo, n, K
    return tab


def pack(imgs, S, align=16, lead=0, extra_taps=0):
    """(pixels uint8 [n], desc DESC [B], coef int32 [m]) for the C-ABI: images `align` bytes apart at least (align = 1: back to
    back, so that image and row starts take every residue), `lead` unused bytes first, every table `extra_taps` wider than it
    must be.  One table per distinct (size, axis use)."""
    desc = np.zeros(len(imgs), dtype=DESC)
    tabs, coef = {}, []
    n_coef = 0
    chunks, pos = [np.full(lead, 0x5A, dtype=np.uint8)], lead
    for i, img in enumerate(imgs):
        h, w, _ = img.shape
        for n_in in (w, h):
            if n_in not in tabs:
                t = table(n_in, S, coefficients(n_in, S)[2].shape[1] + extra_taps)
                tabs[n_in] = (n_coef, t.shape[1] - 2)
                coef.append(t.reshape(-1))
                n_coef += t.size
        pad = (-pos) % align
        chunks.append(np.full(pad, 0x5A, dtype=np.uint8))
        pos += pad
        desc[i] = (pos, h, w, tabs[w][0], tabs[h][0], tabs[w][1], tabs[h][1])
        chunks.append(np.asarray(img).reshape(-1))
        pos += 3 * h * w
    return np.concatenate(chunks), desc, np.concatenate(coef)


# ---- the runner ---------------------------------------------------------------------------------------------------------------
class ByteArena:
    """A device buffer of exactly `n` bytes (its start 16-byte aligned) with GUARD marker bytes on both sides."""

    def __init__(self, n, data=None):
        self.n = int(n)
        lead = GUARD
        self.flat = torch.full((self.n + 2 * GUARD + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda:0")
        lead += (-(self.flat.data_ptr() + lead)) % 16
        self.lead = lead
        self.body = self.flat[lead:lead + self.n]
        if data is not None:
            self.body.copy_(torch.from_numpy(np.ascontiguousarray(data).view(np.uint8).reshape(-1)))
        self.before = self.flat.clone()

    def check(self, what, body_unchanged=True):
        after = self.flat
        assert bool((after[:self.lead] == GUARD_BYTE).all()), "%s: a byte in front of the buffer was overwritten" % what
        assert bool((after[self.lead + self.n:] == GUARD_BYTE).all()), "%s: a byte behind the buffer was overwritten" % what
        if body_unchanged:
            assert bool((after == self.before).all()), "%s: an input buffer was written" % what


LAYOUTS = ("nchw", "nhwc", "view")


def out_geometry(B, S, layout):
    """(floats of the buffer, element offset of the view, (sB, sC, sH, sW)).  view: a [B, 3, S, S] window into a
    [B, 4, S + 3, S + 5] buffer, starting at channel 1, row 2, column 3."""
    if layout == "nchw":
        return B * 3 * S * S, 0, (3 * S * S, S * S, S, 1)
    if layout == "nhwc":
        return B * 3 * S * S, 0, (3 * S * S, 1, 3 * S, 3)
    Hb, Wb = S + 3, S + 5
    return B * 4 * Hb * Wb, Hb * Wb + 2 * Wb + 3, (4 * Hb * Wb, Hb * Wb, Wb, 1)


def run(pixels, desc, coef, S, max_h, max_w, layout="nchw", table=None, bad=True, bad_start=0, expect_rc=0, pixel_bytes=None,
        coef_count=None):
    """One coattn_preprocess_images straight through the C-ABI on host arrays.  Every buffer is an arena of its exact size; the
    output buffer starts as MARK_BITS words.  Afterwards: the margins of every arena, the inputs unchanged, and every cell of
    the output buffer outside the [B, 3, S, S] view still the marker.  Returns the output's bit patterns int32 [B, 3, S, S],
    the whole output buffer's words, the counter and the return code."""
    from vqa_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B = len(desc)
    table = lut() if table is None else table
    n_out, first, strides = out_geometry(B, S, layout)
    ar = {"pixels": ByteArena(pixels.size, pixels), "desc": ByteArena(desc.nbytes, desc), "coef": ByteArena(coef.nbytes, coef),
          "lut": ByteArena(table.nbytes, table)}
    out = ByteArena(4 * n_out)
    out.body.view(torch.int32).fill_(MARK_BITS)
    counter = ByteArena(4, np.array([bad_start], dtype=np.int32))
    body = out.body.view(torch.float32)
    view = torch.as_strided(body, (B, 3, S, S), strides, body.storage_offset() + first)      # (the offset counts from the storage)
    assert view.data_ptr() == body.data_ptr() + 4 * first
    call = _lib.bind("coattn_preprocess_images", pixels=ar["pixels"].body, pixel_bytes=pixels.size if pixel_bytes is None else
                     pixel_bytes, desc=ar["desc"].body, coef=ar["coef"].body, coef_count=coef.size if coef_count is None else
                     coef_count, lut=ar["lut"].body, out=view, sB=strides[0], sC=strides[1], sH=strides[2], sW=strides[3],
                     bad_images=counter.body if bad else None, B=B, S=S, max_h=max_h, max_w=max_w,
                     stream=torch.cuda.current_stream(dev).cuda_stream)
    rc = call.code()
    torch.cuda.synchronize()
    err = lib.coattn_last_error().decode()
    assert rc == expect_rc, (rc, err)
    for k, a in ar.items():
        a.check("preprocess_images %s" % k)
    out.check("preprocess_images out", body_unchanged=False)
    counter.check("preprocess_images bad_images", body_unchanged=False)
    words = out.body.view(torch.int32).clone()
    bits = torch.as_strided(words, (B, 3, S, S), strides, first).cpu().numpy().copy()
    torch.as_strided(words, (B, 3, S, S), strides, first).fill_(MARK_BITS)
    assert bool((words == MARK_BITS).all()), "preprocess_images: a cell of the output buffer outside the view was written"
    return dict(rc=rc, err=err, bits=bits, words=out.body.view(torch.int32).cpu().numpy(),
                bad=int(counter.body.view(torch.int32).cpu()[0]))


def run_images(imgs, S, layout="nchw", align=16, lead=0, extra_taps=0, **kw):
    pixels, desc, coef = pack(imgs, S, align=align, lead=lead, extra_taps=extra_taps)
    max_h, max_w = kw.pop("max_h", max(i.shape[0] for i in imgs)), kw.pop("max_w", max(i.shape[1] for i in imgs))
    return run(pixels, desc, coef, S, max_h, max_w, layout=layout, **kw)


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def diff(got, want):
    """A short account of where two arrays of bit patterns differ (for an assertion message)."""
    ne = np.argwhere(got != want)
    return "%d of %d words differ; first at %s: got %s, want %s" % (
        len(ne), got.size, ne[:3].tolist(), [hex(int(got[tuple(i)]) & 0xFFFFFFFF) for i in ne[:3]],
        [hex(int(want[tuple(i)]) & 0xFFFFFFFF) for i in ne[:3]])


# ---- a dataset fixture on disk ----------------------------------------------------------------------------------------------------
QUESTIONS = ("What color is the cat?", "Is this a dog, or a cat", "How many people's hats are there?", "what is on the table",
             "Is the man sleeping next to a cat on a bed.", "Where is the bus going")
ANSWERS = ("yes", "no", "2", "red", "cat", "yes", "table", "no", "yes", "blue")


def write_fixture(root, n_images=12, n_lines=24, sizes=((37, 23), (40, 64), (64, 48), (5, 7)), K=4, seed=0):
    """A dataset in the reference's file formats under `root`: images/img_XX.npy (uint8 [h, w, 3]), data.txt of
    `img_name \\t question \\t answer` lines (images recur: 2 lines each, not adjacent), vocab.pkl (the five keys of the
    reference's save_vocab, built by the package's build_vocab).  Returns a dict of paths and the parsed lines."""
    import pickle
    from vqa_amd import data as D
    img_dir = os.path.join(root, "images")
    os.makedirs(img_dir, exist_ok=True)
    names = []
    for i in range(n_images):
        h, w = sizes[i % len(sizes)]
        names.append("img_%02d.npy" % i)
        np.save(os.path.join(img_dir, names[-1]), image(h, w, seed + i))
    lines = []
    for j in range(n_lines):
        lines.append((names[(j * 5) % n_images], QUESTIONS[j % len(QUESTIONS)], ANSWERS[(j * 3) % len(ANSWERS)]))
    data_file = os.path.join(root, "data.txt")
    with open(data_file, "w") as fh:
        fh.write("\n".join("\t".join(l) for l in lines) + "\n")
    vocab = D.build_vocab(data_file, 1, K)
    vocab_file = os.path.join(root, "vocab.pkl")
    with open(vocab_file, "wb") as fh:
        pickle.dump(vocab, fh)
    return dict(img_dir=img_dir, data_file=data_file, vocab_file=vocab_file, lines=lines, names=names, vocab=vocab)

"""Record tests/golden/preprocess_pil.npz: a handful of small uint8 images and the bytes Pillow's
``Image.resize((S, S), Image.BILINEAR)`` gives for them, so that the contract of include/coattn_ext.h (tests/_preprocess.py
restates it) is held against Pillow's own output where Pillow is not installed.

    python tools/make_golden_preprocess.py        # needs Pillow; rewrites the file (inputs are drawn from fixed seeds)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "preprocess_pil.npz")
# (h, w, S): downscale, upscale, identity on one axis, one-pixel sources, a ratio above 4
CASES = ((48, 64, 14), (64, 48, 28), (37, 23, 14), (5, 7, 14), (28, 28, 28), (1, 1, 14), (9, 28, 28), (60, 3, 14))


def source(h, w, seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = np.stack([(yy * 5 + xx * 3) % 256, (yy * 11 + xx * 2 + 90) % 256, (yy * xx) % 256], 2)
    img = np.clip(ramp + g.integers(-50, 51, size=(h, w, 3)), 0, 255).astype(np.uint8)
    img[g.random((h, w)) < 0.08] = 255
    img[g.random((h, w)) < 0.08] = 0
    return img


def main():
    import PIL
    from PIL import Image
    arrays = {"shapes": np.array(CASES, dtype=np.int32)}
    for i, (h, w, S) in enumerate(CASES):
        img = source(h, w, 4200 + i)
        arrays["in_%d" % i] = img
        arrays["out_%d" % i] = np.asarray(Image.fromarray(img).resize((S, S), Image.BILINEAR))
    np.savez_compressed(OUT, **arrays)
    print("wrote %s (%d bytes) with Pillow %s" % (OUT, os.path.getsize(OUT), PIL.__version__))


if __name__ == "__main__":
    sys.exit(main())

"""Writes tests/golden/image_io.safetensors: seeded random uint8 images (as windows of two seeded arrays) and the bytes Pillow's resize(..., BILINEAR) gives for
them at torchvision's Resize(R) size (shorter side -> R, longer side truncated) - what the byte-image kernels must reproduce.

    python tests/golden/make_golden_image_io.py

Needs Pillow (its version goes into the metadata) and safetensors; no GPU, no library build."""
import os

import numpy as np
import PIL
from PIL import Image
from safetensors.numpy import save_file

# (height, width, R): upscale with clamped edges; non-integer downscale, portrait; more than 8x downscale (17+ taps); identity; exact 2x
CASES = [(37, 53, 64), (150, 100, 32), (131, 197, 16), (64, 64, 64), (128, 128, 64)]


def resized_size(h: int, w: int, R: int):
    """torchvision Resize(R): (rh, rw)"""
    return (int(R * h / w), R) if w <= h else (R, int(R * w / h))


# The five inputs are windows of two seeded random arrays (`base0` 131 x 197, `base1` 150 x 100): (base, top, left) per case.  Stored
# one by one they would take 189 KB before any result; as windows the whole fixture stays under 200 KB.
WINDOWS = [(0, 80, 10), (1, 0, 0), (0, 0, 0), (0, 50, 100), (0, 3, 60)]


def main():
    rng = np.random.default_rng(20240607)
    bases = [rng.integers(0, 256, size=(131, 197, 3), dtype=np.uint8), rng.integers(0, 256, size=(150, 100, 3), dtype=np.uint8)]
    out = {"base0": bases[0], "base1": bases[1]}
    for i, ((h, w, R), (b, top, left)) in enumerate(zip(CASES, WINDOWS)):
        a = np.ascontiguousarray(bases[b][top:top + h, left:left + w])
        assert a.shape == (h, w, 3)
        rh, rw = resized_size(h, w, R)
        out[f"pil{i}"] = np.asarray(Image.fromarray(a).resize((rw, rh), Image.BILINEAR))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "image_io.safetensors")
    save_file(out, path, metadata={"pillow": PIL.__version__, "cases": repr(CASES), "windows": repr(WINDOWS)})
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()

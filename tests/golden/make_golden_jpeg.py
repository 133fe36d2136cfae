"""Writes tests/golden/jpeg.safetensors (data only): for every case of tests/jpeg_ref.py the JPEG file Pillow's encoder writes (`jpg{i}`)
and the pixels Pillow's Image.open(..).convert("RGB") decodes from it (`rgb{i}`), and the bytes of the reference's
docs/test/source/subject/1.jpg (`photo`) with the SHA-256 of its decoded pixels in the metadata instead of the 786 KB raster - what
csrc/jpeg.h and csrc/jpeg.hip are held against.

    python tests/golden/make_golden_jpeg.py --reference /path/to/the/reference/checkout

Needs Pillow (its version and libjpeg-turbo's go into the metadata) and safetensors; no GPU, no library build."""
import argparse
import os
import sys

import numpy as np
import PIL
from PIL import features
from safetensors.numpy import save_file

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import jpeg_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds docs/test)")
    a = ap.parse_args()
    out, names = {}, []
    for i, (name, w, h, sampling, quality, kind, restart, optimize) in enumerate(R.cases()):
        raw = R.encode(R.content(w, h, kind, 1000 + i, sampling == "gray"), sampling, quality, restart, optimize)
        rgb = R.pillow_rgb(raw)
        assert rgb.shape == (h, w, 3) and rgb.dtype == np.uint8
        out[f"jpg{i}"] = np.frombuffer(raw, dtype=np.uint8).copy()
        out[f"rgb{i}"] = np.ascontiguousarray(rgb)
        names.append(name)
    with open(os.path.join(a.reference, *R.PHOTO.split("/")), "rb") as f:
        photo = f.read()
    rgb = R.pillow_rgb(photo)
    assert rgb.shape == (512, 512, 3) and len(photo) == 11050
    out["photo"] = np.frombuffer(photo, dtype=np.uint8).copy()
    save_file(out, R.GOLDEN, metadata={"cases": repr(names), "pillow": PIL.__version__, "libjpeg_turbo": str(features.version("libjpeg_turbo") or features.version("jpg")),
                                       "photo": R.PHOTO, "photo_sha256": R.sha256(rgb)})
    size = os.path.getsize(R.GOLDEN)
    assert size < 200 * 1024, size
    print(R.GOLDEN, size, "bytes, Pillow", PIL.__version__, "libjpeg-turbo", features.version("libjpeg_turbo"))


if __name__ == "__main__":
    main()

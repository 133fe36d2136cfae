"""Writes tests/golden/ref_pose.safetensors (data only): the key points of the reference's three docs/test pose files, the pose
renderings its own tool chain made from exactly those points (the JPEGs next to them, decoded to uint8 512 x 512 x 3), and the bytes
Pillow's resize(..., LANCZOS) gives for a few small seeded images - what csrc/pose.hip and the Lanczos filter of csrc/image_io.hip are
held against.

    python tests/golden/make_golden_ref_pose.py --reference /path/to/the/reference/checkout

The decoded renderings are 2.4 MB, nearly all of it black; they are stored deflated (zlib, as uint8 tensors `jpg{i}_z`; tests/pose_ref.py
inflates them), which keeps the file under 0.5 MB.  Needs Pillow (its version goes into the metadata) and safetensors; no GPU, no
library build."""
import argparse
import json
import os
import sys
import zlib

import numpy as np
import PIL
from PIL import Image
from safetensors.numpy import save_file

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.pose_ref import GOLDEN, LANCZOS_CASES, POSES, keypoints_array  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds docs/test)")
    a = ap.parse_args()
    out, scores = {}, []
    for i, name in enumerate(POSES):
        base = os.path.join(a.reference, "docs", "test", name)
        with open(base + ".json") as f:
            pose = json.load(f)
        out[f"kp{i}"] = keypoints_array(pose["keypoints"])
        scores.append((pose["total_score"], pose["total_parts"]))
        img = np.asarray(Image.open(base + ".jpg").convert("RGB"))
        assert img.shape == (512, 512, 3) and img.dtype == np.uint8
        out[f"jpg{i}_z"] = np.frombuffer(zlib.compress(img.tobytes(), 9), dtype=np.uint8).copy()
    rng = np.random.default_rng(20240611)
    for i, (h, w, nh, nw) in enumerate(LANCZOS_CASES):
        src = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        out[f"lz_in{i}"] = src
        out[f"lz_out{i}"] = np.asarray(Image.fromarray(src).resize((nw, nh), Image.LANCZOS))
    save_file(out, GOLDEN, metadata={"pillow": PIL.__version__, "lanczos_cases": repr(LANCZOS_CASES), "poses": repr(list(POSES)),
                                     "scores": repr(scores), "jpg_shape": repr((512, 512, 3))})
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()

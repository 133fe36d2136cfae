"""Shared by tests/test_jpeg_encode_cpu.py, tests/test_jpeg_encode_gpu.py and tests/golden/make_golden_jpeg_encode.py: the list of
encoder cases and the fixture (tests/golden/jpeg_encode.safetensors: the input arrays and the bytes Pillow's Image.save wrote for them).
Sizes, content and Pillow's encoder call are tests/jpeg_ref.py's."""
import ast
import os

import numpy as np

from tests import jpeg_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_encode.safetensors")
# (width, height): 4:2:0 sizes whose last chroma block row is partly padding below an EVEN number of source rows - where padding the
# rows at full resolution all the way to whole blocks (instead of to a multiple of 2, then padding the downsampled plane) goes wrong
PADDING_ORDER_SIZES = [(40, 33), (33, 40), (24, 33), (33, 24), (50, 70), (70, 50)]
SUBSAMPLING = {"444": 0, "422": 1, "420": 2, "gray": 0}
BIG = "200x120_420_q90"                                   # 624 blocks in a single interval: the prefix sums cross their chunks


def cases():
    """[(name, width, height, sampling, quality, content, restart, seed)]; quality None: Pillow's defaults, no keyword at all.  Every
    size of jpeg_ref.SIZES at every sampling twice (quality 30, and quality 100 with a restart interval of one MCU; noise and smooth
    content alternate), the padding-order sizes, the quality extremes on 17 x 23, two images of extreme blocks (the largest categories),
    and 200 x 120 noise without and with a restart interval of 3 (more than 8 intervals: the marker number wraps)."""
    out = []
    for k, ((w, h), s) in enumerate((sz, s) for sz in R.SIZES for s in R.SAMPLINGS):
        a, b = ("noise", "smooth") if k % 2 == 0 else ("smooth", "noise")
        out.append((f"{w}x{h}_{s}_q30", w, h, s, 30, a, 0, 2000 + 2 * k))
        out.append((f"{w}x{h}_{s}_q100_rst", w, h, s, 100, b, 1, 2001 + 2 * k))
    for k, (w, h) in enumerate(PADDING_ORDER_SIZES):
        out.append((f"{w}x{h}_420_q90", w, h, "420", 90, "noise" if k % 2 == 0 else "smooth", 0, 2200 + k))
    out.append(("17x23_420_q1", 17, 23, "420", 1, "noise", 0, 2300))
    out.append(("17x23_420_q10", 17, 23, "420", 10, "noise", 0, 2301))
    out.append(("17x23_defaults", 17, 23, "420", None, "noise", 0, 2302))
    out.append(("17x23_420_q95", 17, 23, "420", 95, "photo", 0, 2303))
    out.append(("32x24_gray_q100_extreme", 32, 24, "gray", 100, "extreme", 0, 2304))
    out.append(("32x24_444_q100_extreme", 32, 24, "444", 100, "extreme", 2, 2305))
    out.append((BIG, 200, 120, "420", 90, "noise", 0, 2400))
    out.append((BIG + "_rst3", 200, 120, "420", 90, "noise", 3, 2400))
    return out


def content(w: int, h: int, kind: str, seed: int, gray: bool) -> np.ndarray:
    """jpeg_ref.content, and "extreme": 8 x 8 blocks that alternate between black and white (DC differences of category 11 at
    quality 100), every third one split into a black and a white half (AC values of category 10)"""
    if kind != "extreme":
        return R.content(w, h, kind, seed, gray)
    a = np.zeros((h, w), dtype=np.uint8)
    for by in range(0, h, 8):
        for bx in range(0, w, 8):
            n = by // 8 * (w // 8) + bx // 8
            a[by:by + 8, bx:bx + 8] = 255 * (n % 2)
            if n % 3 == 2:
                a[by:by + 8, bx + 4:bx + 8] = 255 - 255 * (n % 2)
    return a if gray else np.ascontiguousarray(np.stack([a, a, a], axis=2))


def pillow_encode(a: np.ndarray, sampling: str, quality, restart: int) -> bytes:
    """Pillow's encoder (needs Pillow); quality None: no keyword at all"""
    if quality is None:
        import io
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG")
        return buf.getvalue()
    return R.encode(a, sampling, quality, restart)


def keywords(sampling: str, quality, restart: int) -> dict:
    """the same call in edgestyle_amd.jpeg's spelling"""
    if quality is None:
        return {}
    kw = dict(quality=quality, restart_marker_blocks=restart)
    if sampling != "gray":
        kw["subsampling"] = SUBSAMPLING[sampling]
    return kw


_fixture = None


def fixture():
    """{"cases": {name: (input array, Pillow's bytes)}, "photo_jpg": Pillow's default file of the pixels jpeg_ref's photo decodes to,
    "pillow", "libjpeg_turbo", "max_ac_category", "max_dc_category"} (read once, never changed)"""
    global _fixture
    if _fixture is None:
        from safetensors import safe_open
        with safe_open(GOLDEN, framework="np") as f:
            meta = f.metadata()
            names = ast.literal_eval(meta["cases"])
            assert names == [c[0] for c in cases()]
            got = {}
            for i, n in enumerate(names):
                src = i if f"in{i}" in f.keys() else names.index(BIG)          # the two 200 x 120 cases share their input
                got[n] = (f.get_tensor(f"in{src}"), f.get_tensor(f"jpg{i}").tobytes())
            _fixture = dict(cases=got, photo_jpg=f.get_tensor("photo_jpg").tobytes(), pillow=meta["pillow"], libjpeg_turbo=meta["libjpeg_turbo"],
                            max_ac_category=int(meta["max_ac_category"]), max_dc_category=int(meta["max_dc_category"]))
    return _fixture


def photo_pixels() -> np.ndarray:
    """the 512 x 512 pixels the decoder fixture's photo decodes to (its hash is pinned there)"""
    from edgestyle_amd import jpeg as J
    fx = R.fixture()
    rgb = J.decode_host(fx["photo"])
    assert R.sha256(rgb) == fx["photo_sha256"]
    return rgb

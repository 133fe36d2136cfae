"""Shared by tests/test_jpeg_cpu.py, tests/test_jpeg_gpu.py, tests/golden/make_golden_jpeg.py and tools/jpeg_decode_bench.py: the list of
cases, the fixture (JPEG byte strings written by Pillow with the pixels Pillow decodes from them, and one real photo with the hash of its
pixels), the byte edits that make the files the decoder must refuse, and the truncation / corruption sweep."""
import ast
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.safetensors")
# (width, height): 1x1; chroma width <= 2 (replication); chroma width 3 (the first fancy case); whole MCUs; partial MCUs on both axes
SIZES = [(1, 1), (3, 4), (5, 3), (2, 6), (8, 8), (16, 16), (9, 5), (17, 23), (23, 37), (33, 18)]
SAMPLINGS = ["444", "422", "420", "gray"]
PHOTO = "docs/test/source/subject/1.jpg"                  # of the reference: 512 x 512, 4:2:0, 11,050 bytes


def cases():
    """[(name, width, height, sampling, quality, content, restart, optimize)]: every size at every sampling twice - quality 30 without
    and quality 100 (all-ones tables: large coefficients, clamping) with restart markers, noise and smooth content alternating between
    the two - then the crossed combinations once, one file with optimised Huffman tables and the 60 x 45 photo of the crop test"""
    out = []
    for k, ((w, h), s) in enumerate((sz, s) for sz in SIZES for s in SAMPLINGS):
        a, b = ("noise", "smooth") if k % 2 == 0 else ("smooth", "noise")
        out.append((f"{w}x{h}_{s}_q30", w, h, s, 30, a, 0, False))
        out.append((f"{w}x{h}_{s}_q100_rst", w, h, s, 100, b, 1, False))
    out.append(("33x18_420_q30_rst", 33, 18, "420", 30, "noise", 1, False))
    out.append(("23x37_422_q100", 23, 37, "422", 100, "noise", 0, False))
    out.append(("17x23_420_q75_opt", 17, 23, "420", 75, "noise", 0, True))
    out.append(("60x45_420_q90", 60, 45, "420", 90, "photo", 0, False))
    return out


DQT16_SOURCE = "17x23_420_q30"                            # the file whose DQT segment the tests rewrite to 16-bit precision
SWEEP_SOURCE = "9x5_420_q30"                              # the file of the truncation / corruption sweep (under 700 bytes)


def content(w: int, h: int, kind: str, seed: int, gray: bool) -> np.ndarray:
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 7 % 256], axis=2)
    if kind == "noise":
        a = g.integers(0, 256, size=(h, w, 3))
    elif kind == "smooth":
        a = smooth
    else:                                                 # photo-like: gradients plus mild noise
        a = np.clip(smooth + g.integers(-12, 13, size=(h, w, 3)), 0, 255)
    a = a.astype(np.uint8)
    return np.ascontiguousarray(a[:, :, 0]) if gray else a


def encode(a: np.ndarray, sampling: str, quality: int, restart: int = 0, optimize: bool = False, progressive: bool = False) -> bytes:
    """Pillow's encoder (needs Pillow)"""
    import io
    from PIL import Image
    kw = dict(quality=quality, optimize=optimize, progressive=progressive)
    if sampling != "gray":
        kw["subsampling"] = {"444": 0, "422": 1, "420": 2}[sampling]
    if restart:
        kw["restart_marker_blocks"] = restart
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_rgb(raw: bytes) -> np.ndarray:
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"))


def have_pillow() -> bool:
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


_fixture = None


def fixture():
    """{"cases": {name: (jpeg bytes, Pillow's uint8 [H, W, 3])}, "photo": bytes, "photo_sha256": hex, "pillow", "libjpeg_turbo"} (read
    once, never changed)"""
    global _fixture
    if _fixture is None:
        from safetensors import safe_open
        with safe_open(GOLDEN, framework="np") as f:
            meta = f.metadata()
            names = ast.literal_eval(meta["cases"])
            assert names == [c[0] for c in cases()]
            _fixture = dict(cases={n: (f.get_tensor(f"jpg{i}").tobytes(), f.get_tensor(f"rgb{i}")) for i, n in enumerate(names)},
                            photo=f.get_tensor("photo").tobytes(), photo_sha256=meta["photo_sha256"], pillow=meta["pillow"],
                            libjpeg_turbo=meta["libjpeg_turbo"])
    return _fixture


def sha256(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- byte edits ------------------------------------------------------------------------------------------------------------------
def segments(raw: bytes):
    """[(marker, offset of the FF, length field)] of the header segments up to and including SOS"""
    out, pos = [], 2
    while pos + 4 <= len(raw):
        assert raw[pos] == 0xFF
        m, n = raw[pos + 1], raw[pos + 2] << 8 | raw[pos + 3]
        out.append((m, pos, n))
        if m == 0xDA:
            break
        pos += 2 + n
    return out


def find(raw: bytes, marker: int):
    return [(p, n) for m, p, n in segments(raw) if m == marker]


def patch(raw: bytes, pos: int, new: bytes) -> bytes:
    return raw[:pos] + bytes(new) + raw[pos + len(new):]


def dqt_to_16_bit(raw: bytes) -> bytes:
    """every DQT segment rewritten with 16-bit entries (Pq = 1): the same tables, the same pixels"""
    out, pos = bytearray(raw[:2]), 2
    for m, p, n in segments(raw):
        seg = raw[p:p + 2 + n]
        if m == 0xDB:
            body, new = seg[4:], bytearray()
            while body:
                assert body[0] >> 4 == 0
                new.append(0x10 | body[0])
                for v in body[1:65]:
                    new += bytes((0, v))
                body = body[65:]
            seg = b"\xff\xdb" + (len(new) + 2).to_bytes(2, "big") + bytes(new)
        out += seg
        pos = p + 2 + n
    return bytes(out) + raw[pos:]


def without_segment(raw: bytes, marker: int) -> bytes:
    for m, p, n in segments(raw):
        if m == marker:
            return raw[:p] + raw[p + 2 + n:]
    raise AssertionError(hex(marker))


def with_segment_before_sof(raw: bytes, seg: bytes) -> bytes:
    p = [p for m, p, n in segments(raw) if m in (0xC0, 0xC1)][0]
    return raw[:p] + seg + raw[p:]


def sof_offset(raw: bytes) -> int:
    return [p for m, p, n in segments(raw) if m in (0xC0, 0xC1, 0xC2)][0]


def sweep(raw: bytes, first: int = 700):
    """every proper prefix, then each of the first `first` bytes set to 0xFF and to 0x00"""
    for n in range(len(raw)):
        yield raw[:n]
    for i in range(min(first, len(raw))):
        for v in (0xFF, 0x00):
            if raw[i] != v:
                yield raw[:i] + bytes((v,)) + raw[i + 1:]

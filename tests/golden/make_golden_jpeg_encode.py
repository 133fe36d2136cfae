"""Writes tests/golden/jpeg_encode.safetensors (data only): for every case of tests/jpeg_encode_ref.py the input array (`in{i}`) and the
bytes Pillow's Image.fromarray(a).save(f, "JPEG", ...) wrote for it (`jpg{i}`), and Pillow's default file of the pixels the decoder
fixture's 512 x 512 photo decodes to (`photo_jpg`; the pixels themselves are not stored, tests/golden/jpeg.safetensors pins their hash) -
what csrc/jpeg.h's encoder and csrc/jpeg_encode.hip are held against.

    python tests/golden/make_golden_jpeg_encode.py

Before anything is written the case set is checked, on Pillow's output alone, to hold what an entropy coder can get wrong: a stuffed
byte, a run of 16 zeros, a block without EOB, the largest categories, a negative DC difference, dummy blocks on both edges.  Needs
Pillow (its version and libjpeg-turbo's go into the metadata), safetensors and the built library (its Huffman DEcoder reads Pillow's
coefficients); no GPU."""
import os
import sys

import numpy as np
import PIL
from PIL import features
from safetensors.numpy import save_file

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from edgestyle_amd import jpeg as J  # noqa: E402
from tests import jpeg_encode_ref as E, jpeg_ref as R  # noqa: E402

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])


def category(v: int) -> int:
    return int(abs(int(v))).bit_length()


def scan_data(raw: bytes) -> bytes:
    m, p, n = R.segments(raw)[-1]
    assert m == 0xDA
    return raw[p + 2 + n:-2]


def main():
    out, names = {}, []
    seen = dict(stuffed=False, run16=False, no_eob=False, negative_dc=False, dummy_both=False)
    max_ac = max_dc = 0
    cases = E.cases()
    for i, (name, w, h, sampling, quality, kind, restart, seed) in enumerate(cases):
        a = E.content(w, h, kind, seed, sampling == "gray")
        raw = E.pillow_encode(a, sampling, quality, restart)
        if name != E.BIG + "_rst3":
            out[f"in{i}"] = a
        else:
            assert np.array_equal(a, out[f"in{names.index(E.BIG)}"])
        out[f"jpg{i}"] = np.frombuffer(raw, dtype=np.uint8).copy()
        names.append(name)
        # ---- what the case holds, read from Pillow's file alone
        info, coeffs, _ = J.entropy_decode(raw)
        assert (info.width, info.height) == (w, h) and info.restart_interval == restart, name
        data = scan_data(raw)
        seen["stuffed"] |= b"\xff\x00" in data
        blocks = coeffs.reshape(-1, 64)[:, ZIGZAG]
        for b in blocks:
            nz = np.flatnonzero(b[1:]) + 1
            if nz.size and int(np.diff(np.concatenate([[0], nz])).max()) > 16:
                seen["run16"] = True
        seen["no_eob"] |= bool((blocks[:, 63] != 0).any())
        max_ac = max(max_ac, max(category(v) for v in (blocks[:, 1:].max(), blocks[:, 1:].min())))
        if info.components == 1 or info.hmax == 1:             # the scan visits a component's blocks in raster order
            at = 0
            for c in range(info.components):
                n = info.blocks_w[c] * info.blocks_h[c]
                dc = blocks[at:at + n, 0].astype(np.int64)
                at += n
                if restart == 0:
                    d = np.diff(np.concatenate([[0], dc]))
                    max_dc = max(max_dc, max(category(v) for v in d))
                    seen["negative_dc"] |= bool((d < 0).any())
        real_w, real_h = -(-w // 8), -(-h // 8)
        if info.components == 3 and info.blocks_w[0] > real_w and info.blocks_h[0] > real_h:
            seen["dummy_both"] = True
    assert all(seen.values()), seen
    # quality 100 leaves the DCT unquantised: a black block next to a white one is a DC difference of category 11, a block split into a
    # black and a white half an AC value of category 10 - the largest a baseline file of 8-bit samples holds
    assert max_ac == 10 and max_dc == 11, (max_ac, max_dc)
    photo = E.photo_pixels()
    out["photo_jpg"] = np.frombuffer(E.pillow_encode(photo, "420", None, 0), dtype=np.uint8).copy()
    save_file(out, E.GOLDEN, metadata={"cases": repr(names), "pillow": PIL.__version__,
                                       "libjpeg_turbo": str(features.version("libjpeg_turbo") or features.version("jpg")),
                                       "max_ac_category": str(max_ac), "max_dc_category": str(max_dc), "holds": repr(sorted(seen))})
    size = os.path.getsize(E.GOLDEN)
    assert size < 400 * 1024, size
    print(E.GOLDEN, size, "bytes, Pillow", PIL.__version__, "libjpeg-turbo", features.version("libjpeg_turbo"), "categories", max_ac, max_dc)


if __name__ == "__main__":
    main()

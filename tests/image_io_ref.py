"""Shared by tests/test_image_io_cpu.py and tests/test_image_io_gpu.py: the fixture, torchvision's size rules through
es_image_fit, a numpy integer resize built from es_image_resize_coeffs (the host build of the code the kernels run), live Pillow."""
import ctypes as C
import os

import numpy as np

from edgestyle_amd import lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_io.safetensors")
CASES = [(37, 53, 64), (150, 100, 32), (131, 197, 16), (64, 64, 64), (128, 128, 64)]      # (H, W, R) of the fixture, in order
_fixture = None


def fixture():
    """[(input uint8 [H,W,3], Pillow's resize bytes [rh,rw,3], R)] and the Pillow version that wrote them (read once)"""
    global _fixture
    if _fixture is None:
        from safetensors import safe_open
        import ast
        with safe_open(GOLDEN, framework="np") as f:
            meta = f.metadata()
            assert ast.literal_eval(meta["cases"]) == CASES
            bases = [f.get_tensor("base0"), f.get_tensor("base1")]
            cases = []
            for i, ((h, w, r), (b, top, left)) in enumerate(zip(CASES, ast.literal_eval(meta["windows"]))):   # inputs: windows of the bases
                cases.append((np.ascontiguousarray(bases[b][top:top + h, left:left + w]), f.get_tensor(f"pil{i}"), r))
        _fixture = (cases, meta["pillow"])
    return _fixture


def have_pillow() -> bool:
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


def fit(h: int, w: int, R: int):
    out = (C.c_int32 * 4)()
    L.check(L.load().es_image_fit(h, w, R, out), "es_image_fit")
    return tuple(out)                                   # rh, rw, top, left


def pillow_resize(a: np.ndarray, rh: int, rw: int) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((rw, rh), Image.BILINEAR))


def crop(a: np.ndarray, R: int, top: int, left: int) -> np.ndarray:
    return np.ascontiguousarray(a[top:top + R, left:left + R])


def coeffs(n_in: int, n_out: int):
    lib = L.load()
    cap = lib.es_image_resize_coeffs(n_in, n_out, None, None, None, 0)
    assert cap >= 1, lib.es_last_error()
    xmin, nt, k = (C.c_int32 * n_out)(), (C.c_int32 * n_out)(), (C.c_int32 * (n_out * cap))()
    assert lib.es_image_resize_coeffs(n_in, n_out, xmin, nt, k, cap) == cap
    return np.array(xmin), np.array(nt), np.array(k).reshape(n_out, cap)


def resize_axis(a: np.ndarray, n_out: int, axis: int) -> np.ndarray:
    """one pass: out = clip8(((1 << 21) + sum k * src) >> 22); a pass that does not change the size is skipped"""
    if a.shape[axis] == n_out:
        return a
    xmin, nt, k = coeffs(a.shape[axis], n_out)
    src = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], dtype=np.uint8)
    for i in range(n_out):
        acc = (1 << 21) + np.tensordot(k[i, :nt[i]].astype(np.int64), src[xmin[i]:xmin[i] + nt[i]], axes=(0, 0))
        assert acc.max() < 2 ** 31 and acc.min() >= -2 ** 31        # the kernels accumulate in 32 bits
        out[i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def integer_resize(a: np.ndarray, rh: int, rw: int) -> np.ndarray:
    """horizontal pass, then vertical pass, a uint8 image after each (Pillow's order)"""
    return resize_axis(resize_axis(a, rw, 1), rh, 0)


def to_float_host(u8_hwc: np.ndarray, normalize: bool):
    """cli.load_image's conversion of the bytes: ToTensor (-> Normalize(.5, .5)), [H,W,3] uint8 -> torch fp32 [1,3,H,W]"""
    import torch
    x = torch.from_numpy(np.asarray(u8_hwc, dtype=np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)
    return (x - 0.5) / 0.5 if normalize else x

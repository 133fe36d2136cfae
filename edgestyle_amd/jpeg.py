"""Baseline JPEG files to RGB bytes (csrc/jpeg.h, csrc/jpeg.hip): what Pillow's Image.open(..).convert("RGB") returns, byte for byte,
without Pillow.  Headers and Huffman decoding run on the host, dequantisation, inverse DCT, chroma upsampling and YCbCr -> RGB on the
device (decode) or, through the same integer code, on the CPU (decode_host).  include/edgestyle_hip.h lists what is supported and what is
refused; a refused file raises EdgeStyleHipError with the reason.

decode returns device uint8 [H, W, 3] tensors: what ops.person_crop_u8, pipeline.preprocess_images, masks.segment and
NativeBestEmbeddings take unchanged.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import lib as L, ops
from .masks import DEVICE


def _read(item) -> bytes:
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    if isinstance(item, (str, os.PathLike)):
        with open(item, "rb") as f:
            return f.read()
    raise L.EdgeStyleHipError(f"jpeg: bytes or a path expected, got {type(item).__name__}")


def _items(data):
    """-> (list of bytes, whether the input was one file)"""
    if isinstance(data, (list, tuple)):
        if not data:
            raise L.EdgeStyleHipError("jpeg: no files")
        return [_read(d) for d in data], False
    return [_read(data)], True


def info(data) -> L.JpegInfo:
    """es_jpeg_info_host: size, components, sampling, MCU grid and restart interval of one file (bytes or a path)"""
    out = L.JpegInfo()
    raw = _read(data)
    L.check(L.load().es_jpeg_info_host(raw, len(raw), C.byref(out)), "es_jpeg_info_host")
    return out


def _infos(raws):
    arr = (L.JpegInfo * len(raws))()
    lib = L.load()
    for i, raw in enumerate(raws):
        L.check(lib.es_jpeg_info_host(raw, len(raw), C.byref(arr[i])), "es_jpeg_info_host")
    return arr


def entropy_decode(data, jpeg_info: L.JpegInfo = None):
    """es_jpeg_entropy_decode_host -> (info, int16 coefficients [es_jpeg_coeff_count], uint16 tables [components, 64]) as numpy arrays:
    the coefficients block-major per component in natural order, the table of each component in natural order"""
    raw = _read(data)
    lib = L.load()
    if jpeg_info is None:
        jpeg_info = info(raw)
    count = int(lib.es_jpeg_coeff_count(C.byref(jpeg_info)))
    if count == 0:
        L.check(-1, "es_jpeg_coeff_count")
    coeffs = np.empty((count,), dtype=np.int16)
    qtables = np.zeros((jpeg_info.components, 64), dtype=np.uint16)
    L.check(lib.es_jpeg_entropy_decode_host(raw, len(raw), C.byref(jpeg_info), coeffs.ctypes.data, qtables.ctypes.data), "es_jpeg_entropy_decode_host")
    return jpeg_info, coeffs, qtables


def reconstruct_host(infos, coeffs, qtables, out=None):
    """es_jpeg_reconstruct_host: the kernels' integer code on the CPU -> a list of uint8 [H, W, 3] numpy arrays (`out`, when given: C-ordered
    pixels, rows may be pitched)"""
    n = len(infos)
    arr = (L.JpegInfo * n)(*infos)
    if out is None:
        out = [np.empty((arr[i].height, arr[i].width, 3), dtype=np.uint8) for i in range(n)]
    descs = (L.ImageU8 * n)()
    for i, a in enumerate(out):
        H, W = arr[i].height, arr[i].width
        if a.dtype != np.uint8 or a.shape != (H, W, 3) or a.strides[2] != 1 or a.strides[1] != 3 or (H > 1 and a.strides[0] < W * 3):
            raise L.EdgeStyleHipError(f"jpeg: output {i} must be a uint8 [{H}, {W}, 3] array with dense pixels")
        descs[i].data, descs[i].height, descs[i].width, descs[i].channels = a.ctypes.data, H, W, 3
        descs[i].row_stride = a.strides[0] if H > 1 else W * 3
    coeffs = [np.ascontiguousarray(c, dtype=np.int16) for c in coeffs]
    qtables = [np.ascontiguousarray(q, dtype=np.uint16) for q in qtables]
    lib = L.load()
    for i in range(n):
        if coeffs[i].size < int(lib.es_jpeg_coeff_count(C.byref(arr[i]))) or qtables[i].size < 64 * arr[i].components:
            raise L.EdgeStyleHipError(f"jpeg: coefficients or tables of image {i} are shorter than its info asks for")
    cp = (C.c_void_p * n)(*[c.ctypes.data for c in coeffs])
    qp = (C.c_void_p * n)(*[q.ctypes.data for q in qtables])
    L.check(lib.es_jpeg_reconstruct_host(arr, n, cp, qp, descs), "es_jpeg_reconstruct_host")
    return out


def decode_host(data):
    """bytes, a path, or a list of either -> uint8 [H, W, 3] numpy array(s), computed on the CPU by the twin of the device code"""
    raws, single = _items(data)
    parts = [entropy_decode(raw) for raw in raws]
    out = reconstruct_host([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts])
    return out[0] if single else out


def upload(coeffs: np.ndarray, qtables: np.ndarray, device=DEVICE):
    """the two host arrays of entropy_decode as the device int16 tensors ops.jpeg_reconstruct takes"""
    return (torch.from_numpy(np.ascontiguousarray(coeffs, dtype=np.int16)).to(device),
            torch.from_numpy(np.ascontiguousarray(qtables, dtype=np.uint16).view(np.int16).reshape(-1)).to(device))


def decode(data, device=DEVICE):
    """bytes, a path, or a list of either -> device uint8 [H, W, 3] tensor(s).  A list is decoded by one es_jpeg_decode_u8 call per 64
    files: the Huffman decoding on this thread, one upload, two launches per 16 images."""
    raws, single = _items(data)
    out = []
    for first in range(0, len(raws), 64):
        part = raws[first:first + 64]
        out += ops.jpeg_decode_u8(part, _infos(part), device)
    return out[0] if single else out

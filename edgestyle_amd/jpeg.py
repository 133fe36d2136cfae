"""Baseline JPEG files to RGB bytes (csrc/jpeg.h, csrc/jpeg.hip): what Pillow's Image.open(..).convert("RGB") returns, byte for byte,
without Pillow.  Headers and Huffman decoding run on the host, dequantisation, inverse DCT, chroma upsampling and YCbCr -> RGB on the
device (decode) or, through the same integer code, on the CPU (decode_host).  Opt-in, decode(entropy="device") moves the Huffman
decoding onto the device as well (csrc/jpeg_entropy.hip); the default is still the host decoder.  include/edgestyle_hip.h lists what is supported and what is
refused; a refused file raises EdgeStyleHipError with the reason.

decode returns device uint8 [H, W, 3] tensors: what ops.person_crop_u8, pipeline.preprocess_images, masks.segment and
NativeBestEmbeddings take unchanged.

The other direction (csrc/jpeg_encode.hip): encode / encode_device / encode_host turn RGB or gray bytes into the bytes of the file Pillow's
Image.save(f, "JPEG", quality=, subsampling=, restart_marker_blocks=) writes; the device writes the whole file, header and EOI included.
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


def decode(data, device=DEVICE, entropy="host"):
    """bytes, a path, or a list of either -> device uint8 [H, W, 3] tensor(s).  A list is decoded by one es_jpeg_decode_u8 call per 64
    files: the Huffman decoding on this thread, one upload, two launches per 16 images.  That is the default.  entropy="device" (opt-in)
    takes es_jpeg_decode_dev_u8 instead: the files are uploaded as they are and the Huffman decoding runs on the device too
    (csrc/jpeg_entropy.hip); the status words are read back before the images are returned, and a defect raises with its text."""
    if entropy not in ("host", "device"):
        raise L.EdgeStyleHipError(f"jpeg.decode: entropy must be 'host' or 'device', not {entropy!r}")
    raws, single = _items(data)
    out = []
    for first in range(0, len(raws), 64):
        part = raws[first:first + 64]
        if entropy == "host":
            out += ops.jpeg_decode_u8(part, _infos(part), device)
        else:
            images, status = ops.jpeg_decode_dev_u8(part, _infos(part), device)
            ops.jpeg_status_check(status, "jpeg.decode")
            out += images
    return out[0] if single else out


# ---- Huffman decoding in parallel (csrc/jpeg_entropy.hip and its host twin), opt-in ----------------------------------------------------
def scan_prepare(data, jpeg_info: L.JpegInfo = None):
    """es_jpeg_scan_prepare_host: the host half of the parallel decoder -> (info, segments int32 [n, 2] - [begin, end) offsets into the
    file -, tables uint8 [L.JPEG_TABLES_BYTES], uint16 quantisation tables [components, 64]) as numpy arrays.  Refuses what the serial
    decoder refuses around the segments (a missing or misnumbered RSTn marker, no EOI after the scan)."""
    raw = _read(data)
    lib = L.load()
    if jpeg_info is None:
        jpeg_info = info(raw)
    count = int(lib.es_jpeg_segment_count(C.byref(jpeg_info)))
    if count == 0:
        L.check(-1, "es_jpeg_segment_count")
    segments = np.zeros((count, 2), dtype=np.int32)
    tables = np.zeros((L.JPEG_TABLES_BYTES,), dtype=np.uint8)
    qtables = np.zeros((jpeg_info.components, 64), dtype=np.uint16)
    L.check(lib.es_jpeg_scan_prepare_host(raw, len(raw), C.byref(jpeg_info), segments.ctypes.data, tables.ctypes.data, qtables.ctypes.data),
            "es_jpeg_scan_prepare_host")
    return jpeg_info, segments, tables, qtables


def status_text(code: int) -> str:
    return L.load().es_jpeg_status_text(int(code)).decode()


def entropy_decode_parallel_host(data, threads, subseq_bytes=0, check=True):
    """The twin of the device decoder on the CPU (es_jpeg_entropy_decode_parallel_host), `threads` standing for the workgroup's size ->
    (info, int16 coefficients, uint16 tables [components, 64], status, synchronise rounds); the coefficients are what entropy_decode
    gives, whatever threads and subseq_bytes are.  A non-zero status raises with its text unless check is False."""
    raw = _read(data)
    jpeg_info, segments, tables, qtables = scan_prepare(raw)
    lib = L.load()
    coeffs = np.empty((int(lib.es_jpeg_coeff_count(C.byref(jpeg_info))),), dtype=np.int16)
    status = np.zeros((1,), dtype=np.int32)
    rounds = C.c_int32(0)
    buf = np.frombuffer(raw, dtype=np.uint8)
    L.check(lib.es_jpeg_entropy_decode_parallel_host(C.byref(jpeg_info), 1, (C.c_void_p * 1)(buf.ctypes.data), (C.c_size_t * 1)(len(raw)),
                                                     (C.c_void_p * 1)(segments.ctypes.data), (C.c_void_p * 1)(tables.ctypes.data), int(subseq_bytes),
                                                     int(threads), (C.c_void_p * 1)(coeffs.ctypes.data), status.ctypes.data, C.byref(rounds)),
            "es_jpeg_entropy_decode_parallel_host")
    if check and status[0] != 0:
        raise L.EdgeStyleHipError(f"jpeg.entropy_decode_parallel_host: {status_text(status[0])} (status {int(status[0])})")
    return jpeg_info, coeffs, qtables, int(status[0]), int(rounds.value)


def entropy_decode_device(data, subseq_bytes=0, device=DEVICE):
    """bytes, a path, or a list of either -> (infos, a list of device int16 coefficient tensors, a list of device int16 table tensors -
    both as ops.jpeg_reconstruct takes them -, the device int32 status tensor).  The host parses and prepares, the files are uploaded as
    they are, es_jpeg_entropy_decode decodes them.  Nothing is read back: ops.jpeg_status_check(status) does that."""
    raws, _ = _items(data)
    parts = [scan_prepare(raw) for raw in raws]
    infos = (L.JpegInfo * len(raws))(*[p[0] for p in parts])
    files = [torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(device) for raw in raws]
    segments = [torch.from_numpy(p[1].reshape(-1)).to(device) for p in parts]
    tables = [torch.from_numpy(p[2]).to(device) for p in parts]
    qtables = [torch.from_numpy(np.ascontiguousarray(p[3]).view(np.int16).reshape(-1)).to(device) for p in parts]
    coeffs, status = ops.jpeg_entropy_decode(infos, files, segments, tables, subseq_bytes)
    return infos, coeffs, qtables, status


# ---- encoding (csrc/jpeg_encode.hip) ----------------------------------------------------------------------------------------------
# RGB or gray bytes -> the bytes Pillow's Image.fromarray(a).save(f, "JPEG", quality=, subsampling=[, restart_marker_blocks=]) writes.
_SUBSAMPLING = {0: 0, 1: 1, 2: 2, "4:4:4": 0, "4:2:2": 1, "4:2:0": 2, "4:1:1": 2}       # Pillow's spellings (its "4:1:1" is 4:2:0)


def encode_params(quality=75, subsampling="4:2:0", restart_marker_blocks=0, **other) -> L.JpegEncodeParams:
    """Pillow's save arguments as es_jpeg_encode_params.  Anything else Pillow would take (optimize, progressive, dpi, exif, ...) is
    refused, never approximated."""
    if other:
        raise L.EdgeStyleHipError(f"jpeg.encode: {', '.join(sorted(other))} not supported (baseline files with the standard tables only)")
    if isinstance(subsampling, bool) or subsampling not in _SUBSAMPLING:
        raise L.EdgeStyleHipError(f"jpeg.encode: unknown subsampling {subsampling!r} (0, 1, 2, '4:4:4', '4:2:2' or '4:2:0')")
    for name, v in (("quality", quality), ("restart_marker_blocks", restart_marker_blocks)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise L.EdgeStyleHipError(f"jpeg.encode: {name} must be an integer")
    return L.JpegEncodeParams(int(quality), _SUBSAMPLING[subsampling], int(restart_marker_blocks))


def _images(images):
    """-> (list of [H, W, 3] / [H, W] arrays, whether the input was one image)"""
    if isinstance(images, (list, tuple)):
        if not images:
            raise L.EdgeStyleHipError("jpeg.encode: no images")
        return list(images), False
    if images.ndim == 4:
        return [images[i] for i in range(images.shape[0])], False
    return [images], True


def forward_host(arrays, params):
    """es_jpeg_forward_host -> (infos, a list of int16 coefficient arrays in the decoder's layout)"""
    descs = ops.jpeg_image_descs("jpeg.forward_host", arrays)
    infos = ops.jpeg_encode_infos("jpeg.forward_host", descs, params)
    lib = L.load()
    coeffs = [np.empty((int(lib.es_jpeg_coeff_count(C.byref(infos[i]))),), dtype=np.int16) for i in range(len(arrays))]
    cp = (C.c_void_p * len(arrays))(*[c.ctypes.data for c in coeffs])
    L.check(lib.es_jpeg_forward_host(descs, len(arrays), C.byref(params), cp), "es_jpeg_forward_host")
    return infos, coeffs


def entropy_encode_host(infos, params, coeffs):
    """es_jpeg_entropy_encode_host -> a list of bytes: the whole files"""
    lib = L.load()
    n = len(coeffs)
    arr = (L.JpegInfo * n)(*infos)
    coeffs = [np.ascontiguousarray(c, dtype=np.int16) for c in coeffs]
    caps = [int(lib.es_jpeg_encode_capacity(C.byref(arr[i]), C.byref(params))) for i in range(n)]
    if 0 in caps:
        L.check(-1, "es_jpeg_encode_capacity")
    for i in range(n):
        if coeffs[i].size < int(lib.es_jpeg_coeff_count(C.byref(arr[i]))):
            raise L.EdgeStyleHipError(f"jpeg: the coefficients of image {i} are shorter than its info asks for")
    out = [np.empty((c,), dtype=np.uint8) for c in caps]
    lengths = np.zeros((n,), dtype=np.uint32)
    L.check(lib.es_jpeg_entropy_encode_host(arr, n, C.byref(params), (C.c_void_p * n)(*[c.ctypes.data for c in coeffs]),
                                            (C.c_void_p * n)(*[o.ctypes.data for o in out]), (C.c_size_t * n)(*caps), lengths.ctypes.data),
            "es_jpeg_entropy_encode_host")
    return [o[:int(k)].tobytes() for o, k in zip(out, lengths)]


def encode_host(arrays, quality=75, subsampling="4:2:0", restart_marker_blocks=0, **other):
    """numpy uint8 [H, W, 3], [H, W], [B, H, W, 3] or a list -> bytes | list[bytes], computed on the CPU by the twin of the device code"""
    params = encode_params(quality, subsampling, restart_marker_blocks, **other)
    arrays, single = _images(arrays)
    what = "jpeg.encode_host"
    descs = ops.jpeg_image_descs(what, arrays)
    infos = ops.jpeg_encode_infos(what, descs, params)
    lib = L.load()
    n = len(arrays)
    caps = [int(lib.es_jpeg_encode_capacity(C.byref(infos[i]), C.byref(params))) for i in range(n)]
    if 0 in caps:
        L.check(-1, "es_jpeg_encode_capacity")
    out = [np.empty((c,), dtype=np.uint8) for c in caps]
    lengths = np.zeros((n,), dtype=np.uint32)
    L.check(lib.es_jpeg_encode_host(descs, n, C.byref(params), (C.c_void_p * n)(*[o.ctypes.data for o in out]), (C.c_size_t * n)(*caps),
                                    lengths.ctypes.data), "es_jpeg_encode_host")
    files = [o[:int(k)].tobytes() for o, k in zip(out, lengths)]
    return files[0] if single else files


def encode_device(images, quality=75, subsampling="4:2:0", restart_marker_blocks=0, **other):
    """device uint8 [H, W, 3], [H, W], [B, H, W, 3] or a list -> (a list of uint8 buffer tensors, one uint32 lengths tensor), all on the
    device: buffer i holds file i in its first lengths[i] bytes.  Nothing is read back and nothing synchronises; one es_jpeg_encode_u8
    call per 64 images, 8 launches per 16."""
    params = encode_params(quality, subsampling, restart_marker_blocks, **other)
    images, _ = _images(images)
    out, lengths = [], []
    for first in range(0, len(images), 64):
        o, k = ops.jpeg_encode_u8(images[first:first + 64], params)
        out += o
        lengths.append(k)
    return out, lengths[0] if len(lengths) == 1 else torch.cat([k.view(torch.int32) for k in lengths]).view(torch.uint32)


def encode(images, quality=75, subsampling="4:2:0", restart_marker_blocks=0, **other):
    """device uint8 [H, W, 3], [H, W], [B, H, W, 3] or a list -> bytes | list[bytes]: the files Pillow would write.  One download of the
    lengths, then one of the finished files (gathered on the device); the pixels never leave it."""
    single = not isinstance(images, (list, tuple)) and images.ndim != 4
    out, lengths = encode_device(images, quality, subsampling, restart_marker_blocks, **other)
    sizes = [int(k) for k in lengths.cpu().view(torch.int32).tolist()]
    blob = torch.cat([o[:k] for o, k in zip(out, sizes)]).cpu().numpy().tobytes()
    files, at = [], 0
    for k in sizes:
        files.append(blob[at:at + k])
        at += k
    return files[0] if single else files

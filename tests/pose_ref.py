"""Shared by tests/test_pose_cpu.py, tests/test_pose_gpu.py and tools/pose_crop_bench.py: the fixture (the reference's key points and
its own pose renderings, Pillow's LANCZOS bytes), the drawing rule of csrc/pose.hip restated in Python integers and numpy int64 from the
header's text (not from the C code), create_processed_image's geometry line by line, the integer resize built from
es_image_resize_coeffs_ex, and the PSNR / IoU figures the rule is held to."""
import ctypes as C
import math
import os

import numpy as np

from edgestyle_amd import lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pose.safetensors")
POSES = ("source/openpose/1", "target/openpose/0", "target/openpose/2")      # docs/test/<name>.{json,jpg} of the reference
# (H, W, new_h, new_w) of the Pillow-LANCZOS cases of the fixture, in order: up, down, mixed, one axis unchanged
LANCZOS_CASES = [(37, 53, 61, 40), (301, 200, 64, 43), (64, 48, 23, 96), (50, 67, 50, 31)]
FILTER_LANCZOS = 2

# controlnet_aux's limbSeq (1-based) and colours
LIMBS = [(2, 3), (2, 6), (3, 4), (4, 5), (6, 7), (7, 8), (2, 9), (9, 10), (10, 11), (2, 12), (12, 13), (13, 14), (2, 1), (1, 15), (15, 17),
         (1, 16), (16, 18)]
COLOURS = [(255, 0, 0), (255, 85, 0), (255, 170, 0), (255, 255, 0), (170, 255, 0), (85, 255, 0), (0, 255, 0), (0, 255, 85), (0, 255, 170),
           (0, 255, 255), (0, 170, 255), (0, 85, 255), (0, 0, 255), (85, 0, 255), (170, 0, 255), (255, 0, 255), (255, 0, 170), (255, 0, 85)]
STICK = 4
COORD_LIMIT = 65536.0

_fixture = None


def fixture():
    """{"kp": [3 x float32 [18,3]], "jpg": [3 x uint8 [512,512,3]], "lanczos": [(input, Pillow's bytes)], "pillow": version} (read once)"""
    global _fixture
    if _fixture is None:
        from safetensors import safe_open
        import ast
        import zlib
        with safe_open(GOLDEN, framework="np") as f:
            meta = f.metadata()
            assert ast.literal_eval(meta["lanczos_cases"]) == LANCZOS_CASES and ast.literal_eval(meta["poses"]) == list(POSES)
            shape = ast.literal_eval(meta["jpg_shape"])
            jpg = [np.frombuffer(zlib.decompress(f.get_tensor(f"jpg{i}_z").tobytes()), dtype=np.uint8).reshape(shape) for i in range(3)]
            _fixture = dict(kp=[f.get_tensor(f"kp{i}") for i in range(3)], jpg=jpg, scores=ast.literal_eval(meta["scores"]),
                            lanczos=[(f.get_tensor(f"lz_in{i}"), f.get_tensor(f"lz_out{i}")) for i in range(len(LANCZOS_CASES))],
                            pillow=meta["pillow"])
    return _fixture


def keypoints_array(kps) -> np.ndarray:
    """JSON-style key points (None = absent, [x, y, score, ...]) -> float32 [18, 3]; an absent point is (0, 0, 0)"""
    out = np.zeros((18, 3), dtype=np.float32)
    for i, p in enumerate(kps):
        if p is not None:
            out[i] = (p[0], p[1], p[2] if len(p) > 2 else 1.0)
    return out


# ---- the drawing rule ---------------------------------------------------------------------------------------------------
SIN_Q = [int(round(math.sin(math.radians(t)) * 2 ** 30)) for t in range(91)]        # sin(t degrees) in 2^-30 units, t = 0 .. 90


def sin_q(t: int) -> int:
    t %= 360
    if t <= 90:
        return SIN_Q[t]
    if t <= 180:
        return SIN_Q[180 - t]
    return -sin_q(t - 180)


def cos_q(t: int) -> int:
    return sin_q(t + 90)


def _present(p, H, W):
    x, y, s = float(p[0]), float(p[1]), float(p[2])
    return s > 0 and abs(x * W) < COORD_LIMIT and abs(y * H) < COORD_LIMIT


def _angle(qx: int, qy: int) -> int:
    ay, t = abs(qy), 0
    while t < 180 and cos_q(t + 1) * ay - sin_q(t + 1) * qx >= 0:
        t += 1
    return -t if qy < 0 else t


def records(kp: np.ndarray, H: int, W: int):
    """the shapes of one pose in draw order: (cx, cy, A, B, cos, sin, colour) - an ellipse of semi-axes A / 2 along (cos, sin) and
    B / 2 across it, centred on pixel (cx, cy)"""
    out = []
    for (f, t), col in zip(LIMBS, COLOURS):
        p, q = kp[f - 1], kp[t - 1]
        if not (_present(p, H, W) and _present(q, H, W)):
            continue
        xp, yp, xq, yq = float(p[0]) * W, float(p[1]) * H, float(q[0]) * W, float(q[1]) * H
        cx, cy = int((xp + xq) / 2), int((yp + yq) / 2)
        qx, qy = int((xp - xq) * 256), int((yp - yq) * 256)
        a = math.isqrt(qx * qx + qy * qy) >> 9
        ang = _angle(qx, qy)
        out.append((cx, cy, 2 * a + 1, 2 * STICK + 1, cos_q(ang), sin_q(ang), tuple(int(c * 0.6) for c in col)))
    for p, col in zip(kp, COLOURS):
        if _present(p, H, W):
            out.append((int(float(p[0]) * W), int(float(p[1]) * H), 2 * STICK, 2 * STICK, 1 << 30, 0, col))       # a disc of radius 4, rim included
    return out


def covers(rec, H: int, W: int) -> np.ndarray:
    """bool [H, W]: the pixels of the canvas the shape covers (64-bit integers throughout)"""
    cx, cy, A, B, c, s, _ = rec
    v, u = np.mgrid[0:H, 0:W].astype(np.int64)
    u -= cx
    v -= cy
    al = (u * c + v * s + (1 << 21)) >> 22             # along and across the limb, in 1/256 pixel (floor)
    ac = (v * c - u * s + (1 << 21)) >> 22
    near = (np.abs(al) <= 128 * A) & (np.abs(ac) <= 128 * B)
    al, ac = np.where(near, al, 0), np.where(near, ac, 0)
    return near & (al * al * (B * B) + ac * ac * (A * A) <= 16384 * A * A * B * B)


def draw(kp: np.ndarray, H: int, W: int) -> np.ndarray:
    canvas = np.zeros((H, W, 3), dtype=np.uint8)
    for rec in records(np.asarray(kp, dtype=np.float32), H, W):
        canvas[covers(rec, H, W)] = rec[6]
    return canvas


def psnr_iou(got: np.ndarray, ref: np.ndarray):
    """whole-image PSNR in dB, and IoU of the pixel sets whose largest channel exceeds 40"""
    d = got.astype(np.int64) - ref.astype(np.int64)
    mse = float((d * d).mean())
    a, b = got.max(2) > 40, ref.max(2) > 40
    return 10 * math.log10(255.0 ** 2 / mse), float((a & b).sum()) / float((a | b).sum())


# ---- host calls of the library ----------------------------------------------------------------------------------------------
def draw_host(kp: np.ndarray, H: int, W: int) -> np.ndarray:
    kp = np.ascontiguousarray(kp, dtype=np.float32).reshape(-1, 18, 3)
    out = np.full((kp.shape[0], H, W, 3), 0xA5, dtype=np.uint8)
    L.check(L.load().es_pose_draw_host(kp.ctypes.data, out.ctypes.data, kp.shape[0], H, W), "es_pose_draw_host")
    return out


def select_host(kps, scores, parts) -> int:
    kps = np.ascontiguousarray(kps, dtype=np.float32).reshape(-1, 18, 3)
    n = kps.shape[0]
    sc, pa = (C.c_double * max(n, 1))(*scores), (C.c_double * max(n, 1))(*parts)
    return L.load().es_pose_select_host(kps.ctypes.data, sc, pa, n)


def points_host(kp, W: int, H: int) -> np.ndarray:
    kp = np.ascontiguousarray(kp, dtype=np.float32).reshape(18, 3)
    out = np.zeros((18, 2), dtype=np.float32)
    n = L.load().es_pose_points_host(kp.ctypes.data, W, H, out.ctypes.data)
    assert 0 <= n <= 18, L.load().es_last_error()
    return out[:n]


# ---- create_processed_image --------------------------------------------------------------------------------------------------
def crop_fit(height: int, width: int, box, final_width: int = 512, final_height: int = 512, margin: float = 0.1):
    """extract_dataset.py:118-164 as it stands -> (new_w, new_h, left, top)"""
    xmin, ymin, xmax, ymax = (float(v) for v in box)
    bbox_width = xmax - xmin
    bbox_height = ymax - ymin
    margin_width = bbox_width * margin
    margin_height = bbox_height * margin
    xmin = max(0, xmin - margin_width)
    xmax = min(width, xmax + margin_width)
    ymin = max(0, ymin - margin_height)
    ymax = min(height, ymax + margin_height)
    bbox_center_x = (xmin + xmax) / 2
    bbox_center_y = (ymin + ymax) / 2
    scale_x = final_width / (xmax - xmin)
    scale_y = final_height / (ymax - ymin)
    scale = min(scale_x, scale_y)
    new_width = int(width * scale)
    new_height = int(height * scale)
    new_bbox_center_x = int(bbox_center_x * scale)
    new_bbox_center_y = int(bbox_center_y * scale)
    top_left_x = max(0, new_bbox_center_x - final_width // 2)
    top_left_y = max(0, new_bbox_center_y - final_height // 2)
    if top_left_x + final_width > new_width:
        top_left_x = new_width - final_width
    if top_left_y + final_height > new_height:
        top_left_y = new_height - final_height
    return new_width, new_height, top_left_x, top_left_y


def crop_fit_lib(height, width, box, final_width=512, final_height=512, margin=0.1):
    out, b = (C.c_int32 * 4)(), (C.c_double * 4)(*[float(v) for v in box])
    L.check(L.load().es_person_crop_fit(height, width, b, final_width, final_height, margin, out), "es_person_crop_fit")
    return tuple(out)


def coeffs(filt: int, n_in: int, n_out: int):
    lib = L.load()
    cap = lib.es_image_resize_coeffs_ex(filt, n_in, n_out, None, None, None, 0)
    assert cap >= 1, lib.es_last_error()
    xmin, nt, k = (C.c_int32 * n_out)(), (C.c_int32 * n_out)(), (C.c_int32 * (n_out * cap))()
    assert lib.es_image_resize_coeffs_ex(filt, n_in, n_out, xmin, nt, k, cap) == cap
    return np.array(xmin), np.array(nt), np.array(k).reshape(n_out, cap)


def resize_axis(a: np.ndarray, n_out: int, axis: int, filt: int) -> np.ndarray:
    """one pass: out = clip8(((1 << 21) + sum k * src) >> 22); a pass that does not change the size is skipped"""
    if a.shape[axis] == n_out:
        return a
    xmin, nt, k = coeffs(filt, a.shape[axis], n_out)
    src = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], dtype=np.uint8)
    for i in range(n_out):
        taps = k[i, :nt[i]].astype(np.int64)
        acc = (1 << 21) + np.tensordot(taps, src[xmin[i]:xmin[i] + nt[i]], axes=(0, 0))
        assert acc.max() < 2 ** 31 and acc.min() >= -2 ** 31        # the kernels accumulate in 32 bits
        assert (1 << 21) + 255 * int(np.abs(taps).sum()) < 2 ** 31  # ... and so does every partial sum, whatever the bytes
        out[i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def integer_resize(a: np.ndarray, rh: int, rw: int, filt: int = FILTER_LANCZOS) -> np.ndarray:
    """horizontal pass, then vertical pass, a uint8 image after each (Pillow's order)"""
    return resize_axis(resize_axis(a, rw, 1, filt), rh, 0, filt)


def window(full: np.ndarray, left: int, top: int, out_h: int, out_w: int) -> np.ndarray:
    """PIL's crop((left, top, left + out_w, top + out_h)): zeros where the window hangs outside the image"""
    out = np.zeros((out_h, out_w, 3), dtype=np.uint8)
    h, w = full.shape[:2]
    y0, y1, x0, x1 = max(top, 0), min(top + out_h, h), max(left, 0), min(left + out_w, w)
    if y1 > y0 and x1 > x0:
        out[y0 - top:y1 - top, x0 - left:x1 - left] = full[y0:y1, x0:x1, :3]
    return out


def processed_image(a: np.ndarray, box, final_width=512, final_height=512, filt: int = FILTER_LANCZOS) -> np.ndarray:
    nw, nh, left, top = crop_fit(a.shape[0], a.shape[1], box, final_width, final_height)
    return window(integer_resize(a[:, :, :3], nh, nw, filt), left, top, final_height, final_width)


def pillow_lanczos(a: np.ndarray, rh: int, rw: int) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((rw, rh), Image.LANCZOS))


def have_pillow() -> bool:
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


def random_pose(g: np.random.Generator, absent: float = 0.25, spread: float = 0.0) -> np.ndarray:
    """float32 [18,3]: points in [-spread, 1 + spread], a share of them absent (score 0, -1 or NaN)"""
    kp = np.empty((18, 3), dtype=np.float32)
    kp[:, :2] = g.uniform(-spread, 1 + spread, size=(18, 2))
    kp[:, 2] = g.uniform(0.1, 1.0, size=18)
    gone = g.random(18) < absent
    kp[gone, 2] = g.choice(np.array([0.0, -1.0, np.nan], dtype=np.float32), size=int(gone.sum()))
    return kp

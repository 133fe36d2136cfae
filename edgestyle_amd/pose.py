"""The deterministic half of app.py's `preprocess` around the two detectors, under the reference's names (csrc/image_io.hip and
csrc/pose.hip through ops): from a person box to the 512 x 512 processed photo (create_processed_image, extract_dataset.py:112-171),
from 18 body key points to the pose condition image (create_openpose after detect_poses, :222-295, with controlnet_aux's draw_bodypose
as its arithmetic) and to the SAM point prompt (create_sam_images:361-365).  The detectors themselves (YOLOv5, OpenPose) stay with the
caller: what they return - a box, candidate poses - is what these functions take.

Photos are numpy arrays, torch tensors or PIL images; key points are fp32 [18, 3] = (x, y, score) arrays or tensors with x and y in
[0, 1], or JSON-style lists as the reference stores them ([x, y, score, id] or None per point).  A key point is absent iff its score is
not > 0.  Images come back as device uint8 HWC tensors: what pipeline.preprocess_images, masks.segment and NativeBestEmbeddings take
unchanged.
"""
import ctypes as C

import numpy as np
import torch

from . import lib as L, ops
from .masks import DEVICE, to_image

IMAGE_WIDTH = IMAGE_HEIGHT = 512


def _bad(msg: str):
    return L.EdgeStyleHipError("pose: " + msg)


def _keypoints(keypoints):
    """-> (host fp32 [count, 18, 3], whether the input was one pose)"""
    if isinstance(keypoints, dict):
        keypoints = keypoints["keypoints"]
    if torch.is_tensor(keypoints):
        a = keypoints.detach().to("cpu", torch.float32).numpy()
    elif isinstance(keypoints, np.ndarray):
        a = keypoints.astype(np.float32)
    else:
        seq = list(keypoints)
        if len(seq) == 18 and all(p is None or (not isinstance(p, dict) and np.ndim(p) == 1) for p in seq):
            seq = [seq]
            single = True
        else:
            single = False
        a = np.zeros((len(seq), 18, 3), dtype=np.float32)
        for n, pose in enumerate(seq):
            pose = pose["keypoints"] if isinstance(pose, dict) else pose
            if len(pose) != 18:
                raise _bad(f"a pose has 18 key points, got {len(pose)}")
            for i, p in enumerate(pose):
                if p is not None:
                    if len(p) < 2:
                        raise _bad(f"key point {i} must be [x, y(, score, ...)] or None")
                    a[n, i] = (float(p[0]), float(p[1]), float(p[2]) if len(p) > 2 else 1.0)
        return a, single
    single = a.ndim == 2
    if single:
        a = a[None]
    if a.ndim != 3 or a.shape[1:] != (18, 3) or a.shape[0] < 1:
        raise _bad(f"key points are [18, 3] or [count, 18, 3] = (x, y, score), got {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float32), single


def to_keypoints(keypoints) -> np.ndarray:
    """one pose or a batch of poses -> host fp32 [count, 18, 3]; None (an absent point of the reference's JSON) becomes (0, 0, 0), a point
    given without a score gets score 1; a dict is the reference's posedict ({"keypoints": ...})"""
    return _keypoints(keypoints)[0]


def create_processed_image(image, box, final_width: int = IMAGE_WIDTH, final_height: int = IMAGE_HEIGHT) -> torch.Tensor:
    """create_processed_image: the photo resized with Pillow's LANCZOS so that `box` = (xmin, ymin, xmax, ymax) with its 10 % margin fits
    the final size, then the final_width x final_height window around the box centre (zeros where the resized photo ends before the
    window does) -> uint8 [final_height, final_width, 3] on the device, byte for byte Pillow's pixels."""
    img = to_image(image)
    if (int(final_width), int(final_height)) == (IMAGE_WIDTH, IMAGE_HEIGHT):
        return ops.person_crop_u8([img], [box])[0]
    geom = ops.person_crop_fit(img.shape[0], img.shape[1], box, final_width, final_height)
    return ops.image_resize_window_u8([img], [geom], int(final_height), int(final_width), L.FILTER_LANCZOS)[0]


def draw_bodypose(keypoints, H: int, W: int) -> torch.Tensor:
    """controlnet_aux's draw_bodypose on a black canvas: one pose -> uint8 [H, W, 3], a batch of poses -> [count, H, W, 3] (one launch)"""
    kp, single = _keypoints(keypoints)
    dev = keypoints.device if torch.is_tensor(keypoints) and keypoints.is_cuda else DEVICE
    out = ops.pose_draw(torch.from_numpy(kp).to(dev), H, W)
    return out[0] if single else out


def draw_poses(poses, H: int, W: int, draw_body: bool = True, draw_hand: bool = False, draw_face: bool = False) -> torch.Tensor:
    """controlnet_aux's draw_poses as the reference calls it: the one pose create_openpose chose (`[pose]`, or the pose itself), body only
    -> uint8 [H, W, 3].  Several canvases in one launch: draw_bodypose with a batch."""
    if draw_hand or draw_face:
        raise _bad("hands and faces are not drawn (the reference switches them off)")
    kp = to_keypoints(poses)
    if kp.shape[0] != 1:
        raise _bad(f"draw_poses draws the one chosen pose, got {kp.shape[0]} (select_pose picks it; draw_bodypose takes a batch)")
    if not draw_body:
        return torch.zeros((int(H), int(W), 3), dtype=torch.uint8, device=DEVICE)
    return ops.pose_draw(torch.from_numpy(kp).to(DEVICE), H, W)[0]


def select_pose(candidates) -> int:
    """create_openpose's filters and choice over the detector's candidates - each a dict {"keypoints", "total_score", "total_parts"} (the
    reference's posedict) or a (keypoints, total_score, total_parts) tuple -> the index of the chosen pose, -1 when none remains"""
    cands = [(c["keypoints"], c["total_score"], c["total_parts"]) if isinstance(c, dict) else tuple(c) for c in candidates]
    n = len(cands)
    if n == 0:
        return -1
    kps = np.concatenate([to_keypoints(c[0])[:1] for c in cands])
    score, parts = (C.c_double * n)(*[float(c[1]) for c in cands]), (C.c_double * n)(*[float(c[2]) for c in cands])
    r = L.load().es_pose_select_host(kps.ctypes.data, score, parts, n)
    if r < -1:
        L.check(r, "es_pose_select_host")
    return int(r)


def sam_points(keypoints, W: int = IMAGE_WIDTH, H: int = IMAGE_HEIGHT) -> np.ndarray:
    """the SAM point prompt of create_sam_images: the present key points of one pose times (W, H), in order -> host fp32 [P, 2], what
    masks.segment takes as `points`"""
    kp = to_keypoints(keypoints)
    if kp.shape[0] != 1:
        raise _bad("sam_points takes one pose")
    out = np.zeros((18, 2), dtype=np.float32)
    n = L.load().es_pose_points_host(kp.ctypes.data, int(W), int(H), out.ctypes.data)
    if n < 0:
        L.check(n, "es_pose_points_host")
    return out[:n].copy()


def condition_inputs(photo, box, keypoints, final_width: int = IMAGE_WIDTH, final_height: int = IMAGE_HEIGHT):
    """photo + person box + the chosen pose's key points (normalised to the processed photo, as the detector run on it gives them) ->
    (processed uint8 [H, W, 3], pose image uint8 [H, W, 3], SAM points fp32 [P, 2] in the processed photo's pixels)"""
    processed = create_processed_image(photo, box, final_width, final_height)
    kp = to_keypoints(keypoints)
    if kp.shape[0] != 1:
        raise _bad("condition_inputs takes one pose")
    pose_image = ops.pose_draw(torch.from_numpy(kp).to(processed.device), int(final_height), int(final_width))[0]
    return processed, pose_image, sam_points(kp, final_width, final_height)

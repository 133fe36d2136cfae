"""Mask post-processing on the device, under the reference's names (csrc/mask.hip through ops): what extract_dataset.py:316-351
and :394-502 (app.py's `preprocess`) and inference.py:322-447 do on the host with cv2 and skimage between a segmenter's mask
predictions and the images try_on takes.  Every function takes numpy arrays, torch tensors or PIL images, works on the GPU and
returns device uint8 tensors: masks of 0 / 1 (a `.bool()` view away from the reference's arrays), images as uint8 HWC - what
pipeline.preprocess_images and NativeBestEmbeddings take unchanged.

A mask is [H, W] or a batch [count, H, W]; the result has the shape of the input.  The networks (YOLOv5, OpenPose,
EfficientViT-SAM), the `subject_scores < 0.5` test and the choice of which image goes to which slot stay with the caller; getBox is
`get_box` (csrc/sam_decoder.hip), which leaves the box on the device for the next decode's prompt.
"""
import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import lib as L, ops

DEVICE = "cuda"
BG_COLOR = (127, 127, 127)


def _bad(msg: str):
    return L.EdgeStyleHipError("masks: " + msg)


def _tensor(x) -> torch.Tensor:
    if torch.is_tensor(x):
        return x
    if hasattr(x, "convert") and not isinstance(x, np.ndarray):      # PIL hands out a read-only view
        return torch.from_numpy(np.array(x, order="C"))
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x)))


def to_mask(x, device=None):
    """-> (uint8 [count, H, W] device tensor whose nonzero bytes are the true pixels, whether the input was one [H, W] mask)"""
    t = _tensor(x)
    if t.dim() not in (2, 3):
        raise _bad(f"a mask is [H, W] or [count, H, W], got {tuple(t.shape)}")
    single = t.dim() == 2
    if t.dtype not in (torch.uint8, torch.bool):
        t = t != 0
    t = t.to(device or (t.device if t.is_cuda else DEVICE))
    t = (t.view(torch.uint8) if t.dtype == torch.bool else t).contiguous()
    return (t[None] if single else t), single


def to_image(x, device=None) -> torch.Tensor:
    """-> a uint8 [H, W, 3 | 4] device tensor"""
    if hasattr(x, "convert") and not torch.is_tensor(x) and not isinstance(x, np.ndarray):
        x = x.convert("RGB")
    t = _tensor(x)
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] not in (3, 4):
        raise _bad(f"an image is uint8 [H, W, 3 | 4], got {t.dtype} {tuple(t.shape)}")
    return t.to(device or (t.device if t.is_cuda else DEVICE))


def _morph(mask, radii: Sequence[int]) -> torch.Tensor:
    m, single = to_mask(mask)
    out = ops.mask_morph(m, radii)
    return out[0] if single else out


def closing_square(mask, k: int) -> torch.Tensor:
    """skimage.morphology.closing(mask, square(k)) for odd k: erode(dilate(mask)) with the (k-1)/2 clipped window"""
    k = int(k)
    if k < 1 or k % 2 == 0:
        raise _bad(f"closing_square takes an odd k >= 1, got {k}")
    r = (k - 1) // 2
    return _morph(mask, [r, -r])


def smooth_radius(kernel_size: int = 3, iterations: int = 3) -> int:
    """cv2 with a full kernel_size x kernel_size kernel and `iterations` = one pass with radius iterations * (kernel_size - 1) / 2"""
    kernel_size, iterations = int(kernel_size), int(iterations)
    if kernel_size < 1 or kernel_size % 2 == 0 or iterations < 1:
        raise _bad(f"smooth_mask takes an odd kernel_size >= 1 and iterations >= 1, got {kernel_size}, {iterations}")
    return iterations * (kernel_size - 1) // 2


def smooth_mask(mask, kernel_size: int = 3, iterations: int = 3) -> torch.Tensor:
    """extract_dataset.py:334-351: cv2 closing (dilate, erode) then opening (erode, dilate), each `iterations` times"""
    r = smooth_radius(kernel_size, iterations)
    return _morph(mask, [r, -r, -r, r])


def largest_component(mask, return_area: bool = False):
    """extract_dataset.py:437-450: skimage.measure.label (8-connected) and the region of the largest area, the first of equals in
    label order; a mask without a true pixel gives an all-true result, as the reference's `labeled_array == 0` does"""
    m, single = to_mask(mask)
    area = torch.empty((m.shape[0],), dtype=torch.int32, device=m.device) if return_area else None
    out = ops.mask_largest_component(m, area_out=area)
    out = out[0] if single else out
    return (out, area[0] if single else area) if return_area else out


def get_box(mask, margin: int = 20) -> torch.Tensor:
    """extract_dataset.py:298-313: [max(0, xmin - margin), max(0, ymin - margin), min(W, xmax + margin), min(H, ymax + margin)] over the true
    pixels, zeros for a mask without one -> fp32 [4] (or [count, 4]) on the device, never read back here"""
    m, single = to_mask(mask)
    count, H, W = m.shape
    boxes = torch.empty((count, 4), dtype=torch.float32, device=m.device)
    with torch.cuda.device(m.device):
        L.check(L.load().es_mask_bbox(C.c_void_p(m.data_ptr()), C.c_void_p(boxes.data_ptr()), count, H, W, int(margin),
                                      C.c_void_p(torch.cuda.current_stream(m.device).cuda_stream)), "es_mask_bbox")
    return boxes[0] if single else boxes


def draw_binary_mask(image, mask, mask_color=(0, 0, 255)) -> torch.Tensor:
    """extract_dataset.py:316-331: `image` where `mask` is true, mask_color elsewhere; image None = zeros (np.zeros_like(image))"""
    m, single = to_mask(mask)
    if not single and image is not None:
        imgs = [to_image(i, m.device) for i in image]
    else:
        imgs = None if image is None else [to_image(image, m.device)]
    out = ops.image_mask_fill_u8(imgs, m, mask_color)
    return out[0] if single else out


def create_sam_images(image, subject, body, clothes, head, return_masks: bool = False):
    """extract_dataset.py:394-502 after the four SAM predictions, as ONE library call (es_sam_compose).  image: one photo, with
    [H, W] masks, or a list of photos with [count, H, W] masks.  -> the reference's dict order as a tuple of uint8 [H, W, 3] (or
    [count, H, W, 3]) device tensors: (subject, mask, agnostic, clothes, head); with return_masks also the uint8 masks
    (all, agnostic, clothes, head)."""
    s, single = to_mask(subject)
    b, c, h = (to_mask(t, s.device)[0] for t in (body, clothes, head))
    imgs = [to_image(image, s.device)] if single else [to_image(i, s.device) for i in image]
    masks, images = ops.sam_compose(imgs, s, b, c, h, want_masks=return_masks)
    pick = (lambda t, k: t[0, k]) if single else (lambda t, k: t[:, k])
    out = tuple(pick(images, k) for k in range(5))
    return (out, tuple(pick(masks, k) for k in range(4))) if return_masks else out


def segment(photo, points, predictors, labels=None, margin: int = 20):
    """The network half of create_sam_images (extract_dataset.py:371-429) and its device arithmetic, without a host visit between the
    decodes: one encode, the point-prompted base decode (multimask, mask 0), its box with `margin` (get_box), four box-prompted decodes
    (subject, body, clothes, head; single mask), then create_sam_images.  predictors: five sam.NativeSamPredictor in that order (base
    first) that share one encoder.  points: [P, 2] pose key points in the photo's pixels (labels: all foreground unless given).
    -> (create_sam_images' five images, the subject score as a device scalar: the caller's `< SUBJECT_SCORE_THRESHOLD` test)"""
    if len(predictors) != 5:
        raise _bad("segment takes five predictors: base, subject, body, clothes, head")
    img = to_image(photo)
    base = predictors[0]
    feats, _ = base.encoder.encode_u8([img])
    for p in predictors:
        p.set_features(feats, img.shape[:2])
    pts = torch.as_tensor(np.asarray(points, dtype=np.float32))
    lab = torch.ones(pts.shape[0], dtype=torch.int32) if labels is None else torch.as_tensor(labels)
    all_masks, _, _ = base.predict_device(pts, lab, multimask_output=True)
    box = get_box(all_masks[0], margin)
    outs = [p.predict_device(box=box, multimask_output=False) for p in predictors[1:]]
    subject, body, clothes, head = (o[0][0] for o in outs)
    return create_sam_images(img, subject, body, clothes, head), outs[0][1][0]


def subject_image_masks(subject, body, clothes, kernel_size: int = 3, iterations: int = 3):
    """inference.py:341-420's masks, composed from the primitives: smooth_mask without the closings, no largest component, a
    smoothed `unknown`.  -> (all, agnostic, clothes) uint8 masks; the three images are draw_binary_mask(image, m, BG_COLOR)."""
    sm = lambda x: smooth_mask(x, kernel_size, iterations)          # noqa: E731
    s, a, c = sm(subject), sm(body), sm(clothes)
    single = s.dim() == 2
    s3, a3, c3 = (t[None] if single else t for t in (s, a, c))
    all_m = sm(ops.mask_logic(s3, ops.mask_logic(a3, c3, L.MASK_OR), L.MASK_OR))
    unknown = sm(ops.mask_logic(a3, c3, L.MASK_AND))
    agnostic = sm(ops.mask_logic(a3, unknown, L.MASK_ANDNOT))
    return tuple(t[0] if single else t for t in (all_m, agnostic, c3))


def subject_image(image, subject, body, clothes, kernel_size: int = 3, iterations: int = 3):
    """inference.py:341-447 after the predictions: -> (subject_image, agnostic_image, clothes_image), uint8 HWC on the device"""
    all_m, agnostic, clothes_m = subject_image_masks(subject, body, clothes, kernel_size, iterations)
    return tuple(draw_binary_mask(image, m, BG_COLOR) for m in (all_m, agnostic, clothes_m))

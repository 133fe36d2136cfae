#!/usr/bin/env python
"""Fixture for the predictor's arithmetic around the SAM mask decoder, produced by the reference's OWN functions.

`EfficientViTSam.postprocess_masks`, `EfficientViTSamPredictor.apply_coords` / `apply_boxes` (efficientvit/models/efficientvit/sam.py) and
`getBox` (extract_dataset.py) are taken out of their files with `ast` and run as they are on a stand-in `self` that carries nothing but the
attributes they read (image_size, original_size, input_size) - sam.py itself imports segment_anything, which is not installed.  Nothing of
the reference travels: what is committed is tensors.

  ref_sam_decoder.safetensors   per case k (an original size): `size_k` int64 [H, W, new_h, new_w]; `logits_k` fp32 [1, 2, 32, 32] (seeded
                                N(0, 16) on 8 x 8, torch-bicubic to 32 x 32: sign changes every few pixels); `post_k` fp64, postprocess_masks of
                                the fp64 logits with the canvas (frame) 128 instead of 1024, which keeps the file small and the code path the same;
                                `coords_k` / `coords_out_k` fp64 [5, 2] and `boxes_k` / `boxes_out_k` fp64 [2, 4] through apply_coords /
                                apply_boxes at the real frame 1024; `mask_k` uint8 [H, W] and `box_k` fp64 [4]: getBox.

    python tests/golden/make_golden_ref_sam_decoder.py REFERENCE_DIR
"""
import ast
import copy
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from safetensors.torch import save_file

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import sam_dec_ref as D                       # noqa: E402

SIZES = ((37, 53), (75, 113), (96, 64), (150, 110))
FRAME = 128


def pick(path, names, cls=None):
    tree = ast.parse(open(path).read(), path)
    body = tree.body
    if cls is not None:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == cls).body
    fns = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(f.name for f in fns) == sorted(names), [f.name for f in fns]
    for f in fns:
        f.decorator_list = []
    ns = {"torch": torch, "F": F, "np": np, "copy": copy, "Tuple": tuple}
    exec(compile(ast.fix_missing_locations(ast.Module(body=fns, type_ignores=[])), path, "exec"), ns)
    return [ns[n] for n in names]


def case_logits(k):
    g = torch.Generator().manual_seed(700 + k)
    return F.interpolate(4.0 * torch.randn(1, 2, 8, 8, generator=g), (32, 32), mode="bicubic", align_corners=False).contiguous()


def case_mask(k, H, W):
    g = torch.Generator().manual_seed(800 + k)
    m = np.zeros((H, W), np.uint8)
    if k != 2:                                            # case 2: an empty mask
        y0, x0 = int(torch.randint(0, H // 2, (1,), generator=g)), int(torch.randint(0, W // 2, (1,), generator=g))
        m[y0:y0 + H // 3 + 1, x0:x0 + W // 3 + 1] = 1
    if k == 3:
        m[H - 1, W - 1] = 1                               # the margin is clipped at the far sides
    return m


def main():
    ref = sys.argv[1]
    sam_py = os.path.join(ref, "efficientvit/models/efficientvit/sam.py")
    (postprocess,) = pick(sam_py, ["postprocess_masks"], "EfficientViTSam")
    apply_coords, apply_boxes = pick(sam_py, ["apply_coords", "apply_boxes"], "EfficientViTSamPredictor")
    (get_box,) = pick(os.path.join(ref, "extract_dataset.py"), ["getBox"])
    out = {}
    for k, (H, W) in enumerate(SIZES):
        small = D.preprocess_shape(H, W, FRAME)
        model = types.SimpleNamespace(image_size=(FRAME, FRAME // 2))
        lg = case_logits(k)
        post = postprocess(model, lg.double(), small, (H, W))
        real = D.preprocess_shape(H, W, 1024)
        pred = types.SimpleNamespace(original_size=(H, W), input_size=real)
        pred.apply_coords = lambda c, _p=pred: apply_coords(_p, c)
        g = torch.Generator().manual_seed(900 + k)
        coords = np.array([[0, 0], [W, H], [W - 1, H - 1], [0.25 * W, 0.75 * H], [-3.5, H + 7.0]]) + np.array([[0, 0]] * 4 + [[0.125, 0]])
        boxes = (torch.rand(2, 4, generator=g, dtype=torch.float64) * torch.tensor([W, H, W, H])).numpy()
        mask = case_mask(k, H, W)
        out.update({f"size_{k}": torch.tensor([H, W, small[0], small[1]]), f"logits_{k}": lg, f"post_{k}": post.contiguous(),
                    f"coords_{k}": torch.from_numpy(coords), f"coords_out_{k}": torch.from_numpy(apply_coords(pred, coords)),
                    f"boxes_{k}": torch.from_numpy(boxes), f"boxes_out_{k}": torch.from_numpy(apply_boxes(pred, boxes)),
                    f"mask_{k}": torch.from_numpy(mask), f"box_{k}": torch.from_numpy(np.asarray(get_box(mask), dtype=np.float64))})
        mine = D.postprocess_masks(lg.double(), small, (H, W), FRAME)
        print(f"{H}x{W}: post {tuple(post.shape)} restatement max|d| {float((mine - post).abs().max()):.2e}  box {out[f'box_{k}'].tolist()}")
    path = os.path.join(HERE, "ref_sam_decoder.safetensors")
    save_file(out, path)
    print("wrote ref_sam_decoder.safetensors", os.path.getsize(path) >> 10, "KiB")


if __name__ == "__main__":
    main()

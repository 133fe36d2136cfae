#!/usr/bin/env python
"""Time of the native SAM prompt encoder + mask decoder (es_sam_decoder through edgestyle_amd.sam.NativeSamMaskDecoder)
at the real widths - embed 256, 8 heads, mlp 2048, 64 x 64 grid, prompt frame 1024 - against the fp32 restatement on the host's CPU threads.

    python tools/sam_decoder_bench.py [--out profiles/sam_decoder.txt] [--threads 16]

Native: device events around one call on an otherwise idle stream, 5 warm-up calls, then 20 timed ones: median and range, fp16 and bf16:
one predict (box prompt, single mask, photo 1024 x 768), and the five-decode chain of one photo (a point-prompted multimask decode, its box
by es_mask_bbox, four box-prompted decodes), encode and create_sam_images left out.  One predict is ONE library call (es_sam_predict issues its launches from C++); the wall time per call, the
driver's three output allocations included, is reported next to the device time.  Host: tests/sam_dec_ref.py in fp32, one decode +
postprocess_masks, median of 3.  Weights are seeded random numbers under
segment_anything's key names: the time does not depend on them.  The measured section is appended to --out below its hand-written head."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edgestyle_amd import masks as MK                      # noqa: E402
from edgestyle_amd.sam import NativeSamMaskDecoder                   # noqa: E402
from tests import sam_dec_ref as D                                   # noqa: E402

MARK = "## measured by tools/sam_decoder_bench.py\n"
SIZE = (1024, 768)


def timed(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms), statistics.median(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_decoder.txt"))
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.set_num_threads(args.threads)
    cfg = D.REAL
    sds = [D.random_state_dict(cfg, seed) for seed in range(1, 6)]
    new = D.preprocess_shape(SIZE[0], SIZE[1], cfg["frame"])
    emb = torch.randn(1, cfg["embed_dim"], cfg["grid"], cfg["grid"], generator=torch.Generator().manual_seed(9)).to("cuda")
    box = np.array([[100.0, 150.0, 600.0, 900.0]])
    pts = np.array([[[380.0, 300.0], [300.0, 500.0], [450.0, 700.0]]])
    lab = np.ones((1, 3), np.int32)
    lines = [MARK, f"{torch.cuda.get_device_name(0)}; SAM prompt encoder + mask decoder, embed 256, depth 2, 64 x 64 grid, "
                   f"{sum(v.numel() for v in sds[0].values()) / 1e6:.2f} M parameters, photo {SIZE[0]} x {SIZE[1]}; device events, 5 warm-up + 20 timed "
                   "calls: median (min .. max), then the wall time per call\n"]
    for dtype, name in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        decs = [NativeSamMaskDecoder(sd, dtype, "cuda", max_n=1) for sd in sds]
        if name == "fp16":
            lines.append(f"  arena of one decoder for one image: {decs[0].arena_bytes / 2 ** 20:.1f} MiB\n")

        def one():
            return decs[1].predict(emb, new, SIZE, boxes=box, multimask=False)

        def chain():
            m, _, _ = decs[0].predict(emb, new, SIZE, pts, lab, None, True)
            b = MK.get_box(m[:, 0])
            return [d.predict(emb, new, SIZE, boxes=b, multimask=False) for d in decs[1:]]
        med, lo, hi, wall = timed(one)
        lines.append(f"  predict (box, single mask)   {name}: {med:7.3f} ms ({lo:.3f} .. {hi:.3f})   wall {wall:.3f} ms\n")
        med, lo, hi, wall = timed(chain)
        lines.append(f"  five-decode chain of a photo {name}: {med:7.3f} ms ({lo:.3f} .. {hi:.3f})   wall {wall:.3f} ms\n")
    dec = D.Dec(cfg, sds[1], "fp32")
    fb = torch.from_numpy(D.apply_coords(box.reshape(-1, 2, 2), SIZE, new).reshape(-1, 4).astype(np.float32))
    eh = emb.cpu()

    def host_once():
        low, _ = dec.decode(eh, boxes=fb, multimask=False)
        return D.postprocess_masks(low, new, SIZE) > 0
    host_once()
    host = []
    for _ in range(3):
        t = time.perf_counter()
        host_once()
        host.append((time.perf_counter() - t) * 1e3)
    lines.append(f"  fp32 restatement, {args.threads} CPU threads, one predict: {statistics.median(host):.0f} ms ({min(host):.0f} .. {max(host):.0f}), median of 3\n")
    head = ""
    if os.path.exists(args.out):
        head = open(args.out).read().split(MARK)[0]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + "".join(lines))
    print("".join(lines))


if __name__ == "__main__":
    main()

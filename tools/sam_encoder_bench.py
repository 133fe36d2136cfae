#!/usr/bin/env python
"""Time of the native EfficientViT-SAM image encoder (es_sam_encode / es_sam_encode_u8) for the model the reference loads - L2 at
512 x 512 - against the reference-defined network in fp32 on the host's CPU threads.

    python tools/sam_encoder_bench.py [--out profiles/sam_encoder.txt] [--model l2] [--threads 16]

Native: device events around one call on an otherwise idle stream, 5 warm-up calls, then 20 timed ones: median and range, n = 1 and n = 3
(the three photos of a request), fp16 and bf16; es_sam_encode_u8 of three 768 x 1024 photos as well (the resize and the normalisation
included).  Host: tests/sam_ref.py's restatement of the reference's classes in fp32 (the reference tree is not needed), median of 3.
Weights are seeded random numbers under the reference's key names (tests/sam_ref.py::random_state_dict): the time does not depend on
them.  The measured section is appended to --out below its hand-written head, replacing an earlier measured section."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edgestyle_amd.sam import NativeSamImageEncoder, sam_config      # noqa: E402
from tests import sam_ref as R                                       # noqa: E402

MARK = "## measured by tools/sam_encoder_bench.py\n"


def timed(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_encoder.txt"))
    ap.add_argument("--model", default="l2", choices=sorted(R.MODELS))
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.set_num_threads(args.threads)
    cfg = R.model_config(args.model)
    sd = R.random_state_dict(cfg, seed=1)
    lines = [MARK, f"{torch.cuda.get_device_name(0)}; EfficientViT-SAM {args.model.upper()} image encoder at 512 x 512, "
                   f"{sum(v.numel() for v in sd.values()) / 1e6:.1f} M parameters; device events, 5 warm-up + 20 timed calls: median (min .. max)\n"]
    x3 = torch.cat([R.probe_image(512, seed=s) for s in (21, 22, 23)]).to("cuda")
    rng = np.random.default_rng(0)
    photos = [torch.from_numpy(rng.integers(0, 256, (1024, 768, 3), dtype=np.uint8)).to("cuda") for _ in range(3)]
    for dtype, name in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        enc = NativeSamImageEncoder.from_state_dict(sd, sam_config(args.model), dtype=dtype, device="cuda", max_n=3)
        out3 = torch.empty((3,) + enc.out_shape, dtype=torch.float32, device="cuda")
        for n in (1, 3):
            med, lo, hi = timed(lambda: enc(x3[:n], out=out3[:n]))
            lines.append(f"  es_sam_encode     {name} n = {n}: {med:7.3f} ms ({lo:.3f} .. {hi:.3f})   {med / n:.3f} ms per image\n")
        med, lo, hi = timed(lambda: enc.encode_u8(photos, out=out3))
        lines.append(f"  es_sam_encode_u8  {name} n = 3: {med:7.3f} ms ({lo:.3f} .. {hi:.3f})   three 1024 x 768 photos; the driver's workspace allocation included\n")
        lines.append(f"  arena for 3 images: {enc.arena_bytes / 2 ** 20:.0f} MiB\n")
        enc.close()
    module = R.RefModule(cfg, sd)
    xh = x3[:1].cpu()
    module(xh)
    host = []
    for _ in range(3):
        t = time.perf_counter()
        module(xh)
        host.append((time.perf_counter() - t) * 1e3)
    lines.append(f"  reference-defined module, fp32, {args.threads} CPU threads, n = 1: {statistics.median(host):.0f} ms ({min(host):.0f} .. {max(host):.0f}), median of 3\n")
    lines.append("  the reference runs that module five times per photo (five predictors): one native pass replaces all five\n")
    head = ""
    if os.path.exists(args.out):
        head = open(args.out).read().split(MARK)[0]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + "".join(lines))
    print("".join(lines))


if __name__ == "__main__":
    main()

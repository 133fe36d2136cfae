"""es_sam_compose at the application's size against the suite's numpy reference on the same inputs (opt-in, no bar set).

  python tools/mask_compose_bench.py [--out profiles/mask_compose.txt] [--size 512] [--counts 1 8] [--runs 20]

Device time: one pair of device events around each call, after warm-up calls of the same shape; min / median / max over --runs.
Host time: tests/mask_ref.create_sam_images (numpy, written step by step as the reference writes it, a Python union-find for the
labels) on a host clock - the suite's own reference, NOT the reference's cv2 / skimage code, which this project does not depend on.  The
results of the two are compared before anything is timed."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edgestyle_amd import ops  # noqa: E402
from tests import mask_ref as R  # noqa: E402


def inputs(H, W, count, seed=7):
    preds, photos = [], []
    for i in range(count):
        s = 1000 * seed + 10 * i
        body = R.blobs(H, W, s + 1, 0.4)
        preds.append((R.blobs(H, W, s, 0.5), body, R.blobs(H, W, s + 2, 0.4) | (body & R.blobs(H, W, s + 3, 0.3)), R.blobs(H, W, s + 4, 0.15)))
        photos.append(np.random.default_rng(seed + 50 + i).integers(0, 256, size=(H, W, 3), dtype=np.uint8))
    return preds, photos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mask_compose_bench measures on the GPU: none is visible")
    H = W = a.size
    lines = [f"es_sam_compose, {H} x {W}, uint8 masks and RGB photos on the device; device {torch.cuda.get_device_name(0)}; "
             f"host threads {torch.get_num_threads()}"]
    for count in a.counts:
        preds, photos = inputs(H, W, count)
        dev_photos = [torch.from_numpy(p).cuda() for p in photos]
        dev_masks = [torch.from_numpy(np.stack([p[k] for p in preds]).astype(np.uint8)).cuda() for k in range(4)]
        ws = torch.empty((ops.mask_workspace_bytes(H, W, count),), dtype=torch.uint8, device="cuda")
        masks = torch.empty((count, 4, H, W), dtype=torch.uint8, device="cuda")
        images = torch.empty((count, 5, H, W, 3), dtype=torch.uint8, device="cuda")
        call = lambda: ops.sam_compose(dev_photos, *dev_masks, masks_out=masks, images_out=images, workspace=ws)  # noqa: E731
        host = []
        for _ in range(a.host_runs):
            t0 = time.perf_counter()
            ref = [R.create_sam_images(p, *m) for p, m in zip(photos, preds)]
            host.append((time.perf_counter() - t0) * 1e3)
        call()
        torch.cuda.synchronize()
        same = all(np.array_equal(images[i, k].cpu().numpy(), ref[i][0][k]) for i in range(count) for k in range(5)) and \
            all(np.array_equal(masks[i, k].cpu().numpy().astype(bool), ref[i][1][k]) for i in range(count) for k in range(4))
        if not same:
            sys.exit(f"count {count}: the device result differs from the reference; nothing is timed")
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        dev = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            dev.append(e0.elapsed_time(e1))
        lines.append(f"count {count}: es_sam_compose, device events: min {min(dev):.3f}  median {statistics.median(dev):.3f}  "
                     f"max {max(dev):.3f} ms over {len(dev)} runs; workspace {ws.numel() / 2**20:.1f} MiB; results equal the reference")
        lines.append(f"count {count}: tests/mask_ref.create_sam_images (numpy + Python union-find), host clock: min {min(host):.1f}  "
                     f"median {statistics.median(host):.1f}  max {max(host):.1f} ms over {len(host)} runs")
        lines.append(f"count {count}: ratio of medians, host reference / device call: {statistics.median(host) / statistics.median(dev):.0f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

"""es_person_crop_u8 and es_pose_draw at the application's sizes against Pillow and the suite's Python reference (opt-in, no bar set).

  python tools/pose_crop_bench.py [--out profiles/pose_crop.txt] [--counts 1 3] [--runs 20]

Device time: one pair of device events around each call, after warm-up calls of the same shape; min / median / max over --runs.
Host time: Pillow's resize(LANCZOS) + crop on the same photos (the reference's own two lines, where Pillow imports) and
tests/pose_ref.draw (numpy int64, the suite's restatement of the drawing rule - NOT the reference's cv2 code, which this project does not
depend on) on a host clock, median of --host-runs.  The results are compared before anything is timed.  Also reports the PSNR / IoU of
the drawing rule against the reference's own three renderings (tests/golden/ref_pose.safetensors)."""
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
from tests import pose_ref as R  # noqa: E402

PHOTO_H, PHOTO_W, CANVAS = 768, 1024, 512
BOX = (300.0, 60.0, 720.0, 740.0)


def device_times(call, runs):
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def host_times(call, runs):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def fmt(v, unit="ms"):
    return f"min {min(v):.3f}  median {statistics.median(v):.3f}  max {max(v):.3f} {unit} over {len(v)} runs"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pose_crop_bench measures on the GPU: none is visible")
    fx = R.fixture()
    lines = [f"es_person_crop_u8 ({PHOTO_H} x {PHOTO_W} photos -> {CANVAS} x {CANVAS}) and es_pose_draw ({CANVAS} x {CANVAS} canvases); "
             f"device {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}"]
    host_draw = R.draw_host(np.stack(fx["kp"]), CANVAS, CANVAS)
    for i, name in enumerate(R.POSES):
        psnr, iou = R.psnr_iou(host_draw[i], fx["jpg"][i])
        lines.append(f"drawing rule against the reference's rendering of {name}: PSNR {psnr:.2f} dB, IoU {iou:.4f} (condition: >= 34.0 dB, >= 0.92)")
    for count in a.counts:
        photos = [np.random.default_rng(70 + i).integers(0, 256, size=(PHOTO_H, PHOTO_W, 3), dtype=np.uint8) for i in range(count)]
        boxes = [tuple(v + 7.5 * i for v in BOX) for i in range(count)]
        dev_photos = [torch.from_numpy(p).cuda() for p in photos]
        out = torch.empty((count, CANVAS, CANVAS, 3), dtype=torch.uint8, device="cuda")
        need = ops.L.load().es_person_crop_u8_workspace_bytes(ops.image_descriptors(dev_photos), count,
                                                             (ops.C.c_double * (4 * count))(*[v for b in boxes for v in b]))
        ws = torch.empty((max(need, 1),), dtype=torch.uint8, device="cuda")
        crop = lambda: ops.person_crop_u8(dev_photos, boxes, out=out, workspace=ws)  # noqa: E731
        crop()
        torch.cuda.synchronize()
        geoms = [R.crop_fit(PHOTO_H, PHOTO_W, b) for b in boxes]
        pillow = None
        if R.have_pillow():
            from PIL import Image
            pil_photos = [Image.fromarray(p) for p in photos]

            def pillow():
                return [im.resize((g[0], g[1]), Image.Resampling.LANCZOS).crop((g[2], g[3], g[2] + CANVAS, g[3] + CANVAS))
                        for im, g in zip(pil_photos, geoms)]
            ref = [np.asarray(r) for r in pillow()]
        else:
            ref = [R.processed_image(p, b) for p, b in zip(photos, boxes)]
        if not all(np.array_equal(out[i].cpu().numpy(), ref[i]) for i in range(count)):
            sys.exit(f"count {count}: the device crop differs from the reference; nothing is timed")
        dev = device_times(crop, a.runs)
        lines.append(f"count {count}: es_person_crop_u8, device events: {fmt(dev)}; workspace {need / 2**20:.2f} MiB; bytes equal "
                     f"{'Pillow' if pillow else 'the integer reference'}'s")
        if pillow:
            host = host_times(pillow, a.host_runs)
            lines.append(f"count {count}: Pillow resize(LANCZOS) + crop, host clock: {fmt(host)}")
            lines.append(f"count {count}: ratio of medians, Pillow / device call: {statistics.median(host) / statistics.median(dev):.0f}")

        kp_host = np.stack([fx["kp"][i % 3] for i in range(count)])
        kp = torch.from_numpy(kp_host).cuda()
        canvas = torch.empty((count, CANVAS, CANVAS, 3), dtype=torch.uint8, device="cuda")
        draw = lambda: ops.pose_draw(kp, CANVAS, CANVAS, out=canvas)  # noqa: E731
        draw()
        torch.cuda.synchronize()
        host = host_times(lambda: [R.draw(k, CANVAS, CANVAS) for k in kp_host], a.host_runs)
        if not all(np.array_equal(canvas[i].cpu().numpy(), R.draw(kp_host[i], CANVAS, CANVAS)) for i in range(count)):
            sys.exit(f"count {count}: the device drawing differs from the reference; nothing is timed")
        dev = device_times(draw, a.runs)
        lines.append(f"count {count}: es_pose_draw, device events: {fmt(dev)}; results equal tests/pose_ref.draw")
        lines.append(f"count {count}: tests/pose_ref.draw (numpy int64), host clock: {fmt(host)}")
        lines.append(f"count {count}: ratio of medians, host reference / device call: {statistics.median(host) / statistics.median(dev):.0f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

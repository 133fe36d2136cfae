"""The JPEG encoder at the application's sizes against Pillow (opt-in, no bar set).

  python tools/jpeg_encode_bench.py [--out profiles/jpeg_encode.txt] [--runs 20]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/jpeg_encode_bench.py --loop 200      (a run of its own: the eight launches' split)
  python tools/jpeg_encode_bench.py --kernel-stats DIR/.../*_kernel_stats.csv (or *_results.db) --out profiles/jpeg_encode.txt --append

The images: one 1024 x 768 and one 512 x 512, smooth gradients plus noise, quality 75, 4:2:0 (Pillow's defaults).  Device time: one pair
of device events around es_jpeg_encode_u8 (buffers allocated once), after warm-up calls of the same shape; min / median / max over --runs,
for one image and for three in one call.  Host time (host clock): the encode followed by the download of the lengths and of the finished
files; and the reference's route on the same host: the download of the RGB bytes + Image.fromarray(..).save(BytesIO(), "JPEG"), median
of 3.  The files are compared with the host twin's (and with Pillow's where it imports) before anything is timed."""
import argparse
import csv
import ctypes as C
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edgestyle_amd import jpeg as J, lib as L, ops  # noqa: E402
from tests import jpeg_ref as R  # noqa: E402

SIZES = {"1024x768": (1024, 768), "512x512": (512, 512)}
DEV = "cuda"
KERNELS = ("jpeg_fdct_kernel", "jpeg_enc_length_kernel", "jpeg_enc_scan_kernel", "jpeg_enc_place_kernel", "jpeg_enc_emit_kernel",
           "jpeg_enc_count_kernel", "jpeg_enc_scan2_kernel", "jpeg_enc_scatter_kernel")


def image(w, h, i):
    g = np.random.default_rng(70 + i)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([xx * 255 // (w - 1), yy * 255 // (h - 1), (xx + 2 * yy + 40 * i) // 12 % 256], axis=2)
    return np.clip(a + g.integers(-10, 11, size=a.shape), 0, 255).astype(np.uint8)


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


class Prepared:
    """everything one call needs, allocated once"""

    def __init__(self, arrays):
        self.arrays = arrays
        self.images = [torch.from_numpy(a).to(DEV) for a in arrays]
        self.params = J.encode_params()
        self.out, self.lengths = ops.jpeg_encode_u8(self.images, self.params)
        lib = L.load()
        infos = ops.jpeg_encode_infos("bench", ops.jpeg_image_descs("bench", self.images), self.params)
        self.ws_bytes = int(lib.es_jpeg_encode_workspace_bytes(infos, len(arrays), C.byref(self.params)))
        self.ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()

    def encode(self):
        ops.jpeg_encode_u8(self.images, self.params, out=self.out, lengths=self.lengths, workspace=self.ws)

    def files(self):
        self.encode()
        sizes = [int(k) for k in self.lengths.cpu().view(torch.int32).tolist()]                  # waits for the stream
        return [o[:k].cpu().numpy().tobytes() for o, k in zip(self.out, sizes)]

    def pillow_route(self):
        from PIL import Image
        out = []
        for t in self.images:
            buf = io.BytesIO()
            Image.fromarray(t.cpu().numpy()).save(buf, "JPEG")
            out.append(buf.getvalue())
        return out


def kernel_stats(path):
    """the eight kernels' rows of a rocprofv3 --kernel-trace --stats table"""
    lines, total = [], 0.0
    if path.endswith(".db"):                              # a rocprofv3 that writes its results as an SQLite database
        import sqlite3
        q = "select name, count(*), avg(end - start), min(end - start), max(end - start) from kernels group by name"
        rows = [dict(Name=r[0], Calls=r[1], AverageNs=r[2], MinNs=r[3], MaxNs=r[4]) for r in sqlite3.connect(path).execute(q)]
    else:
        with open(path, newline="") as f:
            rows = list(csv.DictReader(f))
    for k in KERNELS:
        for row in rows:
            if k in row.get("Name", ""):
                avg = float(row.get("AverageNs", "nan")) / 1e3
                total += avg
                lines.append(f"rocprofv3 kernel stats, {k}: {row.get('Calls')} calls, average {avg:.1f} us, "
                             f"min {float(row.get('MinNs', 'nan')) / 1e3:.1f} us, max {float(row.get('MaxNs', 'nan')) / 1e3:.1f} us")
    lines.append(f"rocprofv3 kernel stats, the eight kernels together: {total:.1f} us per call (one 1024 x 768 image)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=9)
    ap.add_argument("--loop", type=int, default=0, help="only run es_jpeg_encode_u8 of one 1024 x 768 image this many times (under a profiler)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel-stats CSV of a --loop run: report the kernels' times")
    a = ap.parse_args()
    lines = []
    if a.kernel_stats:
        lines = kernel_stats(a.kernel_stats)
    elif a.loop:
        p = Prepared([image(1024, 768, 0)])
        for _ in range(a.loop):
            p.encode()
        torch.cuda.synchronize()
        return
    else:
        lines.append(f"JPEG encode: gradients plus noise, quality 75, 4:2:0 (Pillow's defaults); device {torch.cuda.get_device_name(0)}; "
                     f"host threads {torch.get_num_threads()}; 8 launches per call")
        for label, (w, h) in SIZES.items():
            for count in (1, 3):
                arrays = [image(w, h, i) for i in range(count)]
                p = Prepared(arrays)
                files = p.files()
                assert files == J.encode_host(arrays), "the device's files are not the host twin's"
                same = "bytes equal the host twin's"
                if R.have_pillow():
                    assert files == p.pillow_route(), "the device's files are not Pillow's"
                    same = "bytes equal Pillow's and the host twin's"
                tag = f"{label} x {count}"
                lines.append(f"{tag}: {sum(x.nbytes for x in arrays) / 2**20:.2f} MiB of RGB in, {sum(len(f) for f in files)} bytes of files out, "
                             f"{p.ws_bytes / 2**20:.2f} MiB of workspace; {same}")
                dev = device_times(p.encode, a.runs)
                lines.append(f"{tag}: es_jpeg_encode_u8 (8 launches), device events: {fmt(dev)}")
                whole = host_times(p.files, a.host_runs)
                lines.append(f"{tag}: es_jpeg_encode_u8 + download of lengths and files, host clock: {fmt(whole)}")
                if R.have_pillow():
                    ref = host_times(p.pillow_route, 3)
                    lines.append(f"{tag}: download of the RGB bytes + Image.fromarray(..).save(BytesIO(), 'JPEG'), host clock: {fmt(ref)}")
                    lines.append(f"{tag}: ratio of medians, Pillow route / device route: {statistics.median(ref) / statistics.median(whole):.2f}")
                else:
                    lines.append(f"{tag}: Pillow does not import here: its route was not measured")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

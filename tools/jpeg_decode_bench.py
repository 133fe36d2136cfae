"""The JPEG decoder at the application's size against Pillow (opt-in, no bar set).

  python tools/jpeg_decode_bench.py [--out profiles/jpeg_decode.txt] [--counts 1 3] [--runs 20]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/jpeg_decode_bench.py --loop 200      (a run of its own: the two launches' split)
  python tools/jpeg_decode_bench.py --kernel-stats DIR/.../*_kernel_stats.csv --out profiles/jpeg_decode.txt --append

The photo: 1024 x 768, 4:2:0, quality 90, smooth gradients plus noise, encoded by Pillow where it imports; otherwise the fixture's
512 x 512 photo.  Device time: one pair of device events around es_jpeg_reconstruct, after warm-up calls of the same shape; min / median /
max over --runs.  Host time (host clock, the device calls followed by a synchronise): es_jpeg_entropy_decode_host per photo, the upload
of coefficients and tables from pinned memory, the whole es_jpeg_decode_u8, and Pillow's open + convert + asarray + upload on the same
host.  The results are compared with Pillow's before anything is timed."""
import argparse
import csv
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

PHOTO_H, PHOTO_W, QUALITY = 768, 1024, 90
DEV = "cuda"


def photos(count):
    """-> (list of JPEG byte strings, list of Pillow's pixels or None, a description)"""
    if R.have_pillow():
        raws = []
        for i in range(count):
            g = np.random.default_rng(50 + i)
            yy, xx = np.mgrid[0:PHOTO_H, 0:PHOTO_W]
            a = np.stack([xx * 255 // (PHOTO_W - 1), yy * 255 // (PHOTO_H - 1), (xx + 2 * yy + 40 * i) // 12 % 256], axis=2)
            a = np.clip(a + g.integers(-10, 11, size=a.shape), 0, 255).astype(np.uint8)
            raws.append(R.encode(a, "420", QUALITY))
        return raws, [R.pillow_rgb(r) for r in raws], f"{PHOTO_W} x {PHOTO_H}, 4:2:0, quality {QUALITY}, gradients plus noise, Pillow's encoder"
    fx = R.fixture()
    return [fx["photo"]] * count, None, "the fixture's 512 x 512 4:2:0 photo (Pillow does not import here)"


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
    """everything one count needs, allocated once"""

    def __init__(self, raws):
        self.raws, n = raws, len(raws)
        self.infos = (L.JpegInfo * n)(*[J.info(r) for r in raws])
        parts = [J.entropy_decode(r) for r in raws]
        self.host = [(torch.from_numpy(p[1]).pin_memory(), torch.from_numpy(p[2].view(np.int16).reshape(-1).copy()).pin_memory()) for p in parts]
        self.coeffs = [h[0].to(DEV) for h in self.host]
        self.qtables = [h[1].to(DEV) for h in self.host]
        lib = L.load()
        self.ws = torch.empty((int(lib.es_jpeg_reconstruct_workspace_bytes(self.infos, n)),), dtype=torch.uint8, device=DEV)
        stage = int(lib.es_jpeg_decode_staging_bytes(self.infos, n))
        self.stage_host = torch.empty((stage,), dtype=torch.uint8).pin_memory()
        self.stage_dev = torch.empty((stage,), dtype=torch.uint8, device=DEV)
        self.out = [torch.empty((i.height, i.width, 3), dtype=torch.uint8, device=DEV) for i in self.infos]
        self.coeff_bytes = sum(p[1].nbytes for p in parts)
        self.out_bytes = sum(o.numel() for o in self.out)

    def reconstruct(self):
        ops.jpeg_reconstruct(self.infos, self.coeffs, self.qtables, out=self.out, workspace=self.ws)

    def entropy(self):
        for r, i in zip(self.raws, self.infos):
            J.entropy_decode(r, i)

    def upload(self):
        for (hc, hq), dc, dq in zip(self.host, self.coeffs, self.qtables):
            dc.copy_(hc, non_blocking=True)
            dq.copy_(hq, non_blocking=True)
        torch.cuda.synchronize()

    def whole(self):
        ops.jpeg_decode_u8(self.raws, self.infos, DEV, out=self.out, staging_host=self.stage_host, staging_dev=self.stage_dev, workspace=self.ws)
        torch.cuda.synchronize()


def pillow_route(raws):
    import warnings
    from PIL import Image
    warnings.filterwarnings("ignore", message="The given NumPy array is not writable")      # asarray's view of Pillow's buffer is only read
    out = [torch.from_numpy(np.asarray(Image.open(io.BytesIO(r)).convert("RGB"))).to(DEV) for r in raws]
    torch.cuda.synchronize()
    return out


def kernel_stats(path):
    """the two kernels' rows of a rocprofv3 --kernel-trace --stats table"""
    lines = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for k in ("jpeg_idct_kernel", "jpeg_colour_kernel"):
                if k in name:
                    lines.append(f"rocprofv3 kernel stats, {k}: {row.get('Calls')} calls, average {float(row.get('AverageNs', 'nan')) / 1e3:.1f} us, "
                                 f"min {float(row.get('MinNs', 'nan')) / 1e3:.1f} us, max {float(row.get('MaxNs', 'nan')) / 1e3:.1f} us")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--host-runs", type=int, default=9)
    ap.add_argument("--loop", type=int, default=0, help="only run es_jpeg_reconstruct of one photo this many times (under a profiler)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel-stats CSV of a --loop run: report the two kernels' times")
    a = ap.parse_args()
    lines = []
    if a.kernel_stats:
        lines = kernel_stats(a.kernel_stats)
    elif a.loop:
        p = Prepared(photos(1)[0])
        for _ in range(a.loop):
            p.reconstruct()
        torch.cuda.synchronize()
        return
    else:
        assert torch.cuda.is_available(), "this measurement needs the GPU"
        raws, want, what = photos(max(a.counts))
        lines.append(f"JPEG decode: {what}; {len(raws[0])} bytes per file; device {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}")
        for n in a.counts:
            p = Prepared(raws[:n])
            p.whole()
            twin = J.decode_host(raws[0])
            same = all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(p.out, want[:n])) if want else True
            assert same and np.array_equal(p.out[0].cpu().numpy(), twin), "the device result differs from Pillow's or from the host twin's"
            tag = f"count {n}:"
            lines.append(f"{tag} {p.coeff_bytes / 2 ** 20:.2f} MiB of coefficients in, {p.out_bytes / 2 ** 20:.2f} MiB of RGB out; bytes equal "
                         f"{'Pillow' + chr(39) + 's and ' if want else ''}the host twin's")
            dev = device_times(p.reconstruct, a.runs)
            lines.append(f"{tag} es_jpeg_reconstruct (two launches), device events: {fmt(dev)}")
            ent, up, whole = host_times(p.entropy, a.host_runs), host_times(p.upload, a.host_runs), host_times(p.whole, a.host_runs)
            lines.append(f"{tag} es_jpeg_entropy_decode_host, host clock: {fmt(ent)}  ({statistics.median(ent) / n:.3f} ms per photo)")
            lines.append(f"{tag} upload of coefficients and tables from pinned memory + synchronise, host clock: {fmt(up)}")
            lines.append(f"{tag} es_jpeg_decode_u8 + synchronise (parse, decode, upload, reconstruct), host clock: {fmt(whole)}")
            if want:
                pil = host_times(lambda: pillow_route(raws[:n]), 3)
                lines.append(f"{tag} Pillow open + convert + asarray + upload + synchronise, host clock: {fmt(pil)}")
                lines.append(f"{tag} ratio of medians, Pillow route / es_jpeg_decode_u8: {statistics.median(pil) / statistics.median(whole):.2f}")
            share = statistics.median(ent) / statistics.median(whole)
            lines.append(f"{tag} the host Huffman decoding is {100 * share:.0f} % of the whole call, the two launches {100 * statistics.median(dev) / statistics.median(whole):.0f} %")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

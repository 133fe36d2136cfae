"""The JPEG decoder at the application's size against Pillow (opt-in, no bar set).

  python tools/jpeg_decode_bench.py [--out profiles/jpeg_decode.txt] [--counts 1 3] [--runs 20]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/jpeg_decode_bench.py --loop 200      (a run of its own: the two launches' split)
  python tools/jpeg_decode_bench.py --kernel-stats DIR/.../*_kernel_stats.csv --out profiles/jpeg_decode.txt --append

The photo: 1024 x 768, 4:2:0, quality 90, smooth gradients plus noise, encoded by Pillow where it imports; otherwise the fixture's
512 x 512 photo.  Device time: one pair of device events around es_jpeg_reconstruct, after warm-up calls of the same shape; min / median /
max over --runs.  Host time (host clock, the device calls followed by a synchronise): es_jpeg_entropy_decode_host per photo, the upload
of coefficients and tables from pinned memory, the whole es_jpeg_decode_u8, and Pillow's open + convert + asarray + upload on the same
host.  The results are compared with Pillow's before anything is timed.

  python tools/jpeg_decode_bench.py --device-entropy [--parent-lib PATH/libedgestyle_hip.so] [--subseq 0 64 256] --out profiles/jpeg_entropy_device.txt
The opt-in Huffman decoding on the device (csrc/jpeg_entropy.hip) for the same files: es_jpeg_entropy_decode alone by device events
(median of --runs), es_jpeg_decode_dev_u8 + synchronise by host clock (median of --host-runs), the synchronise rounds the host twin
counts, and beside them es_jpeg_decode_u8 of this build and, with --parent-lib, of a library built from the parent commit, in the same
session.  The coefficients are compared with the serial decoder's before anything is timed."""
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

PHOTO_H, PHOTO_W, QUALITY = 768, 1024, 90
DEV = "cuda"


def photos(count, kind="generated"):
    """-> (list of JPEG byte strings, list of Pillow's pixels or None, a description)"""
    if kind == "fixture":
        return [R.fixture()["photo"]] * count, None, "the fixture's 512 x 512 4:2:0 photo (a figure on a flat background)"
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


class DevicePrepared:
    """the buffers of the device-entropy legs for one count, allocated once"""

    def __init__(self, raws, infos, subseq):
        self.raws, self.infos, self.subseq, n = raws, infos, subseq, len(raws)
        parts = [J.scan_prepare(r) for r in raws]
        self.files = [torch.from_numpy(np.frombuffer(r, dtype=np.uint8).copy()).to(DEV) for r in raws]
        self.segments = [torch.from_numpy(p[1].reshape(-1)).to(DEV) for p in parts]
        self.tables = [torch.from_numpy(p[2]).to(DEV) for p in parts]
        lib = L.load()
        self.coeffs = [torch.empty((int(lib.es_jpeg_coeff_count(infos[i])),), dtype=torch.int16, device=DEV) for i in range(n)]
        self.status = torch.zeros((n,), dtype=torch.int32, device=DEV)
        self.ews = torch.empty((int(lib.es_jpeg_entropy_decode_workspace_bytes(infos, n)),), dtype=torch.uint8, device=DEV)
        self.ws = torch.empty((int(lib.es_jpeg_reconstruct_workspace_bytes(infos, n)),), dtype=torch.uint8, device=DEV)
        up = C.c_size_t(0)
        stage = int(lib.es_jpeg_decode_dev_staging_bytes(infos, (C.c_size_t * n)(*[len(r) for r in raws]), n, C.byref(up)))
        self.upload_bytes = up.value
        self.stage_host = torch.empty((up.value,), dtype=torch.uint8).pin_memory()
        self.stage_dev = torch.empty((stage,), dtype=torch.uint8, device=DEV)
        self.out = [torch.empty((i.height, i.width, 3), dtype=torch.uint8, device=DEV) for i in infos]

    def entropy(self):
        ops.jpeg_entropy_decode(self.infos, self.files, self.segments, self.tables, self.subseq, coeffs=self.coeffs, status=self.status, workspace=self.ews)

    def whole(self):
        ops.jpeg_decode_dev_u8(self.raws, self.infos, DEV, self.subseq, out=self.out, status=self.status, staging_host=self.stage_host,
                               staging_dev=self.stage_dev, workspace=self.ws)
        torch.cuda.synchronize()


def parent_whole(path, p):
    """es_jpeg_decode_u8 of another build of the library (the parent commit's), on Prepared's buffers"""
    lib = C.CDLL(path)
    name = "es_jpeg_decode_u8"
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = L.SYMBOLS[name]
    n = len(p.raws)
    descs = (L.ImageU8 * n)()
    for i, t in enumerate(p.out):
        descs[i].data, descs[i].height, descs[i].width, descs[i].channels, descs[i].row_stride = t.data_ptr(), t.shape[0], t.shape[1], 3, t.stride(0)
    bp = (C.c_void_p * n)(*[C.cast(C.c_char_p(d), C.c_void_p) for d in p.raws])
    ln = (C.c_size_t * n)(*[len(d) for d in p.raws])

    def call():
        rc = fn(bp, ln, n, descs, C.c_void_p(p.stage_host.data_ptr()), C.c_void_p(p.stage_dev.data_ptr()), p.stage_host.numel(),
                C.c_void_p(p.ws.data_ptr()), p.ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
        torch.cuda.synchronize()
    return call


def device_entropy_lines(a):
    raws, want, what = photos(max(a.counts), a.photo)
    lines = [f"JPEG decode, Huffman decoding on the device (opt-in): {what}; {len(raws[0])} bytes per file; device {torch.cuda.get_device_name(0)}; "
             f"host threads {torch.get_num_threads()}"]
    for n in a.counts:
        p = Prepared(raws[:n])
        tag = f"count {n}:"
        for subseq in a.subseq:
            d = DevicePrepared(raws[:n], p.infos, subseq)
            d.entropy()
            d.whole()
            assert d.status.cpu().tolist() == [0] * n
            for i in range(n):
                assert np.array_equal(d.coeffs[i].cpu().numpy(), J.entropy_decode(raws[i])[1]), "the device coefficients differ from the serial decoder's"
                assert want is None or np.array_equal(d.out[i].cpu().numpy(), want[i]), "the device result differs from Pillow's"
            rounds = [J.entropy_decode_parallel_host(r, 1024, subseq)[4] for r in raws[:n]]
            nseg = [len(J.scan_prepare(r)[1]) for r in raws[:n]]
            sub = f"subseq_bytes {subseq}" + (" (the default, 128)" if subseq == 0 else "")
            lines.append(f"{tag} {sub}: {d.upload_bytes / 2 ** 20:.2f} MiB uploaded (files, segments, tables); segments per file {nseg}; synchronise rounds "
                         f"(host twin, 1024 decoders) {rounds}; coefficients equal the serial decoder's")
            lines.append(f"{tag} {sub}: es_jpeg_entropy_decode (memset + two launches), device events: {fmt(device_times(d.entropy, a.runs))}")
            lines.append(f"{tag} {sub}: es_jpeg_decode_dev_u8 + synchronise (parse, prepare, upload, decode, reconstruct), host clock: "
                         f"{fmt(host_times(d.whole, a.host_runs))}")
        p.whole()
        whole = host_times(p.whole, a.host_runs)
        lines.append(f"{tag} es_jpeg_decode_u8 + synchronise of this build (the default route, host Huffman decoding), host clock: {fmt(whole)}")
        if a.parent_lib:
            call = parent_whole(a.parent_lib, p)
            call()
            lines.append(f"{tag} es_jpeg_decode_u8 + synchronise of the parent commit's build, host clock: {fmt(host_times(call, a.host_runs))}")
    return lines


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
    ap.add_argument("--device-entropy", action="store_true", help="the legs of the opt-in Huffman decoding on the device")
    ap.add_argument("--subseq", type=int, nargs="+", default=[0], help="subseq_bytes values of the device-entropy legs")
    ap.add_argument("--photo", choices=["generated", "fixture"], default="generated", help="the device-entropy legs' file: the generated 1024 x 768 one or "
                    "the fixture's 512 x 512 photo")
    ap.add_argument("--parent-lib", default=None, help="a libedgestyle_hip.so built from the parent commit: its es_jpeg_decode_u8 is timed beside")
    a = ap.parse_args()
    lines = []
    if a.device_entropy:
        assert torch.cuda.is_available(), "this measurement needs the GPU"
        lines = device_entropy_lines(a)
    elif a.kernel_stats:
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

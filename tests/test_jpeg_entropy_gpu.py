"""Huffman decoding on the GPU (csrc/jpeg_entropy.hip): es_jpeg_entropy_decode against the serial host decoder
es_jpeg_entropy_decode_host on the fixture files, the real photo and files written by es_jpeg_encode_host; images of different sizes,
samplings and segment counts in one call; poisoned guard regions; the truncation / corruption sweep against the host twin; graph
capture; es_jpeg_decode_dev_u8, jpeg.decode(entropy="device") and examples/jpeg_host.cpp --device-entropy.  Every comparison is an
equality.  tests/test_jpeg_entropy_cpu.py holds the twin (the same __host__ __device__ code) against the serial decoder without a GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from edgestyle_amd import jpeg as J, lib as L, ops
from tests import jpeg_ref as R
from tests import test_jpeg_entropy_cpu as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0x5A
CASES = R.cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_inputs(raws):
    """-> (JpegInfo array, file tensors, segment tensors, table tensors) of files the prepare step accepts"""
    parts = [K.prepare(raw) for raw in raws]
    assert all(p[3] is None for p in parts), [p[3] for p in parts]
    infos = (L.JpegInfo * len(raws))(*[p[0] for p in parts])
    files = [torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(DEV) for raw in raws]
    segments = [torch.from_numpy(p[1].view(np.int32).reshape(-1)).to(DEV) for p in parts]
    tables = [torch.from_numpy(p[2]).to(DEV) for p in parts]
    return infos, files, segments, tables


def _decode(raws, subseq=0):
    """-> (a list of numpy coefficient arrays, the status words as a list)"""
    infos, files, segments, tables = _device_inputs(raws)
    coeffs, status = ops.jpeg_entropy_decode(infos, files, segments, tables, subseq)
    torch.cuda.synchronize()
    return [c.cpu().numpy() for c in coeffs], status.cpu().tolist()


def _equals_serial(names, raws, subseq):
    got, status = _decode(raws, subseq)
    assert status == [0] * len(raws), [(n, J.status_text(s)) for n, s in zip(names, status) if s]
    for name, raw, g in zip(names, raws, got):
        want, why = K.serial(raw)
        assert want is not None and np.array_equal(g, want), (name, subseq, why, int((g != want).sum()))


@pytest.mark.parametrize("subseq", [0, 4])
@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_the_device_decoder_equals_the_serial_decoder_on_every_fixture_file(sampling, subseq):
    """all files of one sampling in ONE call (more than 16: the call spans two launch groups)"""
    fx = R.fixture()["cases"]
    names = [c[0] for c in CASES if c[3] == sampling]
    assert len(names) > 16
    _equals_serial(names, [fx[n][0] for n in names], subseq)


def test_the_photo_decodes_to_the_serial_coefficients_and_the_fixtures_pixels():
    fx = R.fixture()
    infos, coeffs, qtables, status = J.entropy_decode_device(fx["photo"])
    out = ops.jpeg_reconstruct(infos, coeffs, qtables)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0]
    assert np.array_equal(coeffs[0].cpu().numpy(), K.serial(fx["photo"])[0])
    assert R.sha256(out[0].cpu().numpy()) == fx["photo_sha256"]


@pytest.mark.parametrize("subseq", [0, 4])
def test_the_device_decoder_equals_the_serial_decoder_on_generated_files(subseq):
    """noise at quality 100, smooth content at quality 10, every sampling with restart intervals 0, 1, 2 and mcus_x"""
    gen = K.generated()
    _equals_serial(list(gen), list(gen.values()), subseq)


@pytest.mark.parametrize("subseq", [0, 4])
def test_stray_bytes_before_eoi_and_before_rstn_are_no_error_and_change_no_coefficient(subseq):
    """stray data bytes behind a segment's last block, up to 600 of them (more than two subsequences at 4 bytes and at the default 128):
    status 0 and the serial decoder's coefficients, which are the original file's"""
    names, raws, originals = zip(*K.stray_variants())
    for first in range(0, len(raws), 64):
        _equals_serial(names[first:first + 64], raws[first:first + 64], subseq)
    assert all(np.array_equal(K.serial(r)[0], K.serial(o)[0]) for r, o in zip(raws, originals))


def test_images_of_different_sizes_samplings_and_segment_counts_in_one_call_equal_each_alone():
    fx, gen = R.fixture()["cases"], K.generated()
    raws = [fx["33x18_420_q30"][0], fx["23x37_gray_q100_rst"][0], gen["noise_q100"], fx["17x23_422_q30"][0], gen["33x18_444_ri2"],
            fx["9x5_444_q100_rst"][0], gen["smooth_q10"]]
    assert len({len(K.prepare(r)[1]) for r in raws}) >= 4
    together, status = _decode(raws)
    assert status == [0] * len(raws)
    for k, raw in enumerate(raws):
        alone, st = _decode([raw])
        assert st == [0] and np.array_equal(together[k], alone[0]) and np.array_equal(alone[0], K.serial(raw)[0]), k


@pytest.mark.parametrize("name", ["33x18_420_q30_rst", "23x37_gray_q30", "17x23_422_q100_rst"])
def test_only_the_coefficients_the_workspace_and_the_status_words_change(name):
    raw = R.fixture()["cases"][name][0]
    infos, files, segments, tables = _device_inputs([raw])
    lib = L.load()
    count, need = int(lib.es_jpeg_coeff_count(infos)), int(lib.es_jpeg_entropy_decode_workspace_bytes(infos, 1))
    guard = 4096
    cbuf = torch.full((guard + count + guard,), 0x5A5A, dtype=torch.int16, device=DEV)
    wbuf = torch.full((guard + need + guard,), POISON, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((8 + 1 + 8,), -7, dtype=torch.int32, device=DEV)
    keep = [t.clone() for t in files + segments + tables]
    coeffs, status = ops.jpeg_entropy_decode(infos, files, segments, tables, 0, coeffs=[cbuf[guard:guard + count]], status=sbuf[8:9],
                                             workspace=wbuf[guard:guard + need])
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] and np.array_equal(coeffs[0].cpu().numpy(), K.serial(raw)[0])
    assert bool((cbuf[:guard] == 0x5A5A).all()) and bool((cbuf[guard + count:] == 0x5A5A).all())
    assert bool((wbuf[:guard] == POISON).all()) and bool((wbuf[guard + need:] == POISON).all())
    assert bool((sbuf[:8] == -7).all()) and bool((sbuf[9:] == -7).all())
    assert all(torch.equal(a, b) for a, b in zip(keep, files + segments + tables))
    with pytest.raises(L.EdgeStyleHipError, match="workspace"):
        ops.jpeg_entropy_decode(infos, files, segments, tables, 0, workspace=wbuf[guard:guard + need - 1])
    with pytest.raises(L.EdgeStyleHipError, match="subseq_bytes"):
        ops.jpeg_entropy_decode(infos, files, segments, tables, 3)


def test_the_sweep_is_decided_as_the_twin_decides_it_and_stays_inside_the_buffers():
    """every prefix and every single-byte corruption of one small file that passes the prepare step, 64 variants per call, 4 bytes per
    subsequence: the status is non-zero exactly where the twin's is, the coefficients are the serial decoder's where the file is
    accepted, and the guard values between the coefficient buffers keep their poison.  (Error returns, not faults: the CPU tier runs
    the same variants through the same code first.)"""
    lib = L.load()
    raw = R.fixture()["cases"][R.SWEEP_SOURCE][0]
    variants, dropped = [], 0
    for bad in R.sweep(raw):
        info, segments, tables, refused = K.prepare(bad)
        if refused is None:
            if int(lib.es_jpeg_coeff_count(C.byref(info))) <= K.SWEEP_MAX_COEFFS:      # the CPU tier's own limit
                variants.append(bad)
            else:
                dropped += 1
    print("sweep variants:", len(variants), "left out above", K.SWEEP_MAX_COEFFS, "coefficients:", dropped)
    assert len(variants) > 500
    guard = 64
    accepted = refused = 0
    for first in range(0, len(variants), 64):
        part = variants[first:first + 64]
        infos, files, segments, tables = _device_inputs(part)
        counts = [int(lib.es_jpeg_coeff_count(C.byref(infos[i]))) for i in range(len(part))]
        cbuf = torch.full((guard + sum(c + guard for c in counts),), 0x5A5A, dtype=torch.int16, device=DEV)
        at, views = guard, []
        for c in counts:
            views.append(cbuf[at:at + c])
            at += c + guard
        _, status = ops.jpeg_entropy_decode(infos, files, segments, tables, 4, coeffs=views)
        torch.cuda.synchronize()
        status, host = status.cpu().tolist(), cbuf.cpu().numpy()
        at = guard
        for k, bad in enumerate(part):
            assert (host[at - guard:at] == 0x5A5A).all() and (host[at + counts[k]:at + counts[k] + guard] == 0x5A5A).all(), first + k
            info, seg, tab, _ = K.prepare(bad)
            _, twin_status, _ = K.twin(bad, info, seg, tab, 1024, 4)
            assert (status[k] != 0) == (twin_status != 0), (first + k, status[k], twin_status)
            want, why = K.serial(bad)
            assert (want is None) == (status[k] != 0), (first + k, status[k], why)
            if want is not None:
                assert np.array_equal(host[at:at + counts[k]], want), first + k
                accepted += 1
            else:
                assert J.status_text(status[k])
                refused += 1
            at += counts[k] + guard
    assert accepted > 100 and refused > 10


def test_a_captured_entropy_decode_and_reconstruct_replay_bit_for_bit():
    """two generated files of one geometry: the graph is captured over the first one's bytes and replayed after the second's scan bytes
    and segment table were copied into the same device buffers, and again after the first's came back"""
    a = J.encode_host(R.content(33, 18, "noise", 41, False), quality=60, subsampling="4:2:0", restart_marker_blocks=2)
    b = J.encode_host(R.content(33, 18, "photo", 42, False), quality=60, subsampling="4:2:0", restart_marker_blocks=2)
    assert len(a) != len(b)
    pa, pb = K.prepare(a), K.prepare(b)
    assert bytes(pa[0]) == bytes(pb[0]) and np.array_equal(pa[2], pb[2])
    infos = (L.JpegInfo * 1)(pa[0])
    cap = max(len(a), len(b))
    lib = L.load()
    file = torch.zeros((cap,), dtype=torch.uint8, device=DEV)
    seg = torch.zeros((pa[1].size,), dtype=torch.int32, device=DEV)
    tab = torch.from_numpy(pa[2]).to(DEV)
    qt = J.upload(np.zeros(1, dtype=np.int16), J.entropy_decode(a)[2], DEV)[1]
    assert np.array_equal(J.entropy_decode(a)[2], J.entropy_decode(b)[2])
    coeffs = torch.zeros((int(lib.es_jpeg_coeff_count(infos)),), dtype=torch.int16, device=DEV)
    status = torch.zeros((1,), dtype=torch.int32, device=DEV)
    ws = torch.zeros((int(lib.es_jpeg_entropy_decode_workspace_bytes(infos, 1)),), dtype=torch.uint8, device=DEV)
    rws = torch.zeros((int(lib.es_jpeg_reconstruct_workspace_bytes(infos, 1)),), dtype=torch.uint8, device=DEV)
    out = torch.zeros((18, 33, 3), dtype=torch.uint8, device=DEV)

    def load(raw, parts):
        file.zero_()
        file[:len(raw)].copy_(torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()))
        seg.copy_(torch.from_numpy(parts[1].view(np.int32).reshape(-1)))

    def run():
        ops.jpeg_entropy_decode(infos, [file], [seg], [tab], 0, coeffs=[coeffs], status=status, workspace=ws)
        ops.jpeg_reconstruct(infos, [coeffs], [qt], out=[out], workspace=rws)
    load(a, pa)
    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for raw, parts in ((b, pb), (a, pa)):
        load(raw, parts)
        for t in (coeffs, ws, rws, out):
            t.fill_(POISON)
        status.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0]
        assert np.array_equal(coeffs.cpu().numpy(), K.serial(raw)[0])
        assert np.array_equal(out.cpu().numpy(), J.decode_host(raw))


def test_decode_with_device_entropy_equals_the_default_route_and_pillows_pixels():
    fx = R.fixture()["cases"]
    names = ["33x18_420_q30_rst", "23x37_gray_q30", "17x23_420_q75_opt", "5x3_422_q100_rst", "60x45_420_q90"]
    raws = [fx[n][0] for n in names]
    infos = (L.JpegInfo * len(raws))(*[J.info(r) for r in raws])
    want = ops.jpeg_decode_u8(raws, infos, DEV)                       # es_jpeg_decode_u8
    got, status = ops.jpeg_decode_dev_u8(raws, infos, DEV)            # es_jpeg_decode_dev_u8
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(raws)
    for name, g, w in zip(names, got, want):
        assert torch.equal(g, w) and np.array_equal(g.cpu().numpy(), fx[name][1]), name
    every = [c[0] for c in CASES]
    by_device, by_host = J.decode([fx[n][0] for n in every], entropy="device"), J.decode([fx[n][0] for n in every])
    for name, g, w in zip(every, by_device, by_host):
        assert torch.equal(g, w) and np.array_equal(g.cpu().numpy(), fx[name][1]), name
    single = J.decode(raws[4], entropy="device")
    assert torch.is_tensor(single) and np.array_equal(single.cpu().numpy(), fx[names[4]][1])
    with pytest.raises(L.EdgeStyleHipError, match="truncated"):
        J.decode(raws[0][:-30], entropy="device")                     # refused by the prepare step: no EOI
    cut = raws[4][:-40] + b"\xff\xd9"                                 # the markers are in place, the data is short: a status word
    assert K.serial(cut)[0] is None
    with pytest.raises(L.EdgeStyleHipError, match="status"):
        J.decode(cut, entropy="device")
    with pytest.raises(L.EdgeStyleHipError, match="entropy"):
        J.decode(raws[0], entropy="gpu")


def test_cpp_jpeg_host_with_device_entropy_writes_the_same_ppm(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, libdir = str(tmp_path / "jpeg_host"), os.path.join(ROOT, "edgestyle_amd", "lib")
    c = subprocess.run([hipcc, "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "jpeg_host.cpp"),
                        "-L" + libdir, "-ledgestyle_hip", "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-2000:]
    for name in ("60x45_420_q90", "23x37_gray_q100_rst"):
        raw, want = R.fixture()["cases"][name]
        (tmp_path / "in.jpg").write_bytes(raw)
        outs = []
        for flags in ([], ["--device-entropy"]):
            r = subprocess.run([exe] + flags + [str(tmp_path / "in.jpg"), str(tmp_path / "out.ppm")], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout + r.stderr
            outs.append((tmp_path / "out.ppm").read_bytes())
            (tmp_path / "out.ppm").unlink()
        h, w = want.shape[:2]
        assert outs[0] == outs[1] == b"P6\n%d %d\n255\n" % (w, h) + want.tobytes(), name
    (tmp_path / "bad.jpg").write_bytes(raw[:-40] + b"\xff\xd9")
    r = subprocess.run([exe, "--device-entropy", str(tmp_path / "bad.jpg"), str(tmp_path / "bad.ppm")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and r.stderr and not (tmp_path / "bad.ppm").exists()

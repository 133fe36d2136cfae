"""The JPEG decoder on the GPU (csrc/jpeg.hip): es_jpeg_reconstruct against es_jpeg_reconstruct_host (the same __host__ __device__ integer
code, which tests/test_jpeg_cpu.py holds against Pillow) and against Pillow's pixels in the fixture, images of different sizes in one
call, pitched output in a poisoned buffer, graph capture, es_jpeg_decode_u8, the Python layer (edgestyle_amd/jpeg.py) and the compiled
C++ hosts (examples/jpeg_host.cpp, examples/pose_host.cpp fed a JPEG).  Every comparison is an equality."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from edgestyle_amd import jpeg as J, lib as L, ops
from tests import jpeg_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0xA5
CASES = R.cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _prepared(names):
    """-> (JpegInfo array, device coefficient tensors, device table tensors, host parts) of fixture files"""
    fx = R.fixture()["cases"]
    parts = [J.entropy_decode(fx[n][0]) for n in names]
    infos = (L.JpegInfo * len(names))(*[p[0] for p in parts])
    up = [J.upload(p[1], p[2], DEV) for p in parts]
    return infos, [u[0] for u in up], [u[1] for u in up], parts


def _reconstruct(names, **kw):
    infos, coeffs, qtables, _ = _prepared(names)
    out = ops.jpeg_reconstruct(infos, coeffs, qtables, **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_reconstruct_equals_the_host_twin_and_pillows_pixels_on_every_case(sampling):
    """all files of one sampling in ONE call (more than 16: the call spans two pairs of launches): 1 x 1 up to partial MCUs on both axes,
    quality 30 and 100, restart markers, optimised tables"""
    fx = R.fixture()["cases"]
    names = [c[0] for c in CASES if c[3] == sampling]
    assert len(names) > 16
    infos, coeffs, qtables, parts = _prepared(names)
    got = ops.jpeg_reconstruct(infos, coeffs, qtables)
    torch.cuda.synchronize()
    twin = J.reconstruct_host([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts])
    for name, g, t in zip(names, got, twin):
        g = g.cpu().numpy()
        assert np.array_equal(g, t), (name, int((g != t).sum()))
        assert np.array_equal(g, fx[name][1]), (name, int((g != fx[name][1]).sum()))


def test_a_16_bit_table_and_the_real_photo_decode_to_pillows_pixels():
    fx = R.fixture()
    raw, want = fx["cases"][R.DQT16_SOURCE]
    got = J.decode([R.dqt_to_16_bit(raw), fx["photo"]])
    torch.cuda.synchronize()
    assert np.array_equal(got[0].cpu().numpy(), want)
    photo = got[1].cpu().numpy()
    assert photo.shape == (512, 512, 3) and R.sha256(photo) == fx["photo_sha256"]
    assert np.array_equal(photo, J.decode_host(fx["photo"]))


def test_three_images_of_different_sizes_and_samplings_in_one_call_equal_each_alone():
    names = ["33x18_420_q30", "23x37_gray_q100_rst", "17x23_422_q30", "9x5_444_q100_rst"]
    together = _reconstruct(names)
    fx = R.fixture()["cases"]
    for name, g in zip(names, together):
        alone = _reconstruct([name])[0]
        assert np.array_equal(g, alone) and np.array_equal(g, fx[name][1]), name


@pytest.mark.parametrize("name", ["33x18_420_q30", "17x23_444_q100_rst", "23x37_gray_q30", "16x16_422_q30"])
def test_reconstruct_into_a_pitched_poisoned_buffer_writes_the_pixels_only(name):
    """row stride W * 3 + 5 (rows that are not 4-byte aligned take the byte stores): the row tails, the rows around the image, the guard
    bytes around the workspace all keep the poison"""
    raw, want = R.fixture()["cases"][name]
    h, w = want.shape[:2]
    infos, coeffs, qtables, _ = _prepared([name])
    guard, stride = 4096, w * 3 + 5
    buf = torch.full((guard + h * stride + guard,), POISON, dtype=torch.uint8, device=DEV)
    rows = buf[guard:guard + h * stride].view(h, stride)
    view = rows[:, :w * 3].unflatten(1, (w, 3))
    assert view.stride() == (stride, 3, 1) and view.data_ptr() == buf.data_ptr() + guard
    need = int(L.load().es_jpeg_reconstruct_workspace_bytes(infos, 1))
    wbuf = torch.full((guard + need + guard,), POISON, dtype=torch.uint8, device=DEV)
    ops.jpeg_reconstruct(infos, coeffs, qtables, out=[view], workspace=wbuf[guard:guard + need])
    torch.cuda.synchronize()
    assert np.array_equal(view.cpu().numpy(), want)
    assert bool((rows[:, w * 3:] == POISON).all()) and bool((buf[:guard] == POISON).all()) and bool((buf[guard + h * stride:] == POISON).all())
    assert bool((wbuf[:guard] == POISON).all()) and bool((wbuf[guard + need:] == POISON).all())
    with pytest.raises(L.EdgeStyleHipError, match="workspace"):
        ops.jpeg_reconstruct(infos, coeffs, qtables, out=[view], workspace=wbuf[guard:guard + need - 1])


def test_reconstruct_refuses_outputs_that_do_not_fit_and_unaligned_coefficients():
    infos, coeffs, qtables, _ = _prepared(["9x5_420_q30"])
    lib = L.load()
    need = int(lib.es_jpeg_reconstruct_workspace_bytes(infos, 1))
    ws = torch.zeros((need,), dtype=torch.uint8, device=DEV)
    out = torch.zeros((5, 9, 3), dtype=torch.uint8, device=DEV)
    desc = (L.ImageU8 * 1)()

    def call(data, h, w, ch, stride, cptr):
        desc[0].data, desc[0].height, desc[0].width, desc[0].channels, desc[0].row_stride = data, h, w, ch, stride
        return lib.es_jpeg_reconstruct(infos, 1, (C.c_void_p * 1)(cptr), (C.c_void_p * 1)(qtables[0].data_ptr()), desc, C.c_void_p(ws.data_ptr()),
                                       need, None)
    assert call(out.data_ptr(), 5, 8, 3, 27, coeffs[0].data_ptr()) == -1 and b"size" in lib.es_last_error()
    assert call(out.data_ptr(), 5, 9, 4, 36, coeffs[0].data_ptr()) == -1 and b"channels" in lib.es_last_error()
    assert call(out.data_ptr(), 5, 9, 3, 26, coeffs[0].data_ptr()) == -1 and b"stride" in lib.es_last_error()
    assert call(out.data_ptr(), 5, 9, 3, 27, coeffs[0].data_ptr() + 2) == -1 and b"aligned" in lib.es_last_error()
    assert call(out.data_ptr(), 5, 9, 3, 27, coeffs[0].data_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), R.fixture()["cases"]["9x5_420_q30"][1])


def test_a_captured_reconstruct_replays_bit_for_bit():
    """two files of one geometry: the graph is captured over the first one's coefficients and replayed after the second's were copied
    into the same tensors, and again after the first's came back"""
    fx = R.fixture()["cases"]
    a, b = "33x18_420_q30", "33x18_420_q30_rst"
    ia, ca, qa, _ = _prepared([a])
    ib, cb, qb, _ = _prepared([b])
    ib[0].restart_interval = ia[0].restart_interval        # (the reconstruction does not read it; everything else is equal)
    assert bytes(ia[0]) == bytes(ib[0])
    coeffs, qtables = ca[0].clone(), qa[0].clone()
    out = torch.zeros((18, 33, 3), dtype=torch.uint8, device=DEV)
    ws = torch.zeros((int(L.load().es_jpeg_reconstruct_workspace_bytes(ia, 1)),), dtype=torch.uint8, device=DEV)

    def run():
        ops.jpeg_reconstruct(ia, [coeffs], [qtables], out=[out], workspace=ws)
    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for name, c, q in ((b, cb[0], qb[0]), (a, ca[0], qa[0])):
        coeffs.copy_(c)
        qtables.copy_(q)
        out.fill_(POISON)
        ws.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), fx[name][1]), name


def test_decode_u8_equals_the_two_step_route():
    names = ["33x18_420_q30_rst", "23x37_gray_q30", "17x23_420_q75_opt", "5x3_422_q100_rst", "60x45_420_q90"]
    fx = R.fixture()["cases"]
    raws = [fx[n][0] for n in names]
    infos = (L.JpegInfo * len(raws))(*[J.info(r) for r in raws])
    stage = int(L.load().es_jpeg_decode_staging_bytes(infos, len(raws)))
    host = torch.full((stage + 64,), POISON, dtype=torch.uint8).pin_memory()
    got = ops.jpeg_decode_u8(raws, infos, DEV, staging_host=host[:stage])
    torch.cuda.synchronize()
    two = _reconstruct(names)
    for name, g, t in zip(names, got, two):
        assert np.array_equal(g.cpu().numpy(), t) and np.array_equal(t, fx[name][1]), name
    assert bool((host[stage:] == POISON).all())
    again = J.decode(raws)                                 # the Python layer: its own staging, a list in, a list out
    assert all(torch.equal(x, y) for x, y in zip(again, got))
    with pytest.raises(L.EdgeStyleHipError, match="truncated"):
        J.decode(raws[0][:-30])
    with pytest.raises(L.EdgeStyleHipError, match="staging"):
        ops.jpeg_decode_u8(raws, infos, DEV, staging_host=host[:stage - 16])


def test_decode_returns_what_person_crop_takes_and_the_crop_equals_the_crop_of_pillows_raster(tmp_path):
    raw, raster = R.fixture()["cases"]["60x45_420_q90"]
    assert raster.shape == (45, 60, 3)
    path = tmp_path / "photo.jpg"
    path.write_bytes(raw)
    photo = J.decode(str(path))
    assert photo.dtype == torch.uint8 and photo.is_cuda and tuple(photo.shape) == (45, 60, 3)
    box = (5.0, 4.0, 50.0, 40.0)
    got = ops.person_crop_u8([photo], [box])
    want = ops.person_crop_u8([torch.from_numpy(raster.copy()).to(DEV)], [box])
    torch.cuda.synchronize()
    assert np.array_equal(photo.cpu().numpy(), raster) and torch.equal(got, want) and bool(got.any())


# ---- the C++ hosts -----------------------------------------------------------------------------------------------------------------
def _build(tmp_path, name):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, libdir = str(tmp_path / name), os.path.join(ROOT, "edgestyle_amd", "lib")
    c = subprocess.run([hipcc, "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", name + ".cpp"),
                        "-L" + libdir, "-ledgestyle_hip", "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-2000:]
    return exe


def test_cpp_jpeg_host_writes_the_expected_ppm(tmp_path):
    exe = _build(tmp_path, "jpeg_host")
    for name in ("60x45_420_q90", "23x37_gray_q100_rst"):
        raw, want = R.fixture()["cases"][name]
        (tmp_path / "in.jpg").write_bytes(raw)
        r = subprocess.run([exe, str(tmp_path / "in.jpg"), str(tmp_path / "out.ppm")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        h, w = want.shape[:2]
        assert (tmp_path / "out.ppm").read_bytes() == b"P6\n%d %d\n255\n" % (w, h) + want.tobytes(), name
    (tmp_path / "bad.jpg").write_bytes(raw[:200])
    r = subprocess.run([exe, str(tmp_path / "bad.jpg"), str(tmp_path / "bad.ppm")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "truncated" in r.stderr


def test_cpp_pose_host_gives_the_same_output_for_a_jpeg_as_for_the_ppm_of_its_pixels(tmp_path):
    raw, raster = R.fixture()["cases"]["60x45_420_q90"]
    (tmp_path / "photo.jpg").write_bytes(raw)
    (tmp_path / "photo.ppm").write_bytes(b"P6\n60 45\n255\n" + raster.tobytes())
    g = np.random.default_rng(5)
    with open(str(tmp_path / "kp.txt"), "w") as f:
        for x, y in g.uniform(0.1, 0.9, size=(18, 2)):
            f.write(f"{x:.6f} {y:.6f} 1.0\n")
    exe = _build(tmp_path, "pose_host")
    outs = {}
    for kind in ("jpg", "ppm"):
        r = subprocess.run([exe, str(tmp_path / f"photo.{kind}"), "5", "4", "50", "40", str(tmp_path / "kp.txt"), str(tmp_path / kind)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[kind] = ((tmp_path / f"{kind}_processed.ppm").read_bytes(), (tmp_path / f"{kind}_pose.ppm").read_bytes(), r.stdout)
    assert outs["jpg"] == outs["ppm"] and len(outs["jpg"][0]) == len(b"P6\n512 512\n255\n") + 512 * 512 * 3
    assert any(outs["jpg"][0][15:])

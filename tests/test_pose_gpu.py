"""Person crop and pose rendering on the GPU (csrc/pose.hip, csrc/image_io.hip): es_pose_draw against es_pose_draw_host (the same
__host__ __device__ rule, which tests/test_pose_cpu.py holds against the Python restatement), es_image_resize_window_u8 against the
integer numpy reference built from es_image_resize_coeffs_ex, es_person_crop_u8 against its two halves, graph capture, the Python layer
(edgestyle_amd/pose.py) and the compiled C++ host (examples/pose_host.cpp).  Every comparison is an equality."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from edgestyle_amd import lib as L, ops, pose as P
from tests import pose_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0xA5


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _draw(kp: np.ndarray, H: int, W: int) -> np.ndarray:
    got = ops.pose_draw(_dev(kp.astype(np.float32)), H, W)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _edge_poses(g):
    """shapes clipped at all four edges: limbs that cross each edge, points on and beyond each edge"""
    left, right, top, bottom = (R.random_pose(g, absent=0.0) for _ in range(4))
    left[:, 0] = g.uniform(-0.2, 0.1, size=18)
    right[:, 0] = g.uniform(0.9, 1.2, size=18)
    top[:, 1] = g.uniform(-0.2, 0.1, size=18)
    bottom[:, 1] = g.uniform(0.9, 1.2, size=18)
    corners = R.random_pose(g, absent=0.0)
    corners[:4, :2], corners[4:8, :2], corners[8:12, :2], corners[12:16, :2] = (0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0)
    return [left, right, top, bottom, corners]


@pytest.mark.parametrize("H,W", [(48, 64), (67, 50)])
def test_pose_draw_equals_the_host_form_bit_for_bit(H, W):
    """64 x 48: W * 3 is a multiple of 4 (three dwords per thread); 50 x 67: it is not (byte stores, a ragged last group of pixels, more
    than one tile down).  count = 3 random poses with absent points, five poses clipped at the four edges, one all-absent image."""
    g = np.random.default_rng(H * 131 + W)
    kp = np.stack([R.random_pose(g, absent=a, spread=0.1) for a in (0.0, 0.25, 0.5)] + _edge_poses(g) + [np.zeros((18, 3), dtype=np.float32)])
    got, want = _draw(kp, H, W), R.draw_host(kp, H, W)
    assert got.shape == (kp.shape[0], H, W, 3)
    for i in range(kp.shape[0]):
        assert np.array_equal(got[i], want[i]), (i, int((got[i] != want[i]).sum()))
    assert not got[-1].any() and all(got[i].any() for i in range(3))
    assert np.array_equal(_draw(kp[:3], H, W), want[:3])              # count = 3 alone


def test_pose_draw_of_the_three_reference_poses_in_one_call_equals_the_host_form():
    kp = np.stack(R.fixture()["kp"])
    got, want = _draw(kp, 512, 512), R.draw_host(kp, 512, 512)
    assert np.array_equal(got, want), int((got != want).sum())
    for i in range(3):
        psnr, iou = R.psnr_iou(got[i], R.fixture()["jpg"][i])
        assert psnr >= 34.0 and iou >= 0.92, (i, psnr, iou)


@pytest.mark.parametrize("H,W,offset", [(48, 64, 4096), (67, 50, 4096), (48, 64, 4097)])
def test_pose_draw_stays_inside_an_output_carved_out_of_a_poisoned_buffer(H, W, offset):
    """guard bytes on both sides stay as they were; offset 4097: a canvas that is not 4-byte aligned takes the byte-store path"""
    g = np.random.default_rng(W)
    kp = np.stack([R.random_pose(g, absent=0.2, spread=0.2) for _ in range(3)])
    n = 3 * H * W * 3
    buf = torch.full((offset + n + 4096,), POISON, dtype=torch.uint8, device=DEV)
    out = buf[offset:offset + n].view(3, H, W, 3)
    L.check(L.load().es_pose_draw(C.c_void_p(_dev(kp).data_ptr()), C.c_void_p(out.data_ptr()), 3, H, W, None), "es_pose_draw")
    torch.cuda.synchronize()
    assert bool((buf[:offset] == POISON).all()) and bool((buf[offset + n:] == POISON).all())
    assert np.array_equal(out.cpu().numpy(), R.draw_host(kp, H, W))


# ---- the windowed resize -----------------------------------------------------------------------------------------------------------
def _photo(h, w, seed, ch=3):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, ch), dtype=np.uint8)


def _window_want(a, geom, out_h, out_w, filt):
    nw, nh, left, top = geom
    return R.window(R.integer_resize(a[:, :, :3], nh, nw, filt), left, top, out_h, out_w)


@pytest.mark.parametrize("filt", [L.FILTER_BILINEAR, L.FILTER_BICUBIC, L.FILTER_LANCZOS])
def test_window_resize_equals_the_integer_reference_for_two_images_of_different_sizes_in_one_call(filt):
    """image 0: 37 x 53 -> 61 x 40 (up and down), a window inside; image 1: 90 x 41 -> 50 x 23, smaller than the window on one axis and
    hanging over the end on the other (zero-filled overhang, negative left)"""
    a0, a1 = _photo(37, 53, 1), _photo(90, 41, 2)
    geom = [(40, 61, 5, 9), (23, 50, -4, 30)]
    out_h, out_w = 33, 31
    got = ops.image_resize_window_u8([_dev(a0), _dev(a1)], geom, out_h, out_w, filt)
    torch.cuda.synchronize()
    for i, a in enumerate((a0, a1)):
        want = _window_want(a, geom[i], out_h, out_w, filt)
        assert np.array_equal(got[i].cpu().numpy(), want), (i, int((got[i].cpu().numpy() != want).sum()))
    w1 = got[1].cpu().numpy()
    assert not w1[:, :4].any() and not w1[:, 27:].any() and not w1[20:].any() and w1[:20, 4:27].any()


def test_window_resize_skips_an_axis_whose_size_stays_and_a_window_that_misses_the_image_is_black():
    a = _photo(45, 60, 3)
    geom = [(60, 20, 10, -3), (30, 45, -2, 5), (60, 45, 7, 7), (30, 20, 400, 0)]      # width kept, height kept, both kept, outside
    got = ops.image_resize_window_u8([_dev(a)] * 4, geom, 24, 36, L.FILTER_LANCZOS)
    torch.cuda.synchronize()
    for i in range(4):
        assert np.array_equal(got[i].cpu().numpy(), _window_want(a, geom[i], 24, 36, L.FILTER_LANCZOS)), i
    assert not got[3].any()


def test_window_resize_reads_pitched_rgba_rows_and_stays_inside_output_and_workspace():
    a = _photo(64, 48, 4)
    H, W = a.shape[:2]
    src = torch.full((H, W + 5, 4), POISON, dtype=torch.uint8, device=DEV)
    src[:, :W, :3] = _dev(a)
    view = src[:, :W]
    geom, out_h, out_w, guard = [(96, 23, 20, -6)], 40, 50, 4096
    descs = ops.image_descriptors([view])
    g = (C.c_int32 * 4)(*geom[0])
    need = L.load().es_image_resize_window_u8_workspace_bytes(descs, 1, g, out_h, out_w, L.FILTER_LANCZOS)
    assert need == 64 * 50 * 3                             # every source row (23 rows from 64: the taps reach them all) x the 50 kept columns
    n_out = out_h * out_w * 3
    obuf = torch.full((guard + n_out + guard,), POISON, dtype=torch.uint8, device=DEV)
    wbuf = torch.full((guard + need + guard,), POISON, dtype=torch.uint8, device=DEV)
    out = obuf[guard:guard + n_out].view(1, out_h, out_w, 3)
    ops.image_resize_window_u8([view], geom, out_h, out_w, L.FILTER_LANCZOS, out=out, workspace=wbuf[guard:guard + need])
    torch.cuda.synchronize()
    for buf, n in ((obuf, n_out), (wbuf, need)):
        assert bool((buf[:guard] == POISON).all()) and bool((buf[guard + n:] == POISON).all())
    assert np.array_equal(out[0].cpu().numpy(), _window_want(a, geom[0], out_h, out_w, L.FILTER_LANCZOS))
    assert bool((src[:, W:] == POISON).all())
    with pytest.raises(L.EdgeStyleHipError, match="workspace"):
        ops.image_resize_window_u8([view], geom, out_h, out_w, L.FILTER_LANCZOS, out=out, workspace=wbuf[guard:guard + need - 1])


def test_window_resize_and_pose_draw_replay_inside_one_graph():
    a0, a1 = _photo(37, 53, 5), _photo(37, 53, 6)
    g = np.random.default_rng(7)
    k0, k1 = R.random_pose(g)[None], R.random_pose(g)[None]
    geom, out_h, out_w = [(40, 61, -3, 20)], 48, 64
    src, kp = _dev(a0), _dev(k0)
    need = L.load().es_image_resize_window_u8_workspace_bytes(ops.image_descriptors([src]), 1, (C.c_int32 * 4)(*geom[0]), out_h, out_w, L.FILTER_LANCZOS)
    out = torch.zeros((1, out_h, out_w, 3), dtype=torch.uint8, device=DEV)
    ws = torch.zeros((need,), dtype=torch.uint8, device=DEV)
    canvas = torch.zeros((1, out_h, out_w, 3), dtype=torch.uint8, device=DEV)

    def chain():
        ops.image_resize_window_u8([src], geom, out_h, out_w, L.FILTER_LANCZOS, out=out, workspace=ws)
        ops.pose_draw(kp, out_h, out_w, out=canvas)
    chain()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for a, k in ((a1, k1), (a0, k0)):
        src.copy_(_dev(a))
        kp.copy_(_dev(k))
        out.fill_(POISON)
        canvas.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out[0].cpu().numpy(), _window_want(a, geom[0], out_h, out_w, L.FILTER_LANCZOS))
        assert np.array_equal(canvas.cpu().numpy(), R.draw_host(k, out_h, out_w))


# ---- create_processed_image ----------------------------------------------------------------------------------------------------------
PERSON_CASES = [((60, 45), (5.0, 4.0, 40.0, 50.0)), ((90, 30), (2.0, 5.0, 28.0, 85.0)), ((40, 70), (30.5, 2.25, 66.0, 39.0))]


def test_person_crop_equals_the_fit_followed_by_the_window_resize():
    """three small photos of different sizes in one call; the second is tall and narrow: its resized width stays below 512 and the
    window's left edge is negative"""
    photos = [_photo(h, w, 10 + i) for i, ((h, w), _) in enumerate(PERSON_CASES)]
    boxes = [b for _, b in PERSON_CASES]
    dev = [_dev(a) for a in photos]
    got = ops.person_crop_u8(dev, boxes)
    geom = [ops.person_crop_fit(a.shape[0], a.shape[1], b) for a, b in zip(photos, boxes)]
    assert geom == [R.crop_fit(a.shape[0], a.shape[1], b) for a, b in zip(photos, boxes)] and geom[1][2] < 0
    two = ops.image_resize_window_u8(dev, geom, 512, 512, L.FILTER_LANCZOS)
    torch.cuda.synchronize()
    assert got.shape == (3, 512, 512, 3) and torch.equal(got, two)
    want = R.processed_image(photos[1], boxes[1])
    assert np.array_equal(got[1].cpu().numpy(), want) and not want[:, :-geom[1][2]].any()
    if R.have_pillow():                                    # the reference's own two lines on live Pillow
        from PIL import Image
        nw, nh, left, top = geom[0]
        ref = Image.fromarray(photos[0]).resize((nw, nh), Image.Resampling.LANCZOS).crop((left, top, left + 512, top + 512))
        assert np.array_equal(got[0].cpu().numpy(), np.asarray(ref))
    with pytest.raises(L.EdgeStyleHipError):
        ops.person_crop_u8(dev[:1], [(10, 10, 10, 50)])


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_condition_inputs_returns_what_preprocess_images_accepts():
    """tiny sizes, no networks: preprocess_images is called on a bare pipeline object (it reads the device and the two sizes only)"""
    from edgestyle_amd.pipeline import EdgeStyleStableDiffusionControlNetPipeline as Pipe
    photo, box = _photo(60, 45, 21), (5.0, 4.0, 40.0, 50.0)
    kps = [[0.5, 0.2, 1.0, -1], [0.5, 0.35, 1.0, -1], [0.35, 0.36, 0.9, -1], None, None, [0.65, 0.36, 0.9, -1], None, None, [0.42, 0.7, 0.8, -1], None,
           None, [0.58, 0.7, 0.8, -1], None, None, [0.47, 0.17, 1.0, -1], [0.53, 0.17, 1.0, -1], None, None]
    processed, pose_image, points = P.condition_inputs(photo, box, kps, final_width=64, final_height=48)
    torch.cuda.synchronize()
    assert processed.shape == pose_image.shape == (48, 64, 3) and processed.dtype == pose_image.dtype == torch.uint8 and processed.is_cuda
    assert np.array_equal(processed.cpu().numpy(), R.processed_image(photo, box, 64, 48))
    kp = R.keypoints_array(kps)
    assert np.array_equal(pose_image.cpu().numpy(), R.draw_host(kp, 48, 64)[0])
    assert np.array_equal(points, R.points_host(kp, 64, 48)) and points.shape == (8, 2)
    assert torch.equal(P.draw_poses([kps], 48, 64), pose_image) and torch.equal(P.draw_bodypose(kp, 48, 64), pose_image)
    assert P.draw_bodypose(np.stack([kp, kp]), 48, 64).shape == (2, 48, 64, 3)
    assert P.select_pose([dict(keypoints=kps, total_score=20.0, total_parts=9.0)]) == 0
    pipe = Pipe.__new__(Pipe)
    pipe.device = torch.device(DEV)
    pre = pipe.preprocess_images([processed, pose_image], resolution=32, normalize=[True, False])
    torch.cuda.synchronize()
    from tests import image_io_ref as IR
    for t, src, nrm in zip(pre, (processed, pose_image), (True, False)):
        a = src.cpu().numpy()
        rh, rw, top, left = IR.fit(48, 64, 32)
        want = IR.to_float_host(IR.crop(IR.integer_resize(a, rh, rw), 32, top, left), nrm)
        assert t.shape == (1, 3, 32, 32) and t.is_cuda and torch.equal(t.cpu(), want)


# ---- the C++ host ----------------------------------------------------------------------------------------------------------------
def test_cpp_pose_host_writes_the_bytes_of_the_python_path(tmp_path):
    """examples/pose_host.cpp: one PPM photo, a box and a key-point file in -> es_person_crop_u8 + es_pose_draw -> two PPMs, no Python in
    the process"""
    photo, box = _photo(60, 45, 31), (5.0, 4.0, 40.0, 50.0)
    kp = R.fixture()["kp"][0]
    processed, pose_image, points = P.condition_inputs(photo, box, kp)
    torch.cuda.synchronize()
    with open(str(tmp_path / "photo.ppm"), "wb") as f:
        f.write(b"P6\n# pose_host input\n%d %d\n255\n" % (photo.shape[1], photo.shape[0]) + photo.tobytes())
    with open(str(tmp_path / "kp.txt"), "w") as f:
        for x, y, s in kp:
            f.write(f"{float(x):.9g} {float(y):.9g} {float(s):.9g}\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, libdir = str(tmp_path / "pose_host"), os.path.join(root, "edgestyle_amd", "lib")
    c = subprocess.run([hipcc, "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "pose_host.cpp"),
                        "-L" + libdir, "-ledgestyle_hip", "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-2000:]
    r = subprocess.run([exe, str(tmp_path / "photo.ppm")] + [repr(v) for v in box] + [str(tmp_path / "kp.txt"), str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    head = b"P6\n512 512\n255\n"
    for name, want in (("processed", processed), ("pose", pose_image)):
        raw = open(str(tmp_path / f"out_{name}.ppm"), "rb").read()
        assert raw.startswith(head) and len(raw) == len(head) + 512 * 512 * 3, name
        assert raw[len(head):] == want.cpu().numpy().tobytes(), name
    assert f"{len(points)} SAM points" in r.stdout

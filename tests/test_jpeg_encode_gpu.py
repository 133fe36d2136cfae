"""The JPEG encoder on the GPU (csrc/jpeg_encode.hip): es_jpeg_forward against es_jpeg_forward_host and the coefficients of Pillow's
files, es_jpeg_entropy_encode fed those coefficients against Pillow's bytes, es_jpeg_encode_u8 against Pillow's bytes and the host twin
(tests/test_jpeg_encode_cpu.py holds the twin against Pillow), images of different sizes in one call and more than one launch batch,
poisoned buffers around outputs and workspace, a short capacity, pitched input, graph capture, the refusals, the Python layer
(edgestyle_amd/jpeg.py) and the compiled C++ host (examples/jpeg_encode_host.cpp).  Every comparison is an equality.

One call has one es_jpeg_encode_params, so the files of one sampling go in one call per (quality, restart interval)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from edgestyle_amd import jpeg as J, lib as L, ops
from tests import jpeg_encode_ref as E, jpeg_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0xA5
GUARD = 4096
CASES = E.cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _groups(sampling):
    """{(quality, restart): [names]} of one sampling: what can share a call"""
    out = {}
    for name, w, h, s, quality, kind, restart, _ in CASES:
        if s == sampling:
            out.setdefault((quality, restart), []).append(name)
    return out


def _files(out, lengths):
    torch.cuda.synchronize()
    sizes = [int(k) for k in lengths.cpu().view(torch.int32).tolist()]
    return [o[:k].cpu().numpy().tobytes() for o, k in zip(out, sizes)], sizes


@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_forward_equals_the_host_twin_and_the_coefficients_of_pillows_file(sampling):
    fx = E.fixture()["cases"]
    seen = 0
    for (quality, restart), names in _groups(sampling).items():
        params = J.encode_params(**E.keywords(sampling, quality, restart))
        arrays = [fx[n][0] for n in names]
        infos, got = ops.jpeg_forward([_dev(a) for a in arrays], params)
        torch.cuda.synchronize()
        _, twin = J.forward_host(arrays, params)
        for i, name in enumerate(names):
            info, want, _ = J.entropy_decode(fx[name][1])
            g = got[i].cpu().numpy()
            assert bytes(infos[i]) == bytes(info), name
            assert np.array_equal(g, twin[i]), (name, int((g != twin[i]).sum()))
            assert np.array_equal(g, want), (name, int((g != want).sum()))
            seen += 1
    assert seen >= 2 * len(R.SIZES)


@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_entropy_encode_of_pillows_coefficients_equals_pillows_bytes(sampling):
    """the stage alone: it never sees a pixel"""
    fx = E.fixture()["cases"]
    for (quality, restart), names in _groups(sampling).items():
        params = J.encode_params(**E.keywords(sampling, quality, restart))
        parts = [J.entropy_decode(fx[n][1]) for n in names]
        infos = (L.JpegInfo * len(names))(*[p[0] for p in parts])
        files, sizes = _files(*ops.jpeg_entropy_encode(infos, params, [torch.from_numpy(p[1]).to(DEV) for p in parts]))
        for name, f, k in zip(names, files, sizes):
            assert k == len(fx[name][1]) and f == fx[name][1], (name, k, len(fx[name][1]))


@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_encode_u8_equals_pillows_bytes_and_the_twins_on_every_case(sampling):
    fx = E.fixture()["cases"]
    for (quality, restart), names in _groups(sampling).items():
        kw = E.keywords(sampling, quality, restart)
        arrays = [fx[n][0] for n in names]
        files, sizes = _files(*ops.jpeg_encode_u8([_dev(a) for a in arrays], J.encode_params(**kw)))
        twin = J.encode_host(arrays, **kw)
        for name, f, k, t in zip(names, files, sizes, twin):
            assert k == len(t) == len(fx[name][1]), (name, k, len(t), len(fx[name][1]))
            assert f == t and f == fx[name][1], name


def test_forty_images_of_both_channel_counts_in_one_call_span_three_launch_batches():
    """every size twice, gray and colour alternating, in ONE call: 40 images = 16 + 16 + 8"""
    arrays = [R.content(w, h, "noise" if k % 2 else "photo", 3000 + 4 * k + j, (k + j) % 2 == 0)
              for j in range(4) for k, (w, h) in enumerate(R.SIZES)]
    assert len(arrays) == 40 and {a.ndim for a in arrays} == {2, 3}
    kw = dict(quality=85, subsampling=2, restart_marker_blocks=2)
    files, sizes = _files(*ops.jpeg_encode_u8([_dev(a) for a in arrays], J.encode_params(**kw)))
    twin = J.encode_host(arrays, **kw)
    assert files == twin and sizes == [len(t) for t in twin]
    with pytest.raises(L.EdgeStyleHipError, match="64"):
        ops.jpeg_encode_u8([_dev(arrays[0])] * 65, J.encode_params(**kw))


def test_four_images_of_different_sizes_and_samplings_in_one_call_each_equal_the_image_alone():
    fx = E.fixture()["cases"]
    names = ["33x18_420_q30", "23x37_gray_q30", "17x23_420_q30", "9x5_gray_q30"]
    arrays = [_dev(fx[n][0]) for n in names]
    params = J.encode_params(quality=30, subsampling=2)
    together, _ = _files(*ops.jpeg_encode_u8(arrays, params))
    for name, a, f in zip(names, arrays, together):
        alone, _ = _files(*ops.jpeg_encode_u8([a], params))
        assert f == alone[0] == fx[name][1], name


def test_the_624_block_interval_the_wrapping_marker_number_and_the_photo_equal_pillows_bytes():
    fx = E.fixture()
    a, raw = fx["cases"][E.BIG]
    assert J.encode(_dev(a), quality=90, subsampling="4:2:0") == raw
    assert J.encode(_dev(a), quality=90, subsampling="4:2:0", restart_marker_blocks=3) == fx["cases"][E.BIG + "_rst3"][1]
    assert J.encode(_dev(E.photo_pixels())) == fx["photo_jpg"]


def test_a_stream_of_more_than_256_chunks_equals_the_twin():
    """512 x 512 noise at quality 100, 4:4:4: 12288 blocks (48 chunks of blocks) and over 256 chunks of 1024 stream bytes, so the second
    prefix sum walks more than one tile"""
    a = R.content(512, 512, "noise", 4000, False)
    kw = dict(quality=100, subsampling=0, restart_marker_blocks=7)
    got = J.encode(_dev(a), **kw)
    assert len(got) > 256 * 1024 and got == J.encode_host(a, **kw)


@pytest.mark.parametrize("name", ["33x18_420_q30", "17x23_444_q100_rst", "23x37_gray_q30", E.BIG + "_rst3"])
def test_outputs_and_workspace_inside_poisoned_buffers_keep_the_poison_also_with_a_short_capacity(name):
    _, w, h, s, quality, _, restart, _ = [c for c in CASES if c[0] == name][0]
    a, raw = E.fixture()["cases"][name]
    params = J.encode_params(**E.keywords(s, quality, restart))
    lib = L.load()
    image = _dev(a)
    descs = ops.jpeg_image_descs("test", [image])
    infos = ops.jpeg_encode_infos("test", descs, params)
    cap = int(lib.es_jpeg_encode_capacity(infos, C.byref(params)))
    need = int(lib.es_jpeg_encode_workspace_bytes(infos, 1, C.byref(params)))
    assert cap >= len(raw) and need > 0
    for capacity in (cap, len(raw), len(raw) - 1, 300, 0):
        obuf = torch.full((GUARD + cap + GUARD,), POISON, dtype=torch.uint8, device=DEV)
        wbuf = torch.full((GUARD + need + GUARD,), POISON, dtype=torch.uint8, device=DEV)
        lbuf = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device=DEV).view(torch.uint32)
        rc = lib.es_jpeg_encode_u8(descs, 1, C.byref(params), (C.c_void_p * 1)(obuf.data_ptr() + GUARD), (C.c_size_t * 1)(capacity),
                                   C.c_void_p(lbuf.data_ptr() + 4), C.c_void_p(wbuf.data_ptr() + GUARD), need, None)
        assert rc == 0, lib.es_last_error()
        torch.cuda.synchronize()
        lengths = lbuf.view(torch.int32).cpu().tolist()
        assert lengths == [0x5A5A5A5A, len(raw), 0x5A5A5A5A], (capacity, lengths)          # the needed length, whatever the capacity
        assert bool((obuf[:GUARD] == POISON).all()) and bool((obuf[GUARD + capacity:] == POISON).all()), capacity
        assert bool((wbuf[:GUARD] == POISON).all()) and bool((wbuf[GUARD + need:] == POISON).all()), capacity
        if capacity >= len(raw):
            assert obuf[GUARD:GUARD + len(raw)].cpu().numpy().tobytes() == raw, capacity


def test_a_pitched_input_gives_the_same_bytes():
    for name in ("33x18_420_q30", "23x37_gray_q30", "16x16_422_q30"):
        _, w, h, s, quality, _, restart, _ = [c for c in CASES if c[0] == name][0]
        a, raw = E.fixture()["cases"][name]
        ch = 1 if a.ndim == 2 else 3
        stride = w * ch + 5
        buf = torch.full((h + 2, stride), 0xEE, dtype=torch.uint8, device=DEV)
        rows = buf[1:h + 1, :w * ch]
        rows.copy_(_dev(a).reshape(h, w * ch))
        view = rows if ch == 1 else rows.unflatten(1, (w, 3))
        assert view.stride(0) == stride and view.data_ptr() == buf.data_ptr() + stride
        assert J.encode(view, **E.keywords(s, quality, restart)) == raw, name


def test_a_captured_call_replayed_twice_gives_the_same_bytes():
    """captured over one image, replayed after another of the same geometry was copied into the same tensor, and again after the first
    came back; outputs, lengths and workspace are poisoned before every replay"""
    fx = E.fixture()["cases"]
    names = ("33x18_420_q30",)
    first, second = _dev(fx[names[0]][0]), _dev(R.content(33, 18, "photo", 5000, False))
    kw = E.keywords("420", 30, 0)
    params = J.encode_params(**kw)
    image = first.clone()
    out, lengths = ops.jpeg_encode_u8([image], params)
    need = int(L.load().es_jpeg_encode_workspace_bytes(ops.jpeg_encode_infos("test", ops.jpeg_image_descs("test", [image]), params), 1, C.byref(params)))
    ws = torch.zeros((need,), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.jpeg_encode_u8([image], params, out=out, lengths=lengths, workspace=ws)
    for src, want in ((second, J.encode_host(second.cpu().numpy(), **kw)), (first, fx[names[0]][1]), (first, fx[names[0]][1])):
        image.copy_(src)
        out[0].fill_(POISON)
        ws.fill_(POISON)
        lengths.view(torch.int32).fill_(-1)
        graph.replay()
        files, sizes = _files(out, lengths)
        assert sizes == [len(want)] and files[0] == want


def test_refusals_on_the_device_side():
    lib = L.load()
    a = _dev(E.fixture()["cases"]["17x23_420_q30"][0])
    params = J.encode_params(quality=30)
    descs = ops.jpeg_image_descs("test", [a])
    infos = ops.jpeg_encode_infos("test", descs, params)
    cap = int(lib.es_jpeg_encode_capacity(infos, C.byref(params)))
    need = int(lib.es_jpeg_encode_workspace_bytes(infos, 1, C.byref(params)))
    out = torch.zeros((cap,), dtype=torch.uint8, device=DEV)
    ws = torch.zeros((need + 16,), dtype=torch.uint8, device=DEV)
    lengths = torch.zeros((2,), dtype=torch.int32, device=DEV)
    coeffs = torch.zeros((int(lib.es_jpeg_coeff_count(infos)) + 8,), dtype=torch.int16, device=DEV)

    def encode(ws_bytes=need, lengths_ptr=lengths.data_ptr(), out_ptr=out.data_ptr()):
        return lib.es_jpeg_encode_u8(descs, 1, C.byref(params), (C.c_void_p * 1)(out_ptr), (C.c_size_t * 1)(cap), C.c_void_p(lengths_ptr),
                                     C.c_void_p(ws.data_ptr()), ws_bytes, None)
    assert encode(ws_bytes=need - 1) == -1 and b"workspace too small" in lib.es_last_error()
    assert encode(lengths_ptr=lengths.data_ptr() + 2) == -1 and b"aligned" in lib.es_last_error()
    assert encode(out_ptr=None) == -1 and b"null" in lib.es_last_error()
    rc = lib.es_jpeg_forward(descs, 1, C.byref(params), (C.c_void_p * 1)(coeffs.data_ptr() + 2), None, 0, None)
    assert rc == -1 and b"16-byte aligned" in lib.es_last_error()
    rc = lib.es_jpeg_entropy_encode(infos, 1, C.byref(params), (C.c_void_p * 1)(coeffs.data_ptr() + 2), (C.c_void_p * 1)(out.data_ptr()),
                                    (C.c_size_t * 1)(cap), C.c_void_p(lengths.data_ptr()), C.c_void_p(ws.data_ptr()), need, None)
    assert rc == -1 and b"16-byte aligned" in lib.es_last_error()
    rc = lib.es_jpeg_entropy_encode(infos, 1, C.byref(params), (C.c_void_p * 1)(coeffs.data_ptr()), (C.c_void_p * 1)(out.data_ptr()),
                                    (C.c_size_t * 1)(cap), C.c_void_p(lengths.data_ptr()), C.c_void_p(ws.data_ptr()), need - 1, None)
    assert rc == -1 and b"workspace too small" in lib.es_last_error()
    rgba = torch.zeros((5, 9, 4), dtype=torch.uint8, device=DEV)
    with pytest.raises(L.EdgeStyleHipError, match="RGBA"):
        J.encode(rgba)
    with pytest.raises(L.EdgeStyleHipError, match="optimize"):
        J.encode(a, optimize=True)
    with pytest.raises(L.EdgeStyleHipError, match="progressive"):
        J.encode_device(a, progressive=True)
    assert encode() == 0                                   # and the same arguments, whole, are taken
    torch.cuda.synchronize()
    assert out[:int(lengths[0])].cpu().numpy().tobytes() == E.fixture()["cases"]["17x23_420_q30"][1]


def test_encode_of_a_batch_tensor_returns_one_file_per_image_and_decodes_to_pillows_pixels():
    g = np.random.default_rng(11)
    batch = np.clip(np.stack([R.content(40, 24, "photo", 6000 + i, False) for i in range(3)]).astype(np.int64) + g.integers(-3, 4, size=(3, 24, 40, 3)),
                    0, 255).astype(np.uint8)
    files = J.encode(_dev(batch))
    assert isinstance(files, list) and len(files) == 3 and files == J.encode_host(batch)
    if R.have_pillow():
        assert files == [R.encode(b, "420", 75) for b in batch]
    out, lengths = J.encode_device(_dev(batch))           # nothing read back
    assert len(out) == 3 and lengths.dtype == torch.uint32 and lengths.is_cuda and all(o.is_cuda for o in out)
    back = J.decode(files)
    torch.cuda.synchronize()
    for f, b in zip(files, back):
        assert np.array_equal(b.cpu().numpy(), J.decode_host(f))
        if R.have_pillow():
            assert np.array_equal(b.cpu().numpy(), R.pillow_rgb(f))
    fx = E.fixture()["cases"]
    a, raw = fx["23x37_420_q30"]
    round_trip = J.decode(J.encode(_dev(a), quality=30)).cpu().numpy()
    assert np.array_equal(round_trip, J.decode_host(raw))
    gray = fx["33x18_gray_q30"]
    assert J.encode(_dev(gray[0]), quality=30) == gray[1] and isinstance(J.encode([_dev(gray[0])], quality=30), list)


# ---- the C++ host ------------------------------------------------------------------------------------------------------------------
def test_cpp_jpeg_encode_host_reproduces_fixture_files(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, libdir = str(tmp_path / "jpeg_encode_host"), os.path.join(ROOT, "edgestyle_amd", "lib")
    c = subprocess.run([hipcc, "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "jpeg_encode_host.cpp"),
                        "-L" + libdir, "-ledgestyle_hip", "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-2000:]
    for name, flags in (("70x50_420_q90", ["-q", "90"]), ("33x18_gray_q100_rst", ["-q", "100", "-r", "1"]), ("17x23_422_q30", ["-s", "422", "-q", "30"])):
        a, raw = E.fixture()["cases"][name]
        h, w = a.shape[:2]
        (tmp_path / "in.pnm").write_bytes((b"P5" if a.ndim == 2 else b"P6") + b"\n%d %d\n255\n" % (w, h) + a.tobytes())
        r = subprocess.run([exe, str(tmp_path / "in.pnm"), str(tmp_path / "out.jpg")] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert (tmp_path / "out.jpg").read_bytes() == raw, name
    r = subprocess.run([exe, str(tmp_path / "in.pnm"), str(tmp_path / "bad.jpg"), "-s", "411"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "subsampling" in r.stderr

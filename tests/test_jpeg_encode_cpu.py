"""The JPEG encoder without a GPU (csrc/jpeg.h through the library's host entry points): es_jpeg_forward_host against the coefficients
the project's own Huffman decoder reads from Pillow's files, es_jpeg_entropy_encode_host and es_jpeg_encode_host against Pillow's bytes
(tests/golden/jpeg_encode.safetensors, and live Pillow where it is importable), every refusal with its reason, the size bound, and
examples/jpeg_encode_host.cpp built with -DJPEG_HOST_DRY by the plain host compiler.  Every comparison is an equality."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from edgestyle_amd import jpeg as J, lib as L
from tests import jpeg_encode_ref as E, jpeg_ref as R

NEW_SYMBOLS = ("es_jpeg_encode_info_host", "es_jpeg_header_host", "es_jpeg_encode_capacity", "es_jpeg_encode_workspace_bytes",
               "es_jpeg_forward", "es_jpeg_forward_host", "es_jpeg_entropy_encode", "es_jpeg_entropy_encode_host", "es_jpeg_encode_u8",
               "es_jpeg_encode_host")
CASES = E.cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(sampling, quality, restart):
    return J.encode_params(**E.keywords(sampling, quality, restart))


def test_library_exports_the_new_symbols_and_the_abi_version_stays():
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS and getattr(lib, name)
    assert lib.es_abi_version() == L.ABI_VERSION == 7
    assert C.sizeof(L.JpegEncodeParams) == 12


def test_the_fixture_holds_the_cases_that_decide():
    fx = E.fixture()
    assert len(fx["cases"]) == len(CASES) == 2 * len(R.SIZES) * len(R.SAMPLINGS) + len(E.PADDING_ORDER_SIZES) + 8
    assert (fx["max_ac_category"], fx["max_dc_category"]) == (10, 11)
    assert fx["cases"][E.BIG][1].count(b"\xff\xd0") == 0 and fx["cases"][E.BIG + "_rst3"][1].count(b"\xff\xd7") >= 2      # the number wraps
    assert os.path.getsize(E.GOLDEN) < 1 << 20


@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_forward_host_equals_the_coefficients_of_pillows_file(sampling):
    """every coefficient of every block, the dummy blocks of the MCU-padded grid included; and the geometry is the file's"""
    fx = E.fixture()["cases"]
    seen = 0
    for name, w, h, s, quality, kind, restart, _ in CASES:
        if s != sampling:
            continue
        a, raw = fx[name]
        info, want, _ = J.entropy_decode(raw)
        infos, got = J.forward_host([a], _params(s, quality, restart))
        assert bytes(infos[0]) == bytes(info), name
        assert got[0].shape == want.shape and np.array_equal(got[0], want), (name, int((got[0] != want).sum()))
        seen += 1
    assert seen >= 2 * len(R.SIZES)


@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_entropy_encode_host_of_pillows_coefficients_equals_pillows_bytes(sampling):
    """the stage alone: header, Huffman coding, stuffing, restart markers and EOI"""
    fx = E.fixture()["cases"]
    for name, w, h, s, quality, kind, restart, _ in CASES:
        if s != sampling:
            continue
        raw = fx[name][1]
        info, coeffs, _ = J.entropy_decode(raw)
        got = J.entropy_encode_host([info], _params(s, quality, restart), [coeffs])[0]
        assert got == raw, (name, len(got), len(raw))


@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_encode_host_equals_pillows_bytes_in_the_fixture(sampling):
    fx = E.fixture()["cases"]
    for name, w, h, s, quality, kind, restart, _ in CASES:
        if s != sampling:
            continue
        a, raw = fx[name]
        got = J.encode_host(a, **E.keywords(s, quality, restart))
        assert isinstance(got, bytes) and got == raw, (name, len(got), len(raw))


def test_encode_host_equals_pillows_file_of_the_photo_and_takes_a_batch():
    photo = E.photo_pixels()
    assert J.encode_host(photo) == E.fixture()["photo_jpg"]
    batch = np.stack([photo[:64, :48], photo[100:164, 200:248]])
    got = J.encode_host(batch, quality=75)
    assert isinstance(got, list) and got == [J.encode_host(np.ascontiguousarray(b)) for b in batch]


def test_the_header_alone_is_the_files_first_bytes():
    lib = L.load()
    for name in ("17x23_420_q30", "33x18_gray_q100_rst", "9x5_444_q30"):
        _, w, h, s, quality, _, restart, _ = [c for c in CASES if c[0] == name][0]
        raw = E.fixture()["cases"][name][1]
        info, params = J.info(raw), _params(s, quality, restart)
        buf = np.full((700,), 0xA5, dtype=np.uint8)
        n = C.c_size_t(0)
        assert lib.es_jpeg_header_host(C.byref(info), C.byref(params), buf.ctypes.data, 640, C.byref(n)) == 0
        scan = R.find(raw, 0xDA)[0]
        assert n.value == scan[0] + 2 + scan[1] <= 629 and buf[:n.value].tobytes() == raw[:n.value] and (buf[n.value:] == 0xA5).all()
        buf[:] = 0xA5
        assert lib.es_jpeg_header_host(C.byref(info), C.byref(params), buf.ctypes.data, n.value - 1, C.byref(n)) == -1
        assert b"capacity" in lib.es_last_error() and (buf[n.value - 1:] == 0xA5).all()


@pytest.mark.skipif(not R.have_pillow(), reason="live Pillow is not importable")
def test_encode_host_equals_live_pillow_on_random_sizes_and_every_quality():
    g = np.random.default_rng(77)
    qualities = list(range(1, 101))
    for k, quality in enumerate(qualities):
        w, h = int(g.integers(1, 49)), int(g.integers(1, 49))
        sampling = R.SAMPLINGS[k % 4]
        restart = int(g.integers(0, 4))
        a = R.content(w, h, ("noise", "smooth", "photo")[k % 3], 9000 + k, sampling == "gray")
        want = R.encode(a, sampling, quality, restart)
        got = J.encode_host(a, **E.keywords(sampling, quality, restart))
        assert got == want, (w, h, sampling, quality, restart, len(got), len(want))


def test_decoding_our_file_gives_the_pixels_of_pillows_file():
    fx = E.fixture()["cases"]
    for name in ("23x37_420_q30", "33x18_422_q100_rst", "17x23_444_q30", "9x5_gray_q30", "70x50_420_q90"):
        _, w, h, s, quality, _, restart, _ = [c for c in CASES if c[0] == name][0]
        a, raw = fx[name]
        got = J.decode_host(J.encode_host(a, **E.keywords(s, quality, restart)))
        assert got.shape == (h, w, 3) and np.array_equal(got, J.decode_host(raw)), name
        if R.have_pillow():
            assert np.array_equal(got, R.pillow_rgb(raw)), name


def test_pitched_rows_with_a_poisoned_tail_give_the_same_bytes():
    fx = E.fixture()["cases"]
    for name in ("33x18_420_q30", "23x37_gray_q30"):
        _, w, h, s, quality, _, restart, _ = [c for c in CASES if c[0] == name][0]
        a, raw = fx[name]
        ch = 1 if a.ndim == 2 else 3
        buf = np.full((h + 2, w * ch + 5), 0xEE, dtype=np.uint8)
        view = buf[1:h + 1, :w * ch].reshape(a.shape)
        view[...] = a
        assert view.strides[0] == w * ch + 5 and not view.flags["C_CONTIGUOUS"]
        assert J.encode_host(view, **E.keywords(s, quality, restart)) == raw, name
        buf[:, w * ch:] = 0x11                             # other poison, the same file
        buf[0] = buf[h + 1] = 0x22
        assert J.encode_host(view, **E.keywords(s, quality, restart)) == raw, name


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _host_call(a, params, cap=None, channels=None):
    """es_jpeg_encode_host on one array -> (rc, reason, length, guarded output buffer, capacity)"""
    lib = L.load()
    h, w = a.shape[:2]
    ch = channels if channels is not None else (1 if a.ndim == 2 else a.shape[2])
    desc = L.ImageU8(a.ctypes.data, h, w, ch, w * ch)
    if cap is None:
        cap = 1 << 16
    buf = np.full((64 + cap + 64,), 0xA5, dtype=np.uint8)
    length = np.zeros((1,), dtype=np.uint32)
    rc = lib.es_jpeg_encode_host(C.byref(desc), 1, C.byref(params), (C.c_void_p * 1)(buf[64:].ctypes.data), (C.c_size_t * 1)(cap), length.ctypes.data)
    return rc, lib.es_last_error().decode(), int(length[0]), buf, cap


def test_every_refusal_carries_its_reason():
    lib = L.load()
    rgb = R.content(9, 5, "noise", 1, False)
    rgba = np.ascontiguousarray(np.concatenate([rgb, rgb[:, :, :1]], axis=2))
    good = L.JpegEncodeParams(75, 2, 0)
    rc, msg, *_ = _host_call(rgba, good)
    assert rc == -1 and "cannot write mode RGBA as JPEG" in msg
    rc, msg, *_ = _host_call(rgb, good, channels=2)
    assert rc == -1 and "1 or 3 channels" in msg
    for quality in (0, 101, -5):
        rc, msg, *_ = _host_call(rgb, L.JpegEncodeParams(quality, 2, 0))
        assert rc == -1 and "quality" in msg, quality
    for sub in (3, -1, 7):
        rc, msg, *_ = _host_call(rgb, L.JpegEncodeParams(75, sub, 0))
        assert rc == -1 and "subsampling" in msg, sub
    assert _host_call(R.content(9, 5, "noise", 1, True), L.JpegEncodeParams(75, 9, 0))[0] == 0          # ignored for one channel
    for restart in (-1, 65536):
        rc, msg, *_ = _host_call(rgb, L.JpegEncodeParams(75, 2, restart))
        assert rc == -1 and "restart" in msg, restart
    info = L.JpegInfo()
    for w, h in ((0, 5), (5, 0), (65536, 1)):
        assert lib.es_jpeg_encode_info_host(w, h, 3, C.byref(good), C.byref(info)) == -1 and b"height or width" in lib.es_last_error()
    desc = L.ImageU8(rgb.ctypes.data, 0, 9, 3, 27)
    out = np.zeros((4096,), dtype=np.uint8)
    length = np.zeros((1,), dtype=np.uint32)
    rc = lib.es_jpeg_encode_host(C.byref(desc), 1, C.byref(good), (C.c_void_p * 1)(out.ctypes.data), (C.c_size_t * 1)(4096), length.ctypes.data)
    assert rc == -1 and b"height or width" in lib.es_last_error()
    desc = L.ImageU8(rgb.ctypes.data, 5, 9, 3, 26)                                                      # a stride below the row
    rc = lib.es_jpeg_encode_host(C.byref(desc), 1, C.byref(good), (C.c_void_p * 1)(out.ctypes.data), (C.c_size_t * 1)(4096), length.ctypes.data)
    assert rc == -1 and b"stride" in lib.es_last_error()
    desc = L.ImageU8(None, 5, 9, 3, 27)
    rc = lib.es_jpeg_encode_host(C.byref(desc), 1, C.byref(good), (C.c_void_p * 1)(out.ctypes.data), (C.c_size_t * 1)(4096), length.ctypes.data)
    assert rc == -1 and b"memory" in lib.es_last_error()
    # an info that is not the params' is refused before anything is sized by it
    assert lib.es_jpeg_encode_info_host(9, 5, 3, C.byref(good), C.byref(info)) == 0
    assert lib.es_jpeg_encode_capacity(C.byref(info), C.byref(L.JpegEncodeParams(75, 0, 0))) == 0 and b"subsampling" in lib.es_last_error()
    assert lib.es_jpeg_encode_workspace_bytes(C.byref(info), 1, C.byref(L.JpegEncodeParams(75, 2, 4))) == 0
    huge = L.JpegInfo()
    assert lib.es_jpeg_encode_info_host(65535, 65535, 3, C.byref(L.JpegEncodeParams(75, 0, 0)), C.byref(huge)) == 0
    assert lib.es_jpeg_encode_capacity(C.byref(huge), C.byref(L.JpegEncodeParams(75, 0, 0))) == 0 and b"too large" in lib.es_last_error()
    coeffs = np.zeros((int(lib.es_jpeg_coeff_count(C.byref(info))),), dtype=np.int16)
    coeffs[5] = 1024                                       # category 11: no AC code in a baseline file
    with pytest.raises(L.EdgeStyleHipError, match="baseline"):
        J.entropy_encode_host([info], good, [coeffs])


def test_python_refuses_what_it_would_have_to_approximate():
    a = R.content(9, 5, "noise", 1, False)
    for kw in (dict(optimize=True), dict(progressive=True), dict(dpi=(72, 72)), dict(exif=b""), dict(qtables="web_low")):
        with pytest.raises(L.EdgeStyleHipError, match=next(iter(kw))):
            J.encode_host(a, **kw)
    for sub in ("4:4:0", 3, None, True):
        with pytest.raises(L.EdgeStyleHipError, match="subsampling"):
            J.encode_host(a, subsampling=sub)
    with pytest.raises(L.EdgeStyleHipError, match="quality"):
        J.encode_host(a, quality=0)
    with pytest.raises(L.EdgeStyleHipError, match="quality"):
        J.encode_host(a, quality=75.0)
    with pytest.raises(L.EdgeStyleHipError, match="RGBA"):
        J.encode_host(np.zeros((5, 9, 4), dtype=np.uint8))
    with pytest.raises(L.EdgeStyleHipError):
        J.encode_host(np.zeros((0, 9, 3), dtype=np.uint8))
    assert J.encode_host(a, subsampling="4:2:2") == J.encode_host(a, subsampling=1)


def test_a_capacity_short_by_one_reports_the_length_and_leaves_the_guards():
    for name in ("17x23_420_q30", "33x18_444_q100_rst"):
        _, w, h, s, quality, _, restart, _ = [c for c in CASES if c[0] == name][0]
        a, raw = E.fixture()["cases"][name]
        params = _params(s, quality, restart)
        rc, _, length, buf, cap = _host_call(a, params, cap=len(raw))
        assert rc == 0 and length == len(raw) and buf[64:64 + cap].tobytes() == raw
        assert (buf[:64] == 0xA5).all() and (buf[64 + cap:] == 0xA5).all()
        rc, _, length, buf, cap = _host_call(a, params, cap=len(raw) - 1)
        assert rc == 0 and length == len(raw) and buf[64:64 + cap].tobytes() == raw[:-1]
        assert (buf[:64] == 0xA5).all() and (buf[64 + cap:] == 0xA5).all()
        rc, _, length, buf, cap = _host_call(a, params, cap=0)
        assert rc == 0 and length == len(raw) and (buf == 0xA5).all()


def test_the_capacity_bounds_every_case_and_an_adversarial_image():
    lib = L.load()
    fx = E.fixture()["cases"]
    for name, w, h, s, quality, kind, restart, _ in CASES:
        raw = fx[name][1]
        info, params = J.info(raw), _params(s, quality, restart)
        cap = lib.es_jpeg_encode_capacity(C.byref(info), C.byref(params))
        blocks = sum(info.blocks_w[c] * info.blocks_h[c] for c in range(info.components))
        intervals = -(-info.mcus_x * info.mcus_y // restart) if restart else 1
        header = R.find(raw, 0xDA)[0][0] + 2 + R.find(raw, 0xDA)[0][1]
        assert cap == header + 2 * (-(-blocks * 1660 // 8) + intervals + 2 * (intervals - 1)) + 2, name       # the stated derivation
        assert cap >= len(raw), name
    # quality 100 (all-ones tables) on noise of the full range, and on the image of extreme blocks: the longest codes there are
    g = np.random.default_rng(3)
    for a in (g.integers(0, 2, size=(64, 64, 3)).astype(np.uint8) * 255, E.content(64, 64, "extreme", 0, False)):
        for sub in (0, 2):
            for restart in (0, 1):
                params = L.JpegEncodeParams(100, sub, restart)
                info = L.JpegInfo()
                assert lib.es_jpeg_encode_info_host(64, 64, 3, C.byref(params), C.byref(info)) == 0
                cap = lib.es_jpeg_encode_capacity(C.byref(info), C.byref(params))
                got = J.encode_host(a, quality=100, subsampling=sub, restart_marker_blocks=restart)
                assert 0 < len(got) <= cap, (sub, restart, len(got), cap)


# ---- the C++ host ------------------------------------------------------------------------------------------------------------------
def test_cpp_jpeg_encode_host_dry_builds_with_the_plain_host_compiler_and_reproduces_fixture_files(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) on the PATH")
    exe = str(tmp_path / "jpeg_encode_host_dry")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-DJPEG_HOST_DRY", "-I" + os.path.join(ROOT, "edgestyle_amd", "csrc"),
                        os.path.join(ROOT, "examples", "jpeg_encode_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-2000:]
    for name, flags in (("23x37_420_q30", ["-q", "30"]), ("33x18_gray_q100_rst", ["-q", "100", "-r", "1"]),
                        ("17x23_422_q30", ["-q", "30", "-s", "422"]), ("17x23_defaults", [])):
        a, raw = E.fixture()["cases"][name]
        h, w = a.shape[:2]
        (tmp_path / "in.pnm").write_bytes((b"P5" if a.ndim == 2 else b"P6") + b"\n# a comment\n%d %d\n255\n" % (w, h) + a.tobytes())
        r = subprocess.run([exe, str(tmp_path / "in.pnm"), str(tmp_path / "out.jpg")] + flags, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        assert (tmp_path / "out.jpg").read_bytes() == raw, name
        assert f"{w} x {h}" in r.stdout and f"{len(raw)} bytes" in r.stdout
    r = subprocess.run([exe, str(tmp_path / "in.pnm"), str(tmp_path / "bad.jpg"), "-q", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and "quality" in r.stderr and not (tmp_path / "bad.jpg").exists()

"""The JPEG decoder without a GPU (csrc/jpeg.h through the library's host entry points): es_jpeg_reconstruct_host over
es_jpeg_entropy_decode_host against the pixels Pillow decoded from the same files (tests/golden/jpeg.safetensors, and live Pillow where
it is importable), every refusal with its reason, a truncation / corruption sweep with guard bytes around the coefficient buffer, and
examples/jpeg_host.cpp built with -DJPEG_HOST_DRY by the plain host compiler.  Every comparison is an equality."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from edgestyle_amd import jpeg as J, lib as L
from tests import jpeg_ref as R

NEW_SYMBOLS = ("es_jpeg_info_host", "es_jpeg_coeff_count", "es_jpeg_entropy_decode_host", "es_jpeg_reconstruct_workspace_bytes",
               "es_jpeg_reconstruct", "es_jpeg_reconstruct_host", "es_jpeg_decode_staging_bytes", "es_jpeg_decode_u8")
CASES = R.cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_new_symbols_and_the_abi_version_stays():
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS and getattr(lib, name)
    assert lib.es_abi_version() == L.ABI_VERSION == 7


@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_host_decoder_equals_pillows_pixels_in_the_fixture(sampling):
    """every size, both qualities, noise and smooth content, with and without restart markers, optimised Huffman tables"""
    fx = R.fixture()["cases"]
    seen = 0
    for name, w, h, s, *_ in CASES:
        if s != sampling:
            continue
        raw, want = fx[name]
        info = J.info(raw)
        assert (info.width, info.height, info.components) == (w, h, 1 if s == "gray" else 3), name
        assert (info.hmax, info.vmax) == {"444": (1, 1), "422": (2, 1), "420": (2, 2), "gray": (1, 1)}[s], name
        assert (info.restart_interval > 0) == name.endswith("_rst"), name
        got = J.decode_host(raw)
        assert got.shape == want.shape == (h, w, 3) and np.array_equal(got, want), (name, int((got != want).sum()))
        seen += 1
    assert seen >= 2 * len(R.SIZES)


def test_info_reports_the_geometry_and_the_coefficients_are_block_major_per_component():
    raw, _ = R.fixture()["cases"]["17x23_420_q30"]
    info, coeffs, qtables = J.entropy_decode(raw)
    assert (info.mcus_x, info.mcus_y) == (2, 2) and list(info.blocks_w) == [4, 2, 2] and list(info.blocks_h) == [4, 2, 2]
    assert list(info.h) == [2, 1, 1] and list(info.v) == [2, 1, 1] and list(info.tq) == [0, 1, 1]
    assert coeffs.shape == ((16 + 4 + 4) * 64,) and qtables.shape == (3, 64)
    assert L.load().es_jpeg_coeff_count(C.byref(info)) == coeffs.size
    assert np.array_equal(qtables[1], qtables[2]) and not np.array_equal(qtables[0], qtables[1])
    assert qtables[0][0] < qtables[0][63]                  # natural order: the DC step first, the highest frequency last
    raw100, _ = R.fixture()["cases"]["17x23_420_q100_rst"]
    assert (J.entropy_decode(raw100)[2] == 1).all()        # quality 100: all-ones tables


def test_a_16_bit_quantisation_table_gives_the_same_pixels():
    raw, want = R.fixture()["cases"][R.DQT16_SOURCE]
    wide = R.dqt_to_16_bit(raw)
    assert len(wide) == len(raw) + 2 * 64 and wide != raw
    assert np.array_equal(J.decode_host(wide), want)
    assert np.array_equal(J.entropy_decode(wide)[2], J.entropy_decode(raw)[2])


def test_the_real_photo_decodes_to_the_pixels_pillow_gave():
    fx = R.fixture()
    assert len(fx["photo"]) == 11050
    got = J.decode_host(fx["photo"])
    assert got.shape == (512, 512, 3) and R.sha256(got) == fx["photo_sha256"]


def test_a_list_decodes_to_a_list_and_a_pitched_output_keeps_its_row_tails(tmp_path):
    fx = R.fixture()["cases"]
    names = ["9x5_420_q30", "23x37_gray_q100_rst", "33x18_422_q30"]
    path = tmp_path / "a.jpg"
    path.write_bytes(fx[names[0]][0])
    got = J.decode_host([str(path), fx[names[1]][0], bytearray(fx[names[2]][0])])
    assert isinstance(got, list) and all(np.array_equal(g, fx[n][1]) for g, n in zip(got, names))
    raw, want = fx["33x18_420_q30"]
    info, coeffs, qtables = J.entropy_decode(raw)
    buf = np.full((18 + 2, 33 * 3 + 5), 0xA5, dtype=np.uint8)
    view = buf[1:19, :99].reshape(18, 33, 3)
    J.reconstruct_host([info], [coeffs], [qtables], out=[view])
    assert np.array_equal(view, want) and (buf[:, 99:] == 0xA5).all() and (buf[0] == 0xA5).all() and (buf[19] == 0xA5).all()


@pytest.mark.skipif(not R.have_pillow(), reason="live Pillow is not importable")
@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_host_decoder_equals_live_pillow(sampling):
    """other content and qualities than the fixture's, a restart interval of 2 MCUs, and a 60 x 45 photo-like image"""
    for k, (w, h) in enumerate([(2, 6), (9, 5), (17, 23), (33, 18), (60, 45)]):
        for quality, kind, restart in ((50, "noise", 0), (95, "photo", 2), (100, "smooth", 0)):
            raw = R.encode(R.content(w, h, kind, 7000 + k, sampling == "gray"), sampling, quality, restart)
            got, want = J.decode_host(raw), R.pillow_rgb(raw)
            assert np.array_equal(got, want), (w, h, sampling, quality, kind, restart, int((got != want).sum()))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _refused(raw: bytes, *words):
    """the file is refused by the header parser or by the entropy decoder, and the reason holds one of the words"""
    lib = L.load()
    info = L.JpegInfo()
    rc = lib.es_jpeg_info_host(raw, len(raw), C.byref(info))
    if rc == 0:
        coeffs = np.empty((int(lib.es_jpeg_coeff_count(C.byref(info))),), dtype=np.int16)
        qt = np.empty((3, 64), dtype=np.uint16)
        rc = lib.es_jpeg_entropy_decode_host(raw, len(raw), C.byref(info), coeffs.ctypes.data, qt.ctypes.data)
    msg = lib.es_last_error().decode()
    assert rc == -1 and any(w in msg for w in words), (rc, msg)
    with pytest.raises(L.EdgeStyleHipError):
        J.decode_host(raw)
    return msg


def _base(name="17x23_420_q30"):
    return R.fixture()["cases"][name][0]


def test_refuses_progressive_lossless_and_arithmetic_files():
    raw = _base()
    p = R.sof_offset(raw)
    _refused(R.patch(raw, p + 1, b"\xc2"), "progressive")
    _refused(R.patch(raw, p + 1, b"\xc3"), "lossless")
    _refused(R.patch(raw, p + 1, b"\xc9"), "arithmetic")
    _refused(R.with_segment_before_sof(raw, b"\xff\xcc\x00\x04\x00\x10"), "arithmetic")        # a DAC segment
    if R.have_pillow():
        _refused(R.encode(R.content(17, 23, "noise", 1, False), "420", 75, progressive=True), "progressive")


def test_refuses_12_bit_samples_cmyk_and_files_that_are_not_ycbcr():
    raw = _base()
    p = R.sof_offset(raw)
    _refused(R.patch(raw, p + 4, b"\x0c"), "12-bit")
    _refused(R.patch(raw, p + 9, b"\x04"), "CMYK")
    if R.have_pillow():
        import io
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(R.content(9, 5, "noise", 2, False)).convert("CMYK").save(buf, "JPEG")
        _refused(buf.getvalue(), "CMYK")
    bare = R.without_segment(raw, 0xE0)                    # no JFIF marker: Adobe decides, then the ids
    assert np.array_equal(J.decode_host(bare), R.fixture()["cases"]["17x23_420_q30"][1])          # ids 1, 2, 3: YCbCr
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00"
    assert np.array_equal(J.decode_host(R.with_segment_before_sof(bare, adobe + b"\x01")), R.fixture()["cases"]["17x23_420_q30"][1])
    _refused(R.with_segment_before_sof(bare, adobe + b"\x00"), "Adobe transform")
    q = R.sof_offset(bare)
    rgb_ids = R.patch(R.patch(R.patch(bare, q + 10, b"R"), q + 13, b"G"), q + 16, b"B")
    s = R.find(rgb_ids, 0xDA)[0][0]
    rgb_ids = R.patch(R.patch(R.patch(rgb_ids, s + 5, b"R"), s + 7, b"G"), s + 9, b"B")
    _refused(rgb_ids, "R, G, B")


def test_refuses_other_sampling_factors_multi_scan_files_and_empty_sizes():
    raw = _base()
    p = R.sof_offset(raw)
    _refused(R.patch(raw, p + 11, b"\x41"), "sampling")    # 4:1:1
    _refused(R.patch(raw, p + 11, b"\x12"), "sampling")    # 1x2
    _refused(R.patch(raw, p + 14, b"\x21"), "sampling")    # subsampled luma against wider chroma
    # (Pillow's encoder writes no 4:1:1 file - its "4:1:1" is 4:2:0 - so these are header edits)
    _refused(R.patch(raw, p + 5, b"\x00\x00"), "height or width")
    _refused(R.patch(raw, p + 7, b"\x00\x00"), "height or width")
    s, n = R.find(raw, 0xDA)[0]
    one = raw[:s] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + raw[s + 2 + n:]       # a scan of the first component only
    _refused(one, "multi-scan")
    two = raw[:-2] + raw[s:]                               # a second scan where EOI must stand
    _refused(two, "multi-scan")
    _refused(R.patch(raw, s + 2 + n - 3, b"\x01"), "spectral")


def test_refuses_missing_tables_bad_codes_runs_past_63_and_bad_restart_markers():
    raw = _base()
    _refused(R.without_segment(raw, 0xDB), "quantisation table")
    _refused(R.without_segment(raw, 0xC4), "Huffman table")
    _refused(raw[:-2], "EOI")
    _refused(raw[:-40], "truncated")
    _refused(b"\x89PNG\r\n\x1a\n" + raw, "SOI")
    # a DHT whose counts overflow the code space
    d, n = R.find(raw, 0xC4)[0]
    _refused(R.patch(raw, d + 5, b"\x03"), "DHT")          # three codes of length 1
    # an AC table that maps every code to (run 15, size 1): the first block runs past coefficient 63
    ac = [(p, n) for p, n in R.find(raw, 0xC4) if raw[p + 4] >> 4 == 1][0]
    total = ac[1] - 2 - 17
    _refused(R.patch(raw, ac[0] + 21, bytes([0xF1]) * total), "past coefficient 63", "truncated", "Huffman code")
    rst, _ = R.fixture()["cases"]["33x18_420_q30_rst"]
    first = rst.index(b"\xff\xd0")
    assert np.array_equal(J.decode_host(rst), R.fixture()["cases"]["33x18_420_q30_rst"][1])
    _refused(R.patch(rst, first + 1, b"\xd1"), "RSTn")     # misnumbered
    _refused(rst[:first] + rst[first + 2:], "RSTn", "Huffman code", "truncated", "past coefficient 63")      # missing
    fill = rst[:first] + b"\xff\xff\xff" + rst[first:]     # fill bytes in front of a marker are legal
    assert np.array_equal(J.decode_host(fill), R.fixture()["cases"]["33x18_420_q30_rst"][1])


def test_bad_arguments_are_refused_before_anything_is_touched():
    lib = L.load()
    info = L.JpegInfo()
    assert lib.es_jpeg_info_host(None, 10, C.byref(info)) == -1 and b"null" in lib.es_last_error()
    raw = _base()
    good = J.info(raw)
    bad = L.JpegInfo.from_buffer_copy(good)
    bad.blocks_w[0] = 1000                                 # a derived field that does not belong to the size
    assert lib.es_jpeg_coeff_count(C.byref(bad)) == 0 and b"derived" in lib.es_last_error()
    assert lib.es_jpeg_reconstruct_workspace_bytes(C.byref(bad), 1) == 0
    wide = L.JpegInfo.from_buffer_copy(good)
    wide.width = 65536                                     # (a file's 16-bit fields cannot say this; a caller's struct can)
    assert lib.es_jpeg_coeff_count(C.byref(wide)) == 0 and b"65535" in lib.es_last_error()
    assert lib.es_jpeg_reconstruct_workspace_bytes(C.byref(good), 1) == 16 + (16 + 4 + 4) * 64
    assert lib.es_jpeg_decode_staging_bytes(C.byref(good), 1) == (16 + 4 + 4) * 64 * 2 + 384
    other = J.info(_base("9x5_420_q30"))
    coeffs = np.empty((int(lib.es_jpeg_coeff_count(C.byref(good))),), dtype=np.int16)
    qt = np.empty((3, 64), dtype=np.uint16)
    assert lib.es_jpeg_entropy_decode_host(raw, len(raw), C.byref(other), coeffs.ctypes.data, qt.ctypes.data) == -1
    assert b"info" in lib.es_last_error()


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------
def test_every_prefix_and_every_single_byte_corruption_is_an_error_or_an_image_and_stays_inside_the_buffer():
    """every proper prefix of one small file, and the file with each single byte of its first 700 set to 0xFF and to 0x00: each call
    returns 0 or -1 with a reason, and the guard values on both sides of the coefficient and table buffers stay"""
    lib = L.load()
    raw = _base(R.SWEEP_SOURCE)
    assert 600 < len(raw) < 700
    guard = 4096
    images = errors = 0
    for bad in R.sweep(raw):
        info = L.JpegInfo()
        rc = lib.es_jpeg_info_host(bad, len(bad), C.byref(info))
        assert rc in (0, -1)
        if rc == -1:
            assert lib.es_last_error()
            errors += 1
            continue
        count = int(lib.es_jpeg_coeff_count(C.byref(info)))
        assert 0 < count <= 1 << 22, count                 # (a corrupted size byte may ask for a large image: 65535 wide at most here)
        buf = np.full((guard + count + guard,), 0x5A5A, dtype=np.int16)
        qbuf = np.full((64 + 192 + 64,), 0xA5A5, dtype=np.uint16)
        rc = lib.es_jpeg_entropy_decode_host(bad, len(bad), C.byref(info), buf[guard:].ctypes.data, qbuf[64:].ctypes.data)
        assert rc in (0, -1)
        assert (buf[:guard] == 0x5A5A).all() and (buf[guard + count:] == 0x5A5A).all()
        assert (qbuf[:64] == 0xA5A5).all() and (qbuf[256:] == 0xA5A5).all()
        if rc == -1:
            assert lib.es_last_error()
            errors += 1
            continue
        if info.width * info.height <= 1 << 16:
            out = J.reconstruct_host([info], [buf[guard:guard + count]], [qbuf[64:64 + 64 * info.components]])
            assert out[0].shape == (info.height, info.width, 3)
        images += 1
    assert errors > len(raw) and images > 100              # every prefix is an error; many corruptions still decode


# ---- the C++ host ------------------------------------------------------------------------------------------------------------------
def test_cpp_jpeg_host_dry_builds_with_the_plain_host_compiler_and_writes_the_expected_ppm(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) on the PATH")
    exe = str(tmp_path / "jpeg_host_dry")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-DJPEG_HOST_DRY", "-I" + os.path.join(ROOT, "edgestyle_amd", "csrc"),
                        os.path.join(ROOT, "examples", "jpeg_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-2000:]
    for name in ("23x37_420_q30", "33x18_gray_q100_rst"):
        raw, want = R.fixture()["cases"][name]
        (tmp_path / "in.jpg").write_bytes(raw)
        r = subprocess.run([exe, str(tmp_path / "in.jpg"), str(tmp_path / "out.ppm")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        h, w = want.shape[:2]
        assert (tmp_path / "out.ppm").read_bytes() == b"P6\n%d %d\n255\n" % (w, h) + want.tobytes(), name
        assert f"{w} x {h}" in r.stdout
    (tmp_path / "bad.jpg").write_bytes(R.fixture()["cases"]["23x37_420_q30"][0][:300])
    r = subprocess.run([exe, str(tmp_path / "bad.jpg"), str(tmp_path / "bad.ppm")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and "truncated" in r.stderr and not (tmp_path / "bad.ppm").exists()

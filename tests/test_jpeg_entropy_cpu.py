"""The parallel Huffman decoder without a GPU: es_jpeg_scan_prepare_host plus es_jpeg_entropy_decode_parallel_host - the host twin of
csrc/jpeg_entropy.hip, the same __host__ __device__ code and the same synchronise rounds, run one decoder after the other - against the
serial decoder es_jpeg_entropy_decode_host.  Inputs: the files of tests/golden/jpeg.safetensors and files written here by
es_jpeg_encode_host.  Every comparison is an equality: the coefficients must not depend on the number of decoders or on the bytes per
subsequence, and a file is accepted exactly when the serial decoder accepts it."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from edgestyle_amd import jpeg as J, lib as L
from tests import jpeg_ref as R

NEW_SYMBOLS = ("es_jpeg_segment_count", "es_jpeg_scan_prepare_host", "es_jpeg_entropy_decode_workspace_bytes", "es_jpeg_entropy_decode",
               "es_jpeg_entropy_decode_parallel_host", "es_jpeg_status_text", "es_jpeg_decode_dev_staging_bytes", "es_jpeg_decode_dev_u8")
CASES = R.cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = (1, 2, 7, 64, 1024)
SUBSEQ = (0, 4, 5, 8, 32)
DEFAULT_SUBSEQ = 128
GUARD = 4096
POISON = 0x5A5A
SWEEP_MAX_COEFFS = 1 << 22                                # sweep variants whose corrupted size asks for more are left out, in both tiers


# ---- the two routes, on raw bytes ----------------------------------------------------------------------------------------------------
def serial(raw: bytes):
    """-> (coefficients, None) of the serial route (es_jpeg_info_host + es_jpeg_entropy_decode_host), or (None, the reason)"""
    lib = L.load()
    info = L.JpegInfo()
    if lib.es_jpeg_info_host(raw, len(raw), C.byref(info)) != 0:
        return None, lib.es_last_error().decode()
    coeffs = np.empty((int(lib.es_jpeg_coeff_count(C.byref(info))),), dtype=np.int16)
    qt = np.empty((3, 64), dtype=np.uint16)
    if lib.es_jpeg_entropy_decode_host(raw, len(raw), C.byref(info), coeffs.ctypes.data, qt.ctypes.data) != 0:
        return None, lib.es_last_error().decode()
    return coeffs, None


def prepare(raw: bytes):
    """-> (info, segments, tables, None), or (info | None, None, None, the reason) where the header or the prepare step refuses"""
    lib = L.load()
    info = L.JpegInfo()
    if lib.es_jpeg_info_host(raw, len(raw), C.byref(info)) != 0:
        return None, None, None, lib.es_last_error().decode()
    segments = np.zeros((int(lib.es_jpeg_segment_count(C.byref(info))), 2), dtype=np.uint32)
    tables = np.zeros((L.JPEG_TABLES_BYTES,), dtype=np.uint8)
    qt = np.zeros((3, 64), dtype=np.uint16)
    if lib.es_jpeg_scan_prepare_host(raw, len(raw), C.byref(info), segments.ctypes.data, tables.ctypes.data, qt.ctypes.data) != 0:
        return info, None, None, lib.es_last_error().decode()
    return info, segments, tables, None


def twin(raw: bytes, info, segments, tables, threads: int, subseq: int):
    """-> (coefficients, status, rounds); the coefficient buffer lies between guard values, which must keep their poison"""
    lib = L.load()
    count = int(lib.es_jpeg_coeff_count(C.byref(info)))
    buf = np.full((GUARD + count + GUARD,), POISON, dtype=np.int16)
    status = np.full((3,), -7, dtype=np.int32)
    rounds = C.c_int32(-1)
    data = np.frombuffer(raw, dtype=np.uint8)
    rc = lib.es_jpeg_entropy_decode_parallel_host(C.byref(info), 1, (C.c_void_p * 1)(data.ctypes.data), (C.c_size_t * 1)(len(raw)),
                                                  (C.c_void_p * 1)(segments.ctypes.data), (C.c_void_p * 1)(tables.ctypes.data), subseq, threads,
                                                  (C.c_void_p * 1)(buf[GUARD:].ctypes.data), status[1:].ctypes.data, C.byref(rounds))
    assert rc == 0, lib.es_last_error()
    assert (buf[:GUARD] == POISON).all() and (buf[GUARD + count:] == POISON).all(), "a store outside the coefficient buffer"
    assert status[0] == -7 and status[2] == -7
    return buf[GUARD:GUARD + count], int(status[1]), int(rounds.value)


def round_bound(segments, threads: int, subseq: int) -> int:
    """J + 1 of the longest segment: S = max(subseq_bytes, ceil(len / T)), J = ceil(len / S)"""
    most = 0
    for begin, end in segments.tolist():
        n = end - begin
        s = max(subseq or DEFAULT_SUBSEQ, -(-n // threads))
        most = max(most, -(-n // s) if n else 0)
    return most + 1


def same_as_serial(raw: bytes, threads=THREADS, subseq=SUBSEQ, name=""):
    """the decision and, where the file is accepted, the coefficients of both routes, for every pair of parameters"""
    want, why = serial(raw)
    info, segments, tables, refused = prepare(raw)
    if refused is not None:
        assert want is None and refused, (name, why, refused)
        return False
    for t in threads:
        for s in subseq:
            got, status, rounds = twin(raw, info, segments, tables, t, s)
            assert 0 <= rounds <= round_bound(segments, t, s), (name, t, s, rounds)
            if want is None:
                assert status != 0 and J.status_text(status), (name, t, s, why)
            else:
                assert status == 0, (name, t, s, J.status_text(status))
                assert np.array_equal(got, want), (name, t, s, int((got != want).sum()))
    return want is not None


# ---- files written here by the project's own encoder -----------------------------------------------------------------------------------
_generated = None


def generated():
    """{name: file bytes}: noise at quality 100 (long codes, dense FF 00), smooth content at quality 10 (EOB-only blocks, many blocks
    per subsequence), and two sizes with partial MCUs at each sampling with restart intervals 0, 1, 2 and mcus_x (made once)"""
    global _generated
    if _generated is None:
        out = {}
        sub = {"444": "4:4:4", "422": "4:2:2", "420": "4:2:0", "gray": "4:4:4"}
        out["noise_q100"] = J.encode_host(R.content(64, 48, "noise", 11, False), quality=100, subsampling="4:2:0")
        out["smooth_q10"] = J.encode_host(R.content(64, 48, "smooth", 12, False), quality=10, subsampling="4:2:0")
        for w, h in ((17, 23), (33, 18)):
            for s in R.SAMPLINGS:
                mcus_x = -(-w // (8 if s in ("444", "gray") else 16))
                for k, ri in enumerate((0, 1, 2, mcus_x)):
                    a = R.content(w, h, "noise" if k % 2 == 0 else "photo", 100 + w + k, s == "gray")
                    out[f"{w}x{h}_{s}_ri{k}"] = J.encode_host(a, quality=(35, 90, 100, 60)[k], subsampling=sub[s], restart_marker_blocks=ri)
        _generated = out
    return _generated


# ---- tests -----------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_symbols_and_the_abi_version_stays():
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS and getattr(lib, name)
    assert lib.es_abi_version() == L.ABI_VERSION == 7
    assert J.status_text(0) and "Huffman code (DC)" in J.status_text(1) and "Huffman code (AC)" in J.status_text(2)
    assert "past coefficient 63" in J.status_text(3) and "outside 16 bits" in J.status_text(4) and "truncated" in J.status_text(5)


def test_prepare_finds_the_segments_between_the_restart_markers():
    fx = R.fixture()["cases"]
    raw = fx["33x18_420_q30_rst"][0]
    info, segments, tables, qt = J.scan_prepare(raw)
    assert info.restart_interval == 1 and len(segments) == info.mcus_x * info.mcus_y == 6
    for k, (begin, end) in enumerate(segments.tolist()):
        assert raw[end] == 0xFF and raw[end + 1] == (0xD0 + k if k < 5 else 0xD9)
        assert begin == (segments[k - 1][1] + 2 if k else R.find(raw, 0xDA)[0][0] + 2 + R.find(raw, 0xDA)[0][1])
    one = J.scan_prepare(fx["33x18_420_q30"][0])[1]
    assert one.shape == (1, 2) and one[0][1] == len(fx["33x18_420_q30"][0]) - 2
    assert np.array_equal(qt, J.entropy_decode(raw)[2])
    lib = L.load()
    assert lib.es_jpeg_entropy_decode_workspace_bytes(C.byref(info), 1) == 16 + 32        # one word per segment, in units of 16 bytes
    up = C.c_size_t(0)
    total = lib.es_jpeg_decode_dev_staging_bytes(C.byref(info), (C.c_size_t * 1)(len(raw)), 1, C.byref(up))
    assert up.value == (len(raw) + 15) // 16 * 16 + 48 + L.JPEG_TABLES_BYTES + 384
    assert total == up.value + int(lib.es_jpeg_coeff_count(C.byref(info))) * 2 + 48


@pytest.mark.parametrize("sampling", R.SAMPLINGS)
def test_the_twin_equals_the_serial_decoder_on_every_fixture_file_whatever_the_parameters(sampling):
    """restart interval 1, optimised tables, gray, 4:4:4, 4:2:2, 4:2:0, partial MCUs: threads in {1, 2, 7, 64, 1024} x subseq_bytes in
    {0, 4, 5, 8, 32}"""
    fx = R.fixture()["cases"]
    seen = 0
    for name, w, h, s, *_ in CASES:
        if s == sampling:
            assert same_as_serial(fx[name][0], name=name), name
            seen += 1
    assert seen >= 2 * len(R.SIZES)


def test_the_twin_equals_the_serial_decoder_on_the_16_bit_table_rewrite_and_the_photo():
    fx = R.fixture()
    assert same_as_serial(R.dqt_to_16_bit(fx["cases"][R.DQT16_SOURCE][0]), name="dqt16")
    assert same_as_serial(fx["photo"], name="photo")
    info, coeffs, qtables, status, rounds = J.entropy_decode_parallel_host(fx["photo"], 1024)
    assert status == 0 and R.sha256(J.reconstruct_host([info], [coeffs], [qtables])[0]) == fx["photo_sha256"]


def test_the_twin_equals_the_serial_decoder_on_generated_files():
    for name, raw in generated().items():
        assert same_as_serial(raw, name=name), name
    assert generated()["noise_q100"].count(b"\xff\x00") > 20        # dense stuffing
    assert len(generated()["smooth_q10"]) < 64 * 48 // 2


def test_fill_bytes_and_ff_ff_00_read_as_the_serial_decoder_reads_them():
    """FF FF 00 in the scan is ONE data byte FF; FF fill bytes may stand before an RSTn marker.  The decision and the coefficients of
    each edited file are the serial decoder's."""
    raw = generated()["17x23_420_ri1"]
    scan = R.find(raw, 0xDA)[0][0] + 2 + R.find(raw, 0xDA)[0][1]
    want, _ = serial(raw)
    stuffed = [i for i in range(scan, len(raw) - 2) if raw[i] == 0xFF and raw[i + 1] == 0x00]
    rst = [i for i in range(scan, len(raw) - 2) if raw[i] == 0xFF and 0xD0 <= raw[i + 1] <= 0xD7]
    assert len(stuffed) >= 2 and len(rst) >= 2
    edits = []
    for i in (stuffed[0], stuffed[-1]):
        edits.append(raw[:i] + b"\xff" + raw[i:])                      # FF 00 -> FF FF 00: the same data
        edits.append(raw[:i] + b"\xff\xff\xff" + raw[i:])
    for i in (rst[0], rst[-1]):
        edits.append(raw[:i] + b"\xff\xff\xff" + raw[i:])              # fill bytes before RSTn
    both = raw[:stuffed[0]] + b"\xff" + raw[stuffed[0]:rst[-1]] + b"\xff\xff" + raw[rst[-1]:]
    edits.append(both)
    for k, e in enumerate(edits):
        got, why = serial(e)
        assert got is not None and np.array_equal(got, want), (k, why)
        assert same_as_serial(e, name=f"edit{k}")
    # a data byte FF where none was (FF FF 00 in the middle of other data), a stuffed byte taken away, a marker's FF doubled into data
    plain = [i for i in range(scan + 1, len(raw) - 2) if raw[i] != 0xFF and raw[i - 1] != 0xFF][5]
    for k, e in enumerate((raw[:plain] + b"\xff\xff\x00" + raw[plain:], raw[:stuffed[0] + 1] + raw[stuffed[0] + 2:],
                           raw[:rst[0]] + b"\xff\x00" + raw[rst[0]:], raw[:rst[1]] + b"\x00" + raw[rst[1]:])):
        same_as_serial(e, threads=(1, 16, 1024), subseq=(0, 4, 8), name=f"hostile{k}")


_stray = None


def stray_variants():
    """[(name, file bytes, the original file)]: stray DATA bytes (not FF fills) before EOI and before an RSTn marker, which the serial
    decoder skips: FF 00 and 8, 40, 300 or 600 seeded bytes below FF - up to 150 subsequences of 4 bytes and more than two of the
    default 128 behind the segment's last block (made once)"""
    global _stray
    if _stray is None:
        fx = R.fixture()
        out = []
        g = np.random.default_rng(77)
        for name, raw in (("33x18_420_q30", fx["cases"]["33x18_420_q30"][0]), ("60x45_420_q90", fx["cases"]["60x45_420_q90"][0]),
                          ("photo", fx["photo"]), ("33x18_420_q30_rst", fx["cases"]["33x18_420_q30_rst"][0]),
                          ("33x18_444_ri2", generated()["33x18_444_ri2"])):
            marks = [len(raw) - 2]
            scan = R.find(raw, 0xDA)[0][0] + 2 + R.find(raw, 0xDA)[0][1]
            rst = [i for i in range(scan, len(raw) - 2) if raw[i] == 0xFF and 0xD0 <= raw[i + 1] <= 0xD7]
            if rst:
                marks += [rst[0], rst[-1]]
            for at in marks:
                for k in (8, 40, 300, 600):
                    junk = b"\xff\x00" + bytes(g.integers(0, 255, size=k).astype(np.uint8))
                    out.append((f"{name}@{at}+{k}", raw[:at] + junk + raw[at:], raw))
        _stray = out
    return _stray


def test_stray_bytes_before_eoi_and_before_rstn_are_no_error_and_change_no_coefficient():
    """the true decode runs past the segment's last block into the stray bytes and dies there on an impossible code; nothing behind
    that point may reach the coefficient buffer or the status, at 4 and 8 bytes per subsequence and at the default"""
    for name, raw, original in stray_variants():
        want, why = serial(raw)
        assert want is not None and np.array_equal(want, serial(original)[0]), (name, why)
        assert same_as_serial(raw, threads=(16, 1024), subseq=(0, 4, 8), name=name), name


def test_rounds_stay_within_j_plus_1_and_the_photo_settles_in_a_handful():
    """the synchronise loop is bounded by J + 1 rounds from the sizes alone (same_as_serial asserts it on every file above); the real
    512 x 512 photo at the default subsequence of 128 bytes and 1024 decoders settles in at most 4 (measured: 4; 11 at 32 bytes, 6 at
    64, 3 at 256, 2 at 512)"""
    fx = R.fixture()
    info, segments, tables, refused = prepare(fx["photo"])
    assert refused is None and len(segments) == 1
    _, status, rounds = twin(fx["photo"], info, segments, tables, 1024, 0)
    print("photo: rounds at the default S:", rounds, "J + 1:", round_bound(segments, 1024, 0))
    assert status == 0 and 1 <= rounds <= 4
    assert twin(fx["photo"], info, segments, tables, 1024, 128)[2] == rounds       # 0 means 128
    for t, s in ((1, 0), (1024, 4), (16, 4)):
        _, status, rounds = twin(fx["photo"], info, segments, tables, t, s)
        print("photo: threads", t, "subseq", s, "rounds", rounds)
        assert status == 0 and rounds <= round_bound(segments, t, s)
    assert twin(fx["photo"], info, segments, tables, 1, 0)[2] == 1      # one decoder: one round, nothing to exchange


def test_every_prefix_and_every_single_byte_corruption_is_decided_as_the_serial_decoder_decides_it():
    """the truncation and corruption sweep of tests/test_jpeg_cpu.py through the prepare step and the twin, 16 decoders and 4 bytes per
    subsequence: accepted exactly when the serial route accepts, equal coefficients where accepted, a non-zero status or a refusal by
    the prepare step with a text where not, and the guard values around the coefficient buffer intact on every variant (twin asserts
    that)"""
    raw = R.fixture()["cases"][R.SWEEP_SOURCE][0]
    accepted = refused_by_status = refused_by_prepare = 0
    for bad in R.sweep(raw):
        want, why = serial(bad)
        info, segments, tables, refused = prepare(bad)
        if refused is not None:
            assert want is None and refused, (why, refused)
            refused_by_prepare += 1
            continue
        if int(L.load().es_jpeg_coeff_count(C.byref(info))) > SWEEP_MAX_COEFFS:
            continue
        got, status, rounds = twin(bad, info, segments, tables, 16, 4)
        assert rounds <= round_bound(segments, 16, 4)
        if want is None:
            assert status != 0 and J.status_text(status), why
            refused_by_status += 1
        else:
            assert status == 0 and np.array_equal(got, want), (J.status_text(status), int((got != want).sum()))
            accepted += 1
    assert accepted > 100 and refused_by_status > 10 and refused_by_prepare > len(raw)


def test_bad_arguments_are_refused():
    lib = L.load()
    raw = R.fixture()["cases"]["17x23_420_q30"][0]
    info, segments, tables, _ = prepare(raw)
    data = np.frombuffer(raw, dtype=np.uint8)
    coeffs = np.zeros((int(lib.es_jpeg_coeff_count(C.byref(info))),), dtype=np.int16)
    status = np.zeros((1,), dtype=np.int32)

    def call(threads, subseq):
        return lib.es_jpeg_entropy_decode_parallel_host(C.byref(info), 1, (C.c_void_p * 1)(data.ctypes.data), (C.c_size_t * 1)(len(raw)),
                                                        (C.c_void_p * 1)(segments.ctypes.data), (C.c_void_p * 1)(tables.ctypes.data), subseq, threads,
                                                        (C.c_void_p * 1)(coeffs.ctypes.data), status.ctypes.data, None)
    assert call(0, 0) == -1 and b"threads" in lib.es_last_error()
    assert call(1025, 0) == -1 and b"threads" in lib.es_last_error()
    assert call(16, 3) == -1 and b"subseq_bytes" in lib.es_last_error()
    assert call(16, 4) == 0 and status[0] == 0
    other = J.info(R.fixture()["cases"]["9x5_420_q30"][0])
    qt = np.zeros((3, 64), dtype=np.uint16)
    assert lib.es_jpeg_scan_prepare_host(raw, len(raw), C.byref(other), segments.ctypes.data, tables.ctypes.data, qt.ctypes.data) == -1
    assert b"info" in lib.es_last_error()
    bad = L.JpegInfo.from_buffer_copy(info)
    bad.blocks_w[0] = 1000
    assert lib.es_jpeg_segment_count(C.byref(bad)) == 0 and b"derived" in lib.es_last_error()
    with pytest.raises(L.EdgeStyleHipError, match="truncated"):
        J.entropy_decode_parallel_host(raw[:-40], 16, 4)
    # segment offsets past the file are cut to it: a refusal by status, no read outside the bytes
    wild = segments.copy()
    wild[0][1] = 0xFFFFFFF0
    got, st, _ = twin(raw, info, wild, tables, 16, 4)
    assert st == 0 or J.status_text(st)


def test_cpp_jpeg_host_dry_parallel_compares_the_twin_with_the_serial_decoder(tmp_path):
    """examples/jpeg_host.cpp -DJPEG_HOST_DRY --parallel T S, built by the plain host compiler from csrc/jpeg.h alone"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) on the PATH")
    exe = str(tmp_path / "jpeg_host_dry")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-DJPEG_HOST_DRY", "-I" + os.path.join(ROOT, "edgestyle_amd", "csrc"),
                        os.path.join(ROOT, "examples", "jpeg_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-2000:]
    fx = R.fixture()["cases"]
    for name, t, s in (("23x37_420_q30", 16, 4), ("33x18_gray_q100_rst", 1024, 0), ("60x45_420_q90", 7, 5)):
        raw, want = fx[name]
        (tmp_path / "in.jpg").write_bytes(raw)
        r = subprocess.run([exe, "--parallel", str(t), str(s), str(tmp_path / "in.jpg"), str(tmp_path / "out.ppm")], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 0 and "equal to the serial decoder" in r.stdout, r.stdout + r.stderr
        h, w = want.shape[:2]
        assert (tmp_path / "out.ppm").read_bytes() == b"P6\n%d %d\n255\n" % (w, h) + want.tobytes(), name
    (tmp_path / "bad.jpg").write_bytes(fx["23x37_420_q30"][0][:-20])
    r = subprocess.run([exe, "--parallel", "16", "4", str(tmp_path / "bad.jpg"), str(tmp_path / "bad.ppm")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and "truncated" in r.stderr and "both refuse" in r.stderr and not (tmp_path / "bad.ppm").exists()

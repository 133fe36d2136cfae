"""Person crop and pose rendering without a GPU (csrc/image_io.hip: ES_FILTER_LANCZOS, es_person_crop_fit; csrc/pose.hip: the host
build of the drawing rule, the candidate choice, the point prompt) against tests/pose_ref.py and the fixture made from the reference's
own docs/test pose files.  Every comparison is an equality, except the PSNR / IoU condition the drawing rule is held to."""
import ctypes as C
import itertools

import numpy as np
import pytest

from edgestyle_amd import lib as L
from tests import pose_ref as R

NEW_SYMBOLS = ("es_person_crop_fit", "es_image_resize_window_u8_workspace_bytes", "es_image_resize_window_u8", "es_person_crop_u8_workspace_bytes",
               "es_person_crop_u8", "es_pose_draw", "es_pose_draw_host", "es_pose_select_host", "es_pose_points_host")
FAKE = C.c_void_p(0x1000)


def test_library_exports_the_new_symbols_and_the_abi_version_stays():
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS and getattr(lib, name)
    assert L.FILTER_LANCZOS == R.FILTER_LANCZOS == 2 and (L.FILTER_BILINEAR, L.FILTER_BICUBIC) == (0, 1)
    assert lib.es_abi_version() == L.ABI_VERSION == 7


# ---- Lanczos -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(R.LANCZOS_CASES)))
def test_lanczos_integer_resize_equals_pillows_bytes_in_the_fixture(case):
    """up, down, mixed and one-axis-only; R.resize_axis asserts on the way that every accumulator stays within 32 bits"""
    a, want = R.fixture()["lanczos"][case]
    h, w, nh, nw = R.LANCZOS_CASES[case]
    assert a.shape == (h, w, 3) and want.shape == (nh, nw, 3)
    got = R.integer_resize(a, nh, nw)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.skipif(not R.have_pillow(), reason="live Pillow is not importable")
@pytest.mark.parametrize("h,w,nh,nw", [(37, 53, 61, 40), (301, 200, 64, 43), (45, 60, 9, 7), (20, 31, 160, 32)])
def test_lanczos_integer_resize_equals_live_pillow(h, w, nh, nw):
    a = np.random.default_rng(h * w).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    a[:5, :5] = 255                                       # a saturated corner: the negative lobes push sums below 0 and above 255
    a[5:10, :5] = 0
    assert np.array_equal(R.integer_resize(a, nh, nw), R.pillow_lanczos(a, nh, nw))


def test_lanczos_taps_have_support_three_and_the_32_bit_accumulator_holds_for_any_bytes():
    for n_in, n_out in ((200, 43), (53, 40), (37, 61), (1024, 512), (768, 341), (4000, 7)):
        xmin, nt, k = R.coeffs(R.FILTER_LANCZOS, n_in, n_out)
        scale = max(n_in / n_out, 1.0)
        assert nt.max() <= int(2 * 3.0 * scale) + 2 and nt.max() >= min(n_in, int(2 * 3.0 * scale) - 1)
        assert (xmin >= 0).all() and (xmin + nt <= n_in).all()
        for i in range(n_out):
            taps = k[i, :nt[i]].astype(np.int64)
            assert abs(int(taps.sum()) - (1 << 22)) <= nt[i]          # normalised, up to the rounding of each tap
            assert (1 << 21) + 255 * int(np.abs(taps).sum()) < 2 ** 31
        assert (k.min(axis=1) < 0).any()                  # the lobes are there
    lib = L.load()
    assert lib.es_image_resize_coeffs_ex(3, 10, 10, None, None, None, 0) == -1 and b"filter" in lib.es_last_error()


# ---- create_processed_image's geometry --------------------------------------------------------------------------------------------
def test_person_crop_fit_equals_the_reference_arithmetic():
    cases = [
        (768, 1024, (300, 100, 700, 700), 512, 512),          # the usual: a box inside the photo
        (768, 1024, (0, 0, 1024, 768), 512, 512),             # the box is the photo: both margins are cut away
        (768, 1024, (0, 0, 200, 300), 512, 512),              # top-left corner
        (768, 1024, (900, 600, 1024, 768), 512, 512),         # bottom-right corner
        (768, 1024, (-50, -20, 1100, 900), 512, 512),         # larger than the photo before the margin
        (400, 300, (10, 10, 290, 390), 512, 512),             # larger than the photo after the margin
        (900, 150, (10, 50, 140, 850), 512, 512),             # tall narrow photo: new_w < final_w, left < 0
        (150, 900, (50, 10, 850, 140), 512, 512),             # wide flat photo: top < 0
        (333, 517, (100.5, 20.25, 300.75, 310.125), 64, 48),  # fractional box, other window
        (60, 45, (5, 4, 40, 50), 50, 67),
    ]
    for h, w, box, fw, fh in cases:
        assert R.crop_fit_lib(h, w, box, fw, fh) == R.crop_fit(h, w, box, fw, fh), (h, w, box)
    assert R.crop_fit_lib(900, 150, (10, 50, 140, 850))[2] < 0 and R.crop_fit_lib(150, 900, (50, 10, 850, 140))[3] < 0
    g = np.random.default_rng(11)
    for _ in range(400):
        h, w = int(g.integers(20, 1500)), int(g.integers(20, 1500))
        x0, x1 = sorted(g.uniform(-0.1 * w, 1.1 * w, size=2))
        y0, y1 = sorted(g.uniform(-0.1 * h, 1.1 * h, size=2))
        if x1 - x0 < 2 or y1 - y0 < 2 or min(x1, w) - max(x0, 0) < 2 or min(y1, h) - max(y0, 0) < 2:
            continue
        fw, fh = (512, 512) if g.random() < 0.5 else (int(g.integers(16, 700)), int(g.integers(16, 700)))
        assert R.crop_fit_lib(h, w, (x0, y0, x1, y1), fw, fh) == R.crop_fit(h, w, (x0, y0, x1, y1), fw, fh), (h, w, x0, y0, x1, y1, fw, fh)


def test_person_crop_fit_refuses_what_the_reference_cannot_compute():
    lib = L.load()
    out = (C.c_int32 * 4)()
    for box in ((10, 10, 10, 50), (-30, 0, -10, 50), (0, 0, float("nan"), 5)):         # empty, outside the photo, not a number
        assert lib.es_person_crop_fit(100, 100, (C.c_double * 4)(*box), 512, 512, 0.1, out) == -1 and lib.es_last_error()
    assert lib.es_person_crop_fit(0, 100, (C.c_double * 4)(0, 0, 5, 5), 512, 512, 0.1, out) == -1
    assert lib.es_person_crop_fit(100, 100, (C.c_double * 4)(0, 0, 5, 5), 0, 512, 0.1, out) == -1
    # and the window family's argument checks need no GPU either
    img = (L.ImageU8 * 1)()
    img[0].data, img[0].height, img[0].width, img[0].channels, img[0].row_stride = FAKE, 300, 200, 3, 600
    geom = (C.c_int32 * 4)(100, 150, -5, 7)
    lin = lib.es_image_resize_window_u8_workspace_bytes(img, 1, geom, 64, 64, L.FILTER_BILINEAR)
    lan = lib.es_image_resize_window_u8_workspace_bytes(img, 1, geom, 64, 64, L.FILTER_LANCZOS)
    assert 0 < lin < lan                                  # the wider filter keeps more source rows
    assert lib.es_image_resize_window_u8_workspace_bytes(img, 1, geom, 64, 64, 3) == 0 and b"filter" in lib.es_last_error()
    assert lib.es_image_resize_window_u8(img, 1, (C.c_int32 * 4)(0, 150, 0, 0), FAKE, 64, 64, 0, FAKE, 1 << 20, None) == -1
    assert lib.es_image_resize_window_u8(img, 1, geom, FAKE, 64, 64, L.FILTER_LANCZOS, FAKE, lan - 1, None) == -1 and b"workspace" in lib.es_last_error()


# ---- the drawing rule ----------------------------------------------------------------------------------------------------------------
def test_draw_host_equals_the_python_restatement_on_the_reference_poses():
    fx = R.fixture()
    got = R.draw_host(np.stack(fx["kp"]), 512, 512)
    for i in range(3):
        want = R.draw(fx["kp"][i], 512, 512)
        assert np.array_equal(got[i], want), (i, int((got[i] != want).sum()))


def test_the_drawing_rule_meets_the_closeness_condition_on_the_references_own_renderings():
    """>= 34.0 dB whole-image PSNR and IoU >= 0.92 (pixels whose largest channel exceeds 40) against each of the three JPEGs the
    reference's tool chain rendered from the same key points"""
    fx = R.fixture()
    got = R.draw_host(np.stack(fx["kp"]), 512, 512)
    for i in range(3):
        psnr, iou = R.psnr_iou(got[i], fx["jpg"][i])
        print(f"{R.POSES[i]}: PSNR {psnr:.2f} dB, IoU {iou:.4f}")
        assert psnr >= 34.0 and iou >= 0.92, (i, psnr, iou)


@pytest.mark.parametrize("H,W", [(48, 64), (67, 50), (33, 129)])
def test_draw_host_equals_the_python_restatement_on_a_seeded_sweep(H, W):
    """absent points (score 0, negative, NaN), points outside [0,1] (shapes clipped at every edge), coincident limb ends, far-away and
    NaN coordinates, on non-square canvases"""
    g = np.random.default_rng(1000 * H + W)
    poses = [R.random_pose(g, absent=a, spread=s) for a, s in itertools.product((0.0, 0.25, 0.6), (0.0, 0.3)) for _ in range(4)]
    same = R.random_pose(g, absent=0.0)
    same[2] = same[1]                                     # limb (2,3): both ends on one point
    same[5, :2] = same[1, :2] + np.float32(1e-4)          # limb (2,6): less than a pixel long
    poses.append(same)
    far = R.random_pose(g, absent=0.0)
    far[3, 0], far[6, 1], far[9, 0], far[12, 1] = 2000.0, -3000.0, np.nan, np.inf
    poses.append(far)
    edge = R.random_pose(g, absent=0.0)
    edge[:4, 0], edge[4:8, 0], edge[8:12, 1], edge[12:16, 1] = 0.0, 1.0, 0.0, 1.0
    poses.append(edge)
    poses.append(np.zeros((18, 3), dtype=np.float32))     # nothing present
    kp = np.stack(poses)
    got = R.draw_host(kp, H, W)
    for i in range(kp.shape[0]):
        want = R.draw(kp[i], H, W)
        assert np.array_equal(got[i], want), (i, int((got[i] != want).sum()))
    assert not got[-1].any() and got[:-1].any()


def test_a_limb_of_half_length_zero_is_a_stroke_across_it_and_the_order_of_drawing_holds():
    H, W = 40, 40
    kp = np.zeros((18, 3), dtype=np.float32)
    kp[1] = (0.5, 0.5, 1.0)                               # neck and right shoulder on one pixel: limb 1 = (2,3), a = 0, angle 0
    kp[2] = (0.5, 0.5, 1.0)
    img = R.draw_host(kp, H, W)[0]
    assert np.array_equal(img, R.draw(kp, H, W))
    limb = (img == np.array([153, 0, 0], dtype=np.uint8)).all(axis=2)
    disc3 = (img == np.array([255, 170, 0], dtype=np.uint8)).all(axis=2)          # point 3 is drawn after point 2: it wins
    assert disc3.sum() == 49 and disc3[20, 16] and disc3[20, 24] and disc3[16, 20] and not disc3[17, 17]      # x^2 + y^2 <= 16
    assert not (img == np.array([255, 85, 0], dtype=np.uint8)).all(axis=2).any()
    assert limb.sum() == 0                                # the stroke reaches 4 pixels up and down: it lies under the disc drawn after it
    only = R.records(kp, H, W)[0]
    cover = R.covers(only, H, W)
    ys, xs = np.nonzero(cover)
    assert xs.min() == xs.max() == 20 and ys.min() == 16 and ys.max() == 24                                       # one wide, nine long


def test_select_host_applies_each_filter_breaks_ties_in_input_order_and_reports_an_empty_result():
    fx = R.fixture()
    good = fx["kp"][0]
    assert R.select_host([good], [23.77], [13.0]) == 0
    assert R.select_host([good], [10.0], [13.0]) == -1            # score must exceed 10
    assert R.select_host([good], [23.77], [5.0]) == -1            # parts must exceed 5
    for gone, keep in (((0, 1, 14, 15, 16, 17), -1), ((0, 1, 14, 15, 16), 0), ((2, 5), -1), ((2,), 0), ((8, 11), -1), ((11,), 0)):
        kp = good.copy()
        for k in gone:
            kp[k, 2] = 0.0
        kp[17] = (0.7, 0.19, 1.0) if 17 not in gone else kp[17]   # (this pose has no left ear of its own)
        assert R.select_host([kp], [23.77], [13.0]) == keep, gone
    small = good.copy()
    small[:, :2] = 0.5 + (small[:, :2] - 0.5) * 0.5               # the same pose at half the size: a quarter of the area
    assert R.select_host([small, good], [20, 20], [13, 13]) == 1
    assert R.select_host([small, good, good], [20, 20, 20], [13, 13, 13]) == 1          # a tie: the first of the two
    assert R.select_host([good, small], [9, 20], [13, 13]) == 1                         # the larger one fails a filter
    assert R.select_host([small, good], [9, 20], [13, 3]) == -1
    assert R.select_host(np.zeros((0, 18, 3), dtype=np.float32), [], []) == -1
    for i, (score, parts) in enumerate(fx["scores"]):             # the reference kept all three of its own poses
        assert R.select_host([fx["kp"][i]], [score], [parts]) == 0


def test_points_host_gives_the_present_points_in_pixels_in_order():
    kp = R.fixture()["kp"][0]
    got = R.points_host(kp, 512, 512)
    present = kp[:, 2] > 0
    assert got.shape == (13, 2) and present.sum() == 13
    assert np.array_equal(got, (kp[present, :2].astype(np.float64) * np.array([512, 512])).astype(np.float32))
    assert tuple(got[0]) == (351.0, 116.0)                        # 0.685546875 * 512, 0.2265625 * 512
    got = R.points_host(kp, 640, 480)
    assert np.array_equal(got, (kp[present, :2].astype(np.float64) * np.array([640, 480])).astype(np.float32))
    none = np.zeros((18, 3), dtype=np.float32)
    none[3, 2] = np.nan
    assert R.points_host(none, 512, 512).shape == (0, 2)

"""Mask post-processing without a GPU (csrc/mask.hip): the C-ABI surface, every refusal (all of them come before the first HIP
call, so the pointers here are fakes that are never read), the workspace size, and the suite's own reference (tests/mask_ref.py)
against scipy.ndimage where scipy imports, plus the merged-radii identities the library relies on."""
import ctypes as C

import numpy as np
import pytest

from edgestyle_amd import lib as L
from tests import mask_ref as R

NEW_SYMBOLS = ("es_mask_workspace_bytes", "es_mask_morph", "es_mask_largest_component", "es_mask_logic", "es_image_mask_fill_u8",
               "es_sam_compose")
FAKE = C.c_void_p(1 << 20)            # an aligned address nobody reads: every call below is refused before a launch
SIZES = [(5, 9), (1, 1), (1, 40), (37, 53), (64, 64), (130, 67)]


def _err(lib) -> bytes:
    return lib.es_last_error() or b""


def _radii(*r):
    return (C.c_int32 * max(len(r), 1))(*r), len(r)


def test_symbols_resolve_and_the_abi_version_stays():
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS and getattr(lib, name)
    assert lib.es_abi_version() == 7 == L.ABI_VERSION
    assert (L.MASK_AND, L.MASK_OR, L.MASK_ANDNOT) == (0, 1, 2)


def test_workspace_bytes_is_positive_and_never_decreases():
    lib = L.load()
    for H, W, n in [(1, 1, 1), (5, 9, 1), (130, 67, 3), (512, 512, 8), (4096, 4096, 1), (4096, 4096, 4096)]:
        b = lib.es_mask_workspace_bytes(H, W, n)
        assert b > 0
        # ten packed masks and two int32 [H, W] arrays per image can never take less than this
        assert b >= n * (10 * H * ((W + 63) // 64) * 8 + 8 * H * W)
    for H in (1, 63, 64, 65, 130):
        for W in (1, 63, 64, 65, 128, 129):
            for n in (1, 2, 5):
                b = lib.es_mask_workspace_bytes(H, W, n)
                assert lib.es_mask_workspace_bytes(H + 1, W, n) >= b
                assert lib.es_mask_workspace_bytes(H, W + 1, n) >= b
                assert lib.es_mask_workspace_bytes(H, W, n + 1) >= b
    for H, W, n in [(0, 8, 1), (8, 0, 1), (4097, 8, 1), (8, 4097, 1), (8, 8, 0), (-1, 8, 1), (8, 8, 4097)]:
        assert lib.es_mask_workspace_bytes(H, W, n) == 0 and _err(lib)


@pytest.mark.parametrize("H,W", [(0, 8), (8, 0), (4097, 8), (8, 4097), (-3, 8)])
def test_every_call_refuses_a_height_or_width_outside_1_to_4096(H, W):
    lib = L.load()
    big = 1 << 40
    r, n = _radii(1, -1)
    col = (C.c_uint8 * 3)(127, 127, 127)
    assert lib.es_mask_morph(FAKE, FAKE, 1, H, W, r, n, FAKE, big, None) == -1 and b"1..4096" in _err(lib)
    assert lib.es_mask_largest_component(FAKE, FAKE, None, 1, H, W, FAKE, big, None) == -1 and b"1..4096" in _err(lib)
    assert lib.es_image_mask_fill_u8(None, FAKE, FAKE, 1, H, W, col, None) == -1 and b"1..4096" in _err(lib)
    assert lib.es_sam_compose(None, FAKE, FAKE, FAKE, FAKE, 1, H, W, FAKE, None, FAKE, big, None) == -1 and b"1..4096" in _err(lib)


def test_morph_refuses_long_chains_large_radii_nulls_and_a_count_below_one():
    lib = L.load()
    big = 1 << 40
    r17, n17 = _radii(*([1] * 17))
    assert lib.es_mask_morph(FAKE, FAKE, 1, 8, 8, r17, n17, FAKE, big, None) == -1 and b"n must be" in _err(lib)
    for bad in (16, -16, 100):
        r, n = _radii(3, bad)
        assert lib.es_mask_morph(FAKE, FAKE, 1, 8, 8, r, n, FAKE, big, None) == -1 and b"radius" in _err(lib)
    r, n = _radii(3, -3)
    assert lib.es_mask_morph(None, FAKE, 1, 8, 8, r, n, FAKE, big, None) == -1 and b"null" in _err(lib)
    assert lib.es_mask_morph(FAKE, None, 1, 8, 8, r, n, FAKE, big, None) == -1 and b"null" in _err(lib)
    assert lib.es_mask_morph(FAKE, FAKE, 1, 8, 8, None, 2, FAKE, big, None) == -1 and b"radii" in _err(lib)
    assert lib.es_mask_morph(FAKE, FAKE, 0, 8, 8, r, n, FAKE, big, None) == -1 and b"count" in _err(lib)
    assert lib.es_mask_morph(FAKE, FAKE, 1, 8, 8, r, -1, FAKE, big, None) == -1 and b"n must be" in _err(lib)


def test_a_workspace_that_is_too_small_missing_or_misaligned_is_refused():
    lib = L.load()
    H, W, n = 130, 67, 3
    need = lib.es_mask_workspace_bytes(H, W, n)
    r, nr = _radii(3, -3)
    # es_sam_compose needs exactly what es_mask_workspace_bytes reports; the other two calls need no more than that
    assert lib.es_sam_compose(None, FAKE, FAKE, FAKE, FAKE, n, H, W, FAKE, None, FAKE, need - 1, None) == -1
    assert b"workspace too small" in _err(lib) and str(need).encode() in _err(lib)
    packed = n * H * ((W + 63) // 64) * 8
    assert lib.es_mask_morph(FAKE, FAKE, n, H, W, r, nr, FAKE, 2 * packed - 1, None) == -1 and b"workspace too small" in _err(lib)
    assert lib.es_mask_largest_component(FAKE, FAKE, None, n, H, W, FAKE, 2 * packed + 8 * n * H * W, None) == -1
    assert b"workspace too small" in _err(lib)
    assert 2 * packed + 8 * n * H * W + 8 * n <= need
    assert lib.es_mask_morph(FAKE, FAKE, n, H, W, r, nr, None, need, None) == -1 and b"workspace" in _err(lib)
    assert lib.es_mask_morph(FAKE, FAKE, n, H, W, r, nr, C.c_void_p((1 << 20) + 4), need, None) == -1 and b"aligned" in _err(lib)


def test_logic_fill_and_compose_refuse_bad_arguments():
    lib = L.load()
    for op in (-1, 3, 7):
        assert lib.es_mask_logic(FAKE, FAKE, FAKE, 64, op, None) == -1 and b"op" in _err(lib)
    assert lib.es_mask_logic(FAKE, FAKE, FAKE, 0, L.MASK_AND, None) == -1 and b"n < 1" in _err(lib)
    assert lib.es_mask_logic(None, FAKE, FAKE, 64, L.MASK_AND, None) == -1 and b"null" in _err(lib)
    col = (C.c_uint8 * 3)(1, 2, 3)
    assert lib.es_image_mask_fill_u8(None, FAKE, FAKE, 1, 8, 8, None, None) == -1 and b"null" in _err(lib)
    assert lib.es_image_mask_fill_u8(None, None, FAKE, 1, 8, 8, col, None) == -1 and b"null" in _err(lib)
    img = (L.ImageU8 * 1)()
    img[0].data, img[0].height, img[0].width, img[0].channels, img[0].row_stride = FAKE.value, 8, 9, 3, 27
    assert lib.es_image_mask_fill_u8(img, FAKE, FAKE, 1, 8, 8, col, None) == -1 and b"must equal H and W" in _err(lib)
    img[0].width, img[0].channels = 8, 2
    assert lib.es_image_mask_fill_u8(img, FAKE, FAKE, 1, 8, 8, col, None) == -1 and b"channels" in _err(lib)
    img[0].channels, img[0].row_stride = 4, 31
    assert lib.es_image_mask_fill_u8(img, FAKE, FAKE, 1, 8, 8, col, None) == -1 and b"row_stride" in _err(lib)
    big = 1 << 40
    assert lib.es_sam_compose(img, FAKE, FAKE, FAKE, FAKE, 1, 8, 8, FAKE, FAKE, FAKE, big, None) == -1 and b"row_stride" in _err(lib)
    assert lib.es_sam_compose(img, FAKE, FAKE, FAKE, FAKE, 1, 8, 8, None, None, FAKE, big, None) == -1 and b"both outputs" in _err(lib)
    assert lib.es_sam_compose(None, FAKE, FAKE, FAKE, FAKE, 1, 8, 8, FAKE, FAKE, FAKE, big, None) == -1 and b"imgs" in _err(lib)
    assert lib.es_sam_compose(img, FAKE, None, FAKE, FAKE, 1, 8, 8, FAKE, None, FAKE, big, None) == -1 and b"null" in _err(lib)


def test_no_mask_call_runs_while_a_plan_records():
    lib = L.load()
    plan = C.c_void_p(lib.es_plan_create())
    assert lib.es_plan_begin_record(plan) == 0
    try:
        big = 1 << 40
        r, n = _radii(3, -3)
        col = (C.c_uint8 * 3)(127, 127, 127)
        assert lib.es_mask_morph(FAKE, FAKE, 1, 8, 8, r, n, FAKE, big, None) == -1 and b"recording" in _err(lib)
        assert lib.es_mask_largest_component(FAKE, FAKE, None, 1, 8, 8, FAKE, big, None) == -1 and b"recording" in _err(lib)
        assert lib.es_mask_logic(FAKE, FAKE, FAKE, 64, L.MASK_OR, None) == -1 and b"recording" in _err(lib)
        assert lib.es_image_mask_fill_u8(None, FAKE, FAKE, 1, 8, 8, col, None) == -1 and b"recording" in _err(lib)
        assert lib.es_sam_compose(None, FAKE, FAKE, FAKE, FAKE, 1, 8, 8, FAKE, None, FAKE, big, None) == -1 and b"recording" in _err(lib)
    finally:
        assert lib.es_plan_end_record(plan) == 0
        lib.es_plan_destroy(plan)
    r, n = _radii(16)                                  # not recording any more: the ordinary checks answer again
    assert lib.es_mask_morph(FAKE, FAKE, 1, 8, 8, r, n, FAKE, 1 << 40, None) == -1 and b"radius" in _err(lib)


# ---- the reference itself
@pytest.mark.parametrize("H,W", SIZES)
def test_reference_morphology_and_labels_equal_scipy(H, W):
    ndi = pytest.importorskip("scipy.ndimage")
    for seed in range(3):
        x = R.blobs(H, W, 100 * seed + H + W)
        for r in (1, 3, 6, 15):
            k = np.ones((2 * r + 1, 2 * r + 1), dtype=bool)
            assert np.array_equal(R.dilate(x, r), ndi.binary_dilation(x, structure=k, border_value=0))
            assert np.array_equal(R.erode(x, r), ndi.binary_erosion(x, structure=k, border_value=1))
        for k in (3, 7):                                   # skimage's closing in its older `reflect` grey form
            sq = np.ones((k, k), dtype=np.uint8)
            grey = ndi.grey_erosion(ndi.grey_dilation(x.astype(np.uint8), footprint=sq, mode="reflect"), footprint=sq, mode="reflect")
            assert np.array_equal(R.closing_square(x, k), grey > 0)
        for conn, st in ((8, np.ones((3, 3), dtype=int)), (4, None)):
            want, count = ndi.label(x, structure=st)
            got = R.label(x, conn)
            assert got.max() == count and np.array_equal(got, want)        # scipy, too, numbers in raster order
        mask, area = R.largest_component(x)
        want, count = ndi.label(x, structure=np.ones((3, 3), dtype=int))
        sizes = np.bincount(want.ravel())[1:]
        if count:
            assert area == sizes.max() and np.array_equal(mask, want == 1 + int(np.argmax(sizes)))     # argmax: the first of equals
        else:
            assert area == 0 and mask.all()


@pytest.mark.parametrize("H,W", SIZES)
def test_merged_radii_equal_the_iterations_the_reference_writes(H, W):
    """What the library runs ({+3, -3, -3, +3} for smooth_mask, one step of radius n(k-1)/2 for n iterations, adjacent radii of one
    sign added up) against the reference written out iteration by iteration - also where the image is narrower than the window."""
    for seed in range(3):
        x = R.blobs(H, W, 7 * seed + H * W)
        assert np.array_equal(R.cv2_dilate(x, 3, 3), R.dilate(x, 3)) and np.array_equal(R.cv2_erode(x, 3, 3), R.erode(x, 3))
        assert np.array_equal(R.cv2_dilate(x, 5, 3), R.dilate(x, 6)) and np.array_equal(R.cv2_erode(x, 5, 3), R.erode(x, 6))
        assert np.array_equal(R.smooth_mask(x), R.morph_chain(x, [3, -3, -3, 3]))
        assert np.array_equal(R.smooth_mask(x), R.morph_chain(x, [3, -6, 3]))
        assert np.array_equal(R.smooth_mask(x, 5, 2), R.morph_chain(x, [4, -4, -4, 4]))
        assert np.array_equal(R.smooth_mask(R.closing_square(x, 3)), R.morph_chain(x, [1, -1, 3, -3, -3, 3]))
        assert np.array_equal(R.smooth_mask(R.closing_square(x, 7)), R.morph_chain(x, [3, -3, 3, -3, -3, 3]))
        assert np.array_equal(R.morph_chain(x, [0, 2, 0]), R.dilate(x, 2))


def test_reference_label_order_ties_and_the_empty_mask():
    x = np.zeros((6, 9), dtype=bool)
    x[0, 6:9] = True                     # first in raster order, area 3
    x[2:5, 0] = True                     # second, area 3
    x[5, 4:8] = True                     # third, area 4 ... joined diagonally to nothing
    lab = R.label(x)
    assert lab[0, 6] == 1 and lab[2, 0] == 2 and lab[5, 4] == 3
    mask, area = R.largest_component(x)
    assert area == 4 and np.array_equal(mask, lab == 3)
    x[5, 4] = False                      # three components of area 3: the first wins
    mask, area = R.largest_component(x)
    assert area == 3 and np.array_equal(mask, R.label(x) == 1) and mask[0, 6]
    d = np.zeros((4, 4), dtype=bool)
    d[0, 0] = d[1, 1] = d[2, 2] = True   # a diagonal: one component under 8-connectivity, three under 4
    assert R.label(d, 8).max() == 1 and R.label(d, 4).max() == 3
    mask, area = R.largest_component(np.zeros((3, 5), dtype=bool))
    assert area == 0 and mask.all()      # labeled_array == 0
    s = R.serpentine(9, 7)
    assert R.label(s, 4).max() == 1 and s.sum() == 5 * 7 + 4

"""Mask post-processing on the GPU (csrc/mask.hip) against the suite's numpy reference (tests/mask_ref.py, which
test_masks_cpu.py holds against scipy): bit-packed morphology, the largest 8-connected component, the boolean algebra,
draw_binary_mask, es_sam_compose against the reference's create_sam_images written out line by line, the inference.py recipe
from the primitives, graph capture, the hand-over to es_prepare_conds_u8 and the compiled C++ host (examples/mask_host.cpp).
Every comparison is an equality."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from edgestyle_amd import config as Cfg, lib as L, masks as M, ops
from tests import mask_ref as R
from tests.helpers import make_weights, quantize

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0xA5
GUARD = 4096

SMOOTH = [3, -3, -3, 3]
CHAINS = [[1, -1], [3, -3], SMOOTH, [1, -1] + SMOOTH, [3, -3] + SMOOTH, [15], [-15], [0], [],
          [1, -2, 3, 0, -4, 5, -6, 7, -8, 9, -10, 11, -12, 13, -14, 15]]
# 5 x 9: narrower than the 13-wide window; 130 x 67 and 67 x 130: the 64- and 128-pixel word edges, in rows and in columns
SHAPES = [(5, 9), (1, 1), (37, 53), (64, 64), (130, 67), (67, 130)]


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t: torch.Tensor) -> np.ndarray:
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _stack(H, W, seed, count=3):
    """count blob masks as uint8 whose true pixels are ANY nonzero byte (the library must read nonzero as true)"""
    x = np.stack([R.blobs(H, W, seed + 17 * i, fill=(0.35, 0.5, 0.65)[i % 3]) for i in range(count)])
    g = np.random.default_rng(seed)
    return x, (x * g.integers(1, 256, size=x.shape)).astype(np.uint8)


def _is_01(a: np.ndarray) -> bool:
    return a.dtype == np.uint8 and bool((a <= 1).all())


# ---------------------------------------------------------------------------------------------------------------
# morphology
@pytest.mark.parametrize("H,W", SHAPES)
def test_morph_chains_equal_the_reference(H, W):
    assert len(CHAINS[-1]) == 16
    x, u8 = _stack(H, W, 11 * H + W)
    src = _dev(u8)
    for chain in CHAINS:
        got = _np(ops.mask_morph(src, chain))
        assert got.shape == (3, H, W) and _is_01(got)
        for i in range(3):
            want = R.morph_chain(x[i], chain)
            assert np.array_equal(got[i].astype(bool), want), (chain, i, int((got[i].astype(bool) != want).sum()))
    assert np.array_equal(_np(src), u8)                    # the input is only read


def test_morph_at_512_equals_the_reference_written_step_by_step():
    """the create_sam_images chain of the head mask at the size the application runs, against closing(square(7)) and three 3 x 3
    iterations of each cv2 call"""
    x, u8 = _stack(512, 512, 5, count=1)
    got = _np(ops.mask_morph(_dev(u8), [3, -3] + SMOOTH))
    assert np.array_equal(got[0].astype(bool), R.smooth_mask(R.closing_square(x[0], 7)))


@pytest.mark.parametrize("H,W", [(5, 9), (130, 67)])
def test_morph_in_place_and_inside_guarded_buffers(H, W):
    x, u8 = _stack(H, W, 3)
    n_out = u8.size
    packed = 3 * H * ((W + 63) // 64) * 8
    need = 2 * packed                                      # two packed copies: what es_mask_morph asks for
    assert need <= ops.mask_workspace_bytes(H, W, 3)
    obuf = torch.full((GUARD + n_out + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    wbuf = torch.full((GUARD + need + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    io = obuf[GUARD:GUARD + n_out].view(3, H, W)
    io.copy_(_dev(u8))
    out = ops.mask_morph(io, [1, -1] + SMOOTH, out=io, workspace=wbuf[GUARD:GUARD + need])
    assert out.data_ptr() == io.data_ptr()
    got = _np(io)
    for i in range(3):
        assert np.array_equal(got[i].astype(bool), R.morph_chain(x[i], [1, -1] + SMOOTH))
    for buf, n in ((obuf, n_out), (wbuf, need)):
        assert bool((buf[:GUARD] == POISON).all()) and bool((buf[GUARD + n:] == POISON).all())
    with pytest.raises(L.EdgeStyleHipError, match="workspace too small"):
        ops.mask_morph(io, SMOOTH, out=io, workspace=wbuf[GUARD:GUARD + need - 1])


# ---------------------------------------------------------------------------------------------------------------
# largest component
def _largest_cases(H=130, W=67):
    z = lambda: np.zeros((H, W), dtype=bool)                # noqa: E731
    cases = {}
    d = z()
    d[10:20, 5:15] = True
    d[20:40, 15:40] = True                                  # touches the first square at one corner only: (19,14) - (20,15)
    d[100:110, 50:60] = True
    cases["joined diagonally"] = d
    cases["serpentine"] = R.serpentine(H, W)
    cases["checkerboard"] = np.indices((H, W)).sum(0) % 2 == 0
    t = z()
    t[3:9, 60:66] = True                                    # area 36, first in raster order, inside the second word
    t[50:56, 2:8] = True                                    # area 36
    t[100:105, 30:37] = True                                # area 35
    cases["tie, the right one first"] = t
    cases["tie, the left one first"] = t[:, ::-1].copy()
    cases["all false"] = z()
    cases["all true"] = ~z()
    w = z()
    w[64, :] = True                                         # crosses both word edges of the row
    w[:, 63:65] |= np.arange(H)[:, None] % 3 != 0           # dashes on both sides of the first word edge
    w[5, 0:10] = True
    cases["across the word edges"] = w
    cases["blobs"] = R.blobs(H, W, 77)
    cases["sparse noise"] = np.random.default_rng(2).random((H, W)) < 0.3
    cases["dense noise"] = np.random.default_rng(3).random((H, W)) < 0.6
    return cases


@functools.lru_cache(maxsize=None)
def _largest_reference():
    return {k: (v,) + R.largest_component(v) for k, v in _largest_cases().items()}


def test_largest_component_cases_equal_the_reference():
    ref = _largest_reference()
    names = list(ref)
    x = np.stack([ref[k][0] for k in names])
    area = torch.full((len(names),), -7, dtype=torch.int32, device=DEV)
    got = _np(ops.mask_largest_component(_dev(x.astype(np.uint8) * 255), area_out=area))
    areas = _np(area)
    assert _is_01(got)
    for i, k in enumerate(names):
        _, want, want_area = ref[k]
        assert np.array_equal(got[i].astype(bool), want), (k, int((got[i].astype(bool) != want).sum()))
        assert int(areas[i]) == want_area, k
    # what the cases are there for
    d = ref["joined diagonally"]
    assert d[2] == 100 + 500 and R.label(d[0], 4).max() == 3 and R.label(d[0], 8).max() == 2
    assert ref["serpentine"][2] == 65 * 67 + 65 and ref["checkerboard"][2] == 130 * 67 // 2
    assert ref["tie, the right one first"][1][3, 60] and not ref["tie, the right one first"][1][50, 2]
    assert ref["tie, the left one first"][1][3, 6] and not ref["tie, the left one first"][1][50, 64]
    assert ref["all false"][1].all() and ref["all false"][2] == 0 and ref["all true"][2] == 130 * 67


@pytest.mark.parametrize("H,W", [(5, 9), (1, 1), (37, 53), (64, 64), (67, 130)])
def test_largest_component_of_blobs_at_other_shapes_and_without_area_out(H, W):
    x, u8 = _stack(H, W, H + 3 * W)
    got = _np(ops.mask_largest_component(_dev(u8)))
    for i in range(3):
        assert np.array_equal(got[i].astype(bool), R.largest_component(x[i])[0]), i


def test_largest_component_runs_give_identical_bytes_in_place_and_inside_guards():
    ref = _largest_reference()
    names = list(ref)
    x = np.stack([ref[k][0] for k in names]).astype(np.uint8)
    n, H, W = x.shape
    need = n * 8 + 2 * n * H * ((W + 63) // 64) * 8 + 8 * n * H * W
    assert need <= ops.mask_workspace_bytes(H, W, n)
    obuf = torch.full((GUARD + x.size + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    wbuf = torch.full((GUARD + need + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    io = obuf[GUARD:GUARD + x.size].view(n, H, W)
    runs = []
    for _ in range(2):
        io.copy_(_dev(x))
        ops.mask_largest_component(io, out=io, workspace=wbuf[GUARD:GUARD + need])
        runs.append(_np(io).copy())
    assert np.array_equal(runs[0], runs[1])
    for i, k in enumerate(names):
        assert np.array_equal(runs[0][i].astype(bool), ref[k][1]), k
    for buf, size in ((obuf, x.size), (wbuf, need)):
        assert bool((buf[:GUARD] == POISON).all()) and bool((buf[GUARD + size:] == POISON).all())
    with pytest.raises(L.EdgeStyleHipError, match="workspace too small"):
        ops.mask_largest_component(io, out=io, workspace=wbuf[GUARD:GUARD + need - 1])


# ---------------------------------------------------------------------------------------------------------------
# boolean algebra and draw_binary_mask
def test_logic_equals_numpy_and_may_write_over_an_operand():
    g = np.random.default_rng(9)
    a = (g.random((2, 37, 53)) < 0.5) * g.integers(1, 256, size=(2, 37, 53))
    b = (g.random((2, 37, 53)) < 0.5) * g.integers(1, 256, size=(2, 37, 53))
    a, b = a.astype(np.uint8), b.astype(np.uint8)
    ab, bb = a != 0, b != 0
    for op, want in ((L.MASK_AND, ab & bb), (L.MASK_OR, ab | bb), (L.MASK_ANDNOT, ab & ~bb)):
        got = _np(ops.mask_logic(_dev(a), _dev(b), op))
        assert _is_01(got) and np.array_equal(got.astype(bool), want)
        ta, tb = _dev(a), _dev(b)
        assert np.array_equal(_np(ops.mask_logic(ta, tb, op, out=ta)).astype(bool), want)
        ta = _dev(a)
        assert np.array_equal(_np(ops.mask_logic(ta, tb, op, out=tb)).astype(bool), want)
    big = g.integers(0, 2, size=(1, 4100, 4099), dtype=np.uint8)         # more bytes than one pass of the grid covers
    assert np.array_equal(_np(ops.mask_logic(_dev(big), _dev(big[:, ::-1].copy()), L.MASK_ANDNOT)), big & (1 - big[:, ::-1]))


def _photo(H, W, seed, channels=3, pad=0):
    """-> (the RGB pixels as numpy, a device tensor that holds them: 3 or 4 channels, rows pitched by `pad` poisoned pixels)"""
    g = np.random.default_rng(seed)
    rgb = g.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    buf = torch.full((H, W + pad, channels), POISON, dtype=torch.uint8, device=DEV)
    buf[:, :W, :3] = _dev(rgb)
    if channels == 4:
        buf[:, :W, 3] = _dev(g.integers(0, 256, size=(H, W), dtype=np.uint8))
    return rgb, buf[:, :W]


def test_mask_fill_equals_draw_binary_mask():
    H, W = 37, 53
    x, u8 = _stack(H, W, 21)
    photos = [_photo(H, W, 1), _photo(H, W, 2, channels=4, pad=5), _photo(H, W, 3, channels=3, pad=2)]
    got = _np(ops.image_mask_fill_u8([p[1] for p in photos], _dev(u8), (1, 127, 254)))
    zero = _np(ops.image_mask_fill_u8(None, _dev(u8), (255, 255, 255)))
    for i in range(3):
        assert np.array_equal(got[i], R.draw_binary_mask(photos[i][0], x[i], (1, 127, 254)))
        assert np.array_equal(zero[i], R.draw_binary_mask(np.zeros((H, W, 3), dtype=np.uint8), x[i], (255, 255, 255)))
    one = M.draw_binary_mask(photos[0][0], x[0], (9, 8, 7))              # numpy in, the reference's keyword
    assert one.is_cuda and np.array_equal(_np(one), R.draw_binary_mask(photos[0][0], x[0], (9, 8, 7)))


# ---------------------------------------------------------------------------------------------------------------
# create_sam_images
def _sam_inputs(H, W, count, seed):
    """four predictions per image as a segmenter hands them out: blobs that overlap, an own body / clothes overlap (the
    reference's `unknown`), a small head, stray pixels"""
    out = []
    for i in range(count):
        s = 1000 * seed + 10 * i
        subject = R.blobs(H, W, s, 0.5)
        body = R.blobs(H, W, s + 1, 0.4)
        clothes = R.blobs(H, W, s + 2, 0.4) | (body & R.blobs(H, W, s + 3, 0.3))
        head = R.blobs(H, W, s + 4, 0.15)
        out.append((subject, body, clothes, head))
    return out


@functools.lru_cache(maxsize=None)
def _sam_reference(H, W, count, seed):
    preds = _sam_inputs(H, W, count, seed)
    photos = [np.random.default_rng(seed + 50 + i).integers(0, 256, size=(H, W, 3), dtype=np.uint8) for i in range(count)]
    ref = [R.create_sam_images(p, *m) for p, m in zip(photos, preds)]
    images = np.stack([np.stack(r[0]) for r in ref])                     # [count, 5, H, W, 3]
    masks = np.stack([np.stack(r[1]) for r in ref])                      # [count, 4, H, W]
    return preds, photos, images, masks


def _sam_device(preds, photos, layout="rgb"):
    dev_masks = [_dev(np.stack([p[k] for p in preds]).astype(np.uint8) * (k + 1)) for k in range(4)]
    dev_photos = []
    for i, p in enumerate(photos):
        ch, pad = {"rgb": (3, 0), "rgba pitched": (4, 3 + i), "rgb pitched": (3, 5)}[layout]
        buf = torch.full((p.shape[0], p.shape[1] + pad, ch), POISON, dtype=torch.uint8, device=DEV)
        buf[:, :p.shape[1], :3] = _dev(p)
        dev_photos.append(buf[:, :p.shape[1]])
    return dev_photos, dev_masks


@pytest.mark.parametrize("H,W,count", [(130, 67, 1), (130, 67, 3), (512, 512, 1), (512, 512, 3), (67, 130, 2), (5, 9, 2)])
def test_sam_compose_equals_the_reference_recipe(H, W, count):
    preds, photos, want_images, want_masks = _sam_reference(H, W, count, 7)
    if H >= 64:                                            # the inputs exercise every mask: none is empty, none is full
        assert all(want_masks[:, k].any() and not want_masks[:, k].all() for k in range(4))
    dev_photos, dev_masks = _sam_device(preds, photos)
    masks, images = ops.sam_compose(dev_photos, *dev_masks)
    got_m, got_i = _np(masks), _np(images)
    assert _is_01(got_m) and np.array_equal(got_m.astype(bool), want_masks), int((got_m.astype(bool) != want_masks).sum())
    assert np.array_equal(got_i, want_images), int((got_i != want_images).sum())
    # each output alone
    only_m, none_i = ops.sam_compose(None, *dev_masks, want_images=False)
    none_m, only_i = ops.sam_compose(dev_photos, *dev_masks, want_masks=False)
    assert none_i is None and none_m is None
    assert np.array_equal(_np(only_m), got_m) and np.array_equal(_np(only_i), got_i)


@pytest.mark.parametrize("layout", ["rgba pitched", "rgb pitched"])
def test_sam_compose_reads_four_channels_and_pitched_rows_and_stays_inside_its_buffers(layout):
    H, W, count = 130, 67, 3
    preds, photos, want_images, want_masks = _sam_reference(H, W, count, 7)
    dev_photos, dev_masks = _sam_device(preds, photos, layout)
    need = ops.mask_workspace_bytes(H, W, count)
    n_m, n_i = count * 4 * H * W, count * 5 * H * W * 3
    bufs = [torch.full((GUARD + n + GUARD,), POISON, dtype=torch.uint8, device=DEV) for n in (n_m, n_i, need)]
    masks = bufs[0][GUARD:GUARD + n_m].view(count, 4, H, W)
    images = bufs[1][GUARD:GUARD + n_i].view(count, 5, H, W, 3)
    ops.sam_compose(dev_photos, *dev_masks, masks_out=masks, images_out=images, workspace=bufs[2][GUARD:GUARD + need])
    assert np.array_equal(_np(masks).astype(bool), want_masks) and np.array_equal(_np(images), want_images)
    for buf, n in zip(bufs, (n_m, n_i, need)):
        assert bool((buf[:GUARD] == POISON).all()) and bool((buf[GUARD + n:] == POISON).all())
    with pytest.raises(L.EdgeStyleHipError, match="workspace too small"):
        ops.sam_compose(dev_photos, *dev_masks, masks_out=masks, images_out=images, workspace=bufs[2][GUARD:GUARD + need - 1])


def test_masks_module_takes_numpy_torch_and_pil_under_the_references_names():
    H, W = 130, 67
    preds, photos, want_images, want_masks = _sam_reference(H, W, 1, 7)
    subject, body, clothes, head = preds[0]
    photo = photos[0]
    try:
        from PIL import Image
        photo_in = Image.fromarray(photo)
    except ImportError:
        photo_in = photo
    images, masks = M.create_sam_images(photo_in, subject, torch.from_numpy(body), _dev(clothes.astype(np.uint8) * 200), head,
                                        return_masks=True)
    assert len(images) == 5 and len(masks) == 4
    for k in range(5):
        assert images[k].is_cuda and images[k].dtype == torch.uint8 and images[k].is_contiguous()
        assert np.array_equal(_np(images[k]), want_images[0, k]), k
    for k in range(4):
        assert np.array_equal(_np(masks[k]).astype(bool), want_masks[0, k]), k
    assert len(M.create_sam_images(photo, subject, body, clothes, head)) == 5
    # the primitives, one mask and a batch
    assert np.array_equal(_np(M.closing_square(head, 7)).astype(bool), R.closing_square(head, 7))
    assert np.array_equal(_np(M.smooth_mask(body)).astype(bool), R.smooth_mask(body))
    assert np.array_equal(_np(M.smooth_mask(body, kernel_size=5, iterations=2)).astype(bool), R.smooth_mask(body, 5, 2))
    both = M.smooth_mask(np.stack([body, clothes]), 3, 3)
    assert both.shape == (2, H, W) and np.array_equal(_np(both[1]).astype(bool), R.smooth_mask(clothes))
    lc, area = M.largest_component(subject, return_area=True)
    want, want_area = R.largest_component(subject)
    assert np.array_equal(_np(lc).astype(bool), want) and int(area) == want_area
    for bad in (lambda: M.closing_square(head, 4), lambda: M.smooth_mask(head, 3, 16), lambda: M.smooth_mask(head, 2, 1)):
        with pytest.raises(L.EdgeStyleHipError):
            bad()


@pytest.mark.parametrize("H,W", [(130, 67), (37, 53)])
def test_subject_image_masks_equal_the_inference_recipe(H, W):
    subject, body, clothes, _ = _sam_inputs(H, W, 1, 13)[0]
    want = R.subject_image_masks(subject, body, clothes)
    got = M.subject_image_masks(subject, body, clothes)
    for k in range(3):
        assert got[k].shape == (H, W) and np.array_equal(_np(got[k]).astype(bool), want[k]), k
    photo = np.random.default_rng(4).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    images = M.subject_image(photo, subject, body, clothes)
    for k in range(3):
        assert np.array_equal(_np(images[k]), R.draw_binary_mask(photo, want[k], R.BG_COLOR)), k


def test_sam_compose_captures_into_a_graph_and_replays_to_the_same_bytes():
    H, W, count = 130, 67, 3
    preds, photos, want_images, want_masks = _sam_reference(H, W, count, 7)
    dev_photos, dev_masks = _sam_device(preds, photos)
    ws = torch.empty((ops.mask_workspace_bytes(H, W, count),), dtype=torch.uint8, device=DEV)
    masks = torch.zeros((count, 4, H, W), dtype=torch.uint8, device=DEV)
    images = torch.zeros((count, 5, H, W, 3), dtype=torch.uint8, device=DEV)
    area = torch.zeros((count,), dtype=torch.int32, device=DEV)
    lc = torch.zeros((count, H, W), dtype=torch.uint8, device=DEV)

    def chain():
        ops.sam_compose(dev_photos, *dev_masks, masks_out=masks, images_out=images, workspace=ws)
        ops.mask_largest_component(dev_masks[0], out=lc, area_out=area, workspace=ws)
    chain()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    # other inputs through the same buffers, then the first ones again
    other = _sam_reference(H, W, count, 8)
    for (p, ph, wi, wm) in (other, (preds, photos, want_images, want_masks)):
        src_photos, src_masks = _sam_device(p, ph)
        for d, s in zip(dev_photos + dev_masks, src_photos + src_masks):
            d.copy_(s)
        for t in (masks, images, lc, area):
            t.zero_()
        ws.fill_(POISON)
        graph.replay()
        assert np.array_equal(_np(masks).astype(bool), wm) and np.array_equal(_np(images), wi)
        for i in range(count):
            want, want_area = R.largest_component(p[i][0])
            assert np.array_equal(_np(lc[i]).astype(bool), want) and int(_np(area)[i]) == want_area


# ---------------------------------------------------------------------------------------------------------------
# hand-over: the images are what es_prepare_conds_u8 takes
T_STEPS = 2


@pytest.fixture(scope="module")
def built():
    from edgestyle_amd.models import StepRunner, AutoencoderKL
    from edgestyle_amd.pipeline import EdgeStyleStableDiffusionControlNetPipeline
    from edgestyle_amd.native import NativeEngine
    ucfg, vcfg = Cfg.tiny_unet(), Cfg.tiny_vae()
    ws = {k: quantize(v) for k, v in make_weights(ucfg, vcfg, seed=5).items()}
    runner = StepRunner.from_state_dicts(ws, ucfg, torch.float16, DEV)
    vae = AutoencoderKL(ws["vae"], vcfg).to(DEV)
    pipe = EdgeStyleStableDiffusionControlNetPipeline(vae=vae, unet=runner.unet, controlnet=runner.controlnet).to(DEV)
    for net in pipe.controlnet.nets:
        if getattr(net.config, "uses_vae", False):
            net.set_autoencoder(pipe.vae)
    eng = NativeEngine(pipe, batch_size=1, num_inference_steps=T_STEPS)
    s = ucfg.sample_size
    uses_vae = [bool(getattr(net.config, "uses_vae", False)) for net in pipe.controlnet.nets]
    g = torch.Generator().manual_seed(31)
    noise = [torch.randn(2, vcfg.latent_channels, s, s, generator=g).to(DEV) if v else None for v in uses_vae]
    yield pipe, eng, uses_vae, noise, s * vcfg.scale
    eng.close()


def test_composed_images_go_into_prepare_conds_u8_without_conversion(built):
    """the five images of one photo (and the photo itself as the sixth condition) go straight from es_sam_compose's output buffer
    into es_prepare_conds_u8, at a size that the resize changes; the slots equal those the reference's numpy images give"""
    pipe, eng, uses_vae, noise, res = built
    H, W = 130, 67
    preds, photos, want_images, _ = _sam_reference(H, W, 1, 7)
    images = M.create_sam_images(_dev(photos[0]), *preds[0])
    six = list(images) + [_dev(photos[0])]
    assert all(t.dtype == torch.uint8 and t.is_cuda and t.shape == (H, W, 3) for t in six)
    eng.prepare_conds_u8(six, uses_vae, noise)
    torch.cuda.synchronize()
    got = [t.clone() for t in eng.cond_img]
    for t in eng.cond_img:
        t.fill_(7.0)
    eng.prepare_conds_u8([_dev(want_images[0, k]) for k in range(5)] + [_dev(photos[0])], uses_vae, noise)
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(got, eng.cond_img)):
        assert torch.equal(a, b), k
    pre = pipe.preprocess_images(six)
    assert len(pre) == 6 and all(p.shape == (1, 3, res, res) and p.is_cuda for p in pre)
    assert all(torch.equal(p, slot) for p, slot in zip(pre, got))


# ---------------------------------------------------------------------------------------------------------------
# the C++ host
def _write_pnm(path, a: np.ndarray):
    kind, shape = (b"P6", a.shape[:2]) if a.ndim == 3 else (b"P5", a.shape)
    with open(path, "wb") as f:
        f.write(kind + b"\n# mask_host input\n%d %d\n255\n" % (shape[1], shape[0]) + a.tobytes())


def test_cpp_mask_host_writes_the_bytes_of_the_ctypes_path(tmp_path):
    """examples/mask_host.cpp: one PPM photo and four PGM masks in -> es_sam_compose -> five PPMs, no Python in the process"""
    H, W = 130, 67
    preds, photos, want_images, _ = _sam_reference(H, W, 1, 7)
    dev_photos, dev_masks = _sam_device(preds, photos)
    ctypes_path = _np(ops.sam_compose(dev_photos, *dev_masks, want_masks=False)[1])[0]
    assert np.array_equal(ctypes_path, want_images[0])
    _write_pnm(str(tmp_path / "photo.ppm"), photos[0])
    names = ("subject", "body", "clothes", "head")
    for k, name in enumerate(names):
        _write_pnm(str(tmp_path / f"{name}.pgm"), preds[0][k].astype(np.uint8) * (255 if k % 2 else 1))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, libdir = str(tmp_path / "mask_host"), os.path.join(root, "edgestyle_amd", "lib")
    c = subprocess.run([hipcc, "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "mask_host.cpp"),
                        "-L" + libdir, "-ledgestyle_hip", "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-2000:]
    r = subprocess.run([exe, str(tmp_path / "photo.ppm")] + [str(tmp_path / f"{n}.pgm") for n in names] + [str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    head = b"P6\n%d %d\n255\n" % (W, H)
    for k, name in enumerate(("subject", "mask", "agnostic", "clothes", "head")):
        raw = open(str(tmp_path / f"out_{name}.ppm"), "rb").read()
        assert raw.startswith(head) and len(raw) == len(head) + H * W * 3, name
        assert np.array_equal(np.frombuffer(raw[len(head):], dtype=np.uint8).reshape(H, W, 3), ctypes_path[k]), name

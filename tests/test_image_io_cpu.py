"""Byte images at the C ABI, the part that needs no GPU: torchvision's size and crop rules (es_image_fit), the resampling
coefficients (es_image_resize_coeffs - the host build of the one function the kernels run) against Pillow byte for byte, the
argument checks of every new entry point, and the service's handling of requests that carry decoded photos."""
import ctypes as C

import numpy as np
import pytest
import torch

from edgestyle_amd import lib as L
from tests import image_io_ref as R


def test_es_image_fit_known_answers():
    assert R.fit(1333, 2000, 512) == (512, 768, 0, 128)
    assert R.fit(513, 700, 512) == (512, 698, 0, 93)
    assert R.fit(2000, 1333, 512) == (768, 512, 128, 0)
    # crop offsets that are ties round half to even, as Python's round does: (rh - R) = 3 -> 2, 5 -> 2
    assert R.fit(67, 64, 64) == (67, 64, 2, 0)
    assert R.fit(69, 64, 64) == (69, 64, 2, 0)
    assert R.fit(64, 67, 64) == (64, 67, 0, 2) and R.fit(64, 65, 64)[3] == 0 and R.fit(64, 71, 64)[3] == 4
    assert R.fit(64, 64, 64) == (64, 64, 0, 0)


def test_fixture_is_the_documented_one():
    cases, version = R.fixture()
    assert version and [(a.shape[0], a.shape[1], r) for a, _, r in cases] == R.CASES
    for a, ref, r in cases:
        rh, rw, _, _ = R.fit(a.shape[0], a.shape[1], r)
        assert a.dtype == np.uint8 and ref.dtype == np.uint8 and ref.shape == (rh, rw, 3)
    assert max(nt.max() for nt in [R.coeffs(197, 24)[1]]) >= 17          # the > 8x downscale case runs 17+ taps


@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_integer_resize_from_the_library_coefficients_equals_the_fixture(case):
    a, ref, r = R.fixture()[0][case]
    rh, rw, _, _ = R.fit(a.shape[0], a.shape[1], r)
    got = R.integer_resize(a, rh, rw)
    assert got.shape == ref.shape and np.array_equal(got, ref), int((got != ref).sum())


@pytest.mark.skipif(not R.have_pillow(), reason="Pillow is not installed: the fixture tests cover the same code")
@pytest.mark.parametrize("h,w,r", [(511, 1023, 64), (97, 33, 50), (33, 97, 50), (5, 3, 7), (1, 9, 4), (203, 301, 96)])
def test_integer_resize_equals_live_pillow(h, w, r):
    a = np.random.default_rng(h * 7919 + w).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    rh, rw, _, _ = R.fit(h, w, r)
    got, ref = R.integer_resize(a, rh, rw), R.pillow_resize(a, rh, rw)
    assert np.array_equal(got, ref), int((got != ref).sum())


def test_coefficients_sum_to_one_and_stay_inside_the_axis():
    for n_in, n_out in [(53, 91), (197, 24), (100, 32), (128, 64), (7, 7)]:
        xmin, nt, k = R.coeffs(n_in, n_out)
        assert xmin.min() >= 0 and (xmin + nt).max() <= n_in and nt.min() >= 1
        for i in range(n_out):
            assert abs(int(k[i, :nt[i]].sum()) - (1 << 22)) <= nt[i] and k[i, :nt[i]].min() >= 0
    lib = L.load()
    buf = (C.c_int32 * 24)()
    assert lib.es_image_resize_coeffs(197, 24, None, None, buf, 1) == -1 and b"cap" in lib.es_last_error()
    assert lib.es_image_resize_coeffs(0, 24, None, None, None, 0) == -1


# ---------------------------------------------------------------------------------------------------------------
# argument checks: -1 with a text that names the problem, before any launch (so: without a GPU)
FAKE = 0x10000          # a non-null address that is never dereferenced: every call below is refused before it launches


def _img(h=20, w=30, ch=3, stride=None, data=FAKE):
    return L.ImageU8(data=data, height=h, width=w, channels=ch, row_stride=w * ch if stride is None else stride)


def _resize(imgs, count=None, out=FAKE, r=16, ws=FAKE, ws_bytes=1 << 20):
    arr = (L.ImageU8 * max(len(imgs), 1))(*imgs)
    lib = L.load()
    rc = lib.es_image_resize_u8(arr if imgs else None, len(imgs) if count is None else count, C.c_void_p(out), r, C.c_void_p(ws),
                                ws_bytes, None)
    return rc, lib.es_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(imgs=[]), "null pointer"),
    (dict(imgs=[_img()], out=None), "null pointer"),
    (dict(imgs=[_img(data=None)]), "null pointer"),
    (dict(imgs=[_img()], ws=None), "null pointer"),
    (dict(imgs=[_img()], count=0), "count < 1"),
    (dict(imgs=[_img(ch=2)]), "channels"),
    (dict(imgs=[_img(ch=5)]), "channels"),
    (dict(imgs=[_img(w=30, ch=4, stride=119)]), "row_stride"),
    (dict(imgs=[_img(h=0)]), "height or width < 1"),
    (dict(imgs=[_img(w=-3)]), "height or width < 1"),
    (dict(imgs=[_img()], r=0), "R < 1"),
    (dict(imgs=[_img()], ws_bytes=0), "workspace too small"),
    (dict(imgs=[_img(), _img(40, 25)], ws_bytes=100), "workspace too small"),
])
def test_es_image_resize_u8_refuses_malformed_arguments(kw, word):
    rc, msg = _resize(**kw)
    assert rc == -1 and word in msg and msg.startswith("es_image_resize_u8"), (rc, msg)


def test_workspace_size_is_the_intermediate_image_of_the_images_whose_width_changes():
    lib = L.load()
    arr = (L.ImageU8 * 3)(_img(64, 64), _img(64, 100), _img(100, 64))      # identity; crop only; vertical pass only
    assert lib.es_image_resize_workspace_bytes(arr, 3, 64) == 0
    arr = (L.ImageU8 * 1)(_img(20, 30))                                     # 20x30 -> 16x24: all 20 rows x 16 kept columns x 3
    assert lib.es_image_resize_workspace_bytes(arr, 1, 16) == 20 * 16 * 3
    assert lib.es_image_resize_workspace_bytes(None, 1, 16) == 0 and b"null pointer" in lib.es_last_error()


def test_conversions_and_context_calls_refuse_malformed_arguments():
    lib = L.load()
    P = C.c_void_p

    def err():
        return lib.es_last_error().decode()
    assert lib.es_image_u8_to_f32(None, P(FAKE), 1, 8, 8, 0, None) == -1 and "null pointer" in err()
    assert lib.es_image_u8_to_f32(P(FAKE), None, 1, 8, 8, 0, None) == -1 and "null pointer" in err()
    assert lib.es_image_u8_to_f32(P(FAKE), P(FAKE), 0, 8, 8, 0, None) == -1 and "count < 1" in err()
    assert lib.es_image_u8_to_f32(P(FAKE), P(FAKE), 1, 0, 8, 0, None) == -1 and "height or width < 1" in err()
    assert lib.es_image_f32_to_u8(None, P(FAKE), 1, 8, 8, None) == -1 and "null pointer" in err()
    assert lib.es_image_f32_to_u8(P(FAKE), None, 1, 8, 8, None) == -1 and "null pointer" in err()
    assert lib.es_image_f32_to_u8(P(FAKE), P(FAKE), 0, 8, 8, None) == -1 and "count < 1" in err()
    assert lib.es_image_f32_to_u8(P(FAKE), P(FAKE), 1, 8, -1, None) == -1 and "height or width < 1" in err()
    out = (C.c_int32 * 4)()
    assert lib.es_image_fit(0, 5, 8, out) == -1 and "height or width < 1" in err()
    assert lib.es_image_fit(5, 5, 0, out) == -1 and "R < 1" in err()
    assert lib.es_image_fit(5, 5, 8, None) == -1 and "null pointer" in err()
    arr = (L.ImageU8 * 6)(*[_img() for _ in range(6)])
    nrm = (C.c_int32 * 6)()
    assert lib.es_prepare_conds_u8(None, arr, nrm, None, P(FAKE), 1 << 20, None) == -1 and "null pointer" in err()
    assert lib.es_vae_decode_u8(None, P(FAKE), P(FAKE), None) == -1 and "null pointer" in err()
    ctx = C.c_void_p()
    assert lib.es_ctx_create(0, C.byref(ctx)) == 0
    try:
        assert lib.es_prepare_conds_u8(ctx, None, nrm, None, P(FAKE), 1 << 20, None) == -1 and "null pointer" in err()
        assert lib.es_prepare_conds_u8(ctx, arr, None, None, P(FAKE), 1 << 20, None) == -1 and "null pointer" in err()
        assert lib.es_vae_decode_u8(ctx, None, P(FAKE), None) == -1 and "null pointer" in err()
        assert lib.es_vae_decode_u8(ctx, P(FAKE), None, None) == -1 and "null pointer" in err()
        # an empty context has no plans: refused before anything is touched
        assert lib.es_prepare_conds_u8(ctx, arr, nrm, None, P(FAKE), 1 << 20, None) == -1 and "ES_PLAN_CONDS" in err()
    finally:
        lib.es_ctx_destroy(ctx)


def test_byte_image_calls_are_never_part_of_a_plan():
    lib = L.load()
    P = C.c_void_p
    plan = C.c_void_p(lib.es_plan_create())
    assert lib.es_plan_begin_record(plan) == 0
    try:
        was = lib.es_plan_set_dry(1)
        rc, msg = _resize([_img()])
        assert rc == -1 and "plan is recording" in msg
        assert lib.es_image_u8_to_f32(P(FAKE), P(FAKE), 1, 8, 8, 0, None) == -1 and b"plan is recording" in lib.es_last_error()
        assert lib.es_image_f32_to_u8(P(FAKE), P(FAKE), 1, 8, 8, None) == -1 and b"plan is recording" in lib.es_last_error()
        ctx = C.c_void_p()
        assert lib.es_ctx_create(0, C.byref(ctx)) == 0
        arr, nrm = (L.ImageU8 * 6)(*[_img() for _ in range(6)]), (C.c_int32 * 6)()
        assert lib.es_prepare_conds_u8(ctx, arr, nrm, None, P(FAKE), 1 << 20, None) == -1 and b"plan is recording" in lib.es_last_error()
        assert lib.es_vae_decode_u8(ctx, P(FAKE), P(FAKE), None) == -1 and b"plan is recording" in lib.es_last_error()
        lib.es_ctx_destroy(ctx)
        assert lib.es_plan_size(plan) == 0
    finally:
        lib.es_plan_set_dry(was)
        assert lib.es_plan_end_record(plan) == 0
        lib.es_plan_destroy(plan)


def test_abi_version_is_unchanged():
    assert L.load().es_abi_version() == 7 == L.ABI_VERSION


# ---------------------------------------------------------------------------------------------------------------
# the service: requests that carry decoded photos
class _FakeBytePipe:
    """Stand-in pipeline: `preprocess_images` is a stub (photo of any size -> [1,3,8,8] from its own pixels only), the call
    returns one value per request that depends on that request's inputs only."""

    def __init__(self):
        self.calls, self.preprocessed = [], 0

    def preprocess_images(self, images):
        assert len(images) == 6
        self.preprocessed += 1
        out = []
        for im in images:
            im = torch.as_tensor(np.asarray(im))
            assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3
            out.append((im.float().mean() / 255.0 + im.shape[0] * 1e-3).expand(1, 3, 8, 8).clone())
        return out

    def __call__(self, prompt_embeds, negative_prompt_embeds, image, latents, guidance_scale, num_inference_steps,
                 control_guidance_start, control_guidance_end, output_type):
        import types
        B = latents.shape[0]
        assert all(t.shape == (B, 3, 8, 8) and t.dtype == torch.float32 for t in image)
        self.calls.append((B, output_type))
        per = latents.mean(dim=(1, 2, 3)) + prompt_embeds.mean(dim=(1, 2)) + sum(im.mean(dim=(1, 2, 3)) * (k + 1) for k, im in enumerate(image))
        if output_type == "u8":
            return types.SimpleNamespace(images=(per.abs() * 40).clamp(0, 255).to(torch.uint8)[:, None, None, None].expand(B, 8, 8, 3).clone())
        return types.SimpleNamespace(images=per[:, None, None, None].expand(B, 3, 8, 8).clone())


def _byte_request(seed, hw):
    from edgestyle_amd.serve import TryOnRequest
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(500 + seed)
    photos = [torch.from_numpy(rng.integers(0, 256, size=(hw[0] + k, hw[1], 3), dtype=np.uint8)) for k in range(6)]
    photos[1] = photos[1].numpy()                                   # numpy arrays are photos too
    return TryOnRequest(photos, torch.randn(1, 77, 32, generator=g), torch.randn(1, 77, 32, generator=g), 7.5, 50, seed)


def test_service_batches_photos_of_different_sizes_and_batching_does_not_change_results():
    from edgestyle_amd.serve import TryOnService
    sizes = [(37, 53), (150, 100)]
    solo_pipe = _FakeBytePipe()
    solo = TryOnService(solo_pipe, max_batch=1, max_wait_s=0.0)
    want = [solo.submit(_byte_request(s, hw)).result(timeout=10) for s, hw in enumerate(sizes)]
    solo.shutdown()
    assert [c[0] for c in solo_pipe.calls] == [1, 1]

    pipe = _FakeBytePipe()
    svc = TryOnService(pipe, max_batch=2, max_wait_s=2.0, batch_sizes=(1, 2))
    reqs = [_byte_request(s, hw) for s, hw in enumerate(sizes)]
    futs = [svc.submit(r) for r in reqs]
    got = [f.result(timeout=10) for f in futs]
    svc.shutdown()
    assert pipe.calls == [(2, "pt")] and pipe.preprocessed == 2          # ONE pipeline call for the two sizes
    for a, b in zip(got, want):
        assert a.shape == (1, 3, 8, 8) and torch.equal(a, b)
    assert not torch.equal(got[0], got[1])
    assert all(torch.is_tensor(i) and i.shape == (1, 3, 8, 8) for r in reqs for i in r.images)


def test_service_output_u8_asks_the_pipeline_for_bytes_and_a_bad_photo_fails_alone():
    from edgestyle_amd.serve import TryOnService
    pipe = _FakeBytePipe()
    svc = TryOnService(pipe, max_batch=1, max_wait_s=0.0, output_u8=True)
    bad = _byte_request(3, (20, 20))
    bad.images[2] = torch.zeros(4, 4, 3)                                # float pixels: the stub (like the pipeline) refuses them
    fb, fg = svc.submit(bad), svc.submit(_byte_request(4, (20, 24)))
    img = fg.result(timeout=10)
    with pytest.raises(AssertionError):
        fb.result(timeout=10)
    svc.shutdown()
    assert img.dtype == torch.uint8 and img.shape == (1, 8, 8, 3) and pipe.calls == [(1, "u8")]

"""The CLIP prompt picker at the C ABI, the part that needs no GPU: the size and crop rule against the installed processor, the bicubic
taps against Pillow byte for byte, dry builds of the image tower, every refusal with its text, and the CPU restatement
(tests/clip_ref.py) the GPU tests measure against, pinned to transformers' own CLIPModel."""
import ctypes as C

import numpy as np
import pytest
import torch

from edgestyle_amd import lib as L
from edgestyle_amd.clip import vision_config
from edgestyle_amd.text import state_dict_descriptors
from tests import clip_ref as R
from tests import image_io_ref as IR

NEW_SYMBOLS = ("es_image_fit_ex", "es_image_resize_coeffs_ex", "es_image_resize_workspace_bytes_ex", "es_image_resize_u8_ex", "es_clip_patchify",
               "es_clip_embed", "es_clip_score", "es_clip_bank_create", "es_clip_bank_destroy", "es_clip_bank_rows", "es_clip_bank_data",
               "es_clip_bank_append", "es_clip_text_pool", "es_clip_vision_create", "es_clip_vision_destroy",
               "es_clip_vision_arena_bytes", "es_clip_vision_encode", "es_clip_pick_workspace_bytes", "es_clip_pick")
FAKE = 0x10000          # never dereferenced: every call it goes to is refused before a launch


def test_abi_version_is_unchanged_and_the_new_symbols_resolve():
    lib = L.load()
    assert lib.es_abi_version() == 7
    for name in NEW_SYMBOLS:
        assert name in L.SYMBOLS and getattr(lib, name)
    assert (L.FILTER_BILINEAR, L.FILTER_BICUBIC, L.CROP_TORCHVISION, L.CROP_TRANSFORMERS) == (0, 1, 0, 1)


SIZES = [(300, 200), (200, 300), (97, 131), (131, 97), (224, 224), (56, 120), (120, 56), (40, 30), (30, 40), (56, 56), (57, 56), (1024, 768), (333, 500),
         (61, 59), (225, 224), (227, 224), (2, 3), (1, 1), (500, 333)]


@pytest.mark.parametrize("rr", [56, 224, 57])
def test_fit_with_the_transformers_rule_is_the_installed_processors_geometry(rr):
    """resize: get_resize_output_image_size(shortest edge); crop: where transformers.image_transforms.center_crop starts, read off an index image"""
    from transformers.image_transforms import center_crop, get_resize_output_image_size
    odd_crop = 0
    for h, w in SIZES:
        rh, rw = get_resize_output_image_size(np.zeros((h, w, 3), np.uint8), size=rr, default_to_square=False, input_data_format="channels_last")
        idx = np.stack([np.repeat(np.arange(rh)[:, None], rw, 1), np.repeat(np.arange(rw)[None, :], rh, 0)], 0).astype(np.int32)     # [2, rh, rw]
        c = center_crop(idx, (rr, rr), input_data_format="channels_first")
        assert c.shape == (2, rr, rr)
        got = R.fit(h, w, rr, L.CROP_TRANSFORMERS)
        assert got == (rh, rw, int(c[0, 0, 0]), int(c[1, 0, 0])), (h, w, rr, got)
        tv = R.fit(h, w, rr, L.CROP_TORCHVISION)
        assert tv == IR.fit(h, w, rr) and tv[:2] == got[:2]
        odd_crop += tv != got
    assert odd_crop or rr == 57      # the two crop rules differ somewhere in the sweep (an odd margin of 3 or more)


@pytest.mark.parametrize("h,w,rh,rw", [(300, 200, 84, 56), (97, 131, 56, 75), (40, 30, 74, 56), (56, 120, 56, 120), (120, 56, 56, 56), (64, 64, 200, 13)])
def test_bicubic_taps_applied_on_the_host_equal_pillow(h, w, rh, rw):
    """downscale, upscale, one axis unchanged; the fixture has a hard black / white edge: negative weights occur and sums are clipped"""
    from PIL import Image
    a = R.photo(h, w, seed=h * 1000 + w)
    stats = {}
    got = R.integer_resize(a, rh, rw, L.FILTER_BICUBIC, stats)
    want = np.asarray(Image.fromarray(a).resize((rw, rh), Image.BICUBIC))
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    if (h, w) != (rh, rw):
        assert stats["negative_weights"] > 0 and stats["clipped"] > 0, stats
    assert got.min() == 0 and got.max() == 255


def test_the_bilinear_entry_points_keep_their_answers():
    """old calls, and the new ones asked for the old filter, against tests/image_io_ref.py (which calls the old ones) and live Pillow"""
    for n_in, n_out in [(300, 56), (40, 56), (97, 64), (56, 56)]:
        a, b = IR.coeffs(n_in, n_out), R.coeffs(L.FILTER_BILINEAR, n_in, n_out)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert (b[2] >= 0).all()
    a = R.photo(97, 131, seed=3)
    assert np.array_equal(IR.integer_resize(a, 56, 75), IR.pillow_resize(a, 56, 75))
    assert np.array_equal(R.integer_resize(a, 56, 75, L.FILTER_BILINEAR), IR.pillow_resize(a, 56, 75))
    assert IR.fit(300, 200, 56) == (84, 56, 14, 0) and IR.fit(61, 56, 56)[2] == 2 and R.fit(61, 56, 56, L.CROP_TRANSFORMERS)[2] == 2
    assert IR.fit(59, 56, 56)[2] == 2 and R.fit(59, 56, 56, L.CROP_TRANSFORMERS)[2] == 1          # 1.5: to even | dropped


def test_the_wider_filter_keeps_more_source_rows():
    lib = L.load()
    img = (L.ImageU8 * 1)()
    img[0].data, img[0].height, img[0].width, img[0].channels, img[0].row_stride = FAKE, 300, 200, 3, 600
    lin = lib.es_image_resize_workspace_bytes_ex(img, 1, 56, L.FILTER_BILINEAR, L.CROP_TRANSFORMERS)
    cub = lib.es_image_resize_workspace_bytes_ex(img, 1, 56, L.FILTER_BICUBIC, L.CROP_TRANSFORMERS)
    assert lin == lib.es_image_resize_workspace_bytes(img, 1, 56) > 0 and cub > lin
    # exactly the rows the taps of the kept output rows reach
    xmin, nt, _ = R.coeffs(L.FILTER_BICUBIC, 300, 84)
    top = R.fit(300, 200, 56, L.CROP_TRANSFORMERS)[2]
    rows = (xmin[top:top + 56] + nt[top:top + 56]).max() - xmin[top:top + 56].min()
    assert cub == rows * 56 * 3
    assert lib.es_image_resize_workspace_bytes_ex(img, 1, 56, 2, 0) == 0 and b"filter" in lib.es_last_error()
    assert lib.es_image_resize_u8_ex(img, 1, FAKE, 56, L.FILTER_BICUBIC, 5, FAKE, 1 << 20, None) == -1 and b"crop rule" in lib.es_last_error()


def test_the_host_preprocessing_of_the_reference_file_is_the_processors():
    """clip_ref.pil_bicubic + pixel_formula against CLIPImageProcessor itself: pins the geometry and the arithmetic the GPU tests compare with"""
    from PIL import Image
    from transformers import CLIPImageProcessor
    for rr, (h, w) in [(56, (300, 200)), (56, (97, 131)), (56, (40, 30)), (57, (90, 61))]:
        proc = CLIPImageProcessor(size={"shortest_edge": rr}, crop_size={"height": rr, "width": rr})
        a = R.photo(h, w, seed=h + w)
        want = proc(images=Image.fromarray(a), return_tensors="pt").pixel_values
        got = R.pixel_formula(torch.from_numpy(R.pil_bicubic(a, rr))[None])
        err = float((got - want).abs().max())
        print(f"processor vs restatement {h}x{w} -> {rr}: max abs {err:.3e}")
        assert got.shape == want.shape and err <= 1e-6


@pytest.fixture(scope="module")
def tiny():
    cfg = R.config()
    return cfg, R.make_model(cfg, seed=5, logit_scale=3.0)


def test_the_restatement_equals_transformers_in_fp32(tiny):
    """pins tests/clip_ref.py: plain functional ops in fp32 against CLIPModel's own forward (SURVEY 8c's bar for fp32 against fp32)"""
    from tests import text_ref as TR
    cfg, model = tiny
    ids = TR.token_ids(cfg.text_config, 5, seed=2)
    pv = R.pixel_formula(R.images_u8(cfg, 3, seed=1))
    sd = R.floats(model.state_dict())
    with torch.no_grad():
        want = model(input_ids=ids, pixel_values=pv)
    for mode in ("fp32", "fp64"):
        got = R.forward(sd, cfg, pixel_values=pv, tokens=ids, mode=mode)
        for a, b, name in ((got["image_unit"], want.image_embeds, "image_embeds"), (got["text_unit"], want.text_embeds, "text_embeds"),
                           (got["logits_per_image"], want.logits_per_image, "logits_per_image")):
            rel = float((a.double() - b.double()).abs().max() / b.abs().max())
            print(f"restatement vs transformers, {mode} {name}: {rel:.3e} (max abs / max abs)")
            assert a.shape == b.shape and rel <= 1e-5
    # the legacy rule: with eos_token_id == 2 the pooled position is the argmax of the ids
    assert R.eos_positions(torch.tensor([[5, 9, 2, 2], [7, 2, 8, 1]]), 2).tolist() == [1, 2]
    assert R.eos_positions(torch.tensor([[5, 9, 2, 2], [7, 2, 8, 1]]), 9).tolist() == [1, 0]
    from edgestyle_amd.clip import eos_positions
    assert eos_positions(torch.tensor([[5, 9, 2, 2], [7, 2, 8, 1]]), 2).tolist() == [1, 2]


def _create(sd, vcfg, proj=64, dtype=L.ES_F16, max_n=2, device=-1, **change):
    lib = L.load()
    d = dict(image_size=vcfg.image_size, patch_size=vcfg.patch_size, hidden_size=vcfg.hidden_size, num_attention_heads=vcfg.num_attention_heads,
             num_hidden_layers=vcfg.num_hidden_layers, intermediate_size=vcfg.intermediate_size, layer_norm_eps=vcfg.layer_norm_eps,
             hidden_act=vcfg.hidden_act)
    d.update(change)
    cfg = vision_config(d, proj)
    desc, keep = state_dict_descriptors(sd)
    h = C.c_void_p()
    rc = lib.es_clip_vision_create(C.byref(desc), C.byref(cfg), dtype, max_n, device, C.byref(h))
    del keep
    return rc, h, (lib.es_last_error() or b"").decode()


def test_dry_build_reports_its_arena_and_refuses_to_run(tiny):
    cfg, model = tiny
    lib = L.load()
    sd = R.floats(model.state_dict())
    rc, h, msg = _create(sd, cfg.vision_config)
    assert rc == 0 and h.value, msg
    try:
        a = lib.es_clip_vision_arena_bytes(h)
        # the fp32 position table and the padded patch weights alone
        assert a > 17 * 128 * 4 + 128 * 640 * 2
        assert lib.es_clip_vision_encode(h, FAKE, 1, FAKE, None) == -1 and b"dry build" in lib.es_last_error()
        assert lib.es_clip_vision_encode(h, FAKE, 3, FAKE, None) == -1 and b"outside 1..max_n = 2" in lib.es_last_error()
        img = (L.ImageU8 * 1)()
        img[0].data, img[0].height, img[0].width, img[0].channels, img[0].row_stride = FAKE, 30, 40, 3, 120
        assert lib.es_clip_pick_workspace_bytes(h, img, 1) >= 56 * 56 * 3 + 64 * 2
        assert lib.es_clip_pick_workspace_bytes(h, img, 3) == 0 and b"max_n" in lib.es_last_error()
    finally:
        lib.es_clip_vision_destroy(h)
    # the keys of a bare CLIPVisionModel (no vision_model. prefix) build the same arena; more images need more activations
    bare = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in sd.items() if not k.startswith("text_model.")}
    rc, h2, msg = _create(bare, cfg.vision_config)
    assert rc == 0, msg
    rc, h3, msg = _create(sd, cfg.vision_config, max_n=5)
    assert rc == 0, msg
    try:
        assert lib.es_clip_vision_arena_bytes(h2) == a and lib.es_clip_vision_arena_bytes(h3) > a
    finally:
        lib.es_clip_vision_destroy(h2)
        lib.es_clip_vision_destroy(h3)


@pytest.mark.parametrize("change,text", [
    (dict(hidden_size=96, num_attention_heads=3), "hidden must be a multiple of 64"),
    (dict(hidden_size=4160, num_attention_heads=65), "hidden above 4096"),
    (dict(num_attention_heads=8), "hidden / heads must be 32 or 64"),
    (dict(image_size=60), "image_size must be a multiple of patch_size"),
    (dict(image_size=462), "more than 1025 tokens"),
    (dict(intermediate_size=200), "intermediate must be a multiple of 64"),
])
def test_refused_configurations(tiny, change, text):
    cfg, model = tiny
    rc, h, msg = _create(R.floats(model.state_dict()), cfg.vision_config, **change)
    assert rc == -1 and not h.value and text in msg, msg


def test_other_activations_and_bad_state_dicts_are_refused(tiny):
    cfg, model = tiny
    sd = R.floats(model.state_dict())
    with pytest.raises(L.EdgeStyleHipError, match="quick_gelu"):
        _create(sd, cfg.vision_config, hidden_act="gelu")
    lib = L.load()
    vc = vision_config(cfg.vision_config, 64)
    vc.act = 1
    desc, _keep = state_dict_descriptors(sd)
    h = C.c_void_p()
    assert lib.es_clip_vision_create(C.byref(desc), C.byref(vc), L.ES_F16, 1, -1, C.byref(h)) == -1 and b"quick_gelu" in lib.es_last_error()
    rc, h, msg = _create(sd, cfg.vision_config, dtype=L.ES_F32)
    assert rc == -1 and "dtype" in msg
    for key in ("vision_model.pre_layrnorm.weight", "visual_projection.weight", "vision_model.embeddings.class_embedding",
                "vision_model.encoder.layers.1.mlp.fc2.bias"):
        rc, h, msg = _create({k: v for k, v in sd.items() if k != key}, cfg.vision_config)
        bare = key[len("vision_model."):] if key.startswith("vision_model.") else key
        assert rc == -1 and f"missing key '{bare}'" in msg, msg
    bad = dict(sd)
    bad["vision_model.embeddings.patch_embedding.weight"] = torch.zeros(128, 3, 16, 16)
    rc, h, msg = _create(bad, cfg.vision_config)
    assert rc == -1 and "size mismatch for 'embeddings.patch_embedding.weight': (128,3,16,16) vs (128,3,14,14)" in msg, msg
    rc, h, msg = _create(sd, cfg.vision_config, proj=32)
    assert rc == -1 and "size mismatch for 'visual_projection.weight'" in msg, msg


def test_kernel_entry_points_refuse_malformed_arguments():
    lib = L.load()
    mean, std = (C.c_float * 3)(*R.OPENAI_CLIP_MEAN), (C.c_float * 3)(*R.OPENAI_CLIP_STD)
    err = lambda: lib.es_last_error().decode()
    assert lib.es_clip_patchify(FAKE, FAKE, None, 1, 60, 14, mean, std, L.ES_F16, None) == -1 and "multiple of patch_size" in err()
    assert lib.es_clip_patchify(FAKE, None, None, 1, 56, 14, mean, std, L.ES_F16, None) == -1 and "null pointer" in err()
    assert lib.es_clip_patchify(FAKE, FAKE, None, 1, 56, 14, mean, std, L.ES_F32, None) == -1 and "dtype" in err()
    assert lib.es_clip_embed(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 16, 4104, 1e-5, L.ES_F16, None) == -1 and "at most 4096" in err()
    assert lib.es_clip_embed(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 1025, 128, 1e-5, L.ES_F16, None) == -1 and "patches" in err()
    seg = (C.c_int32 * 2)(7, 20)
    def score(**kw):
        d = dict(W=20, proj=64, seg=seg, nseg=2, k=2)
        d.update(kw)
        return lib.es_clip_score(FAKE, L.ES_F16, FAKE, 1, d["W"], d["proj"], 1.0, d["seg"], d["nseg"], d["k"], FAKE, FAKE, FAKE, None)
    assert score(k=9) == -1 and "k must be in 1..8" in err()
    assert score(W=21) == -1 and "must end at W" in err()
    assert score(nseg=5) == -1 and "nseg" in err()
    assert score(proj=66) == -1 and "proj" in err()
    assert score(W=5000) == -1 and "W must be in" in err()
    assert score(seg=(C.c_int32 * 2)(20, 20)) == -1 and "increasing" in err()
    h = C.c_void_p()
    assert lib.es_clip_bank_create(None, 0, 64, 10, 0, L.ES_F16, -1, C.byref(h)) == -1 and "device" in err()
    assert lib.es_clip_bank_rows(None) == 0


def test_every_new_call_is_refused_while_a_plan_records(tiny):
    cfg, model = tiny
    lib = L.load()
    rc, vis, msg = _create(R.floats(model.state_dict()), cfg.vision_config)
    assert rc == 0, msg
    plan = lib.es_plan_create()
    mean, std = (C.c_float * 3)(*R.OPENAI_CLIP_MEAN), (C.c_float * 3)(*R.OPENAI_CLIP_STD)
    seg = (C.c_int32 * 1)(20)
    img = (L.ImageU8 * 1)()
    img[0].data, img[0].height, img[0].width, img[0].channels, img[0].row_stride = FAKE, 30, 40, 3, 120
    eos = (C.c_int32 * 1)(3)
    h = C.c_void_p()
    try:
        assert lib.es_plan_begin_record(plan) == 0
        try:
            calls = [
                lambda: lib.es_image_resize_u8_ex(img, 1, FAKE, 56, L.FILTER_BICUBIC, L.CROP_TRANSFORMERS, FAKE, 1 << 20, None),
                lambda: lib.es_clip_patchify(FAKE, FAKE, None, 1, 56, 14, mean, std, L.ES_F16, None),
                lambda: lib.es_clip_embed(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 16, 128, 1e-5, L.ES_F16, None),
                lambda: lib.es_clip_score(FAKE, L.ES_F16, FAKE, 1, 20, 64, 1.0, seg, 1, 2, FAKE, FAKE, FAKE, None),
                lambda: lib.es_clip_bank_create(None, 0, 64, 10, 0, L.ES_F16, 0, C.byref(h)),
                lambda: lib.es_clip_bank_append(FAKE, FAKE, 1, None),
                lambda: lib.es_clip_text_pool(FAKE, FAKE, eos, 1, 77, None),
                lambda: _create(R.floats(model.state_dict()), cfg.vision_config)[0],
                lambda: lib.es_clip_vision_encode(vis, FAKE, 1, FAKE, None),
                lambda: lib.es_clip_pick(vis, FAKE, img, 1, 1.0, seg, 1, 2, FAKE, FAKE, FAKE, FAKE, 1 << 20, None),
            ]
            for i, call in enumerate(calls):
                assert call() == -1, i
                assert b"never part of a plan" in lib.es_last_error(), (i, lib.es_last_error())
        finally:
            lib.es_plan_end_record(plan)
        assert lib.es_plan_size(plan) == 0
    finally:
        lib.es_plan_destroy(plan)
        lib.es_clip_vision_destroy(vis)


def test_cli_flag_is_off_by_default():
    from edgestyle_amd.cli import parse_args
    assert parse_args([]).native_prompt_picker is False
    assert parse_args(["--native_prompt_picker"]).native_prompt_picker is True

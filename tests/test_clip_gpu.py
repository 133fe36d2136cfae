"""The CLIP prompt picker at the C ABI on the GPU: bicubic resampling against Pillow, es_clip_patchify / es_clip_embed / es_clip_score, the
image tower, the bank from the text side and the picks end to end (tests/clip_ref.py).

Metric and bar are the project's own (tests/numerics.py): row_err against an fp64 computation on the same inputs, at most MARGIN (2.0)
times the row_err of the textbook fp32 sequence with every op's output rounded to the storage dtype; every result finite.  Equalities
(resampled bytes, patch rows, top-k against the device's own logits, one image against its row in a batch) are bit for bit.  Every figure
is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from edgestyle_amd import lib as L
from edgestyle_amd.clip import NativeBestEmbeddings, eos_positions, vision_config
from edgestyle_amd.text import NativeCLIPTextEncoder, state_dict_descriptors
from tests import clip_ref as R
from tests import numerics as nm
from tests import text_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
ES_DT = {torch.float16: L.ES_F16, torch.bfloat16: L.ES_BF16, torch.float32: L.ES_F32}
GUARD = 4096


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


# ---- bicubic resampling ------------------------------------------------------------------------------------------------------------
def _resize(arrs, rr, strides=None):
    """es_image_resize_u8_ex(BICUBIC, transformers crop) of host images [H, W, 3 | 4] (row stride padded where `strides` says); the
    output sits between guard bytes, which are checked"""
    lib = L.load()
    n = len(arrs)
    keep, imgs = [], (L.ImageU8 * n)()
    for i, a in enumerate(arrs):
        h, w, ch = a.shape
        stride = strides[i] if strides else w * ch
        buf = torch.full((h, stride), 0x5A, dtype=torch.uint8)
        buf[:, :w * ch] = torch.from_numpy(a).reshape(h, w * ch)
        d = buf.to(DEV)
        keep.append(d)
        imgs[i].data, imgs[i].height, imgs[i].width, imgs[i].channels, imgs[i].row_stride = d.data_ptr(), h, w, ch, stride
    need = lib.es_image_resize_workspace_bytes_ex(imgs, n, rr, L.FILTER_BICUBIC, L.CROP_TRANSFORMERS)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
    body = n * rr * rr * 3
    out = torch.full((body + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    L.check(lib.es_image_resize_u8_ex(imgs, n, C.c_void_p(out.data_ptr() + GUARD), rr, L.FILTER_BICUBIC, L.CROP_TRANSFORMERS, _p(ws), need, _stream()),
            "es_image_resize_u8_ex")
    torch.cuda.synchronize()
    host = out.cpu()
    assert bool((host[:GUARD] == 0xA5).all()) and bool((host[GUARD + body:] == 0xA5).all()), "a write outside the output"
    return host[GUARD:GUARD + body].reshape(n, rr, rr, 3).numpy()


@pytest.mark.parametrize("h,w,ch,pad", [(300, 200, 3, 0), (97, 131, 3, 0), (40, 30, 3, 0), (56, 120, 3, 0), (97, 131, 4, 13)])
def test_bicubic_kernels_equal_pillow_byte_for_byte(h, w, ch, pad):
    """downscale, odd sizes with both axes shrinking, upscale, one axis skipped, four channels with a padded row stride"""
    a = R.photo(h, w, seed=h + w, channels=ch)
    got = _resize([a], 56, strides=[w * ch + pad])[0]
    want = R.pil_bicubic(a, 56)
    diff = int((got != want).sum())
    print(f"bicubic {h}x{w}x{ch} -> 56: {diff} differing bytes of {want.size}; output range {got.min()}..{got.max()}")
    assert diff == 0
    assert got.min() == 0 and got.max() == 255          # the edge of the fixture overshoots: clipping happened


def test_seventeen_images_in_one_call_cross_the_launch_cut():
    sizes = [(60 + 7 * i, 150 - 5 * i) for i in range(17)]
    arrs = [R.photo(h, w, seed=i) for i, (h, w) in enumerate(sizes)]
    got = _resize(arrs, 56)
    bad = [i for i, a in enumerate(arrs) if not np.array_equal(got[i], R.pil_bicubic(a, 56))]
    print(f"17 images, sizes {sizes[0]} .. {sizes[-1]}: images that differ from Pillow: {bad}")
    assert not bad


# ---- es_clip_patchify ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("rr,p", [(56, 14), (64, 16)])
def test_patchify_rows_are_the_rounded_formula_and_pad_columns_are_zero(rr, p, dt):
    from transformers import CLIPImageProcessor
    dtype, n = DTYPES[dt], 3
    lib = L.load()
    u8 = torch.from_numpy(np.stack([R.photo(rr, rr, seed=40 + i) for i in range(n)]))
    K, G = 3 * p * p, rr // p
    Kpad = (K + 63) // 64 * 64
    assert (Kpad > K) == (p == 14)
    rows = torch.full((n * G * G, Kpad), float("nan"), dtype=dtype, device=DEV)
    nchw = torch.full((n, 3, rr, rr), float("nan"), dtype=torch.float32, device=DEV)
    mean, std = (C.c_float * 3)(*R.OPENAI_CLIP_MEAN), (C.c_float * 3)(*R.OPENAI_CLIP_STD)
    u8_d = u8.to(DEV)
    L.check(lib.es_clip_patchify(_p(u8_d), _p(rows), _p(nchw), n, rr, p, mean, std, ES_DT[dtype], _stream()), "es_clip_patchify")
    torch.cuda.synchronize()
    pv = R.pixel_formula(u8)
    want = R.patch_rows(pv, p).reshape(n * G * G, K).to(dtype)
    got = rows.cpu()
    assert torch.equal(got[:, :K].view(torch.int16), want.view(torch.int16))
    assert bool((got[:, K:].view(torch.int16) == 0).all())                  # +0.0 exactly, not what the buffer held
    assert torch.equal(nchw.cpu(), pv)                                      # the fp32 values are that formula bit for bit
    proc = CLIPImageProcessor(do_resize=False, do_center_crop=False)
    ref = proc(images=[x.numpy() for x in u8], return_tensors="pt").pixel_values
    err = float((nchw.cpu() - ref).abs().max())
    print(f"patchify R={rr} p={p} {dt}: fp32 NCHW against the processor's pixel_values: max abs {err:.3e}; max |value| {float(ref.abs().max()):.3f}")
    assert float(ref.abs().max()) < 2.7 and err <= 1e-6


# ---- es_clip_embed ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("hidden", [128, 1024])
@pytest.mark.parametrize("P", [16, 256])
def test_embed_against_fp64(P, hidden, dt):
    dtype, eps = DTYPES[dt], 1e-5
    lib = L.load()
    for n in (1, 3):
        g = torch.Generator().manual_seed(P * 7 + hidden + n)
        patch = nm.rnd(torch.randn(n, P, hidden, generator=g), dtype)
        cls, pos = torch.randn(hidden, generator=g), 0.5 * torch.randn(P + 1, hidden, generator=g)
        gamma, beta = 1 + 0.2 * torch.randn(hidden, generator=g), 0.1 * torch.randn(hidden, generator=g)

        def ref(f, r):
            x = r(torch.cat([cls.to(f).reshape(1, 1, -1).expand(n, 1, hidden), patch.to(f)], 1) + pos.to(f)[None])
            return r(F.layer_norm(x, (hidden,), gamma.to(f), beta.to(f), eps))
        ref64 = ref(torch.float64, lambda t: t)
        base_t = ref(torch.float32, lambda t: nm.rnd(t, dtype))
        out = torch.full((n, P + 1, hidden), float("nan"), dtype=dtype, device=DEV)
        dev = [t.to(DEV) for t in (patch.to(dtype), cls, pos, gamma, beta)]          # alive until the synchronise below
        L.check(lib.es_clip_embed(*[_p(t) for t in dev], _p(out), n, P, hidden, eps, ES_DT[dtype], _stream()), "es_clip_embed")
        torch.cuda.synchronize()
        got = out.float().cpu()
        err, base = nm.row_err(got, ref64), nm.row_err(base_t, ref64)
        err0, base0 = nm.row_err(got[:, :1], ref64[:, :1]), nm.row_err(base_t[:, :1], ref64[:, :1])
        print(f"embed P={P} hidden={hidden} {dt} n={n}: row_err {err:.3e}, textbook {base:.3e}, ratio {err / base:.2f}; class rows {err0:.3e} vs {base0:.3e}")
        assert bool(torch.isfinite(got).all())
        assert err <= nm.MARGIN * base and err0 <= nm.MARGIN * base0


# ---- the tower -------------------------------------------------------------------------------------------------------------------------
class Tower:
    def __init__(self, sd, cfg, dtype, max_n):
        self.lib, self.cfg, self.dtype = L.load(), cfg, dtype
        vc = vision_config(cfg.vision_config, cfg.projection_dim)
        desc, keep = state_dict_descriptors({k: v for k, v in sd.items() if k.startswith("vision_model.") or k == "visual_projection.weight"})
        self.h = C.c_void_p()
        L.check(self.lib.es_clip_vision_create(C.byref(desc), C.byref(vc), ES_DT[dtype], max_n, torch.cuda.current_device(), C.byref(self.h)),
                "es_clip_vision_create")
        del keep

    def encode(self, u8):
        out = torch.full((u8.shape[0], self.cfg.projection_dim), float("nan"), dtype=self.dtype, device=DEV)
        u8_d = u8.to(DEV).contiguous()
        L.check(self.lib.es_clip_vision_encode(self.h, _p(u8_d), u8.shape[0], _p(out), _stream()), "es_clip_vision_encode")
        torch.cuda.synchronize()
        return out

    def close(self):
        self.lib.es_clip_vision_destroy(self.h)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape,n", [("tiny", 3), ("long", 2), ("wide", 2)])
def test_tower_end_to_end_against_fp64(shape, n, dt):
    """tiny: 17 tokens; long: 257 = 2 * 128 + 1 keys, a one-key tail behind whole tiles; wide: ViT-L/14's widths, one layer, 34 rows"""
    dtype = DTYPES[dt]
    cfg, sd, u8, ref64, base = R.tower_case(shape, dtype, n)
    tower = Tower(sd, cfg, dtype, n)
    try:
        got = tower.encode(u8)
        err = nm.row_err(got.float().cpu(), ref64)
        print(f"tower {shape} n={n} {dt}: row_err {err:.3e}, textbook {base:.3e}, ratio {err / base:.2f}")
        assert bool(torch.isfinite(got).all())
        assert err <= nm.MARGIN * base, (err, base)
        one = tower.encode(u8[1:2])
        assert torch.equal(one[0].view(torch.int16), got[1].view(torch.int16))       # a row does not depend on its neighbours
    finally:
        tower.close()


# ---- es_clip_score -----------------------------------------------------------------------------------------------------------------------
def _bank_from_rows(raw):
    lib = L.load()
    b = C.c_void_p()
    L.check(lib.es_clip_bank_create(None, 0, raw.shape[1], raw.shape[0], 0, L.ES_F16, torch.cuda.current_device(), C.byref(b)), "es_clip_bank_create")
    raw = raw.contiguous()
    L.check(lib.es_clip_bank_append(b, _p(raw), raw.shape[0], _stream()), "es_clip_bank_append")
    assert lib.es_clip_bank_rows(b) == raw.shape[0]
    return b


@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("W,segs", [(20, (7, 20)), (460, (270, 460))])
def test_score_logits_probabilities_and_top_k(W, segs, k):
    lib = L.load()
    proj, scale, dtype = 64, 20.0, torch.float16
    for n in (1, 5):
        g = torch.Generator().manual_seed(W + k + n)
        raw = torch.randn(W, proj, generator=g) * (0.5 + torch.rand(W, 1, generator=g))
        raw[5] = raw[2]                                                          # two identical rows: exactly equal logits
        pooled = nm.rnd(torch.randn(n, proj, generator=g) * 3.0, dtype)
        bank = _bank_from_rows(raw)
        try:
            seg = (C.c_int32 * 2)(*segs)
            logits, probs = (torch.full((n, W), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2))
            topk = torch.full((n, 2, k), -7, dtype=torch.int32, device=DEV)
            pooled_d = pooled.to(dtype).to(DEV)
            L.check(lib.es_clip_score(_p(pooled_d), ES_DT[dtype], lib.es_clip_bank_data(bank), n, W, proj, scale, seg, 2, k, _p(logits),
                                      _p(probs), _p(topk), _stream()), "es_clip_score")
            torch.cuda.synchronize()
        finally:
            lib.es_clip_bank_destroy(bank)
        lg, pr, tk = logits.cpu(), probs.cpu(), topk.cpu()
        ref64 = R.logits_from(pooled, R.unit(raw.double()), scale, "fp64")
        base = nm.row_err(R.logits_from(pooled, R.unit(raw, lambda t: nm.rnd(t, dtype)), scale, "rounded", dtype), ref64)
        err = nm.row_err(lg, ref64)
        print(f"score W={W} k={k} n={n}: logits row_err {err:.3e}, textbook {base:.3e}, ratio {err / base:.2f}")
        assert bool(torch.isfinite(lg).all()) and err <= nm.MARGIN * base
        assert torch.equal(lg[:, 5], lg[:, 2])
        a = 0
        for s, e in enumerate(segs):
            psum = pr[:, a:e].double().sum(dim=1)
            want_p = torch.softmax(lg[:, a:e].double(), dim=1)
            print(f"  segment {s} [{a}, {e}): |sum p - 1| {float((psum - 1).abs().max()):.3e}, max |p - softmax(logits)| {float((pr[:, a:e] - want_p).abs().max()):.3e}")
            assert float((psum - 1).abs().max()) <= 1e-5 and float((pr[:, a:e] - want_p).abs().max()) <= 1e-5
            order = torch.argsort(lg[:, a:e], dim=1, descending=True, stable=True)[:, :k].to(torch.int32)
            m = order.shape[1]
            assert torch.equal(tk[:, s, :m], order), (tk[:, s], order)
            assert bool((tk[:, s, m:] == -1).all())                              # a segment shorter than k: nothing more to rank
            a = e
        # the pair of identical rows lies in segment 0: wherever both are ranked, the lower index comes first
        for row in tk[:, 0].tolist():
            if 2 in row and 5 in row:
                assert row.index(2) + 1 == row.index(5)


# ---- the bank from the text side -----------------------------------------------------------------------------------------------------------
def _text_bank(sd, cfg, ids, dtype, max_n):
    """es_text_encoder -> es_clip_text_pool in runs of max_n; returns the bank's rows on the host"""
    lib = L.load()
    tc = cfg.text_config
    desc, keep = state_dict_descriptors({"text_projection.weight": sd["text_projection.weight"]})
    bank = C.c_void_p()
    L.check(lib.es_clip_bank_create(C.byref(desc), tc.hidden_size, cfg.projection_dim, ids.shape[0], max_n, ES_DT[dtype], torch.cuda.current_device(),
                                    C.byref(bank)), "es_clip_bank_create")
    enc = NativeCLIPTextEncoder(R.text_sd(sd), tc, dtype=dtype, device=DEV, max_n=max_n)
    try:
        eos = eos_positions(ids, tc.eos_token_id)
        for a in range(0, ids.shape[0], max_n):
            ehs = enc.encode_ids(ids[a:a + max_n])
            e = eos[a:a + max_n].contiguous()
            L.check(lib.es_clip_text_pool(bank, _p(ehs), e.numpy().ctypes.data_as(C.POINTER(C.c_int32)), ehs.shape[0], ids.shape[1], _stream()),
                    "es_clip_text_pool")
        W = lib.es_clip_bank_rows(bank)
        out = torch.empty((W, cfg.projection_dim), dtype=torch.float32, device=DEV)
        L.check(lib.es_memcpy(_p(out), lib.es_clip_bank_data(bank), W * cfg.projection_dim * 4, _stream()), "es_memcpy")
        torch.cuda.synchronize()
        return out.cpu()
    finally:
        enc.close()
        lib.es_clip_bank_destroy(bank)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("eos_id", [95, 2])
def test_bank_from_the_text_side_against_fp64(eos_id, dt):
    """eos_id 95: the first occurrence of eos_token_id, in the middle of the row (padding follows); eos_id 2: the legacy rule, the argmax of
    the ids (the same tokens: 95 is the largest id)"""
    dtype, n = DTYPES[dt], 5
    cfg = R.config(text=dict(eos_token_id=eos_id))
    sd = R.rounded_weights(R.make_model(cfg, seed=9).state_dict(), dtype)
    ids = TR.token_ids(R.config().text_config, n, seed=4)              # rows end in id 95 whatever the config under test calls eos
    pos = R.eos_positions(ids, eos_id)
    assert pos.tolist() == eos_positions(ids, eos_id).tolist() and all(0 < p < 76 for p in pos.tolist()) and len(set(pos.tolist())) > 1
    with torch.no_grad():
        ref64 = R.unit(R.text_forward(sd, cfg, ids, "fp64"))
        base = nm.row_err(R.unit(R.text_forward(sd, cfg, ids, "rounded", dtype), lambda t: nm.rnd(t, dtype)), ref64)
    got = _text_bank(sd, cfg, ids, dtype, max_n=2)           # 5 rows in runs of 2, 2, 1
    err = nm.row_err(got, ref64)
    norms = got.double().norm(dim=1)
    print(f"text bank eos_token_id={eos_id} {dt}: row_err {err:.3e}, textbook {base:.3e}, ratio {err / base:.2f}; |row| - 1 up to {float((norms - 1).abs().max()):.2e}")
    assert got.shape == ref64.shape and bool(torch.isfinite(got).all())
    assert err <= nm.MARGIN * base and float((norms - 1).abs().max()) <= 1e-6


# ---- picks end to end ----------------------------------------------------------------------------------------------------------------------
COLORS = ["red", "green", "blue", "black", "white", "pink", "teal"]
ITEMS = ["shirt", "dress", "coat", "jeans", "skirt", "vest", "scarf", "hoodie", "jacket"]
# Chosen on the CPU, from the reference alone, so that the condition asserted below holds: the model seed, logit_scale = log(100) as in
# OpenAI's checkpoints, and the seeds and sizes of the three photos (the second inverted, the third darkened to a quarter, so that the
# photos do not all pick the same words).  With these the smallest gap over the six (image, list) rows is 17 to 22 times that row's
# largest logit error of the rounded fp16 sequence, depending on the host's fp32 summation order (the bar is 8); in bf16 it is 1.9, so the
# test runs in fp16.
PICK_MODEL_SEED, PICK_LOGIT_SCALE = 20, 4.6052
PICK_PHOTOS = [(0, 90, 61), (1, 120, 200), (2, 56, 56)]


def _pick_case(tmp):
    from tests.test_text_gpu import _synthetic_tokenizer
    tok, vocab = _synthetic_tokenizer(tmp)
    cfg = R.config(text=dict(vocab_size=len(vocab), bos_token_id=vocab["<|startoftext|>"], eos_token_id=vocab["<|endoftext|>"],
                             pad_token_id=vocab["<|endoftext|>"]))
    model = R.make_model(cfg, seed=PICK_MODEL_SEED, logit_scale=PICK_LOGIT_SCALE)
    a, b, c = (R.photo(h, w, seed=s) for s, h, w in PICK_PHOTOS)
    return tok, cfg, model, [a, 255 - b, c // 4]


def test_picks_end_to_end_equal_the_fp64_picks(tmp_path):
    from PIL import Image
    from transformers import CLIPImageProcessor
    dtype, n_best = torch.float16, 2
    tok, cfg, model, photos = _pick_case(tmp_path)
    rr = cfg.vision_config.image_size
    sd = R.rounded_weights(model.state_dict(), dtype)
    proc = CLIPImageProcessor(size={"shortest_edge": rr}, crop_size={"height": rr, "width": rr})
    pv = proc(images=[Image.fromarray(a) for a in photos], return_tensors="pt").pixel_values
    ids = tok(COLORS + ITEMS, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    ref = R.forward(sd, cfg, pixel_values=pv, tokens=ids, mode="fp64")["logits_per_image"]
    rnd = R.forward(sd, cfg, pixel_values=pv, tokens=ids, mode="rounded", dtype=dtype)["logits_per_image"]
    want = []
    for name, a, e in (("colors", 0, len(COLORS)), ("items", len(COLORS), len(COLORS) + len(ITEMS))):
        srt = ref[:, a:e].sort(dim=1, descending=True)
        gap = srt.values[:, n_best - 1] - srt.values[:, n_best]
        noise = (rnd[:, a:e].double() - ref[:, a:e]).abs().max(dim=1).values
        for i in range(len(photos)):
            print(f"picks, {name}, image {i}: fp64 gap between rank {n_best} and {n_best + 1}: {float(gap[i]):.4e}; rounded sequence's max |logit error| "
                  f"{float(noise[i]):.4e}; ratio {float(gap[i] / noise[i]):.1f}")
        assert bool((gap >= 8 * noise).all()), "the reference alone does not separate the picks: choose other seeds"
        want.append(srt.indices[:, :n_best])
    words = [[COLORS[int(j)] for j in want[0][i]] + [ITEMS[int(j)] for j in want[1][i]] for i in range(len(photos))]
    be = NativeBestEmbeddings.from_module(model, tok, colors=COLORS, clothing_items=ITEMS, dtype=dtype, device=DEV, max_images=len(photos), text_batch=4)
    try:
        prompts = be([Image.fromarray(a) for a in photos])
        print("prompts:", prompts)
        assert len(set(prompts)) > 1                                             # the photos do not all choose the same words
        assert prompts == ["edgestyle, " + ", ".join(w) for w in words]
        assert be.find_best(COLORS, photos) == [w[:2] for w in words] and be.find_best(ITEMS, photos) == [w[2:] for w in words]
        # a list of the caller's own goes through a temporary bank; uint8 arrays, tensors and an RGBA copy are the same photo
        assert be.find_best(list(reversed(ITEMS)), photos[:1]) == [words[0][2:]]
        rgba = np.concatenate([photos[0], np.full(photos[0].shape[:2] + (1,), 7, np.uint8)], axis=-1)
        assert be([torch.from_numpy(photos[0])]) == be([rgba]) == prompts[:1]
        lg, pr, _ = be.score(photos, be._bank, be._segments, 2)
        err = nm.row_err(lg.cpu(), ref)
        base = nm.row_err(rnd, ref)
        print(f"picks: logits from bytes, row_err {err:.3e}, textbook {base:.3e}, ratio {err / base:.2f}")
        assert err <= nm.MARGIN * base
        with pytest.raises(L.EdgeStyleHipError, match="max_images"):
            be(photos + photos)
    finally:
        be.close()

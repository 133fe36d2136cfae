"""CPU restatements of the CLIP prompt picker (csrc/clip.hip) for tests/test_clip_cpu.py and tests/test_clip_gpu.py.

`forward(sd, cfg, pixel_values=..., tokens=..., mode=...)` is CLIPModel's forward written out with plain torch.nn.functional ops on a state
dict, under tests/text_ref.py's conventions:
    mode "fp32"     every op in fp32 - held against transformers' own CLIPModel in test_clip_cpu.py, which pins this file;
    mode "fp64"     the same ops in fp64: the truth the GPU results are measured against;
    mode "rounded"  the textbook fp32 sequence with every op's output rounded to the storage dtype (what the reference computes under
                    autocast): its row_err against fp64 times numerics.MARGIN is the bar of the GPU tests.
Linear weights, the patch convolution and the two projections are rounded to the storage dtype before anyone sees them
(`rounded_weights`); class embedding, position tables, biases, LayerNorm parameters and logit_scale stay fp32, as the library keeps them.
The text tower is text_ref.forward; this file adds the pooling, the projections and the logits."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import numerics as nm
from tests import text_ref as TR

QUICK_GELU = TR.QUICK_GELU
OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def config(image_size=56, patch_size=14, hidden=128, heads=2, layers=2, intermediate=256, projection_dim=64, text=None):
    """a small CLIPConfig: the vision widths are the arguments, the text tower is text_ref's tiny one (or `text`, CLIPTextConfig kwargs)"""
    from transformers import CLIPConfig
    tkw = dict(vocab_size=96, hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, max_position_embeddings=77,
               bos_token_id=94, eos_token_id=95, pad_token_id=95)
    tkw.update(text or {})
    vkw = dict(image_size=image_size, patch_size=patch_size, hidden_size=hidden, num_attention_heads=heads, num_hidden_layers=layers,
               intermediate_size=intermediate)
    return CLIPConfig(text_config=tkw, vision_config=vkw, projection_dim=projection_dim)


SHAPES = {
    # 17 tokens; 257 tokens (2 * 128 + 1: one key behind whole tiles); ViT-L/14's widths with one layer
    "tiny": dict(image_size=56, patch_size=14, hidden=128, heads=2, layers=2, intermediate=256, projection_dim=64),
    "long": dict(image_size=224, patch_size=14, hidden=128, heads=2, layers=2, intermediate=256, projection_dim=64),
    "wide": dict(image_size=56, patch_size=14, hidden=1024, heads=16, layers=1, intermediate=4096, projection_dim=768),
}


def make_model(cfg, seed=0, logit_scale=None):
    """random-init CLIPModel whose LayerNorm parameters and biases are NOT the trivial 1 / 0 of a fresh module (text_ref.make_model)"""
    from transformers import CLIPModel
    torch.manual_seed(seed)
    m = CLIPModel(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if ("layer_norm" in k or "layernorm" in k or "layrnorm" in k) and k.endswith(".weight"):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif k.endswith(".bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
        if logit_scale is not None:
            m.logit_scale.fill_(float(logit_scale))
    return m


def floats(sd):
    return {k: v.detach().clone() for k, v in sd.items() if v.is_floating_point()}


def _is_matrix(k):
    return (k.endswith("_proj.weight") or k.endswith("fc1.weight") or k.endswith("fc2.weight") or k.endswith("patch_embedding.weight")
            or k in ("visual_projection.weight", "text_projection.weight"))


def rounded_weights(sd, dtype):
    """the state dict with every matrix the library packs rounded to the storage dtype (kept in fp32)"""
    return {k: (nm.rnd(v, dtype) if _is_matrix(k) else v.clone()) for k, v in floats(sd).items()}


def text_sd(sd):
    return {k[len("text_model."):]: v for k, v in sd.items() if k.startswith("text_model.")}


def pixel_formula(u8_nhwc: torch.Tensor, mean=OPENAI_CLIP_MEAN, std=OPENAI_CLIP_STD) -> torch.Tensor:
    """es_clip_patchify's fp32 formula: ((b / 255) - mean) / std, every op an IEEE fp32 operation (numpy float32 arithmetic: two true
    divisions, no reciprocal); [n, R, R, 3] uint8 -> [n, 3, R, R] fp32"""
    x = u8_nhwc.numpy().astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255.0)
    m, s = (np.asarray(v, dtype=np.float32).reshape(1, 3, 1, 1) for v in (mean, std))
    return torch.from_numpy(np.ascontiguousarray((x - m) / s))


def patch_rows(pv: torch.Tensor, p: int) -> torch.Tensor:
    """[n, 3, R, R] -> [n, (R/p)^2, 3 p^2]: row = (patch row, patch column), column = (c, ky, kx) - the flattened conv weight's order"""
    n, c, R, _ = pv.shape
    g = R // p
    return pv.reshape(n, c, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(n, g * g, c * p * p)


def embed(sd, vc, patch, f, r):
    """class token + positions, then pre_layrnorm: patch [n, P, C] (the patch GEMM's output, already rounded in mode rounded)"""
    w = lambda k: sd["vision_model." + k].to(f)
    n, C = patch.shape[0], vc.hidden_size
    cls = w("embeddings.class_embedding").reshape(1, 1, C).expand(n, 1, C)
    x = r(torch.cat([cls, patch.to(f)], dim=1) + w("embeddings.position_embedding.weight")[None])
    return r(F.layer_norm(x, (C,), w("pre_layrnorm.weight"), w("pre_layrnorm.bias"), vc.layer_norm_eps))


def vision_forward(sd, cfg, pixel_values, mode, dtype=None):
    """image_embeds BEFORE the normalisation: [n, projection_dim]"""
    assert mode in ("fp32", "fp64", "rounded") and (mode != "rounded" or dtype is not None)
    f = torch.float64 if mode == "fp64" else torch.float32
    r = (lambda t: nm.rnd(t, dtype)) if mode == "rounded" else (lambda t: t)
    vc = cfg.vision_config
    w = lambda k: sd["vision_model." + k].to(f)
    C, H, eps, p = vc.hidden_size, vc.num_attention_heads, vc.layer_norm_eps, vc.patch_size
    rows = r(patch_rows(pixel_values.to(f), p))
    patch = r(rows @ w("embeddings.patch_embedding.weight").reshape(C, -1).t())
    x = embed(sd, vc, patch, f, r)
    n, S = x.shape[:2]
    scale = 1.0 / math.sqrt(C // H)
    heads = lambda t: t.reshape(n, S, H, C // H).transpose(1, 2)
    for i in range(vc.num_hidden_layers):
        q_ = f"encoder.layers.{i}."
        lin = lambda t, name: r(F.linear(t, w(q_ + name + ".weight"), w(q_ + name + ".bias")))
        h = r(F.layer_norm(x, (C,), w(q_ + "layer_norm1.weight"), w(q_ + "layer_norm1.bias"), eps))
        q, k, v = lin(h, "self_attn.q_proj"), lin(h, "self_attn.k_proj"), lin(h, "self_attn.v_proj")
        s = heads(q) @ heads(k).transpose(-1, -2) * scale
        a = r((r(torch.softmax(s, dim=-1)) @ heads(v)).transpose(1, 2).reshape(n, S, C))
        x = r(x + lin(a, "self_attn.out_proj"))
        h = r(F.layer_norm(x, (C,), w(q_ + "layer_norm2.weight"), w(q_ + "layer_norm2.bias"), eps))
        u = lin(h, "mlp.fc1")
        u = r(u * r(torch.sigmoid(r(QUICK_GELU * u))))
        x = r(x + lin(u, "mlp.fc2"))
    pooled = r(F.layer_norm(x[:, 0], (C,), w("post_layernorm.weight"), w("post_layernorm.bias"), eps))
    return r(pooled @ sd["visual_projection.weight"].to(f).t())


def eos_positions(ids, eos_token_id):
    """transformers' rule: the argmax of the ids where the config has the legacy eos_token_id == 2, else the first eos_token_id"""
    if eos_token_id == 2:
        return ids.to(torch.int).argmax(dim=-1)
    return (ids == eos_token_id).int().argmax(dim=-1)


def text_forward(sd, cfg, ids, mode, dtype=None):
    """text_embeds BEFORE the normalisation: [n, projection_dim]"""
    f = torch.float64 if mode == "fp64" else torch.float32
    r = (lambda t: nm.rnd(t, dtype)) if mode == "rounded" else (lambda t: t)
    last = TR.forward(text_sd(sd), cfg.text_config, ids, mode, dtype)
    pooled = last[torch.arange(ids.shape[0]), eos_positions(ids, cfg.text_config.eos_token_id)]
    return r(pooled.to(f) @ sd["text_projection.weight"].to(f).t())


def unit(x, r=lambda t: t):
    return r(x / x.norm(dim=-1, keepdim=True))


def logits_from(image_embeds, text_unit, scale_exp, mode, dtype=None):
    """logits_per_image from the raw image embeddings and the unit text rows, as CLIPModel.forward forms them"""
    f = torch.float64 if mode == "fp64" else torch.float32
    r = (lambda t: nm.rnd(t, dtype)) if mode == "rounded" else (lambda t: t)
    e = unit(image_embeds.to(f), r)
    return r(r(e @ text_unit.to(f).t()) * scale_exp)


def forward(sd, cfg, pixel_values=None, tokens=None, mode="fp32", dtype=None):
    """dict with image_embeds / text_embeds (raw), image_unit / text_unit (normalised) and logits_per_image, whichever the inputs allow"""
    r = (lambda t: nm.rnd(t, dtype)) if mode == "rounded" else (lambda t: t)
    out = {}
    with torch.no_grad():
        if pixel_values is not None:
            out["image_embeds"] = vision_forward(sd, cfg, pixel_values, mode, dtype)
            out["image_unit"] = unit(out["image_embeds"], r)
        if tokens is not None:
            out["text_embeds"] = text_forward(sd, cfg, tokens, mode, dtype)
            out["text_unit"] = unit(out["text_embeds"], r)
        if pixel_values is not None and tokens is not None:
            f = torch.float64 if mode == "fp64" else torch.float32
            out["logits_per_image"] = logits_from(out["image_embeds"], out["text_unit"], float(sd["logit_scale"].double().exp()), mode, dtype)
            assert out["logits_per_image"].dtype == f
    return out


def photo(h, w, seed, channels=3):
    """a seeded uint8 image with smooth gradients, noise and a hard black / white edge (negative cubic weights overshoot there)"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 255 // max(h + w - 2, 1))], axis=-1).astype(np.int64)
    img = np.clip(img + g.integers(-40, 41, size=img.shape), 0, 255)
    img[h // 3: h // 3 + max(h // 5, 2), : w // 2] = 255
    img[h // 3: h // 3 + max(h // 5, 2), w // 2:] = 0
    img = img.astype(np.uint8)
    if channels == 4:
        img = np.concatenate([img, g.integers(0, 256, size=(h, w, 1), dtype=np.uint8)], axis=-1)
    return np.ascontiguousarray(img)


def pil_bicubic(img_u8: np.ndarray, R: int) -> np.ndarray:
    """what CLIPImageProcessor does to a photo before the arithmetic: shortest edge -> R with Pillow's BICUBIC, then transformers' centre crop"""
    from PIL import Image
    h, w = img_u8.shape[:2]
    short, long_ = (w, h) if w <= h else (h, w)
    nl = int(R * long_ / short)
    rh, rw = (nl, R) if w <= h else (R, nl)
    out = np.array(Image.fromarray(img_u8[..., :3]).resize((rw, rh), resample=Image.BICUBIC))
    top, left = (rh - R) // 2, (rw - R) // 2
    return np.ascontiguousarray(out[top:top + R, left:left + R])


def images_u8(cfg, n, seed=0):
    """n seeded uint8 images [n, R, R, 3] at the tower's input size"""
    R = cfg.vision_config.image_size
    return torch.from_numpy(np.stack([photo(R, R, 100 * seed + i) for i in range(n)]))


@functools.lru_cache(maxsize=None)
def tower_case(shape, dtype, n):
    """(cfg, rounded state dict, uint8 images, fp64 image_embeds, row_err of the rounded textbook sequence) - once per (shape, dtype)"""
    cfg = config(**SHAPES[shape])
    sd = rounded_weights(make_model(cfg, seed=5).state_dict(), dtype)
    u8 = images_u8(cfg, n, seed=n)
    pv = pixel_formula(u8)
    with torch.no_grad():
        ref64 = vision_forward(sd, cfg, pv, "fp64")
        base = nm.row_err(vision_forward(sd, cfg, pv, "rounded", dtype), ref64)
    return cfg, sd, u8, ref64, base


# ---- the library's resampling taps applied on the host (tests/image_io_ref.py's integer_resize with the filter chosen) ----
def fit(h, w, R, crop):
    import ctypes as C
    from edgestyle_amd import lib as L
    out = (C.c_int32 * 4)()
    L.check(L.load().es_image_fit_ex(h, w, R, crop, out), "es_image_fit_ex")
    return tuple(out)                                   # rh, rw, top, left


def coeffs(filt, n_in, n_out):
    import ctypes as C
    from edgestyle_amd import lib as L
    lib = L.load()
    cap = lib.es_image_resize_coeffs_ex(filt, n_in, n_out, None, None, None, 0)
    assert cap >= 1, lib.es_last_error()
    xmin, nt, k = (C.c_int32 * n_out)(), (C.c_int32 * n_out)(), (C.c_int32 * (n_out * cap))()
    assert lib.es_image_resize_coeffs_ex(filt, n_in, n_out, xmin, nt, k, cap) == cap
    return np.array(xmin), np.array(nt), np.array(k).reshape(n_out, cap)


def resize_axis(a, n_out, axis, filt, stats=None):
    """one pass: out = clip8(((1 << 21) + sum k * src) >> 22); a pass that does not change the size is skipped.  stats (a dict): counts
    the negative weights and the sums that had to be clipped"""
    if a.shape[axis] == n_out:
        return a
    xmin, nt, k = coeffs(filt, a.shape[axis], n_out)
    src = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], dtype=np.uint8)
    for i in range(n_out):
        acc = (1 << 21) + np.tensordot(k[i, :nt[i]].astype(np.int64), src[xmin[i]:xmin[i] + nt[i]], axes=(0, 0))
        assert acc.max() < 2 ** 31 and acc.min() >= -2 ** 31        # the kernels accumulate in 32 bits
        if stats is not None:
            stats["negative_weights"] = stats.get("negative_weights", 0) + int((k[i, :nt[i]] < 0).sum())
            stats["clipped"] = stats.get("clipped", 0) + int(((acc >> 22) < 0).sum() + ((acc >> 22) > 255).sum())
        out[i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def integer_resize(a, rh, rw, filt, stats=None):
    """horizontal pass, then vertical pass, a uint8 image after each (Pillow's order)"""
    return resize_axis(resize_axis(a, rw, 1, filt, stats), rh, 0, filt, stats)

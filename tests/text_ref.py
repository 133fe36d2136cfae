"""CPU restatements of the CLIP text encoder (csrc/text.hip) for tests/test_text_cpu.py and tests/test_text_gpu.py.

`forward(sd, cfg, ids, mode)` is CLIPTextModel's last_hidden_state written out with plain torch.nn.functional ops on a state dict:
    mode "fp32"     every op in fp32 - held against transformers' own forward in test_text_cpu.py, which pins this file;
    mode "fp64"     the same ops in fp64: the truth the GPU results are measured against;
    mode "rounded"  the textbook fp32 sequence with every op's output rounded to the storage dtype (what the reference computes under
                    autocast): its row_err against fp64 times numerics.MARGIN is the bar of the GPU tests.
`causal_ref64` / `causal_base_ref` are numerics.attn_ref64 / attn_base_ref with the causal mask.
The convention for "the same inputs" is numerics.ln_case's: Linear weights are rounded to the storage dtype before anyone sees them
(`rounded_weights`); embedding tables, biases and LayerNorm parameters stay fp32, as the library keeps them."""
import functools
import math

import torch
import torch.nn.functional as F

from tests import numerics as nm

QUICK_GELU = 1.702


def tiny_config(**kw):
    from transformers import CLIPTextConfig
    base = dict(vocab_size=96, hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, max_position_embeddings=77,
                bos_token_id=94, eos_token_id=95, pad_token_id=95)
    base.update(kw)
    return CLIPTextConfig(**base)


def wide_config():
    """SD1.5's widths (ViT-L/14: 768 wide, 12 heads of 64, 3072 inside the MLP) with 2 layers and a small vocabulary"""
    return tiny_config(vocab_size=512, hidden_size=768, num_attention_heads=12, intermediate_size=3072, bos_token_id=510, eos_token_id=511,
                       pad_token_id=511)


def make_model(cfg, seed=0):
    """random-init CLIPTextModel whose LayerNorm parameters and biases are NOT the trivial 1 / 0 of a fresh module (the folds of the
    library multiply by gamma and add W beta: with 1 / 0 they would be checked against nothing)"""
    from transformers import CLIPTextModel
    torch.manual_seed(seed)
    m = CLIPTextModel(cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "layer_norm" in k and k.endswith(".weight"):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif k.endswith(".bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return m


def bare(sd):
    """keys without the `text_model.` prefix, float tensors only"""
    return {(k[len("text_model."):] if k.startswith("text_model.") else k): v.detach().clone() for k, v in sd.items() if v.is_floating_point()}


def rounded_weights(sd, dtype):
    """the state dict with every Linear weight rounded to the storage dtype (kept in fp32)"""
    return {k: (nm.rnd(v, dtype) if (k.endswith("_proj.weight") or k.endswith("fc1.weight") or k.endswith("fc2.weight")) else v.clone())
            for k, v in bare(sd).items()}


def _mask(S, f):
    return torch.full((S, S), float("-inf"), dtype=f).triu(1)


def forward(sd, cfg, ids, mode, dtype=None):
    assert mode in ("fp32", "fp64", "rounded") and (mode != "rounded" or dtype is not None)
    f = torch.float64 if mode == "fp64" else torch.float32
    r = (lambda t: nm.rnd(t, dtype)) if mode == "rounded" else (lambda t: t)
    w = lambda k: sd[k].to(f)
    C, H, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
    n, S = ids.shape
    scale = 1.0 / math.sqrt(C // H)
    heads = lambda t: t.reshape(n, S, H, C // H).transpose(1, 2)
    x = r(w("embeddings.token_embedding.weight")[ids] + w("embeddings.position_embedding.weight")[:S])
    mask = _mask(S, f)
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}."
        lin = lambda t, name: r(F.linear(t, w(p + name + ".weight"), w(p + name + ".bias")))
        h = r(F.layer_norm(x, (C,), w(p + "layer_norm1.weight"), w(p + "layer_norm1.bias"), eps))
        q, k, v = lin(h, "self_attn.q_proj"), lin(h, "self_attn.k_proj"), lin(h, "self_attn.v_proj")
        s = heads(q) @ heads(k).transpose(-1, -2) * scale + mask
        a = r((r(torch.softmax(s, dim=-1)) @ heads(v)).transpose(1, 2).reshape(n, S, C))
        x = r(x + lin(a, "self_attn.out_proj"))
        h = r(F.layer_norm(x, (C,), w(p + "layer_norm2.weight"), w(p + "layer_norm2.bias"), eps))
        u = lin(h, "mlp.fc1")
        u = r(u * r(torch.sigmoid(r(QUICK_GELU * u))))
        x = r(x + lin(u, "mlp.fc2"))
    return r(F.layer_norm(x, (C,), w("final_layer_norm.weight"), w("final_layer_norm.bias"), eps))


def causal_ref64(q, k, v, heads):
    d = q.shape[-1] // heads
    s = nm._heads(q.double(), heads) @ nm._heads(k.double(), heads).transpose(-1, -2) / math.sqrt(d) + _mask(q.shape[1], torch.float64)
    return nm._unheads(torch.softmax(s, dim=-1) @ nm._heads(v.double(), heads))


def causal_base_ref(q, k, v, heads, dtype):
    """numerics.attn_base_ref under the mask: fp32 scores, softmax, P rounded to the storage dtype, P V in fp32, rounded"""
    d = q.shape[-1] // heads
    s = nm._heads(q.float(), heads) @ nm._heads(k.float(), heads).transpose(-1, -2) * (1.0 / math.sqrt(d)) + _mask(q.shape[1], torch.float32)
    return nm.rnd(nm._unheads(nm.rnd(torch.softmax(s, dim=-1), dtype) @ nm._heads(v.float(), heads)), dtype)


def token_ids(cfg, n, seed=0):
    """[n, max_positions] int64 ids like a padded prompt: bos, words, eos padding; ids 0 and vocab - 1 occur"""
    g = torch.Generator().manual_seed(1000 + seed)
    S, V = cfg.max_position_embeddings, cfg.vocab_size
    ids = torch.randint(0, V, (n, S), generator=g)
    ids[:, 0] = cfg.bos_token_id
    for r in range(n):
        ids[r, 20 + 11 * r:] = cfg.eos_token_id
    ids[0, 1], ids[0, 2] = 0, V - 1
    return ids


@functools.lru_cache(maxsize=None)
def encoder_case(shape, dtype, n):
    """(cfg, rounded state dict, ids, fp64 result, row_err of the rounded textbook sequence) - computed once per (shape, dtype)"""
    cfg = tiny_config() if shape == "tiny" else wide_config()
    sd = rounded_weights(make_model(cfg, seed=3).state_dict(), dtype)
    ids = token_ids(cfg, n, seed=n)
    with torch.no_grad():
        ref64 = forward(sd, cfg, ids, "fp64")
        base = nm.row_err(forward(sd, cfg, ids, "rounded", dtype), ref64)
    return cfg, sd, ids, ref64, base

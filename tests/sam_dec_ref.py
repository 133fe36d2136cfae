"""segment_anything 1.0's PromptEncoder and MaskDecoder, as EfficientViT-SAM builds them, and the predictor's arithmetic around them
(apply_coords, postprocess_masks, getBox) restated in plain torch over a state dict that carries segment_anything's key names
(`prompt_encoder.*`, `mask_decoder.*`, bare or under a prefix).  One walk (`Dec`) serves three purposes, as tests/sam_ref.py does:

  mode "fp64"     the truth the kernels are judged against;
  mode "fp32"     what the reference computes without autocast;
  mode "rounded"  the textbook op sequence in fp32 with every op's output and every matrix weight rounded to the storage dtype: the
                  `base_ref` of tests/NUMERICS.md.

segment_anything itself is not installed; the walk is pinned to the installed transformers' SamPromptEncoder / SamMaskDecoder /
SamPositionalEmbedding under the key map `hf_key` (tests/test_sam_decoder_cpu.py) and to the reference's own postprocess_masks / apply_coords /
getBox by the fixture tests/golden/ref_sam_decoder.safetensors.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

TWO_PI = 2 * np.pi


def config(embed_dim=256, heads=8, mlp_dim=2048, depth=2, grid=64, frame=1024, n_mask_tokens=4, iou_hidden=256, iou_depth=3,
           downsample=2, ln_eps=1e-5, ln2d_eps=1e-6):
    return dict(embed_dim=embed_dim, heads=heads, mlp_dim=mlp_dim, depth=depth, grid=grid, frame=frame, n_mask_tokens=n_mask_tokens,
                iou_hidden=iou_hidden, iou_depth=iou_depth, downsample=downsample, ln_eps=ln_eps, ln2d_eps=ln2d_eps)


REAL = config()
TINY = config(embed_dim=128, heads=4, mlp_dim=256, grid=8, frame=128, iou_hidden=128)


def rnd(x, dtype):
    return x.to(torch.float32).to(dtype).to(torch.float32)


# ---- the predictor's host arithmetic ------------------------------------------------------------------------------------------------
def preprocess_shape(old_h, old_w, long_side):
    """ResizeLongestSide.get_preprocess_shape"""
    scale = long_side * 1.0 / max(old_h, old_w)
    return int(old_h * scale + 0.5), int(old_w * scale + 0.5)


def apply_coords(coords, original_size, input_size):
    """EfficientViTSamPredictor.apply_coords: float64 numpy [..., 2] (x, y)"""
    old_h, old_w = original_size
    new_h, new_w = input_size
    coords = np.array(coords, dtype=float, copy=True)
    coords[..., 0] = coords[..., 0] * (new_w / old_w)
    coords[..., 1] = coords[..., 1] * (new_h / old_h)
    return coords


def get_box(mask, margin=20):
    """getBox of extract_dataset.py on a [H, W] array"""
    ys, xs = np.where(np.asarray(mask) > 0)
    if len(xs) == 0:
        return np.zeros(4)
    H, W = mask.shape
    return np.array([max(0, xs.min() - margin), max(0, ys.min() - margin), min(W, xs.max() + margin), min(H, ys.max() + margin)])


def postprocess_masks(masks, input_size, original_size, frame=1024):
    """EfficientViTSam.postprocess_masks: masks [B, M, L, L] in any float dtype"""
    masks = F.interpolate(masks, (frame, frame), mode="bilinear", align_corners=False)
    masks = masks[..., :input_size[0], :input_size[1]]
    return F.interpolate(masks, tuple(original_size), mode="bilinear", align_corners=False)


# ---- the networks -------------------------------------------------------------------------------------------------------------------
def random_state_dict(cfg, seed):
    """seeded weights under segment_anything's names; every matrix is randn / sqrt(fan_in), so a layer's output has a deviation near 1"""
    g = torch.Generator().manual_seed(seed)
    E, M, nm = cfg["embed_dim"], cfg["mlp_dim"], cfg["n_mask_tokens"]
    sd = {}

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    def lin(key, cout, cin):
        sd[key + ".weight"] = rn(cout, cin, scale=1 / math.sqrt(cin))
        sd[key + ".bias"] = rn(cout, scale=0.1)

    def ln(key, c):
        sd[key + ".weight"] = 1 + rn(c, scale=0.2)
        sd[key + ".bias"] = rn(c, scale=0.1)

    def attn(key, internal):
        for p in ("q_proj", "k_proj", "v_proj"):
            lin(f"{key}.{p}", internal, E)
        lin(f"{key}.out_proj", E, internal)

    sd["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"] = rn(2, E // 2)
    for i in range(4):
        sd[f"prompt_encoder.point_embeddings.{i}.weight"] = rn(1, E)
    sd["prompt_encoder.not_a_point_embed.weight"] = rn(1, E)
    sd["prompt_encoder.no_mask_embed.weight"] = rn(1, E)
    sd["mask_decoder.iou_token.weight"] = rn(1, E)
    sd["mask_decoder.mask_tokens.weight"] = rn(nm, E)
    t = "mask_decoder.transformer"
    for i in range(cfg["depth"]):
        attn(f"{t}.layers.{i}.self_attn", E)
        attn(f"{t}.layers.{i}.cross_attn_token_to_image", E // cfg["downsample"])
        attn(f"{t}.layers.{i}.cross_attn_image_to_token", E // cfg["downsample"])
        for k in range(1, 5):
            ln(f"{t}.layers.{i}.norm{k}", E)
        lin(f"{t}.layers.{i}.mlp.lin1", M, E)
        lin(f"{t}.layers.{i}.mlp.lin2", E, M)
    attn(f"{t}.final_attn_token_to_image", E // cfg["downsample"])
    ln(f"{t}.norm_final_attn", E)
    sd["mask_decoder.output_upscaling.0.weight"] = rn(E, E // 4, 2, 2, scale=1 / math.sqrt(E))
    sd["mask_decoder.output_upscaling.0.bias"] = rn(E // 4, scale=0.1)
    ln("mask_decoder.output_upscaling.1", E // 4)
    sd["mask_decoder.output_upscaling.3.weight"] = rn(E // 4, E // 8, 2, 2, scale=1 / math.sqrt(E // 4))
    sd["mask_decoder.output_upscaling.3.bias"] = rn(E // 8, scale=0.1)

    def mlp(key, cin, hidden, cout, depth):
        dims = [cin] + [hidden] * (depth - 1) + [cout]
        for k in range(depth):
            lin(f"{key}.layers.{k}", dims[k + 1], dims[k])
    for i in range(nm):
        mlp(f"mask_decoder.output_hypernetworks_mlps.{i}", E, E, E // 8, 3)
    mlp("mask_decoder.iou_prediction_head", E, cfg["iou_hidden"], nm, cfg["iou_depth"])
    return sd


STATS_RANGE = (0.1, 10.0)


def scaled_state_dict(cfg, seed, emb, points=None, labels=None, boxes=None, passes=8):
    """random_state_dict with every matrix (and its bias) scaled by a POWER OF TWO so that its output has a standard deviation near 1 on the
    probe (emb and prompts in the prompt frame), as tests/sam_ref.py does: randn / sqrt(fan_in) alone lets the output of an attention over 4096
    keys, and what follows it, collapse.  Powers of two keep the state dict reproducible bit for bit.  A few passes, because a layer's scale
    moves the layers behind it.  -> (sd, the final pass's deviations); `assert_stats` is the postcondition."""
    sd = random_state_dict(cfg, seed)
    stats = {}
    for _ in range(passes):
        d = Dec(cfg, sd, "fp32")
        d.stats = {}
        d.decode(emb, points, labels, boxes, True)
        stats, changed = d.stats, False
        for key, std in stats.items():
            if key + ".weight" in sd and sd[key + ".weight"].dim() >= 2:
                f = 2.0 ** round(math.log2(1.0 / max(std, 1e-30)))
                if f != 1.0:
                    sd[key + ".weight"] = sd[key + ".weight"] * f
                    sd[key + ".bias"] = sd[key + ".bias"] * f
                    changed = True
        if not changed:
            break
    return sd, stats


def assert_stats(stats):
    bad = {k: v for k, v in stats.items() if not STATS_RANGE[0] <= v <= STATS_RANGE[1]}
    assert stats and not bad, bad


class Dec:
    def __init__(self, cfg, sd, mode="fp64", dtype=None, prefix=""):
        assert mode in ("fp64", "fp32", "rounded") and (mode != "rounded" or dtype is not None)
        self.cfg, self.sd, self.mode, self.dtype, self.prefix = cfg, sd, mode, dtype, prefix
        self.ct = torch.float64 if mode == "fp64" else torch.float32
        self.stats = None                                         # a dict: the standard deviation of every layer's output, by key

    def _st(self, key, t):
        if self.stats is not None:
            self.stats[key] = float(t.double().std())
        return t

    def r(self, t):
        return rnd(t, self.dtype) if self.mode == "rounded" else t

    def p(self, key, weight=False):
        t = self.sd[self.prefix + key].to(self.ct)
        return rnd(t, self.dtype) if (weight and self.mode == "rounded") else t

    # ---- prompt encoder ----
    def pe(self, c01):
        """PositionEmbeddingRandom._pe_encoding of coordinates in [0, 1]: [..., 2] -> [..., E]"""
        c = 2 * c01 - 1
        c = c @ self.p("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix")
        c = TWO_PI * c
        return torch.cat([torch.sin(c), torch.cos(c)], dim=-1)

    def image_pe(self):
        """get_dense_pe: [E, grid, grid]"""
        g = self.cfg["grid"]
        ones = torch.ones(g, g, dtype=self.ct)
        y = (ones.cumsum(0) - 0.5) / g
        x = (ones.cumsum(1) - 0.5) / g
        return self.pe(torch.stack([x, y], dim=-1)).permute(2, 0, 1)

    def sparse(self, points=None, labels=None, boxes=None):
        """points [n, P, 2] and boxes [n, 4] in the prompt frame (after apply_coords), labels [n, P] -> [n, T, E]"""
        frame = self.cfg["frame"]
        out = []
        if points is not None and points.shape[1] > 0:
            pts = points.to(self.ct) + 0.5
            lab = labels.to(torch.int64)
            if boxes is None:
                pts = torch.cat([pts, torch.zeros(pts.shape[0], 1, 2, dtype=self.ct)], 1)
                lab = torch.cat([lab, -torch.ones(lab.shape[0], 1, dtype=torch.int64)], 1)
            e = self.pe(pts / frame)
            e = torch.where((lab == -1)[..., None], torch.zeros_like(e), e)
            e = e + torch.where((lab == -1)[..., None], self.p("prompt_encoder.not_a_point_embed.weight"), torch.zeros_like(e))
            for k in (0, 1):
                e = e + torch.where((lab == k)[..., None], self.p(f"prompt_encoder.point_embeddings.{k}.weight"), torch.zeros_like(e))
            out.append(e)
        if boxes is not None:
            c = (boxes.to(self.ct) + 0.5).reshape(-1, 2, 2)
            e = self.pe(c / frame)
            e = e + torch.stack([self.p("prompt_encoder.point_embeddings.2.weight")[0], self.p("prompt_encoder.point_embeddings.3.weight")[0]])
            out.append(e)
        return self.r(torch.cat(out, dim=1))

    def tokens(self, points=None, labels=None, boxes=None):
        """[iou_token; mask_tokens; sparse] -> [n, 1 + n_mask_tokens + T, E]"""
        s = self.sparse(points, labels, boxes)
        head = torch.cat([self.p("mask_decoder.iou_token.weight"), self.p("mask_decoder.mask_tokens.weight")], 0)
        return torch.cat([self.r(head)[None].expand(s.shape[0], -1, -1), s], dim=1)

    # ---- mask decoder ----
    def linear(self, key, x, relu=False):
        y = self._st(key, self.r(F.linear(x, self.p(key + ".weight", True), self.p(key + ".bias"))))
        return self.r(torch.relu(y)) if relu else y

    def ln(self, key, x):
        return self._st(key, self.r(F.layer_norm(x, (x.shape[-1],), self.p(key + ".weight"), self.p(key + ".bias"), self.cfg["ln_eps"])))

    def attn(self, key, q, k, v, heads):
        q, k, v = self.linear(key + ".q_proj", q), self.linear(key + ".k_proj", k), self.linear(key + ".v_proj", v)
        n, _, c = q.shape
        d = c // heads
        split = lambda t: t.reshape(n, -1, heads, d).transpose(1, 2)
        a = torch.softmax(split(q) @ split(k).transpose(-1, -2) / math.sqrt(d), dim=-1)
        o = self._st(key + ".attention", self.r((a @ split(v)).transpose(1, 2).reshape(n, -1, c)))
        return self.linear(key + ".out_proj", o)

    def transformer(self, tokens, keys, key_pe):
        """tokens [n, S, E], keys [n, HW, E], key_pe [HW, E] -> queries, keys"""
        h = self.cfg["heads"]
        t = "mask_decoder.transformer"
        queries, query_pe = tokens, tokens
        for i in range(self.cfg["depth"]):
            L = f"{t}.layers.{i}"
            if i == 0:
                queries = self.attn(L + ".self_attn", queries, queries, queries, h)
            else:
                q = self.r(queries + query_pe)
                queries = self.r(queries + self.attn(L + ".self_attn", q, q, queries, h))
            queries = self.ln(L + ".norm1", queries)
            q, k = self.r(queries + query_pe), self.r(keys + key_pe)
            queries = self.ln(L + ".norm2", self.r(queries + self.attn(L + ".cross_attn_token_to_image", q, k, keys, h)))
            queries = self.ln(L + ".norm3", self.r(queries + self.linear(L + ".mlp.lin2", self.linear(L + ".mlp.lin1", queries, relu=True))))
            q, k = self.r(queries + query_pe), self.r(keys + key_pe)
            keys = self.ln(L + ".norm4", self.r(keys + self.attn(L + ".cross_attn_image_to_token", k, q, queries, h)))
        q, k = self.r(queries + query_pe), self.r(keys + key_pe)
        queries = self.ln(t + ".norm_final_attn", self.r(queries + self.attn(t + ".final_attn_token_to_image", q, k, keys, h)))
        return queries, keys

    def mlp(self, key, x, depth):
        for k in range(depth):
            x = self.linear(f"{key}.layers.{k}", x, relu=k < depth - 1)
        return x

    def upscale(self, keys):
        """keys [n, HW, E] -> [n, E / 8, 4 grid, 4 grid]"""
        n, g = keys.shape[0], int(round(math.sqrt(keys.shape[1])))
        x = keys.transpose(1, 2).reshape(n, -1, g, g)
        u = "mask_decoder.output_upscaling"
        x = self._st(u + ".0", self.r(F.conv_transpose2d(x, self.p(u + ".0.weight", True), self.p(u + ".0.bias"), stride=2)))
        mu = x.mean(1, keepdim=True)
        var = (x - mu).pow(2).mean(1, keepdim=True)
        x = (x - mu) / torch.sqrt(var + self.cfg["ln2d_eps"])
        x = self.r(self.p(u + ".1.weight")[:, None, None] * x + self.p(u + ".1.bias")[:, None, None])
        x = self.r(F.gelu(x))
        x = self._st(u + ".3", self.r(F.conv_transpose2d(x, self.p(u + ".3.weight", True), self.p(u + ".3.bias"), stride=2)))
        return self.r(F.gelu(x))

    def decode(self, emb, points=None, labels=None, boxes=None, multimask=True):
        """emb [n, E, grid, grid] -> low-res logits [n, M, 4 grid, 4 grid], iou [n, M]; prompts in the prompt frame"""
        nm = self.cfg["n_mask_tokens"]
        tokens = self.tokens(points, labels, boxes)
        n = tokens.shape[0]
        src = self.r(emb.to(self.ct) + self.p("prompt_encoder.no_mask_embed.weight").reshape(1, -1, 1, 1))
        keys = src.flatten(2).transpose(1, 2)
        key_pe = self.r(self.image_pe()).flatten(1).t()
        queries, keys = self.transformer(tokens, keys, key_pe)
        up = self.upscale(keys)
        hyper = torch.stack([self.mlp(f"mask_decoder.output_hypernetworks_mlps.{i}", queries[:, 1 + i], 3) for i in range(nm)], 1)
        masks = self._st("masks", self.r(hyper @ up.flatten(2))).reshape(n, nm, up.shape[2], up.shape[3])
        iou = self.mlp("mask_decoder.iou_prediction_head", queries[:, 0], self.cfg["iou_depth"])
        sl = slice(1, None) if multimask else slice(0, 1)
        self.iou_row = iou                                       # the head's whole row [n, n_mask_tokens], before the slice
        return masks[:, sl], iou[:, sl]


def upscale_tail(g, ln_g, ln_b, w2, b2, hyper, grid, ct, eps=1e-6, rdt=None):
    """what es_sam_upscale_masks computes, from ConvT1's GEMM output g [n, Gh * Gw, 4 * C1] (column (2 dy + dx) * C1 + c): LayerNorm over
    the channels, erf-GELU, ConvT2 (w2 [C1, C2, 2, 2], b2), erf-GELU, the product with hyper [n, M, C2] -> [n, M, 4 Gh, 4 Gw] in `ct`.
    rdt: every op's output is rounded to it (the mask product's too, as the reference stores it)"""
    r = (lambda t: rnd(t, rdt).to(ct)) if rdt is not None else (lambda t: t)
    Gh, Gw = grid
    n, C1, C2, M = g.shape[0], w2.shape[0], w2.shape[1], hyper.shape[1]
    x = g.to(ct).reshape(n, Gh * Gw, 4, C1)
    mu = x.mean(-1, keepdim=True)
    var = (x - mu).pow(2).mean(-1, keepdim=True)
    y = r((x - mu) / torch.sqrt(var + eps) * ln_g.to(ct) + ln_b.to(ct))
    y = r(F.gelu(y))
    z = r(torch.einsum("npsc,cdq->npsqd", y, w2.to(ct).reshape(C1, C2, 4)) + b2.to(ct))
    z = r(F.gelu(z))
    m = r(torch.einsum("npsqd,nmd->nmpsq", z, hyper.to(ct)))
    return m.reshape(n, M, Gh, Gw, 2, 2, 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(n, M, 4 * Gh, 4 * Gw)


def convt1_as_gemm(w, b):
    """output_upscaling.0 (ConvTranspose2d [E, C1, 2, 2]) as the weight [4 * C1, E] and bias [4 * C1] of a 1x1 GEMM, column (2 dy + dx) * C1 + c"""
    E, C1 = w.shape[:2]
    return w.permute(2, 3, 1, 0).reshape(4 * C1, E), b.repeat(4)


# transformers' names for segment_anything's (SamPromptEncoder / SamMaskDecoder state dicts under "prompt_encoder." / "mask_decoder.")
def hf_key(key):
    k = key
    k = k.replace("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", "prompt_encoder.shared_embedding.positional_embedding")
    k = k.replace("prompt_encoder.point_embeddings.", "prompt_encoder.point_embed.")
    for i in range(1, 5):
        k = k.replace(f".norm{i}.", f".layer_norm{i}.")
    k = k.replace(".norm_final_attn.", ".layer_norm_final_attn.")
    k = k.replace("output_upscaling.0.", "upscale_conv1.").replace("output_upscaling.1.", "upscale_layer_norm.")
    k = k.replace("output_upscaling.3.", "upscale_conv2.")
    if "output_hypernetworks_mlps" in k or "iou_prediction_head" in k:
        last = 2
        k = k.replace(".layers.0.", ".proj_in.").replace(f".layers.{last}.", ".proj_out.").replace(".layers.1.", ".layers.0.")
    return k

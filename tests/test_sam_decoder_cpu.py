"""The SAM prompt encoder / mask decoder pieces without a GPU: the restatement tests/sam_dec_ref.py pinned to the installed transformers and
to the reference's own functions (the fixture), the host twins of the kernels' index code against both, and every refusal text."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

from edgestyle_amd import lib as L
from tests import sam_dec_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_sam_decoder.safetensors")
N_CASES = 4


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


# ---- a. the restatement against transformers -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hf():
    """transformers' SamPromptEncoder, SamMaskDecoder and SamPositionalEmbedding built offline from SamConfig(), loaded with a seeded
    state dict under segment_anything's names through sam_dec_ref.hf_key (every key must land), and the image embedding of the cases"""
    from transformers.models.sam import modeling_sam as M
    hcfg = M.SamConfig()
    cfg = D.config(ln_eps=hcfg.mask_decoder_config.layer_norm_eps)
    sd = D.random_state_dict(cfg, 11)
    pe, md, pos = M.SamPromptEncoder(hcfg), M.SamMaskDecoder(hcfg.mask_decoder_config), M.SamPositionalEmbedding(hcfg.vision_config)
    mapped = {D.hf_key(k): v for k, v in sd.items()}
    res = pe.load_state_dict({k[len("prompt_encoder."):]: v for k, v in mapped.items() if k.startswith("prompt_encoder.")}, strict=False)
    assert not res.unexpected_keys and all(k.startswith("mask_embed.") for k in res.missing_keys), res
    res = md.load_state_dict({k[len("mask_decoder."):]: v for k, v in mapped.items() if k.startswith("mask_decoder.")}, strict=True)
    pos.load_state_dict({"positional_embedding": sd["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"]})
    emb = torch.randn(2, cfg["embed_dim"], cfg["grid"], cfg["grid"], generator=_gen(12))
    return cfg, sd, pe.eval(), md.eval(), pos.eval(), emb


def _prompt(kind, n=2):
    g = _gen(13)
    pts = torch.rand(n, 3, 2, generator=g) * 1024
    lab = torch.tensor([[1, 0, -1], [1, 1, 0]])[:n]
    box = torch.rand(n, 4, generator=g) * 1024
    return dict(points=(pts, lab, None), box=(None, None, box), both=(pts, lab, box))[kind]


@pytest.mark.parametrize("multimask", [True, False], ids=["multi", "single"])
@pytest.mark.parametrize("kind", ["box", "points", "both"])
def test_restatement_equals_transformers_in_fp32(hf, kind, multimask):
    cfg, sd, pe, md, pos, emb = hf
    pts, lab, box = _prompt(kind)
    with torch.no_grad():
        sparse, dense = pe(None if pts is None else pts[:, None], None if lab is None else lab[:, None], None if box is None else box[:, None],
                           None)
        g = cfg["grid"]
        ones = torch.ones(g, g)
        image_pe = pos(torch.stack([(ones.cumsum(1) - 0.5) / g, (ones.cumsum(0) - 0.5) / g], dim=-1)).permute(2, 0, 1)[None]
        masks, iou = md(emb, image_pe, sparse, dense, multimask)[:2]
        dec = D.Dec(cfg, sd, "fp32")
        assert rel(dec.sparse(pts, lab, box), sparse[:, 0]) <= 1e-5
        assert rel(dec.image_pe(), image_pe[0]) <= 1e-5
        mine, mine_iou = dec.decode(emb, pts, lab, box, multimask)
    e_m, e_i = rel(mine, masks[:, 0]), rel(mine_iou, iou[:, 0])
    print(f"{kind} multimask={multimask}: masks {e_m:.2e}  iou {e_i:.2e}")
    assert mine.shape == masks[:, 0].shape == (2, 3 if multimask else 1, 4 * g, 4 * g)
    assert e_m <= 1e-5 and e_i <= 1e-5


def test_rounded_mode_is_close_to_fp64_and_not_equal():
    cfg = D.TINY
    sd = D.random_state_dict(cfg, 3)
    emb = torch.randn(1, cfg["embed_dim"], cfg["grid"], cfg["grid"], generator=_gen(4))
    box = torch.tensor([[10.0, 20.0, 90.0, 100.0]])
    ref, _ = D.Dec(cfg, sd, "fp64").decode(emb, boxes=box)
    for dt, bar in ((torch.float16, 0.05), (torch.bfloat16, 0.3)):
        got, _ = D.Dec(cfg, sd, "rounded", dt).decode(emb, boxes=box)
        e = rel(got, ref)
        print(dt, e)
        assert 0 < e < bar


@pytest.mark.parametrize("cfg", [D.TINY, D.config(grid=5)], ids=["tiny", "real_widths"])
def test_upscale_tail_equals_the_decoder_walk(cfg):
    """sam_dec_ref.upscale_tail (the yardstick of es_sam_upscale_masks: ConvT1 as a 1x1 GEMM in front, the mask product behind) equals
    Dec.upscale and hyper @ up of the walk that is pinned to transformers"""
    sd = D.random_state_dict(cfg, 5)
    dec = D.Dec(cfg, sd, "fp64")
    g = cfg["grid"]
    keys = torch.randn(2, g * g, cfg["embed_dim"], generator=_gen(6), dtype=torch.float64)
    hyper = torch.randn(2, 3, cfg["embed_dim"] // 8, generator=_gen(7), dtype=torch.float64)
    up = dec.upscale(keys)
    want = (hyper @ up.flatten(2)).reshape(2, 3, 4 * g, 4 * g)
    u = "mask_decoder.output_upscaling"
    wg, bg = D.convt1_as_gemm(sd[u + ".0.weight"].double(), sd[u + ".0.bias"].double())
    got = D.upscale_tail(keys @ wg.t() + bg, sd[u + ".1.weight"], sd[u + ".1.bias"], sd[u + ".3.weight"], sd[u + ".3.bias"], hyper, (g, g),
                         torch.float64)
    assert rel(got, want) <= 1e-12


def test_upscale_pack_places_every_weight_where_the_matrix_core_reads_it():
    """es_sam_upscale_pack: element j of lane l of fragment (t, s) is w[k = 32 s + 8 (l >> 4) + j][column 16 t + (l & 15)], column = (2 dy + dx) * C2 + c2"""
    for C1 in (32, 64):
        C2, KS = C1 // 2, C1 // 32
        w = torch.arange(C1 * C2 * 4, dtype=torch.float32).reshape(C1, C2, 2, 2) % 2039        # exact in both storage dtypes
        for dt, es in ((torch.float16, L.ES_F16), (torch.bfloat16, L.ES_BF16)):
            wr = w.to(dt).float()
            out = torch.empty(2 * C1 * C1, dtype=dt)
            L.check(L.load().es_sam_upscale_pack(C.c_void_p(wr.data_ptr()), C1, es, C.c_void_p(out.data_ptr())), "es_sam_upscale_pack")
            frag = out.float().reshape(4 * KS, KS, 64, 8)
            mat = wr.reshape(C1, C2, 4).permute(0, 2, 1).reshape(C1, 4 * C2)                    # [k, column]
            for t in range(4 * KS):
                for s in range(KS):
                    for lane in (0, 5, 16, 37, 63):
                        k0 = 32 * s + 8 * (lane >> 4)
                        assert torch.equal(frag[t, s, lane], mat[k0:k0 + 8, 16 * t + (lane & 15)])


# ---- b. the fixture from the reference's own functions -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return load_file(GOLDEN)


def _sizes(gold, k):
    H, W, nh, nw = (int(v) for v in gold[f"size_{k}"])
    return H, W, nh, nw


@pytest.mark.parametrize("k", range(N_CASES))
def test_restatement_equals_the_reference_functions(gold, k):
    H, W, nh, nw = _sizes(gold, k)
    assert D.preprocess_shape(H, W, 128) == (nh, nw)
    post = D.postprocess_masks(gold[f"logits_{k}"].double(), (nh, nw), (H, W), 128)
    assert float((post - gold[f"post_{k}"]).abs().max()) <= 1e-6
    real = D.preprocess_shape(H, W, 1024)
    assert np.array_equal(D.apply_coords(gold[f"coords_{k}"].numpy(), (H, W), real), gold[f"coords_out_{k}"].numpy())
    assert np.array_equal(D.apply_coords(gold[f"boxes_{k}"].numpy().reshape(-1, 2, 2), (H, W), real).reshape(-1, 4), gold[f"boxes_out_{k}"].numpy())
    assert np.array_equal(D.get_box(gold[f"mask_{k}"].numpy()), gold[f"box_{k}"].numpy())


def _fp(t):
    return t.ctypes.data_as(C.c_void_p)


def post_host(logits, S, nh, nw, H, W, want_u8=True):
    lg = np.ascontiguousarray(logits.numpy().astype(np.float32))
    count, Lr = lg.shape[0] * lg.shape[1], lg.shape[-1]
    f = np.empty((count, H, W), np.float32)
    m = np.empty((count, H, W), np.uint8)
    L.check(L.load().es_sam_postprocess_masks_host(_fp(lg), count, Lr, S, nh, nw, H, W, _fp(f), _fp(m) if want_u8 else None), "postprocess host")
    return torch.from_numpy(f).reshape(*logits.shape[:2], H, W), torch.from_numpy(m).reshape(*logits.shape[:2], H, W)


@pytest.mark.parametrize("k", range(N_CASES))
def test_postprocess_host_twin_against_the_reference(gold, k):
    """the kernel's index and weight code on the CPU: within 2 x torch fp32's own error of the reference's fp64 result, and the masks equal
    wherever the fp64 value is not within 1e-3 of zero"""
    H, W, nh, nw = _sizes(gold, k)
    lg, ref = gold[f"logits_{k}"], gold[f"post_{k}"]
    f, m = post_host(lg, 128, nh, nw, H, W)
    own = float((D.postprocess_masks(lg, (nh, nw), (H, W), 128).double() - ref).abs().max())
    err = float((f.double() - ref).abs().max())
    print(f"{H}x{W}: twin {err:.3e}  torch fp32 {own:.3e}")
    assert err <= 2 * own
    sure = ref.abs() >= 1e-3
    # the fixture's logits are 32 x 32 with a deviation of 4: a pixel within 1e-3 of zero is rare, and the share is bounded like on the GPU
    assert float((~sure).double().mean()) <= 1e-3
    assert torch.equal(m[sure].bool(), (ref > 0)[sure])


@pytest.mark.parametrize("k", range(N_CASES))
def test_bbox_host_twin_equals_get_box(gold, k):
    mask = gold[f"mask_{k}"].numpy()
    for margin in (20, 0, 3):
        stack = np.ascontiguousarray(np.stack([mask, np.zeros_like(mask), np.ones_like(mask), mask[::-1, ::-1]]))
        boxes = np.empty((4, 4), np.float32)
        L.check(L.load().es_mask_bbox_host(_fp(stack), _fp(boxes), 4, mask.shape[0], mask.shape[1], margin), "bbox host")
        for i in range(4):
            assert np.array_equal(boxes[i], D.get_box(stack[i], margin).astype(np.float32)), (k, margin, i)
        if margin == 20:
            assert np.array_equal(boxes[0], gold[f"box_{k}"].numpy().astype(np.float32))


def tokens_host(cfg, sd, size, points, labels, boxes, n):
    E = cfg["embed_dim"]
    keep = []

    def w(key):
        keep.append(np.ascontiguousarray(sd[key].numpy().astype(np.float32)))
        return keep[-1].ctypes.data
    d = L.SamPromptDesc()
    d.gauss = w("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix")
    keep.append(np.ascontiguousarray(np.concatenate([sd[f"prompt_encoder.point_embeddings.{i}.weight"].numpy() for i in range(4)], 0).astype(np.float32)))
    d.point_embeddings = keep[-1].ctypes.data
    d.not_a_point, d.iou_token, d.mask_tokens = w("prompt_encoder.not_a_point_embed.weight"), w("mask_decoder.iou_token.weight"), \
        w("mask_decoder.mask_tokens.weight")
    P = 0 if points is None else points.shape[1]
    for name, t, dt in (("points", points, np.float32), ("labels", labels, np.int32), ("boxes", boxes, np.float32)):
        if t is not None:
            keep.append(np.ascontiguousarray(np.asarray(t).astype(dt)))
            setattr(d, name, keep[-1].ctypes.data)
    d.n, d.P, d.embed_dim, d.n_mask_tokens, d.frame, d.orig_h, d.orig_w = n, P, E, cfg["n_mask_tokens"], cfg["frame"], size[0], size[1]
    T = L.load().es_sam_prompt_token_count(P, 1 if boxes is not None else 0)
    out = np.empty((n, 1 + cfg["n_mask_tokens"] + T, E), np.float32)
    rc = L.load().es_sam_prompt_tokens_host(C.byref(d), _fp(out))
    return rc, torch.from_numpy(out)


def ref_tokens(cfg, sd, size, points, labels, boxes, mode="fp64"):
    """the restatement on apply_coords' result, rounded once to fp32 as the library does"""
    real = D.preprocess_shape(size[0], size[1], cfg["frame"])
    pts = None if points is None else torch.from_numpy(D.apply_coords(np.asarray(points, dtype=np.float64), size, real).astype(np.float32))
    box = None if boxes is None else torch.from_numpy(
        D.apply_coords(np.asarray(boxes, dtype=np.float64).reshape(-1, 2, 2), size, real).reshape(-1, 4).astype(np.float32))
    lab = None if labels is None else torch.as_tensor(labels)
    return D.Dec(cfg, sd, mode).tokens(pts, lab, box)


@pytest.mark.parametrize("case", ["box", "p1", "p3", "p3box"])
def test_prompt_tokens_host_twin_against_fp64(case):
    cfg, size = D.REAL, (300, 451)
    sd = D.random_state_dict(cfg, 21)
    H, W = size
    pts = np.array([[[0.0, 0.0], [W, H], [W / 3 + 0.25, -7.5]], [[W - 1, H - 1], [12.5, 400.0], [2 * W, 5.0]]])
    lab = np.array([[1, 0, -1], [0, 1, 1]])
    box = np.array([[3.0, 4.0, 200.5, 299.0], [0.0, 0.0, W, H]])
    points, labels, boxes = dict(box=(None, None, box), p1=(pts[:, :1], lab[:, :1], None), p3=(pts, lab, None), p3box=(pts, lab, box))[case]
    rc, got = tokens_host(cfg, sd, size, points, labels, boxes, 2)
    assert rc == 0, L.load().es_last_error()
    ref = ref_tokens(cfg, sd, size, points, labels, boxes)
    own = float((ref_tokens(cfg, sd, size, points, labels, boxes, "fp32").double() - ref).abs().max())
    err = float((got.double() - ref).abs().max())
    print(f"{case}: rows {got.shape[1]}  twin {err:.3e}  torch fp32 {own:.3e}")
    assert got.shape == ref.shape
    assert err <= 2 * own
    if case == "p3":      # the padding point and the label -1 are not_a_point_embed exactly
        nap = sd["prompt_encoder.not_a_point_embed.weight"][0]
        assert torch.equal(got[0, 5 + 2], nap) and torch.equal(got[0, 5 + 3], nap) and torch.equal(got[1, 5 + 3], nap)


def test_prompt_token_count():
    f = L.load().es_sam_prompt_token_count
    assert [f(0, 1), f(1, 0), f(3, 0), f(17, 0), f(3, 1), f(0, 0), f(-1, 0)] == [2, 2, 4, 18, 5, 0, -1]


# ---- c. refusals ---------------------------------------------------------------------------------------------------------------------
def _refused(rc, text):
    assert rc == -1
    msg = L.load().es_last_error().decode()
    assert text in msg, (text, msg)
    return msg


def _prompt_desc(**over):
    d = L.SamPromptDesc()
    for name in ("gauss", "point_embeddings", "not_a_point", "iou_token", "mask_tokens", "points", "labels", "boxes", "tokens", "query_pe"):
        setattr(d, name, 64)
    d.n, d.P, d.embed_dim, d.n_mask_tokens, d.frame, d.orig_h, d.orig_w, d.dtype = 1, 2, 256, 4, 1024, 100, 100, L.ES_F16
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _lin_desc(**over):
    d = L.LinearTokensDesc()
    d.x = d.w = d.out = 64
    d.n, d.rows, d.K, d.N, d.dtype = 1, 5, 256, 256, L.ES_F16
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _up_desc(**over):
    d = L.SamUpscaleDesc()
    for name in ("g", "w_packed", "ln_gamma", "ln_beta", "bias2", "hyper", "out"):
        setattr(d, name, 64)
    d.n, d.grid_h, d.grid_w, d.C1, d.M, d.ln_eps, d.dtype = 1, 8, 8, 64, 3, 1e-6, L.ES_F16
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _refusals():
    lib = L.load()
    up = lambda **o: lib.es_sam_upscale_masks(C.byref(_up_desc(**o)), None)              # noqa: E731
    tok = lambda **o: lib.es_sam_prompt_tokens(C.byref(_prompt_desc(**o)), None)          # noqa: E731
    lin = lambda **o: lib.es_linear_tokens(C.byref(_lin_desc(**o)), None)                 # noqa: E731
    post = lambda *a: lib.es_sam_postprocess_masks(64, *a, 64, 64, None)                 # noqa: E731
    bbox = lambda *a: lib.es_mask_bbox(64, 64, *a, None)                                 # noqa: E731
    return [
        (lambda: tok(gauss=None), "null pointer (a weight)"), (lambda: tok(n=0), "n must be in 1..4096"),
        (lambda: tok(embed_dim=255), "embed_dim must be even and in 2..2048"), (lambda: tok(n_mask_tokens=0), "n_mask_tokens must be in 1..8"),
        (lambda: tok(P=-1), "P < 0"), (lambda: tok(points=None), "null pointer (points or labels with P > 0)"),
        (lambda: tok(P=0, boxes=None), "no prompt: neither points nor a box"), (lambda: tok(P=26), "more than 32 tokens"),
        (lambda: tok(P=27, boxes=None), "more than 32 tokens"), (lambda: tok(frame=0), "frame, orig_h and orig_w must be >= 1"),
        (lambda: tok(dtype=L.ES_F32), "dtype must be ES_F16 or ES_BF16"), (lambda: tok(tokens=None), "null pointer (tokens)"),
        (lambda: lib.es_sam_prompt_tokens_host(C.byref(_prompt_desc()), None), "null pointer (tokens_f32)"),
        (lambda: lin(x=None), "null pointer"), (lambda: lin(dtype=L.ES_F32), "dtype must be ES_F16 or ES_BF16"),
        (lambda: lin(n=0), "n must be in 1..4096"), (lambda: lin(rows=33), "rows must be in 1..32"),
        (lambda: lin(K=260), "K must be a multiple of 8 in 8..2048"), (lambda: lin(K=4096), "K must be a multiple of 8 in 8..2048"),
        (lambda: lin(N=6), "N must be a multiple of 4 in 4..2048"), (lambda: lin(ldx=250), "ldx must be a multiple of 8 and >= K"),
        (lambda: lin(ldo=8), "ldr and ldo must be >= N"), (lambda: lin(bsx=12), "sample strides must be >= 0, that of x a multiple of 8"),
        (lambda: lin(x=72), "x and w must be 16-byte aligned"),
        (lambda: post(0, 256, 1024, 10, 10, 10, 10), "count must be in 1..4096"), (lambda: post(1, 0, 1024, 10, 10, 10, 10), "L and S must be in 1..4096"),
        (lambda: post(1, 256, 1024, 1025, 10, 10, 10), "new_h and new_w must be in 1..S"),
        (lambda: post(1, 256, 1024, 10, 10, 5000, 10), "H and W must be in 1..4096"),
        (lambda: lib.es_sam_postprocess_masks(64, 1, 256, 1024, 10, 10, 10, 10, None, None, None), "null pointer (both outputs)"),
        (lambda: bbox(0, 10, 10, 20), "count must be in 1..4096"), (lambda: bbox(1, 0, 10, 20), "H and W must be in 1..4096"),
        (lambda: bbox(1, 10, 10, -1), "margin must be in 0..4096"), (lambda: lib.es_mask_bbox(64, 66, 1, 10, 10, 20, None), "boxes must be 4-byte aligned"),
        (lambda: lib.es_mask_bbox(None, 64, 1, 10, 10, 20, None), "null pointer"),
        (lambda: lib.es_sam_upscale_masks(None, None), "null pointer (desc)"), (lambda: up(g=None), "null pointer"),
        (lambda: up(dtype=L.ES_F32), "dtype must be ES_F16 or ES_BF16"), (lambda: up(n=0), "n must be in 1..4096"),
        (lambda: up(grid_h=0), "grid_h and grid_w must be in 1..256"), (lambda: up(C1=16), "C1 must be 32 or 64 (embed_dim 128 or 256)"),
        (lambda: up(M=5), "M must be in 1..4"), (lambda: up(g=72), "g and w_packed must be 16-byte aligned"),
        (lambda: up(ldh=8), "ldh must be >= C1 / 2 and bsh >= 0"),
        (lambda: lib.es_sam_upscale_pack(64, 48, L.ES_F16, 64), "C1 must be 32 or 64"),
        (lambda: lib.es_sam_upscale_pack(64, 64, L.ES_F32, 64), "dtype must be ES_F16 or ES_BF16"),
        (lambda: lib.es_sam_upscale_pack(None, 64, L.ES_F16, 64), "null pointer"),
        (lambda: lib.es_sam_prompt_tokens(None, None), "null pointer (desc)"), (lambda: lib.es_linear_tokens(None, None), "null pointer (desc)"),
        (lambda: lib.es_sam_postprocess_masks(None, 1, 256, 1024, 10, 10, 10, 10, 64, 64, None), "null pointer (logits)"),
    ]


def test_every_refusal_comes_before_any_launch_and_names_its_reason():
    """no GPU is present here: each call below returns -1 with its text, so nothing was launched"""
    seen = set()
    for call, text in _refusals():
        seen.add(_refused(call(), text).split(": ", 1)[1])
    src = open(os.path.join(ROOT, "edgestyle_amd", "csrc", "sam_decoder.hip")).read()
    texts = set(re.findall(r'fail\(who, "([^"]+)"\)', src)) - {"launch failed"}
    assert texts <= seen, texts - seen


def test_calls_refuse_while_a_plan_records():
    lib = L.load()
    plan = lib.es_plan_create()
    try:
        assert lib.es_plan_set_dry(1) == 0 and lib.es_plan_begin_record(plan) == 0
        for rc in (lib.es_sam_prompt_tokens(C.byref(_prompt_desc()), None), lib.es_linear_tokens(C.byref(_lin_desc()), None),
                   lib.es_sam_upscale_masks(C.byref(_up_desc()), None), lib.es_sam_postprocess_masks(64, 1, 256, 1024, 10, 10, 10, 10, 64, 64, None), lib.es_mask_bbox(64, 64, 1, 10, 10, 20, None)):
            _refused(rc, "a plan is recording on this thread")
    finally:
        lib.es_plan_end_record(plan)
        lib.es_plan_set_dry(0)
        lib.es_plan_destroy(plan)


def test_python_wrappers_refuse_bad_operands_without_a_gpu():
    from edgestyle_amd import sam
    with pytest.raises(L.EdgeStyleHipError, match="missing key"):
        sam.SamPromptWeights({}, device="cpu")
    sd = D.random_state_dict(D.TINY, 1)
    bad = dict(sd)
    bad["prompt_encoder.not_a_point_embed.weight"] = torch.zeros(1, 64)
    with pytest.raises(L.EdgeStyleHipError, match="not_a_point_embed.weight has shape"):
        sam.SamPromptWeights(bad, device="cpu")
    w = sam.SamPromptWeights({"sam." + k: v for k, v in sd.items()}, device="cpu", frame=128)
    assert (w.embed_dim, w.n_mask_tokens) == (128, 4)
    with pytest.raises(L.EdgeStyleHipError, match="CUDA fp16"):
        sam.linear_tokens(torch.zeros(1, 5, 256), torch.zeros(256, 256))
    with pytest.raises(L.EdgeStyleHipError, match="CUDA fp32"):
        sam.postprocess_masks(torch.zeros(1, 1, 8, 8), (4, 4), (4, 4))


# ---- d. the decoder object without a GPU ---------------------------------------------------------------------------------------------
def _dry(sd, **kw):
    from edgestyle_amd import sam
    return sam.NativeSamMaskDecoder(sd, torch.float16, "dry", **kw)


def test_dry_build_reports_the_arena_size():
    """device -1: everything but the allocation.  The arena holds at least the weights in the storage dtype and the activations it names, and
    grows with max_n by the per-image activations and constants"""
    cfg = D.TINY
    sd = D.random_state_dict(cfg, 1)
    kw = dict(heads=cfg["heads"], grid=cfg["grid"], frame=cfg["frame"])
    one, three = _dry(sd, max_n=1, **kw), _dry(sd, max_n=3, **kw)
    weights = sum(v.numel() for k, v in sd.items() if k.startswith("mask_decoder.") and v.dim() >= 2) * 2
    assert weights < one.arena_bytes < 64 * weights
    HW, E = cfg["grid"] ** 2, cfg["embed_dim"]
    per_image = (5 * HW * E + 3 * HW * E // 2) * 2 + 4 * 16 * HW * 4        # key_pe, dense, keys x 3, three projections, the low-res scratch
    assert three.arena_bytes - one.arena_bytes >= 2 * per_image
    assert (three.arena_bytes - one.arena_bytes) % 256 == 0
    with pytest.raises(L.EdgeStyleHipError, match="dry build"):
        one.decode(torch.zeros(1, E, cfg["grid"], cfg["grid"]), (10, 10), boxes=torch.zeros(1, 4))
    real = _dry(D.random_state_dict(D.REAL, 2))
    print("arena of the real decoder for 3 images:", real.arena_bytes >> 20, "MiB")
    assert 2 * 4.0e6 < real.arena_bytes < 256 << 20


_CREATE_REFUSALS = [
    (dict(embed_dim=96), "embed_dim must be a multiple of 64"),
    (dict(embed_dim=192), "embed_dim must be 128 or 256"),
    (dict(heads=3), "heads must divide embed_dim and embed_dim / attn_downsample"),
    (dict(heads=8, attn_downsample=4), "head widths 16 and 4 must be among es_attention's"),
    (dict(heads=32), "head widths 4 and 2 must be among es_attention's"),
    (dict(mlp_dim=4100), "mlp_dim must be a multiple of 8 in 8..2048"),
    (dict(iou_hidden=4), "iou_hidden must be a multiple of 8 in 8..2048"),
    (dict(depth=0), "depth must be in 1..16 and iou_depth in 2..8"),
    (dict(n_mask_tokens=3), "n_mask_tokens must be 4"),
    (dict(grid=65), "grid must be in 1..64"),
    (dict(frame=0), "frame must be in 1..4096"),
    (dict(ln_eps=0.0), "ln_eps and ln2d_eps must be positive"),
]


@pytest.mark.parametrize("over,text", _CREATE_REFUSALS, ids=[t[:40] for _, t in _CREATE_REFUSALS])
def test_decoder_create_refuses_with_the_reason(over, text):
    from edgestyle_amd import sam
    sd = D.random_state_dict(D.TINY, 1)
    cfg = sam.decoder_config_of_state_dict(sd, heads=4, grid=8, frame=128)
    for k, v in over.items():
        setattr(cfg, k, v)
    with pytest.raises(L.EdgeStyleHipError, match=re.escape(text)):
        _dry(sd, config=cfg)


def test_decoder_create_refuses_more_than_32_tokens_bad_arguments_and_mask_input():
    sd = D.random_state_dict(D.TINY, 1)
    kw = dict(heads=4, grid=8, frame=128)
    with pytest.raises(L.EdgeStyleHipError, match="more than 32 tokens: 1 \\+ n_mask_tokens \\+ max_points \\+ 2 = 33"):
        _dry(sd, max_points=26, **kw)
    assert _dry(sd, max_points=25, **kw).arena_bytes > 0
    with pytest.raises(L.EdgeStyleHipError, match="max_n must be in 1..64"):
        _dry(sd, max_n=0, **kw)
    lib = L.load()
    dec = _dry(sd, **kw)
    p = L.SamPrompts(boxes=64, mask_input=64, orig_h=10, orig_w=10)
    _refused(lib.es_sam_decode(dec._h, 64, C.byref(p), 1, 1, 64, 64, None), "mask_input is not supported")
    _refused(lib.es_sam_predict(dec._h, 64, C.byref(p), 1, 1, None, 64, 64, None, None), "mask_input is not supported")
    p.mask_input = None
    _refused(lib.es_sam_decode(dec._h, 64, C.byref(p), 4, 1, 64, 64, None), "n = 4 is outside 1..max_n = 3")
    _refused(lib.es_sam_decode(dec._h, 64, C.byref(p), 1, 1, 64, 64, None), "dry build")
    _refused(lib.es_sam_predict(dec._h, 64, C.byref(p), 1, 1, None, 64, None, None, None), "null pointer (both mask outputs)")
    p.boxes = None
    _refused(lib.es_sam_decode(dec._h, 64, C.byref(p), 1, 1, 64, 64, None), "no prompt: neither points nor a box")
    p.P = 9
    _refused(lib.es_sam_decode(dec._h, 64, C.byref(p), 1, 1, 64, 64, None), "P = 9 is outside 0..max_points = 8")


_KEYS = ["prompt_encoder.no_mask_embed.weight", "prompt_encoder.point_embeddings.2.weight", "mask_decoder.mask_tokens.weight",
         "mask_decoder.transformer.layers.1.self_attn.k_proj.weight", "mask_decoder.transformer.layers.0.cross_attn_image_to_token.out_proj.bias",
         "mask_decoder.transformer.layers.0.mlp.lin2.weight", "mask_decoder.transformer.layers.1.norm3.bias",
         "mask_decoder.transformer.final_attn_token_to_image.v_proj.weight", "mask_decoder.transformer.norm_final_attn.weight",
         "mask_decoder.output_upscaling.0.weight", "mask_decoder.output_upscaling.1.bias", "mask_decoder.output_upscaling.3.weight",
         "mask_decoder.output_hypernetworks_mlps.2.layers.1.weight", "mask_decoder.iou_prediction_head.layers.2.weight",
         "mask_decoder.iou_prediction_head.layers.1.bias"]


@pytest.mark.parametrize("key", _KEYS)
def test_a_missing_key_or_a_wrong_shape_names_the_key(key):
    from edgestyle_amd import sam
    sd = D.random_state_dict(D.TINY, 1)
    cfg = sam.decoder_config_of_state_dict(sd, heads=4, grid=8, frame=128)         # the config of the intact state dict
    for prefix in ("", "sam."):
        full = {prefix + k: v for k, v in sd.items()}
        missing = {k: v for k, v in full.items() if k != prefix + key}
        with pytest.raises(L.EdgeStyleHipError, match=re.escape(f"missing key '{key}'")):
            _dry(missing, config=cfg)
        t = full[prefix + key]
        bad = dict(full)
        bad[prefix + key] = torch.zeros(*t.shape[:-1], t.shape[-1] + 8)
        with pytest.raises(L.EdgeStyleHipError, match=re.escape(f"size mismatch for '{key}'")):
            _dry(bad, config=cfg)

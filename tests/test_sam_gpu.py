"""The EfficientViT-SAM image encoder on the GPU: its new kernels one by one and the whole encoder, against fp64.

Bars are tests/numerics.py's: row_err(kernel) against fp64 on the rounded inputs is at most MARGIN (2) x the row_err of the textbook fp32
computation with every op's output rounded to the storage dtype (`base_ref`), recomputed whenever the test runs; every result is finite;
every figure is printed before it is asserted.  The pieces launch into slices of NaN-filled buffers whose guards are checked."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from safetensors.torch import load_file

from edgestyle_amd import lib as L
from edgestyle_amd import ops
from edgestyle_amd.sam import NativeSamImageEncoder, PIXEL_MEAN, PIXEL_STD, sam_config
from tests import numerics as nm
from tests import sam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
ES = {torch.float16: L.ES_F16, torch.bfloat16: L.ES_BF16}
GUARD = 1024          # elements of NaN in front of and behind every guarded tensor
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_sam.safetensors")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def guarded(t_or_shape, dtype):
    """a tensor (or an output of that shape) as a slice of a NaN-filled device buffer; returns (view, intact) - intact() says whether the
    guards still hold nothing but NaN"""
    src = t_or_shape if torch.is_tensor(t_or_shape) else None
    shape = tuple(src.shape) if src is not None else tuple(t_or_shape)
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    view = big[GUARD:GUARD + n].view(shape)
    if src is not None:
        view.copy_(src.to(dtype))

    def intact():
        return bool(torch.isnan(big[:GUARD]).all()) and bool(torch.isnan(big[GUARD + n:]).all())
    return view, intact


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def judge(what, y, ref64, base, margin=nm.MARGIN):
    ek, eb = nm.row_err(y, ref64), nm.row_err(base, ref64)
    print(f"{what}: row_err kernel {ek:.3e}  base_ref {eb:.3e}  bar {margin * eb:.3e}")
    assert bool(torch.isfinite(y.float()).all()), what
    assert ek <= margin * eb, (what, ek, eb)


# ---- es_dwconv ----------------------------------------------------------------------------------------------------------------------
def dw_ref(x, w, bias, k, s, gelu, ct, rdt=None):
    """x [N, H, W, C], w [k * k, C], bias [C] | None -> [N, Ho, Wo, C] in `ct`; rdt: round the convolution's and the GELU's output to it"""
    p = k // 2
    N, H, W, Cc = x.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xp = F.pad(x.to(ct), (0, 0, p, p, p, p))
    y = torch.zeros(N, Ho, Wo, Cc, dtype=ct)
    for ky in range(k):
        for kx in range(k):
            y += xp[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s, :] * w[ky * k + kx].to(ct)
    if bias is not None:
        y = y + bias.to(ct)
    if rdt is not None:
        y = nm.rnd(y, rdt)
    if gelu:
        y = R.gelu_tanh(y)
        if rdt is not None:
            y = nm.rnd(y, rdt)
    return y


def run_dwconv(x, w, bias, k, s, gelu, dtype):
    N, H, W, Cc = x.shape
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xd, xi = guarded(x, dtype)
    wd, wi = guarded(w, dtype)
    out, oi = guarded((N, Ho, Wo, Cc), dtype)
    bd = bias.to(DEV) if bias is not None else None
    L.check(L.load().es_dwconv(ptr(xd), ptr(wd), ptr(bd) if bd is not None else None, ptr(out), N, H, W, Cc, k, s,
                               L.ACT_GELU_TANH if gelu else L.ACT_NONE, ES[dtype], stream()), "es_dwconv")
    torch.cuda.synchronize()
    assert xi() and wi() and oi(), "a guard was written"
    return out.float().cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("geom", [(5, 7), (16, 16), (33, 31), (1, 9)], ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("ks", [(3, 1), (3, 2), (5, 1)], ids=["k3s1", "k3s2", "k5s1"])
def test_dwconv_against_fp64(ks, geom, dtype):
    k, s = ks
    H, W = geom
    # every channel count with every option at N = 3 where the tensors are small; the wide ones once each, N = 1 and N = 3
    cases = [(Cc, 3, b, g) for Cc in (32, 96) for b in (False, True) for g in (False, True)]
    cases += [(1536, 3, True, False), (1536, 1, False, True), (6144, 1, True, True), (6144, 3 if H * W <= 256 else 1, False, False)]
    for i, (Cc, N, has_bias, gelu) in enumerate(cases):
        g = _gen(1000 * k + 100 * s + 10 * H + i)
        x = nm.rnd(torch.randn(N, H, W, Cc, generator=g), dtype)
        w = nm.rnd(torch.randn(k * k, Cc, generator=g) / k, dtype)
        bias = 0.5 * torch.randn(Cc, generator=g) if has_bias else None
        y = run_dwconv(x, w, bias, k, s, gelu, dtype)
        ref = dw_ref(x, w, bias, k, s, gelu, torch.float64)
        base = dw_ref(x, w, bias, k, s, gelu, torch.float32, dtype)
        assert y.shape == ref.shape
        judge(f"dwconv k{k} s{s} {H}x{W} C={Cc} N={N} bias={has_bias} gelu={gelu}", y, ref, base)
        if N == 3:      # a result does not depend on the batch
            y1 = run_dwconv(x[1:2], w, bias, k, s, gelu, dtype)
            assert torch.equal(y1, y[1:2])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_dwconv_with_zero_weights_returns_the_rounded_bias(dtype):
    g = _gen(5)
    for k, s in ((3, 1), (3, 2), (5, 1)):
        x = torch.randn(2, 9, 6, 96, generator=g)
        bias = torch.randn(96, generator=g)
        y = run_dwconv(x, torch.zeros(k * k, 96), bias, k, s, False, dtype)
        assert torch.equal(y, nm.rnd(bias, dtype).expand_as(y))


# ---- es_relu_linear_attention -------------------------------------------------------------------------------------------------------
def run_attention(a, b, heads, dtype):
    N, HW, _ = a.shape
    ad, ai = guarded(a, dtype)
    bd, bi = guarded(b, dtype)
    out, oi = guarded((N, HW, 2 * heads * 32), dtype)
    L.check(L.load().es_relu_linear_attention(ptr(ad), ptr(bd), ptr(out), N, HW, heads, ES[dtype], stream()), "es_relu_linear_attention")
    torch.cuda.synchronize()
    assert ai() and bi() and oi(), "a guard was written"
    return out.float().cpu()


def attention_ref(a, b, ct):
    """[N, HW, 3 heads 32] x 2 -> [N, HW, 2 heads, 32] through the restated LiteMLA.relu_linear_att"""
    N, HW, _ = a.shape
    ms = torch.cat([a, b], dim=2).to(ct).permute(0, 2, 1).reshape(N, -1, HW, 1)
    o = R.relu_linear_att(ms)                               # [N, 2 heads 32, HW, 1]
    return o.reshape(N, -1, 32, HW).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("HW", [4, 25, 256, 1024])
def test_relu_linear_attention_against_fp64(HW, dtype):
    for heads in (1, 16):
        for N in (1, 3):
            g = _gen(HW + 7 * heads + N)
            a = nm.rnd(torch.randn(N, HW, 96 * heads, generator=g), dtype)
            b = nm.rnd(torch.randn(N, HW, 96 * heads, generator=g), dtype)
            y = run_attention(a, b, heads, dtype).reshape(N, HW, 2 * heads, 32)
            ref = attention_ref(a, b, torch.float64)
            base = nm.rnd(attention_ref(a, b, torch.float32), dtype)
            judge(f"relu_linear_attention HW={HW} groups={2 * heads} N={N}", y, ref, base)
            if N == 3:
                y1 = run_attention(a[2:3], b[2:3], heads, dtype).reshape(1, HW, 2 * heads, 32)
                assert torch.equal(y1, y[2:3])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_relu_linear_attention_dead_groups_give_exact_zeros(dtype):
    g = _gen(11)
    N, HW, heads = 2, 37, 2
    a = nm.rnd(torch.randn(N, HW, 96 * heads, generator=g), dtype)
    b = nm.rnd(torch.randn(N, HW, 96 * heads, generator=g), dtype)
    a[:, :, 96 + 32:96 + 64] = -a[:, :, 96 + 32:96 + 64].abs() - 0.5          # group 1: every k negative
    b[:, :, 0:32] = -b[:, :, 0:32].abs() - 0.5                                # group 2 (b's first): every q negative
    y = run_attention(a, b, heads, dtype).reshape(N, HW, 2 * heads, 32)
    assert bool(torch.isfinite(y).all())
    assert bool((y[:, :, 1] == 0).all()) and bool((y[:, :, 2] == 0).all())
    ref = attention_ref(a, b, torch.float64)
    assert bool((ref[:, :, 1] == 0).all()) and bool((ref[:, :, 2] == 0).all())
    base = nm.rnd(attention_ref(a, b, torch.float32), dtype)
    live = [0, 3]
    judge("relu_linear_attention, live groups beside dead ones", y[:, :, live], ref[:, :, live], base[:, :, live])


def test_relu_linear_attention_with_values_near_2e4_in_fp16():
    dtype = torch.float16
    g = _gen(12)
    N, HW, heads = 1, 256, 2
    a = torch.randn(N, HW, 96 * heads, generator=g)
    b = torch.randn(N, HW, 96 * heads, generator=g)
    for t in (a, b):
        for h in range(heads):
            t[:, :, 96 * h + 64:96 * h + 96] = 2.0e4 * (1 + 0.05 * torch.randn(N, HW, 32, generator=g))
    a, b = nm.rnd(a, dtype), nm.rnd(b, dtype)
    y = run_attention(a, b, heads, dtype).reshape(N, HW, 2 * heads, 32)
    ref = attention_ref(a, b, torch.float64)
    assert float(ref.abs().max()) > 1.5e4
    judge("relu_linear_attention, v near 2e4", y, ref, nm.rnd(attention_ref(a, b, torch.float32), dtype))


# ---- es_sam_neck_merge --------------------------------------------------------------------------------------------------------------
def merge_ref(maps, ct, rdt=None):
    """maps: NHWC tensors -> [N, 64, 64, C]: bicubic to 64 x 64 (identity at 64 x 64), m0 + (m1 + m2)"""
    ups = []
    for m in maps:
        t = m.to(ct).permute(0, 3, 1, 2)
        if tuple(t.shape[-2:]) != (64, 64):
            t = F.interpolate(t, size=(64, 64), mode="bicubic", align_corners=False)
            if rdt is not None:
                t = nm.rnd(t, rdt)
        ups.append(t)
    rr = (lambda v: nm.rnd(v, rdt)) if rdt is not None else (lambda v: v)
    y = ups[0] if len(ups) == 1 else (rr(ups[0] + ups[1]) if len(ups) == 2 else rr(ups[0] + rr(ups[1] + ups[2])))
    return y.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("sizes", [(2,), (5,), (16,), (32,), (64,), (5, 16), (64, 2), (2, 32, 64), (16, 32, 64), (64, 64, 5)], ids=lambda s: "+".join(map(str, s)))
def test_neck_merge_against_fp64_interpolate(sizes, dtype):
    lib = L.load()
    for N, Cc in ((1, 256), (2, 8)):
        g = _gen(sum(sizes) + Cc)
        maps = [nm.rnd(torch.randn(N, s, s, Cc, generator=g) + 0.3, dtype) for s in sizes]
        devs = [guarded(m, dtype) for m in maps]
        out, oi = guarded((N, 64, 64, Cc), dtype)
        arr = (C.c_void_p * 3)(*[d[0].data_ptr() for d in devs])
        hs = (C.c_int32 * 3)(*sizes)
        L.check(lib.es_sam_neck_merge(arr, hs, hs, len(sizes), ptr(out), N, Cc, ES[dtype], stream()), "es_sam_neck_merge")
        torch.cuda.synchronize()
        assert oi() and all(d[1]() for d in devs), "a guard was written"
        y = out.float().cpu()
        ref = merge_ref(maps, torch.float64)
        base = merge_ref(maps, torch.float32, dtype)
        if sizes == (64,):
            assert torch.equal(y, maps[0])                  # read as it is
        else:
            judge(f"neck_merge {sizes} N={N} C={Cc}", y, ref, base)


# ---- es_sam_preprocess_u8 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_preprocess_equals_pillow_and_the_fp32_formula(dtype):
    lib = L.load()
    S = 512
    g = np.random.default_rng(3)
    smooth = lambda h, w, c: (np.clip(np.add.outer(np.linspace(0, 200, h), np.linspace(0, 55, w))[..., None] + g.normal(0, 20, (h, w, c)), 0, 255)).astype(np.uint8)
    photos = [smooth(300, 200, 3), smooth(97, 131, 3), smooth(512, 512, 3), smooth(200, 300, 4), smooth(512, 77, 3)]
    dev = [torch.from_numpy(p).to(DEV) for p in photos]
    wide = torch.zeros(200, 400, 4, dtype=torch.uint8, device=DEV)          # four channels inside rows of a wider buffer
    wide[:, :300] = dev[3]
    dev[3] = wide[:, :300]
    n = len(dev)
    imgs = (L.ImageU8 * n)()
    for i, t in enumerate(dev):
        imgs[i].data, imgs[i].height, imgs[i].width, imgs[i].channels, imgs[i].row_stride = t.data_ptr(), t.shape[0], t.shape[1], t.shape[2], t.stride(0)
    assert imgs[3].row_stride == 1600
    need = lib.es_sam_preprocess_u8_workspace_bytes(imgs, n, S)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
    nhwc, i1 = guarded((n, S, S, 8), dtype)
    nchw = torch.full((n, 3, S, S), float("nan"), dtype=torch.float32, device=DEV)
    u8 = torch.full((n, S, S, 3), 77, dtype=torch.uint8, device=DEV)
    hw = (C.c_int32 * (2 * n))()
    mean, std = (C.c_float * 3)(*PIXEL_MEAN), (C.c_float * 3)(*PIXEL_STD)
    L.check(lib.es_sam_preprocess_u8(imgs, n, S, mean, std, ES[dtype], ptr(nhwc), ptr(nchw), ptr(u8), hw, ptr(ws), need, stream()), "es_sam_preprocess_u8")
    torch.cuda.synchronize()
    assert i1()
    for i, p in enumerate(photos):
        b, t, (h, w) = R.preprocess_ref(p, S)
        assert (hw[2 * i], hw[2 * i + 1]) == (h, w) and max(h, w) == S
        got = u8[i].cpu().numpy()
        assert np.array_equal(got[:h, :w], b), f"photo {i}: the resized bytes differ from Pillow's"
        assert not got[h:].any() and not got[:, w:].any()
        f = nchw[i].cpu()
        assert torch.equal(f, t), f"photo {i}: max|d| {float((f - t).abs().max())}"
        assert bool((f[:, h:] == 0).all()) and bool((f[:, :, w:] == 0).all())
        x8 = nhwc[i].float().cpu()
        assert torch.equal(x8[..., :3], nm.rnd(t, dtype).permute(1, 2, 0)) and bool((x8[..., 3:] == 0).all())
    assert (hw[0], hw[1]) == (512, 341) and (hw[4], hw[5]) == (512, 512)


# ---- ES_ACT_GELU_TANH in the dense GEMM ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(1, 2, 19, 13, 64, 96, 1), (3, 1, 12, 12, 128, 320, 1), (3, 2, 17, 11, 32, 72, 2), (3, 1, 40, 40, 8, 32, 2)],
                         ids=["1x1", "1x1-cout320", "3x3", "3x3-stem"])
def test_gelu_tanh_epilogue_against_fp64(shape, dtype):
    k, N, H, W, cin, cout, stride = shape
    k = 3 if k == 3 else 1
    g = _gen(cin + cout)
    x = nm.rnd(torch.randn(N, H, W, cin, generator=g), dtype)
    w = nm.rnd(torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5 * 1.5, dtype)
    bias = 0.3 * torch.randn(cout, generator=g)
    res = nm.rnd(torch.randn(N, (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1, cout, generator=g), dtype)
    pw = ops.pack_weight(w, bias, dtype, DEV)
    y = ops.conv_gemm(x.to(DEV, dtype), pw, stride=stride, act=L.ACT_GELU_TANH, residual=res.to(DEV, dtype)).float().cpu()
    y_split = ops.conv_gemm(x.to(DEV, dtype), pw, stride=stride, act=L.ACT_GELU_TANH, residual=res.to(DEV, dtype), splitk=2 if cin * k * k >= 128 else None).float().cpu()

    def ref(ct, rdt=None):
        c = F.conv2d(x.to(ct).permute(0, 3, 1, 2), w.to(ct), bias.to(ct), stride, k // 2).permute(0, 2, 3, 1)
        if rdt is not None:
            c = nm.rnd(c, rdt)
        a = R.gelu_tanh(c)
        if rdt is not None:
            a = nm.rnd(a, rdt)
        o = a + res.to(ct)
        return nm.rnd(o, rdt) if rdt is not None else o
    r64, base = ref(torch.float64), ref(torch.float32, dtype)
    judge(f"conv_gemm + tanh-GELU {shape}", y, r64, base)
    judge(f"conv_gemm + tanh-GELU {shape}, split-K reduce", y_split, r64, base)
    plain = ops.conv_gemm(x.to(DEV, dtype), pw, stride=stride).float().cpu()
    assert not torch.equal(plain + res, y)                  # the activation is applied


# ---- the whole encoder --------------------------------------------------------------------------------------------------------------
def lib_config(cfg, S):
    return sam_config("l2", S, widths=cfg["widths"], depths=cfg["depths"], head_width=cfg["head_width"], head_depth=cfg["head_depth"], out_dim=cfg["out_dim"])


def pixel_rows(t):
    """[B, C, H, W] -> [B, H, W, C]: a row of row_err is one pixel's channels"""
    return t.permute(0, 2, 3, 1)


@pytest.fixture(scope="module")
def tiny():
    return R.random_state_dict(R.TINY, R.TINY_SEED), load_file(GOLDEN)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("S", [64, 128])
def test_encoder_pinned_to_the_reference(tiny, S, dtype):
    """the native encoder, built from the state dict the reference's own module loaded, against the reference's own fp64 outputs"""
    sd, gold = tiny
    x = gold[f"x{S}"].float()
    enc = NativeSamImageEncoder.from_state_dict(sd, lib_config(R.TINY, S), dtype=dtype, device=DEV, max_n=2)
    y = enc(x)
    base = R.forward(R.TINY, sd, x, "rounded", dtype)
    for s in (2, 3, 4):
        judge(f"tiny S={S} stage{s}", pixel_rows(enc.stage(s, 1).cpu()), pixel_rows(gold[f"stage{s}_{S}"]), pixel_rows(base[f"stage{s}"]))
    assert y.shape == (1, 8, 64, 64) and y.dtype == torch.float32
    judge(f"tiny S={S} output", pixel_rows(y.cpu()), pixel_rows(gold[f"out_{S}"]), pixel_rows(base["out"]))
    x2 = torch.cat([R.probe_image(S, seed=5), x])
    y2 = enc(x2)
    assert torch.equal(y2[1:2], y)                          # row 1 of a batch equals the image alone, bit for bit
    enc.close()


@pytest.fixture(scope="module")
def shallow():
    return R.random_state_dict(R.SHALLOW, seed=5)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("S", [128, 160])
def test_encoder_at_real_widths(shallow, S, dtype):
    """one block per stage at the real model's widths: every channel count of L2 and its 6144-channel depthwise launch; S = 160 has 25 tokens"""
    x = R.probe_image(S, seed=S)
    enc = NativeSamImageEncoder.from_state_dict(shallow, lib_config(R.SHALLOW, S), dtype=dtype, device=DEV, max_n=1)
    y = enc(x)
    ref = R.forward(R.SHALLOW, shallow, x, "fp64")
    base = R.forward(R.SHALLOW, shallow, x, "rounded", dtype)
    for s in (2, 3, 4):
        judge(f"real widths S={S} stage{s}", pixel_rows(enc.stage(s, 1).cpu()), pixel_rows(ref[f"stage{s}"]), pixel_rows(base[f"stage{s}"]))
    judge(f"real widths S={S} output", pixel_rows(y.cpu()), pixel_rows(ref["out"]), pixel_rows(base["out"]))
    enc.close()


def test_l2_at_512_batch_row_and_graph_replay():
    """the model the reference loads, once: against the restatement, row 1 of a batch of 3 against the image alone, a replayed capture against
    the eager call"""
    dtype = torch.float16
    cfg = R.model_config("l2")
    sd = R.random_state_dict(cfg, seed=1)
    x = R.probe_image(512, seed=21)
    enc = NativeSamImageEncoder.from_state_dict(sd, sam_config("l2"), dtype=dtype, device=DEV, max_n=3)
    print(f"L2 arena for 3 images: {enc.arena_bytes / 2 ** 20:.0f} MiB")
    y = enc(x)
    torch.cuda.synchronize()
    ref = R.forward(cfg, sd, x, "fp64")["out"]
    base = R.forward(cfg, sd, x, "rounded", dtype)["out"]
    judge("L2 at 512 output", pixel_rows(y.cpu()), pixel_rows(ref), pixel_rows(base))
    x3 = torch.cat([R.probe_image(512, seed=22), x, R.probe_image(512, seed=23)]).to(DEV)
    y3 = enc(x3)
    assert torch.equal(y3[1:2], y)
    xd = x.to(DEV).contiguous()
    out = torch.zeros_like(y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            enc(xd, out=out)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, y)
    enc.close()


def test_from_module_and_encode_u8():
    """the drop-in contract on a module with the reference's key names, and photo bytes in: encode_u8 == es_sam_encode of the preprocessed tensor"""
    cfg = dict(R.SHALLOW, image_size=512)
    sd = R.random_state_dict(R.SHALLOW, seed=5)
    module = R.RefModule(cfg, sd)
    enc = NativeSamImageEncoder.from_module(module, dtype=torch.float16, device=DEV, max_n=2)
    assert list(enc.cfg.width) == [32, 64, 128, 256, 512] and enc.cfg.image_size == 512 and enc.to("cpu") is enc
    rng = np.random.default_rng(4)
    photo = np.clip(np.add.outer(np.linspace(20, 220, 300), np.linspace(0, 30, 200))[..., None] + rng.normal(0, 25, (300, 200, 3)), 0, 255).astype(np.uint8)
    feats, hw = enc.encode_u8([photo])
    assert hw == [(512, 341)] and feats.shape == (1, 256, 64, 64) and feats.dtype == torch.float32 and feats.device.type == "cuda"
    _, t, _ = R.preprocess_ref(photo, 512)
    y = enc(t[None])
    assert torch.equal(y, feats)                            # bit for bit
    want = module(t[None])                                  # the module it replaces: same shape and dtype contract, and close to it
    assert want.shape == y.shape and want.dtype == y.dtype
    print(f"from_module: row_err against the fp32 module {nm.row_err(pixel_rows(y.cpu()), pixel_rows(want)):.3e}")
    from PIL import Image
    both, hw2 = enc.encode_u8([Image.fromarray(photo), torch.from_numpy(photo[:97, :131].copy())])
    assert hw2 == [(512, 341), (379, 512)] and torch.equal(both[0:1], feats)
    enc.close()

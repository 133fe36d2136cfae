"""The SAM prompt encoder / mask decoder kernels of csrc/sam_decoder.hip on the GPU, one by one and chained, against fp64.

Bars are tests/numerics.py's and tests/test_sam_gpu.py::judge: row_err(kernel) against fp64 on the rounded inputs is at most MARGIN (2) x the
row_err of the fp32 restatement with every op's output rounded to the storage dtype, recomputed whenever the test runs; where the issue names
torch fp32 itself as the yardstick (prompt tokens, postprocess_masks) the bar is 2 x its maximum absolute error against fp64, measured here.
Every figure is printed before it is asserted, every output is finite, and operands and outputs sit in NaN-guarded slices whose guards are
checked."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from edgestyle_amd import lib as L
from edgestyle_amd import masks as MK
from edgestyle_amd import sam as S
from tests import numerics as nm
from tests import sam_dec_ref as D
from tests.test_sam_decoder_cpu import ref_tokens
from tests.test_sam_gpu import DEV, DTYPES, guarded, judge, ptr, stream

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- es_sam_prompt_tokens -----------------------------------------------------------------------------------------------------------
SIZE = (300, 451)


def _prompts(case, n):
    """(points [n, P, 2] | None, labels | None, boxes [n, 4] | None) in original pixels: 0, W, fractional and outside the image; labels -1 / 0 / 1"""
    H, W = SIZE
    g = _gen(31)
    P = dict(box=0, p1=1, p3=3, p17=17, p3box=3)[case]
    pts = torch.rand(3, 17, 2, generator=g, dtype=torch.float64) * torch.tensor([W, H])
    pts[0, 0] = torch.tensor([0.0, 0.0])
    pts[0, 1] = torch.tensor([float(W), float(H)])
    pts[0, 2] = torch.tensor([W / 3 + 0.25, -7.5])
    pts[1, 0] = torch.tensor([2.0 * W, H - 0.5])
    lab = torch.randint(-1, 2, (3, 17), generator=g)
    lab[0, :3] = torch.tensor([1, 0, -1])
    box = torch.tensor([[3.0, 4.0, 200.5, 299.0], [0.0, 0.0, W, H], [-5.0, 10.0, W + 30.0, 20.25]], dtype=torch.float64)
    with_box = case in ("box", "p3box")
    return (pts[:n, :P].numpy() if P else None, lab[:n, :P].numpy() if P else None, box[:n].numpy() if with_box else None)


def run_prompt_tokens(w, points, labels, boxes, n, dtype, boxes_dev=None):
    P = 0 if points is None else points.shape[1]
    rows = 1 + w.n_mask_tokens + S.prompt_token_count(P, boxes is not None or boxes_dev is not None)
    pd, pi = guarded(torch.from_numpy(points) if P else torch.zeros(1), torch.float32)
    bd, bi = guarded(torch.from_numpy(boxes) if boxes is not None else torch.zeros(1), torch.float32)
    ld = torch.from_numpy(labels).to(DEV, torch.int32).contiguous() if P else None
    tok, ti = guarded((n, rows, w.embed_dim), dtype)
    qpe, qi = guarded((n, rows, w.embed_dim), dtype)
    box_t = boxes_dev if boxes_dev is not None else (bd if boxes is not None else None)
    d = w.desc(n, P, SIZE, pd if P else None, ld, box_t, tok, qpe, dtype)
    L.check(L.load().es_sam_prompt_tokens(C.byref(d), stream()), "es_sam_prompt_tokens")
    torch.cuda.synchronize()
    assert pi() and bi() and ti() and qi(), "a guard was written"
    assert torch.equal(tok, qpe)
    return tok.float().cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", ["box", "p1", "p3", "p17", "p3box"])
def test_prompt_tokens_against_fp64(case, dtype):
    cfg = D.REAL
    sd = D.random_state_dict(cfg, 21)
    w = S.SamPromptWeights(sd, DEV)
    for n in (1, 3):
        points, labels, boxes = _prompts(case, n)
        y = run_prompt_tokens(w, points, labels, boxes, n, dtype)
        ref = ref_tokens(cfg, sd, SIZE, points, labels, boxes)
        base = nm.rnd(ref_tokens(cfg, sd, SIZE, points, labels, boxes, "fp32"), dtype)
        assert y.shape == ref.shape and bool(torch.isfinite(y).all())
        ek, eb = float((y.double() - ref).abs().max()), float((base.double() - ref).abs().max())
        print(f"prompt tokens {case} n={n} rows={y.shape[1]}: max abs err kernel {ek:.3e}  torch fp32 (rounded to storage) {eb:.3e}")
        assert ek <= 2 * eb
        if n == 3:
            p1, l1, b1 = _prompts(case, 1)
            assert torch.equal(run_prompt_tokens(w, p1, l1, b1, 1, dtype), y[:1])


# ---- es_linear_tokens ---------------------------------------------------------------------------------------------------------------
ROWS = (1, 5, 7, 16, 17, 32)
KN = [(256, 256), (256, 128), (128, 256), (256, 2048), (2048, 256), (256, 32), (256, 4)]


def lin_ref(x, w, b, relu, res, ct, rdt=None):
    """x [n, rows, K], w [N, K] | [rows, N, K]; rdt: round the linear's, the ReLU's and the add's output to it"""
    r = (lambda t: nm.rnd(t, rdt)) if rdt is not None else (lambda t: t)
    y = torch.einsum("nrk,rck->nrc", x.to(ct), w.to(ct)) if w.dim() == 3 else x.to(ct) @ w.to(ct).t()
    y = r(y + b.to(ct))
    if relu:
        y = r(torch.relu(y))
    if res is not None:
        y = r(y + res.to(ct))
    return y


def run_linear(x, w, b, relu, res, dtype, pad=0):
    n, rows, K = x.shape
    N = w.shape[-2]
    xd, xi = guarded(F.pad(x, (0, pad)), dtype)
    wd, wi = guarded(w, dtype)
    rd, ri = guarded(res if res is not None else torch.zeros(1), dtype)
    out, oi = guarded((n, rows, N), dtype)
    y = S.linear_tokens(xd[:, :, :K], wd, b.to(DEV), relu, rd if res is not None else None, out)
    torch.cuda.synchronize()
    assert xi() and wi() and ri() and oi(), "a guard was written"
    return y.float().cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("kn", KN, ids=lambda kn: f"K{kn[0]}N{kn[1]}")
def test_linear_tokens_against_fp64(kn, dtype):
    K, N = kn
    g = _gen(K + N)
    w = nm.rnd(torch.randn(N, K, generator=g) / K ** 0.5, dtype)
    # N = 4 with ReLU and no residual: a bias around 2 keeps every row's reference away from all zeros (row_err needs a scale per row)
    b = 0.5 * torch.randn(N, generator=g) + (2.0 if N == 4 else 0.0)
    for rows in ROWS:
        x3 = nm.rnd(torch.randn(3, rows, K, generator=g), dtype)
        r3 = nm.rnd(torch.randn(3, rows, N, generator=g), dtype)
        for relu in (False, True):
            for res in (None, r3):
                y = run_linear(x3, w, b, relu, res, dtype)
                ref = lin_ref(x3, w, b, relu, res, torch.float64)
                base = lin_ref(x3, w, b, relu, res, torch.float32, dtype)
                judge(f"linear_tokens K={K} N={N} rows={rows} relu={relu} res={res is not None}", y, ref, base)
                y1 = run_linear(x3[1:2], w, b, relu, None if res is None else res[1:2], dtype)
                assert torch.equal(y1, y[1:2])                   # n = 3 equals n = 1 bit for bit
        ys = run_linear(x3, w, b, True, r3, dtype, pad=24)      # rows 24 elements apart from dense
        assert torch.equal(ys, y)
    z = run_linear(x3, torch.zeros(N, K), b, False, None, dtype)
    assert torch.equal(z, nm.rnd(b, dtype).expand_as(z))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_linear_tokens_with_a_weight_set_per_row(dtype):
    """MaskDecoder.output_hypernetworks_mlps as one launch: row r of every sample has weights of its own"""
    g = _gen(77)
    for rows, K, N in ((4, 256, 256), (4, 256, 32), (3, 128, 16), (9, 64, 40)):
        x = nm.rnd(torch.randn(3, rows, K, generator=g), dtype)
        w = nm.rnd(torch.randn(rows, N, K, generator=g) / K ** 0.5, dtype)
        b = 0.5 * torch.randn(rows, N, generator=g)
        for relu in (False, True):
            y = run_linear(x, w, b, relu, None, dtype)
            judge(f"linear_tokens per row rows={rows} K={K} N={N} relu={relu}", y, lin_ref(x, w, b, relu, None, torch.float64),
                  lin_ref(x, w, b, relu, None, torch.float32, dtype))
            for r in range(rows):                                # each row equals the shared-weight launch of its own set
                assert torch.equal(run_linear(x[:, r:r + 1], w[r], b[r], relu, None, dtype), y[:, r:r + 1])


# ---- es_sam_upscale_masks -----------------------------------------------------------------------------------------------------------
def run_upscale(g, ln_g, ln_b, w2, b2, hyper, grid, dtype):
    gd, gi = guarded(g, dtype)
    wp, wi = guarded(S.upscale_pack(w2, dtype, "cpu"), dtype)
    hd, hi = guarded(hyper, dtype)
    n, M = hyper.shape[:2]
    out, oi = guarded((n, M, 4 * grid[0], 4 * grid[1]), torch.float32)
    S.upscale_masks(gd, wp, ln_g.to(DEV), ln_b.to(DEV), b2.to(DEV), hd, grid, 1e-6, out)
    torch.cuda.synchronize()
    assert gi() and wi() and hi() and oi(), "a guard was written"
    return out.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("grid", [(3, 5), (8, 8), (64, 64)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_upscale_masks_against_fp64(grid, dtype):
    """grids 3x5 (a ragged last tile of rows), 8x8 and the real 64x64 once; both channel counts; M = 1, 3, 4; n = 1 and 3"""
    big = grid == (64, 64)
    for C1 in ((64,) if big else (64, 32)):
        for M in ((3,) if big else (1, 3, 4)):
            g = _gen(100 * C1 + 10 * M + grid[0])
            n = 3
            x = nm.rnd(torch.randn(n, grid[0] * grid[1], 4 * C1, generator=g) * 1.5 + 0.3, dtype)
            ln_g, ln_b = 1 + 0.2 * torch.randn(C1, generator=g), 0.1 * torch.randn(C1, generator=g)
            w2 = nm.rnd(torch.randn(C1, C1 // 2, 2, 2, generator=g) / C1 ** 0.5, dtype)
            b2 = 0.1 * torch.randn(C1 // 2, generator=g)
            hyper = nm.rnd(torch.randn(n, M, C1 // 2, generator=g), dtype)
            y = run_upscale(x, ln_g, ln_b, w2, b2, hyper, grid, dtype)
            ref = D.upscale_tail(x, ln_g, ln_b, w2, b2, hyper, grid, torch.float64)
            base = D.upscale_tail(x, ln_g, ln_b, w2, b2, hyper, grid, torch.float32, rdt=dtype)
            assert y.shape == ref.shape
            judge(f"upscale_masks {grid[0]}x{grid[1]} C1={C1} M={M} n={n}", y, ref, base)
            y1 = run_upscale(x[1:2], ln_g, ln_b, w2, b2, hyper[1:2], grid, dtype)
            assert torch.equal(y1, y[1:2])                       # batch independence, bit for bit
            if M == 3 and not big:                               # hyper rows as a slice of a wider token matrix (rows 1..3 of [n, 5, C2])
                wide = torch.zeros(n, 5, C1 // 2)
                wide[:, 1:4] = hyper
                wd = wide.to(DEV, dtype)
                ys = S.upscale_masks(x.to(DEV, dtype), S.upscale_pack(w2, dtype), ln_g.to(DEV), ln_b.to(DEV), b2.to(DEV), wd[:, 1:4], grid)
                assert torch.equal(ys.cpu(), y)


# ---- es_sam_postprocess_masks -------------------------------------------------------------------------------------------------------
def seeded_logits(seed, count=2, low=256):
    lg = 4.0 * torch.randn(1, count, 16, 16, generator=_gen(seed))
    return F.interpolate(lg, (low, low), mode="bicubic", align_corners=False).contiguous()


@pytest.mark.parametrize("size", [(37, 53), (300, 451), (1024, 768), (1500, 1100)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_postprocess_masks_against_fp64(size):
    H, W = size
    lg = seeded_logits(H)
    new = D.preprocess_shape(H, W, 1024)
    ld, li = guarded(lg, torch.float32)
    f, fi = guarded((1, 2, H, W), torch.float32)
    m = torch.full((2 * H * W + 2048,), 7, dtype=torch.uint8, device=DEV)
    mv = m[1024:1024 + 2 * H * W].view(1, 2, H, W)
    L.check(L.load().es_sam_postprocess_masks(ptr(ld), 2, 256, 1024, new[0], new[1], H, W, ptr(f), ptr(mv), stream()), "es_sam_postprocess_masks")
    torch.cuda.synchronize()
    assert li() and fi() and bool((m[:1024] == 7).all()) and bool((m[1024 + 2 * H * W:] == 7).all()), "a guard was written"
    ref = D.postprocess_masks(lg.double(), new, size)
    own = float((D.postprocess_masks(lg, new, size).double() - ref).abs().max())
    y = f.cpu()
    err = float((y.double() - ref).abs().max())
    sure = ref.abs() >= 1e-3
    share = float((~sure).double().mean())
    print(f"postprocess {H}x{W}: max abs err kernel {err:.3e}  torch fp32 {own:.3e}  excluded {100 * share:.3f} %")
    assert bool(torch.isfinite(y).all()) and err <= 2 * own
    assert share <= 1e-3
    assert torch.equal(mv.cpu()[sure].bool(), (ref > 0)[sure])
    assert torch.equal(mv.cpu().bool(), y > 0)
    f2, m2 = S.postprocess_masks(ld, new, size, want_logits=True)          # either output alone, through the wrapper
    only_m = S.postprocess_masks(ld, new, size)[1]
    assert torch.equal(f2.cpu(), y) and torch.equal(m2, mv) and torch.equal(only_m, mv)


# ---- es_mask_bbox -------------------------------------------------------------------------------------------------------------------
def test_mask_bbox_equals_get_box():
    for H, W in ((64, 61), (300, 451), (9, 2049)):
        g = _gen(H)
        cases = [np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)]
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):           # a single corner pixel: the margin clipped at two sides each
            c = np.zeros((H, W), np.uint8)
            c[y, x] = 255
            cases.append(c)
        inner = np.zeros((H, W), np.uint8)
        inner[H // 3:H // 2 + 1, W // 4:W // 2 + 1] = 1
        cases.append(inner)
        cases.append((torch.rand(H, W, generator=g) < 0.001).numpy().astype(np.uint8))
        stack = np.stack(cases)
        for margin in (20, 0, 3):
            md = torch.full((stack.size + 2048,), 0, dtype=torch.uint8, device=DEV)
            mv = md[1024:1024 + stack.size].view(stack.shape)
            mv.copy_(torch.from_numpy(stack))
            boxes, bi = guarded((len(cases), 4), torch.float32)
            L.check(L.load().es_mask_bbox(ptr(mv), ptr(boxes), len(cases), H, W, margin, stream()), "es_mask_bbox")
            torch.cuda.synchronize()
            assert bi(), "a guard was written"
            want = np.stack([D.get_box(c, margin) for c in cases]).astype(np.float32)
            assert np.array_equal(boxes.cpu().numpy(), want), (H, W, margin)
        assert np.array_equal(MK.get_box(torch.from_numpy(inner)).cpu().numpy(), D.get_box(inner).astype(np.float32))


# ---- the whole decoder --------------------------------------------------------------------------------------------------------------
def _decoder_prompts(cfg, size, n, kind):
    H, W = size
    g = _gen(41)
    pts = (torch.rand(3, 2, 2, generator=g, dtype=torch.float64) * torch.tensor([W, H])).numpy()
    lab = np.array([[1, 0], [1, 1], [0, 1]])
    box = np.array([[0.1 * W, 0.2 * H, 0.8 * W, 0.9 * H], [0.0, 0.0, W, H], [0.3 * W, 0.1 * H, 0.6 * W, 0.5 * H]])
    return (pts[:n], lab[:n], None) if kind == "points" else (None, None, box[:n])


def _frame_prompts(cfg, size, points, labels, boxes):
    real = D.preprocess_shape(size[0], size[1], cfg["frame"])
    pts = None if points is None else torch.from_numpy(D.apply_coords(points, size, real).astype(np.float32))
    box = None if boxes is None else torch.from_numpy(D.apply_coords(boxes.reshape(-1, 2, 2), size, real).reshape(-1, 4).astype(np.float32))
    return pts, None if labels is None else torch.as_tensor(labels), box


def judge_iou(what, iou, d64, dbase, multimask):
    """judge for the IoU.  With multimask the returned row has three values and goes through judge as it is.  Without, the returned row is
    ONE value: row_err of the rounded base is then a single rounding draw, which can land arbitrarily close to zero and is no yardstick
    (measured: base 4.4e-4 = 0.9 ulp of fp16 on one value, next to 1.1e-3 .. 3.5e-3 on the three-value rows of the same decoder).  The
    IoU head computes all n_mask_tokens columns before the slice, so the scale and the base's error are taken over that whole row of the
    restatement - max over its columns of |base - ref64| / rms(ref64 row) - and the kernel's value is held to MARGIN x that, on the same scale."""
    if multimask:
        return judge(what, iou, d64.iou_row[:, 1:], dbase.iou_row[:, 1:])
    ref, base = d64.iou_row.double(), dbase.iou_row.double()
    rms = ref.pow(2).mean(dim=1, keepdim=True).sqrt()
    ek = float(((iou.double() - ref[:, :1]).abs() / rms).max())
    eb = float(((base - ref).abs() / rms).max())
    print(f"{what}: err kernel {ek:.3e}  base_ref over the head's row {eb:.3e}  bar {nm.MARGIN * eb:.3e}")
    assert bool(torch.isfinite(iou).all()) and ek <= nm.MARGIN * eb, (what, ek, eb)


def check_decoder(cfg, seed, size, dtype, cases, scaled=False):
    sd = D.random_state_dict(cfg, seed)
    if scaled:      # weights scaled by powers of two on the first case's inputs; every layer's deviation is asserted for EVERY case below
        n0, kind0, _ = cases[0]
        emb0 = nm.rnd(torch.randn(n0, cfg["embed_dim"], cfg["grid"], cfg["grid"], generator=_gen(seed + n0)), dtype)
        sd, _ = D.scaled_state_dict(cfg, seed, emb0, *_frame_prompts(cfg, size, *_decoder_prompts(cfg, size, n0, kind0)))
    dec = S.NativeSamMaskDecoder(sd, dtype, DEV, heads=cfg["heads"], grid=cfg["grid"], frame=cfg["frame"])
    for n, kind, multimask in cases:
        emb = nm.rnd(torch.randn(n, cfg["embed_dim"], cfg["grid"], cfg["grid"], generator=_gen(seed + n)), dtype)
        points, labels, boxes = _decoder_prompts(cfg, size, n, kind)
        low, iou = dec.decode(emb.to(DEV), size, points, labels, boxes, multimask)
        torch.cuda.synchronize()
        fp = _frame_prompts(cfg, size, points, labels, boxes)
        d64, dbase = D.Dec(cfg, sd, "fp64"), D.Dec(cfg, sd, "rounded", dtype)
        d64.stats = {} if scaled else None
        ref, ref_iou = d64.decode(emb, *fp, multimask)
        if scaled:
            print("layer deviations:", min(d64.stats.values()), "..", max(d64.stats.values()), "over", len(d64.stats), "layers")
            D.assert_stats(d64.stats)
        base, _ = dbase.decode(emb, *fp, multimask)
        assert low.shape == ref.shape and iou.shape == ref_iou.shape
        what = f"decoder E={cfg['embed_dim']} grid={cfg['grid']} n={n} {kind} multimask={multimask}"
        judge(what + " low-res logits", low.cpu(), ref, base)
        judge_iou(what + " iou", iou.cpu(), d64, dbase, multimask)
        if n == 3:                                               # image i of a batch equals the image alone, bit for bit
            one = lambda t: None if t is None else t[1:2]        # noqa: E731
            low1, iou1 = dec.decode(emb[1:2].to(DEV), size, one(points), one(labels), one(boxes), multimask)
            assert torch.equal(low1, low[1:2]) and torch.equal(iou1, iou[1:2]), what


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_tiny_decoder_against_fp64(dtype):
    check_decoder(D.TINY, 50, (100, 128), dtype, [(1, "box", True), (3, "box", False), (3, "points", True), (1, "points", False)])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_real_decoder_against_fp64_once(dtype):
    check_decoder(D.REAL, 60, (768, 1024), dtype, [(1, "box", False), (3, "points", True)], scaled=True)


def test_predict_masks_equal_fp64_away_from_zero():
    """NativeSamMaskDecoder.predict on the tiny config: masks equal the fp64 masks wherever |logit64| >= tau, tau = MARGIN x the rounded
    base's maximum absolute error at the photo's size, measured here; the excluded share is printed and at most 2 %.  Measured for this
    seed: tau 7.7e-3 at a logit deviation of 0.36, 0.53 % excluded on the MI355X; the rounded base alone (CPU) excludes 0.47 %."""
    cfg, size, dtype = D.TINY, (100, 128), torch.float16
    sd = D.random_state_dict(cfg, 50)
    dec = S.NativeSamMaskDecoder(sd, dtype, DEV, heads=cfg["heads"], grid=cfg["grid"], frame=cfg["frame"])
    emb = nm.rnd(torch.randn(1, cfg["embed_dim"], cfg["grid"], cfg["grid"], generator=_gen(51)), dtype)
    points, labels, boxes = _decoder_prompts(cfg, size, 1, "box")
    new = D.preprocess_shape(size[0], size[1], cfg["frame"])
    masks, iou, low = dec.predict(emb.to(DEV), new, size, boxes=boxes, multimask=True)
    torch.cuda.synchronize()
    fp = _frame_prompts(cfg, size, points, labels, boxes)
    post = lambda t: D.postprocess_masks(t.double(), new, size, cfg["frame"])          # noqa: E731
    ref = post(D.Dec(cfg, sd, "fp64").decode(emb, *fp, True)[0])
    base = post(D.Dec(cfg, sd, "rounded", dtype).decode(emb, *fp, True)[0])
    tau = nm.MARGIN * float((base - ref).abs().max())
    sure = ref.abs() >= tau
    share = float((~sure).double().mean())
    print(f"predict: tau {tau:.3e}  excluded {100 * share:.2f} %  logits std {float(ref.std()):.2f}")
    assert masks.shape == ref.shape and masks.dtype == torch.uint8
    assert share <= 0.02
    assert torch.equal(masks.cpu()[sure].bool(), (ref > 0)[sure])


def test_a_captured_predict_replays_bit_for_bit():
    cfg, size, dtype = D.TINY, (100, 128), torch.float16
    sd = D.random_state_dict(cfg, 50)
    dec = S.NativeSamMaskDecoder(sd, dtype, DEV, heads=cfg["heads"], grid=cfg["grid"], frame=cfg["frame"])
    emb = torch.randn(1, cfg["embed_dim"], cfg["grid"], cfg["grid"], generator=_gen(52)).to(DEV)
    new = D.preprocess_shape(size[0], size[1], cfg["frame"])
    box = torch.tensor([[10.0, 20.0, 100.0, 90.0]], device=DEV)
    want = dec.predict(emb, new, size, boxes=box, multimask=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = dec.predict(emb, new, size, boxes=box, multimask=True)
    torch.cuda.current_stream().wait_stream(side)
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ---- NativeSamPredictor and masks.segment -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def predictor_parts():
    """a small encoder whose out_dim is the tiny decoder's embed_dim (the neck's 64 x 64 grid is fixed), five seeded decoders and a photo"""
    from edgestyle_amd.sam import NativeSamImageEncoder, config_of_state_dict
    from tests import sam_ref as R
    ecfg = R.config(widths=(32, 32, 64, 64, 64), depths=(1, 1, 1, 1, 1), head_width=64, head_depth=1, out_dim=128, image_size=64)
    esd = R.random_state_dict(ecfg, 70)
    enc = NativeSamImageEncoder(esd, config_of_state_dict(esd, 64), torch.float16, DEV, max_n=1)
    cfg = D.config(embed_dim=128, heads=4, mlp_dim=256, grid=64, frame=128, iou_hidden=128)
    sds = [D.random_state_dict(cfg, 80 + i) for i in range(5)]
    class Part:                                             # a module as far as from_modules looks: state_dict() with segment_anything's names
        def __init__(self, sd, pre):
            self.sd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}

        def state_dict(self):
            return self.sd
    kw = dict(dtype=torch.float16, device=DEV, heads=4, grid=64, frame=128)
    decs = [S.NativeSamMaskDecoder.from_modules(Part(sds[0], "prompt_encoder."), Part(sds[0], "mask_decoder."), **kw)]
    decs += [S.NativeSamMaskDecoder.from_state_dict({"sam." + k: v for k, v in sd.items()}, **kw) for sd in sds[1:]]
    photo = (torch.rand(90, 120, 3, generator=_gen(71)) * 255).to(torch.uint8).numpy()
    return enc, cfg, sds, decs, photo


def test_predictor_follows_the_reference_surface(predictor_parts):
    """call order and errors as sam.py:336-339, the returned shapes and dtypes, and predict against the restated predictor on the encoder's
    own features (same bars as the decoder's; masks: tau 6.6e-3, 1.27 % of the pixels excluded as measured on the MI355X, cap 2 %)"""
    enc, cfg, sds, decs, photo = predictor_parts
    p = S.NativeSamPredictor(enc, decs[0])
    with pytest.raises(RuntimeError, match=r"An image must be set with \.set_image\(\.\.\.\) before mask prediction\."):
        p.predict(box=np.array([1, 2, 30, 40]))
    with pytest.raises(AssertionError, match="image_format must be in"):
        p.set_image(photo, "HSV")
    p.set_image(photo)
    assert p.is_image_set and p.original_size == (90, 120) and p.input_size == D.preprocess_shape(90, 120, 128)
    with pytest.raises(AssertionError, match="point_labels must be supplied"):
        p.predict(point_coords=np.array([[5.0, 6.0]]))
    box = np.array([10.0, 12.0, 100.0, 80.0])
    masks, iou, low = p.predict(box=box, multimask_output=False)
    assert masks.shape == (1, 90, 120) and masks.dtype == bool and iou.shape == (1,) and low.shape == (1, 256, 256)
    # the restated predictor on the encoder's own features: same bars as the decoder's
    emb = p.features.cpu()
    fp = _frame_prompts(cfg, (90, 120), None, None, box[None])
    d64, dbase = D.Dec(cfg, sds[0], "fp64"), D.Dec(cfg, sds[0], "rounded", torch.float16)
    ref, _ = d64.decode(emb, *fp, False)
    base, _ = dbase.decode(emb, *fp, False)
    judge("predictor low-res logits", torch.from_numpy(low)[None], ref, base)
    judge_iou("predictor iou", torch.from_numpy(iou)[None], d64, dbase, False)
    post = lambda t: D.postprocess_masks(t.double(), p.input_size, p.original_size, 128)          # noqa: E731
    r64 = post(ref)
    tau = nm.MARGIN * float((post(base) - r64).abs().max())
    sure = r64.abs() >= tau
    print(f"predictor masks: tau {tau:.3e}  excluded {100 * float((~sure).double().mean()):.2f} %")
    assert float((~sure).double().mean()) <= 0.02
    assert torch.equal(torch.from_numpy(masks)[None][sure], (r64 > 0)[sure])
    # predict_torch takes prompts in the input frame: the same box transformed on the host gives the same bits
    m2, iou2, low2 = p.predict_torch(boxes=fp[2].to(DEV), multimask_output=False)
    assert torch.equal(low2.cpu()[0], torch.from_numpy(low)) and torch.equal(m2.cpu()[0], torch.from_numpy(masks))
    three, iou3, _ = p.predict(point_coords=np.array([[60.0, 45.0], [10.0, 10.0]]), point_labels=np.array([1, 0]))
    assert three.shape == (3, 90, 120) and iou3.shape == (3,)
    p.reset_image()
    assert not p.is_image_set and p.features is None


def test_segment_equals_the_chain_through_the_host(predictor_parts):
    """masks.segment (no host visit) against the same five decodes with the box read back and handed in as numpy, as the reference does"""
    enc, cfg, sds, decs, photo = predictor_parts
    preds = [S.NativeSamPredictor(enc, d) for d in decs]
    pts = np.array([[60.0, 45.0], [50.0, 30.0], [70.0, 60.0]])
    images, score = MK.segment(photo, pts, preds)
    torch.cuda.synchronize()
    for p in preds:
        p.set_image(photo)
    all_masks, _, _ = preds[0].predict(point_coords=pts, point_labels=np.ones(3))
    box = D.get_box(all_masks[0])
    outs = [p.predict(box=box, multimask_output=False) for p in preds[1:]]
    want = MK.create_sam_images(photo, *(o[0][0] for o in outs))
    assert len(images) == 5 and all(torch.equal(a, b) for a, b in zip(images, want))
    assert score.is_cuda and float(score) == float(outs[0][1][0])


# ---- chained and captured -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_the_device_chain_equals_the_chain_through_the_host_and_replays(dtype):
    """logits -> es_sam_postprocess_masks -> es_mask_bbox -> es_sam_prompt_tokens with the box read from device memory: equal, bit for
    bit, to the same chain with the box round-tripped through the host, and a captured chain replays to the same bits"""
    H, W = SIZE
    sd = D.random_state_dict(D.REAL, 21)
    w = S.SamPromptWeights(sd, DEV)
    lg = seeded_logits(5, count=1).to(DEV)
    new = D.preprocess_shape(H, W, 1024)

    def chain(tokens):
        mask = S.postprocess_masks(lg, new, SIZE)[1]
        box = MK.get_box(mask[:, 0])
        d = w.desc(1, 0, SIZE, boxes=box, tokens=tokens, dtype=dtype)
        L.check(L.load().es_sam_prompt_tokens(C.byref(d), stream()), "es_sam_prompt_tokens")
        return mask, box
    tok = torch.zeros((1, 7, w.embed_dim), dtype=dtype, device=DEV)
    mask, box = chain(tok)
    torch.cuda.synchronize()
    host_box = D.get_box(mask[0, 0].cpu().numpy())
    assert host_box[2] > host_box[0] and np.array_equal(box.cpu().numpy()[0], host_box.astype(np.float32))
    via_host, _ = S.prompt_tokens(w, SIZE, boxes=host_box[None], dtype=dtype, want_query_pe=False)
    assert torch.equal(via_host, tok)
    out = torch.zeros_like(tok)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            chain(out)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, tok)

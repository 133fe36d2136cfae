"""The HIP kernels against fp64 at trained-model statistics (tests/numerics.py): per-row error, bars recomputed from CPU baselines
whenever the test runs.  Every case prints its figures before anything is asserted, and a test asserts once at its end, on the
list of every bar that was missed, so that one miss does not hide the others.

    row_err(kernel) <= MARGIN * row_err(base_alg)        always (probe tier: PROBE_MARGIN)   - the kernel does what its design says
    row_err(kernel) <= MARGIN * row_err(base_ref)        required tier                       - the design is adequate there
    finite wherever the fp64 reference, rounded to the storage dtype, is finite

`python -m tests.numerics --report` runs the same cases and writes tests/NUMERICS.md."""
import contextlib
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import numerics as nm

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float16, torch.bfloat16]
RECORD = None                    # a list while the report is being written: the figures go there and nothing is asserted


def _name(dtype):
    return "fp16" if dtype == torch.float16 else "bf16"


@contextlib.contextmanager
def knobs(_module=None, **kw):
    """set tuning knobs of edgestyle_amd.ops (or of _module) for the duration of a block, restore them whatever happens"""
    from edgestyle_amd import ops
    mod = _module or ops
    old = {k: getattr(mod, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(mod, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(mod, k, v)


class _Rec:
    """the ops.PROFILE hook without in-kernel stamps: sees the descriptor of every GEMM launch (which kernel / tile ran)"""

    def __init__(self):
        self.descs, self.metas = [], []

    def next(self, meta):
        self.metas.append(meta)
        return None


@contextlib.contextmanager
def launches():
    from edgestyle_amd import ops
    rec, old = _Rec(), ops.PROFILE
    ops.PROFILE = rec
    try:
        yield rec
    finally:
        ops.PROFILE = old


def _div(a, b):
    return a / b if b > 0 else float("inf")


def judge(fails, name, y, ref64, e_alg, e_ref, dtype, required=True, assert_ref=True):
    """e_alg None: the case has no base_alg (block-level cases: the bar is base_ref's).  assert_ref False: base_ref is recorded only."""
    e, e_rms = nm.row_err(y, ref64, both=True)
    margin = nm.MARGIN if required else nm.PROBE_MARGIN
    tier = ("required" if required else "probe") if assert_ref or not required else "recorded"
    alg_s = "-" if e_alg is None else f"{e_alg:.3e}"
    print(f"numerics: {name}: kernel {e:.3e} (row-rms {e_rms:.3e})  base_alg {alg_s}  base_ref {e_ref:.3e}  "
          f"kernel/alg {_div(e, e_alg) if e_alg is not None else float('nan'):.2f}  kernel/ref {_div(e, e_ref):.2f}  [{tier}]", flush=True)
    finite = nm.finite_where_representable(y, ref64, dtype)
    if RECORD is not None:
        RECORD.append(dict(case=name, kernel=e, kernel_rms=e_rms, base_alg=e_alg, base_ref=e_ref, tier=tier, finite=finite))
        return
    if not ((e_alg is None or e_alg > 0) and e_ref > 0):
        fails.append(f"{name}: a baseline without error (base_alg {e_alg}, base_ref {e_ref})")
    if not finite:
        fails.append(f"{name}: not finite where the reference is representable")
    if e_alg is not None and not e <= margin * e_alg:
        fails.append(f"{name}: kernel {e:.3e} > {margin} x base_alg {e_alg:.3e}")
    if required and assert_ref and not e <= nm.MARGIN * e_ref:
        fails.append(f"{name}: kernel {e:.3e} > {nm.MARGIN} x base_ref {e_ref:.3e}")


def done(fails):
    assert not fails, f"{len(fails)} bars missed:\n" + "\n".join(fails)


# ----------------------------------------------------------------------------------------------------------------
# 1. LayerNorm folded into the linear layer behind it
# ----------------------------------------------------------------------------------------------------------------
def _ln_variants(ops, M, pw):
    """(name, knobs, form, check(desc)) of every kernel variant that can run this LayerNorm-folded layer"""
    tiled = dict(XS_ENABLED=False, BIG_TILE_256=False, SMALL_TILE=False)
    out = [("tile128|160", tiled, "fold", lambda d: d.bn in (128, 160)),
           ("8waves", dict(tiled, FORCE_WAVES=8), "fold", lambda d: d.bn in (128, 160) and d.waves == 8),
           ("4waves", dict(tiled, FORCE_WAVES=4), "fold", lambda d: d.bn in (128, 160) and d.waves == 4)]
    if not pw.geglu:
        out.append(("tile64", dict(XS_ENABLED=False, FORCE_BN=64), "fold", lambda d: d.bn == 64))
    if pw.kpad == 1280 and pw.rows_padded % 256 == 0:
        out.append(("tile256", dict(XS_ENABLED=False, FORCE_BN=256), "fold", lambda d: d.bn == 256))
    if pw.kpad in (320, 640) and nm.xs_shape_reference(M, pw, 0):
        from edgestyle_amd import lib
        out.append(("linear_xs", dict(XS_ENABLED=True, XS_MIN_M=0), "xs", lambda d: isinstance(d, lib.XsDesc)))
    return out


LN_LAYERS = [  # name, M, C, Cout, geglu, bias
    ("to_qkv", 300, 320, 960, False, False),
    ("geglu", 257, 320, 2560, True, True),
    ("attn2.to_q", 200, 640, 640, False, False),
    ("to_qkv", 1000, 640, 1920, False, False),
    ("geglu", 130, 640, 5120, True, True),
    ("to_qkv", 130, 1280, 3840, False, False),
    ("attn2.to_q", 300, 1280, 1280, False, False),
    ("geglu", 70, 1280, 10240, True, True),
]


def _ln_inputs(C):
    """(ratio, outlier fraction, peak): everything at C = 320, a cross at the wider levels"""
    full = [(r, f, p) for r in nm.REQUIRED_RATIOS + nm.PROBE_RATIOS for f in (0.0, 0.01) for p in (4.0, 2.0e4)]
    if C == 320:
        return full
    return [(0, 0.01, 4.0), (10, 0.0, 2.0e4), (30, 0.01, 2.0e4), (30, 0.0, 4.0), (100, 0.01, 4.0), (300, 0.01, 2.0e4)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("C", [320, 640, 1280])
def test_layer_norm_fold_at_trained_statistics(C, dtype):
    """Linear(LayerNorm(x)) as one launch on the raw x, every kernel variant that can run it (the 128-pixel tile at bn 128 | 160 on 4
    and 8 waves, the 64 x 64 tile, the 256-pixel tile, es_linear_xs at K = 320 | 640), to_q|k|v / attn2.to_q / GEGLU, ragged M,
    |mean| / std 0 .. 30 (required) and 100, 300 (probe), with and without 1 % outlier channels at x50-100, max|x| 4 and 2e4."""
    from edgestyle_amd import ops
    fails = []
    for layer, M, Cc, Cout, geglu, bias in LN_LAYERS:
        if Cc != C:
            continue
        for ratio, frac, peak in _ln_inputs(C):
            required = ratio in nm.REQUIRED_RATIOS
            x = nm.token_rows(M, C, ratio, frac, (50.0, 100.0), peak, dtype, seed=1000 * ratio + int(peak) + M)
            c = nm.ln_case(x, Cout, dtype, geglu=geglu, bias=bias, seed=M + Cout)
            if required:
                assert nm.ln_intermediates_peak(c) < 3.0e4
            ref = nm.ln_ref64(c)
            e_ref = nm.row_err(nm.ln_base_ref(c), ref)
            e_alg = {form: nm.row_err(nm.ln_base_alg(c, form), ref) for form in ("fold", "xs")}
            pw = ops.pack_weight_ln(c["W"], c["b"], c["gamma"], c["beta"], c["eps"], dtype, DEV, geglu=geglu)
            xd = x.to(DEV, dtype)
            for vname, kn, form, ran in _ln_variants(ops, M, pw):
                with knobs(**kn), launches() as rec:
                    y = ops.linear(xd, pw)
                assert len(rec.descs) == 1 and ran(rec.descs[0]), (vname, layer, C)
                judge(fails, f"ln {layer} C={C} M={M} {_name(dtype)} ratio={ratio} outliers={frac} peak={peak:g} {vname}",
                      y, ref, e_alg[form], e_ref, dtype, required)
    done(fails)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_layer_norm_fold_grouped_launch_keeps_statistics_apart(dtype):
    """one grouped launch over [2, 6, 4, 2] x 256 rows with four weight / LayerNorm parameter sets in which ONLY the second group is
    at |mean| / std = 30 (with outlier channels, peak 2e4; the others at 0 and peak 4): every row is judged on its own scale, so a
    statistic or a column sum leaking across a group boundary shows."""
    from edgestyle_amd import ops, lib
    counts = [512, 1536, 1024, 512]
    for C, Cout, geglu in [(320, 960, False), (320, 2560, True), (1280, 2560, True)]:
        fails = []
        cs = []
        for i, n in enumerate(counts):
            x = nm.token_rows(n, C, 30 if i == 1 else 0, 0.01, (50.0, 100.0), 2.0e4 if i == 1 else 4.0, dtype, seed=50 + i)
            cs.append(nm.ln_case(x, Cout, dtype, geglu=geglu, seed=60 + i))
        ref = torch.cat([nm.ln_ref64(c) for c in cs])
        e_ref = nm.row_err(torch.cat([nm.ln_base_ref(c) for c in cs]), ref)
        e_alg = {form: nm.row_err(torch.cat([nm.ln_base_alg(c, form) for c in cs]), ref) for form in ("fold", "xs")}
        pws = [ops.pack_weight_ln(c["W"], c["b"], c["gamma"], c["beta"], c["eps"], dtype, DEV, geglu=geglu) for c in cs]
        xd = torch.cat([c["x"] for c in cs]).to(DEV, dtype)
        variants = [("tile128|160", dict(XS_ENABLED=False, BIG_TILE_256=False, SMALL_TILE=False), "fold", lambda d: d.bn in (128, 160))]
        if C == 1280:
            variants.append(("tile256", dict(XS_ENABLED=False, FORCE_BN=256), "fold", lambda d: d.bn == 256))
        else:
            variants.append(("linear_xs", dict(XS_ENABLED=True, XS_MIN_M=0), "xs", lambda d: isinstance(d, lib.XsDesc)))
        for vname, kn, form, ran in variants:
            with knobs(**kn), launches() as rec:
                y = ops.linear(xd, pws, group_n=counts)
            assert len(rec.descs) == 1 and ran(rec.descs[0]) and rec.descs[0].ngroups == 4
            judge(fails, f"ln grouped [2,6,4,2]x256 C={C} Cout={Cout} {_name(dtype)} {vname}", y, ref, e_alg[form], e_ref, dtype)
        done(fails)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_layer_norm_fold_constant_and_zero_rows(dtype):
    """Rows of zeros and constant rows: variance exactly 0, the clamp of E[x^2] - mean^2 and the rsqrt(eps) path.  The reference
    output of such a row is W beta + b.  A row of zeros is exact in every form (all sums are 0): required tier.  For a constant row
    c the fold computes rsqrt(eps) * (c sum(W') - mean colsum(W')): 316 times the fp32 rounding noise of two sums of c * 14, whose
    size depends on the order of summation - the probe bar (PROBE_MARGIN x base_alg, finite), the ratio to base_ref is printed."""
    from edgestyle_amd import ops
    fails = []
    for C, Cout, geglu, M in [(320, 960, False, 300), (640, 5120, True, 130), (1280, 1280, False, 300)]:
        x = nm.token_rows(M, C, 3, 0.0, peak=4.0, dtype=dtype, seed=C)
        zero_rows, const_rows = [0, 17, M - 1], {5: 3.0, 64: -0.5, M - 2: 4.0}
        c = nm.ln_case(x, Cout, dtype, geglu=geglu, seed=C + 1)
        pw = ops.pack_weight_ln(c["W"], c["b"], c["gamma"], c["beta"], c["eps"], dtype, DEV, geglu=geglu)
        for kind, rows in (("zero", zero_rows), ("constant", list(const_rows))):
            xk = x.clone()
            for r in rows:
                xk[r] = 0.0 if kind == "zero" else const_rows[r]
            ck = dict(c, x=xk)
            ref = nm.ln_ref64(ck)
            e_ref = nm.row_err(nm.ln_base_ref(ck)[rows], ref[rows])
            e_alg = {form: nm.row_err(nm.ln_base_alg(ck, form)[rows], ref[rows]) for form in ("fold", "xs")}
            xd = xk.to(DEV, dtype)
            for vname, kn, form, ran in _ln_variants(ops, M, pw):
                with knobs(**kn), launches() as rec:
                    y = ops.linear(xd, pw)
                assert ran(rec.descs[0])
                judge(fails, f"ln {kind} rows C={C} {_name(dtype)} {vname}", y[rows], ref[rows], e_alg[form], e_ref, dtype,
                      required=kind == "zero")
                if kind == "zero":          # all of a zero row's sums are exactly 0: the same output in every one of them
                    yz = y[rows].float()
                    assert bool((yz == yz[0]).all())
    done(fails)


# ----------------------------------------------------------------------------------------------------------------
# 2. GroupNorm
# ----------------------------------------------------------------------------------------------------------------
def _split(x, C1):
    """the first C1 channels and the rest as two contiguous device tensors (the concatenated second source)"""
    return x[..., :C1].contiguous(), x[..., C1:].contiguous()


GN_SHAPES = [  # C, H, C1 (first source; C = one source), N, counts
    (320, 64, 320, 2, None), (640, 32, 640, 2, None), (1280, 16, 1280, 16, None), (2560, 8, 1280, 16, None),
    (1920, 32, 1280, 2, None), (960, 64, 640, 2, None), (320, 32, 320, 14, [2, 6, 4, 2]), (1280, 8, 1280, 14, [2, 6, 4, 2]),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("C,H,C1,N,counts", GN_SHAPES)
def test_group_norm_at_trained_statistics(C, H, C1, N, counts, dtype):
    """es_group_norm, the one-launch slab form and the statistics + apply form (which of the two runs is the library's rule:
    es_group_norm_is_slab, printed), with and without SiLU, with the concatenated second source, grouped [2, 6, 4, 2]: per
    (sample, group) |mean| / std of 0 .. 30 with 1 % outlier channels at x50-100 and peak 2e3, plus a group whose variance is one
    channel's."""
    from edgestyle_amd import ops, lib
    fails = []
    slab = bool(lib.load().es_group_norm_is_slab(H * H, C, 32))
    for ratio, dom in [(0, False), (3, False), (10, False), (30, False), (30, True)]:
        if N > 2 and ratio in (3, 10):
            continue
        x = nm.group_maps(N, C, H, 32, ratio, 0.0 if dom else 0.01, (50.0, 100.0), 4.0 if dom else 2.0e3, dtype, seed=C + H + ratio,
                          dominant_channel=dom)
        for silu in (True, False):
            c = nm.gn_case(x, 32, dtype, silu=silu, seed=C + H, ngroups=len(counts) if counts else 1)
            assert nm.gn_intermediates_peak(c, counts) < 3.0e4
            ref = nm.gn_ref64(c, counts)
            e_ref, e_alg = nm.row_err(nm.gn_base_ref(c, counts), ref), nm.row_err(nm.gn_base_alg(c, counts), ref)
            xd = x.to(DEV, dtype)
            x1, x2 = (xd, None) if C1 == C else _split(xd, C1)
            gam, bet = [t.to(DEV) for t in c["gamma"]], [t.to(DEV) for t in c["beta"]]
            if counts:
                y = ops.group_norm(x1, gam, bet, 32, c["eps"], silu, x2=x2, group_n=counts)
            else:
                y = ops.group_norm(x1, gam[0], bet[0], 32, c["eps"], silu, x2=x2)
            judge(fails, f"gn C={C1}+{C - C1} H={H} N={N}{' grouped' if counts else ''} {_name(dtype)} ratio={ratio}"
                         f"{' one-channel groups' if dom else ''} silu={int(silu)} {'slab' if slab else 'stats+apply'}",
                  y, ref, e_alg, e_ref, dtype)
    done(fails)


@pytest.mark.parametrize("C,H", [(128, 256), (512, 64)])
def test_group_norm_vae_sizes(C, H):
    """the VAE decoder's GroupNorms (eps 1e-6, SiLU) in fp16, one sample"""
    from edgestyle_amd import ops
    fails, dtype = [], torch.float16
    for ratio in (0, 30):
        x = nm.group_maps(1, C, H, 32, ratio, 0.01, (50.0, 100.0), 2.0e3, dtype, seed=C + ratio)
        c = nm.gn_case(x, 32, dtype, silu=True, eps=1e-6, seed=C)
        ref = nm.gn_ref64(c)
        e_ref, e_alg = nm.row_err(nm.gn_base_ref(c), ref), nm.row_err(nm.gn_base_alg(c), ref)
        y = ops.group_norm(x.to(DEV, dtype), c["gamma"][0].to(DEV), c["beta"][0].to(DEV), 32, 1e-6, True)
        judge(fails, f"gn vae C={C} H={H} fp16 ratio={ratio}", y, ref, e_alg, e_ref, dtype)
    done(fails)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("C,H,N,G,counts", [(320, 64, 2, 32, None), (320, 32, 14, 32, [2, 6, 4, 2]), (320, 64, 2, 1, None), (320, 64, 2, 5, None),
                                            (640, 64, 8, 32, None), (640, 64, 8, 1, None), (640, 64, 8, 2, None)])
def test_group_norm_in_front_of_proj_in_at_trained_statistics(C, H, N, G, counts, dtype):
    """ops.gn_proj_in, fused (es_group_norm stats_only + es_linear_xs normalising the rows it holds) and as two launches + the
    projection, for every GroupNorm group count class the fused kernel's channel -> group map has to get right (32; 1, 2, 5: groups
    of 640, 320, 64 channels)."""
    from edgestyle_amd import ops, lib
    fails = []
    if counts and N * H * H < 8192:
        counts = [4 * n for n in counts]
        N = sum(counts)
    for ratio in ((0, 30) if C == 640 else nm.REQUIRED_RATIOS):
        x = nm.group_maps(N, C, H, G, ratio, 0.01, (50.0, 100.0), 2.0e3, dtype, seed=C + G + ratio)
        c = nm.gn_case(x, G, dtype, eps=1e-6, seed=C + G, Cout=C, ngroups=len(counts) if counts else 1)
        assert nm.gn_intermediates_peak(c, counts) < 3.0e4
        ref = nm.gn_ref64(c, counts)
        e_ref, e_alg = nm.row_err(nm.gn_base_ref(c, counts), ref), nm.row_err(nm.gn_base_alg(c, counts), ref)
        pws = [ops.pack_weight(w[:, :, None, None], b, dtype, DEV) for w, b in zip(c["W"], c["b"])]
        gam, bet = [t.to(DEV) for t in c["gamma"]], [t.to(DEV) for t in c["beta"]]
        xd = x.to(DEV, dtype)
        assert ops.gn_fold_ok(N * H * H, H * H, G, pws[0], pws if counts else None, counts)
        for fused in (True, False):
            with knobs(GN_FOLD=fused), launches() as rec:
                if counts:
                    y = ops.gn_proj_in(xd, gam, bet, G, 1e-6, pws, group_n=counts)
                else:
                    y = ops.gn_proj_in(xd, gam[0], bet[0], G, 1e-6, pws[0])
            if fused:
                assert len(rec.descs) == 1 and isinstance(rec.descs[0], lib.XsDesc) and rec.descs[0].gn_part
            else:
                assert not any(isinstance(d, lib.XsDesc) and d.gn_part for d in rec.descs)
            judge(fails, f"gn->proj_in C={C} G={G} N={N}{' grouped' if counts else ''} {_name(dtype)} ratio={ratio} "
                         f"{'fused' if fused else 'two launches'}", y, ref, e_alg, e_ref, dtype)
    done(fails)


@pytest.mark.parametrize("N,H,C,bn,splitk", [(2, 64, 320, 160, None), (2, 16, 640, 128, None), (1, 8, 1280, 64, None), (2, 64, 320, 160, 3)])
def test_group_norm_statistics_from_the_producer_at_trained_statistics(N, H, C, bn, splitk):
    """The hand-over (gn_groups= on ops.conv_gemm): the statistics are sums of the producer's fp32 ACCUMULATORS while the GroupNorm
    normalises the ROUNDED values.  The producer is a 3x3 convolution whose output has |mean| / std = 30 per (sample, group) (an
    identity centre tap plus noise on a group_maps input; the ratio of the actual output is asserted); the truth is the fp64
    GroupNorm of that ROUNDED output, base_alg takes its statistics from the fp32 convolution."""
    from edgestyle_amd import ops
    import torch.nn.functional as F
    fails, dtype = [], torch.float16
    for ratio in (0, 30):
        x = nm.group_maps(N, C, H, 32, ratio, 0.01, (50.0, 100.0), 2.0e3, dtype, seed=C + ratio)
        g = torch.Generator().manual_seed(C)
        w = 0.005 * torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)
        w[:, :, 1, 1] += torch.eye(C)
        w = nm.rnd(w, dtype)
        b = 0.01 * torch.randn(C, generator=g)
        pw = ops.pack_weight(w, b, dtype, DEV)
        xd = x.to(DEV, dtype)
        with knobs(FORCE_BN=bn, GN_HANDOVER_ALL=True, GN_HANDOVER=True):
            y0 = ops.conv_gemm(xd, pw, splitk=splitk)
            y1 = ops.conv_gemm(xd, pw, splitk=splitk, gn_groups=32)
            assert torch.equal(y0, y1) and hasattr(y1, "_gnp") and not hasattr(y0, "_gnp")
            c = nm.gn_case(y1.float().cpu(), 32, dtype, silu=True, seed=C)
            n0 = ops.group_norm(y0, c["gamma"][0].to(DEV), c["beta"][0].to(DEV), 32, 1e-5, True)
            n1 = ops.group_norm(y1, c["gamma"][0].to(DEV), c["beta"][0].to(DEV), 32, 1e-5, True)
        yc = c["x"].double().reshape(N, H * H, 32, C // 32)
        got_ratio = yc.mean(dim=(1, 3)).abs() / yc.std(dim=(1, 3), unbiased=False)
        assert ratio == 0 or (float(got_ratio.min()) > 0.8 * ratio and float(got_ratio.max()) < 1.2 * ratio), (float(got_ratio.min()), float(got_ratio.max()))
        acc32 = (F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=1)).permute(0, 2, 3, 1).contiguous()       # the fp32 accumulators
        ref = nm.gn_ref64(c)
        e_ref = nm.row_err(nm.gn_base_ref(c), ref)
        e_own, e_hand = nm.row_err(nm.gn_base_alg(c), ref), nm.row_err(nm.gn_base_alg(c, stats_from=acc32), ref)
        tag = f"C={C} H={H} bn={bn} splitk={splitk} fp16 ratio={ratio}"
        judge(fails, f"gn own statistics {tag}", n0, ref, e_own, e_ref, dtype)
        judge(fails, f"gn statistics handed over {tag}", n1, ref, e_hand, e_ref, dtype)
    done(fails)


# ----------------------------------------------------------------------------------------------------------------
# 3. attention
# ----------------------------------------------------------------------------------------------------------------
def _attn_cases(d, dtype, kvres=False):
    """name -> (q, k, v, heads) for one head width"""
    heads = 1 if d == 512 else 2
    Sq = 64 if d == 512 else 256
    if kvres:           # K / V resident in registers, a single pass over <= 96 keys: no sea (Skv >= 1024), no tiles to rise over
        return {
            "shift+300": nm.common_shift(2, heads, Sq, 77, d, 300.0, dtype, seed=d + 1) + (heads,),
            "shift-300": nm.common_shift(2, heads, Sq, 96, d, -300.0, dtype, seed=d + 2) + (heads,),
            "one_loud_query": nm.one_loud_query(2, heads, Sq, 77, d, wave=32, dtype=dtype, seed=d + 3) + (heads,),
            "loud_values_2e4": nm.loud_values(2, heads, Sq, 77, d, 2.0e4, dtype, seed=d + 4) + (heads,),
        }
    out = {"sea_1024_15": nm.spike_and_sea(1, heads, Sq, 1024, d, 15, dtype, seed=d + 5) + (heads,)}
    if d == 40:
        out["sea_4096_15"] = nm.spike_and_sea(1, heads, Sq, 4096, d, 15, dtype, seed=d + 6) + (heads,)
        out["sea_4096_17"] = nm.spike_and_sea(1, heads, Sq, 4096, d, 17, dtype, seed=d + 7) + (heads,)
        out["control_4096_20"] = nm.spike_and_sea(1, heads, Sq, 4096, d, 20, dtype, seed=d + 8, control=True) + (heads,)
    out["late_risers"] = nm.late_risers(1, heads, Sq, 512, d, dtype=dtype, seed=d + 9) + (heads,)
    out["shift+300"] = nm.common_shift(1, heads, Sq, 256, d, 300.0, dtype, seed=d + 10) + (heads,)
    out["shift-300"] = nm.common_shift(1, heads, Sq, 320, d, -300.0, dtype, seed=d + 11) + (heads,)
    out["one_loud_query_32"] = nm.one_loud_query(1, heads, Sq, 512, d, wave=32, dtype=dtype, seed=d + 12) + (heads,)
    out["one_loud_query_64"] = nm.one_loud_query(1, heads, Sq, 512, d, wave=64, dtype=dtype, seed=d + 13) + (heads,)
    out["loud_values_2e4"] = nm.loud_values(1, heads, Sq, 256, d, 2.0e4, dtype, seed=d + 14) + (heads,)
    return out


# kernel -> (environment of the child process - the dispatcher's switches are read once per process -, head widths, kvres setting)
ATTN_KERNEL_ID = dict(generic=1, generic_32q=2, tile32=3, tile32_2blocks=4, attention40pp_32q=5, attention40pp_64q=6, kv_resident=7)   # es_attention_last_kernel
ATTN_KERNELS = {
    "generic": (dict(ES_ATTN32="0"), (40, 80, 160, 512), 0),                                   # 16 queries per wave
    "generic_32q": (dict(ES_ATTN32="0", ES_ATTN_BIG="1"), (40, 80), 0),                        # 32 queries per wave
    "tile32": (dict(ES_ATTN32="2", ES_ATTN_BIG="1", ES_ATTN_PP="0", ES_ATTN_QB="1"), (40, 80), 0),
    "tile32_2blocks": (dict(ES_ATTN32="1", ES_ATTN_BIG="1", ES_ATTN_PP="0"), (40,), 0),
    "attention40pp_32q": (dict(ES_ATTN_BIG="1", ES_ATTN_PP="1"), (40,), 0),
    "attention40pp_64q": (dict(ES_ATTN_BIG="1", ES_ATTN_PP="2"), (40,), 0),
    "kv_resident": ({}, (40, 80), 2),
}


def attention_child(argv):
    """python -m tests.numerics --attn-child IN OUT KVRES: run every (q, k, v, heads) of IN through ops.attention"""
    from edgestyle_amd import ops, lib
    src, dst, kvres = argv[0], argv[1], int(argv[2])
    cases = torch.load(src, weights_only=True)
    L = lib.load()
    prev = L.es_attention_set_kvres(kvres)
    outs = {}
    try:
        for name, (q, k, v, heads, bf) in cases.items():
            dt = torch.bfloat16 if bf else torch.float16
            outs[name] = ops.attention(q.to(DEV, dt), k.to(DEV, dt), v.to(DEV, dt), heads).cpu()
            outs[name + " #kernel"] = torch.tensor(L.es_attention_last_kernel())
        torch.cuda.synchronize()
    finally:
        L.es_attention_set_kvres(prev)
    torch.save(outs, dst)


@pytest.mark.parametrize("kernel", list(ATTN_KERNELS))
def test_attention_at_trained_statistics(kernel, tmp_path):
    """Every kernel the dispatcher can pick (selected the way it selects: its switches, in a child process because they are read
    once), fp16 and bf16: a spike over a sea of keys whose P is below the fp16 normal range (does the conversion and the matrix core
    keep subnormal P?), maxima that rise tile after tile, all logits shifted by +-300, one loud query per wave, V at 2e4."""
    env, widths, kvres = ATTN_KERNELS[kernel]
    cases = {}
    for dtype in DTYPES:
        for d in widths:
            for name, (q, k, v, heads) in _attn_cases(d, dtype, kvres=kvres == 2).items():
                if "40pp" in kernel and k.shape[1] % 64:
                    continue
                cases[f"{name} d={d} {_name(dtype)}"] = (q, k, v, heads, dtype == torch.bfloat16)
    src, dst = str(tmp_path / "in.pt"), str(tmp_path / "out.pt")
    torch.save(cases, src)
    r = subprocess.run([sys.executable, "-m", "tests.numerics", "--attn-child", src, dst, str(kvres)], cwd=ROOT,
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    if r.returncode in (134, 139, 124, 137, -6, -11, -9):      # the child died on the GPU: nothing more is started on it in this session
        pytest.exit(f"attention child ({kernel}) ended with status {r.returncode}:\n" + r.stdout[-2000:] + r.stderr[-2000:], returncode=3)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    outs = torch.load(dst, weights_only=True)
    fails = []
    ran = {name: int(outs[name + " #kernel"]) for name in cases}
    assert set(ran.values()) == {ATTN_KERNEL_ID[kernel]}, (kernel, {n: i for n, i in ran.items() if i != ATTN_KERNEL_ID[kernel]})
    for name, (q, k, v, heads, bf) in cases.items():
        dtype = torch.bfloat16 if bf else torch.float16
        ref = nm.attn_ref64(q, k, v, heads)
        assert float(ref.abs().max()) < 3.0e4
        e_ref = nm.row_err(nm.attn_base_ref(q, k, v, heads, dtype), ref)
        e_alg = nm.attn_design_err(q, k, v, heads, dtype, ref)
        judge(fails, f"attention {kernel} {name}", outs[name], ref, e_alg, e_ref, dtype)
    done(fails)


# ----------------------------------------------------------------------------------------------------------------
# 4. one Transformer2DModel at full width: the ff.net.2 || proj_out fold and the wide residual stream under outlier channels
# ----------------------------------------------------------------------------------------------------------------
def _transformer_weights(C, dtype, seed):
    p, tb, D = "attentions.0", "attentions.0.transformer_blocks.0", 768
    shapes = {f"{p}.norm.weight": (C,), f"{p}.norm.bias": (C,), f"{p}.proj_in.weight": (C, C, 1, 1), f"{p}.proj_in.bias": (C,),
              f"{p}.proj_out.weight": (C, C, 1, 1), f"{p}.proj_out.bias": (C,)}
    for i in (1, 2, 3):
        shapes[f"{tb}.norm{i}.weight"] = (C,)
        shapes[f"{tb}.norm{i}.bias"] = (C,)
    for a, kin in (("attn1", C), ("attn2", D)):
        shapes[f"{tb}.{a}.to_q.weight"] = (C, C)
        shapes[f"{tb}.{a}.to_k.weight"] = (C, kin)
        shapes[f"{tb}.{a}.to_v.weight"] = (C, kin)
        shapes[f"{tb}.{a}.to_out.0.weight"] = (C, C)
        shapes[f"{tb}.{a}.to_out.0.bias"] = (C,)
    shapes[f"{tb}.ff.net.0.proj.weight"] = (8 * C, C)
    shapes[f"{tb}.ff.net.0.proj.bias"] = (8 * C,)
    shapes[f"{tb}.ff.net.2.weight"] = (C, 4 * C)
    shapes[f"{tb}.ff.net.2.bias"] = (C,)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in shapes.items():
        if "norm" in k and k.endswith(".weight"):
            t = 1 + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith(".bias"):
            t = 0.05 * torch.randn(shp, generator=g)
        else:
            t = torch.randn(shp, generator=g) / (shp[1] ** 0.5)
        sd[k] = nm.rnd(t, dtype)
    return sd, p, D


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("ffo", [True, False], ids=["ffo_fold", "two_launches"])
@pytest.mark.parametrize("C,heads,H", [(320, 8, 32), (1280, 8, 8)])
def test_transformer_block_with_outlier_channels(C, heads, H, ffo, dtype):
    """engine.Transformer at SD1.5 widths on an input with 1 % outlier channels at x50 and max|x| = 2e3, with ff.net.2 and proj_out as
    one GEMM (engine.FFO_FOLD) and as two launches; in bf16 the block adds into the two-word residual stream (the output is hi + lo).
    Truth: the oracle's block in fp64 (its functions take double tensors) on the rounded weights; base_ref: the oracle's block in fp32,
    the output rounded once.  There is no base_alg for a whole block: the bar is kernel <= MARGIN * base_ref - the block's output is x
    plus a correction of O(1), so against a row's rms (set by its outlier channels) the rounding of the final sum is what both carry,
    and a fold or a residual path that loses more than that shows."""
    from oracle import sd15_oracle as O
    from edgestyle_amd import engine as E, ops
    fails, N = [], 2
    sd, p, D = _transformer_weights(C, dtype, seed=C)
    x = nm.token_rows(N * H * H, C, 3, 0.01, 50.0, 2.0e3, dtype, seed=C + 1).reshape(N, H, H, C)
    ehs = nm.rnd(0.5 * torch.randn(N, 77, D, generator=torch.Generator().manual_seed(C + 2)), dtype)
    xc = x.permute(0, 3, 1, 2).contiguous()
    ref = O.transformer({k: v.double() for k, v in sd.items()}, p, xc.double(), ehs.double(), heads, 32).permute(0, 2, 3, 1)
    assert float(ref.abs().max()) < 3.0e4
    e_ref = nm.row_err(nm.rnd(O.transformer(sd, p, xc, ehs, heads, 32), dtype).permute(0, 2, 3, 1), ref)
    with knobs(E, FFO_FOLD=ffo):
        blk = E.Transformer(E._Packer(sd, dtype, DEV), p, heads, 32)
    assert (blk.ffo is not None) == ffo and blk.ln_fold
    out = blk(x.to(DEV, dtype), blk.context(ehs.to(DEV, dtype)))
    lo = getattr(out, "_lo", None)
    assert (lo is not None) == ops.wide_stream(dtype)
    y = out.float() if lo is None else out.float() + lo.float()
    judge(fails, f"transformer C={C} H={H} {_name(dtype)} {'ffo fold' if ffo else 'ff.net.2, proj_out apart'}"
                 f"{' wide stream' if lo is not None else ''}", y, ref, None, e_ref, dtype)
    done(fails)


# ----------------------------------------------------------------------------------------------------------------
# 5. one VAE-decoder up block in fp16 close to the top of the format's range
# ----------------------------------------------------------------------------------------------------------------
def test_vae_up_block_near_the_fp16_range():
    """decoder.up_blocks.0 of the SD VAE (three ResnetBlock2D at 512 channels, 64 x 64, eps 1e-6, then nearest 2x upsampling + conv to
    128 x 128) in fp16, the input scaled so that the LARGEST tensor the fp64 reference stores is 2.8e4 .. 3e4: finite output, both bars
    (base_ref: fp32 ops with every output rounded to fp16; base_alg: the engine's launches - one-pass GroupNorm + SiLU rounded once,
    convolution + residual rounded once).  The reference runs its VAE in fp32: the ratio to an fp32 block, output rounded once, is
    recorded."""
    from edgestyle_amd import engine as E, ops
    fails, dtype, p, C, H, G, eps = [], torch.float16, "decoder.up_blocks.0", 512, 64, 32, 1e-6
    g = torch.Generator().manual_seed(5)
    sd = {}
    for j in range(3):
        for n in ("norm1", "norm2"):
            sd[f"{p}.resnets.{j}.{n}.weight"] = nm.rnd(1 + 0.1 * torch.randn(C, generator=g), dtype)
            sd[f"{p}.resnets.{j}.{n}.bias"] = nm.rnd(0.05 * torch.randn(C, generator=g), dtype)
        for n in ("conv1", "conv2"):
            sd[f"{p}.resnets.{j}.{n}.weight"] = nm.rnd(torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C), dtype)
            sd[f"{p}.resnets.{j}.{n}.bias"] = nm.rnd(0.05 * torch.randn(C, generator=g), dtype)
    sd[f"{p}.upsamplers.0.conv.weight"] = nm.rnd(torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C), dtype)
    sd[f"{p}.upsamplers.0.conv.bias"] = nm.rnd(0.05 * torch.randn(C, generator=g), dtype)
    peak = 2.9e4
    for _ in range(2):                       # the residual stream carries x through the block: the largest intermediate is ~linear in peak
        x = nm.group_maps(1, C, H, G, 3, 0.01, (50.0, 100.0), peak, dtype, seed=7)
        pk = []
        nm.vae_up_block(sd, p, x.permute(0, 3, 1, 2), G, eps, "fp32", dtype, peaks=pk)
        if 2.85e4 <= max(pk) <= 2.95e4:
            break
        peak *= 2.9e4 / max(pk)
    xc = x.permute(0, 3, 1, 2).contiguous()
    pk = []
    ref = nm.vae_up_block(sd, p, xc, G, eps, "ref64", peaks=pk).permute(0, 2, 3, 1)
    assert 2.8e4 <= max(pk) <= 3.0e4, max(pk)
    e_ref = nm.row_err(nm.vae_up_block(sd, p, xc, G, eps, "ref", dtype).permute(0, 2, 3, 1), ref)
    e_alg = nm.row_err(nm.vae_up_block(sd, p, xc, G, eps, "alg", dtype).permute(0, 2, 3, 1), ref)
    e_f32 = nm.row_err(nm.vae_up_block(sd, p, xc, G, eps, "fp32", dtype).permute(0, 2, 3, 1), ref)
    pkr = E._Packer(sd, dtype, DEV)
    rs = [E.Resnet(pkr, f"{p}.resnets.{j}", G, eps, None) for j in range(3)]
    us = pkr.conv(f"{p}.upsamplers.0.conv")
    h = x.to(DEV, dtype)
    for r in rs:
        h = r(h, None)
    y = ops.conv_gemm(h, us, upsample=True)
    assert bool(torch.isfinite(y).all())
    judge(fails, "vae up block 512ch 64->128 fp16, largest fp64 intermediate %.3g" % max(pk), y, ref, e_alg, e_ref, dtype)
    judge(fails, "vae up block 512ch 64->128 fp16 against the fp32 block", y, ref, None, e_f32, dtype, assert_ref=False)
    done(fails)


# ----------------------------------------------------------------------------------------------------------------
# report
# ----------------------------------------------------------------------------------------------------------------
CONV_MARKER = "<!-- convolution table: everything below this line is written by `python -m tests.numerics --report` -->"


def _write_conv_table(f, conv_rows):
    """the convolution sweep's rows (tests/test_conv_gpu.py): the misrounded share beside the row_err bars"""
    f.write("\n" + CONV_MARKER + "\n\n")
    f.write(f"Convolution sweep, measured on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {len(conv_rows)} launches judged.  "
            "`differs`: elements that differ from the correctly rounded fp64 result (forms with a residual: from `base_alg`); the bar is "
            "2 x the largest baseline count, 100 elements where that is under 50.  The device library's unfold + mm was among the baselines "
            f"of {sum('device' in r['counts'] for r in conv_rows)} of them.\n\n")
    f.write("| case | elements | kernel differs | share | alg32 | torch32 | device mm | alg8 | bar | kernel / base_alg | kernel / base_ref |\n")
    f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
    for r in conv_rows:
        n = r["numel"]
        pct = lambda k: "-" if k not in r["counts"] else f"{r['counts'][k] / n:.3%}"
        f.write(f"| {r['case']} | {n} | {r['kernel']} | {r['kernel'] / n:.3%} | {pct('alg32')} | {pct('torch32')} | {pct('device')} | {pct('alg8')} | "
                f"{r['bar']} | {_div(r['kernel_err'], r['base_alg']):.2f} | {_div(r['kernel_err'], r['base_ref']):.2f} |\n")


FUSION_MARKERS = ("<!-- fusion table begin: written by `python -m tests.numerics --report --only fusion` -->", "<!-- fusion table end -->")
SAMPLER_MARKERS = ("<!-- sampler table begin: written by `python -m tests.numerics --report --only sampler` -->", "<!-- sampler table end -->")


def _replace_between(text, markers, body):
    begin, end = markers
    assert begin in text and end in text, f"tests/NUMERICS.md has lost its marker lines {markers}"
    return text[:text.index(begin) + len(begin)] + "\n\n" + body.rstrip("\n") + "\n\n" + text[text.index(end):]


def _fusion_section():
    from tests import test_fusion_gpu as FG
    rows, secs = FG.report_rows()
    out = [f"Fusion sweep, measured on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {len(rows)} launches judged in {secs:.1f} s "
           "(CPU baselines included).  Error per sample: max|y - ref64| / rms(ref64) over the sample.", "",
           "| case | tier | kernel | base_alg | base_ref | kernel / base_alg | kernel / base_ref | old metric |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['case']} | {r['tier']} | {r['kernel']:.2e} | {r['base_alg']:.2e} | {r['base_ref']:.2e} | {_div(r['kernel'], r['base_alg']):.2f} | "
                   f"{_div(r['kernel'], r['base_ref']):.2f} | {r['old_metric']:.1e} |")
    return "\n".join(out), len(rows)


def _sampler_section():
    from tests import test_sampler_gpu as SG
    rows, secs = SG.report_rows()
    out = [f"Sampler trajectories, measured on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {len(rows)} trajectories in {secs:.1f} s.  "
           "Per trajectory the step at which kernel / base_alg of the fp32 latents is largest; error: max|x - ref64| / rms(ref64).", "",
           "| trajectory | step | kernel | base_alg | kernel / base_alg |", "|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['case']} | {r.get('step')} | {r['kernel']:.2e} | {r['base_alg']:.2e} | {r['ratio']:.2f} |")
    return "\n".join(out), len(rows)


ATTENTION_MARKERS = ("<!-- attention table begin: written by `python -m tests.numerics --report --only attention` -->", "<!-- attention table end -->")


def _attention_section():
    from tests import test_attention_gpu as AG
    rows, secs, cpu = AG.report_rows()
    out = [f"Attention at ragged lengths, measured on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {len(rows)} rows (three launches each) in "
           f"{sum(secs.values()):.1f} s, of which CPU baselines {cpu:.2f} s; per variant: " + ", ".join(f"{v} {s:.1f} s" for v, s in secs.items()) + ".  "
           "`views`: the outputs through NaN- and huge-poisoned views equal the dense launch's bit for bit; `guards`: every guard element kept its NaN "
           "bits and the view holds no NaN.  One key: the output is v[:, 0] bit for bit (kernel error 0, no baselines).", "",
           "| case | kernel ids | kernel | base_alg | base_ref | kernel / base_alg | kernel / base_ref | views | guards |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if r["base_alg"] is None:
            num = f"{r['kernel']:.2e} | - | - | - | -"
        else:
            num = f"{r['kernel']:.2e} | {r['base_alg']:.2e} | {r['base_ref']:.2e} | {_div(r['kernel'], r['base_alg']):.2f} | {_div(r['kernel'], r['base_ref']):.2f}"
        out.append(f"| {r['case']} | {','.join(str(i) for i in r['ids'])} | {num} | {'equal' if r['same'] else 'DIFFER'} | {'intact' if r['guards'] else 'BROKEN'} |")
    return "\n".join(out), len(rows)


NORM_MARKERS = ("<!-- norm table begin: written by `python -m tests.numerics --report --only norm` -->", "<!-- norm table end -->")


def _norm_section():
    from tests import test_norm_gpu as NG
    rows, secs = NG.report_rows()
    out = [f"GroupNorm and LayerNorm on every route, measured on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {len(rows)} rows (five launches and "
           f"more each, guarded operands) in {secs:.1f} s, CPU baselines included.  Error per row (pixel or token): max|y - ref64| / rms(ref64).", "",
           "| case | route | kernel | base_alg | base_ref | kernel / base_alg | kernel / base_ref | old metric |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['case']} | {r['route']} | {r['kernel']:.2e} | {r['base_alg']:.2e} | {r['base_ref']:.2e} | {_div(r['kernel'], r['base_alg']):.2f} | "
                   f"{_div(r['kernel'], r['base_ref']):.2f} | {r['old_metric']:.1e} |")
    return "\n".join(out), len(rows)


XS_MARKERS = ("<!-- xs table begin: written by `python -m tests.numerics --report --only xs` -->", "<!-- xs table end -->")


def _xs_section():
    from tests import test_linear_xs_gpu as XG
    rows, secs = XG.report_rows()
    out = [f"es_linear_xs in every form, measured on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {len(rows)} rows (four or five launches each: dense, "
           f"guarded views, dense again, the other ping-pong setting) in {secs:.1f} s, CPU baselines included.  Error per row: max|y - ref64| / rms(ref64).  "
           "`differs`: elements that differ from the correctly rounded fp64 result (plain and GEGLU rows) or from `base_alg` (residual rows), and the bar.", "",
           "| case | form | kernel | base_alg | base_ref | kernel / base_alg | kernel / base_ref | differs / bar (elements) | old metric |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        share = "-" if r["differs"] is None else f"{r['differs']} / {r['bar']} ({r['numel']})"
        out.append(f"| {r['case']} | {r['form']} | {r['kernel']:.2e} | {r['base_alg']:.2e} | {r['base_ref']:.2e} | {_div(r['kernel'], r['base_alg']):.2f} | "
                   f"{_div(r['kernel'], r['base_ref']):.2f} | {share} | {r['old_metric']:.1e} |")
    return "\n".join(out), len(rows)


_SECTIONS = {"fusion": (_fusion_section, FUSION_MARKERS), "sampler": (_sampler_section, SAMPLER_MARKERS), "attention": (_attention_section, ATTENTION_MARKERS),
             "norm": (_norm_section, NORM_MARKERS), "xs": (_xs_section, XS_MARKERS)}


def _write_sections(doc, path, which):
    text = open(doc).read()
    for name in which:
        section, markers = _SECTIONS[name]
        body, n = section()
        text = _replace_between(text, markers, body)
        print(f"{n} {name} cases -> {path}")
    with open(path, "w") as f:
        f.write(text)


def write_report(path=None, only=None):
    """python -m tests.numerics --report [--only conv | fusion | sampler | attention | norm | xs]: run every case above and the convolution sweep of
    tests/test_conv_gpu.py without asserting and write the measured tables (--only conv: the convolution table alone, the other is kept
    as it is; --only fusion, --only sampler, --only attention, --only norm, --only xs: the table of tests/test_fusion_gpu.py,
    tests/test_sampler_gpu.py, tests/test_attention_gpu.py, tests/test_norm_gpu.py or tests/test_linear_xs_gpu.py alone, between its marker lines)"""
    global RECORD
    import tempfile
    import pathlib
    assert torch.cuda.is_available(), "the report is measured on the GPU"
    doc = os.path.join(ROOT, "tests", "NUMERICS.md")
    RECORD = []
    if only in _SECTIONS:                                    # their tables sit between marker lines of their own, above the first measured table
        try:
            _write_sections(doc, path or doc, [only])
        finally:
            RECORD = None
        return
    if only == "conv":
        from tests import test_conv_gpu as CV
        conv_rows = CV.report_rows()
        RECORD = None
        text = open(doc).read().split(CONV_MARKER)[0].rstrip("\n") + "\n"
        path = path or doc
        with open(path, "w") as f:
            f.write(text)
            _write_conv_table(f, conv_rows)
        print(f"{len(conv_rows)} convolution launches -> {path}")
        return
    for C in (320, 640, 1280):
        for dt in DTYPES:
            test_layer_norm_fold_at_trained_statistics(C, dt)
    for dt in DTYPES:
        test_layer_norm_fold_grouped_launch_keeps_statistics_apart(dt)
        test_layer_norm_fold_constant_and_zero_rows(dt)
        for shape in GN_SHAPES:
            test_group_norm_at_trained_statistics(*shape, dt)
        for args in [(320, 64, 2, 32, None), (320, 32, 14, 32, [2, 6, 4, 2]), (320, 64, 2, 1, None), (320, 64, 2, 5, None),
                     (640, 64, 8, 32, None), (640, 64, 8, 1, None), (640, 64, 8, 2, None)]:
            test_group_norm_in_front_of_proj_in_at_trained_statistics(*args, dt)
    for C, H in [(128, 256), (512, 64)]:
        test_group_norm_vae_sizes(C, H)
    for args in [(2, 64, 320, 160, None), (2, 16, 640, 128, None), (1, 8, 1280, 64, None), (2, 64, 320, 160, 3)]:
        test_group_norm_statistics_from_the_producer_at_trained_statistics(*args)
    for kernel in ATTN_KERNELS:
        with tempfile.TemporaryDirectory() as t:
            test_attention_at_trained_statistics(kernel, pathlib.Path(t))
    for C, heads, H in [(320, 8, 32), (1280, 8, 8)]:
        for ffo in (True, False):
            for dt in DTYPES:
                test_transformer_block_with_outlier_channels(C, heads, H, ffo, dt)
    test_vae_up_block_near_the_fp16_range()
    rows = list(RECORD)
    from tests import test_conv_gpu as CV
    conv_rows = CV.report_rows()
    RECORD = None
    marker = "<!-- measured table: everything below this line is written by `python -m tests.numerics --report` -->"
    head = open(doc).read().split(marker)[0] if os.path.exists(doc) else "# Numerics at trained-model statistics\n\n"
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    path = path or doc
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(head + marker + "\n\n")
        f.write(f"Measured on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, on top of commit {commit}; {len(rows)} cases.\n\n")
        f.write("| case | tier | kernel | row-rms | base_alg | base_ref | kernel / base_alg | kernel / base_ref | finite |\n")
        f.write("|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            alg = r["base_alg"]
            f.write(f"| {r['case']} | {r['tier']} | {r['kernel']:.2e} | {r['kernel_rms']:.2e} | {'-' if alg is None else format(alg, '.2e')} | "
                    f"{r['base_ref']:.2e} | {'-' if alg is None else format(_div(r['kernel'], alg), '.2f')} | {_div(r['kernel'], r['base_ref']):.2f} | "
                    f"{'yes' if r['finite'] else 'NO'} |\n")
        _write_conv_table(f, conv_rows)
    print(f"{len(rows)} cases, {len(conv_rows)} convolution launches -> {path}")

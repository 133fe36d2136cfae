"""es_conv_gemm (csrc/gemm_conv.hip, the 256 x 320 tile of csrc/gemm_conv8p.hip) on odd geometries, judged by the misrounded share
(tests/numerics.py): every launch writes into a slice cut from the middle of a NaN-filled buffer, the guard rows around the slice must
stay NaN and the slice must hold none; the kernel that ran is read from es_conv_gemm_last_kernel (the launcher's own template arguments)
and must be the tile the row names, with its ring depth, waves and K order; the share of elements that differ from
the correctly rounded fp64 result (with a residual: from base_alg, the design rounds twice there) must stay within MARGIN x the largest
share among independent fp32 implementations of the same launch - base_alg with chains of 8 and of 32, torch's fp32 convolution, and
F.unfold + torch.mm on the device's own matrix cores - all computed when the test runs; and the row_err bars of test_numerics_gpu.py.

TABLE is not a cross product: every form (tile, ring depth, split-K, K order, XCD order, epilogue) meets every geometry class
(non-square, odd, stride 2, upsample, W == 1, tiles that straddle samples, linear rows) at least once where the form can run at all; that is
asserted when the module is imported, and `coverage()` prints the matrix."""
import math

import pytest
import torch
import torch.nn.functional as F

from edgestyle_amd import lib
from tests import numerics as nm
from tests import test_numerics_gpu as T
from tests.test_numerics_gpu import knobs, launches, judge, done

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256                     # rows of NaN in front of and behind every output slice
RECORD = []                     # one dict per judged launch (python -m tests.numerics --report writes them to NUMERICS.md)
DEVICE_BASELINE = dict(ran=0, left_out=0)     # launches judged with / without the device library's unfold + mm among the baselines

GEOMS = {  # name -> H, W and the geometry arguments of nm.conv_case
    "s1_5x7": dict(H=5, W=7), "s1_7x5": dict(H=7, W=5), "s1_12x20": dict(H=12, W=20), "s1_9x16": dict(H=9, W=16),
    "s1_1x37": dict(H=1, W=37), "s1_37x1": dict(H=37, W=1), "s1_33x31": dict(H=33, W=31),
    "s1_8x16": dict(H=8, W=16),                                       # (added: 128 pixels per sample - one time-embedding row per workgroup)
    "s2_5x7": dict(H=5, W=7, stride=2), "s2_9x12": dict(H=9, W=12, stride=2), "s2_15x16": dict(H=15, W=16, stride=2),
    "s2_33x31": dict(H=33, W=31, stride=2),
    "vae_10x14": dict(H=10, W=14, stride=2, pad=0, out_hw=(5, 7)), "vae_16x24": dict(H=16, W=24, stride=2, pad=0, out_hw=(8, 12)),
    "up_5x7": dict(H=5, W=7, upsample=True), "up_3x8": dict(H=3, W=8, upsample=True), "up_12x10": dict(H=12, W=10, upsample=True),
    "up_4x8": dict(H=4, W=8, upsample=True),                         # (added: 128 output pixels per sample behind the upsample)
    "k1_9x7": dict(H=9, W=7, k=1), "k1_1x1": dict(H=1, W=1, k=1), "k1_13x1": dict(H=13, W=1, k=1),
    # linear rows (ops.linear: [M, 1, 1, K], the sample count is the row count): the time-embedding MLP's 2 rows, one prompt's 77, 3 x 77 = 231
    # (a ragged last 128-row tile and a ragged 256-row tile), 385 (the same at four tiles).  The entry names its own sample counts
    "lin": dict(H=1, W=1, k=1, Ns=([2], [77], [231], [385])),
}
CHANNELS = {"8>64": (8, 0, 64), "16>32": (16, 0, 32), "64>64": (64, 0, 64), "128+64>320": (128, 64, 320), "320>4": (320, 0, 4),
            "128>3": (128, 0, 3), "256>640": (256, 0, 640),
            "8>320": (8, 0, 320),                 # conv_in: 4 latent channels padded to 8 (unaligned: the 4-wave 128-pixel tile only)
            "768>640": (768, 0, 640)}             # the text K / V projection
CLASSES = ("non-square", "odd", "stride 2", "upsample", "W == 1", "straddles samples", "linear rows")
EPILOGUES = ("bias", "temb_tuni", "temb_pix", "temb_silu_res", "tail1", "tail2", "wide1", "wide2", "grouped",
             # res: a plain residual (to_out, ff of an fp16 pipeline).  silu_scale: ES_ACT_SILU and out_scale = 1 / 1.702, nothing else (CLIP's
             # quick_gelu, the time-embedding MLP).  shared: x_rep = 3 (es_gemm_desc.x_nmod).  scale_dev: out_scale = 0.5 times a device scalar 0.7
             "res", "silu_scale", "shared", "scale_dev",
             # single forms, each pinned to the geometry it exists at (not in FORMS): shared_grouped - a shared source of two samples under
             # two weight sets over 3 + 5 samples, the second group starting at launch index 3 (gemm_check accepts the launch: no refusal to
             # assert); conv_in - models.py's grouped conv_in exactly; scale_dev_res - scale, then a residual; scale_dev_gn - the device
             # scale in splitk_reduce_gn_kernel
             "shared_grouped", "conv_in", "scale_dev_res", "scale_dev_gn", "gn_part")
SINGLE_FORMS = ("shared_grouped", "conv_in", "scale_dev_res", "scale_dev_gn", "gn_part")
TEMB = ("temb_tuni", "temb_pix", "temb_silu_res")
SILU = ("temb_silu_res", "silu_scale")
RESIDUAL = ("temb_silu_res", "wide1", "wide2", "res", "conv_in", "scale_dev_res")
WIDE = ("wide1", "wide2", "conv_in")
GN_PART = ("gn_part", "scale_dev_gn")
SHARED = {"shared": 3, "shared_grouped": 4, "conv_in": 4}            # form -> x_rep
SCALES = {"temb_silu_res": (0.7, None), "silu_scale": (1 / 1.702, None), "scale_dev": (0.5, 0.7), "scale_dev_res": (0.5, 0.7),
          "scale_dev_gn": (0.5, 0.7)}                                # form -> (out_scale, the device scalar)
GROUPS = {"shared_grouped": [3, 5], "conv_in": [1, 1, 1, 1]}         # form -> group_n (the `grouped` form: sample_counts)


def R(geom, chan, dt, tile, stages, splitk, korder, xcd, epi, inputs="randn", weights="randn"):
    return dict(geom=geom, chan=chan, dtype=torch.float16 if dt == "f" else torch.bfloat16, tile=tile, stages=stages, splitk=splitk,
                korder=korder, xcd=xcd, epi=epi, inputs=inputs, weights=weights)


TABLE = [
    # the 128-pixel tile on 4 waves (bn 128 | 160), the only one that takes channels that are no multiple of 64
    R("s1_5x7", "8>64", "f", "t4w", 2, 1, 0, 0, "bias"),
    R("s1_7x5", "16>32", "b", "t4w", 2, 2, 0, 1, "bias"),
    R("s1_37x1", "8>64", "f", "t4w", 2, 2, 0, 0, "temb_pix"),
    R("s2_5x7", "16>32", "f", "t4w", 2, 2, 0, 1, "temb_pix"),
    R("up_5x7", "8>64", "b", "t4w", 2, 1, 0, 1, "bias"),
    R("vae_10x14", "16>32", "f", "t4w", 2, 1, 0, 0, "bias"),
    R("k1_13x1", "16>32", "f", "t4w", 2, 1, 0, 0, "temb_pix"),
    R("s1_33x31", "320>4", "f", "t4w", 4, 7, 0, 0, "bias", "silu3"),
    R("up_12x10", "128>3", "f", "t4w", 2, 4, 0, 1, "bias", "silu0"),
    R("s2_33x31", "320>4", "b", "t4w", 2, 2, 1, 0, "temb_silu_res"),
    R("s1_12x20", "128+64>320", "f", "t4w", 4, 1, 0, 1, "temb_silu_res", "silu3"),
    R("s1_9x16", "256>640", "b", "t4w", 2, 5, 1, 0, "wide1"),
    R("s1_1x37", "64>64", "f", "t4w", 4, 2, 1, 1, "tail1"),
    R("s1_37x1", "64>64", "b", "t4w", 2, 1, 1, 0, "tail2"),
    R("vae_16x24", "128+64>320", "f", "t4w", 2, 1, 1, 1, "temb_pix", "peak"),
    R("up_3x8", "64>64", "f", "t4w", 4, 1, 0, 0, "temb_silu_res", "silu0"),
    R("k1_9x7", "128+64>320", "b", "t4w", 2, 2, 0, 0, "wide2"),
    R("k1_1x1", "256>640", "f", "t4w", 2, 1, 0, 1, "temb_pix"),
    R("s1_8x16", "64>64", "f", "t4w", 2, 1, 0, 0, "temb_tuni"),
    R("up_4x8", "128+64>320", "f", "t4w", 4, 2, 1, 1, "temb_tuni"),
    R("s1_8x16", "128+64>320", "f", "t4w", 2, 1, 0, 1, "grouped"),
    R("s2_9x12", "256>640", "f", "t4w", 2, 1, 0, 0, "bias", "near_2^10", "subnormal"),
    R("s1_7x5", "256>640", "b", "t4w", 4, 1, 1, 1, "bias", "randn", "zero"),
    # ... on 8 waves
    R("s1_5x7", "128+64>320", "f", "t8w", 2, 1, 0, 0, "temb_silu_res"),
    R("s1_33x31", "64>64", "b", "t8w", 4, 2, 0, 1, "bias"),
    R("s1_37x1", "256>640", "f", "t8w", 2, 5, 1, 1, "temb_pix"),
    R("s2_9x12", "128+64>320", "b", "t8w", 2, 1, 1, 0, "wide1"),
    R("up_5x7", "64>64", "f", "t8w", 2, 2, 1, 0, "bias", "peak"),
    R("k1_13x1", "128+64>320", "f", "t8w", 2, 1, 0, 1, "temb_silu_res"),
    R("s1_8x16", "256>640", "f", "t8w", 4, 1, 0, 0, "temb_tuni"),
    R("s1_9x16", "64>64", "f", "t8w", 2, 1, 0, 1, "tail1"),
    R("s1_7x5", "256>640", "b", "t8w", 2, 4, 0, 0, "tail2"),
    R("s2_15x16", "64>64", "f", "t8w", 2, 1, 0, 0, "grouped"),
    R("s2_5x7", "256>640", "b", "t8w", 2, 2, 0, 1, "wide2"),
    R("up_12x10", "128+64>320", "f", "t8w", 2, 1, 0, 1, "temb_pix"),
    R("up_4x8", "64>64", "b", "t8w", 4, 1, 1, 0, "temb_tuni"),
    R("s1_37x1", "64>64", "f", "t8w", 4, 1, 0, 0, "tail1"),
    R("up_3x8", "256>640", "b", "t8w", 2, 1, 0, 0, "wide1"),
    # the 64 x 64 tile
    R("s1_7x5", "64>64", "f", "t64", 2, 1, 0, 0, "bias", "silu0"),
    R("s1_12x20", "128+64>320", "b", "t64", 4, 2, 0, 1, "temb_silu_res"),
    R("s1_37x1", "64>64", "f", "t64", 2, 2, 1, 0, "temb_pix"),
    R("s2_15x16", "64>64", "f", "t64", 2, 1, 0, 1, "temb_tuni"),
    R("s2_33x31", "256>640", "b", "t64", 4, 5, 1, 1, "wide1"),
    R("up_5x7", "128+64>320", "f", "t64", 2, 1, 1, 0, "temb_pix"),
    R("k1_13x1", "64>64", "b", "t64", 2, 1, 0, 0, "bias"),
    R("s1_1x37", "256>640", "f", "t64", 2, 1, 0, 1, "tail2"),
    R("vae_10x14", "64>64", "f", "t64", 4, 1, 0, 0, "bias", "randn", "zero"),
    R("k1_9x7", "256>640", "b", "t64", 2, 2, 0, 1, "wide2"),
    R("up_4x8", "64>64", "f", "t64", 2, 1, 0, 0, "grouped"),
    R("s1_9x16", "64>64", "f", "t64", 2, 2, 0, 1, "tail1"),
    R("k1_1x1", "128+64>320", "f", "t64", 2, 1, 0, 0, "bias"),
    R("up_12x10", "256>640", "b", "t64", 4, 5, 0, 1, "wide2"),
    R("s1_37x1", "256>640", "b", "t64", 4, 1, 0, 1, "wide1"),
    # the 256 x 320 tile (the epilogue forms es_conv_gemm8p_form_ok accepts; everything once K is split)
    R("s1_5x7", "128+64>320", "f", "t320", 2, 1, 0, 0, "bias", "near_2^10", "subnormal"),
    R("s1_33x31", "256>640", "b", "t320", 2, 1, 0, 1, "wide1"),
    R("s1_37x1", "128+64>320", "f", "t320", 2, 2, 0, 0, "temb_silu_res"),
    R("s2_9x12", "256>640", "f", "t320", 2, 5, 1, 1, "temb_pix"),
    R("up_12x10", "128+64>320", "b", "t320", 2, 1, 1, 0, "wide2"),
    R("s1_8x16", "256>640", "f", "t320", 2, 1, 0, 1, "temb_tuni"),
    R("k1_13x1", "128+64>320", "f", "t320", 2, 1, 0, 0, "bias"),
    R("s1_1x37", "256>640", "f", "t320", 2, 1, 0, 1, "tail1"),
    R("vae_16x24", "256>640", "b", "t320", 2, 2, 0, 0, "bias"),
    R("up_3x8", "128+64>320", "f", "t320", 2, 1, 0, 1, "bias", "silu3"),
    R("s1_8x16", "128+64>320", "f", "t320", 2, 1, 1, 0, "grouped"),
    R("s1_12x20", "256>640", "f", "t320", 2, 4, 0, 0, "tail2"),
    R("up_4x8", "256>640", "f", "t320", 2, 1, 1, 0, "temb_tuni"),
    R("s2_15x16", "128+64>320", "f", "t320", 2, 1, 1, 1, "bias"),
    R("s1_37x1", "256>640", "b", "t320", 2, 1, 1, 1, "tail2"),
    R("s2_5x7", "128+64>320", "b", "t320", 2, 1, 0, 0, "wide1"),
    R("k1_13x1", "256>640", "b", "t320", 2, 1, 0, 1, "wide2"),
    # tm * tn * splitk = 1 * 5 * 11 = 55 workgroups: no multiple of 8, prime factor 11 - the XCD remap in both tile orders
    R("s1_5x7", "256>640", "f", "t4w", 2, 11, 0, 0, "bias"),
    R("s1_5x7", "256>640", "f", "t4w", 2, 11, 0, 1, "bias"),
    # GroupNorm statistics handed over: the gn_part table is guarded like the outputs
    R("s1_8x16", "128+64>320", "f", "t4w", 2, 1, 0, 0, "gn_part"),
    R("s2_15x16", "64>64", "b", "t64", 2, 2, 0, 0, "gn_part"),
    # a plain residual, no time embedding, no activation (judged against base_alg like every form that rounds twice)
    R("lin", "768>640", "f", "t8w", 2, 1, 0, 0, "res"),
    R("s2_5x7", "64>64", "f", "t4w", 4, 1, 1, 1, "res"),
    R("up_3x8", "128+64>320", "b", "t64", 2, 2, 0, 0, "res"),
    R("lin", "768>640", "b", "t320", 2, 5, 0, 1, "res"),
    # SiLU and a scale, nothing else.  The 256 x 320 tile has no SiLU epilogue (es_conv_gemm8p_form_ok sends the fused form to the
    # 128 x 160 tile: asserted below, at import); with K split its partials go through the reduce, which has every form
    R("lin", "768>640", "f", "t4w", 2, 1, 0, 0, "silu_scale"),
    R("lin", "256>640", "b", "t64", 4, 2, 0, 1, "silu_scale"),
    R("s2_9x12", "64>64", "f", "t8w", 4, 1, 1, 0, "silu_scale"),
    R("up_5x7", "128+64>320", "f", "t320", 2, 2, 0, 0, "silu_scale"),
    # a shared source, x_rep = 3: both loaders (aligned and not), both K orders, every tile; 33 x 31 and 17 x 16 pixels per sample put the
    # wrap from source sample nsrc - 1 to 0 inside a tile; lin x 768>640 is the text K / V projection (231 rows: nsrc = 77)
    R("lin", "768>640", "f", "t4w", 2, 1, 0, 0, "shared"),
    R("s1_5x7", "64>64", "f", "t8w", 2, 1, 1, 1, "shared"),
    R("s2_33x31", "256>640", "b", "t64", 2, 5, 0, 0, "shared"),
    R("up_3x8", "256>640", "f", "t320", 2, 1, 0, 1, "shared"),
    R("s1_33x31", "64>64", "f", "t4w", 4, 2, 1, 0, "shared"),
    R("lin", "768>640", "b", "t320", 2, 1, 0, 0, "shared"),
    R("s1_37x1", "8>64", "f", "t4w", 2, 1, 0, 0, "shared"),
    # ... under two weight sets, the second group starting at launch index 3 of a source of 2: sample n of the LAUNCH reads n % x_nmod
    R("s1_8x16", "64>64", "f", "t4w", 2, 1, 0, 0, "shared_grouped"),
    R("up_4x8", "64>64", "b", "t64", 2, 2, 0, 1, "shared_grouped"),
    # conv_in of all nets in one launch: four weight sets over one sample each, all reading the one latent, + condition, two-word output
    R("s1_8x16", "8>320", "b", "t4w", 2, 1, 0, 0, "conv_in"),
    # the device scalar at each of its read sites: the fused epilogue of every tile, the plain reduce (split in two, ragged), the reduce
    # that hands GroupNorm statistics over; and followed by a residual in the same launch
    R("s1_7x5", "64>64", "f", "t4w", 2, 1, 0, 0, "scale_dev"),
    R("s2_15x16", "64>64", "b", "t8w", 2, 1, 1, 1, "scale_dev"),
    R("up_5x7", "256>640", "f", "t64", 2, 1, 0, 0, "scale_dev"),
    R("s1_37x1", "256>640", "f", "t320", 2, 1, 0, 1, "scale_dev"),
    R("k1_9x7", "128+64>320", "f", "t4w", 2, 2, 0, 0, "scale_dev"),
    R("s1_12x20", "256>640", "b", "t320", 2, 7, 1, 0, "scale_dev"),
    R("lin", "768>640", "f", "t64", 2, 1, 0, 1, "scale_dev"),
    R("s2_15x16", "64>64", "f", "t64", 2, 2, 0, 0, "scale_dev_gn"),
    R("lin", "768>640", "f", "t4w", 4, 3, 0, 0, "scale_dev_res"),
    # the other epilogue forms on linear rows
    R("lin", "256>640", "f", "t8w", 2, 1, 0, 0, "temb_silu_res"),
    R("lin", "768>640", "b", "t4w", 2, 2, 0, 1, "wide1"),
    R("lin", "256>640", "b", "t64", 4, 1, 0, 0, "wide2"),
    R("lin", "64>64", "f", "t4w", 4, 1, 0, 1, "tail1"),
    R("lin", "64>64", "f", "t64", 2, 2, 0, 0, "tail2"),
]
# the scale_dev row that is launched a second time with the device scalar at 0.0 (conditioning_scale = 0): every element == 0 and finite
ZERO_SCALE = ("s1_7x5", "t4w", "scale_dev")


def _tile_rows(row):
    return {"t64": 64, "t320": 256}.get(row["tile"], 128)


def _geometry(row):
    g = dict(GEOMS[row["geom"]])
    k = g.setdefault("k", 3)
    g.setdefault("stride", 1)
    g.setdefault("upsample", False)
    g["pad"] = g.get("pad", 1 if k == 3 else 0)
    g["out_hw"] = nm.conv_out_hw(g["H"], g["W"], k, g["stride"], g["pad"], g["upsample"], g.get("out_hw"))
    return g


def _tails(row):
    return {"tail1": (64,), "tail2": (64, 128)}.get(row["epi"], ())


def _nk(row):
    g = _geometry(row)
    C1, C2, _ = CHANNELS[row["chan"]]
    return (g["k"] ** 2 * (C1 + C2) + sum(_tails(row)) + 63) // 64


def row_classes(row):
    g = _geometry(row)
    Hout, Wout = g["out_hw"]
    half = 128 if row["tile"] == "t320" else _tile_rows(row)            # the 256-pixel tile stores in two 128-pixel halves
    out = set()
    if g["H"] != g["W"] and Hout * Wout > 1:
        out.add("non-square")
    if g["H"] % 2 or g["W"] % 2:
        out.add("odd")
    if g["stride"] == 2:
        out.add("stride 2")
    if g["upsample"]:
        out.add("upsample")
    if Wout == 1:
        out.add("W == 1")
    if (Hout * Wout) % half:
        out.add("straddles samples")                                   # at N = 3 (grouped rows: inside a group)
    if (g["H"], g["W"], g["k"]) == (1, 1, 1):
        out.add("linear rows")                                         # the HWout == 1 branch of the pixel decode: n = m
    return out


def row_forms(row):
    nk, sk = _nk(row), row["splitk"]
    out = {row["tile"], f"stages {row['stages']}", f"korder {row['korder']}", f"xcd {row['xcd']}", row["epi"]}
    if sk == 1:
        out.add("splitk 1")
    if sk == 2:
        out.add("splitk 2")
    if sk > 1 and nk % sk:
        out.add("splitk ragged")
    return out


FORMS = ("t4w", "t8w", "t64", "t320", "stages 2", "stages 4", "splitk 1", "splitk 2", "splitk ragged", "korder 0", "korder 1", "xcd 0", "xcd 1") \
    + tuple(e for e in EPILOGUES if e not in SINGLE_FORMS)
# (form, class) pairs no launch can realise: the form's own preconditions.  (The new forms - res, silu_scale, shared, scale_dev - have
# none: each meets every geometry class, "linear rows" included.)
IMPOSSIBLE = {("tail1", "stride 2"), ("tail1", "upsample"), ("tail2", "stride 2"), ("tail2", "upsample"),      # tails: same-size output
              ("temb_tuni", "W == 1"), ("temb_tuni", "straddles samples"), ("temb_tuni", "linear rows"),        # H * W % tile rows == 0
              ("grouped", "W == 1"), ("grouped", "linear rows"),                                                # groups of whole 128-pixel tiles
              ("korder 1", "linear rows")}                                                                      # chunk-major K: 3 x 3 only


def row_id(row):
    return "-".join([row["geom"], row["chan"], T._name(row["dtype"]), row["tile"], f"st{row['stages']}", f"sk{row['splitk']}", f"ko{row['korder']}",
                     f"xcd{row['xcd']}", row["epi"]] + ([row["inputs"]] if row["inputs"] != "randn" else []) + ([row["weights"]] if row["weights"] != "randn" else []))


def route_desc(row):
    """the row's launch of one sample as a descriptor for lib.gemm_route: geometry and flags as launch() will record them, pointers as
    present or absent (the route reads no more of them)"""
    g, (C1, C2, Cout), epi, tails = _geometry(row), CHANNELS[row["chan"]], row["epi"], _tails(row)
    pw_bn = 160 if (Cout % 160 == 0 and Cout % 128 != 0) else 128          # ops.choose_bn
    d = lib.GemmDesc()
    d.x = d.w = d.out = 1
    d.N, d.Hsrc, d.Wsrc, d.C1, d.C2, d.x2 = 1, g["H"], g["W"], C1, C2, 1 if C2 else None
    (d.Hout, d.Wout), d.Cout = g["out_hw"], Cout
    d.rows_padded, d.Kpad = -(-Cout // pw_bn) * pw_bn, _nk(row) * 64
    d.ksize, d.stride, d.pad, d.upsample = g["k"], g["stride"], g["pad"], int(g["upsample"])
    d.splitk, d.workspace = row["splitk"], 1 if row["splitk"] > 1 else None
    d.bn, d.waves = {"t64": 64, "t320": 320}.get(row["tile"], pw_bn), {"t4w": 4, "t8w": 8}.get(row["tile"], 0)
    d.stages, d.korder, d.xcd_m_fastest, d.dtype = row["stages"], row["korder"], row["xcd"], lib.ES_F16 if row["dtype"] == torch.float16 else lib.ES_BF16
    for i, ct in enumerate(tails):
        setattr(d, f"t{i + 1}", 1)
        setattr(d, f"Ct{i + 1}", ct)
    d.temb = 1 if epi in TEMB else None
    d.act = lib.ACT_SILU if epi in SILU else lib.ACT_NONE
    d.residual = 1 if epi in RESIDUAL else None
    d.out_lo, d.residual_lo = 1 if epi in WIDE else None, 1 if epi == "wide2" else None
    d.gn_part, d.gn_groups = 1 if epi in GN_PART else None, 32
    d.out_scale = SCALES.get(epi, (1.0, None))[0]
    d.out_scale_dev = 1 if SCALES.get(epi, (1.0, None))[1] is not None else None
    d.x_nmod = 1 if epi in SHARED else 0                                   # (one sample: the source is that sample)
    return d


def expected_kernel(row, bn):
    """es_conv_gemm_last_kernel, unpacked (lib.gemm_kernel_fields), of the tile the row names: its pixels, waves, ring depth and K order.
    A row that names the 256 x 320 tile with an epilogue that tile lacks (es_conv_gemm8p_form_ok: a fused SiLU, ...) is expected where the
    library sends it - the 128 x 160 tile on 4 waves; validate() refuses such a row in TABLE, so that none passes on another tile unseen"""
    C1, C2, _ = CHANNELS[row["chan"]]
    if row["tile"] == "t320" and not nm.gemm_big_tile_takes(route_desc(row)):
        return dict(bn=160, bm=128, stages=2, waves=4, aligned=True, ln=False, ko=bool(row["korder"]), geglu=False, bf16=row["dtype"] == torch.bfloat16)
    return dict(bn=bn, bm=_tile_rows(row), stages=row["stages"], waves={"t8w": 8, "t320": 8}.get(row["tile"], 4),
                aligned=C1 % 64 == 0 and C2 % 64 == 0, ln=False, ko=bool(row["korder"]), geglu=False, bf16=row["dtype"] == torch.bfloat16)


def validate(row):
    """the preconditions of the row's form, so that a table entry that cannot run is found at import and not on the GPU"""
    g, (C1, C2, Cout) = _geometry(row), CHANNELS[row["chan"]]
    Hout, Wout = g["out_hw"]
    hw, nk, name = Hout * Wout, _nk(row), row_id(row)
    aligned = C1 % 64 == 0 and C2 % 64 == 0
    bn = {"t64": 64, "t320": 320}.get(row["tile"], 160 if (Cout % 160 == 0 and Cout % 128 != 0) else 128)
    assert 1 <= row["splitk"] <= nk, name
    assert aligned or (row["tile"] == "t4w" and row["stages"] == 2 and row["korder"] == 0 and not _tails(row)), name
    assert row["korder"] == 0 or (g["k"] == 3 and aligned), name
    assert row["tile"] != "t8w" or row["stages"] == 2 or bn == 128, name
    assert row["tile"] != "t320" or (row["stages"] == 2 and Cout % 320 == 0), name
    assert row["tile"] != "t64" or Cout % 64 == 0, name
    if _tails(row):
        assert g["stride"] == 1 and not g["upsample"] and (Hout, Wout) == (g["H"], g["W"]), name
    if row["epi"] == "temb_tuni":
        assert hw % (128 if bn == 320 else _tile_rows(row)) == 0, name
    if row["epi"] == "temb_pix":
        assert hw % _tile_rows(row) != 0, name
    if row["epi"] in WIDE:
        assert row["dtype"] == torch.bfloat16 and Cout % 8 == 0, name
    if row["epi"] in SHARED:
        assert C2 == 0 and not _tails(row), name                         # gemm_check: x_nmod needs a single source
    if row["epi"] in GROUPS:
        assert hw % (256 if row["tile"] == "t320" else 128) == 0, name   # groups of whole tiles at any sample counts
    if row["epi"] == "conv_in":
        assert (row["geom"], row["chan"], row["tile"], g["k"]) == ("s1_8x16", "8>320", "t4w", 3), name
    if "Ns" in GEOMS[row["geom"]]:
        assert row["epi"] not in GROUPS and row["epi"] != "grouped" and all(len(ns) == 1 for ns in GEOMS[row["geom"]]["Ns"]), name
    # the tile the row names is the tile its descriptor reaches: the library's route (no GPU needed) and its Python mirror both say so.
    # A t320 row whose epilogue the 256-pixel kernel lacks would run - and pass - on the 128 x 160 tile
    d = route_desc(row)
    got, mirror = lib.gemm_route(d), nm.gemm_route(d)
    assert lib.gemm_kernel_fields(got["kernel"]) == lib.gemm_kernel_fields(mirror["kernel"]) == expected_kernel(row, d.bn), (name, got, mirror)
    assert row["tile"] != "t320" or (got["family"] == 1 and expected_kernel(row, d.bn)["bm"] == 256), \
        f"{name}: the 256 x 320 tile lacks this epilogue form, the row would run on the 128 x 160 tile"
    if row["inputs"] == "peak":
        assert row["dtype"] == torch.float16, name
    if row["weights"] == "zero":
        assert row["epi"] == "bias", name
    if row["epi"] in GN_PART:
        assert hw % 64 == 0 and Cout % 32 == 0 and Cout // 32 <= (160 if bn == 320 else bn) and (row["splitk"] == 1 or Cout // 32 <= 64), name


def coverage():
    """form x geometry class -> number of table rows; asserts that every possible pair is met"""
    cells = {(f, c): 0 for f in FORMS for c in CLASSES}
    for row in TABLE:
        for f in row_forms(row):
            for c in row_classes(row):
                if (f, c) in cells:
                    cells[(f, c)] += 1
    lines = [f"{'form':<16}" + "".join(f"{c:>19}" for c in CLASSES)]
    for f in FORMS:
        lines.append(f"{f:<16}" + "".join(f"{'-' if (f, c) in IMPOSSIBLE else cells[(f, c)]:>19}" for c in CLASSES))
    missing = [fc for fc, n in cells.items() if n == 0 and fc not in IMPOSSIBLE]
    return "\n".join(lines), missing


for _row in TABLE:
    validate(_row)
# a fused silu_scale launch recorded with bn = 320 lands on the 128 x 160 tile (which is why TABLE has that form on t320 with K split only):
# the library's route and its mirror say so, expected_kernel says so, and validate() refuses the row
_fused = dict([r for r in TABLE if r["epi"] == "silu_scale" and r["tile"] == "t320"][0], splitk=1)
_d = route_desc(_fused)
assert lib.gemm_kernel_fields(lib.gemm_route(_d)["kernel"]) == lib.gemm_kernel_fields(nm.gemm_route(_d)["kernel"]) == expected_kernel(_fused, 320) \
    and expected_kernel(_fused, 320)["bn"] == 160 and lib.gemm_route(_d)["family"] == 0
try:
    validate(_fused)
except AssertionError as _e:
    assert "lacks this epilogue form" in str(_e), _e
else:
    raise AssertionError("validate() lets a fused SiLU row on the 256 x 320 tile pass")
assert len([r for r in TABLE if (r["geom"], r["tile"], r["epi"]) == ZERO_SCALE]) == 1
_matrix, _missing = coverage()
assert not _missing, f"test_conv_gpu.TABLE leaves (form, geometry class) pairs unmet: {_missing}\n{_matrix}"
assert len({row_id(r) for r in TABLE}) == len(TABLE)


# ----------------------------------------------------------------------------------------------------------------
# launching
# ----------------------------------------------------------------------------------------------------------------
def guarded(rows, width, dtype):
    """(whole buffer, the slice [rows, width] cut from its middle): everything NaN"""
    big = torch.full(((rows + 2 * GUARD) * width,), float("nan"), dtype=dtype, device=DEV)
    return big, big[GUARD * width:(GUARD + rows) * width].view(rows, width)


def guards_intact(big, rows, width):
    return bool(torch.isnan(big[:GUARD * width]).all()) and bool(torch.isnan(big[(GUARD + rows) * width:]).all())


def _variant(row, pw_bn):
    """(knobs, expected descriptor fields) of the row's tile"""
    bn = {"t64": 64, "t320": 320}.get(row["tile"], pw_bn)
    waves = {"t4w": 4, "t8w": 8}.get(row["tile"], 0)
    kn = dict(FORCE_BN=bn, FORCE_WAVES=waves, XCD_ORDER=row["xcd"], XS_ENABLED=False)
    return kn, dict(bn=bn, waves=waves, stages=row["stages"], splitk=row["splitk"], korder=row["korder"], xcd_m_fastest=row["xcd"])


def _pack(ops, c, korder):
    with knobs(CHUNK_MAJOR=bool(korder)):
        if c["tails"]:
            return ops.pack_weight_tail(c["w"], c["wt"], c["b"], c["dtype"], DEV)
        return ops.pack_weight(c["w"], c["b"], c["dtype"], DEV)


def launch(row, cases, dev_scale=None):
    """one es_conv_gemm launch over the concatenated samples of `cases` (one case; several = a grouped launch with one weight set per
    case) into guarded buffers.  A shared source: the launch is handed the cases' common "x_src" and x_rep.  A device scale: element
    [1:2] of a 3-element fp32 vector whose neighbours are NaN (the engine passes scales_dev[0:1] of a longer vector); dev_scale
    overrides its value.  Returns dict(y, lo, desc, problems)."""
    from edgestyle_amd import ops, lib
    c0, dt = cases[0], cases[0]["dtype"]
    Hout, Wout = c0["out_hw"]
    N, Cout = sum(c["N"] for c in cases), c0["Cout"]
    M = N * Hout * Wout
    dev = lambda key: None if c0[key] is None else torch.cat([c[key] for c in cases]).to(DEV, dt)
    pws = [_pack(ops, c, row["korder"]) for c in cases]
    kn, want = _variant(row, pws[0].bn)
    problems = []
    big, out2 = guarded(M, Cout, dt)
    out = out2.view(N, Hout, Wout, Cout)
    kw = dict(stride=c0["stride"], pad=c0["pad"], upsample=c0["upsample"], out_hw=c0["out_hw"], x2=dev("x2"), out=out,
              splitk=row["splitk"], stages=row["stages"])
    if c0["tails"]:
        kw["tail"] = tuple(torch.cat([c["tails"][i] for c in cases]).to(DEV, dt) for i in range(len(c0["tails"])))
    if c0["temb"] is not None:       # a slice of a wider table, as the engine passes it (es_gemm_desc.temb_stride)
        table = torch.zeros(N, Cout + 64, dtype=dt, device=DEV)
        table[:, 64:] = dev("temb")
        kw["temb"] = table[:, 64:]
    if c0["silu"]:
        kw["act"] = lib.ACT_SILU
    if c0["scale_dev"] is not None:
        vec = torch.tensor([float("nan"), c0["scale_dev"] if dev_scale is None else dev_scale, float("nan")], dtype=torch.float32, device=DEV)
        kw.update(out_scale=c0["scale_host"], out_scale_dev=vec[1:2])
    elif c0["scale"] != 1.0:
        kw["out_scale"] = c0["scale"]
    nsrc = c0["nsrc"]
    if nsrc:
        assert N % nsrc == 0 and all(c["x_src"] is c0["x_src"] for c in cases)
        kw["x_rep"] = N // nsrc
        xdev = c0["x_src"].to(DEV, dt)
    else:
        xdev = dev("x")
    wide = row["epi"] in WIDE
    big_lo = None
    if c0["res"] is not None:
        kw["residual"] = dev("res")
        if wide:
            if c0["res_lo"] is not None:
                kw["residual"]._lo = dev("res_lo")
            big_lo, lo2 = guarded(M, Cout, dt)
            kw.update(wide=True, out_lo=lo2.view(N, Hout, Wout, Cout))
    big_gn = None
    if row["epi"] in GN_PART:
        gshape = (N, 2 * (Hout * Wout // 64), 32, 2)
        big_gn, gn2 = guarded(gshape[0] * gshape[1], 64, torch.float32)
        kw.update(gn_groups=32, gn_part=gn2.view(gshape))
        kn.update(GN_HANDOVER=True, GN_HANDOVER_ALL=True)
    if len(cases) > 1:
        kw["group_n"] = [c["N"] for c in cases]
    with knobs(**kn), launches() as rec:
        y = ops.conv_gemm(xdev, pws if len(cases) > 1 else pws[0], **kw)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr() and len(rec.descs) == 1
    d = rec.descs[0]
    got = {k: int(getattr(d, k)) for k in want}
    if got != want:
        problems.append(f"descriptor {got} != {want}")
    ran = lib.gemm_kernel_fields(lib.load().es_conv_gemm_last_kernel())          # the launcher's own template arguments
    if ran != expected_kernel(row, want["bn"]):
        problems.append(f"kernel {ran} ran, the row's tile is {expected_kernel(row, want['bn'])}")
    if len(cases) > 1 and int(d.ngroups) != len(cases):
        problems.append(f"ngroups {int(d.ngroups)}")
    if int(d.x_nmod) != nsrc or int(d.N) != N:
        problems.append(f"descriptor: x_nmod {int(d.x_nmod)} and N {int(d.N)}, the source holds {nsrc} samples (0: not shared) and the launch covers {N}")
    if (int(d.out_scale_dev or 0) != 0) != (c0["scale_dev"] is not None):
        problems.append("the device scale's pointer is not in the descriptor")
    if wide and not (int(d.out_lo or 0) and (int(d.residual_lo or 0) != 0) == (c0["res_lo"] is not None)):
        problems.append("the two-word stream's pointers are not in the descriptor")
    for name, b, t, rows, width in (("out", big, out2, M, Cout), ("out_lo", big_lo, kw.get("out_lo"), M, Cout),
                                    ("gn_part", big_gn, kw.get("gn_part"), 0 if big_gn is None else gshape[0] * gshape[1], 64)):
        if b is None:
            continue
        if not guards_intact(b, rows, width):
            problems.append(f"{name}: a store outside the output (guard rows no longer NaN)")
        nan = int(torch.isnan(t).sum())
        if nan:
            problems.append(f"{name}: {nan} elements never written (still NaN)")
    return dict(y=out.float().cpu(), lo=None if big_lo is None else kw["out_lo"].float().cpu(), problems=problems, desc=got)


def device_matmul(c, wide):
    """F.unfold + torch.mm in the storage dtype on the device (fp32 result, reduced-precision reductions off), then the kernel's
    epilogue on the CPU: an independent implementation on the same matrix cores.  None where the library has no such call."""
    dt = c["dtype"]
    f16, b16 = torch.backends.cuda.matmul.allow_fp16_reduced_precision_reduction, torch.backends.cuda.matmul.allow_bf16_reduced_precision_reduction
    torch.backends.cuda.matmul.allow_fp16_reduced_precision_reduction = False
    torch.backends.cuda.matmul.allow_bf16_reduced_precision_reduction = False
    try:
        x = c["x"] if c["x2"] is None else torch.cat([c["x"], c["x2"]], dim=-1)
        x = x.permute(0, 3, 1, 2).to(DEV, dt)
        if c["upsample"]:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
        Hout, Wout = c["out_hw"]
        k, s, p = c["k"], c["stride"], c["pad"]
        x = F.pad(x, (p, max((Wout - 1) * s + k - x.shape[3] - p, 0), p, max((Hout - 1) * s + k - x.shape[2] - p, 0)))
        Hf, Wf = (x.shape[2] - k) // s + 1, (x.shape[3] - k) // s + 1
        cols = F.unfold(x, k, stride=s).reshape(x.shape[0], -1, Hf, Wf)[:, :, :Hout, :Wout]
        A = cols.permute(0, 2, 3, 1).reshape(-1, cols.shape[1])
        Wm = c["w"].reshape(c["Cout"], -1).to(DEV, dt)
        if c["tails"]:
            A = torch.cat([A] + [t.reshape(-1, t.shape[-1]).to(DEV, dt) for t in c["tails"]], dim=1)
            Wm = torch.cat([Wm, c["wt"].to(DEV, dt)], dim=1)
        acc = torch.mm(A.contiguous(), Wm.t().contiguous(), out_dtype=torch.float32)
        torch.cuda.synchronize()
    except (RuntimeError, TypeError, NotImplementedError) as e:
        print(f"numerics: device unfold + mm not available here: {type(e).__name__}: {str(e)[:120]}", flush=True)
        return None
    finally:
        torch.backends.cuda.matmul.allow_fp16_reduced_precision_reduction = f16
        torch.backends.cuda.matmul.allow_bf16_reduced_precision_reduction = b16
    return nm.conv_epilogue(c, acc.cpu().reshape(c["N"], Hout, Wout, c["Cout"]), wide)


def _pair_differs(a, b):
    """number of elements in which two results differ; (hi, lo) pairs differ where either word does"""
    if isinstance(a, tuple):
        return int(((a[0] != b[0]) | (a[1] != b[1])).sum())
    return nm.differs(a, b, count=True)


def check(fails, name, row, c, y, lo):
    """the bars of one case against one launch's output (a grouped launch: the case's samples of it)"""
    dt = c["dtype"]
    wide = lo is not None
    ref = nm.conv_ref64(c)
    base = nm.conv_baselines(c, row["splitk"], row["korder"], wide)
    dev = device_matmul(c, wide)
    DEVICE_BASELINE["ran" if dev is not None else "left_out"] += 1
    if dev is not None:
        base["device"] = dev
    got = (y, lo) if wide else y
    if c["res"] is None:
        counts = {k: nm.misrounded(v, ref, dt, count=True) for k, v in base.items()}
        n_kernel, against = nm.misrounded(y, ref, dt, count=True), "the rounded fp64 result"
    else:
        counts = {k: _pair_differs(v, base["alg8"]) for k, v in base.items() if k != "alg8"}
        n_kernel, against = _pair_differs(got, base["alg8"]), "base_alg"
    numel = ref.numel()
    bar = nm.misrounded_bar(counts.values())
    small = "" if numel >= nm.CONV_MIN_ELEMENTS else f" [{numel} elements: under {nm.CONV_MIN_ELEMENTS}, the floor of {nm.MISROUNDED_FLOOR} is loose here]"
    print(f"numerics: {name}: differing from {against}: kernel {n_kernel} ({n_kernel / numel:.4%})  baselines "
          + " ".join(f"{k} {v / numel:.4%}" for k, v in counts.items()) + ("" if dev is not None else " device left out")
          + f"  bar {bar} elements{small}", flush=True)
    ysum = y if not wide else y + lo
    alg = base["alg8"] if not wide else base["alg8"][0] + base["alg8"][1]
    e_alg, e_ref = nm.row_err(alg, ref), nm.row_err(nm.conv_base_ref(c), ref)
    judge(fails, name, ysum, ref, e_alg, e_ref, dt)
    RECORD.append(dict(case=name, numel=numel, kernel=n_kernel, counts=counts, bar=bar, against=against, kernel_err=nm.row_err(ysum, ref),
                       base_alg=e_alg, base_ref=e_ref))
    if T.RECORD is not None:
        return
    if n_kernel > bar:
        fails.append(f"{name}: {n_kernel} elements differ from {against}, the bar is {bar} ({counts})")
    if c["w"].abs().max() == 0 and not torch.equal(y, nm.rnd(c["b"], dt).expand_as(y)):
        fails.append(f"{name}: all-zero weights must return the rounded bias in every tile")
    if row["inputs"] == "peak" and not bool(torch.isfinite(y).all()):
        fails.append(f"{name}: not finite at a peak of {float(ref.abs().max()):.3g}")


def make_cases(row, Ns, seed):
    g, (C1, C2, Cout) = _geometry(row), CHANNELS[row["chan"]]
    epi = row["epi"]
    scale, scale_dev = SCALES.get(epi, (1.0, None))
    kw = dict(k=g["k"], stride=g["stride"], pad=g["pad"], upsample=g["upsample"], out_hw=g["out_hw"], C2=C2, tails=_tails(row),
              temb=epi in TEMB, silu=epi in SILU, scale=scale, scale_dev=scale_dev,
              residual=epi in RESIDUAL, residual_lo=epi == "wide2", inputs=row["inputs"], weights=row["weights"])
    if epi in SHARED:                  # one source for the whole launch: the first case draws it, the other groups' cases are handed it
        nsrc, cases = sum(Ns) // SHARED[epi], []
        assert nsrc * SHARED[epi] == sum(Ns)
        for i, n in enumerate(Ns):
            cases.append(nm.conv_case(n, g["H"], g["W"], C1, Cout, row["dtype"], seed=seed + 7 * i, nsrc=nsrc, first=sum(Ns[:i]),
                                      src=cases[0]["x_src"] if i else None, **kw))
        assert len(Ns) == 1 or epi == "conv_in" or any(c["first"] % nsrc for c in cases)      # a group that starts off a multiple of nsrc
        return cases
    return [nm.conv_case(n, g["H"], g["W"], C1, Cout, row["dtype"], seed=seed + 7 * i, **kw) for i, n in enumerate(Ns)]


def sample_counts(row):
    """N = 1 and N = 3 (tiles straddle sample boundaries); one larger N where three samples are under CONV_MIN_ELEMENTS outputs, so
    that the misrounded bar has something to bite on; grouped launches: two weight sets over whole tiles.  A geometry that names its
    sample counts (GEOMS[..]["Ns"]) gets those.  A shared source (x_rep = 3) takes multiples of 3: 3 and 6 samples (a source of one and
    of two), a named count rounded down to one (3, 75 = 3 x 25, 231 = 3 x 77, 384 = 3 x 128 rows).  The single grouped forms: GROUPS"""
    Hout, Wout = _geometry(row)["out_hw"]
    hw, Cout = Hout * Wout, CHANNELS[row["chan"]][2]
    rep = SHARED.get(row["epi"], 1)
    if row["epi"] in GROUPS:
        return [GROUPS[row["epi"]]]
    if "Ns" in GEOMS[row["geom"]]:
        return [[max(rep, n // rep * rep) for n in ns] for ns in GEOMS[row["geom"]]["Ns"]]
    if rep > 1:
        out = [[rep], [2 * rep]]
        if 2 * rep * hw * Cout < nm.CONV_MIN_ELEMENTS:
            big = -(-nm.CONV_MIN_ELEMENTS // (hw * Cout * rep)) * rep
            if big <= 160:
                out.append([big])
        return out
    if row["epi"] == "grouped":
        gran = 256 if row["tile"] == "t320" else 128
        unit = gran // math.gcd(gran, hw)
        return [[unit, 2 * unit]] if unit * 3 * hw <= 1024 else [[unit, unit]]
    out = [[1], [3]]
    if 3 * hw * Cout < nm.CONV_MIN_ELEMENTS:
        big = -(-nm.CONV_MIN_ELEMENTS // (hw * Cout))
        if big <= 160:
            out.append([big])
    return out


def twin_of(row):
    """the variant the existing tests require the row's tile to equal bit for bit (test_conv_gemm_small_tile_equals_default_tile,
    ..._eight_wave_tile_equals_four_wave_tile, ..._big_tile_equals_small_tile): the 4-wave 128-pixel tile, same K order and slices"""
    if row["tile"] == "t4w" or row["epi"] in GN_PART:
        return None
    return dict(row, tile="t4w", stages=2)


def run_row(row):
    fails = []
    rid = row_id(row)
    for i, Ns in enumerate(sample_counts(row)):
        cases = make_cases(row, Ns, seed=1000 * TABLE.index(row) + 31 * i)
        r = launch(row, cases)
        tag = f"conv {rid} N={'+'.join(map(str, Ns))}"
        print(f"numerics: {tag}: ran {r['desc']}", flush=True)
        fails += [f"{tag}: {p}" for p in r["problems"]]
        a = 0
        for gi, c in enumerate(cases):
            n = c["N"]
            check(fails, tag + (f" group {gi}" if len(cases) > 1 else ""), row, c, r["y"][a:a + n], None if r["lo"] is None else r["lo"][a:a + n])
            a += n
        if (row["geom"], row["tile"], row["epi"]) == ZERO_SCALE:          # conditioning_scale = 0: the device scalar at 0.0
            z = launch(row, cases, dev_scale=0.0)
            zero = bool((z["y"] == 0).all()) and bool(torch.isfinite(z["y"]).all())
            print(f"numerics: {tag}: device scale 0.0: every element == 0 and finite: {zero}", flush=True)
            fails += [f"{tag} (device scale 0.0): {p}" for p in z["problems"]]
            if not zero:
                fails.append(f"{tag}: device scale 0.0 leaves {int((z['y'] != 0).sum())} elements that are not 0, {int((~torch.isfinite(z['y'])).sum())} not finite")
        tw = twin_of(row)
        if tw is not None and "non-square" in row_classes(row):
            r2 = launch(tw, cases)
            same = torch.equal(r["y"], r2["y"]) and (r["lo"] is None or torch.equal(r["lo"], r2["lo"]))
            print(f"numerics: {tag}: bit-identical to the 4-wave 128-pixel tile: {same}", flush=True)
            fails += [f"{tag} (twin): {p}" for p in r2["problems"]]
            if not same and T.RECORD is None:
                fails.append(f"{tag}: differs from the 4-wave 128-pixel tile ({nm.differs(r['y'], r2['y'], count=True)} elements)")
    return fails


@pytest.mark.parametrize("row", TABLE, ids=row_id)
def test_conv_gemm_on_odd_geometries(row):
    """one table row: N = 1 and N = 3 (and a larger N where those are small), guards, kernel identity, misrounded share, row_err bars,
    bit identity with the 4-wave tile on the non-square rows"""
    done(run_row(row))


def test_table_coverage_is_printed():
    """every (form, geometry class) pair that can exist is met (asserted at import); the matrix, for the log - and how many of the
    launches judged so far in this process had the device library's unfold + mm among their baselines: a run in which the library
    offered it for none (an older torch without torch.mm(out_dtype=)) ends with a warning in the summary, not only with log lines"""
    import warnings
    matrix, missing = coverage()
    d = DEVICE_BASELINE
    print(f"test_conv_gpu: {len(TABLE)} rows\n{matrix}\ndevice unfold + mm baseline: in {d['ran']} judged launches, left out of {d['left_out']}")
    assert not missing
    if d["left_out"]:
        warnings.warn(f"test_conv_gpu: the device unfold + mm baseline was left out of {d['left_out']} of {d['ran'] + d['left_out']} judged launches")


def report_rows():
    """python -m tests.numerics --report: run every row without asserting, return the records"""
    del RECORD[:]
    DEVICE_BASELINE.update(ran=0, left_out=0)
    for row in TABLE:
        run_row(row)
    return list(RECORD)


@pytest.mark.parametrize("h,w", [(16, 24), (24, 16)])
def test_one_non_square_step_through_the_model(h, w):
    """The pipeline takes h and w apart from the condition images: one denoising step at non-square latents through the tiny UNet and
    ONE ControlNet (the six-net form's fusion blocks carry LayerNorm planes of a fixed square size), StepRunner.step_nchw against
    oracle.sd15_oracle.denoise_step - the bound test_engine_gpu.py applies to the square step.  A layer that cannot run non-square
    has to refuse with an error text; a wrong image is the failure this looks for."""
    from oracle import sd15_oracle as O
    from edgestyle_amd import config as C, lib
    from edgestyle_amd.models import StepRunner, UNet2DConditionModel, ControlNetModel
    from tests.helpers import make_weights, quantize
    ucfg, vcfg = C.tiny_unet(), C.tiny_vae()
    ws = {k: quantize(v) for k, v in make_weights(ucfg, vcfg, seed=0).items()}
    g = torch.Generator().manual_seed(100 * h + w)
    N, c0 = 2, ucfg.block_out_channels[0]
    x = torch.randn(N, 4, h, w, generator=g).half().float()
    ehs = (torch.randn(N, 77, ucfg.cross_attention_dim, generator=g) * 0.5).half().float()
    cond = (torch.randn(N, c0, h, w, generator=g) * 0.3).half().float()
    ref = O.denoise_step(ws["unet"], ucfg, None, [(ws["openpose"], ucfg)], x, 501, ehs, [cond], [0.8])
    assert ref.shape == (N, 4, h, w)
    unet = UNet2DConditionModel(ws["unet"], ucfg, torch.float16).to(DEV)
    runner = StepRunner(unet, ControlNetModel(ws["openpose"], ucfg, torch.float16).to(DEV))
    try:
        out = runner.step_nchw(x.to(DEV), 501, ehs.to(DEV), [cond.to(DEV)], [0.8])
    except lib.EdgeStyleHipError as e:                       # a refusal is a legitimate outcome; it must say what it refuses
        assert len(str(e)) > 20, str(e)
        pytest.fail(f"the engine refuses {h} x {w} latents: {e}")
    torch.cuda.synchronize()
    assert out.shape == ref.shape
    err = float((out.float().cpu() - ref).abs().max())
    rel = err / float(ref.abs().max())
    print(f"numerics: one step at {h} x {w} latents, one ControlNet: max abs err {err:.3e}, relative to the reference's largest value {rel:.3e}")
    assert err < 2e-2 and rel < 1e-2, (err, rel)

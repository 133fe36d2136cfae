"""The route's answer is the kernel that runs: es_conv_gemm_route / es_linear_xs_route (what the library says it would launch, asked
without a launch) against es_conv_gemm_last_kernel / es_linear_xs_last_form (what the launcher instantiated, written from its own
template arguments) after a real launch of the same descriptor.  Outputs are not judged here - tests/test_conv_gpu.py and
tests/test_linear_xs_gpu.py do that; every operand is a zero-filled buffer of the size the descriptor states."""
import ctypes

import pytest
import torch

from edgestyle_amd import lib
from tests import numerics as nm

pytestmark = pytest.mark.gpu

DEV = "cuda"
SILU = lib.ACT_SILU
# (name, descriptor fields, what the kernel id must unpack to: bn, pixels per workgroup, ring depth, waves), each on every channel set it fits
GEMM_CASES = [
    ("bn 64", dict(bn=64), (64, 64, 2, 4)),
    ("bn 128, 4 waves", dict(bn=128, waves=4), (128, 128, 2, 4)),
    ("bn 128, 8 waves, 4 stages", dict(bn=128, waves=8, stages=4), (128, 128, 4, 8)),
    ("bn 160", dict(bn=160), (160, 128, 2, 4)),
    ("bn 320 taken", dict(bn=320), (320, 256, 2, 8)),
    ("bn 320 refused (SiLU) -> 160", dict(bn=320, act=SILU), (160, 128, 2, 4)),
    ("bn 256 with the LayerNorm fold", dict(bn=256, ln=True), (256, 256, 2, 8)),
    ("bn 256 refused (SiLU) -> 128", dict(bn=256, act=SILU), (128, 128, 2, 4)),
    ("split-K 2, plain reduce", dict(bn=160, splitk=2), (160, 128, 2, 4)),
    ("split-K 2, GroupNorm hand-over", dict(bn=160, splitk=2, gn=True), (160, 128, 2, 4)),
    ("split-K 2 on the 256-pixel kernel, GroupNorm hand-over", dict(bn=320, splitk=2, gn=True, act=SILU), (320, 256, 2, 8)),
]
CHANNELS = {"64>64": (64, 0, 64, 3), "128+64>320": (128, 64, 320, 3), "K=64->256": (64, 0, 256, 1)}       # C1, C2, Cout, ksize


def _zeros(numel, dtype):
    return torch.zeros(max(int(numel), 1) + 64, dtype=dtype, device=DEV)


def gemm_launch(case, chan, M, dt):
    """(descriptor, the tensors it points to) of one case, or None where the case cannot take these channels or this M"""
    C1, C2, Cout, ksize = CHANNELS[chan]
    ln, gn, splitk = case.get("ln", False), case.get("gn", False), case.get("splitk", 1)
    # the fold is a plain linear layer; the hand-over needs whole 64-pixel blocks, and is run where Cout fills its N tiles, as the model's do
    if ln != (ksize == 1) or (gn and (M % 64 or Cout % 160)):
        return None
    bn = case["bn"]
    d, keep = lib.GemmDesc(), {}

    def buf(name, numel, dtype=dt):
        keep[name] = _zeros(numel, dtype)
        setattr(d, name, keep[name].data_ptr())
    d.N, d.Hsrc, d.Wsrc, d.Hout, d.Wout, d.C1, d.C2, d.Cout = 1, M, 1, M, 1, C1, C2, Cout
    d.rows_padded, d.Kpad = -(-Cout // bn) * bn, ksize * ksize * (C1 + C2)
    d.ksize, d.stride, d.pad, d.act, d.splitk, d.bn = ksize, 1, ksize // 2, case.get("act", 0), splitk, bn
    d.stages, d.waves, d.out_scale, d.ln_eps, d.gn_groups = case.get("stages", 0), case.get("waves", 0), 1.0, 1e-5, 32
    d.dtype = lib.ES_F16 if dt == torch.float16 else lib.ES_BF16
    buf("x", M * C1), buf("w", d.rows_padded * d.Kpad), buf("bias", d.rows_padded, torch.float32), buf("out", M * Cout)
    if C2:
        buf("x2", M * C2)
    if ln:
        buf("ln_colsum", d.rows_padded, torch.float32)
    if splitk > 1:
        buf("workspace", lib.load().es_conv_gemm_workspace_bytes(ctypes.byref(d)) // 4, torch.float32)
    if gn:
        buf("gn_part", 2 * (M // 64) * 32 * 2, torch.float32)
    return d, keep


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_conv_gemm_route_names_the_kernel_that_runs(dt):
    """es_conv_gemm at every tile request of GEMM_CASES - the 64-wide tile, 128 on 4 waves and on 8 with a ring of 4, 160, 320 and 256
    where the phase-interleaved kernel takes the launch and where it does not, split-K with both reduce forms - at 256 and 257 pixels
    on every channel set the case fits: the id the route gives is the id the launcher wrote, it unpacks to the tile the case names,
    and the mirror gives the same id."""
    L, ran = lib.load(), 0
    for name, case, (bn, bm, stages, waves) in GEMM_CASES:
        for chan in CHANNELS:
            for M in (256, 257):
                made = gemm_launch(case, chan, M, dt)
                if made is None:
                    continue
                d, keep = made
                r = lib.gemm_route(d)
                lib.check(L.es_conv_gemm(ctypes.byref(d), None), "es_conv_gemm")
                torch.cuda.synchronize()
                last, tag = L.es_conv_gemm_last_kernel(), (name, chan, M)
                assert last == r["kernel"] == nm.gemm_route(d)["kernel"], (tag, last, r)
                f = lib.gemm_kernel_fields(last)
                assert (f["bn"], f["bm"], f["stages"], f["waves"], f["ln"], f["bf16"]) == \
                    (bn, bm, stages, waves, case.get("ln", False), dt == torch.bfloat16), (tag, f)
                assert (r["family"], r["reduce"]) == (int(bm == 256), 0 if case.get("splitk", 1) == 1 else 2 if case.get("gn") else 1), (tag, r)
                ran += 1
    assert ran == 8 * 2 * 2 + 2 * 1 * 1 + 1 * 1 * 2     # cases x channel sets x M: eight plain ones, two hand-overs (320 couts, M = 256), the fold


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_linear_xs_route_names_the_form_that_runs(dt):
    """es_linear_xs at M = 256 and 257, K = 320 and 640, every form (nm.XS_FORMS: plain, LayerNorm fold, GEGLU, both, residual, GroupNorm
    in front; one-barrier and ping-pong under es_linear_xs_set_pp): the form the route gives is the form the launcher wrote."""
    L, forms = lib.load(), set()
    first = L.es_linear_xs_set_pp(1)
    try:
        for K, kind, pp in nm.XS_FORMS:
            for M in (256, 257):
                if kind == "gn" and M % 256:
                    continue
                geglu, Cout = kind.startswith("geglu"), 256
                d = lib.XsDesc()
                keep = dict(x=_zeros(512 * K, dt), w=_zeros(Cout * K, dt), bias=_zeros(Cout, torch.float32), out=_zeros(512 * Cout, dt),
                            residual=_zeros(512 * Cout, dt), gn_part=_zeros(4 * 32 * 2, torch.float32), gn_gamma=_zeros(K, torch.float32),
                            gn_beta=_zeros(K, torch.float32))
                d.x, d.w, d.bias, d.out = (keep[k].data_ptr() for k in ("x", "w", "bias", "out"))
                d.M, d.K, d.Cout, d.rows_padded, d.ldo = M, K, Cout, Cout, Cout // 2 if geglu else Cout
                d.geglu, d.ln, d.ln_eps, d.dtype = int(geglu), int(kind in ("ln", "geglu_ln")), 1e-5, lib.ES_F16 if dt == torch.float16 else lib.ES_BF16
                d.nslices, d.chunks_per_slice = 1, Cout // (64 if K == 320 else 32)
                if kind == "res":
                    d.residual = keep["residual"].data_ptr()
                if kind == "gn":
                    d.gn_part, d.gn_gamma, d.gn_beta = (keep[k].data_ptr() for k in ("gn_part", "gn_gamma", "gn_beta"))
                    d.gn_groups, d.gn_nchunk, d.gn_hw, d.gn_eps = 32, 4, 256, 1e-6
                L.es_linear_xs_set_pp(pp)
                r = lib.xs_route(d)
                lib.check(L.es_linear_xs(ctypes.byref(d), None), "es_linear_xs")
                torch.cuda.synchronize()
                assert L.es_linear_xs_last_form() == r["form"] == nm.xs_form_id(K, kind, pp) == nm.xs_route(d, pp)["form"], (K, kind, pp, M, r)
                assert r["grid"] == -(-M // 256) and r["runs"] == 1
                forms.add(r["form"])
    finally:
        L.es_linear_xs_set_pp(first)
    assert len(forms) == 16

"""splitk_reduce_kernel (csrc/gemm_conv.hip): the S fp32 slabs of a split-K launch are summed strictly in slice order, whatever the number
of slices whose loads the kernel keeps in flight (batches of four and a one-by-one remainder today).

One 1x1 layer with forced split-K: M = 70 rows (2 samples of 5 x 7: ragged against every pixel tile, the time-embedding row changes inside
a tile), K = 2048 = 32 K tiles, so every S <= 32 can be forced.  S = 2, 5, 8, 9, 17, 32: fewer slices than one batch, every remainder of
batches of 4, 8 and 16, and the maximum.  Cout = 320 (five N tiles of 64), 24 (three whole 16-byte chunks in a 64-wide tile) and 20
(Cout % 8 != 0: every thread on the element-wise loads and stores, the last chunk with 4 valid channels).  Plain (no bias, no time
embedding, no residual, scale 1) and full (all three, scale 0.7); fp16 and bf16.

The expected value is computed HERE from what the GEMM wrote: the workspace is filled with NaN before the launch, the S slabs are read back
from it afterwards (the reduce kernel leaves them as they are) and summed in numpy float32 in slice order, starting from +0 as the kernel
does; then the documented epilogue - ((v + bias) + temb) * scale, round to the storage dtype, + residual, round - and the output must
equal that in every bit.  (fp16 with a scale: the product is rounded to fp16 ONCE, from its exact value - the compiler's fused
multiply-and-convert; rounding it to fp32 first differs in about one element in 10^4.)  The workspace past the launch's own
S x M x rows_padded floats must still be NaN (no store ran over) and the output holds no NaN (no LOAD ran over: slab S would be one).
The same launch runs twice and must repeat bit for bit, and is held to the fp64 bars tests/test_conv_gpu.py uses (row_err against base_alg
and base_ref through judge)."""
import numpy as np
import pytest
import torch

from tests import numerics as nm
from tests import test_numerics_gpu as T
from tests.test_numerics_gpu import judge, done

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, H, W, K = 2, 5, 7, 2048
M = N * H * W
_CASES, _REFS = {}, {}


def case_of(cout, full, dtype):
    key = (cout, full, dtype)
    if key not in _CASES:
        _CASES[key] = nm.conv_case(N, H, W, K, cout, dtype, k=1, temb=full, residual=full, bias=full, scale=0.7 if full else 1.0,
                                   seed=cout + 2 * int(full))
        ref = nm.conv_ref64(_CASES[key])
        _REFS[key] = (ref, nm.row_err(nm.conv_base_ref(_CASES[key]), ref))
    return _CASES[key], _REFS[key]


def expected_from_slabs(slabs, c, dtype):
    """slabs [S, M, Cout] fp32 (numpy) -> the output the reduce kernel must store, as fp32 [M, Cout]"""
    f32 = np.float32
    v = np.zeros(slabs.shape[1:], dtype=f32)
    for z in range(slabs.shape[0]):
        v = v + slabs[z]
    bias = np.zeros(slabs.shape[2], dtype=f32) if c["b"] is None else c["b"].numpy().astype(f32)
    temb = np.zeros((N, slabs.shape[2]), dtype=f32) if c["temb"] is None else c["temb"].numpy().astype(f32)
    x = (v + bias[None, :]) + np.repeat(temb, H * W, axis=0)
    assert x.dtype == f32
    if dtype == torch.float16:
        # hipcc forms round16(x * scale) as ONE v_fma_mixlo_f16: the exact product rounded once to fp16 (no fp32 rounding in between).  The
        # product of two fp32 values is exact in fp64, and numpy converts fp64 to fp16 directly with one rounding.
        y = torch.from_numpy((x.astype(np.float64) * np.float64(f32(c["scale"]))).astype(np.float16).astype(f32))
    else:
        y = nm.rnd(torch.from_numpy(x * f32(c["scale"])), dtype)
    if c["res"] is not None:
        y = nm.rnd(torch.from_numpy(y.numpy() + c["res"].reshape(M, -1).numpy().astype(f32)), dtype)
    return y


@pytest.mark.parametrize("dtype", T.DTYPES, ids=T._name)
@pytest.mark.parametrize("full", [False, True], ids=["plain", "bias-temb-res-scale"])
@pytest.mark.parametrize("S", [2, 5, 8, 9, 17, 32])
@pytest.mark.parametrize("cout", [24, 320, 20])
def test_splitk_reduce_sums_the_slabs_in_slice_order(cout, S, full, dtype):
    from edgestyle_amd import ops
    c, (ref, e_ref) = case_of(cout, full, dtype)
    name = f"splitk reduce Cout{cout} S{S} {'full' if full else 'plain'} {T._name(dtype)}"
    pw = ops.pack_weight(c["w"], c["b"], dtype, DEV)
    rp = pw.rows_padded
    need = S * M * rp
    x = c["x"].to(DEV, dtype)
    ws = ops._get_workspace(need * 4, x.device)
    assert ws.numel() > need
    ws.fill_(float("nan"))
    out = torch.full((N, H, W, cout), float("nan"), dtype=dtype, device=DEV)
    kw = dict(out=out, splitk=S)
    if full:
        table = torch.zeros(N, cout + 64, dtype=dtype, device=DEV)         # a slice of a wider table, as the engine passes it
        table[:, 64:] = c["temb"].to(DEV, dtype)
        kw.update(temb=table[:, 64:], residual=c["res"].to(DEV, dtype), out_scale=c["scale"])
    y = ops.conv_gemm(x, pw, **kw)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr() and ops._get_workspace(need * 4, x.device) is ws
    got = out.float().cpu().reshape(M, cout)
    slabs = ws[:need].view(S, M, rp)[:, :, :cout].cpu()
    fails = []
    if not bool(torch.isfinite(slabs).all()):
        fails.append(f"{name}: {int((~torch.isfinite(slabs)).sum())} slab values never written - the launch did not run with {S} slices")
    if not bool(torch.isnan(ws[need:]).all()):
        fails.append(f"{name}: the workspace behind slab {S - 1} was written")
    if not bool(torch.isfinite(got).all()):
        fails.append(f"{name}: {int((~torch.isfinite(got)).sum())} outputs not finite (never written, or a slab index past {S - 1} was read)")
    want = expected_from_slabs(slabs.numpy(), c, dtype)
    diff = nm.differs(got, want, count=True)
    print(f"{name}: {diff} of {got.numel()} elements differ from the slice-ordered fp32 sum of the slabs read back")
    if diff:
        fails.append(f"{name}: {diff} elements differ from the slice-ordered sum of the slabs + the documented epilogue")
    y2 = torch.full_like(out, float("nan"))
    ops.conv_gemm(x, pw, **dict(kw, out=y2))
    torch.cuda.synchronize()
    if not torch.equal(y2.float().cpu().reshape(M, cout), got):
        fails.append(f"{name}: the same launch twice differs")
    e_alg = nm.row_err(nm.conv_base_alg(c, 8, S), ref)
    judge(fails, name, got.reshape(N, H, W, cout), ref, e_alg, e_ref, dtype)
    done(fails)

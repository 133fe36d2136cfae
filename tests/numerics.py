"""Numerics at trained-model statistics: input generators, a per-row error metric and CPU baselines.

The kernel tests in test_ops_gpu.py feed randn activations and judge by max|y - ref| / max|ref| over the whole tensor.  Both hide
the mistakes this code base is most exposed to: the folds form variances in one pass (E[x^2] - mean^2) and cancel
`x W'^T - mean colsum(W')` by a factor mean / sigma, real token streams have |mean| / sigma of 10-30 per token and a few channels
two orders of magnitude above the rest, and one loud row sets the denominator of a whole-tensor metric.

This module is plain Python (no fixtures):

* generators (seeded, CPU, values rounded through the storage dtype before anything else sees them) that ASSERT their own
  postconditions: `token_rows`, `group_maps`, `spike_and_sea`, `late_risers`, `common_shift`, `one_loud_query`, `loud_values`,
  `last_key_decides`;
* `row_err(y, ref64)`: max over rows r and columns c of |y[r, c] - ref64[r, c]| / rms_c(ref64[r, :]) - every row is its own scale;
* for every operation three CPU computations on the SAME rounded inputs and rounded weights:
    `*_ref64`     the plain operation in fp64 (the truth),
    `*_base_ref`  the textbook op sequence in fp32 with every op's output rounded to the storage dtype (what the reference
                  computes under fp16 autocast),
    `*_base_alg`  the algorithm the kernel is DESIGNED to run, in fp32 (one-pass variance, the folded forms, a lazily raised
                  softmax reference) - with an optional planted `defect`, for the tests that show the bars have teeth.

Bars (tests/test_numerics_gpu.py): row_err(kernel) <= MARGIN * row_err(base_alg) always; in the required tier (ratio <= 30,
outlier gain <= 100, peak <= 2e4) also row_err(kernel) <= MARGIN * row_err(base_ref).  MARGIN = 2 separates "rounds in a different
order" from "lost a bit or more" and is not tuned per case.  In the probe tier (ratio 100, 300) only the first bar holds, with
PROBE_MARGIN = 4: there the error is cancellation noise whose size depends on the order of summation.

The implicit-GEMM convolution has a metric of its own, the misrounded share (`misrounded`, `conv_case`, `conv_ref64`, `conv_base_ref`,
`conv_base_alg`, further down): an extra rounding inside the launch is invisible to row_err and plain to it.

`python -m tests.numerics --report` (GPU) runs the cases of test_numerics_gpu.py and the convolution sweep of test_conv_gpu.py and writes
the measured tables to tests/NUMERICS.md (`--only conv`: the convolution table alone; `--only fusion`, `--only sampler`, `--only attention`,
`--only norm`, `--only xs`: the sweep of test_fusion_gpu.py, the trajectories of test_sampler_gpu.py, the rows of test_attention_gpu.py, of
test_norm_gpu.py or of test_linear_xs_gpu.py alone).

The fusion block (`fusion_case`, `fusion_ref64`, `fusion_base_ref`, `fusion_base_alg`, `fusion_grids`; judged per SAMPLE, `sample_err`) and the
sampler step (`unipc_apply`, `ddim_apply`, `run_trajectory`, `traj_err`) have sections of their own at the end.
"""
import math

import torch
import torch.nn.functional as F

from edgestyle_amd.lib import EdgeStyleHipError

MARGIN = 2.0
PROBE_MARGIN = 4.0
LAZY = 8.0                      # csrc/attention.hip: the running softmax reference may sit up to 2^8 below the true maximum
REQUIRED_RATIOS = (0, 3, 10, 30)
PROBE_RATIOS = (100, 300)
FP16_NORMAL_MIN_LOG2 = -14


def rnd(x: torch.Tensor, dtype) -> torch.Tensor:
    """x rounded to the storage dtype (round to nearest even, subnormals kept), returned in fp32"""
    return x.to(torch.float32).to(dtype).to(torch.float32)


# ----------------------------------------------------------------------------------------------------------------
# metric
# ----------------------------------------------------------------------------------------------------------------
def row_err(y: torch.Tensor, ref64: torch.Tensor, both: bool = False):
    """max over rows r, columns c of |y[r, c] - ref64[r, c]| / rms_c(ref64[r, :]); rows = everything but the last dimension (tokens,
    pixels, (sample, head, query)).  No row is left out and no row may have a reference rms of 0.  both=True: also the row-rms
    variant max_r rms_c(y - ref64) / rms_c(ref64) (for the report).  A non-finite y gives inf."""
    r = ref64.detach().to("cpu", torch.float64).reshape(-1, ref64.shape[-1])
    v = y.detach().to("cpu", torch.float64).reshape(-1, ref64.shape[-1])
    assert r.shape == v.shape, (r.shape, v.shape)
    rms = r.pow(2).mean(dim=1).sqrt()
    assert bool((rms > 0).all()) and bool(torch.isfinite(rms).all()), "a reference row with rms 0 (or not finite): fix the generator"
    d = (v - r).abs()
    if not bool(torch.isfinite(d).all()):
        return (float("inf"), float("inf")) if both else float("inf")
    e_max = float((d.max(dim=1).values / rms).max())
    if not both:
        return e_max
    return e_max, float((d.pow(2).mean(dim=1).sqrt() / rms).max())


def old_metric(y: torch.Tensor, ref: torch.Tensor) -> float:
    """the whole-tensor metric of test_ops_gpu.py (rel_err): max|y - ref| / max|ref|"""
    a, b = y.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-6))


def finite_where_representable(y: torch.Tensor, ref64: torch.Tensor, dtype) -> bool:
    """Overflow bar: wherever ref64 rounded to the storage dtype is finite, y is finite."""
    ok = torch.isfinite(ref64.detach().cpu().to(torch.float32).to(dtype).float())
    return bool(torch.isfinite(y.detach().cpu().float())[ok].all())


# ----------------------------------------------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _outlier_gains(C, frac, gain, g):
    """per-channel gain: `frac` of the channels (a fixed set, as in a trained model) carry `gain` (a number, or a (lo, hi) range
    drawn uniformly) times the standard deviation of the rest"""
    gains = torch.ones(C, dtype=torch.float64)
    n = int(round(frac * C)) if frac > 0 else 0
    if n:
        idx = torch.randperm(C, generator=g)[:n]
        lo, hi = (gain, gain) if not isinstance(gain, (tuple, list)) else gain
        gains[idx] = lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)
    return gains


def ratio_tolerance(ratio, dtype) -> float:
    """+-10 % of the nominal |mean| / std; bf16 cannot hold a ratio of 300 that well after rounding (8 significant bits on values
    300 standard deviations from 0): +-35 % there only"""
    return 0.35 if (dtype == torch.bfloat16 and ratio >= 300) else 0.10


def measured_ratio(x: torch.Tensor, dim=-1) -> torch.Tensor:
    x = x.double()
    return x.mean(dim=dim).abs() / x.std(dim=dim, unbiased=False)


def token_rows(M, C, ratio, outlier_frac=0.0, outlier_gain=(50.0, 100.0), peak=4.0, dtype=torch.float16, seed=0):
    """[M, C] fp32 tensor of dtype-rounded values: every row's actual |mean| / std (fp64, on the rounded values) lies within
    ratio_tolerance() of `ratio` (ratio 0: below 0.05), a fixed `outlier_frac` of the channels carries `outlier_gain` times the
    spread of the rest, and max|x| == peak (up to rounding).  Rows are standardised AFTER the outlier channels have been scaled and
    then shifted (sign per row): adding a constant to randn * sigma instead leaves a heavy-tailed row std and ratios spread by 4x."""
    g = _gen(seed)
    x = torch.randn(M, C, generator=g, dtype=torch.float64) * _outlier_gains(C, outlier_frac, outlier_gain, g)
    x = (x - x.mean(dim=1, keepdim=True)) / x.std(dim=1, unbiased=False, keepdim=True)
    sign = torch.where(torch.rand(M, 1, generator=g) < 0.5, -1.0, 1.0).double()
    x = x + sign * float(ratio)
    x = x * (float(peak) / float(x.abs().max()))
    x = rnd(x, dtype)
    r = measured_ratio(x)
    tol = ratio_tolerance(ratio, dtype)
    if ratio == 0:
        assert float(r.max()) < 0.05, float(r.max())
    else:
        assert float(r.min()) >= ratio * (1 - tol) and float(r.max()) <= ratio * (1 + tol), (ratio, float(r.min()), float(r.max()))
    assert abs(float(x.abs().max()) / peak - 1) < 2 ** -7 and bool(torch.isfinite(x).all())
    return x


def group_maps(N, C, H, groups, ratio, outlier_frac=0.0, outlier_gain=(50.0, 100.0), peak=4.0, dtype=torch.float16, seed=0,
               dominant_channel=False, W=None):
    """[N, H, W, C] (NHWC) fp32 tensor of dtype-rounded values: every (sample, group)'s |mean| / std over its H * W * C / groups values
    is within ratio_tolerance() of `ratio`.  dominant_channel: ONE channel of every group holds >= 90 % of the group's variance
    (that fraction is asserted) - the group statistics are then those of a single channel."""
    g = _gen(seed)
    W = W or H
    cpg = C // groups
    gains = _outlier_gains(C, outlier_frac, outlier_gain, g)
    if dominant_channel:
        gains = torch.ones(C, dtype=torch.float64)
        gains[torch.arange(groups) * cpg + torch.randint(0, cpg, (groups,), generator=g)] = 10.0 * math.sqrt(cpg)
    x = torch.randn(N, H * W, C, generator=g, dtype=torch.float64) * gains
    xg = x.reshape(N, H * W, groups, cpg)
    xg = (xg - xg.mean(dim=(1, 3), keepdim=True)) / xg.std(dim=(1, 3), unbiased=False, keepdim=True)
    sign = torch.where(torch.rand(N, 1, groups, 1, generator=g) < 0.5, -1.0, 1.0).double()
    xg = xg + sign * float(ratio)
    xg = xg * (float(peak) / float(xg.abs().max()))
    x = rnd(xg.reshape(N, H, W, C), dtype)
    xs = x.double().reshape(N, H * W, groups, cpg)
    r = xs.mean(dim=(1, 3)).abs() / xs.std(dim=(1, 3), unbiased=False)
    tol = ratio_tolerance(ratio, dtype)
    if ratio == 0:
        assert float(r.max()) < 0.05, float(r.max())
    else:
        assert float(r.min()) >= ratio * (1 - tol) and float(r.max()) <= ratio * (1 + tol), (ratio, float(r.min()), float(r.max()))
    if dominant_channel:
        dev = (xs - xs.mean(dim=(1, 3), keepdim=True)).pow(2).sum(dim=1)            # [N, groups, cpg]: each channel's part of the group's
        assert float((dev.max(dim=-1).values / dev.sum(dim=-1)).min()) >= 0.9       # squared deviations from the group mean
    assert bool(torch.isfinite(x).all())
    return x


def _unit(shape, g):
    u = torch.randn(*shape, generator=g, dtype=torch.float64)
    return u / u.norm(dim=-1, keepdim=True)


def _softmax64(q, k, heads, scale=None):
    """fp64 logits (natural units) [N, heads, Sq, Skv] of the [N, S, heads * d] layouts"""
    N, Sq, Cc = q.shape
    d = Cc // heads
    qh = q.double().reshape(N, Sq, heads, d).transpose(1, 2)
    kh = k.double().reshape(N, -1, heads, d).transpose(1, 2)
    return qh @ kh.transpose(-1, -2) * (scale if scale is not None else 1.0 / math.sqrt(d))


def spike_and_sea(N, heads, Sq, Skv, d, spread_log2, dtype=torch.float16, seed=0, control=False):
    """q, k [N, S, heads * d], v: for >= 90 % of the (sample, head, query) rows of the fp64 softmax one key holds the maximum, every
    other key's weight is below 2^-14 of it (the fp16 normal range) and the other keys together - the sea - hold between 2.5 % and
    50 % of the mass; the sea's V carries a common offset (+1.5 against -1.5 for the spike), so losing the sea moves the output.
    control=True: the same construction with a sea mass below 1 % asserted instead (a tail that is negligible)."""
    assert Skv >= 1024
    g = _gen(seed)
    u = _unit((N, 1, heads, d), g)
    q = math.sqrt(d) * u + 0.05 * torch.randn(N, Sq, heads, d, generator=g, dtype=torch.float64)
    k = 0.05 * torch.randn(N, Skv, heads, d, generator=g, dtype=torch.float64)
    v = torch.randn(N, Skv, heads, d, generator=g, dtype=torch.float64) + 1.5
    pos = torch.randint(0, Skv, (N, heads), generator=g)
    ni, hi = torch.meshgrid(torch.arange(N), torch.arange(heads), indexing="ij")
    k[ni, pos, hi] = u[:, 0] * (spread_log2 * math.log(2.0))
    v[ni, pos, hi] = v[ni, pos, hi] - 3.0
    q, k, v = (rnd(t.reshape(N, -1, heads * d), dtype) for t in (q, k, v))
    s = _softmax64(q, k, heads)
    top2 = s.topk(2, dim=-1).values
    gap_log2 = (top2[..., 0] - top2[..., 1]) / math.log(2.0)
    w = torch.softmax(s, dim=-1)
    sea = 1.0 - w.max(dim=-1).values
    if control:
        assert float(sea.median()) < 0.01, float(sea.median())
    else:
        ok = (gap_log2 > -FP16_NORMAL_MIN_LOG2) & (sea >= 0.025) & (sea <= 0.5)
        assert float(ok.double().mean()) >= 0.9, (float(ok.double().mean()), float(gap_log2.min()), float(sea.median()))
    assert bool((s.argmax(dim=-1) == pos[:, :, None]).all())
    return q, k, v


def late_risers(N, heads, Sq, Skv, d, tile=64, step_log2=10.0, dtype=torch.float16, seed=0):
    """The per-key-tile maximum of every query rises by about `step_log2` from one tile of `tile` keys to the next, for at least four
    tiles (asserted in fp64: every rise within 2 of step_log2): the running reference is re-raised and the accumulators rescaled
    again and again."""
    g = _gen(seed)
    ntile = Skv // tile
    assert ntile >= 5
    u = _unit((N, 1, heads, d), g)
    q = math.sqrt(d) * u + 0.1 * torch.randn(N, Sq, heads, d, generator=g, dtype=torch.float64)
    k = 0.3 * torch.randn(N, Skv, heads, d, generator=g, dtype=torch.float64)
    k = k - (k * u).sum(dim=-1, keepdim=True) * u                       # the calm keys carry nothing along u
    rises = min(ntile - 1, 6)
    for t in range(1, rises + 1):
        p = t * tile + int(torch.randint(0, tile, (1,), generator=g))
        k[:, p] = k[:, p] + u[:, 0] * (t * step_log2 * math.log(2.0) + 2.0)
    v = torch.randn(N, Skv, heads, d, generator=g, dtype=torch.float64)
    q, k, v = (rnd(t.reshape(N, -1, heads * d), dtype) for t in (q, k, v))
    s = _softmax64(q, k, heads) / math.log(2.0)
    tm = s[..., :ntile * tile].reshape(N, heads, Sq, ntile, tile).max(dim=-1).values
    inc = tm[..., 1:rises + 1] - tm[..., :rises]
    assert rises >= 4 and float((inc[..., 1:] - step_log2).abs().max()) < 2.0 and float(inc[..., 0].min()) > 3.0, \
        (float(inc.min()), float(inc.max()))
    return q, k, v


def common_shift(N, heads, Sq, Skv, d, shift=300.0, dtype=torch.float16, seed=0):
    """randn q, k, v plus a shared q / k component that moves ALL logits of a query by `shift` (+ or -): softmax does not care, the
    kernel's first-tile reference has to absorb it.  The component sits in one coordinate with values exact in bf16, so the shift is
    common to every key exactly.  Asserted: every query's logits have |mean| within 5 % of |shift| and (from 8 keys on) a spread that
    stays O(1)."""
    g = _gen(seed)
    q = torch.randn(N, Sq, heads, d, generator=g, dtype=torch.float64)
    k = torch.randn(N, Skv, heads, d, generator=g, dtype=torch.float64)
    v = torch.randn(N, Skv, heads, d, generator=g, dtype=torch.float64)
    a = 2.0 ** round(math.log2(math.sqrt(abs(shift) * math.sqrt(d))))
    b = abs(shift) * math.sqrt(d) / a
    b = float(torch.tensor(b).to(torch.bfloat16))                       # exact in both storage dtypes
    q[..., 0] = a * (1.0 if shift > 0 else -1.0)
    k[..., 0] = b
    q, k, v = (rnd(t.reshape(N, -1, heads * d), dtype) for t in (q, k, v))
    s = _softmax64(q, k, heads)
    assert float((s.mean(dim=-1).abs() / abs(shift) - 1).abs().max()) < 0.05
    if Skv >= 8:                # below that the sample spread of a query's few logits says little (and is undefined for one key)
        assert float(s.std(dim=-1).max()) < 3.0
    assert (float(s.mean()) > 0) == (shift > 0)
    return q, k, v


def one_loud_query(N, heads, Sq, Skv, d, wave=32, gain_log2=20.0, dtype=torch.float16, seed=0):
    """One query of every `wave` consecutive queries spikes on a key of a LATE tile (its maximum rises by ~gain_log2 there), the
    others stay calm: the kernels' rescale branch is wave-uniform (__all(calm)), so the calm queries of that wave are rescaled by
    2^0 alongside.  Asserted: exactly the chosen queries have a logit range above gain_log2 - 4, all others below 8."""
    g = _gen(seed)
    q = 0.5 * torch.randn(N, Sq, heads, d, generator=g, dtype=torch.float64)
    k = 0.5 * torch.randn(N, Skv, heads, d, generator=g, dtype=torch.float64)
    v = torch.randn(N, Skv, heads, d, generator=g, dtype=torch.float64)
    u = _unit((d,), g)
    q = q - (q * u).sum(dim=-1, keepdim=True) * u
    k = k - (k * u).sum(dim=-1, keepdim=True) * u
    loud = torch.arange(0, Sq, wave) + torch.randint(0, min(wave, Sq), ((Sq + wave - 1) // wave,), generator=g)
    loud = loud[loud < Sq]
    key = Skv - 1 - int(torch.randint(0, min(16, Skv // 2), (1,), generator=g))
    amp = math.sqrt(gain_log2 * math.log(2.0) * math.sqrt(d))
    q[:, loud] = q[:, loud] + u * amp
    k[:, key] = k[:, key] + u * amp
    q, k, v = (rnd(t.reshape(N, -1, heads * d), dtype) for t in (q, k, v))
    s = _softmax64(q, k, heads) / math.log(2.0)
    rng = s.max(dim=-1).values - s.median(dim=-1).values
    mask = torch.zeros(Sq, dtype=torch.bool)
    mask[loud] = True
    assert float(rng[:, :, mask].min()) > gain_log2 - 4 and float(rng[:, :, ~mask].max()) < 8.0, \
        (float(rng[:, :, mask].min()), float(rng[:, :, ~mask].max()))
    return q, k, v


def loud_values(N, heads, Sq, Skv, d, peak=2.0e4, dtype=torch.float16, seed=0):
    """calm logits (randn q, k) and V scaled so that max|V| == peak: the output is a convex combination of V rows, so every
    intermediate the reference stores stays below peak, and P V must not overflow on the way."""
    g = _gen(seed)
    q = torch.randn(N, Sq, heads * d, generator=g, dtype=torch.float64)
    k = torch.randn(N, Skv, heads * d, generator=g, dtype=torch.float64)
    v = torch.randn(N, Skv, heads * d, generator=g, dtype=torch.float64)
    v = v * (peak / float(v.abs().max()))
    q, k, v = (rnd(t, dtype) for t in (q, k, v))
    assert float(v.abs().max()) <= peak * (1 + 2 ** -8) and bool(torch.isfinite(v).all())
    return q, k, v


def last_key_decides(N, heads, Sq, Skv, d, dtype=torch.float16, seed=0):
    """Calm logits, except that key Skv - 1 carries a logit about 12 (natural units) above the rest for EVERY query, and its V row is
    offset by -3 against +1.5 for the others (as in spike_and_sea): a kernel that drops the last valid key - the one a ragged tile's
    mask sits next to - returns the others' mean, three units away.  Asserted in fp64: that key's softmax weight is >= 0.99 in
    every row."""
    g = _gen(seed)
    q = 0.5 * torch.randn(N, Sq, heads, d, generator=g, dtype=torch.float64)
    k = 0.5 * torch.randn(N, Skv, heads, d, generator=g, dtype=torch.float64)
    v = torch.randn(N, Skv, heads, d, generator=g, dtype=torch.float64) + 1.5
    u = _unit((d,), g)
    q = q - (q * u).sum(dim=-1, keepdim=True) * u
    k = k - (k * u).sum(dim=-1, keepdim=True) * u
    amp = math.sqrt(12.0 * math.sqrt(d))
    q = q + u * amp
    k[:, Skv - 1] = k[:, Skv - 1] + u * amp
    v[:, Skv - 1] = v[:, Skv - 1] - 3.0
    q, k, v = (rnd(t.reshape(N, -1, heads * d), dtype) for t in (q, k, v))
    w = torch.softmax(_softmax64(q, k, heads), dim=-1)
    assert float(w[..., Skv - 1].min()) >= 0.99, float(w[..., Skv - 1].min())
    return q, k, v


# ----------------------------------------------------------------------------------------------------------------
# LayerNorm -> Linear (-> GEGLU)
# ----------------------------------------------------------------------------------------------------------------
def ln_case(x, Cout, dtype, geglu=False, bias=True, seed=0, eps=1e-5):
    """weights of a LayerNorm + Linear pair for the rows x [M, C]: W rounded to the storage dtype (the weights the fold is SPECIFIED
    to equal are the unfolded rounded W), gamma / beta / bias fp32"""
    g = _gen(seed + 7919)
    C = x.shape[1]
    return dict(x=x, dtype=dtype, geglu=geglu, eps=eps,
                gamma=1 + 0.2 * torch.randn(C, generator=g), beta=0.1 * torch.randn(C, generator=g),
                W=rnd(torch.randn(Cout, C, generator=g) / math.sqrt(C), dtype),
                b=(torch.randn(Cout, generator=g) * 0.1) if bias else None)


def ln_ref64(c):
    """c["ln"] False (the plain forms of es_linear_xs; absent: True): no LayerNorm in front.  c["res"]: a residual added to the result."""
    x = c["x"].double()
    y = F.layer_norm(x, (x.shape[1],), c["gamma"].double(), c["beta"].double(), c["eps"]) if c.get("ln", True) else x
    y = F.linear(y, c["W"].double(), None if c["b"] is None else c["b"].double())
    if c["geglu"]:
        h, gate = y.chunk(2, dim=-1)
        y = h * F.gelu(gate)
    if c.get("res") is not None:
        y = y + c["res"].double()
    return y


def ln_intermediates_peak(c) -> float:
    """largest magnitude (fp64) among what the REFERENCE would store in the storage dtype: the LayerNorm output, the Linear output,
    the GEGLU product"""
    x = c["x"].double()
    n = F.layer_norm(x, (x.shape[1],), c["gamma"].double(), c["beta"].double(), c["eps"])
    y = F.linear(n, c["W"].double(), None if c["b"] is None else c["b"].double())
    m = max(float(n.abs().max()), float(y.abs().max()))
    if c["geglu"]:
        h, gate = y.chunk(2, dim=-1)
        m = max(m, float((h * F.gelu(gate)).abs().max()))
    return m


def ln_base_ref(c):
    """two-pass LayerNorm -> round -> Linear with fp32 accumulation -> round (-> GELU -> round -> product -> round)"""
    dt = c["dtype"]
    x = c["x"].float()
    n = rnd(F.layer_norm(x, (x.shape[1],), c["gamma"], c["beta"], c["eps"]), dt) if c.get("ln", True) else x
    y = rnd(F.linear(n, c["W"], c["b"]), dt)
    if c["geglu"]:
        h, gate = y.chunk(2, dim=-1)
        y = rnd(h * rnd(F.gelu(gate), dt), dt)
    if c.get("res") is not None:
        y = rnd(y + c["res"].float(), dt)
    return y


def _chain_sums(x, order):
    """fp32 sums of x and x^2 along the last dimension in the order the LayerNorm-folding kernels form them (every step rounded to
    fp32; the products and the 8-wide partial dot products are taken exactly, in fp64):
      "mfma8"   es_conv_gemm: both sums ride on the matrix core - one chain of 16x16x32 MFMAs per row.  A lane supplies 8 consecutive
                channels of an operand, and the accumulator takes one such 8-channel partial dot product after the other (four per
                instruction): with this order the emulation reproduces the kernels' error at |mean| / std = 300 to four digits on
                the MI355X (C = 320, 640, 1280), with one rounding per 32 channels it is 2-4 times too small there;
      "xs"      es_linear_xs: a row's channels sit in four lanes, lane f holding channels 32 i + 8 f .. + 7 of every 32-channel
                chunk i; each lane runs s += v, ss = fma(v, v, ss) over its values in order, then (l0 + l1) + (l2 + l3)."""
    M, K = x.shape
    xd = x.double()
    if order == "mfma8":
        s = torch.zeros(M, dtype=torch.float32)
        ss = torch.zeros(M, dtype=torch.float32)
        for i in range(0, K, 8):
            blk = xd[:, i:i + 8]
            s = (s.double() + blk.sum(dim=1)).float()
            ss = (ss.double() + (blk * blk).sum(dim=1)).float()
        return s[:, None], ss[:, None]
    assert order == "xs" and K % 32 == 0
    lanes = xd.reshape(M, K // 32, 4, 8).permute(0, 2, 1, 3).reshape(M, 4, K // 4)
    s = torch.zeros(M, 4, dtype=torch.float32)
    ss = torch.zeros(M, 4, dtype=torch.float32)
    for j in range(K // 4):
        v = lanes[:, :, j]
        s = (s.double() + v).float()
        ss = (ss.double() + v * v).float()
    fold = lambda t: ((t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3]))[:, None]
    return fold(s), fold(ss)


def one_pass_stats(x, dim, eps, partial_dtype=None, chunks=1, order="tree"):
    """mean and rstd as the kernels form them: fp32 sums of x and x^2, var = E[x^2] - mean^2 clamped at 0.
    order: "tree" (torch's blocked fp32 sums) or one of _chain_sums' orders (2-d x, dim 1) - at |mean| / std of 100 and more the
    variance is what the rounding of these sums leaves, and a tree sum is several times more accurate than a chain of the same length.
    partial_dtype (a planted defect): the sums are formed in `chunks` partial sums that are rounded to that dtype before they are
    added up."""
    x = x.float()
    cnt = x.shape[dim] if isinstance(dim, int) else math.prod(x.shape[d] for d in dim)
    if partial_dtype is not None:
        assert isinstance(dim, int)
        parts = x.chunk(chunks, dim=dim)
        s = sum(rnd(p.sum(dim=dim, keepdim=True), partial_dtype) for p in parts)
        ss = sum(rnd((p * p).sum(dim=dim, keepdim=True), partial_dtype) for p in parts)
    elif order != "tree":
        assert dim == 1 and x.dim() == 2
        s, ss = _chain_sums(x, order)
    else:
        s, ss = x.sum(dim=dim, keepdim=True), (x * x).sum(dim=dim, keepdim=True)
    mean = s * (1.0 / cnt) if order != "tree" else s / cnt
    var = (ss * (1.0 / cnt) if order != "tree" else ss / cnt) - mean * mean
    return mean, torch.rsqrt(var.clamp_min(0.0) + eps)


def fold_weights(c):
    """ops.pack_weight_ln's definitions: W' = round(W * gamma), colsum of the ROUNDED W' (fp64 sum, rounded once to fp32), folded
    bias W beta + b (fp64, rounded once)"""
    Wf = rnd(c["W"] * c["gamma"][None, :], c["dtype"])
    colsum = Wf.double().sum(dim=1).float()
    fb = c["W"].double() @ c["beta"].double()
    if c["b"] is not None:
        fb = fb + c["b"].double()
    return Wf, colsum, fb.float()


def ln_base_alg(c, form="fold", defect=None, chain=None):
    """form "fold" (es_conv_gemm, ln_colsum): rstd * (x W'^T - mean * colsum(W')) + (W beta + b), one-pass statistics, rounded once.
    form "xs" (es_linear_xs): the row is normalised in registers, x * rstd + (-mean * rstd) rounded to the storage dtype, then
    multiplied with W'.  With chain = 8 | 32 (form "xs" only) every output is ONE fp32 chain over K that STARTS from the bias (the
    bias is the C operand of the first MFMA: no separate add), `chain`-wide partial dot products as _chain_dot takes them; c["ln"]
    False: no LayerNorm (the plain forms: x, W and b as they are); c["res"]: round, + residual in fp32, round again.
    defect: "colsum_unrounded" (colsum taken from W * gamma before rounding), "partial_sums_fp16" (the statistics' partial sums of 64
    channels rounded to fp16); form "xs" with a chain: "geglu_halves_swapped" (gate * gelu(hidden)), "residual_row_shift" (the residual
    read one 16-row fragment further down; rows past M read as zeros, as a range-checked buffer load returns them)."""
    dt = c["dtype"]
    x = c["x"].float()
    ln = c.get("ln", True)
    assert form == "xs" or (ln and chain is None and c.get("res") is None)
    if ln:
        Wf, colsum, fb = fold_weights(c)
    else:
        Wf, fb = c["W"], (c["b"] if c["b"] is not None else torch.zeros(c["W"].shape[0]))
    if defect == "colsum_unrounded":
        colsum = (c["W"].double() * c["gamma"].double()[None, :]).sum(dim=1).float()
    if not ln:
        mean = rstd = None
    elif defect == "partial_sums_fp16":
        mean, rstd = one_pass_stats(x, 1, c["eps"], partial_dtype=torch.float16, chunks=x.shape[1] // 64)
    else:
        mean, rstd = one_pass_stats(x, 1, c["eps"], order="mfma8" if form == "fold" else "xs")
    if form == "fold":
        y = rstd * (x @ Wf.t() - mean * colsum[None, :]) + fb[None, :]
    else:
        xn = rnd(torch.addcmul(-mean * rstd, x, rstd), dt) if ln else x
        y = xn @ Wf.t() + fb[None, :] if chain is None else _chain_dot(xn, Wf, chain, init=fb)
    if c["geglu"]:
        h, gate = y.chunk(2, dim=-1)
        y = gate * F.gelu(h) if defect == "geglu_halves_swapped" else h * F.gelu(gate)
    y = rnd(y, dt)
    if c.get("res") is not None:
        res = c["res"].float()
        if defect == "residual_row_shift":
            res = torch.cat([res[16:], torch.zeros(min(16, res.shape[0]), res.shape[1])], 0)
        y = rnd(y + res, dt)
    return y


# ----------------------------------------------------------------------------------------------------------------
# GroupNorm (-> SiLU) and GroupNorm -> 1x1 projection
# ----------------------------------------------------------------------------------------------------------------
def gn_case(x, groups, dtype, silu=False, eps=1e-5, seed=0, Cout=0, ngroups=1):
    """x [N, H, W, C] NHWC.  Cout > 0: a 1x1 projection behind the GroupNorm (Transformer2DModel.norm -> proj_in).  ngroups > 1: that
    many parameter sets (grouped launches)."""
    g = _gen(seed + 104729)
    C = x.shape[-1]
    c = dict(x=x, groups=groups, dtype=dtype, silu=silu, eps=eps,
             gamma=[1 + 0.2 * torch.randn(C, generator=g) for _ in range(ngroups)],
             beta=[0.2 * torch.randn(C, generator=g) for _ in range(ngroups)])
    if Cout:
        c["W"] = [rnd(torch.randn(Cout, C, generator=g) / math.sqrt(C), dtype) for _ in range(ngroups)]
        c["b"] = [torch.randn(Cout, generator=g) * 0.1 for _ in range(ngroups)]
    return c


def _gn_groups_view(x, groups):
    N, H, W, C = x.shape
    return x.reshape(N, H * W, groups, C // groups)


def _per_set(c, counts, fn):
    """apply fn(x_slice, i) to the sample ranges of a grouped launch"""
    counts = counts or [c["x"].shape[0]]
    out, a = [], 0
    for i, n in enumerate(counts):
        out.append(fn(c["x"][a:a + n], i))
        a += n
    return torch.cat(out, 0)


def gn_ref64(c, counts=None):
    def one(x, i):
        xg = _gn_groups_view(x.double(), c["groups"])
        mean = xg.mean(dim=(1, 3), keepdim=True)
        var = xg.var(dim=(1, 3), unbiased=False, keepdim=True)
        y = ((xg - mean) / torch.sqrt(var + c["eps"])).reshape(x.shape) * c["gamma"][i].double() + c["beta"][i].double()
        if c["silu"]:
            y = F.silu(y)
        if "W" in c:
            y = y @ c["W"][i].double().t() + c["b"][i].double()
        return y
    return _per_set(c, counts, one)


def gn_intermediates_peak(c, counts=None) -> float:
    keep = {k: c[k] for k in c if k not in ("W", "b")}
    m = float(gn_ref64(dict(keep, silu=False), counts).abs().max())
    return max(m, float(gn_ref64(c, counts).abs().max()))


def gn_base_ref(c, counts=None):
    """two-pass GroupNorm in fp32 -> round (-> SiLU -> round) (-> projection with fp32 accumulation -> round)"""
    dt = c["dtype"]

    def one(x, i):
        xg = _gn_groups_view(x.float(), c["groups"])
        mean = xg.mean(dim=(1, 3), keepdim=True)
        var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
        y = rnd(((xg - mean) * torch.rsqrt(var + c["eps"])).reshape(x.shape) * c["gamma"][i] + c["beta"][i], dt)
        if c["silu"]:
            y = rnd(F.silu(y), dt)
        if "W" in c:
            y = rnd(y @ c["W"][i].t() + c["b"][i], dt)
        return y
    return _per_set(c, counts, one)


def xs_group_of_channel(c: int, cpg: int) -> int:
    """the integer channel -> group map of csrc/linear_xs.hip (GroupNorm in front): a 2^20 reciprocal"""
    inv = ((1 << 20) + cpg - 1) // cpg
    return ((c * inv) & 0xFFFFFFFF) >> 20


def xs_group_of_channel_2_16(c: int, cpg: int) -> int:
    """the map that code used before: a 2^16 reciprocal - inexact for cpg = 640 (a planted defect here)"""
    inv = (65536 + cpg - 1) // cpg
    return (c * inv) >> 16


GN_MAX_CHUNK = 64               # csrc/norm.hip: pixel chunks per sample of the statistics pass


def gn_pixels_per_chunk(HW: int) -> int:
    """gn_pixels_per_block of csrc/norm.hip: max(16, ceil(HW / 64)) - rounded UP, so that no HW gives more than 64 chunks"""
    return max(16, (HW + GN_MAX_CHUNK - 1) // GN_MAX_CHUNK)


def gn_chunked_stats(xg, eps):
    """GroupNorm statistics of xg [N, HW, groups, cpg] summed the way the kernels sum them - in three short levels, never as one long
    sum: a channel's pixels inside a chunk of max(16, ceil(HW / 64)) pixels, the channels of a group, the chunks of a sample
    (gn_stats_kernel + the prologue of gn_apply_kernel; the slab kernel and the producer's epilogue have the same three levels with
    other chunk sizes).  Every level's result is rounded to fp32 once (taken in fp64 inside the level - a little better than the
    kernels' chains of at most a few dozen fp32 additions there).  A flat fp32 sum over a group of 40960 values and more is up to ten
    times noisier than this at |mean| / std = 30, and than the kernels."""
    N, HW, G, cpg = xg.shape
    ppb = gn_pixels_per_chunk(HW)
    nchunk = (HW + ppb - 1) // ppb
    assert nchunk <= GN_MAX_CHUNK
    pad = nchunk * ppb - HW
    xd = xg.double()
    if pad:
        xd = torch.cat([xd, torch.zeros(N, pad, G, cpg, dtype=torch.float64)], 1)
    xd = xd.reshape(N, nchunk, ppb, G, cpg)

    def levels(t):
        t = t.sum(dim=2).float()                    # pixels of a chunk, per channel
        t = t.double().sum(dim=3).float()           # channels of a group
        return t.double().sum(dim=1).float()        # chunks of a sample -> [N, G]
    cnt = float(cpg) * float(HW)
    mean = levels(xd) / cnt
    var = (levels(xd * xd) / cnt - mean * mean).clamp_min(0.0)
    return mean.reshape(N, 1, G, 1), torch.rsqrt(var + eps).reshape(N, 1, G, 1)


def gn_base_alg(c, counts=None, defect=None, stats_from=None, geom=None, chain=None):
    """chain = 8 | 32: the projection as es_linear_xs forms it - one fp32 chain per output that starts from the bias (_chain_dot).
    geom (a route of gn_route / lib.group_norm_route): the norm sweep's form of this function, gn_base_alg_geom - the statistics in the
    chunk geometry of the form that RUNS (the slab's pixel slots too), two sources, and the planted defects GN_DEFECTS.  Without geom:
    one-pass statistics (fp32 sums in the kernels' chunking: gn_chunked_stats; E[x^2] - mean^2 clamped at 0); x * (rstd gamma) + (beta - mean rstd gamma) (-> SiLU) rounded
    once; then the projection.  stats_from: another tensor of x's shape from which the STATISTICS are taken (the producer hand-over:
    sums of the fp32 accumulators, while the rounded values are normalised).
    defect "wrong_group_tail": the last three channels are normalised with the statistics of another group - what the 2^16
    reciprocal did to channels 637..639 of K = 640 with one group: they took (rstd, -mean rstd) of a "group 1" that nobody had
    written.  With several groups the stand-in is the first group's pair; with one group it is (0, 0), memory read as zeros."""
    if geom is not None:
        assert stats_from is None
        return gn_base_alg_geom(c, geom, counts, defect)
    dt = c["dtype"]
    G = c["groups"]

    def one(x, i, xs=None):
        xg = _gn_groups_view(x.float(), G)
        sg = xg if xs is None else _gn_groups_view(xs.float(), G)
        mean, rstd = gn_chunked_stats(sg, c["eps"])
        N, HW, _, cpg = xg.shape
        mean_c = mean.expand(N, 1, G, cpg).reshape(N, 1, G * cpg).clone()
        rstd_c = rstd.expand(N, 1, G, cpg).reshape(N, 1, G * cpg).clone()
        if defect == "wrong_group_tail":
            if G > 1:
                mean_c[:, :, -3:] = mean.reshape(N, 1, G)[:, :, :1]
                rstd_c[:, :, -3:] = rstd.reshape(N, 1, G)[:, :, :1]
            else:
                mean_c[:, :, -3:] = 0.0
                rstd_c[:, :, -3:] = 0.0
        a = rstd_c * c["gamma"][i]
        b = c["beta"][i] - mean_c * a
        y = x.float().reshape(N, HW, -1) * a + b
        if c["silu"]:
            y = F.silu(y)
        y = rnd(y, dt).reshape(x.shape)
        if "W" in c and chain is not None:
            y = rnd(_chain_dot(y.reshape(N * HW, -1), c["W"][i], chain, init=c["b"][i]), dt).reshape(*x.shape[:-1], -1)
        elif "W" in c:
            y = rnd(y @ c["W"][i].t() + c["b"][i], dt)
        return y
    if stats_from is None:
        return _per_set(c, counts, one)
    assert counts is None
    return one(c["x"], 0, stats_from)


# ----------------------------------------------------------------------------------------------------------------
# csrc/norm.hip on every route (tests/test_norm_gpu.py): GroupNorm in the geometry that runs, plain LayerNorm
# ----------------------------------------------------------------------------------------------------------------
GN_UNROLL = 4                   # csrc/norm.hip: loads in flight per thread in the streaming loops
GN_LDS_LIMIT = 64 * 1024
GN_FORM_SLAB, GN_FORM_TWO = 1, 2
GN_DEFECTS = ("pad_pixel_counted", "tail_pixels_dropped", "second_source_stride", "group_by_chunk", "neighbour_sample", "variance_unclamped")
LN_DEFECTS = ("one_pass_variance", "group_boundary_by_block")
NORM_KINDS = ("ratio_0", "ratio_30", "dominant", "constant", "zero")
NORM_CONSTANT = 2.71875         # 87 / 32: exact in bf16 and fp16
NORM_NAN_BITS_F32 = 0x7FC5A5A5  # the fp32 operands' guard: a quiet NaN with a payload no arithmetic produces (as ATTN_NAN_BITS for the 16-bit types)


def gn_route(N, HW, C, groups, stats_only=False):
    """Python mirror of gn_route() in csrc/norm.hip (chunk rule rounded up), keyed like lib.GN_ROUTE_FIELDS.  The GPU rows assert the
    LIBRARY's answer (es_group_norm_route); this mirror places the table's rows without a GPU and is held to the library on the CPU."""
    r = dict.fromkeys(("form", "gpb", "slots", "cpt", "ppb", "nchunk", "ps", "lanes", "blocks", "ipt", "general", "lds"), 0)
    cpg, CH8 = C // groups, C // 8
    if not stats_only:
        for gpb in (1, 2, 4):
            if groups % gpb or (gpb * cpg) % 8:
                continue
            W8 = gpb * cpg // 8
            if W8 > 256:
                break
            PS = 256 // W8
            cpt = (HW + PS - 1) // PS
            if cpt <= 24:
                r.update(form=GN_FORM_SLAB, gpb=gpb, slots=PS, cpt=8 if cpt <= 8 else 16 if cpt <= 16 else 24, lds=(2 * PS * gpb * cpg + 2 * gpb) * 4)
                return r
            break
    ppb = gn_pixels_per_chunk(HW)
    ps = 256 // CH8 if CH8 <= 256 else 1
    r.update(form=GN_FORM_TWO, ppb=ppb, nchunk=(HW + ppb - 1) // ppb, ps=ps, lanes=8 if groups <= 32 else 4, lds=2 * ps * C * 4)
    if stats_only:
        return r
    total = HW * CH8
    ipt = GN_UNROLL
    for cand in (16, 8):
        if ((total + 256 * cand - 1) // (256 * cand)) * N >= 1024:
            ipt = cand
            break
    blocks = min(max((total + 256 * ipt - 1) // (256 * ipt), 1), 1024)
    q = CH8 // math.gcd(CH8, 256)
    if q <= 64:
        blocks = q if blocks < q else blocks // q * q
    r.update(blocks=blocks, ipt=ipt, general=int((blocks * 256) % CH8 != 0), lds=(2 * C + 2 * groups + 256) * 4)
    return r


def gn_sum_chain(route, cpg) -> int:
    """h of the standard bound |S - S64| <= h 2^-24 sum|x| for one row of `partials`: the longest chain of fp32 additions on the
    two-launch route - a thread's pixels of one slot, a lane's share of the group's ps * cpg LDS entries, the fold steps"""
    assert route["form"] == GN_FORM_TWO
    L = route["lanes"]
    return -(-route["ppb"] // route["ps"]) + -(-(route["ps"] * cpg) // L) + int(math.log2(L))


NORM_TIE_CLEARANCE = 2.0 ** -19        # 32 fp32 ulps: an fp32 SiLU from a hardware exp and reciprocal (about 1 ulp each, two more roundings) is well inside


def tie_distance(v64: torch.Tensor, dtype) -> torch.Tensor:
    """relative distance of |v64| to the nearest rounding boundary of the storage dtype (the midpoint between the value it rounds to and that
    value's neighbours): below the error of the arithmetic that produced v, WHICH neighbour is stored is a draw, not a property of the kernel"""
    a = v64.double().abs()
    bits = a.float().to(dtype).view(torch.int16)
    assert bool((bits > 0).all()), "tie_distance is for nonzero finite values"
    r, up, dn = (b.view(dtype).double() for b in (bits, bits + 1, bits - 1))
    return torch.minimum((a - (r + up) / 2).abs(), (a - (r + dn) / 2).abs()) / a


def norm_case(HW, C1, C2, groups, N, kind, dtype, silu=False, counts=None, seed=0, eps=1e-5):
    """A GroupNorm case of the norm sweep: x [N, HW, 1, C1 + C2] from group_maps (which asserts its own postconditions), split into two
    sources at C1.  kind: ratio_0 | ratio_30 (|mean| / std per (sample, group)), dominant (one channel holds >= 90 % of a group's
    variance, ratio 30), constant (sample 0 is NORM_CONSTANT everywhere), zero (sample 0 is 0 everywhere; with SiLU no SiLU(beta) lies
    within NORM_TIE_CLEARANCE of a rounding boundary of the storage dtype); the other samples of a constant / zero case are ratio_0 maps.  A geometry whose groups hold ONE value (HW * cpg == 1) has no spread to shape: only
    constant and zero exist there.  Postconditions of the overwritten sample are asserted here."""
    assert kind in NORM_KINDS
    C = C1 + C2
    cpg = C // groups
    if HW * cpg == 1:
        assert kind in ("constant", "zero"), "a group of one value is constant"
        x = rnd(torch.randn(N, HW, 1, C, generator=_gen(seed), dtype=torch.float64), dtype)
    else:
        ratio = 30 if kind in ("ratio_30", "dominant") else 0
        x = group_maps(N, C, HW, groups, ratio, 0.0, peak=4.0, dtype=dtype, seed=seed, dominant_channel=kind == "dominant", W=1)
    if kind in ("constant", "zero"):
        x[0] = NORM_CONSTANT if kind == "constant" else 0.0
        assert float(rnd(x[0], dtype).min()) == float(x[0].max()) == (NORM_CONSTANT if kind == "constant" else 0.0)
    c = gn_case(x, groups, dtype, silu=silu, eps=eps, seed=seed, ngroups=len(counts) if counts else 1)
    c.update(C1=C1, C2=C2, kind=kind, counts=list(counts) if counts else None)
    if kind == "zero" and silu:
        # a zero sample's output is act(beta), asserted bit for bit: no SiLU(beta) may sit on a rounding boundary of the storage dtype
        # (to within what an fp32 SiLU can resolve).  About C / 250 of the drawn betas do in fp16; they are moved by steps of 2^-12.
        for beta in c["beta"]:
            for _ in range(8):
                close = tie_distance(F.silu(beta.double()), dtype) < NORM_TIE_CLEARANCE
                if not bool(close.any()):
                    break
                beta[close] += 2.0 ** -12
            assert float(tie_distance(F.silu(beta.double()), dtype).min()) >= NORM_TIE_CLEARANCE
    return c


def _gn_read_sources(c, x, defect):
    """x [n, HW, 1, C] as the kernel reads it from its two dense sources; second_source_stride: x2 [n HW, C2] read with C1's row pitch
    (element (row, cc) <- flat[row * C1 + cc]; addresses behind the buffer wrap, standing in for whatever lies there)"""
    C1, C2 = c.get("C1", x.shape[-1]), c.get("C2", 0)
    if defect != "second_source_stride" or not C2:
        return x
    n, HW = x.shape[0], x.shape[1]
    flat = x[..., C1:].reshape(-1)
    idx = (torch.arange(n * HW)[:, None] * C1 + torch.arange(C2)[None, :]) % flat.numel()
    return torch.cat([x[..., :C1], flat[idx].reshape(n, HW, 1, C2)], dim=-1)


def gn_geom_sums(xg, route, defect=None):
    """fp32 (S, SS) per (sample, chunk, group) of xg [n, HW, G, cpg] in the chunk geometry of `route`, and the pixel count the geometry
    covers.  Two launches: chunk k holds pixels [k ppb, (k + 1) ppb), inside it pixel j sits in slot j % ps; level 1 a (slot, channel)'s
    pixels, level 2 the ps * cpg entries of a group.  Slab: ONE chunk of slots * ceil(HW / slots) pixels; level 1 as above, level 2a the
    slots of a channel, 2b the channels of a group.  Every level is summed in fp64 and rounded to fp32 once (see gn_chunked_stats).
    defects: tail_pixels_dropped (a slot's pixels behind its last full round of GN_UNROLL), neighbour_sample (pad pixels read the
    next sample's first pixels, cyclically, instead of zeros)."""
    n, HW, G, cpg = xg.shape
    slab = route["form"] == GN_FORM_SLAB
    ps = route["slots"] if slab else route["ps"]
    ppb = ps * (-(-HW // ps)) if slab else route["ppb"]
    nchunk = 1 if slab else route["nchunk"]
    assert nchunk * ppb >= HW
    rounds = -(-ppb // ps)
    xd = xg.double()
    pad = nchunk * ppb - HW
    if pad:
        if defect == "neighbour_sample":
            nxt = torch.roll(xd, -1, 0)
            fill = torch.cat([nxt] * (-(-pad // HW)), 1)[:, :pad]
        else:
            fill = torch.zeros(n, pad, G, cpg, dtype=torch.float64)
        xd = torch.cat([xd, fill], 1)
    xd = xd.reshape(n, nchunk, ppb, G, cpg)
    if rounds * ps != ppb:
        xd = torch.cat([xd, torch.zeros(n, nchunk, rounds * ps - ppb, G, cpg, dtype=torch.float64)], 2)
    xd = xd.reshape(n, nchunk, rounds, ps, G, cpg)
    if defect == "tail_pixels_dropped":
        j = torch.arange(rounds)[:, None] * ps + torch.arange(ps)[None, :]                              # pixel inside the chunk
        px = torch.arange(nchunk)[:, None, None] * ppb + j[None]
        valid = (j[None] < ppb) & (px < HW)
        keep = valid.sum(dim=1, keepdim=True) // GN_UNROLL * GN_UNROLL                                  # [nchunk, 1, ps]
        mask = (torch.arange(rounds)[None, :, None] < keep).double()
        xd = xd * mask[None, :, :, :, None, None]

    def levels(t):
        t = t.sum(dim=2).float()                                    # [n, nchunk, ps, G, cpg]
        if slab:
            t = t.double().sum(dim=2).float()                       # slots of a channel
            return t.double().sum(dim=3).float()                    # channels of a group -> [n, 1, G]
        return t.double().sum(dim=(2, 4)).float()                   # [n, nchunk, G]
    return levels(xd), levels(xd * xd), nchunk * ppb


def gn_base_alg_geom(c, route, counts=None, defect=None):
    """The algorithm of csrc/norm.hip on the route that runs: gn_geom_sums, the chunks of a sample added up (rounded once), mean = S / cnt,
    var = SS / cnt - mean^2 clamped at 0, y = x (rstd gamma) + (beta - mean rstd gamma) (-> SiLU), rounded once.  Defects: GN_DEFECTS."""
    assert defect is None or defect in GN_DEFECTS, defect
    dt, G = c["dtype"], c["groups"]

    def one(x, i):
        n, C = x.shape[0], x.shape[-1]
        HW, cpg = x[0].numel() // C, C // G
        xr = _gn_read_sources(c, x.float().reshape(n, HW, 1, C), defect)
        xg = xr.reshape(n, HW, G, cpg)
        S, SS, covered = gn_geom_sums(xg, route, defect)
        S, SS = S.double().sum(dim=1).float(), SS.double().sum(dim=1).float()          # [n, G]
        cnt = float(cpg) * float(covered if defect == "pad_pixel_counted" else HW)
        mean = S / cnt
        var = SS / cnt - mean * mean
        if defect != "variance_unclamped":
            var = var.clamp_min(0.0)
        rstd = torch.rsqrt(var + c["eps"])
        grp = torch.arange(C) // cpg
        if defect == "group_by_chunk":
            grp = (torch.arange(C) // 8 * 8) // cpg
        a = rstd[:, grp] * c["gamma"][i]                                                # [n, C]
        b = c["beta"][i] - mean[:, grp] * a
        y = xr.reshape(n, HW, C) * a[:, None, :] + b[:, None, :]
        if c["silu"]:
            y = F.silu(y)
        return rnd(y, dt).reshape(x.shape)
    return _per_set(c, counts, one)


def ln_plain_case(x, dtype, ngroups=1, seed=0, eps=1e-5):
    """rows x [M, C] and `ngroups` parameter sets of a plain LayerNorm (es_layer_norm / es_layer_norm_grouped)"""
    g = _gen(seed + 15485863)
    C = x.shape[1]
    return dict(x=x, dtype=dtype, eps=eps, gamma=[1 + 0.2 * torch.randn(C, generator=g) for _ in range(ngroups)],
                beta=[0.2 * torch.randn(C, generator=g) for _ in range(ngroups)])


def _ln_sets(c, rows, by_block=False):
    """parameter set of every row; by_block (a planted defect): a 4-row block takes its first row's set"""
    M = c["x"].shape[0]
    rows = rows or [M]
    assert sum(rows) == M and len(rows) == len(c["gamma"])
    r = torch.arange(M)
    if by_block:
        r = r // 4 * 4
    ends = torch.tensor(rows).cumsum(0)
    return (r[:, None] >= ends[None, :]).sum(dim=1)


def ln_plain_ref64(c, rows=None):
    x = c["x"].double()
    st = _ln_sets(c, rows)
    gam, bet = torch.stack(c["gamma"]).double()[st], torch.stack(c["beta"]).double()[st]
    return (x - x.mean(dim=1, keepdim=True)) / torch.sqrt(x.var(dim=1, unbiased=False, keepdim=True) + c["eps"]) * gam + bet


def ln_plain_base_ref(c, rows=None):
    """the textbook sequence in fp32 with every op's output rounded to the storage dtype: normalise -> round -> scale -> round -> shift -> round"""
    dt = c["dtype"]
    x = c["x"].float()
    st = _ln_sets(c, rows)
    gam, bet = torch.stack(c["gamma"])[st], torch.stack(c["beta"])[st]
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    n = rnd((x - mean) * torch.rsqrt(var + c["eps"]), dt)
    return rnd(rnd(n * gam, dt) + bet, dt)


def ln_plain_base_alg(c, rows=None, defect=None):
    """layer_norm_kernel as designed: one wave per row, lane l holds the 16-byte chunks l, l + 64, ...; EXACT two-pass statistics in fp32 -
    a lane's values added in order, the 64 lanes folded by wave_sum's tree, mean = s / C, then the squared deviations the same way;
    (x - mean) rstd gamma + beta rounded once.  Lanes behind the row's end add nothing to either sum.
    defects: one_pass_variance (E[x^2] - mean^2 clamped at 0), group_boundary_by_block (_ln_sets by_block)."""
    assert defect is None or defect in LN_DEFECTS, defect
    x = c["x"].float()
    M, C = x.shape
    CH8 = C // 8
    vpl = -(-CH8 // 64)
    st = _ln_sets(c, rows, by_block=defect == "group_boundary_by_block")
    gam, bet = torch.stack(c["gamma"])[st], torch.stack(c["beta"])[st]
    xp = torch.cat([x, torch.zeros(M, vpl * 512 - C)], 1).reshape(M, vpl, 64, 8)
    live = (torch.arange(vpl * 64).reshape(vpl, 64) < CH8).float()[None, :, :, None]

    def lanes_then_tree(t):                      # t [M, vpl, 64, 8] -> [M, 1]
        acc = torch.zeros(M, 64)
        for i in range(vpl):
            for e in range(8):
                acc = acc + t[:, i, :, e]
        return _wave_tree(acc)[:, None]
    mean = lanes_then_tree(xp) / float(C)
    if defect == "one_pass_variance":
        var = (lanes_then_tree(xp * xp) / float(C) - mean * mean).clamp_min(0.0)
    else:
        d = (xp - mean[:, :, None, None]) * live
        var = lanes_then_tree(d * d) / float(C)
    rstd = torch.rsqrt(var + c["eps"])
    return rnd((x - mean) * rstd * gam + bet, c["dtype"])


def norm_guarded(t, guard, dtype, device="cpu"):
    """(whole buffer, recipe of the middle slice) for an operand t: `guard` elements of NaN on each side (fp16 / bf16: the payload NaNs
    of ATTN_NAN_BITS; fp32: NORM_NAN_BITS_F32), the operand's values in the middle.  guard must keep the slice 16-byte aligned."""
    assert (guard * torch.empty(0, dtype=dtype).element_size()) % 16 == 0
    n = t.numel()
    if dtype == torch.float32:
        big = torch.full((n + 2 * guard,), NORM_NAN_BITS_F32, dtype=torch.int32).view(torch.float32)
    else:
        big = torch.full((n + 2 * guard,), ATTN_NAN_BITS[dtype], dtype=torch.int16).view(dtype)
    big[guard:guard + n] = t.reshape(-1).to(dtype)
    return big.to(device), (guard, n)


# ----------------------------------------------------------------------------------------------------------------
# implicit-GEMM convolution (es_conv_gemm): the misrounded share
# ----------------------------------------------------------------------------------------------------------------
# With fp32 accumulation and ONE rounding a convolution's output equals the correctly rounded fp64 result except where the fp64 value
# sits within the accumulation noise of a rounding boundary: 0.1-0.2 % of the elements in fp16, next to none in bf16.  An extra
# rounding anywhere (split-K slabs stored in the storage dtype, a bias added behind the rounding) moves that share to 25-40 %, while
# max|y - ref| / max|ref| and row_err move by a factor of under two - the rounding of the output dominates both.  So the convolution
# is judged by `misrounded`, against a bar that is recomputed from independent fp32 implementations of the same launch.
MISROUNDED_FLOOR = 100          # elements: the bar where the largest baseline count is under 50 (bf16, small cases)
CONV_MIN_ELEMENTS = 20000       # a case of this size keeps that floor below 0.5 % - fifty times under what one extra rounding makes
BM_CONV = 128                   # pixels per workgroup tile of csrc/gemm_conv.hip (the planted tile defects cut here)


def round64(ref64: torch.Tensor, dtype) -> torch.Tensor:
    """ref64 correctly rounded to the storage dtype (returned in fp32).  fp64 -> fp32 -> dtype rounds twice: where the fp32 value sits
    on a tie of the storage dtype the second rounding cannot know on which side the fp64 value was.  Both neighbours of such a value
    are formed (the fp32 value as it is, and nudged one fp32 step towards the fp64 value) and the one closer in fp64 is taken."""
    r = ref64.detach().to("cpu", torch.float64)
    r32 = r.float()
    d = r - r32.double()
    toward = torch.where(d > 0, torch.full_like(r32, float("inf")), torch.full_like(r32, float("-inf")))
    nudged = torch.where(d == 0, r32, torch.nextafter(r32, toward))
    h1, h2 = r32.to(dtype).float(), nudged.to(dtype).float()
    take2 = (h2.double() - r).abs() < (h1.double() - r).abs()
    return torch.where(take2, h2, h1)


def misrounded(y: torch.Tensor, ref64: torch.Tensor, dtype, count: bool = False):
    """share (count=True: number) of elements with y != ref64 correctly rounded to the storage dtype; a NaN counts as different"""
    want = round64(ref64, dtype)
    v = y.detach().to("cpu", torch.float32)
    assert v.shape == want.shape, (v.shape, want.shape)
    n = int((v != want).sum())
    return n if count else n / max(1, want.numel())


def differs(y: torch.Tensor, z: torch.Tensor, count: bool = False):
    """share of elements in which two results in the storage dtype differ (forms with a residual round twice BY DESIGN: they are
    judged by the share that differs from base_alg, not from the correctly rounded truth)"""
    a, b = y.detach().to("cpu", torch.float32), z.detach().to("cpu", torch.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    n = int((a != b).sum())
    return n if count else n / max(1, a.numel())


def misrounded_bar(counts) -> int:
    """largest number of differing elements a launch may show: MARGIN x the largest count among the independent fp32 implementations
    of the same launch, MISROUNDED_FLOOR elements where that count is under 50"""
    top = max(counts)
    return int(math.floor(MARGIN * top)) if top >= 50 else MISROUNDED_FLOOR


def conv_out_hw(H, W, k, stride, pad, upsample, out_hw=None):
    if out_hw is not None:
        return tuple(out_hw)
    Hin, Win = (2 * H, 2 * W) if upsample else (H, W)
    return (Hin + 2 * pad - k) // stride + 1, (Win + 2 * pad - k) // stride + 1


def silu_maps(N, C, H, W, ratio, dtype, seed=0, outlier_frac=0.01, outlier_gain=50.0):
    """post-SiLU activation maps [N, H, W, C] (what every 3x3 convolution of a ResnetBlock2D reads): silu of group_maps at |mean| / std
    = `ratio` per (sample, group) with 1 % outlier channels at x50, rounded to the storage dtype.  Asserted: the values are those of a
    SiLU (>= its minimum -0.2785, <= the peak), rounded, and in front of the SiLU the loudest channel's rms is >= 10 x the quietest
    channel's (group_maps standardises every group: an outlier channel stands x50 over the other channels of ITS group)."""
    groups = 32 if C % 32 == 0 else (8 if C % 8 == 0 else 1)
    x = group_maps(N, C, H, groups, ratio, outlier_frac, outlier_gain, 4.0, dtype, seed=seed, W=W)
    y = rnd(F.silu(x.double()), dtype)
    assert float(y.min()) >= -0.2785 * (1 + 2.0 ** -7) and float(y.max()) <= 4.0 and torch.equal(y, rnd(y, dtype))
    if outlier_frac > 0 and C >= 100:
        top = (x.double().reshape(N, -1, C) - x.double().reshape(N, -1, C).mean(dim=1, keepdim=True)).pow(2).mean(dim=(0, 1)).sqrt()
        assert float(top.max()) >= 10.0 * float(top.min()), (float(top.max()), float(top.min()))
    return y


def conv_case(N, H, W, C1, Cout, dtype, k=3, stride=1, pad=None, upsample=False, out_hw=None, C2=0, tails=(), temb=False, silu=False,
              scale=1.0, residual=False, residual_lo=False, bias=True, inputs="randn", weights="randn", seed=0, rep=1, nsrc=None, src=None,
              first=0, scale_dev=None):
    """One es_conv_gemm launch, everything seeded, NHWC and rounded to the storage dtype (returned in fp32): x [N, H, W, C1] (+ x2 with C2
    channels, + tail sources [N, Hout, Wout, Ct] of a 1x1 convolution summed in, + temb [N, Cout], + residual and its low word),
    w [Cout, C1 + C2, k, k], wt [Cout, sum(tails)], b fp32, and the geometry.
    rep > 1: a shared source (es_gemm_desc.x_nmod, ops.conv_gemm(..., x_rep=)).  "x_src" holds the nsrc = N // rep samples the launch is
             handed, "x" - what every reference reads - the N samples of the launch: sample i reads x_src[(first + i) % nsrc].  nsrc /
             src / first: the case is one weight group of a grouped launch - nsrc source samples (or `src`, the tensor another group
             of the same launch made) and `first`, the index of the group's first sample in the launch.
    scale_dev: a device scalar (es_gemm_desc.out_scale_dev).  "scale" - what every reference multiplies by - is the fp32 product
             float32(scale) * float32(scale_dev), as the kernels form it; the factors are kept as "scale_host" and "scale_dev".
    inputs:  "randn" zero-mean; "silu0" / "silu3" post-SiLU maps (silu_maps at ratio 0 / 3); "near_2^10" activations of magnitude about
             2^10 with random signs (for weights="subnormal"); "peak" randn scaled so that the largest fp64 OUTPUT lies at 2e4 .. 3e4.
    weights: "randn" / sqrt(fan-in); "subnormal" every |w| < 2^-14 (fp16 subnormals: a flush to zero returns the bias); "zero".
    Every postcondition is asserted."""
    assert (C1 + C2) % 8 == 0 and C1 % 8 == 0, "es_conv_gemm takes channels in multiples of 8 (conv_in is padded 4 -> 8)"
    g = _gen(seed + 15485863)
    pad = (1 if k == 3 else 0) if pad is None else pad
    Hout, Wout = conv_out_hw(H, W, k, stride, pad, upsample, out_hw)
    Ct, Ctot = sum(tails), C1 + C2
    if src is not None:
        nsrc = src.shape[0]
    elif nsrc is None and rep > 1:
        assert N % rep == 0, (N, rep)
        nsrc = N // rep
    if nsrc:
        assert not C2 and not tails and inputs != "peak", "a shared source is a single source (gemm_check)"
    Nx = nsrc or N                                # samples drawn for the source
    if src is not None:
        assert tuple(src.shape) == (nsrc, H, W, C1) and torch.equal(src, rnd(src, dtype))
        xa = src
    elif inputs in ("silu0", "silu3"):
        xa = silu_maps(Nx, Ctot, H, W, 0 if inputs == "silu0" else 3, dtype, seed=seed)
    elif inputs == "near_2^10":
        sgn = torch.where(torch.rand(Nx, H, W, Ctot, generator=g) < 0.5, -1.0, 1.0)
        xa = rnd(sgn * 1024.0 * (1 + 0.1 * torch.randn(Nx, H, W, Ctot, generator=g)), dtype)
        assert float(xa.abs().min()) > 512.0 and float(xa.abs().max()) < 2048.0
    else:
        xa = torch.randn(Nx, H, W, Ctot, generator=g)
        xa = rnd(xa - xa.mean(), dtype)
        assert abs(float(xa.double().mean())) < 1e-3
    x_src = None
    if nsrc:
        x_src = xa.contiguous()
        xa = x_src[(first + torch.arange(N)) % nsrc]
    fan = k * k * Ctot + Ct
    if weights == "subnormal":
        lim = 2.0 ** FP16_NORMAL_MIN_LOG2
        mk = lambda *s: rnd(lim * (0.1 + 0.89 * torch.rand(*s, generator=g)) * torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0), dtype)
    elif weights == "zero":
        mk = lambda *s: torch.zeros(*s)
    else:
        mk = lambda *s: rnd(torch.randn(*s, generator=g) / math.sqrt(fan), dtype)
    w = mk(Cout, Ctot, k, k)
    wt = mk(Cout, Ct) if Ct else None
    if weights == "subnormal":
        assert float(w.abs().max()) < 2.0 ** FP16_NORMAL_MIN_LOG2 and float((w != 0).double().mean()) > 0.99
    c = dict(dtype=dtype, N=N, H=H, W=W, C1=C1, C2=C2, Cout=Cout, k=k, stride=stride, pad=pad, upsample=bool(upsample),
             out_hw=(Hout, Wout), silu=bool(silu), scale=float(torch.tensor(scale, dtype=torch.float32)),
             scale_host=float(torch.tensor(scale, dtype=torch.float32)), scale_dev=None, x_src=x_src, nsrc=nsrc or 0, first=first if nsrc else 0,
             x=xa[..., :C1].contiguous(), x2=xa[..., C1:].contiguous() if C2 else None, w=w, wt=wt,
             b=(0.1 * torch.randn(Cout, generator=g)) if bias else None,
             tails=[rnd(torch.randn(N, Hout, Wout, t, generator=g), dtype) for t in tails],
             temb=rnd(torch.randn(N, Cout, generator=g), dtype) if temb else None, res=None, res_lo=None)
    if nsrc:
        assert all(torch.equal(c["x"][i], x_src[(first + i) % nsrc]) for i in range(N))
    if scale_dev is not None:   # scale *= *p.out_scale_dev: one fp32 product
        c["scale_dev"] = float(torch.tensor(scale_dev, dtype=torch.float32))
        c["scale"] = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(scale_dev, dtype=torch.float32))
    if residual:
        c["res"] = rnd(torch.randn(N, Hout, Wout, Cout, generator=g), dtype)
        if residual_lo:         # the low word of a value pair: what is left of a sum after its rounding - below half a unit of the high word
            full = c["res"].double() * (1 + 2.0 ** -9 * torch.randn(N, Hout, Wout, Cout, generator=g, dtype=torch.float64))
            c["res"] = rnd(full, dtype)
            c["res_lo"] = rnd(full - c["res"].double(), dtype)
    if inputs == "peak":
        for _ in range(3):
            top = float(conv_ref64(c).abs().max())
            if 2.2e4 <= top <= 2.8e4:
                break
            s = 2.5e4 / top
            c["x"] = rnd(c["x"] * s, dtype)
            if C2:
                c["x2"] = rnd(c["x2"] * s, dtype)
            c["tails"] = [rnd(t * s, dtype) for t in c["tails"]]
        top = float(conv_ref64(c).abs().max())
        assert 2.0e4 <= top <= 3.0e4, top
    if weights == "subnormal":                  # a flush of the weights would return the bias: the signal must stand clear of it
        sig = conv_ref64(c) - (c["b"].double() if bias else 0.0)
        assert float(sig.pow(2).mean().sqrt()) > 0.1, float(sig.pow(2).mean().sqrt())
    return c


def _conv_sources(c, t=lambda v: v):
    x = t(c["x"]) if c["x2"] is None else torch.cat([t(c["x"]), t(c["x2"])], dim=-1)
    return x.permute(0, 3, 1, 2)                # NCHW for F.conv2d


def _conv_plain(c, t):
    """the convolution (+ tail 1x1 convolution) without bias or epilogue, NHWC, in t's precision (t = .double() or .float())"""
    x = _conv_sources(c, t)
    if c["upsample"]:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    Hout, Wout = c["out_hw"]
    k, s, p = c["k"], c["stride"], c["pad"]
    need_h, need_w = (Hout - 1) * s + k - x.shape[2] - p, (Wout - 1) * s + k - x.shape[3] - p     # bottom / right padding of an explicit out_hw
    x = F.pad(x, (p, max(need_w, 0), p, max(need_h, 0)))
    y = F.conv2d(x, t(c["w"]), None, stride=s)[:, :, :Hout, :Wout]
    assert y.shape[2:] == (Hout, Wout), (y.shape, c["out_hw"])
    y = y.permute(0, 2, 3, 1)
    if c["tails"]:
        y = y + torch.cat([t(v) for v in c["tails"]], dim=-1) @ t(c["wt"]).t()
    return y


def conv_ref64(c):
    """the plain operation with the whole epilogue in fp64: ((conv + bias) + temb) -> SiLU -> * scale -> + residual (+ its low word)"""
    d = lambda v: v.double()
    y = _conv_plain(c, d)
    if c["b"] is not None:
        y = y + d(c["b"])
    if c["temb"] is not None:
        y = y + d(c["temb"])[:, None, None, :]
    if c["silu"]:
        y = F.silu(y)
    y = y * c["scale"]
    if c["res"] is not None:
        y = y + d(c["res"])
        if c["res_lo"] is not None:
            y = y + d(c["res_lo"])
    return y


def conv_torch32(c):
    """torch's own fp32 convolution with the epilogue in fp32, rounded where the kernel rounds: an independent order of summation"""
    return conv_epilogue(c, _conv_plain(c, lambda v: v.float()))


def conv_base_ref(c):
    """the textbook fp32 sequence with every op's output rounded to the storage dtype: conv + bias | tail conv | their sum | + temb |
    SiLU | * scale | + residual.  (The reference has no two-word stream: a low word is added with the residual.)"""
    dt = c["dtype"]
    f = lambda v: v.float()
    keep = dict(c, tails=[], wt=None)
    y = _conv_plain(keep, f)
    y = rnd(y + c["b"] if c["b"] is not None else y, dt)
    if c["tails"]:
        y = rnd(y + rnd(torch.cat(c["tails"], dim=-1) @ c["wt"].t(), dt), dt)
    if c["temb"] is not None:
        y = rnd(y + c["temb"][:, None, None, :], dt)
    if c["silu"]:
        y = rnd(F.silu(y), dt)
    if c["scale"] != 1.0:
        y = rnd(y * c["scale"], dt)
    if c["res"] is not None:
        y = rnd(y + (c["res"] if c["res_lo"] is None else c["res"] + c["res_lo"]), dt)
    return y


def conv_epilogue(c, acc, wide=False, defect=None, temb_rows=None):
    """csrc/gemm_conv.hip's epilogue on the fp32 accumulators [N, Hout, Wout, Cout]: ((acc + bias) + temb), SiLU, * scale, ROUND, then
    + residual in fp32 and ROUND AGAIN.  wide: the two-word stream - the fp32 sum over the rounded value, the residual and its low
    word, stored as hi = round(sum) and lo = round(sum - hi); returns (hi, lo).
    Planted: "scale_before_act" - silu(x * scale) where the design is silu(x) * scale."""
    dt = c["dtype"]
    y = acc.float()
    late_bias = defect == "late_bias" and c["b"] is not None
    if c["b"] is not None and not late_bias:
        y = y + c["b"]
    if c["temb"] is not None:
        y = y + (c["temb"][:, None, None, :] if temb_rows is None else temb_rows)
    sc = torch.tensor(c["scale"], dtype=torch.float32)
    if c["silu"] and defect == "scale_before_act":
        y = rnd(F.silu(y * sc), dt)
    else:
        y = rnd((F.silu(y) if c["silu"] else y) * sc, dt)
    if late_bias:
        y = rnd(y + c["b"], dt)
    if c["res"] is None:
        return y
    s = y + c["res"]
    if wide:
        if c["res_lo"] is not None:
            s = s + c["res_lo"]
        hi = rnd(s, dt)
        return hi, rnd(s - hi, dt)
    return rnd(s, dt)


def conv_im2col(c, korder=0, defect=None):
    """(A [M, K], Wm [Cout, K]) in the kernel's K order: tap-major (ky, kx, c) over the concatenated sources, or chunk-major
    (c / 64, ky, kx, c % 64) for korder 1, the tail channels last.  Rows are output pixels m = (n, oy, ox); a tap outside the
    (upsampled) image reads zero.  Geometry defects (planted):
      "hw_swapped"       the pixel decode divides by Hout where it should divide by Wout
      "right_tap"        the right-hand tap column (kx = k - 1) is dropped at ox == Wout - 1
      "wrap_next_sample" a tap below the last row of sample n reads row 0 .. of sample n + 1 (a flat offset with no range check)
    With a shared source (conv_case(rep= | nsrc=)) row m of sample n reads source sample (first + n) % nsrc.  Planted there:
      "mod_per_tile"     every row of a 128-row tile reads the source sample of the tile's FIRST row (modulo nsrc): the modulo taken once
                         per workgroup.  Identical to the design where no tile straddles a sample (H * W % 128 == 0)
      "mod_in_group"     the modulo is taken of the sample's index inside its weight group (n % nsrc, without `first`): identical to the
                         design unless the group starts at a launch index that is no multiple of nsrc"""
    N, H, W, k, s, p = c["N"], c["H"], c["W"], c["k"], c["stride"], c["pad"]
    Hout, Wout = c["out_hw"]
    x = c["x"] if c["x2"] is None else torch.cat([c["x"], c["x2"]], dim=-1)
    if defect in ("mod_per_tile", "mod_in_group"):
        assert c.get("nsrc"), f"{defect} is a defect of the shared source"
    up = 1 if c["upsample"] else 0
    Hin, Win = H << up, W << up
    Ctot = x.shape[-1]
    m = torch.arange(N * Hout * Wout)
    n, rem = m // (Hout * Wout), m % (Hout * Wout)
    oy, ox = (rem // Wout, rem % Wout) if defect != "hw_swapped" else (rem // Hout, rem % Hout)
    if defect == "mod_per_tile":                 # (groups start on whole tiles: the case's tiles are the launch's)
        x, n, N = c["x_src"], (c["first"] + (m // BM_CONV) * BM_CONV // (Hout * Wout)) % c["nsrc"], c["nsrc"]
    elif defect == "mod_in_group":
        x, n, N = c["x_src"], n % c["nsrc"], c["nsrc"]
    cols = []
    for ky in range(k):
        for kx in range(k):
            iy, ix = oy * s - p + ky, ox * s - p + kx
            ok = (iy >= 0) & (iy < Hin) & (ix >= 0) & (ix < Win)
            nn, yy = n, iy
            if defect == "wrap_next_sample":
                wrap = (iy >= Hin) & (ix >= 0) & (ix < Win) & (n + 1 < N)
                nn, yy = torch.where(wrap, n + 1, n), torch.where(wrap, iy - Hin, iy)
                ok = ok | wrap
            if defect == "right_tap" and kx == k - 1:
                ok = ok & (ox != Wout - 1)
            v = x[nn.clamp(0, N - 1), (yy >> up).clamp(0, H - 1), (ix >> up).clamp(0, W - 1)]
            cols.append(torch.where(ok[:, None], v, torch.zeros_like(v)))
    A = torch.stack(cols, dim=1)                                        # [M, k * k, Ctot]
    Wm = c["w"].permute(0, 2, 3, 1).reshape(c["Cout"], k * k, Ctot)
    if korder == 1:
        assert k == 3 and Ctot % 64 == 0 and c["C1"] % 64 == 0
        A = A.reshape(-1, k * k, Ctot // 64, 64).permute(0, 2, 1, 3)
        Wm = Wm.reshape(-1, k * k, Ctot // 64, 64).permute(0, 2, 1, 3)
    A, Wm = A.reshape(A.shape[0], -1), Wm.reshape(c["Cout"], -1)
    if c["tails"]:
        A = torch.cat([A] + [t.reshape(-1, t.shape[-1]) for t in c["tails"]], dim=1)
        Wm = torch.cat([Wm, c["wt"]], dim=1)
    return A.contiguous(), Wm.contiguous()


def _chain_dot(A, Wm, width, init=None):
    """init (fp32 [rows of Wm]): the value every chain STARTS from (es_linear_xs: the bias is the C operand of the first MFMA).
    fp32 accumulators of A Wm^T formed as es_conv_gemm's matrix-core chain forms them (see _chain_sums, "mfma8"): one `width`-wide
    partial dot product after the other, each taken exactly (fp64) and added with one rounding to fp32.  width 8: what a lane
    supplies to a 16x16x32 MFMA; width 32: one rounding per instruction - the other reading of the same hardware."""
    M, K = A.shape
    pad = (-K) % width
    if pad:
        A, Wm = F.pad(A, (0, pad)), F.pad(Wm, (0, pad))
    G = (K + pad) // width
    Ad = A.double().reshape(M, G, width).permute(1, 0, 2)
    Wd = Wm.double().reshape(-1, G, width).permute(1, 2, 0)
    acc = torch.zeros(M, Wm.shape[0], dtype=torch.float32) if init is None else init.float()[None, :].expand(M, -1).clone()
    for g0 in range(0, G, 64):
        part = torch.bmm(Ad[g0:g0 + 64], Wd[g0:g0 + 64])
        for j in range(part.shape[0]):
            acc = (acc.double() + part[j]).float()
    return acc


def conv_splitk_slices(K, splitk):
    """[k0, k1) of every split-K slice: the kernel cuts the Kpad / 64 K-steps at floor(nk * z / splitk)"""
    nk = (K + 63) // 64
    return [(64 * (nk * z // splitk), min(K, 64 * (nk * (z + 1) // splitk))) for z in range(splitk)]


def conv_base_alg(c, chain=8, splitk=1, korder=0, wide=False, defect=None):
    """The launch as designed, in fp32 on the CPU: im2col in the kernel's K order, chains of `chain`-wide partial dot products, split-K
    slices cut where the kernel cuts them - each its own fp32 chain, the slabs summed in slice order in fp32 - then the kernel's
    epilogue (conv_epilogue).  wide: returns (hi, lo) of the two-word stream.
    Planted defects: conv_im2col's geometry defects, and
      "rounded_slabs"   the split-K slabs are rounded to the storage dtype before the reduce
      "late_bias"       the bias is added behind the rounding (and the sum rounded again)
      "tile_unwritten"  the second 128-pixel tile (the last, if there is one only) is never stored: NaN, as a sentinel-filled output shows it
      "temb_first_pixel" every pixel of a 128-pixel tile takes the time-embedding row of the tile's FIRST pixel's sample
      "dev_scale_dropped_in_reduce"  with splitk > 1 (the epilogue is the reduce kernel's) only the host out_scale is applied
      "scale_before_act" conv_epilogue's"""
    dt = c["dtype"]
    N, (Hout, Wout), Cout = c["N"], c["out_hw"], c["Cout"]
    A, Wm = conv_im2col(c, korder, defect if defect in ("hw_swapped", "right_tap", "wrap_next_sample", "mod_per_tile", "mod_in_group") else None)
    if defect == "dev_scale_dropped_in_reduce" and splitk > 1:
        c = dict(c, scale=c["scale_host"])
    acc = None
    for k0, k1 in conv_splitk_slices(A.shape[1], splitk):
        slab = _chain_dot(A[:, k0:k1], Wm[:, k0:k1], chain) if k1 > k0 else torch.zeros(A.shape[0], Cout)
        if defect == "rounded_slabs":
            slab = rnd(slab, dt)
        acc = slab if acc is None else acc + slab
    temb_rows = None
    if defect == "temb_first_pixel":
        m = torch.arange(N * Hout * Wout)
        first = (m // BM_CONV) * BM_CONV // (Hout * Wout)
        temb_rows = c["temb"][first].reshape(N, Hout, Wout, Cout)
    out = conv_epilogue(c, acc.reshape(N, Hout, Wout, Cout), wide, defect, temb_rows)
    if defect == "tile_unwritten":
        M = N * Hout * Wout
        t0 = BM_CONV if M > BM_CONV else 0
        for o in (out if wide and c["res"] is not None else (out,)):
            o.reshape(M, Cout)[t0:t0 + BM_CONV] = float("nan")
    return out


def conv_baselines(c, splitk=1, korder=0, wide=False):
    """name -> result of the independent fp32 implementations of one launch that set the misrounded bar (the GPU test adds the device
    library's unfold + matmul): base_alg with chains of 8, with chains of 32, torch's fp32 convolution.  wide (with a residual): (hi, lo) pairs."""
    out = {"alg8": conv_base_alg(c, 8, splitk, korder, wide), "alg32": conv_base_alg(c, 32, splitk, korder, wide)}
    t = _conv_plain(c, lambda v: v.float())
    out["torch32"] = conv_epilogue(c, t, wide)
    return out


# ----------------------------------------------------------------------------------------------------------------
# a VAE-decoder up block: ResnetBlock2D x 3 (GroupNorm -> SiLU -> conv3x3, twice, + x) and nearest 2x upsampling + conv3x3
# ----------------------------------------------------------------------------------------------------------------
def vae_up_block(sd, p, x, groups, eps, mode, dtype=None, peaks=None, nres=3):
    """x [N, C, H, W].  mode "ref64": the plain block in fp64; "fp32": the same in fp32 (what the reference runs its VAE in), the
    output rounded once; "ref": fp32 with EVERY op's output rounded to the storage dtype (GroupNorm, SiLU, convolution, sum);
    "alg": what the engine's launches are designed to compute - GroupNorm with one-pass chunked statistics and x * a + b -> SiLU
    rounded once, convolution + bias (+ residual) in the fp32 accumulator rounded once.  peaks: a list that receives max|t| of every
    tensor the block stores."""
    import torch.nn.functional as F
    f64 = mode == "ref64"
    cast = (lambda t: t.double()) if f64 else (lambda t: t.float())
    r = (lambda t: rnd(t, dtype)) if mode in ("ref", "alg") else (lambda t: t)

    def note(t):
        if peaks is not None:
            peaks.append(float(t.abs().max()))
        return t

    def gn_silu(t, q):
        w, b = cast(sd[q + ".weight"]), cast(sd[q + ".bias"])
        if mode != "alg":
            return note(r(F.silu(note(r(F.group_norm(t, groups, w, b, eps))))))
        N, C, H, W = t.shape
        tg = t.permute(0, 2, 3, 1).reshape(N, H * W, groups, C // groups)
        mean, rstd = gn_chunked_stats(tg, eps)
        a = (rstd.expand(N, 1, groups, C // groups).reshape(N, 1, C) * w)
        sh = b - mean.expand(N, 1, groups, C // groups).reshape(N, 1, C) * a
        y = F.silu(t.permute(0, 2, 3, 1).reshape(N, H * W, C) * a + sh)
        return note(r(y).reshape(N, H, W, C).permute(0, 3, 1, 2).contiguous())

    def conv(t, q, res=None):
        y = F.conv2d(t, cast(sd[q + ".weight"]), cast(sd[q + ".bias"]), padding=1)
        if res is None:
            return note(r(y))
        return note(r(y + res)) if mode == "alg" else note(r(note(r(y)) + res))

    h = note(cast(x))
    for j in range(nres):
        q = f"{p}.resnets.{j}"
        t = conv(gn_silu(h, q + ".norm1"), q + ".conv1")
        h = conv(gn_silu(t, q + ".norm2"), q + ".conv2", res=h)
    h = conv(F.interpolate(h, scale_factor=2.0, mode="nearest"), f"{p}.upsamplers.0.conv")
    return rnd(h, dtype) if mode == "fp32" else h


# ----------------------------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------------------------
def _heads(t, heads):
    N, S, Cc = t.shape
    return t.reshape(N, S, heads, Cc // heads).transpose(1, 2)


def _unheads(o):
    N, h, S, d = o.shape
    return o.transpose(1, 2).reshape(N, S, h * d)


def attn_ref64(q, k, v, heads, scale=None):
    w = torch.softmax(_softmax64(q, k, heads, scale), dim=-1)
    return _unheads(w @ _heads(v.double(), heads))


def attn_base_ref(q, k, v, heads, dtype, scale=None):
    """fp32 scores, softmax against the TRUE maximum, P rounded to the storage dtype with subnormals, P V in fp32, rounded"""
    d = q.shape[-1] // heads
    s = _heads(q.float(), heads) @ _heads(k.float(), heads).transpose(-1, -2) * (scale if scale is not None else 1.0 / math.sqrt(d))
    p = rnd(torch.softmax(s, dim=-1), dtype)
    return rnd(_unheads(p @ _heads(v.float(), heads)), dtype)


def attn_base_alg(q, k, v, heads, dtype, scale=None, offset=0.0, defect=None, tile=64, rowsum="fp32"):
    """csrc/attention.hip's design: Q pre-multiplied by scale * log2(e) and re-rounded to the storage dtype; P = 2^(s - m) with a
    reference m that sits `offset` (0 .. LAZY) below the row maximum; the row sum from the fp32 P, P rounded to the storage dtype
    for the P V product (fp32 accumulation), the quotient rounded once.
    rowsum="rounded": the ONES forms (head widths with d % 16 == 8: 8, 24, 40 - every kernel that runs them) keep 1.0 in V's first pad
    column, so the row sum comes out of the matrix core with the P V product: it is the sum of the ROUNDED P.
    defects: "flush_p" - P below 2^-14 becomes zero on its way into the product (a conversion or a matrix core that flushes fp16
    subnormals); "stale_reference" - the reference stays at the FIRST tile's maximum and is never raised, so P overflows the
    storage dtype's range where later tiles rise; "pad_key_admitted" - one key of a ragged tile's padding (zero K row: score 0, zero V
    row) joins the softmax; "last_key_dropped" - the last valid key is left out."""
    d = q.shape[-1] // heads
    sl2 = (scale if scale is not None else 1.0 / math.sqrt(d)) * 1.4426950408889634
    kh, vh = _heads(k.float(), heads), _heads(v.float(), heads)
    if defect == "pad_key_admitted":
        kh = torch.cat([kh, torch.zeros_like(kh[:, :, :1])], dim=2)
        vh = torch.cat([vh, torch.zeros_like(vh[:, :, :1])], dim=2)
    if defect == "last_key_dropped":
        assert kh.shape[2] >= 2
        kh, vh = kh[:, :, :-1], vh[:, :, :-1]
    s = _heads(rnd(q.float() * sl2, dtype), heads) @ kh.transpose(-1, -2)
    if defect == "stale_reference":
        m = s[..., :tile].max(dim=-1, keepdim=True).values
    else:
        m = s.max(dim=-1, keepdim=True).values - float(offset)
    p = torch.exp2(s - m)
    l = p.sum(dim=-1, keepdim=True)
    if defect == "flush_p":
        p = torch.where(p < 2.0 ** FP16_NORMAL_MIN_LOG2, torch.zeros_like(p), p)
    p = rnd(p, dtype)
    if rowsum == "rounded":
        l = p.sum(dim=-1, keepdim=True)
    else:
        assert rowsum == "fp32"
    return rnd(_unheads((p @ vh) / l), dtype)


def attn_ones(d) -> bool:
    """head widths whose kernels take the row sum from the ones column (rowsum="rounded")"""
    return d % 16 == 8


def attn_design_err(q, k, v, heads, dtype, ref64, scale=None, rowsum="fp32"):
    """row_err of the design: the worse of the two ends of the reference's allowed range (at the maximum: small P lowest; LAZY
    below it: large P highest)"""
    return max(row_err(attn_base_alg(q, k, v, heads, dtype, scale, offset=o, rowsum=rowsum), ref64) for o in (0.0, LAZY))


ATTN_WIDTHS = (8, 16, 24, 32, 40, 48, 64, 80, 128, 160, 512)            # the head widths es_attention has a kernel for
ATTN_KNOBS = dict(kvres=1, big_thr=512, attn32=1, qb=2, pp=-1)          # ES_ATTN_KVRES | _BIG | ATTN32 | _QB | _PP unset
ATTN_ROUTE_KEYS = ("kernel", "q_per_wg", "q_per_wave", "grid_x", "grid_y", "grid_z", "threads", "lds", "qper")


def attn_route(N, heads, Sq, Skv, d, knobs=None):
    """Python mirror of attn_route() in csrc/attention.hip, keyed like lib.ATTN_ROUTE_FIELDS: which kernel (es_attention_last_kernel's ids)
    a launch goes to under `knobs` (a dict like ATTN_KNOBS; None: the defaults), with which grid, LDS size and - K/V-resident kernel -
    strip length.  Written from the rules, not from the library's table (the generic kernel's tile is a formula of d here); the tables of
    tests/test_attention_gpu.py are placed with it without a GPU, and tests/test_host_cpu.py holds it to es_attention_route."""
    k = ATTN_KNOBS if knobs is None else knobs
    assert d in ATTN_WIDTHS and min(N, heads, Sq, Skv) >= 1
    cdiv = lambda a, b: (a + b - 1) // b

    def tiled(kernel, q_per_wg, q_per_wave, threads, lds):
        return dict(kernel=kernel, q_per_wg=q_per_wg, q_per_wave=q_per_wave, grid_x=cdiv(Sq, q_per_wg), grid_y=heads, grid_z=N, threads=threads,
                    lds=lds, qper=0)

    if k["kvres"] != 0 and Skv <= 96 and Sq >= 64 and d in (40, 80):
        groups = cdiv(heads, 8) * N
        if k["kvres"] == 2 or groups >= (12 if d == 40 else 64):
            blocks32 = cdiv(Sq, 32)
            strips = max(1, min(256 // groups, blocks32))
            qper = cdiv(blocks32, strips) * 32
            return dict(kernel=7, q_per_wg=qper, q_per_wave=32, grid_x=cdiv(Sq, qper), grid_y=cdiv(heads, 8), grid_z=N, threads=512,
                        lds=3 * 32 * (min(heads, 8) * d * 2 + 16), qper=qper)          # three tiles of 32 whole rows (+ 16 B): Q twice, O
    big = cdiv(Sq, 128) * heads * N >= k["big_thr"]
    ring32 = lambda: 2 * 2 * 64 * (16 * cdiv(d, 16) * 2 + 16)           # two slots of a 64-key K tile and V tile, rows of d padded to 16 (+ 16 B)
    if big and k["attn32"] != 0:
        wg256 = cdiv(Sq, 256) * heads * N
        if d == 40 and k["pp"] != 0 and Skv % 64 == 0 and Skv >= 128:
            if k["pp"] == 2:
                return tiled(6, 512, 64, 512, ring32())
            if k["pp"] == 1 or (k["pp"] == -1 and wg256 >= 256):
                return tiled(5, 256, 32, 512, ring32())
        if d == 40 and k["qb"] == 2 and wg256 >= k["big_thr"]:
            return tiled(4, 256, 64, 256, ring32())
        if d == 40 or (d == 80 and k["attn32"] == 2):
            return tiled(3, 128, 32, 256, ring32())
    # the generic kernel: four waves; 16 queries per wave only at 40 | 48 | 80 in launches that are not big, and at 512
    two_forms = d in (40, 48, 80)
    w = 16 if d == 512 or (two_forms and not big) else 32
    kvt, ks, df = (32 if d == 512 else 64), cdiv(d, 32), cdiv(d, 16)
    lds = (2 if ks <= 5 else 1) * kvt * ((32 * ks * 2 + 16) + (16 * df * 2 + 16))
    return tiled(2 if (big and two_forms) else 1, 4 * w, w, 256, lds)


GEMM_ROUTE_KEYS = ("kernel", "row", "family", "bn", "stages", "waves", "aligned", "grid", "threads", "lds", "reduce", "reduce_cb", "reduce_grid",
                   "reduce_threads", "runs", "samples_per_run")


def gemm_kernel_id(bm, bn, stages, waves, aligned, ln, ko, geglu, bf16) -> int:
    """es_conv_gemm_last_kernel of an instantiation (include/edgestyle_hip.h ES_GEMM_KERNEL_*): couts per workgroup in bits 0-8, pixels / 64
    in 9-11, ring depth in 12-14, then one bit each for 8 waves, aligned channels, LayerNorm fold, chunk-major K, GEGLU (big tile), bf16"""
    return bn | (bm // 64) << 9 | stages << 12 | (waves == 8) << 15 | bool(aligned) << 16 | bool(ln) << 17 | bool(ko) << 18 | bool(geglu) << 19 | \
        bool(bf16) << 20


def gemm_big_tile_takes(d) -> bool:
    """whether the phase-interleaved 256-pixel kernel has the epilogue a launch recorded with bn = 320 | 256 needs (csrc/gemm_conv8p.hip,
    DESIGN section 4): split-K partials of the 320 tile always; else no SiLU, whole 8-channel stores, and a time embedding only as one row
    per 128-pixel half without a residual.  The 256-wide form: no time embedding at all, GEGLU only as the bare projection, and neither
    GEGLU nor the LayerNorm fold with split-K or a GroupNorm hand-over."""
    geglu, hw = d.act == 2, d.Hout * d.Wout
    if d.Cout % 8:
        return d.bn == 320 and d.splitk > 1
    if d.bn == 320:
        return d.splitk > 1 or (d.act == 0 and not (d.temb and (hw % 128 or d.residual)))
    if d.temb or d.act == 1:
        return False
    bare = not (d.splitk > 1 or d.gn_part)
    return (not geglu or (bare and not d.residual and not d.out_lo)) and (not d.ln_colsum or bare)


def gemm_route(d, limit=0x7FFFFFFF):
    """Python mirror of gemm_route() in csrc/gemm_conv.hip for a descriptor es_conv_gemm accepts (any object with es_gemm_desc's fields;
    pointers count as present or absent), keyed like lib.GEMM_ROUTE_FIELDS with row = None: the mirror names the instantiation by its
    template arguments, not by its place in the library's table.  Written from the rules (header of csrc/gemm_conv.hip):
    which ring depths and wave counts exist for which tile, not the order in which the library looks them up."""
    cdiv = lambda a, b: (a + b - 1) // b
    hw, ln, geglu = d.Hout * d.Wout, bool(d.ln_colsum), d.act == 2
    aligned = d.C1 % 64 == 0 and d.C2 % 64 == 0
    bn, stages = d.bn, d.stages or 2
    big = bn in (320, 256) and gemm_big_tile_takes(d)
    if bn in (320, 256) and not big:
        bn, stages = bn // 2, 2             # the tile of half the width, as the planner would have launched it
    if big:
        bm, waves, stages, ko = 256, 8, 2, bn == 320 and d.korder == 1
    else:
        bm = 64 if bn == 64 else 128
        waves = 8 if (d.waves == 8 and bm == 128 and aligned) else 4
        # ring depths that exist: 2 everywhere; 4 on aligned channels except 8 waves x 160; 3 only for the plain 4-wave 128-pixel tile
        have = {2}
        if aligned and not (waves == 8 and bn == 160):
            have.add(4)
        if aligned and bm == 128 and waves == 4 and not ln:
            have.add(3)
        stages = stages if stages in have else 2
        ko = d.korder == 1 and aligned and not ln
    kid = gemm_kernel_id(bm, bn, stages, waves, aligned or big, ln, ko, big and geglu, d.dtype == 1)
    # operands beyond `limit` bytes: runs of whole samples per weight group
    cs = d.Cout // 2 if geglu else d.Cout
    per = max(0 if d.x_nmod else d.Hsrc * d.Wsrc * max(d.C1, d.C2) * 2, hw * cs * 2, hw * max(d.Ct1, d.Ct2) * 2 if d.t1 else 0)
    slab_rows = hw * (d.rows_padded // 8)
    over = per * d.N >= limit or (d.x_nmod and d.x_nmod * d.Hsrc * d.Wsrc * d.C1 * 2 >= limit) or (d.splitk > 1 and d.N * slab_rows >= 2 ** 31)
    N, runs, ns = d.N, 1, d.N
    if over:
        ns = (limit - 1) // per
        if d.splitk > 1:
            ns = min(ns, (2 ** 31 - 1) // slab_rows)
        if hw == 1 and ns >= 256:
            ns -= ns % 256
        if d.x_nmod:
            ns -= ns % d.x_nmod
        ends = [d.mt_end[g] * 128 // hw for g in range(d.ngroups)] if d.ngroups > 1 else [d.N]
        runs = sum(cdiv(e - s, ns) for s, e in zip([0] + ends, ends))
        N = min(ns, ends[0])
    M = N * hw
    r = dict(kernel=kid, row=None, family=int(big), bn=bn, stages=stages, waves=waves, aligned=int(aligned), grid=cdiv(M, bm) * (d.rows_padded // bn) * d.splitk,
             threads=64 * waves, lds=stages * (bm + bn) * 64 * 2, reduce=0, reduce_cb=0, reduce_grid=0, reduce_threads=0, runs=runs, samples_per_run=ns)
    if d.splitk > 1 and d.gn_part:
        cb = {320: 80, 160: 80, 128: 128}.get(bn, 64)          # the statistics' two-entry scheme assumes the N tile of the 4-wave kernels
        r.update(reduce=2, reduce_cb=cb, reduce_grid=(M // 64) * (d.rows_padded // cb), reduce_threads=64 * cb // 8)
    elif d.splitk > 1:
        r.update(reduce=1, reduce_grid=cdiv(M * (d.rows_padded // 8), 256), reduce_threads=256)
    return r


# ----------------------------------------------------------------------------------------------------------------
# The launch policy (csrc/launch_policy.hip): independent restatements of its planner, of where es_linear_xs is taken and of how such a
# launch is cut into slices (tests/test_load_weights_cpu.py and tests/test_host_cpu.py sweep the library against them)
# ----------------------------------------------------------------------------------------------------------------
PLAN_BK, PLAN_BM = 64, 128
PLAN_T160, PLAN_ALONE, PLAN_TFIX, PLAN_RED_FIX, PLAN_SLAB_BYTES_PER_UNIT = 1.25, 0.9, 2.0, 12.0, 4.0e6
PLAN_T320, PLAN_BIG_MIN_M, PLAN_T320_FIX, PLAN_BIG_MIN_NK = 2.3, 2048, 3.0, 16
PLAN_T256, PLAN_T256_FIX, PLAN_T256_GEGLU, PLAN_LN_TK, PLAN_T256_MARGIN = 2.6, 6.0, 7.0, 1.55, 0.93
PLAN_T64_ALONE, PLAN_T64, PLAN_T64_LONG, PLAN_SMALL_MAX_M = 0.5, 0.16, 1.5, 16384
PLAN_MIN_SLICE, PLAN_NK_NOSPLIT, PLAN_RESIDENT = 12, 10, 512


def plan_gemm_reference(M: int, rows_padded: int, kpad: int, geglu: bool = False, bns=(160, 128, 64), allow_split: bool = True, deep_ring: bool = True):
    """An independent restatement of the library's planner (csrc/launch_policy.hip plan_gemm): (bn, splitk, stages) with the
    lowest modelled time among the legal N tiles (ties go to the wider tile).  bn = 256 (the 256 x 256 phase-interleaved tile,
    offered for the LayerNorm-folded / GEGLU linear layers whose N is a multiple of 256) is decided AFTER the choice among the
    other tiles, on a model fitted on those layers (tools/ln256_bench.py).  deep_ring False (the knob, or a concurrent chain of the Python
    host): no 4-deep ring."""
    if 256 in bns:
        others = tuple(b for b in bns if b != 256)
        nk = kpad // PLAN_BK
        other = None
        if others:
            try:
                other = plan_gemm_reference(M, rows_padded, kpad, geglu, others, allow_split, deep_ring)
            except EdgeStyleHipError:
                other = None
        if rows_padded % 256:
            if other is None:
                raise EdgeStyleHipError(f"plan_gemm: rows_padded {rows_padded} fits no N tile")
            return other
        t256 = ((M + 255) // 256) * (rows_padded // 256)
        c256 = float(-(-t256 // 256)) * (nk * PLAN_T256 + PLAN_T256_FIX + (PLAN_T256_GEGLU if geglu else 0.0))
        take = other is None
        if other is not None and M >= PLAN_BIG_MIN_M and nk >= PLAN_BIG_MIN_NK and other[1] == 1 and other[0] != 64:
            to = ((M + PLAN_BM - 1) // PLAN_BM) * (rows_padded // other[0])
            co = float(-(-to // PLAN_RESIDENT)) * (nk * PLAN_LN_TK * (PLAN_T160 if other[0] == 160 else 1.0) + PLAN_T256_FIX)
            take = c256 < PLAN_T256_MARGIN * co
        return (256, 1, 2) if take else other
    if geglu:
        return 128, 1, 2
    nk = kpad // PLAN_BK
    best = None
    for bn in bns:
        if rows_padded % bn:
            continue
        if bn == 320 and (M < PLAN_BIG_MIN_M or nk < PLAN_BIG_MIN_NK) and len(bns) > 1:
            continue
        if bn == 64 and M > PLAN_SMALL_MAX_M and len(bns) > 1:
            continue
        bm = {320: 256, 64: 64}.get(bn, PLAN_BM)
        resident = {320: PLAN_RESIDENT // 2, 64: 2 * PLAN_RESIDENT}.get(bn, PLAN_RESIDENT)
        tiles = ((M + bm - 1) // bm) * (rows_padded // bn)
        cands = [1]
        if allow_split and tiles < resident // 2 and nk > PLAN_NK_NOSPLIT:
            cands += list(range(2, min(nk // PLAN_MIN_SLICE, 32) + 1))
        for sk in cands:
            wgs = tiles * sk
            if bn == 320:
                tk = PLAN_T320
            elif bn == 64:
                if sk > 1 and wgs > PLAN_RESIDENT:
                    continue
                w = wgs / (PLAN_RESIDENT // 2)                 # workgroups per CU
                tk = (PLAN_T64_ALONE + PLAN_T64 * max(0.0, w - 1.0) ** 2) * (1.0 if nk <= 40 else PLAN_T64_LONG)
            else:
                tk = (PLAN_T160 if bn == 160 else 1.0) * (PLAN_ALONE if wgs <= PLAN_RESIDENT // 2 else 1.0)
            # rounds of workgroups: whole ones for the two-per-CU tiles; the 256 x 320 tile (one workgroup per CU, long tiles) is
            # measured to cost its FRACTIONAL number of rounds - 896 tiles = 3.5 rounds run in 3.5 tile times, the CUs of a part-filled
            # round run faster (tools/plan_fit_bench.py, round 4) - and no less than 0.9 of a round
            rounds = max(wgs / 256.0, 0.9) if bn == 320 else float(-(-wgs // resident))
            t = rounds * ((nk / sk) * tk + (PLAN_T320_FIX if bn == 320 else PLAN_TFIX))
            if sk > 1:
                t += PLAN_RED_FIX + sk * M * rows_padded * 8.0 / PLAN_SLAB_BYTES_PER_UNIT
            if best is None or t < best[0]:
                best = (t, bn, sk, wgs)
    if best is None:
        raise EdgeStyleHipError(f"plan_gemm: rows_padded {rows_padded} fits no N tile")
    _, bn, sk, wgs = best
    # at most one workgroup per CU: a 4-deep LDS ring (3 K-steps of DMA in flight) hides the HBM round trip that the
    # 2-stage ring leaves exposed when no second workgroup shares the CU.  Not inside concurrent chains of the Python host (ops.LANE > 0,
    # ES_CHAIN_MODE=streams): there 2 stages = 72 KB LDS let workgroups of different chains share a CU.
    if bn == 64:
        stages = 4 if (deep_ring and wgs <= PLAN_RESIDENT and nk // sk >= 6) else 2
    else:
        stages = 4 if (bn != 320 and deep_ring and wgs <= PLAN_RESIDENT // 2 and nk // sk >= 6) else 2
    return bn, sk, stages


def xs_shape_reference(M: int, pw, min_m: int) -> bool:
    """An independent restatement of the library's es_linear_xs_eligible (min_m = 8192) / "can the kernel run this" (min_m = 0):
    csrc/launch_policy.hip xs_shape_ok.  pw: an ops.PackedWeight.  K = 320 | 640 linear layers with an output width of whole 128-byte
    lines: the to_q|k|v and GEGLU projections of the 64x64 and 32x32 levels."""
    if pw.ksize != 1 or pw.kpad not in (320, 640) or pw.cin != pw.kpad or pw.ctail:
        return False
    ch = 64 if pw.kpad == 320 else 32
    line = ch * (128 // (ch if pw.geglu else 2 * ch))        # GEMM columns per 128-byte output line
    if pw.cout % line or pw.cout < 4 * line:
        return False
    # where it wins (tools/xs_bench.py, batch-1 shapes): 1.4-1.6x on the 14-sample launches of both levels and 1.05-1.1x on
    # the decoder's wide K = 320 projections; it loses where a workgroup's share of N is a few chunks (the activation
    # rows are re-read per slice and the 40 KB stages no longer amortise): small M with K = 640, narrow N at small M
    if min_m and (M < min_m or (M < 4 * min_m and pw.cout < (960 if pw.kpad == 320 else 1920))):
        return False
    return True


XS_WGS_WANTED = 256             # workgroups an es_linear_xs launch is cut towards


def xs_slices_reference(M: int, kpad: int, cout: int, geglu: bool, force_slices: int = 0):
    """An independent restatement of es_launch_xs_slices: (nslices, chunks_per_slice) of an es_linear_xs launch over M rows, or None where
    the kernel does not run the shape (K, no row, Cout not in whole 128-byte lines).  The arithmetic ops.linear_xs used to write out."""
    if M < 1 or kpad not in (320, 640):
        return None
    ch = 64 if kpad == 320 else 32
    pline = 128 // (ch if geglu else 2 * ch)                # chunks per 128-byte output line
    total = cout // ch
    lines = total // pline
    if cout % (ch * pline) or lines < 1:
        return None
    rbs = (M + 255) // 256
    want = max(1, min(lines, XS_WGS_WANTED // rbs))
    if force_slices > 0:
        want = max(1, min(lines, force_slices))
    lps = -(-lines // want)                                  # lines per slice
    nslices = -(-lines // lps)
    return nslices, lps * pline


ATTN_INPUT_KINDS = ("randn", "shift-300", "shift+300", "last_key_decides", "one_loud_query", "loud_values_2e4")


def attn_inputs(kind, N, heads, Sq, Skv, d, dtype, seed):
    """(q, k, v) of one input class of the ragged-length cases, at any Skv >= 1 ("one_loud_query", "last_key_decides": Skv >= 2; the
    loud key of one_loud_query sits among the last 16 keys - the ragged tile)"""
    if kind == "randn":
        g = _gen(seed)
        return tuple(rnd(torch.randn(N, S, heads * d, generator=g, dtype=torch.float64), dtype) for S in (Sq, Skv, Skv))
    if kind in ("shift-300", "shift+300"):
        return common_shift(N, heads, Sq, Skv, d, 300.0 if kind == "shift+300" else -300.0, dtype, seed=seed)
    if kind == "last_key_decides":
        return last_key_decides(N, heads, Sq, Skv, d, dtype, seed=seed)
    if kind == "one_loud_query":
        return one_loud_query(N, heads, Sq, Skv, d, wave=32, dtype=dtype, seed=seed)
    assert kind == "loud_values_2e4", kind
    return loud_values(N, heads, Sq, Skv, d, 2.0e4, dtype, seed=seed)


# Ragged lengths and poisoned views (tests/test_attention_gpu.py).  The kernels read K and V through buffer resources whose range check does
# the predication and Q under `chunk < d / 8` with a clamped row: what lies behind a view must never reach the result, whatever it holds.
ATTN_NAN_BITS = {torch.float16: 0x7E5A, torch.bfloat16: 0x7FA5}         # quiet NaNs with a payload no arithmetic produces
ATTN_HUGE = {torch.float16: 6.0e4, torch.bfloat16: 3.0e38}              # finite, alternating sign: a max-reduction hides a NaN, not these
ATTN_GUARD_ROWS = 64
ATTN_PAD_COLS = 8


def attn_poison_fill(numel, dtype, poison):
    """flat tensor of the storage dtype filled with the poison: "nan" (the payload NaN) or "huge" (+-ATTN_HUGE, alternating)"""
    if poison == "nan":
        return torch.full((numel,), ATTN_NAN_BITS[dtype], dtype=torch.int16).view(dtype)
    assert poison == "huge"
    t = torch.full((numel,), ATTN_HUGE[dtype], dtype=torch.float32)
    t[1::2] = -ATTN_HUGE[dtype]
    t = t.to(dtype)
    assert bool(torch.isfinite(t.float()).all()) and float(t.float().abs().min()) >= 0.99 * ATTN_HUGE[dtype]
    return t


def view_recipe(t):
    """(storage offset, size, stride) of a view: with the whole buffer (t._base) enough to make the same view again elsewhere"""
    return (int(t.storage_offset()), tuple(int(x) for x in t.shape), tuple(int(x) for x in t.stride()))


def view_from(buf, recipe):
    off, size, stride = recipe
    return torch.as_strided(buf, size, stride, off)


def attn_views(q, k, v, heads, dtype, poison, batch_slice=False):
    """q [N, Sq, C], k, v [N, Skv, C] (fp32 tensors of dtype-rounded values) as column slices of ONE buffer [N, S_alloc, 3 * (C + 8)] of
    the storage dtype: columns q | 8 pad | k | 8 pad | v | 8 pad (the chunk behind the last head of every operand is padding, the chunk
    behind any other head is the next head), S_alloc = max(Sq, Skv) + 64 rows, and 64 rows' worth of elements between the samples (the
    batch stride is larger than S_alloc * ld).  Every element that is not an operand element holds the poison.  batch_slice: the buffer
    has a poisoned sample in front and one behind, the views are buf[1 : N + 1].
    Returns the three views (each a view of the flat buffer, view._base) and the mask of poisoned elements (flat, bool)."""
    N, Sq, C = q.shape
    Skv = k.shape[1]
    assert k.shape == v.shape and k.shape[0] == N and k.shape[2] == C and C % heads == 0 and (C // heads) % 8 == 0
    ld = 3 * (C + ATTN_PAD_COLS)
    s_alloc = max(Sq, Skv) + ATTN_GUARD_ROWS
    bs = (s_alloc + ATTN_GUARD_ROWS) * ld
    nb = N + (2 if batch_slice else 0)
    buf = attn_poison_fill(nb * bs, dtype, poison)
    mask = torch.ones(nb * bs, dtype=torch.bool)
    views = []
    for i, t in enumerate((q, k, v)):
        off = (bs if batch_slice else 0) + i * (C + ATTN_PAD_COLS)
        size, stride = (N, t.shape[1], C), (bs, ld, 1)
        view = torch.as_strided(buf, size, stride, off)
        view.copy_(t.to(dtype))
        torch.as_strided(mask, size, stride, off).fill_(False)
        views.append(view)
    return views[0], views[1], views[2], mask


def attn_out_guarded(N, Sq, C, dtype, device="cpu"):
    """An `out` view [N, Sq, C] with ldo = C + 8 inside a buffer that is NaN (the payload NaN) everywhere: in the 8 padding columns of every
    row, in 64 rows before the first sample, after the last and between samples.  Returns (out, check): out._base is the flat buffer;
    check(out_buf) raises unless every guard element still holds the NaN's bit pattern (compared as integers) and the view holds no NaN."""
    ldo = C + ATTN_PAD_COLS
    bso = (Sq + ATTN_GUARD_ROWS) * ldo
    numel = ATTN_GUARD_ROWS * ldo + N * bso
    recipe = (ATTN_GUARD_ROWS * ldo, (N, Sq, C), (bso, ldo, 1))
    guard = torch.ones(numel, dtype=torch.bool)
    view_from(guard, recipe).fill_(False)
    bits = ATTN_NAN_BITS[dtype]
    out = view_from(attn_poison_fill(numel, dtype, "nan").to(device), recipe)

    def check(out_buf):
        b = out_buf.detach().to("cpu").reshape(-1)
        assert b.dtype == dtype and b.numel() == numel, (b.dtype, b.numel(), numel)
        raw = b.view(torch.int16).to(torch.int32) & 0xFFFF
        hit = guard & (raw != bits)
        assert not bool(hit.any()), f"{int(hit.sum())} guard elements of `out` were overwritten, the first at flat index {int(hit.nonzero()[0])} " \
                                    f"(row {int(hit.nonzero()[0]) // ldo}, column {int(hit.nonzero()[0]) % ldo} of rows of {ldo})"
        inside = view_from(b, recipe).float()
        assert not bool(torch.isnan(inside).any()), f"{int(torch.isnan(inside).sum())} NaNs inside the `out` view (unwritten or poisoned elements)"
    return out, check


# ----------------------------------------------------------------------------------------------------------------
# the fusion block (csrc/fusion.hip): interleave + ControlNetBlock, judged per SAMPLE against fp64
# ----------------------------------------------------------------------------------------------------------------
# Layouts are the kernel's: residuals [N, HW, C] (NHWC), w1 [C, 3, 2], b1 [C, 3], g1 / be1 [HW, C, 3], w2 [C, 3], b2 [C], g2 / be2
# [HW, C], w3 / b3 [C] - what ops.pack_fusion_params makes of a ControlNetBlock's state dict (fusion_state_dict is its inverse).
FU_MAX_CHUNK = 256              # csrc/fusion.hip: partial sums per sample (workgroups of passes A and B)
FU_MAX_CB = 512                 # ... workgroups of pass C
FUSION_KINDS = ("randn",) + tuple(f"ratio_{r}" for r in REQUIRED_RATIOS + PROBE_RATIOS) + \
    ("outliers", "loud_net", "gated_off", "constant", "u_offset_10", "u_offset_30")
FUSION_DEFECTS = ("stale_column", "partials_past_64", "scale_behind_bias", "count_c_hw", "variance_unclamped", "sample_stride_dense")


def fusion_kind_required(kind) -> bool:
    return not (kind.startswith("ratio_") and int(kind[6:]) in PROBE_RATIOS)


def fusion_grids(C, HW):
    """(nchunk, cb): the workgroups per sample of passes A / B and of pass C - a Python mirror of fusion_grids() in csrc/fusion.hip"""
    ch8 = C // 8
    items = HW * ch8
    q = ch8 // math.gcd(ch8, 256)

    def pick(want, cap):
        n = (want // q) * q
        if n < q:
            n = q
        while n > cap:
            n -= q
        return n if n >= 1 else (1 if want < 1 else min(want, cap))
    return pick(items // 2048, FU_MAX_CHUNK), pick(items // 1024, FU_MAX_CB)


def fusion_fixed_column(C, nb) -> bool:
    """a thread of a pass with nb workgroups per sample keeps one 8-channel column (its parameters are loaded once)"""
    return (nb * 256) % (C // 8) == 0


def _fusion_z64(res, scales, w1, b1):
    """[N, HW, C, 3] fp64: the first grouped convolution on the scaled residuals"""
    r = [t.double() * float(s) for t, s in zip(res, scales)]
    w, b = w1.double(), b1.double()
    return torch.stack([w[:, q, 0] * r[2 * q] + w[:, q, 1] * r[2 * q + 1] + b[:, q] for q in range(3)], dim=-1)


def _fusion_u64(z, p, eps):
    N = z.shape[0]
    mean = z.reshape(N, -1).mean(dim=1).reshape(N, 1, 1, 1)
    var = z.reshape(N, -1).var(dim=1, unbiased=False).reshape(N, 1, 1, 1)
    y = F.silu((z - mean) / torch.sqrt(var + eps) * p["g1"].double() + p["be1"].double())
    return (y * p["w2"].double()).sum(dim=-1) + p["b2"].double()


def fusion_case(N, C, HW, dtype, kind="randn", scales=(1.0, 0.5, 1.0, 2.0, 1.0, 0.0), seed=0, addend=False, eps=1e-5):
    """One es_fusion_block launch, seeded: dict with `res` (six [N, HW, C] residuals, rounded to the storage dtype, fp32), `params` (the
    ten parameter tensors in the kernel's storage: w1 b1 w2 b2 w3 b3 fp32, the four affine planes rounded to `dtype`, in
    ops.pack_fusion_params' layout), `scales` (six fp32-exact host scales), `addend` ([N, HW, C] or None).  kind (FUSION_KINDS):
      randn          zero-mean residuals, small biases
      ratio_r        the fp64 LayerNorm-1 input z of EVERY sample has |mean| / std = r over its 3 C HW values (asserted, ratio_tolerance)
      outliers       1 % of the channels (at least one) at 50 .. 100 times the spread of the rest, in all six nets
      loud_net       net 3 at 2e3, the others at 1
      gated_off      all scales 0: z == b1[c, q] - a variance that is small and not 0
      constant       scales 0 and b1 == 0: variance exactly 0, the output depends on the planes alone
      u_offset_r     second_conv bias such that the fp64 LayerNorm-2 input u has |mean| / std = r (10, 30)"""
    assert kind in FUSION_KINDS and C % 8 == 0, kind
    g = _gen(seed + 32452843)
    f32 = lambda t: t.to(torch.float32)
    scales = [float(torch.tensor(s, dtype=torch.float32)) for s in scales]
    res = [torch.randn(N, HW, C, generator=g, dtype=torch.float64) for _ in range(6)]
    p = dict(w1=f32(0.7 * torch.randn(C, 3, 2, generator=g)), b1=f32(0.1 * torch.randn(C, 3, generator=g)),
             g1=rnd(1 + 0.1 * torch.randn(HW, C, 3, generator=g), dtype), be1=rnd(0.1 * torch.randn(HW, C, 3, generator=g), dtype),
             w2=f32(0.6 * torch.randn(C, 3, generator=g)), b2=f32(0.1 * torch.randn(C, generator=g)),
             g2=rnd(1 + 0.1 * torch.randn(HW, C, generator=g), dtype), be2=rnd(0.1 * torch.randn(HW, C, generator=g), dtype),
             w3=f32(torch.randn(C, generator=g)), b3=f32(0.1 * torch.randn(C, generator=g)))
    if kind == "outliers":
        gains = _outlier_gains(C, max(0.01, 1.0 / C), (50.0, 100.0), g)
        assert int((gains > 1).sum()) == max(1, int(round(0.01 * C)))
        res = [t * gains * (8.0 / 100.0) for t in res]                 # the quiet channels at 0.08, the loud ones at 4 .. 8
    if kind == "loud_net":
        res[3] = res[3] * 2.0e3
    if kind in ("gated_off", "constant"):
        scales = [0.0] * 6
    if kind == "constant":
        p["b1"] = torch.zeros(C, 3)
    res = [rnd(t, dtype) for t in res]
    if kind.startswith("ratio_"):
        ratio = int(kind[6:])
        z = _fusion_z64(res, scales, p["w1"], p["b1"]).reshape(N, -1)
        shift = ratio * float(z.std(dim=1, unbiased=False).mean()) - float(z.mean())
        p["b1"] = f32(p["b1"].double() + (shift if seed % 2 == 0 else -shift - 2 * float(z.mean())))
        r = measured_ratio(_fusion_z64(res, scales, p["w1"], p["b1"]).reshape(N, -1))
        tol = ratio_tolerance(ratio, dtype)
        if ratio == 0:
            assert float(r.max()) < 0.05, float(r.max())
        else:
            assert float(r.min()) >= ratio * (1 - tol) and float(r.max()) <= ratio * (1 + tol), (ratio, float(r.min()), float(r.max()))
    if kind.startswith("u_offset_"):
        ratio = int(kind[9:])
        u = _fusion_u64(_fusion_z64(res, scales, p["w1"], p["b1"]), p, eps).reshape(N, -1)
        p["b2"] = f32(p["b2"].double() + ratio * float(u.std(dim=1, unbiased=False).mean()) - float(u.mean()))
        r = measured_ratio(_fusion_u64(_fusion_z64(res, scales, p["w1"], p["b1"]), p, eps).reshape(N, -1))
        assert float(r.min()) >= ratio * 0.9 and float(r.max()) <= ratio * 1.1, (ratio, float(r.min()), float(r.max()))
    c = dict(N=N, C=C, HW=HW, dtype=dtype, kind=kind, eps=eps, res=res, params=p, scales=scales,
             addend=rnd(torch.randn(N, HW, C, generator=g), dtype) if addend else None)
    z = _fusion_z64(res, scales, p["w1"], p["b1"]).reshape(N, -1)
    var = z.var(dim=1, unbiased=False)
    if kind == "gated_off":
        assert torch.equal(z.reshape(N, HW, C, 3)[0, 0], p["b1"].double()) and 0 < float(var.max()) < 0.1
    if kind == "constant":
        assert float(z.abs().max()) == 0.0
    if kind == "loud_net":
        assert 5.0e2 < float(res[3].pow(2).mean().sqrt()) < 8.0e3 and float(res[2].pow(2).mean().sqrt()) < 4.0     # (8 values at the smallest shape)
    if kind == "outliers":
        rms = res[0].double().pow(2).mean(dim=(0, 1)).sqrt()
        assert float(rms.max()) >= 30.0 * float(rms.median()) or C < 100
    assert all(bool(torch.isfinite(t).all()) and torch.equal(t, rnd(t, dtype)) for t in res)
    assert all(torch.equal(p[k], rnd(p[k], dtype)) for k in ("g1", "be1", "g2", "be2"))
    return c


def fusion_state_dict(c, prefix, H, W):
    """the ControlNetBlock state dict (fp64) that ops.pack_fusion_params packs into c["params"]"""
    p, C = {k: v.double() for k, v in c["params"].items()}, c["C"]
    assert H * W == c["HW"]
    return {f"{prefix}.first_conv.weight": p["w1"].reshape(3 * C, 2, 1, 1), f"{prefix}.first_conv.bias": p["b1"].reshape(3 * C),
            f"{prefix}.first_normalization.weight": p["g1"].permute(1, 2, 0).reshape(3 * C, H, W),
            f"{prefix}.first_normalization.bias": p["be1"].permute(1, 2, 0).reshape(3 * C, H, W),
            f"{prefix}.second_conv.weight": p["w2"].reshape(C, 3, 1, 1), f"{prefix}.second_conv.bias": p["b2"],
            f"{prefix}.second_normalization.weight": p["g2"].permute(1, 0).reshape(C, H, W),
            f"{prefix}.second_normalization.bias": p["be2"].permute(1, 0).reshape(C, H, W),
            f"{prefix}.third_conv.weight": p["w3"].reshape(C, 1, 1, 1), f"{prefix}.third_conv.bias": p["b3"]}


def _fusion_scales(c, scales_dev=None):
    """the six effective scales: host scale x device scale (both fp32 values; their product is taken exactly)"""
    return [s * (1.0 if scales_dev is None else float(scales_dev[i])) for i, s in enumerate(c["scales"])]


def fusion_ref64(c, scales_dev=None):
    """the plain operation in fp64, [N, HW, C]: interleave, three grouped 1x1 convolutions, two LayerNorms over the whole sample with
    affine planes, SiLU (+ the addend)"""
    p, N, eps = c["params"], c["N"], c["eps"]
    u = _fusion_u64(_fusion_z64(c["res"], _fusion_scales(c, scales_dev), p["w1"], p["b1"]), p, eps)
    mean = u.reshape(N, -1).mean(dim=1).reshape(N, 1, 1)
    var = u.reshape(N, -1).var(dim=1, unbiased=False).reshape(N, 1, 1)
    v = F.silu((u - mean) / torch.sqrt(var + eps) * p["g2"].double() + p["be2"].double())
    out = v * p["w3"].double() + p["b3"].double()
    return out if c["addend"] is None else out + c["addend"].double()


def fusion_base_ref(c, scales_dev=None):
    """the textbook fp32 sequence with every op's output rounded to the storage dtype: scaled residuals | first_conv | LayerNorm
    (two-pass) | SiLU | second_conv | LayerNorm | SiLU | third_conv | + addend"""
    p, N, eps, dt = c["params"], c["N"], c["eps"], c["dtype"]
    sc = _fusion_scales(c, scales_dev)
    r = [rnd(t * torch.tensor(s, dtype=torch.float32), dt) for t, s in zip(c["res"], sc)]
    z = rnd(torch.stack([p["w1"][:, q, 0] * r[2 * q] + p["w1"][:, q, 1] * r[2 * q + 1] + p["b1"][:, q] for q in range(3)], dim=-1), dt)

    def ln(t, gam, bet):
        flat = t.reshape(N, -1)
        mean = flat.mean(dim=1).reshape([N] + [1] * (t.dim() - 1))
        var = ((t - mean) ** 2).reshape(N, -1).mean(dim=1).reshape(mean.shape)
        return rnd((t - mean) * torch.rsqrt(var + eps) * gam + bet, dt)
    y = rnd(F.silu(ln(z, p["g1"], p["be1"])), dt)
    u = rnd((y * p["w2"]).sum(dim=-1) + p["b2"], dt)
    v = rnd(F.silu(ln(u, p["g2"], p["be2"])), dt)
    out = rnd(v * p["w3"] + p["b3"], dt)
    return out if c["addend"] is None else rnd(out + c["addend"], dt)


def _wave_tree(t):
    """wave_sum of common.h over the last dimension (64 lanes): neighbours first, then quads, eights, ... - every level rounded to fp32"""
    while t.shape[-1] > 1:
        t = t.reshape(*t.shape[:-1], t.shape[-1] // 2, 2)
        t = t[..., 0] + t[..., 1]
    return t[..., 0]


def fusion_sums(v, nb, drop_from=None):
    """fp32 (sum, sum of squares) per sample of v [N, items, k] as csrc/fusion.hip forms them with nb workgroups per sample, in three
    levels: a thread's chain over its items (stride nb * 256) and the k values of each in order (s += v; ss = fma(v, v, ss)), the
    workgroup (wave_sum, then the four waves in order), the nb partials (reduce_partials: lane l chains partials l, l + 64, ..., then
    wave_sum).  drop_from (a planted defect): the partials from that index on are never read."""
    N, items, k = v.shape
    stride = nb * 256
    J = (items + stride - 1) // stride
    if J * stride != items:
        v = torch.cat([v, torch.zeros(N, J * stride - items, k)], dim=1)
    v = v.float().reshape(N, J, stride, k)
    s, ss = torch.zeros(N, stride), torch.zeros(N, stride)
    for j in range(J):
        for e in range(k):
            t = v[:, j, :, e]
            s = s + t
            ss = (ss.double() + t.double() * t.double()).float()
    out = []
    for t in (s, ss):
        w = _wave_tree(t.reshape(N, nb, 4, 64))
        part = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]                                # [N, nb]
        if drop_from is not None:
            part = part[:, :drop_from]
        lanes = torch.cat([part, torch.zeros(N, 256 - part.shape[1])], dim=1).reshape(N, 4, 64)
        acc = lanes[:, 0]
        for j in range(1, 4):
            acc = acc + lanes[:, j]
        out.append(_wave_tree(acc))
    return out[0], out[1]


def _fusion_stats(v, nb, cnt, eps, defect):
    s, ss = fusion_sums(v, nb, drop_from=64 if defect == "partials_past_64" else None)
    cnt = torch.tensor(float(cnt), dtype=torch.float32)
    mean = s / cnt
    var = ((ss / cnt).double() - mean.double() * mean.double()).float()                         # fma(-mean, mean, ss / cnt)
    if defect != "variance_unclamped":
        var = var.clamp_min(0.0)
    return mean, torch.rsqrt(var + eps)


def _fusion_columns(t, C, items, nb, stale):
    """the per-channel parameter t [C, ...] as every 8-channel item sees it, [HW, C, ...]: its own column, or (stale) the column of
    the FIRST item of the thread that handles it with nb workgroups per sample"""
    ch8 = C // 8
    i = torch.arange(items)
    col = ((i % (nb * 256)) % ch8) if stale else (i % ch8)
    ch = (col[:, None] * 8 + torch.arange(8)[None, :]).reshape(items // ch8, C)
    return t[ch]


def fusion_base_alg(c, nchunk=None, cb=None, defect=None, scales_dev=None, layout=None, want_u=False):
    """csrc/fusion.hip as designed, in fp32 on the CPU: r * (scale * scale_dev) first; z = w1[0] r0 + w1[1] r1 + b1; one-pass sums in
    the kernel's three levels (fusion_sums: a thread's items at stride nchunk * 256, its 24 values in (q, e) order); mean = s / cnt,
    var = ss / cnt - mean^2 clamped at 0; u = b2 + sum_q w2 y_q rounded to the storage dtype; the statistics of the ROUNDED u;
    w3 v + b3 rounded; with an addend a second rounding.  nchunk, cb: the grids (default: fusion_grids).
    layout: [(flat buffer, offset, batch stride)] x 6 - where the residuals sit in memory (for "sample_stride_dense").
    Planted defects (FUSION_DEFECTS):
      stale_column        a thread keeps the parameter column of its first item (wrong wherever nb * 256 is no multiple of C / 8)
      partials_past_64    reduce_partials reads the first 64 partial sums only
      scale_behind_bias   the second net's scale of every pair multiplies w r + b1 instead of r
      count_c_hw          LayerNorm 1 divides by C HW instead of 3 C HW
      variance_unclamped  a negative one-pass variance is not clamped
      sample_stride_dense sample n of every net is read at n HW C instead of n * res_bs"""
    assert defect is None or defect in FUSION_DEFECTS, defect
    p, N, C, HW, eps, dt = c["params"], c["N"], c["C"], c["HW"], c["eps"], c["dtype"]
    g_n, g_c = fusion_grids(C, HW)
    nchunk, cb = nchunk or g_n, cb or g_c
    items = HW * (C // 8)
    stale = defect == "stale_column"
    res = c["res"]
    if defect == "sample_stride_dense":
        assert layout is not None
        res = [torch.stack([buf[off + n * HW * C: off + (n + 1) * HW * C] for n in range(N)]).reshape(N, HW, C).float() for buf, off, _ in layout]
    sc = [torch.tensor(a, dtype=torch.float32) * (torch.tensor(1.0) if scales_dev is None else scales_dev[i].float())
          for i, a in enumerate(c["scales"])]
    col = lambda t, nb: _fusion_columns(t, C, items, nb, True) if stale else t
    w1, b1, w2, b2 = (col(p[k], nchunk) for k in ("w1", "b1", "w2", "b2"))
    zs = []
    for q in range(3):
        if defect == "scale_behind_bias":
            zs.append(w1[..., q, 0] * (res[2 * q] * sc[2 * q]) + (w1[..., q, 1] * res[2 * q + 1] + b1[..., q]) * sc[2 * q + 1])
        else:
            zs.append(w1[..., q, 0] * (res[2 * q] * sc[2 * q]) + w1[..., q, 1] * (res[2 * q + 1] * sc[2 * q + 1]) + b1[..., q])
    z = torch.stack(zs, dim=-1)                                                                 # [N, HW, C, 3]
    order = z.reshape(N, items, 8, 3).transpose(2, 3).reshape(N, items, 24)                     # a thread's (q, e) order
    mean1, rstd1 = _fusion_stats(order, nchunk, (1 if defect == "count_c_hw" else 3) * C * HW, eps, defect)
    y = F.silu((z - mean1.reshape(N, 1, 1, 1)) * rstd1.reshape(N, 1, 1, 1) * p["g1"] + p["be1"])
    u = b2 + w2[..., 0] * y[..., 0]
    u = u + w2[..., 1] * y[..., 1]
    u = rnd(u + w2[..., 2] * y[..., 2], dt)
    if want_u:
        return u
    mean2, rstd2 = _fusion_stats(u.reshape(N, items, 8), nchunk, C * HW, eps, defect)
    v = F.silu((u - mean2.reshape(N, 1, 1)) * rstd2.reshape(N, 1, 1) * p["g2"] + p["be2"])
    out = rnd(col(p["w3"], cb) * v + col(p["b3"], cb), dt)
    return out if c["addend"] is None else rnd(out + c["addend"], dt)


def fusion_layout(c, seed=0, dense=False):
    """Where a launch's residuals sit in memory: six (flat NaN-padded fp32 buffer, offset, batch stride) - nets 1, 3 and 5 are the three
    thirds of ONE dense [3 N, HW, C] buffer (the batched openpose pass), nets 0, 2 and 4 have buffers of their own with batch strides
    of HW C + 8, + 24 and + 64 elements (NaN in the gaps, 16-byte alignment kept) behind a NaN prefix.  dense: all strides HW C."""
    N, per = c["N"], c["HW"] * c["C"]
    nan = float("nan")
    pose = torch.full((3 * N * per + 16,), nan)
    out = [None] * 6
    for j, k in enumerate((1, 3, 5)):
        pose[8 + j * N * per: 8 + (j + 1) * N * per] = c["res"][k].reshape(-1)
        out[k] = (pose, 8 + j * N * per, per)
    for j, k in enumerate((0, 2, 4)):
        bs = per if dense else per + (8, 24, 64)[j]
        off = 8 * (j + 1)
        buf = torch.full((off + N * bs + 8,), nan)
        for n in range(N):
            buf[off + n * bs: off + n * bs + per] = c["res"][k][n].reshape(-1)
        out[k] = (buf, off, bs)
    return out


def nearly_constant_fusion_case(N, C, HW, dtype, seed=0):
    """`gated_off` with b1 = 100 +- 1e-3: every sample's z is constant up to 1e-5 of its value, so the noise of the one-pass
    E[z^2] - mean^2 (about 1e-3) exceeds both the true variance (1e-6) and eps, and its sign is a matter of summation order.  No error
    bar can hold here (the design's own result is noise); what must hold is that the output is finite: the clamp at 0."""
    c = fusion_case(N, C, HW, dtype, "gated_off", seed=seed)
    c["params"]["b1"] = (100.0 + 1e-3 * torch.randn(C, 3, generator=_gen(seed + 1), dtype=torch.float64)).float()
    c["kind"] = "nearly_constant"
    return c


def sample_err(y, ref64, both=False):
    """row_err with one SAMPLE as the row: a LayerNorm over the whole sample gives the sample one scale"""
    N = ref64.shape[0]
    return row_err(y.reshape(N, -1), ref64.reshape(N, -1), both=both)


# ----------------------------------------------------------------------------------------------------------------
# the sampler step (es_cfg_unipc_step, es_cfg_ddim_step): a linear recombination with a host-made fp32 coefficient table
# ----------------------------------------------------------------------------------------------------------------
def traj_err(x, ref64) -> float:
    """max|x - ref| / rms(ref) over the whole latent tensor; inf where x is not finite"""
    r, v = ref64.detach().double().cpu(), x.detach().double().cpu()
    if not bool(torch.isfinite(v).all()):
        return float("inf")
    return float((v - r).abs().max() / r.pow(2).mean().sqrt())


def guided_eps(noise, B, gs, cfg, t):
    """the guided noise of the step kernels in t's precision: eu + gs * (ec - eu) over the two halves of noise [2 B | B, ...]"""
    n = noise.to(t)
    if not cfg:
        return n
    return n[:B] + torch.tensor(gs, dtype=t) * (n[B:] - n[:B])


def unipc_apply(row, eps, x, last, m0, m1):
    """one es_cfg_unipc_step in the precision of x (fp64: the truth for a given table; fp32: base_alg), row = the 12 coefficients of
    the step.  Returns (next x, last = corrected sample, m0 = x0, m1 = previous x0)."""
    c = row.to(x.dtype)
    x0 = (x - c[1] * eps) / c[0]
    xc = (c[3] * last + c[4] * m0 + c[5] * m1 + c[6] * x0) if float(c[2]) != 0.0 else x
    return c[7] * xc + c[8] * x0 + c[9] * m0, xc, x0, m0


def ddim_apply(row, eps, x):
    c = row.to(x.dtype)
    x0 = (x - c[1] * eps) / c[0]
    return c[2] * x0 + c[3] * eps


def unipc_oracle_step64(s, eps, x):
    """oracle.UniPC.step without its closing cast to fp32: the trajectory stays in fp64 from end to end"""
    a_t, s_t = s._alpha_sigma(s.sigmas[s.step_index])
    x0 = (x.double() - s_t * eps.double()) / a_t
    sample = x.double()
    if s.step_index > 0 and s.last_sample is not None:
        sample = s._uni_c(x0, s.last_sample, s.this_order)
    s.model_outputs = s.model_outputs[1:] + [x0]
    s.this_order = min(min(s.solver_order, len(s.timesteps) - s.step_index), s.lower_order_nums + 1)
    s.last_sample = sample
    prev = s._uni_p(sample, s.this_order)
    if s.lower_order_nums < s.solver_order:
        s.lower_order_nums += 1
    s.step_index += 1
    return prev


def sampler_eps(T, shape, dtype, seed=0):
    """T model outputs [2 B | B, H, W, L] rounded to the storage dtype, and the fp32 start latents"""
    g = _gen(seed + 49979687)
    return [rnd(torch.randn(*shape, generator=g), dtype) for _ in range(T)]


def run_trajectory(kind, table, eps_list, x0, B, gs, cfg, prec):
    """the whole trajectory through unipc_apply / ddim_apply in precision `prec`; returns the list of per-step states
    (x, last, m0, m1) - DDIM: (x,)"""
    x = x0.to(prec)
    last, m0, m1 = (torch.zeros_like(x) for _ in range(3))
    out = []
    for i, noise in enumerate(eps_list):
        e = guided_eps(noise, B, gs, cfg, prec)
        if kind == "unipc":
            x, last, m0, m1 = unipc_apply(table[i], e, x, last, m0, m1)
            out.append((x, last, m0, m1))
        else:
            x = ddim_apply(table[i], e, x)
            out.append((x,))
    return out


def sinusoid64(t, dim):
    """the timestep embedding in fp64: [cos | sin] of t * exp(-ln(1e4) k / half)"""
    half = dim // 2
    a = t.double()[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)[None]
    return torch.cat([torch.cos(a), torch.sin(a)], dim=-1)


def sinusoid32(t, dim, dtype):
    """... as torch computes it in fp32, rounded once: the baseline of the kernel's misrounded count"""
    half = dim // 2
    a = t.float()[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)[None]
    return rnd(torch.cat([torch.cos(a), torch.sin(a)], dim=-1), dtype)


def vae_sample_ref(mom, noise, L, scaling, prec, dtype=None):
    """(mean + exp(0.5 clamp(logvar, -30, 20)) noise) scaling for NHWC moments [N, H, W, 2 L] and NCHW noise, in `prec`; dtype: every
    op's output rounded to it (base_ref)"""
    r = (lambda v: rnd(v, dtype)) if dtype is not None else (lambda v: v)
    m = mom.to(prec)
    mean, logvar = m[..., :L], m[..., L:2 * L].clamp(-30.0, 20.0)
    std = r(torch.exp(r(0.5 * logvar)))
    return r(r(mean + r(std * noise.to(prec).permute(0, 2, 3, 1))) * scaling)


# ----------------------------------------------------------------------------------------------------------------
# es_linear_xs (csrc/linear_xs.hip): every form, stage count and ragged edge (tests/test_linear_xs_gpu.py)
# ----------------------------------------------------------------------------------------------------------------
XS_KINDS = ("plain", "ln", "geglu", "geglu_ln", "res", "gn")
# (K, kind, ping-pong): the 16 instantiations per dtype that launch() of csrc/linear_xs.hip can pick
XS_FORMS = tuple([(320, k, 0) for k in ("plain", "ln", "geglu", "geglu_ln", "res")] + [(640, k, 0) for k in ("plain", "ln", "geglu", "geglu_ln")] +
                 [(320, k, 1) for k in ("plain", "ln", "res", "gn")] + [(640, k, 1) for k in ("plain", "ln", "gn")])
XS_FORM_GEGLU, XS_FORM_LN, XS_FORM_RES, XS_FORM_PP, XS_FORM_GN = 0x100, 0x200, 0x400, 0x800, 0x1000      # include/edgestyle_hip.h
XS_ROWS = 256                   # rows per workgroup
XS_GUARD_ROWS = 256             # NaN rows in front of and behind a guarded output
XS_PAD_COLS = 64                # NaN columns behind every row of one
XS_DEFECTS = ("stale_stage", "row_dropped", "short_slice_line_dropped", "residual_row_shift", "geglu_halves_swapped", "ln_zero_row_nan")


def xs_form_id(K, kind, pp) -> int:
    """es_linear_xs_last_form of the instantiation (K, kind, pp)"""
    return K // 32 | (XS_FORM_GEGLU if kind.startswith("geglu") else 0) | (XS_FORM_LN if kind in ("ln", "geglu_ln") else 0) | \
        (XS_FORM_RES if kind == "res" else 0) | (XS_FORM_PP if pp else 0) | (XS_FORM_GN if kind == "gn" else 0)


XS_ROUTE_KEYS = ("form", "grid", "threads", "lds", "runs", "rows_per_run")
XS_LDS = 3 * (40960 + 256) + 8 * 32 * 144        # csrc/linear_xs.hip: three 40 KB weight stages (+ 64 fp32 bias values each), eight 32-row output tiles


def xs_route(d, pp=1, limit=0x7FFFFFFF):
    """Python mirror of xs_route() in csrc/linear_xs.hip for a descriptor es_linear_xs accepts (any object with es_xs_desc's fields), keyed
    like lib.XS_ROUTE_FIELDS.  The form is what the descriptor's epilogue is called in XS_KINDS; the ping-pong form runs everything without
    GEGLU when the knob is on and GroupNorm-in-front always."""
    cdiv = lambda a, b: (a + b - 1) // b
    kind = "gn" if d.gn_part else "res" if d.residual else ("geglu" if d.geglu else "") + ("_ln" if d.geglu and d.ln else "ln" if d.ln else "") or "plain"
    form = xs_form_id(d.K, kind, kind == "gn" or (pp != 0 and not d.geglu))
    M, runs, rows = d.M, 1, d.M
    if d.M * d.K * 2 >= limit or (d.M + 256) * d.ldo * 2 >= limit:
        # whole 256-row blocks (whole samples with GroupNorm in front) that leave one block of slack below the limit; never less than one block
        row_bytes = max(d.K, d.ldo) * 2
        rows = max(256, ((limit - 1) // row_bytes - 256) // 256 * 256 if limit > 512 * row_bytes else 256)
        if d.gn_part:
            rows -= rows % d.gn_hw
        ends = [d.mt_end[g] * 128 for g in range(d.ngroups - 1)] + [d.M] if d.ngroups > 1 else [d.M]
        runs = sum(cdiv(e - s, rows) for s, e in zip([0] + ends, ends))
        M = min(rows, ends[0])
    return dict(form=form, grid=cdiv(M, XS_ROWS) * d.nslices, threads=512, lds=XS_LDS, runs=runs, rows_per_run=rows)


def xs_geometry(K, kind):
    """(GEMM columns per stage, stored columns per stage, stages per 128-byte output line) of csrc/linear_xs.hip"""
    ch = 64 if K == 320 else 32
    outw = ch // 2 if kind.startswith("geglu") else ch
    return ch, outw, 64 // outw


def xs_split(lines, slices, P):
    """ops.linear_xs's cut of `lines` output lines into at most `slices` slices: (nslices, chunks_per_slice, stages of the last slice)"""
    want = max(1, min(lines, slices))
    lps = -(-lines // want)
    nslices = -(-lines // lps)
    return nslices, lps * P, (lines - (nslices - 1) * lps) * P


def _xs_clear_ties(final_bias, b, dtype):
    """moves entries of b (by 2^-13 of the value: a quarter of an fp16 step or less) until no entry of final_bias() - the value a zero row stores - lies within NORM_TIE_CLEARANCE
    of a rounding boundary of the storage dtype (or below its normal range), as norm_case does for SiLU(beta)"""
    for _ in range(16):
        fb = final_bias().double()
        small = fb.abs() < 2.0 ** -14
        close = small.clone()
        close[~small] = tie_distance(fb[~small], dtype) < NORM_TIE_CLEARANCE
        if not bool(close.any()):
            return
        b[close] += torch.where(small, torch.full_like(fb, 2.0 ** -12), fb.abs() * 2.0 ** -13)[close].float()
    raise AssertionError("a bias stayed on a rounding boundary")


def xs_case(M, K, lines, kind, dtype, seed=0, counts=None, ratio=0, hw=None, G=None, N=None, loud=16.0):
    """One es_linear_xs launch: M rows of K = 320 | 640 channels -> `lines` 128-byte output lines (64 stored columns each; GEGLU kinds: twice
    as many GEMM columns).  kind: XS_KINDS.  counts: a grouped launch - rows per weight set (kind "gn": SAMPLES per set), the second
    set's weights and bias `loud` times the others' (a row that took its neighbour's weights is then wrong by that factor).
    Inputs, seeded and rounded through the storage dtype: token_rows at |mean| / std = `ratio` for the LayerNorm kinds, group_maps [N, hw, 1, K]
    with G groups at that ratio for "gn" (M == N * hw), randn for the others (the output of an attention or a feed-forward layer, the
    residual of the same size).  Weights: ln_case's per set (gamma / beta used by the LayerNorm kinds only), gn_case's for "gn"; every bias is
    kept clear of the storage dtype's rounding boundaries."""
    assert kind in XS_KINDS and K in (320, 640) and (kind != "res" or K == 320)
    geglu = kind.startswith("geglu")
    cstore = 64 * lines
    Cout = 2 * cstore if geglu else cstore
    c = dict(M=M, K=K, lines=lines, kind=kind, dtype=dtype, cstore=cstore, counts=list(counts) if counts else None)
    if kind == "gn":
        assert M == N * hw and (counts is None or sum(counts) == N)
        x = group_maps(N, K, hw, G, ratio, dtype=dtype, seed=seed, W=1)
        g = gn_case(x, G, dtype, eps=1e-6, seed=seed, Cout=Cout, ngroups=len(counts) if counts else 1)
        for i in range(len(g["W"])):
            if i == 1:
                g["W"][i], g["b"][i] = g["W"][i] * loud, g["b"][i] * loud
            _xs_clear_ties(lambda: g["b"][i], g["b"][i], dtype)
        c.update(gn=g, hw=hw, G=G, N=N, x=x.reshape(M, K))
        return c
    assert counts is None or sum(counts) == M
    if kind in ("ln", "geglu_ln"):
        x = token_rows(M, K, ratio, dtype=dtype, seed=seed)
    else:
        x = rnd(torch.randn(M, K, generator=_gen(seed), dtype=torch.float64), dtype)
    res = rnd(torch.randn(M, cstore, generator=_gen(seed + 31), dtype=torch.float64), dtype) if kind == "res" else None
    sets, a = [], 0
    for i, n in enumerate(counts or [M]):
        q = ln_case(x[a:a + n], Cout, dtype, geglu=geglu, bias=True, seed=seed + 13 * i)
        q["ln"] = kind in ("ln", "geglu_ln")
        q["res"] = None if res is None else res[a:a + n]
        if i == 1:
            q["W"], q["b"] = q["W"] * loud, q["b"] * loud
        _xs_clear_ties((lambda: fold_weights(q)[2]) if q["ln"] else (lambda: q["b"]), q["b"], dtype)
        sets.append(q)
        a += n
    c.update(sets=sets, x=x, res=res)
    return c


def xs_ref64(c):
    """the plain operation in fp64 on the rounded inputs and the UNFOLDED rounded weights"""
    if c["kind"] == "gn":
        return gn_ref64(c["gn"], c["counts"]).reshape(c["M"], -1)
    return torch.cat([ln_ref64(q) for q in c["sets"]], 0)


def xs_base_ref(c):
    """the per-op-rounded fp32 sequence (ln_base_ref / gn_base_ref)"""
    if c["kind"] == "gn":
        return gn_base_ref(c["gn"], c["counts"]).reshape(c["M"], -1)
    return torch.cat([ln_base_ref(q) for q in c["sets"]], 0)


def _xs_stale(W, b, c, stage):
    """W, b with the rows of `stage` replaced by those of the stage three earlier (the LDS ring has three slots: a stage's slot last held
    stage - 3).  Stages are runs of stored columns; a GEGLU stage holds its hidden AND its gate rows."""
    ch, outw, _ = xs_geometry(c["K"], c["kind"])
    assert stage >= 3 and (stage + 1) * outw <= c["cstore"]
    W, b = W.clone(), b.clone()
    for off in ((0, c["cstore"]) if c["kind"].startswith("geglu") else (0,)):
        d0, s0 = off + stage * outw, off + (stage - 3) * outw
        W[d0:d0 + outw], b[d0:d0 + outw] = W[s0:s0 + outw].clone(), b[s0:s0 + outw].clone()
    return W, b


def xs_base_alg(c, chain=8, defect=None, stage=3):
    """The launch as designed (ln_base_alg form "xs" / gn_base_alg with a chain): LayerNorm or GroupNorm rounded to the storage dtype in
    registers, every output one fp32 chain over K that starts from the bias, `chain`-wide partial dot products, GEGLU in fp32 with one
    rounding, the residual kinds round, + residual, round.  chain None: torch's fp32 matmul and a separate bias add (a third, independent
    reading for the misrounded bar).  Planted defects (XS_DEFECTS):
      "stale_stage"               the output columns of `stage` computed with the weights and bias of the stage three earlier - what a counted
                                  wait one group too loose lets the MFMAs read
      "row_dropped"               row M - 1 never stored (NaN, as a sentinel-filled output shows it)
      "short_slice_line_dropped"  the last 128-byte line - the last line of the last, short slice - never stored
      "residual_row_shift"        the residual read one 16-row fragment off
      "geglu_halves_swapped"      gate * gelu(hidden)
      "ln_zero_row_nan"           an arithmetic NaN stored into row M (returned as an extra row): an out-of-range row's statistics leaking out"""
    assert defect is None or defect in XS_DEFECTS
    inner = defect if defect in ("residual_row_shift", "geglu_halves_swapped") else None
    if c["kind"] == "gn":
        g = c["gn"]
        if defect == "stale_stage":
            Wb = [_xs_stale(W, b, c, stage) for W, b in zip(g["W"], g["b"])]
            g = dict(g, W=[w for w, _ in Wb], b=[b for _, b in Wb])
        y = gn_base_alg(g, c["counts"], chain=chain).reshape(c["M"], -1)
    else:
        outs = []
        for q in c["sets"]:
            if defect == "stale_stage":
                W, b = _xs_stale(q["W"], q["b"], c, stage)
                q = dict(q, W=W, b=b)
            outs.append(ln_base_alg(q, "xs", defect=inner, chain=chain))
        y = torch.cat(outs, 0)
    if defect == "row_dropped":
        y[-1] = float("nan")
    if defect == "short_slice_line_dropped":
        y[:, -64:] = float("nan")
    if defect == "ln_zero_row_nan":
        y = torch.cat([y, torch.full((1, y.shape[1]), float("nan"))], 0)
    return y


# ---- the counted waits of csrc/linear_xs.hip: a walk of one wave's vector-memory queue (tests/test_numerics_cpu.py) ----
# ASSUMPTION (the kernel's own, not checked here): s_waitcnt vmcnt(N) returns when all but the N YOUNGEST vector-memory operations of the
# wave - loads, LDS-DMA loads and stores alike - have completed, i.e. they retire in issue order.
XS_NDMA, XS_ST, XS_RS = 6, 4, 4         # VMEM operations per wave: per weight stage, per finished 128-byte line, residual loads per stage
# every wait_vm<...> of the source in source order: (site, template argument as written)
XS_WAIT_SITES = (
    ("top_last", "0"), ("top_first", "NDMA"), ("top_p1", "NDMA + 8 + (RES ? 4 : 0)"), ("top_p2", "NDMA + 4"), ("top_p4_store", "NDMA + 4"),
    ("top_p4", "NDMA"),
    ("res_early", "NDMA"), ("res_early_end", "0"), ("res_late", "NDMA + 4 + 4 + NDMA"), ("res_late_end", "0"),
    ("pp_open", "NDMA"), ("pp_open_one", "0"),
    ("pp_late_first", "RS"), ("pp_late_store", "ST + RS"), ("pp_late", "RS"),
    ("pp_early_store", "NDMA + ST"), ("pp_early", "NDMA"), ("pp_early_end_store", "ST"), ("pp_early_end", "0"))


def xs_wait_count(site, res):
    env = dict(NDMA=XS_NDMA, ST=XS_ST, RS=XS_RS if res else 0)
    expr = dict(XS_WAIT_SITES)[site].replace("(RES ? 4 : 0)", "4" if res else "0")
    return eval(expr, {"__builtins__": {}}, env)


def xs_wave_walk(pp, late, P, res, nch, loosen=None):
    """One wave's program (the order of csrc/linear_xs.hip; one-barrier form: pp False) as a walk of its VMEM queue.  Returns
    dict(barriers, arrive: per barrier the stages whose own DMAs were still in flight when the wave ARRIVED at it, compute: stage ->
    barriers passed when its MFMAs run, issue: stage -> barriers passed when its DMAs are issued, problems: residual loads still in flight
    in the epilogue that adds them).  loosen: {site: extra operations} added to that wait's count (the planted defects)."""
    loosen = loosen or {}
    q, out = [], dict(barriers=0, arrive=[], compute={}, issue={}, problems=[])

    def wait(site):
        n = xs_wait_count(site, res) + loosen.get(site, 0)
        del q[:max(0, len(q) - n)]

    def barrier():
        out["arrive"].append(sorted({s for kind, s in q if kind == "dma"}))
        out["barriers"] += 1

    def issue(s):
        out["issue"][s] = out["barriers"]
        q.extend([("dma", s)] * XS_NDMA)

    def load_res(s):
        if res:
            q.extend([("res", s)] * XS_RS)

    def compute(s):
        out["compute"][s] = out["barriers"]

    def line_done(t):
        return t >= 0 and t % P == P - 1

    def stores(s):
        if line_done(s):
            q.extend([("st", s)] * XS_ST)

    def used(s):
        if any(kind == "res" and st == s for kind, st in q):
            out["problems"].append(f"residual of stage {s} still in flight in its epilogue")

    q.extend([("x", 0)] * 20)                           # the activation loads (their number does not matter: they are the oldest)
    if nch > 0:
        issue(0)
    if nch > 1:
        issue(1)
    if pp:
        wait("pp_open" if nch > 1 else "pp_open_one")
        if late:
            barrier()
        for t in range(nch):
            barrier()
            load_res(t)
            compute(t)
            if late and t + 1 < nch:
                wait("pp_late_first" if (t + 2 >= nch and t == 0) else "pp_late_store" if line_done(t - 1) else "pp_late")
            if not late or t + 1 < nch:
                barrier()
            if t + 2 < nch:
                issue(t + 2)
            if res:
                wait("res_early" if t + 2 < nch else "res_early_end")
                used(t)
            stores(t)
            if not late and t + 1 < nch:
                if t + 2 < nch:
                    wait("pp_early_store" if line_done(t) else "pp_early")
                else:
                    wait("pp_early_end_store" if line_done(t) else "pp_early_end")
        return out

    def top(ci):
        cio = ci - (1 if late else 0)
        if ci + 1 >= nch:
            wait("top_last")
        elif ci < (3 if late else 2):
            wait("top_first")
        elif P == 1:
            wait("top_p1")
        elif P == 2:
            wait("top_p2")
        else:
            wait("top_p4_store" if (cio & 3) < 2 else "top_p4")
        barrier()
        load_res(ci)
        if ci + 2 < nch:
            issue(ci + 2)

    def epilogue(ci):
        if res:
            if not late:
                wait("res_early" if ci + 2 < nch else "res_early_end")
            else:
                wait("res_late" if (ci >= 1 and ci + 3 < nch) else "res_late_end")
            used(ci)
        stores(ci)

    for ci in range(nch):                               # (the late waves' loop is unrolled by two in the source: the same order, two register sets)
        top(ci)
        if late and ci > 0:
            epilogue(ci - 1)
        compute(ci)
        if not late:
            epilogue(ci)
    if late and nch > 0:
        epilogue(nch - 1)
    return out


def xs_wait_audit(pp, P, res, nch, loosen=None, late_only=None):
    """The walks of an early and a late wave held against each other: the problems found (empty: the counts are safe).
      * when a wave ARRIVES at the barrier that opens compute(s) for any wave, its own DMAs of stage s are retired;
      * every residual load is retired in the epilogue that adds it;
      * both groups pass the same number of barriers;
      * the DMAs of stage s (s >= 3) are issued after the barrier that follows the last compute(s - 3) of either group (the ring slot's
        last readers).
    late_only: apply `loosen` to the late (True) / early (False) wave alone; None: to both."""
    w = {late: xs_wave_walk(pp, late, P, res, nch, loosen if late_only in (None, late) else None) for late in (False, True)}
    bad = [f"{'late' if late else 'early'}: {p}" for late in w for p in w[late]["problems"]]
    if w[False]["barriers"] != w[True]["barriers"]:
        bad.append(f"barriers: early {w[False]['barriers']}, late {w[True]['barriers']}")
    for who in w:
        for s, passed in w[who]["compute"].items():
            b = passed - 1                              # the barrier that opened this compute
            for other in w:
                if b < len(w[other]["arrive"]) and s in w[other]["arrive"][b]:
                    bad.append(f"{'late' if other else 'early'} wave reaches barrier {b} (opens compute({s}) of the {'late' if who else 'early'} "
                               f"waves) with its DMAs of stage {s} in flight")
    for who in w:
        for s, passed in w[who]["issue"].items():
            for other in w:
                if s >= 3 and passed < w[other]["compute"][s - 3] + 1:
                    bad.append(f"{'late' if who else 'early'} wave issues stage {s} before the barrier behind compute({s - 3}) of the "
                               f"{'late' if other else 'early'} waves")
    return bad


def xs_wait_programs():
    """(pp, P, res) of every wave program pair the kernel instantiates: a residual exists at P = 1 only (static_assert), ping-pong at
    P = 1 | 2 (no GEGLU)"""
    return [(False, P, False) for P in (1, 2, 4)] + [(False, 1, True)] + [(True, P, False) for P in (1, 2)] + [(True, 1, True)]


def xs_rounds_once(kind) -> bool:
    """plain and GEGLU-without-LayerNorm launches round ONCE after the fp32 accumulation: judged by the misrounded share too"""
    return kind in ("plain", "geglu")


def xs_baselines(c):
    """the independent fp32 implementations of one launch that set the misrounded bar: chains of 8, chains of 32, torch's fp32 matmul"""
    return {"alg8": xs_base_alg(c, 8), "alg32": xs_base_alg(c, 32), "torch32": xs_base_alg(c, None)}


def xs_out_guarded(M, cstore, dtype, device="cpu"):
    """(buffer, payload view) of an output with pitch cstore + XS_PAD_COLS and XS_GUARD_ROWS rows on either side, every element the payload
    NaN of ATTN_NAN_BITS (which no arithmetic produces)"""
    big = torch.full((M + 2 * XS_GUARD_ROWS, cstore + XS_PAD_COLS), ATTN_NAN_BITS[dtype], dtype=torch.int16).view(dtype).to(device)
    return big, big[XS_GUARD_ROWS:XS_GUARD_ROWS + M, :cstore]


def xs_guards_intact(big, M, cstore) -> bool:
    """every guard row and guard column still holds the NaN bits it was filled with"""
    bits = big.detach().cpu().view(torch.int16).clone()
    want = bits[0, 0].item()
    bits[XS_GUARD_ROWS:XS_GUARD_ROWS + M, :cstore] = want
    return bool((bits == want).all())


if __name__ == "__main__":
    import sys
    if "--attn-child" in sys.argv:
        args = sys.argv[sys.argv.index("--attn-child") + 1:]
        if args[2] == "views":          # IN OUT views: the rows of tests/test_attention_gpu.py (views, guarded outputs, three launches each)
            from tests import test_attention_gpu as A
            A.attention_views_child(args)
        else:
            from tests import test_numerics_gpu as T
            T.attention_child(args)
    elif "--report" in sys.argv:
        from tests import test_numerics_gpu as T
        only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
        rest = [a for a in sys.argv[sys.argv.index("--report") + 1:] if not a.startswith("-") and a != only]
        T.write_report(rest[0] if rest else None, only=only)
    else:
        print(__doc__)

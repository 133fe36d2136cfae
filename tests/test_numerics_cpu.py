"""tests/numerics.py has teeth (no GPU needed): the generators meet their postconditions at the shapes test_numerics_gpu.py uses,
the design of every kernel family (base_alg) stays inside the bar against the textbook sequence (base_ref) in the required tier,
and planted defects - CPU emulations that differ from base_alg in ONE way - exceed the bars the GPU test applies."""
import math

import pytest
import torch

from tests import numerics as nm

DTYPES = [torch.float16, torch.bfloat16]


def _bar(e_alg, e_ref):
    """a planted defect must be out by BOTH bars of the GPU test (it asserts kernel <= MARGIN * base_alg and <= MARGIN * base_ref)"""
    return nm.MARGIN * max(e_alg, e_ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_generators_meet_their_postconditions(dtype):
    """every generator asserts its own postconditions; here at the shapes and settings of the GPU cases"""
    for ratio in nm.REQUIRED_RATIOS + nm.PROBE_RATIOS:
        for frac in (0.0, 0.01):
            for peak in (4.0, 2.0e4):
                x = nm.token_rows(300, 320, ratio, frac, (50.0, 100.0), peak, dtype, seed=ratio)
                assert x.shape == (300, 320) and torch.equal(x, nm.rnd(x, dtype))
        nm.token_rows(130, 1280, ratio, 0.01, (50.0, 100.0), 2.0e4, dtype, seed=1)
    for (C, H, G) in [(320, 16, 32), (640, 16, 32), (640, 16, 1), (320, 16, 5), (128, 16, 32)]:
        for ratio in nm.REQUIRED_RATIOS:
            x = nm.group_maps(2, C, H, G, ratio, 0.01, (50.0, 100.0), 2.0e3, dtype, seed=C + ratio)
            assert x.shape == (2, H, H, C)
        nm.group_maps(2, C, H, G, 30, peak=4.0, dtype=dtype, seed=C, dominant_channel=True)
    for Skv, spread in [(1024, 15), (4096, 15), (4096, 17)]:
        q, k, v = nm.spike_and_sea(1, 2, 128, Skv, 40, spread, dtype, seed=Skv + spread)
        assert q.shape == (1, 128, 80) and k.shape == v.shape == (1, Skv, 80)
    nm.spike_and_sea(1, 2, 128, 4096, 40, 20, dtype, seed=3, control=True)
    with pytest.raises(AssertionError):
        nm.spike_and_sea(1, 2, 128, 4096, 40, 20, dtype, seed=3)                  # spread 20 is the control: its tail is no sea
    for d in (40, 80, 160):
        nm.late_risers(1, 2, 128, 512, d, dtype=dtype, seed=d)
        nm.one_loud_query(1, 2, 128, 512, d, wave=32, dtype=dtype, seed=d)
        nm.one_loud_query(1, 2, 128, 77, d, wave=64, dtype=dtype, seed=d)
        for shift in (300.0, -300.0):
            nm.common_shift(1, 2, 128, 256, d, shift, dtype, seed=d)
        nm.loud_values(1, 2, 128, 256, d, 2.0e4, dtype, seed=d)


def test_row_err_is_per_row_and_refuses_a_silent_row():
    ref = torch.tensor([[100.0, -100.0], [1.0, -1.0]], dtype=torch.float64)
    y = ref.clone()
    y[1, 0] = 1.05                                          # the quiet row is 5 % off
    assert abs(nm.row_err(y, ref) - 0.05) < 1e-12
    assert nm.old_metric(y, ref) < 1e-3                     # ... which the whole-tensor metric forgives
    e_max, e_rms = nm.row_err(y, ref, both=True)
    assert e_rms < e_max
    with pytest.raises(AssertionError):
        nm.row_err(torch.zeros(2, 2), torch.tensor([[1.0, 1.0], [0.0, 0.0]]))
    assert nm.row_err(torch.tensor([[float("inf"), 0.0]]), torch.ones(1, 2)) == float("inf")
    assert nm.finite_where_representable(torch.tensor([1.0, float("inf")]), torch.tensor([1.0, 1.0e5]), torch.float16)
    assert not nm.finite_where_representable(torch.tensor([1.0, float("inf")]), torch.tensor([1.0, 6.0e4]), torch.float16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layer_norm_fold_design_is_inside_the_bar_in_the_required_tier(dtype):
    """row_err(base_alg) <= MARGIN * row_err(base_ref), both > 0, for both forms (the tiled kernels' fold and es_linear_xs's
    normalise-in-registers), plain and GEGLU, with and without outlier channels, at both peaks - before the GPU test relies on it."""
    for ratio in nm.REQUIRED_RATIOS:
        for frac in (0.0, 0.01):
            for peak in (4.0, 2.0e4):
                for (M, C, Cout, geglu) in [(300, 320, 960, False), (130, 640, 5120, True)]:
                    x = nm.token_rows(M, C, ratio, frac, (50.0, 100.0), peak, dtype, seed=ratio)
                    c = nm.ln_case(x, Cout, dtype, geglu=geglu, seed=1)
                    assert nm.ln_intermediates_peak(c) < 3.0e4
                    ref = nm.ln_ref64(c)
                    e_ref = nm.row_err(nm.ln_base_ref(c), ref)
                    for form in ("fold", "xs"):
                        e_alg = nm.row_err(nm.ln_base_alg(c, form), ref)
                        assert 0 < e_alg <= nm.MARGIN * e_ref and e_ref > 0, (ratio, frac, peak, C, form, e_alg, e_ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_group_norm_design_is_inside_the_bar_in_the_required_tier(dtype):
    """... including groups of 40960 and 262144 values (the 64 x 64 level, the VAE's 256 x 256 maps), where the ORDER of the one-pass
    sums decides: base_alg sums in the kernels' three short levels (numerics.gn_chunked_stats); one flat fp32 sum per group is up to
    ten times base_ref there at |mean| / std = 30"""
    for ratio in nm.REQUIRED_RATIOS:
        for (C, H, G, silu, Cout, dom) in [(320, 16, 32, True, 0, False), (320, 16, 32, False, 0, True), (640, 16, 32, False, 640, False),
                                           (640, 16, 1, False, 640, False), (320, 16, 5, False, 320, False),
                                           (320, 64, 32, True, 0, False), (128, 256, 32, True, 0, False)]:
            if H > 16 and ratio in (3, 10):
                continue
            x = nm.group_maps(1 if H > 64 else 2, C, H, G, ratio, 0.0 if dom else 0.01, (50.0, 100.0), 4.0 if dom else 2.0e3, dtype, seed=C + ratio,
                              dominant_channel=dom)
            c = nm.gn_case(x, G, dtype, silu=silu, eps=1e-6 if Cout else 1e-5, seed=2, Cout=Cout)
            assert nm.gn_intermediates_peak(c) < 3.0e4
            ref = nm.gn_ref64(c)
            e_ref, e_alg = nm.row_err(nm.gn_base_ref(c), ref), nm.row_err(nm.gn_base_alg(c), ref)
            assert 0 < e_alg <= nm.MARGIN * e_ref and e_ref > 0, (ratio, C, G, silu, Cout, e_alg, e_ref)


ATTN_FAMILIES = [
    ("sea_1024_15", lambda dt: nm.spike_and_sea(1, 2, 128, 1024, 40, 15, dt, seed=1)),
    ("sea_4096_15", lambda dt: nm.spike_and_sea(1, 2, 128, 4096, 40, 15, dt, seed=2)),
    ("sea_4096_17", lambda dt: nm.spike_and_sea(1, 2, 128, 4096, 40, 17, dt, seed=3)),
    ("control_4096_20", lambda dt: nm.spike_and_sea(1, 2, 128, 4096, 40, 20, dt, seed=4, control=True)),
    ("late_risers", lambda dt: nm.late_risers(1, 2, 128, 512, 40, dtype=dt, seed=5)),
    ("shift_plus_300", lambda dt: nm.common_shift(1, 2, 128, 256, 40, 300.0, dt, seed=6)),
    ("shift_minus_300", lambda dt: nm.common_shift(1, 2, 128, 256, 40, -300.0, dt, seed=7)),
    ("one_loud_query", lambda dt: nm.one_loud_query(1, 2, 128, 512, 40, dtype=dt, seed=8)),
    ("loud_values", lambda dt: nm.loud_values(1, 2, 128, 256, 40, 2.0e4, dt, seed=9)),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,make", ATTN_FAMILIES, ids=[n for n, _ in ATTN_FAMILIES])
def test_attention_design_is_inside_the_bar(name, make, dtype):
    """the design (Q pre-scaled and re-rounded, a reference anywhere between the maximum and LAZY below it) against the textbook
    softmax, both against fp64; a reference kept LAZY below the maximum changes (nearly) nothing"""
    q, k, v = make(dtype)
    ref = nm.attn_ref64(q, k, v, 2)
    e_ref = nm.row_err(nm.attn_base_ref(q, k, v, 2, dtype), ref)
    e0 = nm.row_err(nm.attn_base_alg(q, k, v, 2, dtype, offset=0.0), ref)
    e8 = nm.row_err(nm.attn_base_alg(q, k, v, 2, dtype, offset=nm.LAZY), ref)
    print(f"{name} {dtype}: base_ref {e_ref:.3e}  base_alg {e0:.3e} (reference at the maximum) {e8:.3e} (LAZY below)")
    assert e_ref > 0 and 0 < max(e0, e8) <= nm.MARGIN * e_ref, (name, e0, e8, e_ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_colsum_of_the_unrounded_weights_exceeds_the_bar(dtype):
    """the column sums must be those of the ROUNDED W * gamma the matrix cores multiply: taken from the unrounded product they leave
    mean * (rounding error of a weight row) in every output, which grows with |mean| / std"""
    x = nm.token_rows(300, 320, 10, 0.0, peak=4.0, dtype=dtype, seed=10)
    c = nm.ln_case(x, 960, dtype, seed=1)
    ref = nm.ln_ref64(c)
    e_ref, e_alg = nm.row_err(nm.ln_base_ref(c), ref), nm.row_err(nm.ln_base_alg(c), ref)
    bad = nm.ln_base_alg(c, defect="colsum_unrounded")
    assert nm.row_err(bad, ref) > _bar(e_alg, e_ref), (nm.row_err(bad, ref), e_alg, e_ref)
    if dtype == torch.float16:
        # The reason this file exists: the whole-tensor max / max metric with the tolerance test_linear_with_folded_layer_norm applies
        # (4e-3 in fp16) PASSES this defect - max|ref| is 4-5 row rms, and one bar serves every row.
        assert nm.old_metric(bad, ref) < 4e-3


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_fp16_partial_sums_in_the_statistics_exceed_the_bar(dtype):
    """the one-pass sums must stay in fp32: partial sums of 64 channels rounded to fp16 move the mean by 2^-11 |mean|, i.e. by
    |mean| / std * 2^-11 standard deviations"""
    x = nm.token_rows(300, 320, 30, 0.01, peak=4.0, dtype=dtype, seed=30)
    c = nm.ln_case(x, 960, dtype, seed=1)
    ref = nm.ln_ref64(c)
    e_ref = nm.row_err(nm.ln_base_ref(c), ref)
    for form in ("fold", "xs"):
        e_alg = nm.row_err(nm.ln_base_alg(c, form), ref)
        assert nm.row_err(nm.ln_base_alg(c, form, defect="partial_sums_fp16"), ref) > _bar(e_alg, e_ref)


def test_channel_to_group_map_of_the_group_norm_fold_is_exact():
    """csrc/linear_xs.hip finds a channel's GroupNorm group with an integer reciprocal: it must equal c // cpg for every (K, G) that
    es_linear_xs accepts (K = 320 | 640, 1 <= G <= 32 dividing K) and fit 32 bits.  The 2^16 reciprocal used before was wrong for
    exactly one of those pairs, (640, 1): channels 637..639 went to a group 1 that does not exist."""
    wrong = []
    for K in (320, 640):
        for G in range(1, 33):
            if K % G:
                continue
            cpg = K // G
            assert (K - 1) * (((1 << 20) + cpg - 1) // cpg) < 1 << 32
            assert all(nm.xs_group_of_channel(c, cpg) == c // cpg for c in range(K)), (K, G)
            if any(nm.xs_group_of_channel_2_16(c, cpg) != c // cpg for c in range(K)):
                wrong.append((K, G, [c for c in range(K) if nm.xs_group_of_channel_2_16(c, cpg) != c // cpg]))
    assert wrong == [(640, 1, [637, 638, 639])]
    # the kernel source uses the map this test checks
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "edgestyle_amd", "csrc", "linear_xs.hip")).read()
    assert "((1u << 20) + (unsigned)cpg - 1u) / (unsigned)cpg" in src and "* inv) >> 20)" in src and ">> 16" not in src


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_wrong_group_for_the_last_channels_exceeds_the_bar(dtype):
    """K = 640 with ONE GroupNorm group in front of the projection: channels 637..639 normalised with statistics that are not their
    group's - the (640, 1) case of test_group_norm_in_front_of_the_row_stationary_projection would have caught the 2^16 reciprocal"""
    for ratio in (0, 30):
        x = nm.group_maps(2, 640, 16, 1, ratio, 0.01, (50.0, 100.0), 2.0e3, dtype, seed=640 + ratio)
        c = nm.gn_case(x, 1, dtype, eps=1e-6, seed=2, Cout=640)
        ref = nm.gn_ref64(c)
        e_ref, e_alg = nm.row_err(nm.gn_base_ref(c), ref), nm.row_err(nm.gn_base_alg(c), ref)
        assert nm.row_err(nm.gn_base_alg(c, defect="wrong_group_tail"), ref) > _bar(e_alg, e_ref)


@pytest.mark.parametrize("Skv,spread", [(1024, 15), (4096, 15), (4096, 17)])
def test_planted_flush_of_subnormal_p_exceeds_the_bar(Skv, spread):
    """fp16: every sea key's P is below 2^-14 of the maximum, i.e. an fp16 SUBNORMAL when the reference sits at the maximum; a
    conversion or a matrix core that flushes them loses the sea (2.5 % .. 50 % of the mass, V offset by 3): an order of magnitude over
    the bars.  (bf16 has fp32's exponent range: there the case measures rounding only.)"""
    dt = torch.float16
    q, k, v = nm.spike_and_sea(1, 2, 128, Skv, 40, spread, dt, seed=Skv + spread)
    ref = nm.attn_ref64(q, k, v, 2)
    e_ref = nm.row_err(nm.attn_base_ref(q, k, v, 2, dt), ref)
    e_alg = nm.attn_design_err(q, k, v, 2, dt, ref)
    e_bad = nm.row_err(nm.attn_base_alg(q, k, v, 2, dt, defect="flush_p"), ref)
    assert e_bad > 10 * _bar(e_alg, e_ref), (e_bad, e_alg, e_ref)
    # the control (spread 20: a tail below 1 % of the mass) is where such a flush would hide
    q, k, v = nm.spike_and_sea(1, 2, 128, 4096, 40, 20, dt, seed=4, control=True)
    ref = nm.attn_ref64(q, k, v, 2)
    assert nm.row_err(nm.attn_base_alg(q, k, v, 2, dt, defect="flush_p"), ref) < 0.05


@pytest.mark.parametrize("dtype,step", [(torch.float16, 10.0), (torch.bfloat16, 25.0)])
def test_planted_stale_softmax_reference_exceeds_the_bar(dtype, step):
    """a reference that stays at the first tile's maximum while later tiles rise by `step` each: P leaves the storage dtype's range
    (fp16: 2^16 after two rises of 10; bf16 and the fp32 row sum: 2^128 after six rises of 25)"""
    q, k, v = nm.late_risers(1, 2, 128, 512, 40, step_log2=step, dtype=dtype, seed=5)
    ref = nm.attn_ref64(q, k, v, 2)
    e_ref = nm.row_err(nm.attn_base_ref(q, k, v, 2, dtype), ref)
    e_alg = nm.attn_design_err(q, k, v, 2, dtype, ref)
    assert math.isfinite(e_alg) and e_alg <= nm.MARGIN * e_ref
    assert nm.row_err(nm.attn_base_alg(q, k, v, 2, dtype, defect="stale_reference"), ref) > _bar(e_alg, e_ref)


# ----------------------------------------------------------------------------------------------------------------
# convolution: the misrounded share
# ----------------------------------------------------------------------------------------------------------------
OLD_CONV_TOL = {torch.float16: 3e-3, torch.bfloat16: 2e-2}          # test_ops_gpu.py::test_conv_gemm
CONV_INPUT_CLASSES = [("randn", "randn"), ("silu0", "randn"), ("silu3", "randn"), ("peak", "randn"), ("near_2^10", "subnormal")]


def _conv_counts(c, ref, splitk=1, korder=0, against=None):
    """name -> number of elements of every independent fp32 implementation that differ from the correctly rounded truth (or, for a
    form with a residual, from `against` = base_alg)"""
    dt = c["dtype"]
    base = nm.conv_baselines(c, splitk, korder)
    if against is None:
        return {k: nm.misrounded(v, ref, dt, count=True) for k, v in base.items()}
    return {k: nm.differs(v, against, count=True) for k, v in base.items() if k != "alg8"}


def test_round64_breaks_the_ties_of_a_double_rounding():
    """1 + 2^-11 + 2^-40 lies ABOVE the fp16 tie between 1 and 1 + 2^-10; fp64 -> fp32 lands on the tie and fp32 -> fp16 rounds it to
    even, i.e. down.  round64 must round up; exact ties still go to even, and misrounded counts NaN as different."""
    v = torch.tensor([1 + 2.0 ** -11 + 2.0 ** -40, 1 + 2.0 ** -11 - 2.0 ** -40, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11 + 2.0 ** -40)],
                     dtype=torch.float64)
    assert float(v[:1].float().half()) == 1.0                                           # the double rounding this guards against
    assert nm.round64(v, torch.float16).tolist() == [1 + 2.0 ** -10, 1.0, 1.0, 1 + 2.0 ** -9, -(1 + 2.0 ** -10)]
    y = torch.tensor([1 + 2.0 ** -10, 1.0, float("nan"), 1 + 2.0 ** -9, -1.0])
    assert nm.misrounded(y, v, torch.float16, count=True) == 2 and nm.misrounded(y, v, torch.float16) == 0.4
    assert nm.misrounded_bar([3, 49]) == nm.MISROUNDED_FLOOR and nm.misrounded_bar([50, 7]) == 100 and nm.misrounded_bar([400]) == 800


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_generators_and_references_agree_with_each_other(dtype):
    """conv_im2col (the kernel's K orders, the upsample, stride 2, an explicit out_hw, the concat, tail sources) times the weights in
    fp64 equals conv_ref64's F.conv2d, for every geometry class of the GPU sweep; the split-K slices tile K"""
    for kw in [dict(H=5, W=7), dict(H=9, W=12, stride=2), dict(H=10, W=14, stride=2, pad=0, out_hw=(5, 7)), dict(H=3, W=8, upsample=True),
               dict(H=1, W=37), dict(H=37, W=1), dict(H=13, W=1, k=1), dict(H=1, W=1, k=1), dict(H=6, W=5, C2=64, tails=(64, 128)),
               dict(H=12, W=10, upsample=True, korder=1), dict(H=9, W=12, stride=2, korder=1, C2=64, tails=(64,))]:
        kw = dict(kw)
        korder = kw.pop("korder", 0)
        c = nm.conv_case(2, kw.pop("H"), kw.pop("W"), 64, 24, dtype, bias=False, seed=3, **kw)
        A, Wm = nm.conv_im2col(c, korder)
        want = nm.conv_ref64(c)
        got = (A.double() @ Wm.double().t()).reshape(want.shape)
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), kw
    for K, sk in [(576, 1), (576, 3), (704, 5), (2880, 7), (72, 2)]:
        sl = nm.conv_splitk_slices(K, sk)
        assert sl[0][0] == 0 and sl[-1][1] == K and all(a[1] == b[0] or (a[1] == K and b[0] >= K) for a, b in zip(sl, sl[1:]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_design_is_inside_every_bar(dtype):
    """base_alg with chains of 8 (the launch as designed) against the bars the GPU test applies, for every input class: its
    misrounded count within MARGIN x the largest count of the OTHER fp32 implementations (chains of 32, torch's fp32 convolution; the
    floor of 100 elements where those are under 50), row_err within MARGIN x base_ref, finite wherever the truth is representable -
    3x3 at K = 2880 with split-K 4, 1x1 at K = 64, and the epilogue forms (with a residual: nothing differs from base_alg by
    definition; the others' distance to it is what sets the GPU bar)."""
    shapes = [dict(N=3, H=9, W=12, C1=320, Cout=160, splitk=4), dict(N=3, H=9, W=12, C1=1280, Cout=64, splitk=4),
              dict(N=3, H=13, W=11, C1=64, Cout=64, k=1, splitk=1)]
    for inputs, weights in CONV_INPUT_CLASSES:
        for sh in shapes:
            sh = dict(sh)
            sk = sh.pop("splitk")
            c = nm.conv_case(dtype=dtype, inputs=inputs, weights=weights, seed=11, **sh)
            ref = nm.conv_ref64(c)
            assert ref.numel() >= nm.CONV_MIN_ELEMENTS
            cnt = _conv_counts(c, ref, sk)
            bar = nm.misrounded_bar([cnt["alg32"], cnt["torch32"]])
            y = nm.conv_base_alg(c, 8, sk)
            e, e_ref = nm.row_err(y, ref), nm.row_err(nm.conv_base_ref(c), ref)
            print(f"conv design {inputs}/{weights} {sh} {dtype}: misrounded " + " ".join(f"{k} {v / ref.numel():.4%}" for k, v in cnt.items())
                  + f"  bar {bar} elements  row_err {e:.3e} base_ref {e_ref:.3e}")
            assert cnt["alg8"] <= bar, (inputs, sh, cnt, bar)
            assert 0 < e <= nm.MARGIN * e_ref and nm.finite_where_representable(y, ref, dtype), (inputs, sh, e, e_ref)
            if inputs == "peak":
                assert 2.0e4 <= float(ref.abs().max()) <= 3.0e4 and bool(torch.isfinite(y).all())
    c = nm.conv_case(3, 9, 12, 128, 192, dtype, C2=64, temb=True, silu=True, scale=0.7, residual=True, seed=12)
    alg = nm.conv_base_alg(c, 8, 2)
    cnt = _conv_counts(c, None, 2, against=alg)
    print(f"conv design +temb +SiLU +scale +residual {dtype}: differing from base_alg " + " ".join(f"{k} {v / alg.numel():.4%}" for k, v in cnt.items()))
    assert max(cnt.values()) < 0.01 * alg.numel()                   # two legitimate fp32 orders: far below what one extra rounding makes
    c = nm.conv_case(3, 9, 12, 128, 192, torch.bfloat16, k=1, residual=True, residual_lo=True, seed=13)
    hi, lo = nm.conv_base_alg(c, 8, 1, wide=True)
    ref = nm.conv_ref64(c)
    one = nm.conv_base_alg(c, 8, 1)
    # the convolution's own value is rounded BEFORE the sum in both forms (the design): the pair saves the second rounding, no more
    assert 0 < nm.row_err(hi + lo, ref) < nm.row_err(one, ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_zero_weights_return_the_rounded_bias_and_subnormal_weights_are_kept(dtype):
    c = nm.conv_case(3, 9, 12, 64, 96, dtype, weights="zero", seed=14)
    y = nm.conv_base_alg(c, 8, 3)
    assert torch.equal(y, nm.rnd(c["b"], dtype).expand_as(y)) and nm.misrounded(y, nm.conv_ref64(c), dtype) == 0
    c = nm.conv_case(3, 9, 12, 64, 96, dtype, inputs="near_2^10", weights="subnormal", seed=15)
    ref = nm.conv_ref64(c)
    cnt = _conv_counts(c, ref)
    flushed = nm.conv_base_alg(dict(c, w=torch.zeros_like(c["w"])), 8)          # what a flush of fp16 subnormals would return: the bias
    assert nm.misrounded(flushed, ref, dtype, count=True) > 0.9 * ref.numel() > nm.misrounded_bar(cnt.values())
    assert nm.row_err(flushed, ref) > _bar(nm.row_err(nm.conv_base_alg(c, 8), ref), nm.row_err(nm.conv_base_ref(c), ref))


ROUNDING_DEFECTS = ["rounded_slabs", "late_bias"]
GEOMETRY_DEFECTS = [  # defect, the case it is planted in
    ("hw_swapped", dict(N=3, H=9, W=12, C1=64, Cout=96)),                                   # non-square
    ("right_tap", dict(N=3, H=9, W=12, C1=64, Cout=320, stride=2)),                         # even width, stride 2: tap kx = 2 of the last column reads column W - 1
    ("wrap_next_sample", dict(N=3, H=9, W=12, C1=64, Cout=96)),
    ("tile_unwritten", dict(N=3, H=9, W=12, C1=64, Cout=96)),                               # 324 pixels: three tiles
    ("temb_first_pixel", dict(N=3, H=9, W=12, C1=64, Cout=96, temb=True)),                  # 108 pixels per sample: tiles straddle samples
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect", ROUNDING_DEFECTS)
def test_planted_extra_rounding_in_the_convolution_exceeds_the_misrounded_bar_and_passes_the_old_metric(defect, dtype):
    """split-K slabs rounded to the storage dtype before the reduce, and the bias added behind the rounding: 25-40 % of the elements
    leave the correctly rounded value (the bar: under 1 %), while test_conv_gemm's max|y - ref| / max|ref| against torch's fp32
    convolution PASSES both, and row_err cannot tell them from the design within MARGIN (printed)."""
    for inputs, weights in CONV_INPUT_CLASSES[:3]:
        for sh in [dict(N=3, H=9, W=12, C1=320, Cout=160), dict(N=3, H=9, W=12, C1=1280, Cout=64)]:
            c = nm.conv_case(dtype=dtype, inputs=inputs, weights=weights, seed=21, **sh)
            ref = nm.conv_ref64(c)
            cnt = _conv_counts(c, ref, 4)
            bar = nm.misrounded_bar(cnt.values())
            bad = nm.conv_base_alg(c, 8, 4, defect=defect)
            n_bad = nm.misrounded(bad, ref, dtype, count=True)
            old = nm.old_metric(bad, nm._conv_plain(c, lambda v: v.float()) + c["b"])
            e_bad, e_alg, e_ref = nm.row_err(bad, ref), nm.row_err(nm.conv_base_alg(c, 8, 4), ref), nm.row_err(nm.conv_base_ref(c), ref)
            print(f"conv {defect} {inputs} {sh} {dtype}: misrounded {n_bad / ref.numel():.2%} (design "
                  + " ".join(f"{k} {v / ref.numel():.4%}" for k, v in cnt.items()) + f", bar {bar / ref.numel():.3%})  old metric {old:.2e} "
                  f"(passes < {OLD_CONV_TOL[dtype]:g})  row_err defect / design {e_bad / e_alg:.2f}")
            assert n_bad > 10 * bar, (defect, inputs, sh, n_bad, bar)
            assert old < OLD_CONV_TOL[dtype], (defect, old)
            assert e_bad <= 1.1 * _bar(e_alg, e_ref)        # ... and the per-row metric does not separate them either: why the share is needed


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect,shape", GEOMETRY_DEFECTS, ids=[d for d, _ in GEOMETRY_DEFECTS])
def test_planted_geometry_defects_in_the_convolution_exceed_the_bars(defect, shape, dtype):
    """a swapped H / W in the pixel decode, a dropped tap at the right edge, a bottom tap that reads the next sample, a tile that is
    never stored, a time-embedding row taken per tile where a tile straddles two samples: each is outside the misrounded bar AND
    outside the row_err bars (or not finite)"""
    c = nm.conv_case(dtype=dtype, seed=22, **shape)
    ref = nm.conv_ref64(c)
    assert ref.numel() >= nm.CONV_MIN_ELEMENTS
    cnt = _conv_counts(c, ref)
    bar = nm.misrounded_bar(cnt.values())
    bad = nm.conv_base_alg(c, 8, defect=defect)
    n_bad = nm.misrounded(bad, ref, dtype, count=True)
    e_bad, e_alg, e_ref = nm.row_err(bad, ref), nm.row_err(nm.conv_base_alg(c, 8), ref), nm.row_err(nm.conv_base_ref(c), ref)
    print(f"conv {defect} {shape} {dtype}: misrounded {n_bad / ref.numel():.2%} (bar {bar / ref.numel():.3%})  row_err {e_bad:.2e} (design {e_alg:.2e})")
    assert n_bad > bar and n_bad > 0.01 * ref.numel(), (defect, n_bad, bar)
    assert e_bad > _bar(e_alg, e_ref), (defect, e_bad, e_alg, e_ref)
    if defect == "tile_unwritten":
        assert e_bad == float("inf") and nm.BM_CONV * c["Cout"] <= n_bad <= nm.BM_CONV * c["Cout"] + bar
    if defect == "hw_swapped":                   # ... and invisible on a square image
        sq = nm.conv_case(dtype=dtype, seed=22, **dict(shape, W=shape["H"]))
        assert torch.equal(nm.conv_base_alg(sq, 8, defect=defect), nm.conv_base_alg(sq, 8))

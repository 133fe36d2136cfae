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


def _attn_errs(q, k, v, heads, dtype, ref, **kw):
    """row_err of attn_base_alg at both ends of the reference's range (offsets 0 and LAZY)"""
    return [nm.row_err(nm.attn_base_alg(q, k, v, heads, dtype, offset=o, **kw), ref) for o in (0.0, nm.LAZY)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [40, 80])
@pytest.mark.parametrize("Skv", [5, 65, 77, 129])
def test_attention_masking_defects_at_ragged_lengths(Skv, d, dtype):
    """Key counts that end inside a tile, where the kernels mask: the design stays inside both bars on every input class, a padded key
    admitted at score 0 (zero K row, zero V row) is outside them when all logits sit at -300 and EXACTLY as good as the design when
    they sit at +300 (its weight is e^-300: the reason the shift-300 class exists, and why randn - weight 1 / (Skv + 1) - is a poor
    judge of masking), and dropping the last valid key is outside them when that key decides."""
    N, heads, Sq = 2, 2, 70
    rowsum = "rounded" if nm.attn_ones(d) else "fp32"
    got = {}
    for kind in ("shift-300", "shift+300", "last_key_decides", "randn"):
        q, k, v = nm.attn_inputs(kind, N, heads, Sq, Skv, d, dtype, seed=Skv + d)
        ref = nm.attn_ref64(q, k, v, heads)
        e_ref = nm.row_err(nm.attn_base_ref(q, k, v, heads, dtype), ref)
        for rs in ("fp32", "rounded"):
            e_alg = max(_attn_errs(q, k, v, heads, dtype, ref, rowsum=rs))
            assert nm.attn_design_err(q, k, v, heads, dtype, ref, rowsum=rs) == e_alg
            print(f"Skv={Skv} d={d} {dtype} {kind} rowsum={rs}: base_ref {e_ref:.3e} base_alg {e_alg:.3e}")
            assert e_ref > 0 and 0 < e_alg <= nm.MARGIN * e_ref, (kind, rs, e_alg, e_ref)
        e_alg = nm.attn_design_err(q, k, v, heads, dtype, ref, rowsum=rowsum)
        got[kind] = (q, k, v, ref, e_alg, e_ref)
    q, k, v, ref, e_alg, e_ref = got["shift-300"]
    bad = _attn_errs(q, k, v, heads, dtype, ref, rowsum=rowsum, defect="pad_key_admitted")
    print(f"Skv={Skv} d={d} {dtype} pad_key_admitted at -300: {min(bad):.3e} against base_alg {e_alg:.3e} base_ref {e_ref:.3e}")
    assert min(bad) > _bar(e_alg, e_ref), (bad, e_alg, e_ref)
    q, k, v, ref, e_alg, e_ref = got["shift+300"]
    bad = _attn_errs(q, k, v, heads, dtype, ref, rowsum=rowsum, defect="pad_key_admitted")
    print(f"Skv={Skv} d={d} {dtype} pad_key_admitted at +300: {max(bad):.3e} against base_alg {e_alg:.3e} base_ref {e_ref:.3e}")
    assert max(bad) <= nm.MARGIN * min(e_alg, e_ref) and max(bad) == e_alg, (bad, e_alg, e_ref)
    q, k, v, ref, e_alg, e_ref = got["last_key_decides"]
    bad = _attn_errs(q, k, v, heads, dtype, ref, rowsum=rowsum, defect="last_key_dropped")
    print(f"Skv={Skv} d={d} {dtype} last_key_dropped: {min(bad):.3e} against base_alg {e_alg:.3e} base_ref {e_ref:.3e}")
    assert min(bad) > _bar(e_alg, e_ref), (bad, e_alg, e_ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_generators_at_ragged_and_tiny_key_counts(dtype):
    """the input classes of tests/test_attention_gpu.py assert their postconditions at every key count its table uses"""
    for Skv in (1, 2, 5, 31, 33, 63, 64, 65, 77, 81, 96, 127, 129, 193, 320):
        for d in (8, 40, 64, 512):
            for kind in nm.ATTN_INPUT_KINDS:
                if Skv == 1 and kind in ("one_loud_query", "last_key_decides"):
                    continue
                q, k, v = nm.attn_inputs(kind, 1, 2, 33, Skv, d, dtype, seed=Skv + d)
                assert q.shape == (1, 33, 2 * d) and k.shape == v.shape == (1, Skv, 2 * d)
                assert all(torch.equal(t, nm.rnd(t, dtype)) for t in (q, k, v))


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_view_builders(dtype, poison):
    """attn_views: the poisoned mask and the three views partition the buffer, the views equal the dense operands bit for bit, the
    layout is the documented one; attn_out_guarded's check() notices one overwritten guard element and one NaN inside the view"""
    N, heads, Sq, Skv, d = 3, 3, 70, 77, 40
    C = heads * d
    q, k, v = nm.attn_inputs("randn", N, heads, Sq, Skv, d, dtype, seed=1)
    for sl in (False, True):
        qv, kv, vv, mask = nm.attn_views(q, k, v, heads, dtype, poison, batch_slice=sl)
        buf = qv._base
        assert kv._base is buf and vv._base is buf and buf.dim() == 1 and buf.dtype == dtype and mask.shape == buf.shape
        ld, s_alloc = 3 * (C + 8), max(Sq, Skv) + 64
        assert qv.stride() == kv.stride() == vv.stride() == ((s_alloc + 64) * ld, ld, 1) and qv.stride(0) > s_alloc * ld
        assert buf.numel() == (N + 2 * sl) * qv.stride(0)
        assert kv.storage_offset() - qv.storage_offset() == C + 8 == vv.storage_offset() - kv.storage_offset()
        assert qv.storage_offset() == (qv.stride(0) if sl else 0)
        cover = torch.zeros(buf.numel(), dtype=torch.int32)
        for t in (qv, kv, vv):
            nm.view_from(cover, nm.view_recipe(t)).add_(1)
        cover += mask.int()
        assert bool((cover == 1).all())                                             # a partition: every element exactly once
        for t, dense in ((qv, q), (kv, k), (vv, v)):
            assert t.shape == dense.shape and torch.equal(t.contiguous().view(torch.int16), dense.to(dtype).view(torch.int16))
            assert torch.equal(nm.view_from(buf, nm.view_recipe(t)), t)
        pz = buf[mask].float()
        if poison == "nan":
            assert bool(torch.isnan(pz).all()) and bool((buf[mask].view(torch.int16).int() & 0xFFFF == nm.ATTN_NAN_BITS[dtype]).all())
        else:
            assert bool(torch.isfinite(pz).all()) and float(pz.abs().min()) > 5.9e4 and bool((pz > 0).any()) and bool((pz < 0).any())
    out, check = nm.attn_out_guarded(N, Sq, C, dtype)
    ob = out._base
    assert out.shape == (N, Sq, C) and out.stride() == ((Sq + 64) * (C + 8), C + 8, 1) and out.storage_offset() == 64 * (C + 8)
    assert ob.numel() == (64 + N * (Sq + 64)) * (C + 8) and bool(torch.isnan(ob.float()).all())
    with pytest.raises(AssertionError, match="inside"):
        check(ob)                                                                   # nothing written yet: the view is all NaN
    out.copy_(q.to(dtype))
    check(ob)
    for where in (0, out.storage_offset() - 1, out.storage_offset() + C, out.storage_offset() + Sq * (C + 8), ob.numel() - 1):
        hurt = ob.clone()
        hurt[where] = 1.0
        with pytest.raises(AssertionError, match="guard"):
            check(hurt)
        hurt[where] = float("nan")                                                  # another NaN than the payload one is an overwrite too
        if (int(hurt[where].view(torch.int16)) & 0xFFFF) != nm.ATTN_NAN_BITS[dtype]:
            with pytest.raises(AssertionError, match="guard"):
                check(hurt)
    hurt = ob.clone()
    nm.view_from(hurt, nm.view_recipe(out))[N - 1, Sq - 1, C - 1] = float("nan")
    with pytest.raises(AssertionError, match="inside"):
        check(hurt)


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


def _group_of_five(dtype):
    """the second weight group of a grouped launch over a shared source of two samples: five samples that start at launch index 3"""
    first = nm.conv_case(3, 8, 16, 64, 96, dtype, nsrc=2, seed=23)
    return nm.conv_case(5, 8, 16, 64, 96, dtype, src=first["x_src"], first=3, seed=24)


SOURCE_AND_SCALE_DEFECTS = [  # defect, the case it is planted in, split-K
    ("mod_per_tile", lambda dt: nm.conv_case(6, 9, 12, 64, 96, dt, rep=3, seed=25), 1),         # 108 pixels per sample: tiles straddle samples
    ("mod_in_group", _group_of_five, 1),                                                         # 3 % 2 != 0
    ("dev_scale_dropped_in_reduce", lambda dt: nm.conv_case(3, 9, 12, 64, 96, dt, scale=0.5, scale_dev=0.7, seed=26), 2),
    ("scale_before_act", lambda dt: nm.conv_case(3, 9, 12, 64, 96, dt, silu=True, scale=1 / 1.702, seed=27), 1),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect,make,splitk", SOURCE_AND_SCALE_DEFECTS, ids=[d for d, _, _ in SOURCE_AND_SCALE_DEFECTS])
def test_planted_source_and_scale_defects_in_the_convolution_exceed_the_bars(defect, make, splitk, dtype):
    """a shared source's modulo taken once per tile, or of the index inside the weight group; a device scale the split-K reduce forgets;
    a scale applied in front of the SiLU: each is outside the misrounded bar AND outside the row_err bars at the shape it is planted
    in, and the design - on the same case - is inside both"""
    c = make(dtype)
    ref = nm.conv_ref64(c)
    assert ref.numel() >= nm.CONV_MIN_ELEMENTS
    cnt = _conv_counts(c, ref, splitk)
    bar = nm.misrounded_bar(cnt.values())
    good, bad = nm.conv_base_alg(c, 8, splitk), nm.conv_base_alg(c, 8, splitk, defect=defect)
    n_bad = nm.misrounded(bad, ref, dtype, count=True)
    e_bad, e_alg, e_ref = nm.row_err(bad, ref), nm.row_err(good, ref), nm.row_err(nm.conv_base_ref(c), ref)
    print(f"conv {defect} {dtype}: misrounded {n_bad / ref.numel():.2%} (design {cnt['alg8'] / ref.numel():.4%}, bar {bar / ref.numel():.3%})  "
          f"row_err {e_bad:.2e} (design {e_alg:.2e}, base_ref {e_ref:.2e})")
    assert cnt["alg8"] <= nm.misrounded_bar([cnt["alg32"], cnt["torch32"]]) and 0 < e_alg <= nm.MARGIN * e_ref, (defect, cnt, e_alg, e_ref)
    assert n_bad > bar and n_bad > 0.01 * ref.numel(), (defect, n_bad, bar)
    assert e_bad > _bar(e_alg, e_ref), (defect, e_bad, e_alg, e_ref)
    if defect == "mod_per_tile":                 # ... and invisible where every tile lies inside one sample: why the straddling rows are needed
        whole = nm.conv_case(6, 8, 16, 64, 96, dtype, rep=3, seed=25)
        assert (whole["out_hw"][0] * whole["out_hw"][1]) % nm.BM_CONV == 0
        assert torch.equal(nm.conv_base_alg(whole, 8, defect=defect), nm.conv_base_alg(whole, 8))
    if defect == "mod_in_group":                 # ... and invisible in a group that starts on a multiple of nsrc
        even = nm.conv_case(5, 8, 16, 64, 96, dtype, src=c["x_src"], first=2, seed=24)
        assert torch.equal(nm.conv_base_alg(even, 8, defect=defect), nm.conv_base_alg(even, 8))
    if defect == "dev_scale_dropped_in_reduce":  # ... and in the fused epilogue of an unsplit launch
        assert torch.equal(nm.conv_base_alg(c, 8, 1, defect=defect), nm.conv_base_alg(c, 8, 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_case_with_a_shared_source_equals_the_repeated_tensor(dtype):
    """conv_case(rep=3): "x" is "x_src" repeated along the batch, and every reference of the case equals that of a case that was handed
    the repeated tensor as an ordinary source"""
    for kw in [dict(H=5, W=7), dict(H=1, W=1, k=1), dict(H=9, W=12, stride=2), dict(H=3, W=8, upsample=True)]:
        c = nm.conv_case(6, C1=64, Cout=24, dtype=dtype, rep=3, seed=28, **kw)
        assert c["nsrc"] == 2 and c["x_src"].shape[0] == 2 and c["x"].shape[0] == 6 and torch.equal(c["x"], c["x_src"].repeat(3, 1, 1, 1))
        plain = dict(c, x=c["x_src"].repeat(3, 1, 1, 1).contiguous(), x_src=None, nsrc=0)
        for f in (nm.conv_ref64, nm.conv_base_ref, nm.conv_torch32, nm.conv_base_alg):
            assert torch.equal(f(c), f(plain)), (kw, f.__name__)
        assert all(torch.equal(a, b) for a, b in zip(nm.conv_im2col(c), nm.conv_im2col(plain)))
    g = _group_of_five(dtype)
    assert [int(i) for i in (3 + torch.arange(5)) % 2] == [1, 0, 1, 0, 1] and torch.equal(g["x"][0], g["x_src"][1]) and torch.equal(g["x"][1], g["x_src"][0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_case_with_a_device_scale_equals_the_fp32_product_as_out_scale(dtype):
    """scale_dev: the references multiply by float32(out_scale) * float32(dev), one fp32 product as `scale *= *p.out_scale_dev` forms it"""
    kw = dict(N=3, H=9, W=12, C1=64, Cout=96, dtype=dtype, residual=True, seed=29)
    c = nm.conv_case(scale=0.5, scale_dev=0.7, **kw)
    prod = float(torch.tensor(0.5, dtype=torch.float32) * torch.tensor(0.7, dtype=torch.float32))
    assert c["scale"] == prod and c["scale_host"] == 0.5 and c["scale_dev"] == float(torch.tensor(0.7, dtype=torch.float32))
    one = nm.conv_case(scale=prod, **kw)
    assert one["scale_dev"] is None and one["scale"] == one["scale_host"] == prod
    for sk in (1, 3):
        assert torch.equal(nm.conv_base_alg(c, 8, sk), nm.conv_base_alg(one, 8, sk))
    assert torch.equal(nm.conv_ref64(c), nm.conv_ref64(one)) and torch.equal(nm.conv_base_ref(c), nm.conv_base_ref(one))


# ----------------------------------------------------------------------------------------------------------------
# the fusion block
# ----------------------------------------------------------------------------------------------------------------
FUSION_GRID_PINS = {  # (C, HW) -> (nchunk, cb, a thread keeps its column in passes A / B, in pass C): read off fusion_grids() in csrc/fusion.hip
    (8, 1): (1, 1, True, True), (24, 35): (3, 3, True, True),
    (64, 256): (1, 2, True, True),          # items = 2048: items / 2048 = 1 workgroup in A / B, items / 1024 = 2 in pass C
    (320, 4096): (80, 160, True, True), (320, 9216): (180, 360, True, True), (320, 16384): (255, 510, True, True),
    (64, 65536): (256, 512, True, True), (1280, 64): (5, 10, True, True),
    (2056, 16): (2, 257, False, True),      # q = 257 > 256: passes A and B reload their parameters per item, pass C does not
    (4168, 8): (2, 4, False, False),        # q = 521 > 512: all three passes reload per item
}
OLD_FUSION_SHAPES = [(64, 16), (320, 8), (1280, 8), (320, 64), (128, 8), (64, 32)]      # (C, S) of test_fusion_block_* in test_ops_gpu.py


def test_fusion_grid_mirror_is_pinned():
    for (C, HW), (nchunk, cb, fix_ab, fix_c) in FUSION_GRID_PINS.items():
        assert nm.fusion_grids(C, HW) == (nchunk, cb), (C, HW, nm.fusion_grids(C, HW))
        assert nm.fusion_fixed_column(C, nchunk) == fix_ab and nm.fusion_fixed_column(C, cb) == fix_c, (C, HW)
        assert nchunk <= nm.FU_MAX_CHUNK and cb <= nm.FU_MAX_CB


@pytest.mark.parametrize("dtype", DTYPES)
def test_fusion_generator_meets_its_postconditions(dtype):
    for kind in nm.FUSION_KINDS:
        for (N, C, HW) in [(3, 24, 35), (2, 64, 256), (1, 2056, 16)]:
            if kind.startswith("u_offset") and C == 24:
                N = 1           # b2 is shared by the samples: 840 heavy-tailed values per sample do not pin every sample's ratio to 10 %
            c = nm.fusion_case(N, C, HW, dtype, kind, seed=C + len(kind))
            assert len(c["res"]) == 6 and all(t.shape == (N, HW, C) for t in c["res"]) and len(c["params"]) == 10
            ref = nm.fusion_ref64(c)
            assert ref.shape == (N, HW, C) and bool(torch.isfinite(ref).all()) and float(ref.reshape(N, -1).std(dim=1).min()) > 0
    with pytest.raises(AssertionError):
        nm.fusion_case(1, 64, 16, dtype, "no_such_kind")


def test_fusion_ref64_equals_the_oracle_and_the_packing():
    """fusion_ref64 == oracle.controlnet_block(interleave_tensors(...)) on double tensors to 1e-12, and ops.pack_fusion_params packs the
    state dict of fusion_state_dict into exactly the case's parameter tensors (layout and storage dtypes)"""
    from edgestyle_amd import ops
    from oracle import sd15_oracle as O
    for (N, C, H, W, kind, dtype) in [(2, 24, 5, 7, "randn", torch.float16), (3, 64, 4, 4, "ratio_10", torch.bfloat16),
                                      (1, 8, 1, 1, "outliers", torch.float16), (1, 40, 3, 2, "u_offset_30", torch.bfloat16)]:
        c = nm.fusion_case(N, C, H * W, dtype, kind, seed=C)
        sd = nm.fusion_state_dict(c, "blk", H, W)
        nchw = [(t.double() * s).reshape(N, H, W, C).permute(0, 3, 1, 2) for t, s in zip(c["res"], c["scales"])]
        want = O.controlnet_block(sd, "blk", O.interleave_tensors(nchw)).permute(0, 2, 3, 1).reshape(N, H * W, C)
        got = nm.fusion_ref64(c)
        assert got.dtype == want.dtype == torch.float64
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (C, float((got - want).abs().max()))
        packed = ops.pack_fusion_params(sd, "blk", dtype, "cpu")
        for k, v in c["params"].items():
            assert packed[k].dtype == (dtype if k in ("g1", "be1", "g2", "be2") else torch.float32) and packed[k].is_contiguous(), k
            assert packed[k].shape == v.shape and torch.equal(packed[k].float(), v), k


@pytest.mark.parametrize("dtype", DTYPES)
def test_fusion_design_is_inside_the_bar_in_the_required_tier(dtype):
    """sample_err(base_alg) <= MARGIN * sample_err(base_ref), both > 0, for every required input kind at a one-workgroup shape, a
    several-workgroup shape and a per-item-reload shape - before the GPU test relies on it"""
    for kind in nm.FUSION_KINDS:
        if not nm.fusion_kind_required(kind):
            continue
        for (N, C, HW) in [(2, 64, 256), (1, 1280, 64), (2, 2056, 16)]:
            c = nm.fusion_case(N, C, HW, dtype, kind, seed=7, addend=(C == 1280))
            ref = nm.fusion_ref64(c)
            e_alg, e_ref = nm.sample_err(nm.fusion_base_alg(c), ref), nm.sample_err(nm.fusion_base_ref(c), ref)
            print(f"numerics: fusion design {kind} {dtype} C{C} HW{HW}: base_alg {e_alg:.3e} base_ref {e_ref:.3e}")
            assert 0 < e_alg <= nm.MARGIN * e_ref and e_ref > 0, (kind, C, HW, e_alg, e_ref)


def test_fusion_gpu_table_rows_have_a_design_inside_the_bars():
    """every row of tests/test_fusion_gpu.py's table under a million elements per net: the generator's postconditions hold, and in the
    required tier the DESIGN is inside the bar the GPU test applies to the kernel (base_alg <= MARGIN x base_ref) - a row whose
    yardsticks disagree by a draw of rounding luck (samples of 8 outputs) is found here, not on the GPU"""
    from tests import test_fusion_gpu as FG
    for row in FG.TABLE:
        if row["N"] * row["C"] * row["HW"] > 1_000_000:
            continue
        c = FG.make_case(row)
        ref = nm.fusion_ref64(c)
        e_alg, e_ref = nm.sample_err(nm.fusion_base_alg(c), ref), nm.sample_err(nm.fusion_base_ref(c), ref)
        assert e_alg > 0 and e_ref > 0, FG.row_id(row)
        if nm.fusion_kind_required(row["kind"]):
            assert e_alg <= nm.MARGIN * e_ref, (FG.row_id(row), e_alg, e_ref)


def _fusion_defect(c, defect, **kw):
    """(error of the planted defect, the bar of the same data, whether the old metric at 4e-3 passes the defect)"""
    ref = nm.fusion_ref64(c)
    e_alg, e_ref = nm.sample_err(nm.fusion_base_alg(c, **{k: v for k, v in kw.items() if k != "layout"}), ref), nm.sample_err(nm.fusion_base_ref(c), ref)
    y = nm.fusion_base_alg(c, defect=defect, **kw)
    e = nm.sample_err(y, ref)
    old = nm.old_metric(y, ref)
    old_passes = old < 4e-3                     # NaN compares false: a non-finite output fails the old metric as well
    print(f"numerics: fusion defect {defect} C{c['C']} HW{c['HW']} N{c['N']} {c['dtype']} {c['kind']}: defect {e:.3e}  bar {_bar(e_alg, e_ref):.3e}  "
          f"old metric {old:.3e} -> {'PASSES' if old_passes else 'fails'} at 4e-3")
    return e, _bar(e_alg, e_ref), old_passes


@pytest.mark.parametrize("dtype", DTYPES)
def test_fusion_planted_defects_are_outside_the_bar(dtype):
    same = lambda c, defect, **kw: torch.equal(nm.fusion_base_alg(c, defect=defect, **kw), nm.fusion_base_alg(c, **{k: v for k, v in kw.items() if k != "layout"}))
    # stale_column: invisible at every shape test_ops_gpu.py uses (its grids keep every thread on one column), visible at C = 2056, 4168
    from tests import helpers as H
    for C, S in OLD_FUSION_SHAPES + sorted(set(H.REF_FUSION_LEVELS)):
        nchunk, cb = nm.fusion_grids(C, S * S)
        assert nm.fusion_fixed_column(C, nchunk) and nm.fusion_fixed_column(C, cb), (C, S)
    for C, S in [(64, 16), (320, 8), (128, 8)]:
        assert same(nm.fusion_case(2, C, S * S, dtype, seed=C), "stale_column")
    for C, HW in [(2056, 16), (4168, 8)]:
        e, bar, _ = _fusion_defect(nm.fusion_case(2, C, HW, dtype, seed=C), "stale_column")
        assert e > bar, (C, e, bar)
    # partials_past_64: the emulation run with the grid forced, on as many pixels as give every thread one item
    for nchunk in (1, 40, 64):
        assert same(nm.fusion_case(1, 320, nchunk * 256 // 40 + 3, dtype, seed=nchunk), "partials_past_64", nchunk=nchunk)
    for nchunk in (80, 180, 255):
        e, bar, _ = _fusion_defect(nm.fusion_case(1, 320, nchunk * 256 // 40, dtype, seed=nchunk), "partials_past_64", nchunk=nchunk)
        assert e > bar, (nchunk, e, bar)
    c = nm.fusion_case(2, 64, 256, dtype, seed=5)
    for defect in ("scale_behind_bias", "count_c_hw"):
        e, bar, _ = _fusion_defect(c, defect)
        assert e > bar, (defect, e, bar)
    c1 = nm.fusion_case(2, 64, 256, dtype, scales=[1.0] * 6, seed=5)
    e, bar, _ = _fusion_defect(c1, "scale_behind_bias")                 # with all scales 1 there is nothing to misplace: another order of
    assert e <= bar                                                     # additions and no more
    # sample_stride_dense: visible only where the batch strides differ from HW C
    c = nm.fusion_case(3, 24, 35, dtype, seed=6)
    assert same(c, "sample_stride_dense", layout=nm.fusion_layout(c, dense=True))
    e, bar, _ = _fusion_defect(c, "sample_stride_dense", layout=nm.fusion_layout(c))
    assert e > bar
    c = nm.fusion_case(1, 24, 35, dtype, seed=6)
    assert same(c, "sample_stride_dense", layout=nm.fusion_layout(c))  # ... and only with more than one sample


@pytest.mark.parametrize("dtype", DTYPES)
def test_fusion_unclamped_variance(dtype):
    """A one-pass variance can come out negative only where the noise of E[z^2] - mean^2 exceeds the true variance, and it makes
    rsqrt(var + eps) a NaN only where that noise exceeds eps as well - where the result is no longer accurate in any case.  On `constant`
    (z == 0 exactly: s = ss = 0, var = 0 - 0) and on `gated_off` (var(b1) ~ 1e-2 >> 1e-7 of noise) the fp32 variance is never negative:
    the planted defect computes the same bits as the design there (asserted), so these two kinds do not guard the clamp.  What guards it
    is a sample that is constant up to 1e-5 of its value (b1 = 100 +- 1e-3 behind scales of 0): the design stays finite, the defect does
    not - the finiteness bar of the GPU sweep is the one that holds there."""
    for kind in ("constant", "gated_off"):
        c = nm.fusion_case(2, 64, 256, dtype, kind, seed=3)
        assert torch.equal(nm.fusion_base_alg(c, defect="variance_unclamped"), nm.fusion_base_alg(c))
        assert bool(torch.isfinite(nm.fusion_base_alg(c)).all())
    found = 0
    for seed in range(6):
        c = nm.nearly_constant_fusion_case(2, 64, 256, dtype, seed)
        good, bad = nm.fusion_base_alg(c), nm.fusion_base_alg(c, defect="variance_unclamped")
        assert bool(torch.isfinite(good).all()) and nm.finite_where_representable(good, nm.fusion_ref64(c), dtype)
        if not bool(torch.isfinite(bad).all()):
            found += 1
            assert not nm.finite_where_representable(bad, nm.fusion_ref64(c), dtype)
            print(f"numerics: fusion defect variance_unclamped seed {seed} {dtype}: not finite; old metric {nm.old_metric(bad, nm.fusion_ref64(c))} -> fails at 4e-3")
    assert found >= 1, "no seed drove the one-pass variance below -eps: the case no longer guards the clamp"


# ----------------------------------------------------------------------------------------------------------------
# the sampler step: coefficient tables applied as the kernels apply them, against the oracle's schedulers
# ----------------------------------------------------------------------------------------------------------------
# Worst per-step figure max|x - ref| / rms(ref) over every trajectory below, measured on the CPU (tests/NUMERICS.md, "Sampler step"):
# the fp32 table applied in fp64, and the whole recombination in fp32 (base_alg).  The assertions allow 4 x these, because the figures
# depend on the seed of eps; 1e-4 is where a figure would become a finding about the formulation.
UNIPC_TABLE_ERR, UNIPC_FP32_ERR = 1.4e-6, 3.2e-6
DDIM_TABLE_ERR, DDIM_FP32_ERR = 3.9e-7, 2.3e-6
SAMPLER_SHAPE = (2, 8, 8, 4)


def _unipc_trajectories(T, spacing, order, seed):
    from edgestyle_amd.schedulers import UniPCMultistepScheduler
    from oracle import sd15_oracle as O
    mine = UniPCMultistepScheduler(solver_order=order, timestep_spacing=spacing)
    orc = O.UniPC(solver_order=order, timestep_spacing=spacing)
    ts = orc.set_timesteps(T)
    assert mine.set_timesteps(T).tolist() == ts.tolist()
    table = mine.coef_table()
    assert table.shape == (T, 12) and table.dtype == torch.float32
    eps = nm.sampler_eps(T, SAMPLER_SHAPE, torch.float16, seed)
    x0 = torch.randn(*SAMPLER_SHAPE, generator=torch.Generator().manual_seed(seed)).float()
    t64 = nm.run_trajectory("unipc", table, eps, x0, SAMPLER_SHAPE[0], 1.0, False, torch.float64)
    t32 = nm.run_trajectory("unipc", table, eps, x0, SAMPLER_SHAPE[0], 1.0, False, torch.float32)
    x, e_table, e_alg = x0.double(), 0.0, 0.0
    for i in range(T):
        x = nm.unipc_oracle_step64(orc, eps[i], x)
        e_table, e_alg = max(e_table, nm.traj_err(t64[i][0], x)), max(e_alg, nm.traj_err(t32[i][0], x))
    # the oracle's own step (which hands an fp32 sample on) agrees with its fp64 form to fp32 rounding
    orc.set_timesteps(T)
    y = x0
    for i in range(T):
        y = orc.step(eps[i], int(ts[i]), y)
    assert nm.traj_err(y, x) < 1e-5
    return e_table, e_alg


def test_unipc_table_applied_as_the_kernel_applies_it_matches_the_oracle():
    """UniPCMultistepScheduler.coef_table() applied as es_cfg_unipc_step's linear recombination, in fp64 and in fp32, against
    oracle.UniPC fed the same eps over whole trajectories: T in {1, 2, 3, 4, 10, 50} (1 and 2: warm-up and lower_order_final meet),
    both spacings, solver_order 1 and 2, every step including the last"""
    worst_t, worst_a = 0.0, 0.0
    for T in (1, 2, 3, 4, 10, 50):
        for spacing in ("leading", "linspace"):
            for order in (1, 2):
                e_table, e_alg = _unipc_trajectories(T, spacing, order, seed=T)
                print(f"numerics: unipc T {T} {spacing} order {order}: fp32 table in fp64 {e_table:.3e}  all fp32 {e_alg:.3e}")
                assert e_table < 1e-4 and e_alg < 1e-4, (T, spacing, order, e_table, e_alg)
                worst_t, worst_a = max(worst_t, e_table), max(worst_a, e_alg)
    print(f"numerics: unipc worst: fp32 table {worst_t:.3e}  all fp32 {worst_a:.3e}")
    assert worst_t <= 4 * UNIPC_TABLE_ERR and worst_a <= 4 * UNIPC_FP32_ERR, (worst_t, worst_a)


def test_ddim_table_applied_as_the_kernel_applies_it_matches_the_oracle():
    from edgestyle_amd.schedulers import DDIMScheduler
    from oracle import sd15_oracle as O
    worst_t, worst_a = 0.0, 0.0
    for T in (1, 2, 10, 50):
        mine, orc = DDIMScheduler(), O.DDIM()
        ts = orc.set_timesteps(T)
        assert mine.set_timesteps(T).tolist() == ts.tolist()
        table = mine.coef_table()
        assert table.shape == (T, 4)
        eps = nm.sampler_eps(T, SAMPLER_SHAPE, torch.float16, seed=T)
        x0 = torch.randn(*SAMPLER_SHAPE, generator=torch.Generator().manual_seed(T)).float()
        t64 = nm.run_trajectory("ddim", table, eps, x0, SAMPLER_SHAPE[0], 1.0, False, torch.float64)
        t32 = nm.run_trajectory("ddim", table, eps, x0, SAMPLER_SHAPE[0], 1.0, False, torch.float32)
        orc.alphas_cumprod, orc.final_alpha_cumprod = orc.alphas_cumprod.double(), orc.alphas_cumprod[0].double()
        x = x0.double()
        for i in range(T):                      # every step, the last (alphas_cumprod[0]) included
            x = orc.step(eps[i].double(), int(ts[i]), x)
            e_table, e_alg = nm.traj_err(t64[i][0], x), nm.traj_err(t32[i][0], x)
            assert e_table < 1e-4 and e_alg < 1e-4, (T, i, e_table, e_alg)
            worst_t, worst_a = max(worst_t, e_table), max(worst_a, e_alg)
        print(f"numerics: ddim T {T}: worst so far fp32 table {worst_t:.3e}  all fp32 {worst_a:.3e}")
    assert worst_t <= 4 * DDIM_TABLE_ERR and worst_a <= 4 * DDIM_FP32_ERR, (worst_t, worst_a)


# ----------------------------------------------------------------------------------------------------------------
# csrc/norm.hip on every route (tests/test_norm_gpu.py)
# ----------------------------------------------------------------------------------------------------------------
def _norm_case(geo, kind, dtype, N=3, silu=False, seed=1):
    HW, C1, C2, G = geo
    return nm.norm_case(HW, C1, C2, G, N, kind, dtype, silu=silu, seed=seed), nm.gn_route(N, HW, C1 + C2, G)


def _norm_bars(c, route):
    """(ref64, base_alg's output, the larger of the two baselines' errors): a planted defect is OUTSIDE when its error exceeds MARGIN x that -
    it then misses both bars of the GPU test, whichever baseline is the better one"""
    ref = nm.gn_ref64(c)
    clean = nm.gn_base_alg(c, geom=route)
    return ref, clean, max(nm.row_err(clean, ref), nm.row_err(nm.gn_base_ref(c), ref))


@pytest.mark.parametrize("dtype", DTYPES)
def test_norm_gpu_table_rows_build_and_their_design_is_inside_the_bars(dtype):
    """every row of test_norm_gpu.GN_TABLE and LN_TABLE: the generator's postconditions hold, the library's route is the mirror's (the table
    itself is checked against the mirror when that module is imported), both baselines have an error and the design is inside 2 x base_ref"""
    from tests import test_norm_gpu as NG
    from edgestyle_amd import lib
    for row in NG.GN_TABLE:
        c = nm.norm_case(row["HW"], row["C1"], row["C2"], row["groups"], NG.N_ROW, row["kind"], dtype, silu=row["silu"], seed=row["seed"])
        route = lib.group_norm_route(NG.N_ROW, row["HW"], row["C1"], row["C2"], row["groups"])
        NG.assert_route(row, route)
        ref = nm.gn_ref64(c)
        e_alg, e_ref = nm.row_err(nm.gn_base_alg(c, geom=route), ref), nm.row_err(nm.gn_base_ref(c), ref)
        assert 0 < e_alg <= nm.MARGIN * e_ref, (NG.gn_id(row), e_alg, e_ref)
    for row in NG.LN_TABLE:
        assert lib.load().es_layer_norm_route(row["C"]) == NG.LN_VPL[row["C"]]
        c = nm.ln_plain_case(nm.token_rows(row["M"], row["C"], row["ratio"], dtype=dtype, seed=row["M"] + row["C"]), dtype, seed=row["C"])
        ref = nm.ln_plain_ref64(c)
        e_alg, e_ref = nm.row_err(nm.ln_plain_base_alg(c), ref), nm.row_err(nm.ln_plain_base_ref(c), ref)
        assert 0 < e_alg <= nm.MARGIN * e_ref, (NG.ln_id(row), e_alg, e_ref)


def test_norm_geometry_sums_agree_with_the_plain_chunking():
    """gn_base_alg with the route's geometry and without one (gn_chunked_stats, the form the older tests use) are the same algorithm with the
    levels cut differently: both inside the bar on the same case, and with a geometry of one slot per chunk the sums are the same numbers"""
    x = nm.group_maps(2, 320, 36, 32, 30, dtype=torch.float16, seed=3)
    c = nm.gn_case(x, 32, torch.float16, seed=3)
    route = nm.gn_route(2, 1296, 320, 32)
    assert (route["ppb"], route["nchunk"], route["ps"]) == (21, 62, 6)
    ref = nm.gn_ref64(c)
    a, b = nm.row_err(nm.gn_base_alg(c), ref), nm.row_err(nm.gn_base_alg(c, geom=route), ref)
    assert max(a, b) <= nm.MARGIN * min(a, b)
    one_slot = dict(route, ps=1)
    xg = x.reshape(2, 1296, 32, 10)
    S, SS, covered = nm.gn_geom_sums(xg, one_slot)
    assert covered == 62 * 21 and S.shape == (2, 62, 32)
    mean, rstd = nm.gn_chunked_stats(xg, c["eps"])
    m2 = S.double().sum(dim=1).float() / (10.0 * 1296.0)
    assert torch.allclose(m2, mean.reshape(2, 32), rtol=1e-6, atol=0)


GN_DEFECT_ROWS = {  # defect -> (rows it is OUTSIDE the bars at, rows it cannot be seen at: (geometry, kind, why))
    "pad_pixel_counted": ([((1225, 320, 0, 32), "ratio_30"), ((409, 320, 0, 32), "ratio_30"), ((17, 8, 16, 8), "ratio_30")],
                          [((408, 320, 0, 32), "ratio_30", "8 x 51 pixel slots hold exactly 408 pixels"), ((24, 2048, 0, 1), "ratio_30", "one slot, 24 pixels: no pad")]),
    "tail_pixels_dropped": ([((1225, 320, 0, 32), "ratio_0"), ((25, 2048, 0, 1), "ratio_30"), ((1087, 8, 16, 8), "ratio_0")],
                            [((300, 1040, 0, 8), "ratio_30", "one slot, chunks of 16 and a last one of 12 pixels: whole rounds of GN_UNROLL")]),
    "second_source_stride": ([((409, 104, 216, 32), "ratio_0"), ((17, 8, 16, 8), "ratio_30")],
                             [((409, 320, 0, 32), "ratio_0", "one source")]),
    "group_by_chunk": ([((17, 8, 16, 8), "ratio_30"), ((50, 120, 0, 40), "ratio_30"), ((1, 320, 0, 32), "ratio_30"), ((300, 1040, 0, 8), "ratio_30")],
                       [((9, 1280, 0, 32), "ratio_30", "40 channels per group: a 16-byte chunk never straddles two groups")]),
    "neighbour_sample": ([((1225, 320, 0, 32), "ratio_30"), ((409, 320, 0, 32), "ratio_30")],
                         [((408, 320, 0, 32), "ratio_30", "no pad pixels")]),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect", sorted(GN_DEFECT_ROWS))
def test_norm_planted_group_norm_defects(defect, dtype):
    """every planted defect of gn_base_alg (geometry form) misses the bars at the rows of the GPU table built for it - by a factor of 8 and
    more past MARGIN x the worse baseline, in both dtypes - and leaves base_alg's output untouched, bit for bit, where the geometry gives it
    nothing to act on (the reason is in GN_DEFECT_ROWS)"""
    from tests import test_norm_gpu as NG
    table = {(r["HW"], r["C1"], r["C2"], r["groups"]) for r in NG.GN_TABLE}
    outside, unseen = GN_DEFECT_ROWS[defect]
    for geo, kind in outside:
        assert geo in table
        c, route = _norm_case(geo, kind, dtype)
        ref, clean, bar = _norm_bars(c, route)
        e = nm.row_err(nm.gn_base_alg(c, geom=route, defect=defect), ref)
        assert e > 8 * nm.MARGIN * bar, (defect, geo, kind, e, bar)
    for geo, kind, why in unseen:
        assert geo in table
        c, route = _norm_case(geo, kind, dtype)
        assert torch.equal(nm.gn_base_alg(c, geom=route, defect=defect), nm.gn_base_alg(c, geom=route)), (defect, geo, why)


@pytest.mark.parametrize("dtype", DTYPES)
def test_norm_wrong_group_is_invisible_at_ratio_0(dtype):
    """group_by_chunk hands a channel the statistics of the NEIGHBOURING group.  At |mean| / std = 0 group_maps gives every group a mean
    near 0 and the same spread, so the neighbour's statistics are as good as the channel's own: inside the bars - which is why every
    geometry with cpg % 8 != 0 meets ratio_30 or dominant in the GPU table as well"""
    for geo in [(17, 8, 16, 8), (50, 120, 0, 40), (300, 1040, 0, 8)]:
        c, route = _norm_case(geo, "ratio_0", dtype)
        ref, clean, bar = _norm_bars(c, route)
        assert nm.row_err(nm.gn_base_alg(c, geom=route, defect="group_by_chunk"), ref) <= nm.MARGIN * bar


@pytest.mark.parametrize("dtype", DTYPES)
def test_norm_unclamped_variance(dtype):
    """variance_unclamped on the table's constant samples cannot be seen: the sample holds 87 / 32, k * 87 / 32 is exact in fp32 for every k that
    occurs, so the mean is exact and E[x^2] - mean^2 is the rounding of ONE fp32 quotient, |var| <= 2^-23 * 7.4 < 1e-6 < eps - var + eps > 0
    with or without the clamp, and x - mean = 0 wipes out what is left of the difference: inside the bars.  It is seen where the values are
    large: per (sample, group) one value in 1000 .. 2000 - the rounding of 10^6 * 2^-24 dwarfs eps, some groups come out negative and the
    unclamped form returns NaN where the clamped one stays finite."""
    for geo in [(1296, 320, 0, 32), (9, 1280, 0, 32), (49, 8000, 0, 32)]:
        c, route = _norm_case(geo, "constant", dtype)
        ref, clean, bar = _norm_bars(c, route)
        y = nm.gn_base_alg(c, geom=route, defect="variance_unclamped")
        assert bool(torch.isfinite(y).all()) and nm.row_err(y, ref) <= nm.MARGIN * bar
    HW, C, G, N = 1296, 320, 32, 3
    vals = nm.rnd(1000 + 1000 * torch.rand(N, 1, G, 1, generator=torch.Generator().manual_seed(5)), dtype)
    x = vals.expand(N, HW, G, C // G).reshape(N, HW, 1, C).clone()
    c = nm.gn_case(x, G, dtype, seed=1)
    c.update(C1=C, C2=0)
    route = nm.gn_route(N, HW, C, G)
    clean, bad = nm.gn_base_alg(c, geom=route), nm.gn_base_alg(c, geom=route, defect="variance_unclamped")
    assert bool(torch.isfinite(clean).all()) and not bool(torch.isfinite(bad).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_norm_planted_layer_norm_defects(dtype):
    """group_boundary_by_block: outside the bars on the grouped launch [3, 6, 1, 3] (rows 3, 9 and 10 take another set), nothing to act on with
    one set.  one_pass_variance: its relative error in the variance is about ratio^2 x 2^-24 x the chain length - at |mean| / std <= 30 under the
    rounding of the output in either dtype and at 300 still under bf16's (inside the bars, which is why GroupNorm may be built that way);
    in fp16 at 300 it is outside, and the GPU table carries two such rows.  On a row of ONE value both forms return the rounded beta."""
    rows = [3, 6, 1, 3]
    for C in (8, 520, 4096):
        c = nm.ln_plain_case(nm.token_rows(13, C, 30, dtype=dtype, seed=C), dtype, ngroups=4, seed=C)
        ref = nm.ln_plain_ref64(c, rows)
        bar = max(nm.row_err(nm.ln_plain_base_alg(c, rows), ref), nm.row_err(nm.ln_plain_base_ref(c, rows), ref))
        assert nm.row_err(nm.ln_plain_base_alg(c, rows, defect="group_boundary_by_block"), ref) > 8 * nm.MARGIN * bar
        one = nm.ln_plain_case(c["x"], dtype, seed=C)
        assert torch.equal(nm.ln_plain_base_alg(one, defect="group_boundary_by_block"), nm.ln_plain_base_alg(one))
    for C, M in [(1024, 5), (2056, 4)]:
        for ratio in (0, 30, 300):
            c = nm.ln_plain_case(nm.token_rows(M, C, ratio, dtype=dtype, seed=M + C), dtype, seed=C)
            ref = nm.ln_plain_ref64(c)
            bar = max(nm.row_err(nm.ln_plain_base_alg(c), ref), nm.row_err(nm.ln_plain_base_ref(c), ref))
            e = nm.row_err(nm.ln_plain_base_alg(c, defect="one_pass_variance"), ref)
            if ratio == 300 and dtype == torch.float16:
                assert e > nm.MARGIN * bar, (C, ratio, e, bar)
            else:
                assert e <= nm.MARGIN * bar, (C, ratio, e, bar)
    x = nm.token_rows(5, 520, 0, dtype=dtype, seed=2)
    x[1] = nm.NORM_CONSTANT
    x[3] = 0.0
    c = nm.ln_plain_case(x, dtype, seed=2)
    for defect in (None, "one_pass_variance"):
        y = nm.ln_plain_base_alg(c, defect=defect)
        assert torch.equal(y[1], nm.rnd(c["beta"][0], dtype)) and torch.equal(y[3], nm.rnd(c["beta"][0], dtype))


# ----------------------------------------------------------------------------------------------------------------
# es_linear_xs: the table of tests/test_linear_xs_gpu.py on the CPU, the planted defects, the counted waits
# ----------------------------------------------------------------------------------------------------------------
def _xs_row_case(r, dtype):
    kw = dict(hw=r["hw"], G=r["G"], N=r["N"]) if r["kind"] == "gn" else {}
    return nm.xs_case(r["M"], r["K"], r["lines"], r["kind"], dtype, seed=r["seed"], counts=r["counts"], ratio=r["ratio"], **kw)


def _xs_verdict(c, y, ref, alg8, e_ref):
    """what tests/test_linear_xs_gpu.py would hold against an output y of case c (a y with more rows than M: stored through a guarded
    buffer, as the GPU test launches): the list of bars missed"""
    M, cstore, dt = c["M"], c["cstore"], c["dtype"]
    bad = []
    big, view = nm.xs_out_guarded(M, cstore, dt)
    rows = y.shape[0]
    big[nm.XS_GUARD_ROWS:nm.XS_GUARD_ROWS + rows, :cstore] = y.to(dt)
    if not nm.xs_guards_intact(big, M, cstore):
        bad.append("guard")
    y = view.float()
    if bool(torch.isnan(y).any()):
        bad.append("nan in the payload")
    e, e_alg = nm.row_err(y, ref), nm.row_err(alg8, ref)
    if not e <= nm.MARGIN * e_alg:
        bad.append(f"base_alg bar: {e:.3e} > 2 x {e_alg:.3e}")
    if not e <= nm.MARGIN * e_ref:
        bad.append(f"base_ref bar: {e:.3e} > 2 x {e_ref:.3e}")
    if nm.xs_rounds_once(c["kind"]):
        base = dict(alg8=alg8, alg32=nm.xs_base_alg(c, 32), torch32=nm.xs_base_alg(c, None))
        bar = nm.misrounded_bar([nm.misrounded(v, ref, dt, count=True) for v in base.values()])
        n = nm.misrounded(y, ref, dt, count=True)
        if n > bar:
            bad.append(f"misrounded: {n} > {bar}")
    if c["kind"] == "res":
        bar = nm.misrounded_bar([nm.differs(nm.xs_base_alg(c, k), alg8, count=True) for k in (32, None)])
        n = nm.differs(y, alg8, count=True)
        if n > bar:
            bad.append(f"differs from base_alg: {n} > {bar}")
    return bad


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_xs_gpu_table_rows_build_and_their_design_is_inside_the_bars(dtype):
    """every row of the GPU table builds its case (the generators assert their postconditions, every bias is clear of the rounding
    boundaries) and the design - xs_base_alg with chains of 8 - passes every check the GPU test makes of the kernel.  Every other row per
    dtype (the even rows in fp16, the odd ones in bf16: each row is walked once here; on the GPU every row runs in both)"""
    from tests import test_linear_xs_gpu as X
    for r in X.TABLE[(0 if dtype == torch.float16 else 1)::2]:
        c = _xs_row_case(r, dtype)
        ref = nm.xs_ref64(c)
        assert ref.shape == (r["M"], 64 * r["lines"])
        alg8 = nm.xs_base_alg(c, 8)
        bad = _xs_verdict(c, alg8, ref, alg8, nm.row_err(nm.xs_base_ref(c), ref))
        assert not bad, (X.row_id(r), bad)


def _xs_smallest(pred):
    from tests import test_linear_xs_gpu as X
    rows = [r for r in X.TABLE if pred(r)]
    return min(rows, key=lambda r: (r["M"] * r["lines"], r["K"], r["pp"]))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("defect", nm.XS_DEFECTS)
def test_xs_planted_defects_land_outside_the_bars(defect, dtype):
    """each planted defect of nm.xs_base_alg, at the smallest row of the GPU table where it applies, misses a check the GPU test makes -
    while the design passes all of them on the same row"""
    from tests import test_linear_xs_gpu as X
    P = lambda r: nm.xs_geometry(r["K"], r["kind"])[2]
    pred = {
        "stale_stage": lambda r: X.row_split(r)[1] >= 4,                               # a fourth stage in the first slice
        "row_dropped": lambda r: True,
        "short_slice_line_dropped": lambda r: X.row_split(r)[0] > 1 and X.row_split(r)[2] < X.row_split(r)[1],
        "residual_row_shift": lambda r: r["kind"] == "res",
        "geglu_halves_swapped": lambda r: r["kind"].startswith("geglu"),
        "ln_zero_row_nan": lambda r: r["kind"] in ("ln", "geglu_ln"),
    }[defect]
    r = _xs_smallest(pred)
    c = _xs_row_case(r, dtype)
    ref, alg8 = nm.xs_ref64(c), nm.xs_base_alg(c, 8)
    e_ref = nm.row_err(nm.xs_base_ref(c), ref)
    assert not _xs_verdict(c, alg8, ref, alg8, e_ref), X.row_id(r)
    bad = _xs_verdict(c, nm.xs_base_alg(c, 8, defect=defect), ref, alg8, e_ref)
    print(f"xs defect {defect} at {X.row_id(r)}: {bad}")
    assert bad, (defect, X.row_id(r))
    want = {"row_dropped": "nan in the payload", "short_slice_line_dropped": "nan in the payload", "ln_zero_row_nan": "guard"}.get(defect)
    assert want is None or want in bad


def test_xs_stale_stage_is_seen_in_every_stage_of_every_form():
    """the stale stage (a wait one group too loose) at EVERY stage index >= 3 of one long row per kind: always outside the base_alg bar"""
    for K, kind in ((320, "plain"), (320, "geglu_ln"), (640, "ln"), (640, "geglu"), (320, "res"), (640, "gn")):
        kw = dict(hw=256, G=32, N=1) if kind == "gn" else {}
        c = nm.xs_case(256 if kind == "gn" else 17, K, 3, kind, torch.float16, seed=5, ratio=30, **kw)
        ref, alg8 = nm.xs_ref64(c), nm.xs_base_alg(c, 8)
        e_alg = nm.row_err(alg8, ref)
        outw = nm.xs_geometry(K, kind)[1]
        for stage in range(3, 3 * 64 // outw):
            e = nm.row_err(nm.xs_base_alg(c, 8, defect="stale_stage", stage=stage), ref)
            assert e > 100 * e_alg, (K, kind, stage, e, e_alg)


def _xs_source():
    import os
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "edgestyle_amd", "csrc", "linear_xs.hip")).read()


def test_xs_wait_model_is_the_source():
    """the walk of nm.xs_wave_walk is tied to csrc/linear_xs.hip by its TEXT: the ordered list of wait_vm<...> arguments, NDMA, ST, RS and
    the static_assert that keeps a residual at P = 1.  An edit to any of them fails here until the model is updated with it."""
    import re
    src = _xs_source()
    args = [a.strip() for a in re.findall(r"wait_vm<([^>]*)>\(\)", src)]
    assert args == [a for _, a in nm.XS_WAIT_SITES], args
    assert int(re.search(r"constexpr int NDMA = (\d+);", src).group(1)) == nm.XS_NDMA
    assert int(re.search(r"constexpr int ST = (\d+);", src).group(1)) == nm.XS_ST
    assert int(re.search(r"constexpr int RS = RES \? (\d+) : 0;", src).group(1)) == nm.XS_RS
    assert "static_assert(!RES || (P == 1 && !GEGLU && !LN)" in src and "constexpr int XS_STAGES = 3;" in src
    # five weight pieces and one bias load per wave per stage; four residual loads, four stores per line
    assert src.count("for (int i = 0; i < 5; ++i)") == 1 and src.count("__builtin_amdgcn_raw_ptr_buffer_load_lds(") == 2
    assert src.count("for (int i = 0; i < 4; ++i)") == 2
    # the conditions under which each count is chosen, as the walk spells them
    for text in ("} else if (ci + 1 >= nch) {", "} else if (ci < (late ? 3 : 2)) {", "if ((cio & 3) < 2) wait_vm<NDMA + 4>(); else wait_vm<NDMA>();",
                 "if (PP || !late) { if (ci + 2 < nch) wait_vm<NDMA>(); else wait_vm<0>(); }",
                 "else { if (ci >= 1 && ci + 3 < nch) wait_vm<NDMA + 4 + 4 + NDMA>(); else wait_vm<0>(); }",
                 "if (nch > 1) wait_vm<NDMA>(); else wait_vm<0>();", "if (late) __builtin_amdgcn_s_barrier();",
                 "if (t + 2 >= nch && t == 0) wait_vm<RS>();", "else if (line_done(t - 1)) wait_vm<ST + RS>(); else wait_vm<RS>();",
                 "if (!late || t + 1 < nch) __builtin_amdgcn_s_barrier();",
                 "if (t + 2 < nch) { if (line_done(t)) wait_vm<NDMA + ST>(); else wait_vm<NDMA>(); }",
                 "else { if (line_done(t)) wait_vm<ST>(); else wait_vm<0>(); }"):
        assert text in src, text


def test_xs_counted_waits_are_safe_and_every_loosened_count_is_caught():
    """One wave's vector-memory queue walked through both forms, both wave groups, every P, with and without a residual, nch = P .. 12:
    whenever a wave arrives at a barrier that opens compute(s) for any wave its own DMAs of stage s are retired, every residual load
    is retired in its epilogue, both groups pass the same number of barriers, and a ring slot is refilled only behind the barrier that
    follows its last readers.  Then every wait of the source, one at a time, is loosened by one store group (4) and by one DMA group (6):
    each such kernel is caught in at least one program - also when only the early or only the late waves run the loose count."""
    walked = 0
    for pp, P, res in nm.xs_wait_programs():
        for nch in range(P, 13, P):
            assert not nm.xs_wait_audit(pp, P, res, nch), (pp, P, res, nch, nm.xs_wait_audit(pp, P, res, nch))
            a, b = nm.xs_wave_walk(pp, False, P, res, nch), nm.xs_wave_walk(pp, True, P, res, nch)
            assert a["barriers"] == b["barriers"] == (2 * nch if pp else nch)
            assert sorted(a["compute"]) == sorted(b["compute"]) == list(range(nch)) == sorted(a["issue"])
            walked += 2
    assert walked == 2 * sum(12 // P for _, P, _ in nm.xs_wait_programs())
    for site, _ in nm.XS_WAIT_SITES:
        for extra in (nm.XS_ST, nm.XS_NDMA):
            caught = [(pp, P, res, nch) for pp, P, res in nm.xs_wait_programs() for nch in range(P, 13, P) if nm.xs_wait_audit(pp, P, res, nch, {site: extra})]
            assert caught, f"wait {site} loosened by {extra} passes the audit"
    # a count one group TIGHTER is safe (the audit is no equality test of the counts)
    assert not nm.xs_wait_audit(False, 1, False, 7, {"top_p1": -4}) and not nm.xs_wait_audit(True, 2, False, 8, {"pp_early_store": -4})
    # the steady-state counts are exact where the issue says so: one more operation than they allow is already too loose
    assert nm.xs_wait_audit(False, 1, False, 7, {"top_p1": 1}) and nm.xs_wait_audit(True, 1, True, 7, {"pp_late_store": 1})

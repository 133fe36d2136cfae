"""Seeded noise at the C ABI, the part that needs no GPU (csrc/rng.hip): Philox4x32-10 against the Random123 known answers,
torch's grid and offset arithmetic, es_randn_host - the host build of the code the kernel runs - against a numpy restatement
written here (Philox in Python integers, u and v in np.float32 arithmetic, the transcendental part in float64), the NHWC
scatter, scale and rounding, and the argument checks of every new entry point."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from edgestyle_amd import lib as L

M32 = 0xFFFFFFFF
FAKE = 0x1000          # never dereferenced: every call below fails its checks first


def _philox_py(ctr, key):
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def _philox_lib(ctr, key):
    out = (C.c_uint32 * 4)()
    assert L.load().es_philox4x32_10((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out) == 0
    return list(out)


@pytest.mark.parametrize("ctr, key, want", [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([M32] * 4, [M32] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    assert _philox_py(ctr, key) == want             # the restatement below stands on the same answers
    assert _philox_lib(ctr, key) == want


@pytest.mark.parametrize("numel, blocks, advance", [(1, 1, 4), (1024, 4, 4), (1025, 5, 4), (2097152, 2048, 4), (2097153, 2048, 8)])
def test_grid_and_advance_with_cap_2048(numel, blocks, advance):
    lib = L.load()
    assert lib.es_philox_blocks(numel, 2048) == blocks
    assert lib.es_philox_advance(numel, blocks) == advance


def _randn_ref(numel, seed, offset, blocks):
    """float64 reference of the draw, laid out as torch's grid-stride kernel lays it out"""
    T = 256 * blocks
    key = [seed & M32, (seed >> 32) & M32]
    c32, c2pi = np.float32(2.3283064e-10), np.float32(1.46291807e-09)
    out = np.empty(numel, dtype=np.float64)
    words = {}
    for li in range(numel):
        i, ii, t = li // (4 * T), (li % (4 * T)) // T, li % T
        if (i, t) not in words:
            n = offset // 4 + i
            words[(i, t)] = _philox_py([n & M32, (n >> 32) & M32, t & M32, t >> 32], key)
        x, y = words[(i, t)][2 * (ii // 2):2 * (ii // 2) + 2]
        u = c32 + np.float32(x) * c32
        v = c2pi + np.float32(y) * c2pi
        assert u.dtype == np.float32 and v.dtype == np.float32
        s = math.sqrt(-2.0 * math.log(float(u)))
        out[li] = (math.cos(float(v)) if ii % 2 else math.sin(float(v))) * s
    return out


def _desc(numel, seed=0, offset=0, blocks=1, scale=1.0, round_dtype=L.ES_F32, perm=(0, 0, 0, 0)):
    return L.RandnDesc(seed=seed, offset=offset, numel=numel, blocks=blocks, scale=scale, round_dtype=round_dtype,
                       N=perm[0], C=perm[1], HW=perm[2], Cstride=perm[3])


def _host(numel, out_len=None, fill=None, **kw):
    out = np.full(out_len or numel, np.nan if fill is None else fill, dtype=np.float32)
    d = _desc(numel, **kw)
    rc = L.load().es_randn_host(out.ctypes.data_as(C.c_void_p), C.byref(d))
    assert rc == 0, L.load().es_last_error()
    return out


T2 = 256 * 2
_REF = {}


def _ref(numel, seed, offset):
    k = (numel, seed, offset)
    if k not in _REF:
        _REF[k] = _randn_ref(numel, seed, offset, 2)
    return _REF[k]


@pytest.mark.parametrize("seed", [0, 42, 2 ** 63 + 5])
@pytest.mark.parametrize("offset", [0, 4000])
@pytest.mark.parametrize("numel", [1, 3, 4, 257, 1025, 4 * T2 + 5])
def test_randn_host_equals_the_numpy_restatement_within_4_ulp(numel, offset, seed):
    """three functions, each correctly rounded to about 1 ulp, in sequence; |z| <= 6.66.  A misplaced element is wrong by
    O(1), so the bar proves the layout too (4 * T + 5 at blocks = 2 runs the second grid-stride iteration)."""
    got = _host(numel, seed=seed, offset=offset, blocks=2)
    ref = _ref(numel, seed, offset)
    bar = 4 * np.spacing(np.maximum(np.abs(ref), 1.0).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref)
    print("max error / bar:", float((err / bar).max()))
    assert np.all(np.isfinite(got)) and np.all(err <= bar), int((err > bar).sum())
    assert np.abs(ref).max() <= 6.66


def test_randn_host_depends_on_blocks_as_torchs_layout_does():
    a, b = _host(2000, seed=42, blocks=2), _host(2000, seed=42, blocks=8)
    assert np.array_equal(a[:512], b[:512]) and not np.array_equal(a[512:1024], b[512:1024])
    # (element 512 at blocks = 2 is thread 0's second normal; at blocks = 8, T = 2048 > 2000, every element is some thread's first)


def test_nhwc_permutation_leaves_the_pad_untouched():
    N, Cc, HW, Cs = 2, 4, 35, 7
    flat = _host(N * Cc * HW, seed=9, offset=8, blocks=1)
    got = _host(N * Cc * HW, out_len=N * HW * Cs, fill=-77.0, seed=9, offset=8, blocks=1, perm=(N, Cc, HW, Cs)).reshape(N, HW, Cs)
    assert np.array_equal(got[:, :, :Cc], flat.reshape(N, Cc, HW).transpose(0, 2, 1))
    assert np.all(got[:, :, Cc:] == -77.0)
    dense = _host(N * Cc * HW, seed=9, offset=8, blocks=1, perm=(N, Cc, HW, Cc)).reshape(N, HW, Cc)
    assert np.array_equal(dense, got[:, :, :Cc])


@pytest.mark.parametrize("dtype, code", [(torch.float16, L.ES_F16), (torch.bfloat16, L.ES_BF16)])
def test_scale_and_round_dtype_equal_torchs_cast_of_the_fp32_draw(dtype, code):
    n = 4 * T2 + 5
    z = torch.from_numpy(_host(n, seed=42, blocks=2))
    got = torch.from_numpy(_host(n, seed=42, blocks=2, round_dtype=code))
    assert torch.equal(got, z.to(dtype).float())
    scaled = torch.from_numpy(_host(n, seed=42, blocks=2, round_dtype=code, scale=1.7))
    assert torch.equal(scaled, z.to(dtype).float() * 1.7)
    assert torch.equal(torch.from_numpy(_host(n, seed=42, blocks=2, scale=14.6146)), z * 14.6146)


def test_argument_checks_name_the_argument():
    lib = L.load()
    P = C.c_void_p

    def err():
        return lib.es_last_error().decode()
    for name, call in (("es_randn", lambda o, d: lib.es_randn(o, d, None)), ("es_randn_host", lambda o, d: lib.es_randn_host(o, d))):
        def bad(text, out=P(FAKE), **kw):
            d = _desc(**{"numel": 8, **kw})
            assert call(out, C.byref(d)) == -1 and text in err() and name in err(), err()
        assert call(P(FAKE), None) == -1 and "null pointer (descriptor)" in err()
        bad("null pointer (out)", out=None)
        bad("numel < 1", numel=0)
        bad("blocks < 0", blocks=-1)
        bad("round_dtype", round_dtype=3)
        bad("round_dtype", round_dtype=-1)
        bad("offset is not a multiple of 4", offset=6)
        bad("N*C*HW != numel", perm=(2, 2, 3, 2))
        bad("N*C*HW != numel", perm=(1, 2, 2 ** 62, 2))
        bad("Cstride < C", perm=(1, 4, 2, 3))
        bad("permutation", perm=(0, 4, 2, 4))
    d = _desc(8, blocks=0)
    assert lib.es_randn_host(P(FAKE), C.byref(d)) == -1 and "blocks must be given" in err()
    w = (C.c_uint32 * 4)()
    assert lib.es_philox4x32_10(None, w, w) == -1 and "null pointer" in err()
    assert lib.es_philox_blocks(0, 8) == -1 and "numel < 1" in err()
    assert lib.es_philox_blocks(8, 0) == -1 and "block_cap < 1" in err()
    assert lib.es_philox_advance(0, 1) == -1 and "numel < 1" in err()
    assert lib.es_philox_advance(8, 0) == -1 and "blocks < 1" in err()
    assert lib.es_philox_block_cap(-1) == -1 and "device < 0" in err()
    gens = (L.Philox * 3)()
    assert lib.es_ctx_draw_latents(None, gens, 1, 1.0, L.ES_F32, P(FAKE), None) == -1 and "null pointer" in err()
    assert lib.es_ctx_draw_cond_noise(None, gens, L.ES_F32, None) == -1 and "null pointer" in err()
    ctx = C.c_void_p()
    assert lib.es_ctx_create(0, C.byref(ctx)) == 0
    try:
        assert lib.es_ctx_draw_latents(ctx, None, 1, 1.0, L.ES_F32, P(FAKE), None) == -1 and "null pointer" in err()
        assert lib.es_ctx_draw_latents(ctx, gens, 1, 1.0, L.ES_F32, None, None) == -1 and "null pointer" in err()
        assert lib.es_ctx_draw_latents(ctx, gens, 1, 1.0, L.ES_F32, P(FAKE), None) == -1 and "geometry" in err()
        assert lib.es_ctx_draw_cond_noise(ctx, None, L.ES_F32, None) == -1 and "null pointer" in err()
        geo = L.CtxGeometry(B=2, cfg=1, h=8, w=8, latent_channels=4, latent_pad=8, n_conds=6, n_steps=2, dtype=L.ES_F16, guess_mode=0)
        assert lib.es_ctx_set_geometry(ctx, C.byref(geo)) == 0
        for n in (0, 3, -1):
            assert lib.es_ctx_draw_latents(ctx, gens, n, 1.0, L.ES_F32, P(FAKE), None) == -1 and "n_gens" in err()
        gens[1].offset = 2
        assert lib.es_ctx_draw_latents(ctx, gens, 2, 1.0, L.ES_F32, P(FAKE), None) == -1 and "multiple of 4" in err()
        gens[1].offset = 0
        assert lib.es_ctx_draw_latents(ctx, gens, 2, 1.0, 7, P(FAKE), None) == -1 and "round_dtype" in err()
        assert gens[0].offset == 0 and gens[1].offset == 0
    finally:
        lib.es_ctx_destroy(ctx)


def test_noise_calls_are_never_part_of_a_plan():
    lib = L.load()
    P = C.c_void_p
    plan = C.c_void_p(lib.es_plan_create())
    assert lib.es_plan_begin_record(plan) == 0
    try:
        was = lib.es_plan_set_dry(1)

        def recording():
            return b"plan is recording" in lib.es_last_error()
        w, k = (C.c_uint32 * 4)(), (C.c_uint32 * 2)()
        d = _desc(8)
        buf = np.zeros(8, dtype=np.float32)
        assert lib.es_philox4x32_10(w, k, w) == -1 and recording()
        assert lib.es_philox_block_cap(0) == -1 and recording()
        assert lib.es_philox_blocks(8, 8) == -1 and recording()
        assert lib.es_philox_advance(8, 1) == -1 and recording()
        assert lib.es_randn(P(FAKE), C.byref(d), None) == -1 and recording()
        assert lib.es_randn_host(buf.ctypes.data_as(P), C.byref(d)) == -1 and recording() and not buf.any()
        ctx = C.c_void_p()
        assert lib.es_ctx_create(0, C.byref(ctx)) == 0
        gens = (L.Philox * 1)()
        assert lib.es_ctx_draw_latents(ctx, gens, 1, 1.0, L.ES_F32, P(FAKE), None) == -1 and recording()
        assert lib.es_ctx_draw_cond_noise(ctx, gens, L.ES_F32, None) == -1 and recording()
        lib.es_ctx_destroy(ctx)
        assert lib.es_plan_size(plan) == 0
    finally:
        lib.es_plan_set_dry(was)
        assert lib.es_plan_end_record(plan) == 0
        lib.es_plan_destroy(plan)


def test_abi_version_is_unchanged():
    assert L.load().es_abi_version() == 7 and L.ABI_VERSION == 7


def test_pipeline_and_service_refuse_an_unknown_noise_source():
    from edgestyle_amd.serve import TryOnService
    with pytest.raises(ValueError, match="noise_source"):
        TryOnService(lambda **kw: None, noise_source="cuda")
    svc = TryOnService(lambda **kw: None)
    try:
        assert svc.noise_source == "host"
    finally:
        svc.shutdown()

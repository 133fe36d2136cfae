"""Seeded noise at the C ABI on the GPU (csrc/rng.hip): es_randn against live torch.randn on the same device bit for bit
(every size at which torch's grid changes, up to the block cap and the second grid-stride iteration), continuity of the
generator's offset, half and bfloat16 draws, the context-level draws, the pipeline with noise_source="device" against the same
pipeline fed torch's own draws, and the compiled C++ host with --seed (examples/image_host.cpp).  Every comparison is an equality."""
import ctypes as C

import numpy as np
import pytest
import torch

from edgestyle_amd import config as Cfg, lib as L, ops
from tests.helpers import make_weights, quantize

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = -77.0


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _gen(seed):
    return torch.Generator(DEV).manual_seed(seed)


def _cap():
    return L.load().es_philox_block_cap(torch.cuda.current_device())


def test_block_cap_is_the_devices():
    p = torch.cuda.get_device_properties(torch.cuda.current_device())
    assert _cap() == p.multi_processor_count * (p.max_threads_per_multi_processor // 256) and _cap() >= 1


@pytest.mark.parametrize("seed", [42, 2 ** 63 + 5])
@pytest.mark.parametrize("n", [1, 3, 4, 255, 256, 257, 1023, 1024, 1025, "cap"])
def test_randn_equals_torch_randn_bitwise(n, seed):
    """"cap": 4 * 256 * cap + 5 elements, the smallest draw that reaches the block cap and the second grid-stride iteration"""
    if n == "cap":
        n = 4 * 256 * _cap() + 5
    g = _gen(seed)
    want = torch.randn(n, device=DEV, generator=g)
    got, off = ops.randn((n,), seed, 0)
    torch.cuda.synchronize()
    bad = _bits(got) != _bits(want)
    if bool(bad.any()):
        idx = bad.nonzero().flatten()
        print("differing elements:", int(idx.numel()), "of", n, "first:", idx[:8].tolist(),
              "max |diff|:", float((got - want).abs().max()))
    assert not bool(bad.any())
    assert off == g.get_offset()


def test_two_successive_draws_continue_like_torchs_generator():
    lib = L.load()
    g = _gen(1234)
    w1 = torch.randn(1000, device=DEV, generator=g)
    mid = g.get_offset()
    w2 = torch.randn(5000, device=DEV, generator=g)
    a, off1 = ops.randn((1000,), 1234, 0)
    assert off1 == mid == lib.es_philox_advance(1000, lib.es_philox_blocks(1000, _cap()))
    b, off2 = ops.randn((5000,), 1234, off1)
    assert off2 == g.get_offset() == off1 + lib.es_philox_advance(5000, lib.es_philox_blocks(5000, _cap()))
    assert _same(a, w1) and _same(b, w2)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_draws_equal_torchs_draw_in_that_dtype(dtype):
    for n in (5, 1025, 70001):
        want = torch.randn(n, device=DEV, generator=_gen(7), dtype=dtype).float()
        got, _ = ops.randn((n,), 7, 0, round_dtype=dtype)
        assert _same(got, want), n
    got, _ = ops.randn((1025,), 7, 0, round_dtype=dtype, scale=14.6146)
    assert _same(got, torch.randn(1025, device=DEV, generator=_gen(7), dtype=dtype).float() * 14.6146)


def test_randn_nhwc_with_a_padded_stride_and_an_explicit_grid():
    want = torch.randn((2, 4, 5, 7), device=DEV, generator=_gen(3))
    out = torch.full((2, 5, 7, 6), POISON, device=DEV)
    got, _ = ops.randn((2, 4, 5, 7), 3, 0, nhwc=6, out=out)
    assert got is out and _same(out[..., :4], want.permute(0, 2, 3, 1)) and bool((out[..., 4:] == POISON).all())
    dense, _ = ops.randn((2, 4, 5, 7), 3, 0, nhwc=True)
    assert _same(dense, want.permute(0, 2, 3, 1))
    # a grid that is not this device's: the layout of a device with a block cap of 2 (the CPU tests' reference layout)
    small, off = ops.randn((4 * 512 + 5,), 3, 0, blocks=2)
    assert off == 8 and _same(small[:512], torch.randn(512, device=DEV, generator=_gen(3)))


def test_randn_is_capturable():
    out = torch.zeros(3000, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.randn((3000,), 11, 0, out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.randn((3000,), 11, 0, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, torch.randn(3000, device=DEV, generator=_gen(11)))


# ---------------------------------------------------------------------------------------------------------------
# context level: a bare context (geometry and slots only - the draws run no plan)
def _ctx(B=2, h=8, w=8, Lc=4):
    lib = L.load()
    ctx = C.c_void_p()
    assert lib.es_ctx_create(torch.cuda.current_device(), C.byref(ctx)) == 0
    geo = L.CtxGeometry(B=B, cfg=1, h=h, w=w, latent_channels=Lc, latent_pad=8, n_conds=6, n_steps=2, dtype=L.ES_F16, guess_mode=0)
    assert lib.es_ctx_set_geometry(ctx, C.byref(geo)) == 0
    return lib, ctx


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_ctx_draw_latents_one_generator_and_a_list_of_generators():
    lib, ctx = _ctx()
    try:
        sigma = 14.6146
        out = torch.full((3, 8, 8, 4), POISON, device=DEV)               # one image more than the context's: must stay poisoned
        g = _gen(42)
        want = torch.randn((2, 4, 8, 8), device=DEV, generator=g) * sigma
        gens = (L.Philox * 1)(L.Philox(42, 0))
        L.check(lib.es_ctx_draw_latents(ctx, gens, 1, sigma, L.ES_F32, C.c_void_p(out.data_ptr()), _stream()), "es_ctx_draw_latents")
        torch.cuda.synchronize()
        assert _same(out[:2], want.permute(0, 2, 3, 1)) and bool((out[2] == POISON).all())
        assert gens[0].offset == g.get_offset() and gens[0].seed == 42
        # the list-of-generators case: one [1, L, h, w] draw per image; the second generator is already part-way through its stream
        out.fill_(POISON)
        g0, g1 = _gen(5), _gen(6)
        torch.randn(3000, device=DEV, generator=g1)
        start1 = g1.get_offset()
        want = torch.cat([torch.randn((1, 4, 8, 8), device=DEV, generator=g0), torch.randn((1, 4, 8, 8), device=DEV, generator=g1)])
        gens = (L.Philox * 2)(L.Philox(5, 0), L.Philox(6, start1))
        L.check(lib.es_ctx_draw_latents(ctx, gens, 2, 1.0, L.ES_F32, C.c_void_p(out.data_ptr()), _stream()), "es_ctx_draw_latents")
        torch.cuda.synchronize()
        assert _same(out[:2], want.permute(0, 2, 3, 1)) and bool((out[2] == POISON).all())
        assert gens[0].offset == g0.get_offset() and gens[1].offset == g1.get_offset()
        # a half draw, as a pipeline in fp16 would make it
        gens = (L.Philox * 1)(L.Philox(42, 0))
        L.check(lib.es_ctx_draw_latents(ctx, gens, 1, 1.0, L.ES_F16, C.c_void_p(out.data_ptr()), _stream()), "es_ctx_draw_latents")
        torch.cuda.synchronize()
        assert _same(out[:2], torch.randn((2, 4, 8, 8), device=DEV, generator=_gen(42), dtype=torch.float16).float().permute(0, 2, 3, 1))
    finally:
        lib.es_ctx_destroy(ctx)


def test_ctx_draw_cond_noise_fills_exactly_the_bound_slots_in_net_order():
    lib, ctx = _ctx()
    try:
        arena = torch.full((4096,), POISON, device=DEV)
        n1, n4 = 4 * 4 * 8 * 8, 4 * 4 * 8 * 8 + 0                        # [N = 4, L, h, w] each
        at = {1: (100, n1), 4: (2000, n4)}                               # net -> (first element, elements) inside the arena
        for net, (a, n) in at.items():
            assert lib.es_ctx_bind(ctx, L.BUF_COND_NOISE0 + net, C.c_void_p(arena.data_ptr() + 4 * a), 4 * n) == 0
        g = _gen(7)
        want = {net: torch.randn((4, 4, 8, 8), device=DEV, generator=g) for net in (1, 4)}      # net order, one advancing generator
        gen = L.Philox(7, 0)
        L.check(lib.es_ctx_draw_cond_noise(ctx, C.byref(gen), L.ES_F32, _stream()), "es_ctx_draw_cond_noise")
        torch.cuda.synchronize()
        assert gen.offset == g.get_offset()
        mask = torch.ones(4096, dtype=torch.bool, device=DEV)
        for net, (a, n) in at.items():
            assert _same(arena[a:a + n], want[net].flatten()), net
            mask[a:a + n] = False
        assert bool((arena[mask] == POISON).all())
    finally:
        lib.es_ctx_destroy(ctx)


# ---------------------------------------------------------------------------------------------------------------
# pipeline and C++ host: the tiny configuration (16 x 16 latents, 128 x 128 images), 2 steps
T_STEPS = 2


@pytest.fixture(scope="module")
def built():
    from edgestyle_amd.models import StepRunner, AutoencoderKL
    from edgestyle_amd.pipeline import EdgeStyleStableDiffusionControlNetPipeline
    ucfg, vcfg = Cfg.tiny_unet(), Cfg.tiny_vae()
    ws = {k: quantize(v) for k, v in make_weights(ucfg, vcfg, seed=5).items()}
    runner = StepRunner.from_state_dicts(ws, ucfg, torch.float16, DEV)
    vae = AutoencoderKL(ws["vae"], vcfg).to(DEV)
    pipe = EdgeStyleStableDiffusionControlNetPipeline(vae=vae, unet=runner.unet, controlnet=runner.controlnet).to(DEV)
    assert pipe.noise_source == "host" and pipe.noise_dtype is None
    for net in pipe.controlnet.nets:
        if getattr(net.config, "uses_vae", False):
            net.set_autoencoder(pipe.vae)
    g = torch.Generator().manual_seed(31)
    s = ucfg.sample_size
    uses_vae = [bool(getattr(net.config, "uses_vae", False)) for net in pipe.controlnet.nets]
    H = s * vcfg.scale
    imgs = []
    for v in uses_vae:
        im = torch.rand(1, 3, H, H, generator=g)
        imgs.append(im * 2 - 1 if v else im)
    inputs = dict(
        pe=(torch.randn(1, 77, ucfg.cross_attention_dim, generator=g) * 0.5).half().float(),
        ne=(torch.randn(1, 77, ucfg.cross_attention_dim, generator=g) * 0.5).half().float(),
        imgs=imgs, uses_vae=uses_vae, s=s, L=vcfg.latent_channels, R=H)
    return pipe, inputs


def _kw(inp, **more):
    return dict(prompt_embeds=inp["pe"], negative_prompt_embeds=inp["ne"], image=inp["imgs"], guidance_scale=5.0,
                num_inference_steps=T_STEPS, output_type="pt", **more)


@pytest.mark.parametrize("resample", [False, True])
def test_pipeline_device_noise_equals_host_mode_fed_torchs_own_draws(built, resample):
    pipe, inp = built
    s, Lc = inp["s"], inp["L"]
    # what torch draws: the VAE-sample noise from the device's default generator (net order; step by step when re-sampling),
    # the latents from the caller's device generator
    torch.manual_seed(7)
    g = _gen(42)
    if resample:
        per_step = [[torch.randn((2, Lc, s, s), device=DEV) if v else None for v in inp["uses_vae"]] for _ in range(T_STEPS)]
        noise = [torch.stack([row[i] for row in per_step]) if v else None for i, v in enumerate(inp["uses_vae"])]
    else:
        noise = [torch.randn((2, Lc, s, s), device=DEV) if v else None for v in inp["uses_vae"]]
    default_after = torch.cuda.default_generators[torch.cuda.current_device()].get_offset()
    lat = torch.randn((1, 4, s, s), device=DEV, generator=g)
    assert pipe.noise_source == "host"
    want = pipe(latents=lat, cond_noise=noise, resample_cond_each_step=resample, **_kw(inp)).images.clone()
    pipe.noise_source = "device"
    try:
        for _ in range(2):                                  # re-seeding both generators gives the same image again
            torch.manual_seed(7)
            g2 = _gen(42)
            got = pipe(generator=g2, resample_cond_each_step=resample, **_kw(inp)).images
            torch.cuda.synchronize()
            assert _same(got, want), float((got - want).abs().max())
            assert g2.get_offset() == g.get_offset()
            assert torch.cuda.default_generators[torch.cuda.current_device()].get_offset() == default_after
        # explicit latents= and cond_noise= still win; a CPU generator is refused with the remedy
        got = pipe(latents=lat, cond_noise=noise, resample_cond_each_step=resample, generator=_gen(1), **_kw(inp)).images
        assert _same(got, want)
        with pytest.raises(ValueError, match="torch.Generator"):
            pipe(generator=torch.Generator().manual_seed(42), resample_cond_each_step=resample, **_kw(inp))
    finally:
        pipe.noise_source = "host"


def test_pipeline_device_noise_default_generator_and_service(built):
    pipe, inp = built
    s = inp["s"]
    # generator=None: the latents follow the condition noise on the device's default generator
    torch.manual_seed(9)
    noise = [torch.randn((2, inp["L"], s, s), device=DEV) if v else None for v in inp["uses_vae"]]
    lat = torch.randn((1, 4, s, s), device=DEV)
    want = pipe(latents=lat, cond_noise=noise, resample_cond_each_step=False, **_kw(inp)).images.clone()
    pipe.noise_source = "device"
    try:
        torch.manual_seed(9)
        got = pipe(resample_cond_each_step=False, **_kw(inp)).images
        assert _same(got, want)
    finally:
        pipe.noise_source = "host"
    from edgestyle_amd.serve import device_latents_for, latents_for
    assert _same(device_latents_for(42, 4, s, s), torch.randn((1, 4, s, s), device=DEV, generator=_gen(42)))
    assert latents_for(42, 4, s, s).device.type == "cpu"


def test_cpp_image_host_with_a_seed_writes_the_device_mode_pipelines_bytes(built, tmp_path):
    """examples/image_host.cpp --seed 42 on a saved context image: es_ctx_draw_cond_noise + es_ctx_draw_latents in a process
    without Python == the pipeline with noise_source="device", the default generator seeded 42 and a device generator seeded 42."""
    import os
    import shutil
    import subprocess
    from edgestyle_amd.native import NativeEngine
    pipe, inp = built
    gs, s, ucfg = 6.0, inp["s"], pipe.unet.cfg
    rng = np.random.default_rng(53)
    photos = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in [(150, 100), (37, 53), (131, 197), (128, 128), (300, 128), (129, 129)]]
    kw = dict(prompt_embeds=inp["pe"], negative_prompt_embeds=inp["ne"], guidance_scale=gs, num_inference_steps=T_STEPS,
              resample_cond_each_step=False)
    pipe.noise_source = "device"
    try:
        torch.manual_seed(42)
        want = pipe(image=pipe.preprocess_images(photos), output_type="u8", generator=_gen(42), **kw).images[0].cpu().numpy()
    finally:
        pipe.noise_source = "host"
    eng = NativeEngine(pipe, batch_size=1, num_inference_steps=T_STEPS)
    path = str(tmp_path / "ctx.esctx")
    try:
        eng.save(path)
    finally:
        eng.close()
    for i, a in enumerate(photos):
        with open(str(tmp_path / f"c{i}.ppm"), "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (a.shape[1], a.shape[0]) + a.tobytes())
    junk = np.full(2 * inp["L"] * s * s, 1e3, dtype=np.float32)          # the file's latents and noise records must be ignored
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(np.array([1, s, s, 4, ucfg.cross_attention_dim, 6, T_STEPS] + [int(v) for v in inp["uses_vae"]] +
                         [int(v) for v in inp["uses_vae"]], dtype=np.int32).tobytes())
        f.write(np.float32(gs).tobytes())
        f.write(pipe.scheduler.set_timesteps(T_STEPS).float().numpy().astype(np.float32).tobytes())
        f.write(junk[:s * s * 4].tobytes())
        f.write(torch.cat([inp["ne"], inp["pe"]]).half().numpy().tobytes())
        for v in inp["uses_vae"]:
            if v:
                f.write(junk.tobytes())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, libdir = str(tmp_path / "image_host"), os.path.join(root, "edgestyle_amd", "lib")
    c = subprocess.run([hipcc, "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "image_host.cpp"),
                        "-L" + libdir, "-ledgestyle_hip", "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-2000:]
    out = str(tmp_path / "out.ppm")
    r = subprocess.run([exe, path] + [str(tmp_path / f"c{i}.ppm") for i in range(6)] + [str(tmp_path / "in.bin"), out, "--seed", "42"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    head = b"P6\n%d %d\n255\n" % (inp["R"], inp["R"])
    assert raw.startswith(head) and len(raw) == len(head) + want.size
    assert np.array_equal(np.frombuffer(raw[len(head):], dtype=np.uint8).reshape(want.shape), want)
    bad = subprocess.run([exe, path] + ["x"] * 8 + ["--cond-seed", "1"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "usage" in bad.stderr

"""Byte images at the C ABI on the GPU (csrc/image_io.hip): the resize kernels against Pillow byte for byte (fixture always,
live Pillow when it imports), the two conversions against the host formulas bit for bit, es_prepare_conds_u8 / es_vae_decode_u8
against the float entry points they wrap, the pipeline's preprocess_images + output_type "u8", graph capture, and the compiled
C++ host (examples/image_host.cpp).  Every comparison is an equality."""
import numpy as np
import pytest
import torch

from edgestyle_amd import config as Cfg, lib as L, ops
from tests import image_io_ref as R
from tests.helpers import make_weights, quantize

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0xA5


def _expected(a: np.ndarray, r: int, fixture_ref=None):
    """the bytes Resize(r) -> CenterCrop(r) must give for `a`: from the fixture where it holds this (image, r), from the host
    build of the coefficient code otherwise, and - held against both - from live Pillow when it imports"""
    rh, rw, top, left = R.fit(a.shape[0], a.shape[1], r)
    full = fixture_ref if fixture_ref is not None else R.integer_resize(a, rh, rw)
    if R.have_pillow():
        assert np.array_equal(R.pillow_resize(a, rh, rw), full)
    return R.crop(full, r, top, left)


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_resize_equals_pillow_on_each_fixture_case(case):
    a, ref, r = R.fixture()[0][case]
    got = ops.image_resize_u8([_dev(a)], r)
    torch.cuda.synchronize()
    want = _expected(a, r, ref)
    assert got.shape == (1, r, r, 3) and np.array_equal(got[0].cpu().numpy(), want), int((got[0].cpu().numpy() != want).sum())


@pytest.mark.parametrize("r", [64, 32, 16])
def test_resize_of_all_fixture_cases_in_one_call(r):
    """count = 5, five geometries, one target size per call: every fixture case meets its own R in one of the three calls (and
    is then held against the fixture's bytes); at the other sizes the reference is the host build of the same coefficients"""
    cases = R.fixture()[0]
    got = ops.image_resize_u8([_dev(a) for a, _, _ in cases], r)
    torch.cuda.synchronize()
    assert got.shape == (5, r, r, 3)
    hit = 0
    for i, (a, ref, ri) in enumerate(cases):
        want = _expected(a, r, ref if ri == r else None)
        hit += ri == r
        assert np.array_equal(got[i].cpu().numpy(), want), (i, int((got[i].cpu().numpy() != want).sum()))
    assert hit == {64: 3, 32: 1, 16: 1}[r]


def test_resize_reads_rgba_rows_with_a_pitch_and_ignores_alpha_and_padding():
    a, ref, r = R.fixture()[0][1]                          # 150 x 100 -> R 32
    H, W = a.shape[:2]
    pitch_px = W + 7
    buf = torch.full((H, pitch_px, 4), POISON, dtype=torch.uint8, device=DEV)
    buf[:, :W, :3] = _dev(a)
    buf[:, :W, 3] = torch.randint(0, 256, (H, W), dtype=torch.uint8, device=DEV)
    view = buf[:, :W]
    assert view.stride(0) == pitch_px * 4 > W * 4
    got = ops.image_resize_u8([view, _dev(a)], r)
    torch.cuda.synchronize()
    want = _expected(a, r, ref)
    assert np.array_equal(got[0].cpu().numpy(), want) and np.array_equal(got[1].cpu().numpy(), want)
    assert bool((buf[:, W:] == POISON).all())


def test_resize_stays_inside_an_output_and_a_workspace_of_exactly_the_reported_size():
    cases = R.fixture()[0]
    imgs = [_dev(a) for a, _, _ in cases]
    r, guard = 32, 4096
    need = ops.image_resize_workspace_bytes(ops.image_descriptors(imgs), r)
    # at R = 32 every case changes its width: per image the source rows the kept output rows read (at most all of them) x 32 kept
    # columns x 3 bytes; 150 x 100 keeps 32 of its 48 resized rows, so it needs fewer than its 150
    assert 0 < need < sum(h for h, _, _ in R.CASES) * r * 3
    n_out = len(imgs) * r * r * 3
    obuf = torch.full((guard + n_out + guard,), POISON, dtype=torch.uint8, device=DEV)
    wbuf = torch.full((guard + need + guard,), POISON, dtype=torch.uint8, device=DEV)
    out = obuf[guard:guard + n_out].view(len(imgs), r, r, 3)
    ops.image_resize_u8(imgs, r, out=out, workspace=wbuf[guard:guard + need])
    torch.cuda.synchronize()
    for buf, n in ((obuf, n_out), (wbuf, need)):
        assert bool((buf[:guard] == POISON).all()) and bool((buf[guard + n:] == POISON).all())
    for i, (a, ref, ri) in enumerate(cases):
        assert np.array_equal(out[i].cpu().numpy(), _expected(a, r, ref if ri == r else None))
    # one byte less is refused before anything is launched
    with pytest.raises(L.EdgeStyleHipError, match="workspace"):
        ops.image_resize_u8(imgs, r, out=out, workspace=wbuf[guard:guard + need - 1])


def test_wrappers_refuse_operands_the_library_would_misread():
    a = _dev(R.fixture()[0][0][0])
    for bad in ([a.cpu()], [a.float()], [a.permute(1, 0, 2)], [a[:, :, :2]], [a[:, ::2]], []):
        with pytest.raises(L.EdgeStyleHipError):
            ops.image_resize_u8(bad, 16)
    with pytest.raises(L.EdgeStyleHipError):
        ops.image_u8_to_f32(a[None].float(), False)
    with pytest.raises(L.EdgeStyleHipError):
        ops.image_u8_to_f32(a[None][:, :, ::2], False)
    with pytest.raises(L.EdgeStyleHipError):
        ops.image_f32_to_u8(torch.zeros(1, 4, 8, 8, device=DEV))
    with pytest.raises(L.EdgeStyleHipError):
        ops.image_f32_to_u8(torch.zeros(1, 3, 8, 8, device=DEV, dtype=torch.float16))


@pytest.mark.parametrize("normalize", [False, True])
def test_u8_to_f32_equals_the_host_formula_on_all_256_values(normalize):
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    a = np.stack([v, v[::-1], np.roll(v, 85)], axis=-1)                   # every value in every channel
    got = ops.image_u8_to_f32(_dev(np.stack([a, a[:, ::-1]])), normalize)
    torch.cuda.synchronize()
    want = torch.cat([R.to_float_host(a, normalize), R.to_float_host(a[:, ::-1], normalize)])
    assert got.shape == (2, 3, 16, 16) and torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("H,W", [(64, 64), (8, 37), (5, 37)])
def test_f32_to_u8_equals_the_host_rounding(H, W):
    """W 64: whole float4 runs; 8 x 37: runs of four that straddle rows; 5 x 37: H*W = 185, a ragged tail and planes that are not
    16-byte aligned.  Values: random in [0,1], every k/255, the rounding ties (k + 0.5)/255, and values just outside [0,1]
    (they must clamp)."""
    g = np.random.default_rng(W)
    a = g.random((2, 3, H, W), dtype=np.float32)
    flat = a.reshape(-1)
    k = np.arange(256, dtype=np.float32)
    special = np.concatenate([k / np.float32(255), (k + np.float32(0.5)) / np.float32(255),
                              np.array([-1e-3, -1e-7, -0.0, 1.0 + 1e-6, 1.002, 1.5, -3.0], dtype=np.float32)])
    pos = g.choice(flat.size, size=special.size, replace=False)
    flat[pos] = special
    want = np.clip((a * 255).round(), 0, 255).astype("uint8").transpose(0, 2, 3, 1)
    inside = (a >= 0) & (a <= 1)                           # there the clamp is idle: pipeline.py's (a * 255).round().astype("uint8")
    plain = (np.where(inside, a, np.float32(0)) * 255).round().astype("uint8").transpose(0, 2, 3, 1)
    assert np.array_equal(want[inside.transpose(0, 2, 3, 1)], plain[inside.transpose(0, 2, 3, 1)])
    got = ops.image_f32_to_u8(torch.from_numpy(a).to(DEV))
    torch.cuda.synchronize()
    assert got.shape == (2, H, W, 3) and np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())


def test_resize_and_conversions_replay_inside_one_graph():
    a0, ref0, r = R.fixture()[0][0]                        # 37 x 53 -> 64
    a1 = np.random.default_rng(5).integers(0, 256, size=a0.shape, dtype=np.uint8)
    src = _dev(a0)
    need = ops.image_resize_workspace_bytes(ops.image_descriptors([src]), r)
    u8 = torch.zeros((1, r, r, 3), dtype=torch.uint8, device=DEV)
    ws = torch.zeros((need,), dtype=torch.uint8, device=DEV)
    f32 = torch.zeros((1, 3, r, r), dtype=torch.float32, device=DEV)
    back = torch.zeros((1, r, r, 3), dtype=torch.uint8, device=DEV)

    def chain():
        ops.image_resize_u8([src], r, out=u8, workspace=ws)
        ops.image_u8_to_f32(u8, False, out=f32)
        ops.image_f32_to_u8(f32, out=back)
    chain()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for a, ref in ((a1, None), (a0, ref0)):
        src.copy_(_dev(a))
        for t in (u8, f32, back):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = _expected(a, r, ref)
        assert np.array_equal(u8[0].cpu().numpy(), want)
        assert torch.equal(f32.cpu(), R.to_float_host(want, False))
        assert np.array_equal(back[0].cpu().numpy(), want)             # x / 255 * 255 rounds back to x for every byte


# ---------------------------------------------------------------------------------------------------------------
# context level and pipeline: the tiny configuration (16 x 16 latents, 128 x 128 images), 2 steps
T_STEPS = 2


@pytest.fixture(scope="module")
def built():
    from edgestyle_amd.models import StepRunner, AutoencoderKL
    from edgestyle_amd.pipeline import EdgeStyleStableDiffusionControlNetPipeline
    from edgestyle_amd.native import NativeEngine
    ucfg, vcfg = Cfg.tiny_unet(), Cfg.tiny_vae()
    ws = {k: quantize(v) for k, v in make_weights(ucfg, vcfg, seed=5).items()}
    runner = StepRunner.from_state_dicts(ws, ucfg, torch.float16, DEV)
    vae = AutoencoderKL(ws["vae"], vcfg).to(DEV)
    pipe = EdgeStyleStableDiffusionControlNetPipeline(vae=vae, unet=runner.unet, controlnet=runner.controlnet).to(DEV)
    for net in pipe.controlnet.nets:
        if getattr(net.config, "uses_vae", False):
            net.set_autoencoder(pipe.vae)                  # TT:252-258 (vae= of from_pretrained)
    eng = NativeEngine(pipe, batch_size=1, num_inference_steps=T_STEPS)
    assert L.PLAN_CONDS in eng.plan_sizes
    g = torch.Generator().manual_seed(31)
    s = ucfg.sample_size
    uses_vae = [bool(getattr(net.config, "uses_vae", False)) for net in pipe.controlnet.nets]
    inputs = dict(
        lat=torch.randn(1, 4, s, s, generator=g),
        pe=(torch.randn(1, 77, ucfg.cross_attention_dim, generator=g) * 0.5).half().float(),
        ne=(torch.randn(1, 77, ucfg.cross_attention_dim, generator=g) * 0.5).half().float(),
        noise=[torch.randn(2, vcfg.latent_channels, s, s, generator=g) if v else None for v in uses_vae],
        uses_vae=uses_vae, R=s * vcfg.scale)
    yield pipe, eng, inputs
    eng.close()


def _photos(sizes, seed):
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]


def _slots(eng):
    torch.cuda.synchronize()
    return [t.clone() for t in eng.cond_img] + [t.clone() for t in eng.loop.conds]


def _check_prepare_conds_u8(built, sizes, seed):
    pipe, eng, inp = built
    photos = _photos(sizes, seed)
    floats = [R.to_float_host(_expected(a, inp["R"]), nrm) for a, nrm in zip(photos, inp["uses_vae"])]
    noise = [None if z is None else z.to(DEV) for z in inp["noise"]]
    for use_graphs in (True, False):
        eng.set_options(use_graphs=use_graphs)
        eng.prepare_conds([f.to(DEV) for f in floats], noise)
        want = _slots(eng)
        for t in eng.cond_img + eng.loop.conds:
            t.fill_(7.0)
        eng.prepare_conds_u8([_dev(a) for a in photos], inp["uses_vae"], noise)
        got = _slots(eng)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a.view(torch.int16 if a.dtype == torch.float16 else torch.int32),
                               b.view(torch.int16 if b.dtype == torch.float16 else torch.int32)), i
        for f, slot in zip(floats, got):
            assert torch.equal(slot.cpu(), f)
    eng.set_options(use_graphs=True)


def test_prepare_conds_u8_of_images_already_the_right_size_equals_prepare_conds(built):
    r = built[2]["R"]
    _check_prepare_conds_u8(built, [(r, r)] * 6, 41)


def test_prepare_conds_u8_of_odd_sized_images_equals_prepare_conds_on_pillows_bytes(built):
    _check_prepare_conds_u8(built, [(150, 100), (37, 53), (131, 197), (128, 200), (300, 128), (129, 129)], 43)


def test_prepare_conds_u8_refuses_a_missing_noise_and_a_short_workspace(built):
    pipe, eng, inp = built
    photos = [_dev(a) for a in _photos([(150, 100)] * 6, 3)]
    with pytest.raises(L.EdgeStyleHipError, match="noise"):
        eng.prepare_conds_u8(photos, inp["uses_vae"], None)
    import ctypes as C
    descs = ops.image_descriptors(photos)
    need = ops.image_resize_workspace_bytes(descs, inp["R"])
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    nz = [None if z is None else z.to(DEV) for z in inp["noise"]]
    npz = (C.c_void_p * 6)(*[None if z is None else z.data_ptr() for z in nz])
    nrm = (C.c_int32 * 6)(*[int(v) for v in inp["uses_vae"]])
    rc = eng.lib.es_prepare_conds_u8(eng.ctx, descs, nrm, npz, C.c_void_p(ws.data_ptr()), need - 1, eng._stream())
    assert rc == -1 and b"workspace too small" in eng.lib.es_last_error()
    torch.cuda.synchronize()


def test_vae_decode_u8_equals_the_host_rounding_of_vae_decode(built):
    pipe, eng, inp = built
    x = (torch.randn(1, 16, 16, 4, generator=torch.Generator().manual_seed(9)) * 0.8).to(DEV)
    for use_graphs in (True, False):
        eng.set_options(use_graphs=use_graphs)
        img = eng.vae_decode(x)
        got = eng.vae_decode_u8(x)
        torch.cuda.synchronize()
        want = (img.permute(0, 2, 3, 1).cpu().numpy() * 255).round().astype("uint8")
        assert got.shape == (1, inp["R"], inp["R"], 3) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), want)
    eng.set_options(use_graphs=True)


def test_pipeline_preprocess_images_and_u8_output_equal_the_host_path(built):
    pipe, eng, inp = built
    photos = _photos([(150, 100), (37, 53), (131, 197), (128, 128), (300, 128), (129, 129)], 47)
    floats = [R.to_float_host(_expected(a, inp["R"]), nrm) for a, nrm in zip(photos, inp["uses_vae"])]
    mixed = [torch.from_numpy(photos[0]), photos[1], _dev(photos[2]), photos[3], photos[4], photos[5]]
    if R.have_pillow():
        from PIL import Image
        mixed[3] = Image.fromarray(photos[3])
    kw = dict(prompt_embeds=inp["pe"], negative_prompt_embeds=inp["ne"], latents=inp["lat"], guidance_scale=5.0,
              num_inference_steps=T_STEPS, cond_noise=inp["noise"])
    want = pipe(image=floats, output_type="pt", **kw).images
    want = (want.permute(0, 2, 3, 1).cpu().numpy() * 255).round().astype("uint8")
    pre = pipe.preprocess_images(mixed)
    assert all(p.shape == (1, 3, inp["R"], inp["R"]) and p.is_cuda and torch.equal(p.cpu(), f) for p, f in zip(pre, floats))
    for _ in range(2):                                     # the second call replays the captured decode graph
        got = pipe(image=pre, output_type="u8", **kw).images
        assert got.dtype == torch.uint8 and got.is_cuda and got.shape == (1, inp["R"], inp["R"], 3)
        assert np.array_equal(got.cpu().numpy(), want)
    pipe.use_graph = False
    try:
        assert np.array_equal(pipe(image=pre, output_type="u8", **kw).images.cpu().numpy(), want)
    finally:
        pipe.use_graph = True
    # explicit flags / resolution, and what cannot be defaulted is refused
    one = pipe.preprocess_images([photos[1]], resolution=32, normalize=True)[0]
    assert torch.equal(one.cpu(), R.to_float_host(_expected(photos[1], 32), True))
    with pytest.raises(ValueError):
        pipe.preprocess_images(photos[:2])
    with pytest.raises(ValueError):
        pipe.preprocess_images([photos[0].astype(np.float32)], normalize=False)


def test_cpp_image_host_writes_the_pipelines_u8_bytes(built, tmp_path):
    """examples/image_host.cpp on a saved context image: six PPM files of different sizes -> es_prepare_conds_u8 ->
    es_denoise_loop -> es_vae_decode_u8 -> a PPM whose pixels equal the Python pipeline's "u8" output."""
    import os
    import shutil
    import subprocess
    pipe, eng, inp = built
    photos = _photos([(150, 100), (37, 53), (131, 197), (128, 128), (300, 128), (129, 129)], 53)
    gs = 6.0
    kw = dict(prompt_embeds=inp["pe"], negative_prompt_embeds=inp["ne"], latents=inp["lat"], guidance_scale=gs,
              num_inference_steps=T_STEPS, cond_noise=inp["noise"])
    want = pipe(image=pipe.preprocess_images(photos), output_type="u8", **kw).images[0].cpu().numpy()
    path = str(tmp_path / "ctx.esctx")
    eng.save(path)
    s, ucfg = 16, pipe.unet.cfg
    for i, a in enumerate(photos):
        with open(str(tmp_path / f"c{i}.ppm"), "wb") as f:
            f.write(b"P6\n# condition image\n%d %d\n255\n" % (a.shape[1], a.shape[0]) + a.tobytes())
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(np.array([1, s, s, 4, ucfg.cross_attention_dim, 6, T_STEPS] + [int(z is not None) for z in inp["noise"]] +
                         [int(v) for v in inp["uses_vae"]], dtype=np.int32).tobytes())
        f.write(np.float32(gs).tobytes())
        f.write(pipe.scheduler.set_timesteps(T_STEPS).float().numpy().astype(np.float32).tobytes())
        f.write(inp["lat"].permute(0, 2, 3, 1).contiguous().numpy().astype(np.float32).tobytes())
        f.write(torch.cat([inp["ne"], inp["pe"]]).half().numpy().tobytes())
        for z in inp["noise"]:
            if z is not None:
                f.write(z.numpy().astype(np.float32).tobytes())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, libdir = str(tmp_path / "image_host"), os.path.join(root, "edgestyle_amd", "lib")
    c = subprocess.run([hipcc, "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "image_host.cpp"),
                        "-L" + libdir, "-ledgestyle_hip", "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-2000:]
    out = str(tmp_path / "out.ppm")
    r = subprocess.run([exe, path] + [str(tmp_path / f"c{i}.ppm") for i in range(6)] + [str(tmp_path / "in.bin"), out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    head = b"P6\n%d %d\n255\n" % (inp["R"], inp["R"])
    assert raw.startswith(head) and len(raw) == len(head) + want.size
    assert np.array_equal(np.frombuffer(raw[len(head):], dtype=np.uint8).reshape(want.shape), want)

"""The prompt assembly and the device entry of the text encoder on the GPU: es_prompt_assemble against its host mirror,
es_text_encode_dev against es_text_encode, the two captured into one graph, NativeBestEmbeddings.encode_prompts against the string
path it replaces, the compiled host, and the pipeline under the native tokenizer.  Every comparison is an equality, bit for bit."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from edgestyle_amd import lib as L
from edgestyle_amd.clip import NativeBestEmbeddings
from edgestyle_amd.text import NativeCLIPTextEncoder
from edgestyle_amd.tokenizer import NativeCLIPTokenizer
from tests import clip_ref as CR
from tests import text_ref as TR
from tests import tokenizer_ref as R
from tests.test_tokenizer_cpu import COLORS, ITEMS, assemble_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
GUARD, POISON = 64, -77
KW = dict(padding="max_length", truncation=True, return_tensors="pt")
SUFFIX = "best quality, a polo shirt they're wearing"
PHOTOS = [(0, 90, 61), (1, 120, 200), (2, 56, 56)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return R.write_files(tmp_path_factory.mktemp("prompt_tok"))


def _tokenizer(files, max_length=77):
    return NativeCLIPTokenizer(files[0], files[1], max_length)


def _text_config(tok, max_positions=77, **kw):
    """the tiny text model of these tests: hidden 64, 2 heads of 32, 2 layers, intermediate 128"""
    base = dict(vocab_size=tok.vocab_size, hidden_size=64, num_attention_heads=2, num_hidden_layers=2, intermediate_size=128,
                max_position_embeddings=max_positions, bos_token_id=tok.bos_token_id, eos_token_id=tok.eos_token_id, pad_token_id=tok.pad_token_id)
    base.update(kw)
    return TR.tiny_config(**base)


def _encoder(tok, dtype, max_n, max_positions=77, seed=5, **kw):
    cfg = _text_config(tok, max_positions, **kw)
    return NativeCLIPTextEncoder.from_module(TR.make_model(cfg, seed=seed), dtype=dtype, device=DEV, max_n=max_n), cfg


def _photos():
    a, b, c = (CR.photo(h, w, seed=s) for s, h, w in PHOTOS)
    return [a, 255 - b, c // 4]


def _clip_model(tok, seed=20):
    cfg = CR.config(text=dict(vocab_size=tok.vocab_size, bos_token_id=tok.bos_token_id, eos_token_id=tok.eos_token_id, pad_token_id=tok.pad_token_id))
    return CR.make_model(cfg, seed=seed, logit_scale=4.6052)


@pytest.mark.parametrize("Lm", [8, 16, 77])
def test_assemble_equals_its_host_mirror(files, Lm):
    tok = _tokenizer(files, Lm)
    words = COLORS + ITEMS
    for suffix in ("", SUFFIX):
        for name, nseg, k, topk in assemble_cases():
            seg_ends = [len(words)] if nseg == 1 else [len(COLORS), len(words)]
            table = tok.prompt_table(words, seg_ends, prefix="edgestyle", separator=",", suffix=suffix, device=torch.cuda.current_device())
            try:
                for n in (1, 3):
                    want_ids, want_eos = table.assemble_host(topk[:n])
                    buf = torch.full((n * Lm + 2 * GUARD,), POISON, dtype=torch.int32, device=DEV)
                    ebuf = torch.full((n + 2 * GUARD,), POISON, dtype=torch.int32, device=DEV)
                    ids, eos = table.assemble(topk[:n].to(DEV), ids_out=buf[GUARD:GUARD + n * Lm].view(n, Lm), eos_out=ebuf[GUARD:GUARD + n])
                    torch.cuda.synchronize()
                    assert torch.equal(ids.cpu(), want_ids) and torch.equal(eos.cpu(), want_eos), (name, suffix, n)
                    for b in (buf.cpu(), ebuf.cpu()):
                        assert bool((b[:GUARD] == POISON).all()) and bool((b[-GUARD:] == POISON).all()), "a write outside the output"
                    # eos_pos is optional
                    ids2 = torch.full((n, Lm), POISON, dtype=torch.int32, device=DEV)
                    L.check(table.lib.es_prompt_assemble(table._h, C.c_void_p(topk[:n].to(DEV).data_ptr()), n, k, C.c_void_p(ids2.data_ptr()), None,
                                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "es_prompt_assemble")
                    torch.cuda.synchronize()
                    assert torch.equal(ids2.cpu(), want_ids)
            finally:
                table.close()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("S", [16, 77])
def test_text_encode_dev_is_bitwise_text_encode(files, S, dt):
    tok, max_n = _tokenizer(files, S), 3
    enc, cfg = _encoder(tok, DTYPES[dt], max_n, S)
    try:
        ids = TR.token_ids(cfg, max_n, seed=2) if S == 77 else tok(["red", "a polo shirt, a tank top and the jeans they're wearing", ""], **KW).input_ids
        assert ids.shape == (max_n, S)
        for n in range(1, max_n + 1):
            want = enc.encode_ids(ids[:n])
            got = enc.encode_ids_device(ids[:n].to(DEV, torch.int32).contiguous())
            torch.cuda.synchronize()
            assert got.dtype == DTYPES[dt] and tuple(got.shape) == (n, S, 64) and bool(torch.isfinite(got.float()).all())
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), n
        with pytest.raises(L.EdgeStyleHipError, match=r"n = 4 is outside 1\.\.max_n = 3"):
            enc.encode_ids_device(torch.zeros(4, S, dtype=torch.int32, device=DEV))
        with pytest.raises(L.EdgeStyleHipError, match="ids_dev must be"):
            enc.encode_ids_device(ids[:1].to(DEV))                      # int64
    finally:
        enc.close()


def test_assemble_and_encode_replay_from_one_graph(files):
    """one chain, no parallel branches: es_prompt_assemble -> es_text_encode_dev captured once, replayed for two topk contents"""
    tok = _tokenizer(files)
    words, n, k = COLORS + ITEMS, 2, 2
    enc, cfg = _encoder(tok, torch.float16, n)
    table = tok.prompt_table(words, [len(COLORS), len(words)], prefix="edgestyle", separator=",", suffix=SUFFIX, device=torch.cuda.current_device())
    try:
        first = torch.tensor([[[0, 3], [1, 2]], [[6, 5], [8, 0]]], dtype=torch.int32)
        second = torch.tensor([[[2, -1], [7, 7]], [[4, 1], [9, 3]]], dtype=torch.int32)           # an unfilled slot and one past the list among them
        topk = first.to(DEV)
        ids = torch.zeros((n, 77), dtype=torch.int32, device=DEV)
        eos = torch.zeros((n,), dtype=torch.int32, device=DEV)
        out = torch.zeros((n, 77, 64), dtype=torch.float16, device=DEV)

        def chain():
            table.assemble(topk, ids_out=ids, eos_out=eos)
            enc.encode_ids_device(ids, out=out)
        eager = []
        for t in (first, second):
            topk.copy_(t)
            chain()
            torch.cuda.synchronize()
            eager.append((ids.cpu().clone(), eos.cpu().clone(), out.cpu().clone()))
        assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[0][2], eager[1][2])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            chain()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            chain()
        for t, (w_ids, w_eos, w_out) in zip((first, second), eager):
            topk.copy_(t)
            ids.zero_(), eos.zero_(), out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(ids.cpu(), w_ids) and torch.equal(eos.cpu(), w_eos)
            assert torch.equal(out.cpu().view(torch.int16), w_out.view(torch.int16))
        # the host-staged entry still refuses a capturing stream; nothing of it lands in the graph
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2):
            rc = enc.lib.es_text_encode(enc._h, C.c_void_p(eager[0][0].data_ptr()), n, C.c_void_p(out.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
            table.assemble(topk, ids_out=ids, eos_out=eos)               # so that the capture is not empty
        assert rc == -1 and b"capturing" in enc.lib.es_last_error()
    finally:
        table.close()
        enc.close()


def test_encode_prompts_is_the_string_path_bit_for_bit(files):
    """encode_prompts == encoder(tokenizer(picker(images) + " " + suffix)), with the native tokenizer and with transformers'"""
    tok, oracle = _tokenizer(files), R.oracle(files[0], files[1])
    photos = _photos()
    be = NativeBestEmbeddings.from_module(_clip_model(tok), tok, colors=COLORS, clothing_items=ITEMS, dtype=torch.float16, device=DEV,
                                          max_images=len(photos), text_batch=4)
    enc, cfg = _encoder(tok, torch.float16, len(photos))
    try:
        prompts = be(photos)
        print("prompts:", prompts)
        assert len(set(prompts)) > 1
        for suffix in ("", SUFFIX):
            got = be.encode_prompts(photos, enc, suffix=suffix)
            assert got.is_cuda and tuple(got.shape) == (len(photos), 77, 64)
            texts = [p + " " + suffix for p in prompts]
            for t in (tok, oracle):
                want = enc(t(texts, max_length=77, **KW).input_ids)[0]
                torch.cuda.synchronize()
                assert torch.equal(got.view(torch.int16), want.view(torch.int16))
            one = be.encode_prompts(photos[1:2], enc, suffix=suffix)
            assert torch.equal(one[0], got[1])
        assert set(be._tables) == {"", SUFFIX}                            # one table per suffix, kept
        # a picker over transformers' tokenizer has no token table to assemble from
        be2 = NativeBestEmbeddings.from_module(_clip_model(tok), oracle, colors=COLORS[:3], clothing_items=ITEMS[:3], dtype=torch.float16, device=DEV,
                                               max_images=1, text_batch=4)
        try:
            with pytest.raises(L.EdgeStyleHipError, match="needs tokenizer=NativeCLIPTokenizer"):
                be2.encode_prompts(photos[:1], enc)
        finally:
            be2.close()
        with pytest.raises(L.EdgeStyleHipError, match="the word 'shirt!' tokenises differently"):
            NativeBestEmbeddings.from_module(_clip_model(tok), tok, colors=COLORS[:3], clothing_items=["shirt!", "coat"], dtype=torch.float16,
                                             device=DEV, max_images=1, text_batch=4)
    finally:
        enc.close()
        be.close()


def test_compiled_prompt_host_writes_the_bytes_of_the_ctypes_path(files, tmp_path):
    """examples/prompt_host.cpp: a CLIPModel directory, the tokenizer's two files, a words file, a PPM and two texts -> the `ehs` record"""
    tok = _tokenizer(files)
    model = _clip_model(tok)
    d = tmp_path / "clip"
    model.save_pretrained(str(d))
    assert (d / "model.safetensors").exists() and (d / "config.json").exists()
    photo = _photos()[1]
    with open(tmp_path / "garment.ppm", "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (photo.shape[1], photo.shape[0]) + photo.tobytes())
    (tmp_path / "words.txt").write_text("\n".join(COLORS) + "\n\n" + "\n".join(ITEMS) + "\n")
    negative = "low quality, blurry, bad hands"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, libdir = str(tmp_path / "prompt_host"), os.path.join(root, "edgestyle_amd", "lib")
    c = subprocess.run([hipcc, "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "prompt_host.cpp"),
                        "-L" + libdir, "-ledgestyle_hip", "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-2000:]
    text_sd = CR.text_sd(CR.floats(model.state_dict()))
    for dt, dtype in DTYPES.items():
        r = subprocess.run([exe, str(d), files[0], files[1], str(tmp_path / "words.txt"), str(tmp_path / "garment.ppm"), SUFFIX, negative,
                            str(tmp_path / f"ehs_{dt}.bin"), dt], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        be = NativeBestEmbeddings.from_module(model, tok, colors=COLORS, clothing_items=ITEMS, dtype=dtype, device=DEV, max_images=1)
        enc = NativeCLIPTextEncoder.from_state_dict(text_sd, model.config.text_config, dtype=dtype, device=DEV, max_n=2)
        try:
            assert f"prompt: {be([photo])[0]} {SUFFIX}" in r.stdout, r.stdout
            _, _, topk = be.score([photo], be._bank, be._segments, 2)
            ids = torch.empty((2, 77), dtype=torch.int32, device=DEV)
            ids[0] = tok([negative], **KW).input_ids[0].to(DEV, torch.int32)
            be.prompt_table(SUFFIX).assemble(topk, ids_out=ids[1:2])
            want = enc.encode_ids_device(ids).cpu().contiguous()
        finally:
            enc.close()
            be.close()
        got = np.fromfile(str(tmp_path / f"ehs_{dt}.bin"), dtype=np.int16)
        assert got.size == want.numel() and np.array_equal(got, want.view(torch.int16).numpy().reshape(-1))


def test_pipeline_under_the_native_tokenizer_gives_the_transformers_image(files):
    from edgestyle_amd import config as Cf
    from edgestyle_amd.models import AutoencoderKL, ControlLoRAModel, ControlNetModel, EdgeStyleMultiControlNetModel, UNet2DConditionModel
    from edgestyle_amd.pipeline import StableDiffusionControlNetPipeline
    from tests.helpers import make_weights, quantize
    from tests.test_pipeline_gpu import _inputs
    ucfg, vcfg = Cf.tiny_unet(), Cf.tiny_vae()
    ws = {k: quantize(v) for k, v in make_weights(ucfg, vcfg).items()}
    unet, vae = UNet2DConditionModel(ws["unet"], ucfg, torch.float16), AutoencoderKL(ws["vae"], vcfg)
    pose = ControlNetModel(ws["openpose"], ucfg, torch.float16)
    l0, l1 = (ControlLoRAModel(ws[k], ucfg, lora_linear_rank=4, uses_vae=True) for k in ("lora0", "lora1"))
    for net in (l0, l1):
        net.set_autoencoder(vae)
        net.tie_weights(unet)
    mc = EdgeStyleMultiControlNetModel([l0, pose, l1, pose, l1, pose])
    mc.load_state_dict(ws["fusion"])
    pipe = StableDiffusionControlNetPipeline.from_pretrained(None, vae=vae, unet=unet, controlnet=mc, safety_checker=None, torch_dtype=torch.float16)
    tok, oracle = _tokenizer(files), R.oracle(files[0], files[1])
    enc, _ = _encoder(tok, torch.float16, 2, hidden_size=ucfg.cross_attention_dim, seed=11)
    try:
        lat, _, _, conds = _inputs(ucfg, 1, seed=91)
        kw = dict(prompt="edgestyle, red, navy, dress, tank top " + SUFFIX, negative_prompt="low quality, blurry", image=conds, latents=lat,
                  guidance_scale=5.0, num_inference_steps=3, output_type="pt")
        images = []
        for t in (tok, oracle):
            p = StableDiffusionControlNetPipeline(vae=pipe.vae, text_encoder=enc, tokenizer=t, unet=pipe.unet, controlnet=pipe.controlnet).to(DEV)
            assert p.tokenizer is t
            images.append(p(**kw).images)
        assert torch.equal(images[0], images[1]) and bool(torch.isfinite(images[0]).all())
    finally:
        enc.close()

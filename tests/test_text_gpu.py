"""The text encoder at the C ABI on the GPU: es_attention_causal, es_text_embed and es_text_encoder against fp64 (tests/text_ref.py).

Metric and bar are the project's own (tests/numerics.py): row_err against an fp64 computation on the same inputs, at most MARGIN (2.0)
times the row_err of the textbook fp32 sequence with every op's output rounded to the storage dtype; every result finite.  Equalities
(the mask, the embedding, the pipeline, the compiled host) are bit for bit.  Every figure is printed before it is asserted."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from edgestyle_amd import lib as L
from tests import numerics as nm
from tests import text_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
ES_DT = {torch.float16: L.ES_F16, torch.bfloat16: L.ES_BF16}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def causal(q, k, v, o, heads, dtype):
    """es_attention_causal on views [N, S, C] of device buffers (any row / batch strides)"""
    N, S, Cc = q.shape
    a = L.AttnDesc()
    a.q, a.k, a.v, a.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    a.N, a.heads, a.Sq, a.Skv, a.d = N, heads, S, S, Cc // heads
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(1), k.stride(1), v.stride(1), o.stride(1)
    a.bsq, a.bsk, a.bsv, a.bso = q.stride(0), k.stride(0), v.stride(0), o.stride(0)
    a.scale, a.dtype = (Cc // heads) ** -0.5, ES_DT[dtype]
    L.check(L.load().es_attention_causal(C.byref(a), _stream()), "es_attention_causal")


def _poisoned_run(q, k, v, heads, dtype):
    """q | k | v as column slices of one NaN-filled buffer, into an `out` view inside NaN guards; returns the output on the host"""
    qv, kv, vv, _ = nm.attn_views(q, k, v, heads, dtype, "nan")
    buf = qv._base.to(DEV)
    views = [nm.view_from(buf, nm.view_recipe(t)) for t in (qv, kv, vv)]
    N, S, Cc = q.shape
    out, check = nm.attn_out_guarded(N, S, Cc, dtype, device=DEV)
    causal(*views, out, heads, dtype)
    torch.cuda.synchronize()
    check(out._base)
    return out.float().cpu()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("S", [1, 16, 17, 77, 128])
def test_attention_causal_against_fp64_through_poisoned_views(S, d, dt):
    dtype = DTYPES[dt]
    for N in (1, 3):
        for heads in (1, 3):
            g = torch.Generator().manual_seed(S * 1000 + d * 10 + N * 3 + heads)
            q, k, v = (nm.rnd(torch.randn(N, S, heads * d, generator=g), dtype) for _ in range(3))
            ref64 = R.causal_ref64(q, k, v, heads)
            base = nm.row_err(R.causal_base_ref(q, k, v, heads, dtype), ref64)
            got = _poisoned_run(q, k, v, heads, dtype)
            err = nm.row_err(got, ref64)
            print(f"causal S={S} d={d} {dt} N={N} heads={heads}: row_err {err:.3e}, textbook {base:.3e}, ratio {err / base if base else 0.0:.2f}")
            assert bool(torch.isfinite(got).all())
            assert err <= nm.MARGIN * base, (err, base)
            # query 0 sees key 0 alone: its output IS v[:, 0]
            assert torch.equal(got[:, 0], v[:, 0])


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("d", [32, 64])
def test_the_mask_is_real(d, dt):
    """K and V rows from p = 40 on rewritten to finite loud values: output rows below p do not move by a bit"""
    dtype, S, p, N, heads = DTYPES[dt], 77, 40, 2, 3
    g = torch.Generator().manual_seed(77 + d)
    q, k, v = (nm.rnd(torch.randn(N, S, heads * d, generator=g), dtype) for _ in range(3))
    first = _poisoned_run(q, k, v, heads, dtype)
    loud = torch.full(((S - p) * heads * d,), 6.0e4)              # finite, not NaN: a zero probability times NaN is NaN in any matrix product
    loud[1::2] = -6.0e4
    loud = nm.rnd(loud, dtype).reshape(1, S - p, heads * d)
    k2, v2 = k.clone(), v.clone()
    k2[:, p:], v2[:, p:] = loud, loud
    second = _poisoned_run(q, k2, v2, heads, dtype)
    assert torch.equal(first[:, :p], second[:, :p])
    assert not torch.equal(first[:, p:], second[:, p:])
    assert bool(torch.isfinite(first).all()) and bool(torch.isfinite(second).all())


@pytest.mark.parametrize("dt", list(DTYPES))
def test_text_embed_is_bit_equal(dt):
    dtype, V, S, Cc, n = DTYPES[dt], 96, 77, 128, 3
    g = torch.Generator().manual_seed(5)
    tok, pos = torch.randn(V, Cc, generator=g), 0.1 * torch.randn(S, Cc, generator=g)
    ids = torch.randint(0, V, (n, S), generator=g)
    ids[0, 0], ids[0, 1], ids[2, S - 1] = 0, V - 1, V - 1
    want = (tok[ids] + pos).to(dtype)
    out = torch.full((n * S, Cc), float("nan"), dtype=dtype, device=DEV)
    ids_d, tok_d, pos_d = ids.to(DEV, torch.int32).reshape(-1).contiguous(), tok.to(DEV), pos.to(DEV)
    L.check(L.load().es_text_embed(ids_d.data_ptr(), tok_d.data_ptr(), pos_d.data_ptr(), out.data_ptr(), n * S, S, Cc, V, ES_DT[dtype], _stream()),
            "es_text_embed")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().reshape(n, S, Cc), want)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape,n", [("tiny", 3), ("wide", 2)])
def test_encoder_end_to_end_against_fp64(shape, n, dt):
    """tiny: C = 128, 2 heads of 64, 2 layers; wide: SD1.5's widths (768, 12 heads, 3072) with 2 layers - 154 rows, the ragged GEMM edge"""
    from edgestyle_amd.text import NativeCLIPTextEncoder
    dtype = DTYPES[dt]
    cfg, sd, ids, ref64, base = R.encoder_case(shape, dtype, n)
    enc = NativeCLIPTextEncoder.from_state_dict(sd, cfg, dtype=dtype, device=DEV, max_n=n)
    try:
        got = enc(ids)[0]
        torch.cuda.synchronize()
        assert got.dtype == dtype and tuple(got.shape) == (n, cfg.max_position_embeddings, cfg.hidden_size)
        err = nm.row_err(got.float().cpu(), ref64)
        print(f"encoder {shape} n={n} {dt}: row_err {err:.3e}, textbook {base:.3e}, ratio {err / base:.2f}")
        assert bool(torch.isfinite(got).all())
        assert err <= nm.MARGIN * base, (err, base)
        # another id at position 40 leaves output rows 0..39 bit-identical (transformers does exactly that on the CPU: test_text_cpu.py)
        ids2 = ids.clone()
        ids2[:, 40] = (ids2[:, 40] + 7) % cfg.vocab_size
        got2 = enc(ids2)[0]
        torch.cuda.synchronize()
        assert torch.equal(got2[:, :40], got[:, :40]) and not torch.equal(got2[:, 40:], got[:, 40:])
        # fewer prompts than max_n, and the same rows again: a row does not depend on its neighbours
        one = enc(ids[1:2])[0]
        assert torch.equal(one[0], got[1])
        with pytest.raises(L.EdgeStyleHipError, match="position 5"):
            bad = ids.clone()
            bad[0, 5] = cfg.vocab_size
            enc(bad)
    finally:
        enc.close()


def _synthetic_tokenizer(tmp_path):
    """the byte-level BPE vocabulary test_pipeline_gpu.py builds"""
    import json
    from transformers import CLIPTokenizer
    chars = [chr(c) for c in range(ord("a"), ord("z") + 1)] + [",", "."]
    vocab = {}
    for ch in chars:
        vocab[ch] = len(vocab)
    for ch in chars:
        vocab[ch + "</w>"] = len(vocab)
    vocab["<|startoftext|>"] = len(vocab)
    vocab["<|endoftext|>"] = len(vocab)
    (tmp_path / "vocab.json").write_text(json.dumps(vocab))
    (tmp_path / "merges.txt").write_text("#version: 0.2\n")
    return CLIPTokenizer(str(tmp_path / "vocab.json"), str(tmp_path / "merges.txt"), model_max_length=77), vocab


def test_pipeline_with_the_native_text_encoder(tmp_path):
    """text_encoder=NativeCLIPTextEncoder: prompt= / negative_prompt= gives the image of the prompt_embeds= call fed the encoder's own output"""
    from edgestyle_amd import config as Cf
    from edgestyle_amd.models import AutoencoderKL, ControlLoRAModel, ControlNetModel, EdgeStyleMultiControlNetModel, UNet2DConditionModel
    from edgestyle_amd.pipeline import StableDiffusionControlNetPipeline
    from edgestyle_amd.text import NativeCLIPTextEncoder
    from tests.helpers import make_weights, quantize
    from tests.test_pipeline_gpu import _inputs
    # the tiny pipeline of test_pipeline_gpu.py
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
    tok, vocab = _synthetic_tokenizer(tmp_path)
    cfg = R.tiny_config(vocab_size=len(vocab), hidden_size=ucfg.cross_attention_dim, intermediate_size=128, num_attention_heads=2,
                        bos_token_id=vocab["<|startoftext|>"], eos_token_id=vocab["<|endoftext|>"], pad_token_id=vocab["<|endoftext|>"])
    enc = NativeCLIPTextEncoder.from_module(R.make_model(cfg, seed=11), dtype=torch.float16, device=DEV, max_n=2)
    try:
        p2 = StableDiffusionControlNetPipeline(vae=pipe.vae, text_encoder=enc, tokenizer=tok, unet=pipe.unet, controlnet=pipe.controlnet).to(DEV)
        assert p2.text_encoder is enc and enc.device.type == "cuda"          # pipeline.to() sends text encoders to the CPU: this one stays
        lat, _, _, conds = _inputs(ucfg, 1, seed=91)
        prompt, neg = "edgestyle, red, dress some text", "blurry"

        def emb(t):
            return enc(tok([t], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids)[0].float()
        pe, ne = emb(prompt), emb(neg)
        assert pe.shape == (1, 77, ucfg.cross_attention_dim) and not torch.equal(pe, ne) and bool(torch.isfinite(pe).all())
        kw = dict(image=conds, latents=lat, guidance_scale=5.0, num_inference_steps=3, output_type="pt")
        a = p2(prompt=prompt, negative_prompt=neg, **kw).images
        b = p2(prompt_embeds=pe, negative_prompt_embeds=ne, **kw).images
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    finally:
        enc.close()


def test_compiled_text_host_writes_the_bytes_of_the_ctypes_path(tmp_path):
    """examples/text_host.cpp: a text_encoder/ directory as transformers saves it + a file of int32 ids -> the `ehs` record"""
    from edgestyle_amd.text import NativeCLIPTextEncoder
    cfg = R.tiny_config()
    model = R.make_model(cfg, seed=3)
    d = tmp_path / "text_encoder"
    model.save_pretrained(str(d))
    assert (d / "model.safetensors").exists() and (d / "config.json").exists()
    ids = R.token_ids(cfg, 2)
    ids.to(torch.int32).numpy().tofile(str(tmp_path / "ids.bin"))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe, libdir = str(tmp_path / "text_host"), os.path.join(root, "edgestyle_amd", "lib")
    c = subprocess.run([hipcc, "-O1", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "text_host.cpp"),
                        "-L" + libdir, "-ledgestyle_hip", "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-2000:]
    for dt, dtype in DTYPES.items():
        r = subprocess.run([exe, str(d), str(tmp_path / "ids.bin"), str(tmp_path / f"ehs_{dt}.bin"), dt], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        enc = NativeCLIPTextEncoder.from_module(model, dtype=dtype, device=DEV, max_n=2)
        try:
            want = enc(ids)[0].cpu().contiguous()
        finally:
            enc.close()
        got = np.fromfile(str(tmp_path / f"ehs_{dt}.bin"), dtype=np.int16)
        assert got.size == want.numel() and np.array_equal(got, want.view(torch.int16).numpy().reshape(-1))

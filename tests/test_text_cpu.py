"""The text encoder at the C ABI, the part that needs no GPU: dry builds from a random-init CLIPTextModel, every refusal with its error
text, and the CPU restatement (tests/text_ref.py) the GPU tests measure against, pinned to transformers' own forward."""
import ctypes as C

import pytest
import torch

from edgestyle_amd import lib as L
from edgestyle_amd.lib import EdgeStyleHipError
from edgestyle_amd.text import NativeCLIPTextEncoder, state_dict_descriptors
from tests import text_ref as R


@pytest.fixture(scope="module")
def tiny():
    cfg = R.tiny_config()
    return cfg, R.make_model(cfg, seed=3)


def _cfg_dict(cfg, **kw):
    d = dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_attention_heads=cfg.num_attention_heads,
             num_hidden_layers=cfg.num_hidden_layers, intermediate_size=cfg.intermediate_size,
             max_position_embeddings=cfg.max_position_embeddings, layer_norm_eps=cfg.layer_norm_eps, hidden_act=cfg.hidden_act)
    d.update(kw)
    return d


def test_abi_version_is_unchanged_and_the_new_symbols_resolve():
    lib = L.load()
    assert lib.es_abi_version() == 7
    for name in ("es_attention_causal", "es_text_embed", "es_text_encoder_create", "es_text_encoder_destroy", "es_text_encoder_arena_bytes",
                 "es_text_encode"):
        assert name in L.SYMBOLS and getattr(lib, name)


def test_dry_build_with_bare_and_prefixed_keys(tiny):
    cfg, model = tiny
    sd = R.bare(model.state_dict())
    assert "embeddings.token_embedding.weight" in sd
    a = NativeCLIPTextEncoder.from_module(model, device=None, max_n=3)
    b = NativeCLIPTextEncoder.from_state_dict(sd, cfg, device=None, max_n=3)
    pre = {"text_model." + k: v for k, v in sd.items()}
    pre["text_model.embeddings.position_ids"] = torch.arange(cfg.max_position_embeddings)[None]       # int64, as older checkpoints carry it
    desc, _keep = state_dict_descriptors(pre)
    assert desc.count == len(sd)                                                                       # dropped by the binding
    c = NativeCLIPTextEncoder.from_state_dict(pre, _cfg_dict(cfg), device=None, max_n=3)
    assert a.arena_bytes == b.arena_bytes == c.arena_bytes > 0
    # the fp32 tables alone are (vocab + positions) * hidden * 4 bytes; more prompts need more activations
    assert a.arena_bytes > (cfg.vocab_size + cfg.max_position_embeddings) * cfg.hidden_size * 4
    assert NativeCLIPTextEncoder.from_module(model, device=None, max_n=8).arena_bytes > a.arena_bytes
    assert NativeCLIPTextEncoder.from_module(model, dtype=torch.bfloat16, device=None, max_n=3).arena_bytes == a.arena_bytes
    assert a.to("cpu") is a and a.device is None


def test_a_missing_key_and_a_wrong_shape_are_named(tiny):
    cfg, model = tiny
    sd = R.bare(model.state_dict())
    for key in ("encoder.layers.1.mlp.fc2.bias", "final_layer_norm.weight", "embeddings.position_embedding.weight"):
        with pytest.raises(EdgeStyleHipError, match="missing key '" + key.replace(".", r"\.") + "'"):
            NativeCLIPTextEncoder.from_state_dict({k: v for k, v in sd.items() if k != key}, cfg, device=None)
    bad = dict(sd)
    bad["encoder.layers.0.self_attn.k_proj.weight"] = torch.zeros(128, 64)
    with pytest.raises(EdgeStyleHipError, match=r"size mismatch for 'encoder\.layers\.0\.self_attn\.k_proj\.weight': \(128,64\) vs \(128,128\)"):
        NativeCLIPTextEncoder.from_state_dict(bad, cfg, device=None)
    bad = dict(sd)
    bad["embeddings.token_embedding.weight"] = torch.zeros(95, 128)
    with pytest.raises(EdgeStyleHipError, match=r"size mismatch for 'embeddings\.token_embedding\.weight'"):
        NativeCLIPTextEncoder.from_state_dict(bad, cfg, device=None)


@pytest.mark.parametrize("change,text", [
    (dict(hidden_size=96, num_attention_heads=3), "hidden must be a multiple of 64"),
    (dict(num_attention_heads=8), "hidden / heads must be 32 or 64"),
    (dict(num_attention_heads=3), "hidden / heads must be 32 or 64"),
    (dict(max_position_embeddings=129), r"max_positions must be in 1\.\.128"),
    (dict(intermediate_size=200), "intermediate must be a multiple of 64"),
    (dict(hidden_act="gelu"), "quick_gelu"),
])
def test_refused_configurations(tiny, change, text):
    cfg, model = tiny
    with pytest.raises(EdgeStyleHipError, match=text):
        NativeCLIPTextEncoder.from_state_dict(R.bare(model.state_dict()), _cfg_dict(cfg, **change), device=None)


def test_act_is_refused_by_the_library_too(tiny):
    cfg, model = tiny
    lib = L.load()
    desc, _keep = state_dict_descriptors(R.bare(model.state_dict()))
    tc = L.TextConfig(vocab_size=96, hidden=128, heads=2, layers=2, intermediate=256, max_positions=77, ln_eps=1e-5, act=1)
    h = C.c_void_p()
    assert lib.es_text_encoder_create(C.byref(desc), C.byref(tc), L.ES_F16, 1, -1, C.byref(h)) == -1 and not h.value
    assert b"quick_gelu" in lib.es_last_error()
    tc.act = 0
    assert lib.es_text_encoder_create(C.byref(desc), C.byref(tc), L.ES_F32, 1, -1, C.byref(h)) == -1
    assert b"dtype" in lib.es_last_error()


def test_encode_on_a_dry_object_and_more_prompts_than_max_n_are_errors(tiny):
    cfg, model = tiny
    e = NativeCLIPTextEncoder.from_module(model, device=None, max_n=2)
    ids = R.token_ids(cfg, 3)
    with pytest.raises(EdgeStyleHipError, match="dry build"):
        e.encode_ids(ids[:2])
    with pytest.raises(EdgeStyleHipError, match=r"n = 3 is outside 1\.\.max_n = 2"):
        e.encode_ids(ids)
    with pytest.raises(EdgeStyleHipError, match="input_ids must be"):
        e.encode_ids(ids[:, :50])


def _attn_desc(Sq, Skv, d, heads=2, N=1):
    a = L.AttnDesc()
    a.q, a.k, a.v, a.o = 0x10000, 0x20000, 0x30000, 0x40000      # never dereferenced: every case here is refused before a launch
    a.N, a.heads, a.Sq, a.Skv, a.d = N, heads, Sq, Skv, d
    a.ldq = a.ldk = a.ldv = a.ldo = heads * d
    a.bsq, a.bsk, a.bsv, a.bso = Sq * heads * d, Skv * heads * d, Skv * heads * d, Sq * heads * d
    a.scale, a.dtype = d ** -0.5, L.ES_F16
    return a


@pytest.mark.parametrize("kw,text", [
    (dict(Sq=77, Skv=76, d=64), b"Sq != Skv"),
    (dict(Sq=129, Skv=129, d=64), b"S must be in 1..128"),
    (dict(Sq=77, Skv=77, d=40), b"unsupported head_dim (32, 64)"),
])
def test_attention_causal_refusals(kw, text):
    lib = L.load()
    a = _attn_desc(**kw)
    assert lib.es_attention_causal(C.byref(a), None) == -1
    assert text in lib.es_last_error()


def test_attention_causal_refuses_bad_strides_and_a_recording_plan():
    lib = L.load()
    a = _attn_desc(77, 77, 64)
    a.ldk = 2 * 64 + 4
    assert lib.es_attention_causal(C.byref(a), None) == -1 and b"strides" in lib.es_last_error()
    a = _attn_desc(77, 77, 64)
    a.ldv = 64                                                    # below heads * head_dim
    assert lib.es_attention_causal(C.byref(a), None) == -1 and b"row stride below" in lib.es_last_error()
    plan = lib.es_plan_create()
    try:
        assert lib.es_plan_begin_record(plan) == 0
        try:
            a = _attn_desc(77, 77, 64)
            assert lib.es_attention_causal(C.byref(a), None) == -1 and b"never part of a plan" in lib.es_last_error()
            assert lib.es_text_embed(0x1000, 0x2000, 0x3000, 0x4000, 77, 77, 128, 96, L.ES_F16, None) == -1
            assert b"never part of a plan" in lib.es_last_error()
        finally:
            lib.es_plan_end_record(plan)
        assert lib.es_plan_size(plan) == 0
    finally:
        lib.es_plan_destroy(plan)


def test_the_restatement_equals_transformers_in_fp32(tiny):
    """pins tests/text_ref.py, the reference of the GPU tests: plain functional ops in fp32 against CLIPTextModel's own forward"""
    cfg, model = tiny
    ids = R.token_ids(cfg, 3)
    with torch.no_grad():
        want = model(ids)[0]
        got = R.forward(R.bare(model.state_dict()), cfg, ids, "fp32")
        got64 = R.forward(R.bare(model.state_dict()), cfg, ids, "fp64")
    rel = float((got - want).abs().max() / want.abs().max())
    rel64 = float((got64 - want.double()).abs().max() / want.abs().max())
    print(f"restatement vs transformers: fp32 {rel:.3e}, fp64 {rel64:.3e} (max abs / max abs)")
    assert rel <= 1e-5 and rel64 <= 1e-5
    # the causal mask is in it: another id at position 40 leaves rows 0..39 as they were, in transformers and in the restatement
    ids2 = ids.clone()
    ids2[:, 40] = (ids2[:, 40] + 7) % cfg.vocab_size
    with torch.no_grad():
        want2, got2 = model(ids2)[0], R.forward(R.bare(model.state_dict()), cfg, ids2, "fp32")
    assert torch.equal(want2[:, :40], want[:, :40]) and not torch.equal(want2[:, 40:], want[:, 40:])
    assert torch.equal(got2[:, :40], got[:, :40]) and not torch.equal(got2[:, 40:], got[:, 40:])


def test_cli_flag_is_off_by_default():
    from edgestyle_amd.cli import parse_args
    assert parse_args([]).native_text_encoder is False
    assert parse_args(["--native_text_encoder"]).native_text_encoder is True

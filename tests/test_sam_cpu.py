"""The EfficientViT-SAM image encoder, the part that needs no GPU: the restatement (tests/sam_ref.py) against the reference's own fp64
outputs (tests/golden/ref_sam.safetensors), dry builds of es_sam_encoder with every refusal and its error text, the BatchNorm fold
against the unfolded computation, and the size rule of the preprocessing."""
import ctypes as C
import os

import pytest
import torch
from safetensors.torch import load_file

from edgestyle_amd import lib as L
from edgestyle_amd.lib import EdgeStyleHipError
from edgestyle_amd.sam import NativeSamImageEncoder, config_of_state_dict, sam_config
from tests import sam_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_sam.safetensors")


@pytest.fixture(scope="module")
def tiny():
    return R.random_state_dict(R.TINY, R.TINY_SEED), load_file(GOLDEN)


def tiny_config(**over):
    c = R.TINY
    kw = dict(widths=c["widths"], depths=c["depths"], head_width=c["head_width"], head_depth=c["head_depth"], out_dim=c["out_dim"])
    kw.update(over)
    size = kw.pop("image_size", 64)
    return sam_config("l2", size, **kw)


def test_abi_version_is_unchanged_and_the_new_symbols_resolve():
    lib = L.load()
    assert lib.es_abi_version() == 7 and L.ACT_GELU_TANH == 3
    for name in ("es_dwconv", "es_relu_linear_attention", "es_sam_neck_merge", "es_sam_preprocess_u8", "es_sam_encoder_create", "es_sam_encoder_destroy",
                 "es_sam_encoder_arena_bytes", "es_sam_encode", "es_sam_encode_u8_workspace_bytes", "es_sam_encode_u8"):
        assert name in L.SYMBOLS and getattr(lib, name)
    # the tiles that have no tanh-GELU epilogue keep refusing it, so the launch policy sends such launches to the 128-wide kernel
    assert lib.es_conv_gemm8p_form_ok(L.ACT_GELU_TANH, 320, 0, 4096, 0) == 0
    assert lib.es_conv_gemm8p_form_ok(L.ACT_NONE, 320, 0, 4096, 0) == 1


def test_the_regenerated_state_dict_is_the_one_the_fixture_was_written_from(tiny):
    sd, gold = tiny
    keys, sums = R.state_dict_sums(sd)
    assert len(keys) == gold["sd_sums"].shape[0] == 128
    assert torch.equal(sums, gold["sd_sums"]), "tests/sam_ref.py::random_state_dict no longer reproduces the fixture's weights"
    for S in (64, 128):
        assert torch.equal(R.probe_image(S, seed=100 + S), gold[f"x{S}"].float())


@pytest.mark.parametrize("S", [64, 128])
def test_restatement_in_fp64_equals_the_reference(tiny, S):
    """both sides are fp64 and differ in summation order only: 1e-9 leaves six decimal orders over fp64 rounding and stays six below fp32's"""
    sd, gold = tiny
    got, stats = R.forward(R.TINY, sd, gold[f"x{S}"].double(), "fp64", want_stats=True)
    R.assert_stats(stats)
    for k in ("stage2", "stage3", "stage4", "out"):
        ref = gold[f"{k}_{S}"] if k != "out" else gold[f"out_{S}"]
        assert got[k].shape == ref.shape and ref.dtype == torch.float64
        err = float((got[k] - ref).abs().max() / ref.abs().max())
        print(f"S={S} {k}: max|d| / max|ref| = {err:.2e}")
        assert err <= 1e-9


def test_full_width_generator_keeps_its_postcondition():
    sd = R.random_state_dict(R.SHALLOW, seed=5)
    _, stats = R.forward(R.SHALLOW, sd, R.probe_image(160, seed=9), "fp32", want_stats=True)
    R.assert_stats(stats)
    assert "backbone.stages.4.op_list.0.main.depth_conv.conv.weight" in sd and sd["backbone.stages.4.op_list.0.main.depth_conv.conv.weight"].shape[0] == 6144


def test_dry_builds_report_an_arena(tiny):
    sd, _ = tiny
    a = NativeSamImageEncoder.from_state_dict(sd, tiny_config(), device=None, max_n=1)
    b = NativeSamImageEncoder.from_state_dict({"image_encoder." + k: v for k, v in sd.items()}, tiny_config(), device=None, max_n=1)
    extra = dict(sd)
    extra["backbone.stages.0.op_list.0.norm.num_batches_tracked"] = torch.tensor(3)                  # int64: dropped by the binding
    extra["mask_decoder.iou_token.weight"] = torch.zeros(1, 256)                                     # unknown: ignored by the builder
    c = NativeSamImageEncoder.from_state_dict(extra, tiny_config(), device=None, max_n=1)
    assert a.arena_bytes == b.arena_bytes == c.arena_bytes > sum(v.numel() for v in sd.values() if v.dim() == 4) * 2
    assert NativeSamImageEncoder.from_state_dict(sd, tiny_config(), device=None, max_n=3).arena_bytes > a.arena_bytes
    assert NativeSamImageEncoder.from_state_dict(sd, tiny_config(image_size=128), device=None).arena_bytes > a.arena_bytes
    m = R.RefModule(R.TINY, sd)
    d = NativeSamImageEncoder.from_module(m, device=None, image_size=64)
    assert d.arena_bytes == a.arena_bytes and list(d.cfg.width) == list(R.TINY["widths"]) and list(d.cfg.depth) == [1] * 5
    assert d.cfg.out_dim == 8 and d.cfg.head_width == 64 and d.cfg.head_depth == 1
    with pytest.raises(EdgeStyleHipError, match="dry build"):
        a(torch.zeros(1, 3, 64, 64))
    holder = torch.nn.Module()                      # the drop-in: an nn.Module child can only be replaced by an nn.Module
    holder.image_encoder = m
    holder.image_encoder = NativeSamImageEncoder.from_module(holder.image_encoder, device=None, image_size=64)
    assert not list(holder.image_encoder.parameters()) and holder.eval().image_encoder.to("cpu") is holder.image_encoder


def test_l2_dry_build():
    cfg = R.model_config("l2")
    sd = R.random_state_dict(cfg, seed=1)
    # the reference's state_dict() has 508 keys: these, and one num_batches_tracked counter per BatchNorm
    assert len(sd) + sum(k.endswith("running_var") for k in sd) == 508
    weights = sum(v.numel() for v in sd.values())
    assert weights > 57e6
    e = NativeSamImageEncoder.from_state_dict(sd, sam_config("l2"), device=None, max_n=1)
    print(f"L2 at 512: {weights / 1e6:.1f} M parameters, arena {e.arena_bytes / 2 ** 20:.0f} MiB")
    assert 114e6 < e.arena_bytes < 2 ** 30
    auto = config_of_state_dict(sd)
    assert list(auto.depth) == [1, 2, 2, 8, 8] and auto.head_depth == 12 and list(auto.width) == [32, 64, 128, 256, 512]


def _refused(sd, cfg, match, **kw):
    with pytest.raises(EdgeStyleHipError, match=match):
        NativeSamImageEncoder.from_state_dict(sd, cfg, device=None, **kw)


def test_every_refusal_says_why(tiny):
    sd, _ = tiny
    _refused(sd, tiny_config(widths=(32, 32, 48, 64, 64)), r"width\[2\] = 48 must be a multiple of 32")
    _refused(sd, tiny_config(image_size=97), "image_size = 97 must be a multiple of 32 in 64..512")
    _refused(sd, tiny_config(image_size=544), "image_size = 544 must be a multiple of 32 in 64..512")
    _refused(sd, tiny_config(), "max_n must be in 1..1024", max_n=0)
    _refused(sd, tiny_config(), "fp16 or bf16", dtype=torch.float32)
    bad = tiny_config()
    bad.qkv_dim = 16
    _refused(sd, bad, "qkv_dim must be 32")
    for key in ("backbone.stages.4.op_list.1.context_module.main.aggreg.0.1.weight", "neck.middle.op_list.0.main.point_conv.norm.running_var",
                "backbone.stages.3.op_list.0.main.depth_conv.conv.weight", "norm.bias"):
        _refused({k: v for k, v in sd.items() if k != key}, tiny_config(), "missing key '" + key.replace(".", r"\.") + "'")
    key = "backbone.stages.1.op_list.0.main.spatial_conv.conv.weight"
    wrong = dict(sd)
    wrong[key] = sd[key][:, :, :, :2].contiguous()
    _refused(wrong, tiny_config(), "size mismatch for '" + key.replace(".", r"\.") + r"': \(512,32,3,2\) vs \(512,32,3,3\)")
    _refused(sd, tiny_config(depths=(1, 1, 2, 1, 1)), r"missing key 'backbone\.stages\.2\.op_list\.2\.main\.spatial_conv\.conv\.weight'")


def test_bn_fold_equals_the_unfolded_computation(tiny):
    """W g / sqrt(v + eps), b' = beta + (b - mean) g / sqrt(v + eps), as the builder forms them in fp64, against conv -> BatchNorm in fp64;
    the builder's own arithmetic is held to the reference by the GPU tier (the golden outputs come from the unfolded modules)"""
    sd, _ = tiny
    p = "backbone.stages.1.op_list.0.main.spatial_conv"
    w = sd[p + ".conv.weight"].double()
    g, bt, mu, var = (sd[p + ".norm." + k].double() for k in ("weight", "bias", "running_mean", "running_var"))
    x = torch.randn(2, 32, 9, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    y = torch.nn.functional.conv2d(x, w, None, 2, 1)
    unfolded = (y - mu.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + 1e-6) * g.view(1, -1, 1, 1) + bt.view(1, -1, 1, 1)
    sc = g / torch.sqrt(var + 1e-6)
    folded = torch.nn.functional.conv2d(x, w * sc.view(-1, 1, 1, 1), bt - mu * sc, 2, 1)
    assert float((folded - unfolded).abs().max() / unfolded.abs().max()) < 1e-13
    assert float((sc - 1).abs().max()) > 0.2 and float(mu.abs().max()) > 0.1          # the fold is not trivial


def test_resize_shape_rule_rounds_both_ways():
    lib = L.load()
    hw = (C.c_int32 * 2)()
    cases = [(200, 300, 512), (300, 200, 512), (97, 131, 512), (512, 512, 512), (512, 300, 512), (1000, 3, 512), (341, 1024, 512), (683, 1024, 512),
             (1023, 1024, 512), (5, 7, 64), (333, 1000, 256), (667, 1000, 256)]
    ups = 0
    for h, w, S in cases:
        lib.es_sam_resize_shape(h, w, S, hw)
        want = (h, w) if max(h, w) == S else R.sam_resize_shape(h, w, S)
        assert (hw[0], hw[1]) == want, (h, w, S, tuple(hw), want)
        short = min(h, w) * S / max(h, w)
        ups += int(min(want) > short)
    assert 0 < ups < len(cases)           # some short sides round up, some down
    lib.es_sam_resize_shape(300, 200, 512, hw)
    assert tuple(hw) == (512, 341)

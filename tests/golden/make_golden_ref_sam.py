#!/usr/bin/env python
"""Fixture for the EfficientViT-SAM image encoder, produced by the reference's OWN classes, in the build container only.

`efficientvit/` of the reference is vendored and torch-only, but its package `__init__`s and `sam.py` import `segment_anything`,
which is not installed.  This script puts empty stand-ins for the three package `__init__`s (`efficientvit`, `efficientvit.models`,
`efficientvit.models.efficientvit`) into `sys.modules` with their real `__path__`, so that `backbone.py`, `nn/` and `utils/` import as
they are, and takes `SamNeck` and `EfficientViTSamImageEncoder` out of `sam.py` with `ast` (as make_golden_ref_fusion.py does for the
fusion block) - no stand-in for anything that computes.  Nothing of the reference travels: what is committed is tensors.

  ref_sam.safetensors   the tiny network tests/sam_ref.py::TINY (widths 32,32,64,64,64, one block per stage, head_width 64, out_dim 8,
                        every norm's eps 1e-6 as create_sam_model sets it).  Its state dict is tests/sam_ref.py::random_state_dict(TINY,
                        TINY_SEED): the reference's module takes it with load_state_dict (no key unexpected, none missing but the
                        num_batches_tracked counters), which pins every key and shape to the reference.  A state dict of these widths is 2.5 MB, more than a committed file may hold, so it is regenerated
                        from the seed (bit for bit: see sam_ref.py) and the fixture stores every tensor's sum and sum of squares
                        (`sd_sums`, keys sorted) instead.  The two inputs (S = 64: 4 tokens in stage4, every map upsampled;
                        S = 128) are stored in bf16, which holds them exactly; stored in fp64: the reference's stage2 / stage3 / stage4 maps and its output for each.

    python tests/golden/make_golden_ref_sam.py            (needs /root/reference; a few seconds)
"""
import ast
import importlib
import os
import sys
import types

import torch
from torch import nn
from safetensors.torch import save_file

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import sam_ref as R                           # noqa: E402

REF = "/root/reference"
SAM_PY = os.path.join(REF, "efficientvit/models/efficientvit/sam.py")
WANT = ("SamNeck", "EfficientViTSamImageEncoder")


def reference_classes():
    for name, rel in (("efficientvit", "efficientvit"), ("efficientvit.models", "efficientvit/models"),
                      ("efficientvit.models.efficientvit", "efficientvit/models/efficientvit")):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, rel)]
        sys.modules[name] = m
    backbone = importlib.import_module("efficientvit.models.efficientvit.backbone")
    nnmod = importlib.import_module("efficientvit.models.nn")
    tree = ast.parse(open(SAM_PY).read(), SAM_PY)
    picked = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in WANT]
    assert sorted(n.name for n in picked) == sorted(WANT)
    ns = {"torch": torch, "nn": nn, "List": list, "EfficientViTBackbone": backbone.EfficientViTBackbone,
          "EfficientViTLargeBackbone": backbone.EfficientViTLargeBackbone}
    for k in ("DAGBlock", "OpSequential", "ConvLayer", "UpSampleLayer", "MBConv", "FusedMBConv", "ResidualBlock", "IdentityLayer", "build_norm"):
        ns[k] = getattr(nnmod, k)
    exec(compile(ast.fix_missing_locations(ast.Module(body=picked, type_ignores=[])), SAM_PY, "exec"), ns)
    return backbone.EfficientViTLargeBackbone, ns["SamNeck"], ns["EfficientViTSamImageEncoder"], nnmod.set_norm_eps


def main():
    Backbone, Neck, Encoder, set_norm_eps = reference_classes()
    cfg = R.TINY
    w = cfg["widths"]
    enc = Encoder(Backbone(list(w), list(cfg["depths"]), qkv_dim=cfg["qkv_dim"]),
                  Neck(fid_list=["stage4", "stage3", "stage2"], in_channel_list=[w[4], w[3], w[2]], head_width=cfg["head_width"],
                       head_depth=cfg["head_depth"], expand_ratio=1, middle_op="fmbconv", out_dim=cfg["out_dim"]))
    # the reference builds its final norm with 256 features whatever out_dim is (sam.py:182): rebuilt for the fixture's out_dim
    enc.norm = type(enc.norm)(cfg["out_dim"])
    set_norm_eps(enc, cfg["bn_eps"])
    sd = R.random_state_dict(cfg, R.TINY_SEED)
    ref_keys = {k for k in enc.state_dict() if not k.endswith("num_batches_tracked")}
    assert ref_keys == set(sd), (sorted(ref_keys - set(sd))[:5], sorted(set(sd) - ref_keys)[:5])
    res = enc.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.endswith("num_batches_tracked") for k in res.missing_keys), res
    enc = enc.double().eval()
    keys, sums = R.state_dict_sums(sd)
    out = {"sd_sums": sums}
    torch.set_num_threads(8)
    with torch.no_grad():
        for S in (64, 128):
            x = R.probe_image(S, seed=100 + S).double()
            _, stats = R.forward(cfg, sd, x, "fp32", want_stats=True)
            R.assert_stats(stats)
            fd = enc.backbone(x)
            y = enc(x)
            out[f"x{S}"] = x.to(torch.bfloat16).contiguous()          # exact: probe_image rounds to bf16
            for s in (2, 3, 4):
                out[f"stage{s}_{S}"] = fd[f"stage{s}"].contiguous()
            out[f"out_{S}"] = y.contiguous()
            mine = R.forward(cfg, sd, x, "fp64")
            for k, t in (("stage2", fd["stage2"]), ("stage3", fd["stage3"]), ("stage4", fd["stage4"]), ("out", y)):
                print(f"S={S} {k}: shape {tuple(t.shape)} std {float(t.std()):.3f}  restatement max|d| / max|ref| "
                      f"{float((mine[k] - t).abs().max() / t.abs().max()):.2e}", flush=True)
    print(len(keys), "keys; first", keys[:3])
    path = os.path.join(HERE, "ref_sam.safetensors")
    save_file(out, path)
    print("wrote ref_sam.safetensors", os.path.getsize(path) >> 10, "KiB")


if __name__ == "__main__":
    main()

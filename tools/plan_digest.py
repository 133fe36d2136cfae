#!/usr/bin/env python
"""What both hosts build, as digests that two commits can be compared by (no GPU: the library's dry recorder): for each of the six plans
of a context, the number of recorded calls, a SHA-256 over the calls with pointer fields reduced to null / set (native.plan_records, as
tests/helpers.py diff_plans reads them) and a SHA-256 over the constant blobs behind them (tests/helpers.py plan_constants).

  native leg: es_load_weights (device = -2) for every configuration of tests/test_load_weights_cpu.py, with the arena a real build
              of it would allocate (es_ctx_arena_bytes);
  python leg: the model walk of engine.py / models.py (tests/helpers.py python_dry_context) for the six-slot context, a single net and
              guess_mode, once per setting of the switches that pick its branches.  Both modules read their switches at import, so
              every setting is a child process of this tool.

A change to either builder or to the launch policy that is meant to move nothing prints the same lines before and after.

    python tools/plan_digest.py > after.txt        (and the same at the parent commit; diff the two)
"""
import dataclasses
import hashlib
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from edgestyle_amd import config as Cfg, lib as L, weights as W  # noqa: E402
from edgestyle_amd.native import NativeContext, plan_records  # noqa: E402
from tests.helpers import make_weights, quantize, plan_constants, python_dry_context  # noqa: E402

SWITCHES = ("ES_LN_FOLD", "ES_FFO_FOLD", "ES_SHORTCUT_FOLD", "ES_CHAIN_MODE")
SETTINGS = [("default switches", {}),
            ("folds off", dict(ES_LN_FOLD="0", ES_FFO_FOLD="0", ES_SHORTCUT_FOLD="0")),
            ("ES_LN_FOLD=qk", dict(ES_LN_FOLD="qk")),
            ("ES_CHAIN_MODE=serial", dict(ES_CHAIN_MODE="serial"))]


def print_plans(name, lib, ctx):
    for which in range(L.PLAN_COUNT):
        size = lib.es_ctx_plan_size(ctx, which)
        if size < 0:
            print(f"{name}: plan {which}: not recorded")
            continue
        calls, blobs = hashlib.sha256(), hashlib.sha256()
        for kind, rec in plan_records(lib, ctx, which):
            calls.update(kind.to_bytes(8, "little", signed=True) + len(rec).to_bytes(8, "little") + rec)
        consts = plan_constants(lib, ctx, which)
        for c in consts:
            blobs.update(len(c).to_bytes(8, "little") + c)
        print(f"{name}: plan {which}: {size} calls {calls.hexdigest()}  {len(consts)} blobs, {sum(map(len, consts))} bytes {blobs.hexdigest()}")


def model():
    ucfg, vcfg = dataclasses.replace(Cfg.tiny_unet(), sample_size=64), Cfg.tiny_vae()
    ws = {k: quantize(v) for k, v in make_weights(ucfg, vcfg, seed=3).items()}
    ws["lora_stack"] = quantize(W.random_state_dict(W.controllora_saved_shapes(ucfg, 4, uses_vae=False), 3, "controlnet_2."))
    return ucfg, vcfg, ws


def native_leg():
    ucfg, vcfg, ws = model()
    single = dict(controlnets=(("openpose", 0),), net_of_cond=(0,))
    configs = [("B=1 guidance T=6", dict(batch_size=1, guidance=True, num_inference_steps=6)),
               ("B=2 no guidance T=3", dict(batch_size=2, guidance=False, num_inference_steps=3)),
               ("two nets", dict(num_inference_steps=4, controlnets=(("lora0", 1), ("openpose", 0)), net_of_cond=(0, 1, 0, 1, 0, 1))),
               ("three nets, own conv stack", dict(num_inference_steps=4, controlnets=(("lora_stack", 2), ("openpose", 0), ("lora1", 1)), net_of_cond=(0, 1, 2, 1, 2, 2))),
               ("single net", dict(num_inference_steps=4, **single)),
               ("guess B=1 guidance", dict(batch_size=1, guidance=True, num_inference_steps=4, guess_mode=True)),
               ("guess B=2 no guidance", dict(batch_size=2, guidance=False, num_inference_steps=4, guess_mode=True)),
               ("guess single net", dict(batch_size=1, guidance=True, num_inference_steps=4, guess_mode=True, **single)),
               ("bf16", dict(num_inference_steps=4, dtype=torch.bfloat16))]
    lib = L.load()
    for name, kw in configs:
        wsn = {k: v for k, v in ws.items() if k != "fusion"} if len(kw.get("net_of_cond", ())) == 1 else ws
        nat = NativeContext(wsn, ucfg, vcfg, device=-2, **kw)
        print(f"{name}: arena {lib.es_ctx_arena_bytes(nat.ctx)} bytes")
        print_plans(name, lib, nat.ctx)
        nat.close()


def python_leg(setting):
    ucfg, vcfg, ws = model()
    for name, kw in (("six slots", {}), ("single net", dict(controlnets=(("openpose", 0),), net_of_cond=(0,))), ("guess", dict(guess=True))):
        lib, ctx, keep = python_dry_context(ws, ucfg, vcfg, **kw)
        print_plans(f"python host, {setting}, {name}", lib, ctx)
        lib.es_ctx_destroy(ctx)
        del keep


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--python-leg":
        return python_leg(sys.argv[2])
    native_leg()
    sys.stdout.flush()
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    for setting, env in SETTINGS:
        subprocess.run([sys.executable, os.path.abspath(__file__), "--python-leg", setting], env={**base, **env}, check=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What es_load_weights builds, as digests that two commits can be compared by (no GPU: device = -2, the dry recorder): for every
configuration of tests/test_load_weights_cpu.py and each of the six plans, the number of recorded calls, a SHA-256 over the calls with
pointer fields reduced to null / set (native.plan_records, as tests/helpers.py diff_plans reads them) and a SHA-256 over the constant
blobs behind them (tests/helpers.py plan_constants).  A change to the native builder or the launch policy that is meant to move nothing
prints the same lines before and after; the Python host is not involved.

    python tools/plan_digest.py > after.txt        (and the same at the parent commit; diff the two)
"""
import dataclasses
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from edgestyle_amd import config as Cfg, lib as L, weights as W  # noqa: E402
from edgestyle_amd.native import NativeContext, plan_records  # noqa: E402
from tests.helpers import make_weights, quantize, plan_constants  # noqa: E402


def main():
    ucfg, vcfg = dataclasses.replace(Cfg.tiny_unet(), sample_size=64), Cfg.tiny_vae()
    ws = {k: quantize(v) for k, v in make_weights(ucfg, vcfg, seed=3).items()}
    ws["lora_stack"] = quantize(W.random_state_dict(W.controllora_saved_shapes(ucfg, 4, uses_vae=False), 3, "controlnet_2."))
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
        for which in range(L.PLAN_COUNT):
            if nat.plan_size(which) < 0:
                print(f"{name}: plan {which}: not recorded")
                continue
            calls, blobs = hashlib.sha256(), hashlib.sha256()
            for kind, rec in plan_records(lib, nat.ctx, which):
                calls.update(kind.to_bytes(8, "little", signed=True) + len(rec).to_bytes(8, "little") + rec)
            consts = plan_constants(lib, nat.ctx, which)
            for c in consts:
                blobs.update(len(c).to_bytes(8, "little") + c)
            print(f"{name}: plan {which}: {nat.plan_size(which)} calls {calls.hexdigest()}  {len(consts)} blobs, {sum(map(len, consts))} bytes {blobs.hexdigest()}")
        nat.close()


if __name__ == "__main__":
    main()

"""One request of the CLIP prompt picker, timed: NativeBestEmbeddings (edgestyle_amd/clip.py, csrc/clip.hip) on the GPU against
prompts.BestEmbeddings over transformers on the host's threads - what the parent path runs per request (model/utils.py:647-684).

ViT-L/14 widths (CLIPModel's defaults scaled to openai/clip-vit-large-patch14: vision 1024 x 24 layers x 16 heads, text 768 x 12 x 12,
projection 768) with seeded random weights, one 768 x 1024 photo, 270 + 190 synthetic words over a synthetic character-level tokenizer.
The native bank (the 460 text forwards) is built once, beforehand, and its build time is reported on its own; the host path runs the text
tower inside every request, as the reference does.

    python tools/clip_picker_bench.py [--reps 20] [--warmup 3] [--host_reps 3] [--dtype fp16] [--small] [--suffix TEXT]

Native requests are timed twice: device events around es_clip_pick alone (the photo already on the device), and a host clock around the
whole NativeBestEmbeddings call (upload, workspace allocation, the call, top-k read back, ending in a synchronise).  Prints every
repetition's spread (min / median / max).
The last native section times photo -> text states `ehs`: NativeBestEmbeddings.encode_prompts (es_clip_pick -> es_prompt_assemble ->
es_text_encode_dev on one stream, tokenizer.NativeCLIPTokenizer) against the path it replaces - picker(images), the transformers
tokenizer over the string, encode_ids - both from the photo on the host to a synchronise, host clock, and checks that the two give
the same bits.  --host_reps 0 skips the transformers-on-the-host section.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def synthetic_tokenizer(d):
    from transformers import CLIPTokenizer
    chars = [chr(c) for c in range(ord("a"), ord("z") + 1)] + [",", "."]
    vocab = {}
    for ch in chars:
        vocab[ch] = len(vocab)
    for ch in chars:
        vocab[ch + "</w>"] = len(vocab)
    vocab["<|startoftext|>"] = len(vocab)
    vocab["<|endoftext|>"] = len(vocab)
    with open(os.path.join(d, "vocab.json"), "w") as f:
        json.dump(vocab, f)
    with open(os.path.join(d, "merges.txt"), "w") as f:
        f.write("#version: 0.2\n")
    return CLIPTokenizer(os.path.join(d, "vocab.json"), os.path.join(d, "merges.txt"), model_max_length=77), vocab


def words(n, seed):
    g = np.random.default_rng(seed)
    out = set()
    while len(out) < n:
        out.add("".join(chr(ord("a") + int(c)) for c in g.integers(0, 26, size=int(g.integers(3, 9)))))
    return sorted(out)


def spread(ms):
    return f"min {min(ms):.3f}  median {statistics.median(ms):.3f}  max {max(ms):.3f} ms over {len(ms)} runs"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host_reps", type=int, default=3)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--suffix", default="a photo of a person wearing it, best quality", help="the caller's prompt suffix of the photo -> ehs section")
    ap.add_argument("--small", action="store_true", help="a 2-layer model of the tests' widths: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_picker_bench needs a GPU (a timing taken anywhere else says nothing)")
    from PIL import Image
    from transformers import CLIPConfig, CLIPImageProcessor, CLIPModel, CLIPProcessor
    from edgestyle_amd.clip import NativeBestEmbeddings
    from edgestyle_amd.prompts import BestEmbeddings
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
    tmp = tempfile.mkdtemp()
    tok, vocab = synthetic_tokenizer(tmp)
    tkw = dict(vocab_size=len(vocab), bos_token_id=vocab["<|startoftext|>"], eos_token_id=vocab["<|endoftext|>"], pad_token_id=vocab["<|endoftext|>"])
    if args.small:
        tkw.update(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256)
        vkw = dict(image_size=56, patch_size=14, hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256)
        cfg = CLIPConfig(text_config=tkw, vision_config=vkw, projection_dim=64)
    else:
        tkw.update(hidden_size=768, num_attention_heads=12, num_hidden_layers=12, intermediate_size=3072)
        vkw = dict(image_size=224, patch_size=14, hidden_size=1024, num_attention_heads=16, num_hidden_layers=24, intermediate_size=4096)
        cfg = CLIPConfig(text_config=tkw, vision_config=vkw, projection_dim=768)
    torch.manual_seed(0)
    model = CLIPModel(cfg).eval()
    colors, items = words(270, 1), words(190, 2)
    g = np.random.default_rng(3)
    photo = g.integers(0, 256, size=(1024, 768, 3), dtype=np.uint8)          # 768 wide, 1024 high
    pil = Image.fromarray(photo)
    rr = cfg.vision_config.image_size
    print(f"model: vision {vkw['hidden_size']} x {vkw['num_hidden_layers']} layers, text {tkw['hidden_size']} x {tkw['num_hidden_layers']}, "
          f"projection {cfg.projection_dim}; {len(colors)} + {len(items)} words; photo {photo.shape[1]} x {photo.shape[0]}; {args.dtype}; "
          f"device {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}")

    # ---- native: the bank once, then requests ----
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    be = NativeBestEmbeddings.from_module(model, tok, colors=colors, clothing_items=items, dtype=dtype, device="cuda", max_images=1, text_batch=64)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    print(f"native: build (image tower packed and uploaded + bank: 460 words through the text encoder in runs of 64): {build_ms:.1f} ms, once")
    try:
        for _ in range(args.warmup):
            native_prompt = be([pil])[0]
        whole = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            be([pil])
            torch.cuda.synchronize()
            whole.append((time.perf_counter() - t0) * 1e3)
        print(f"native: whole request (upload, es_clip_pick, read back), host clock: {spread(whole)}")
        # es_clip_pick alone, device events
        import ctypes as C
        from edgestyle_amd import lib as L
        dev = torch.from_numpy(photo).to("cuda")
        imgs = (L.ImageU8 * 1)()
        imgs[0].data, imgs[0].height, imgs[0].width, imgs[0].channels, imgs[0].row_stride = dev.data_ptr(), photo.shape[0], photo.shape[1], 3, dev.stride(0)
        need = be.lib.es_clip_pick_workspace_bytes(be._vision, imgs, 1)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        W = len(colors) + len(items)
        seg = (C.c_int32 * 2)(len(colors), W)
        logits, probs = torch.empty((1, W), device="cuda"), torch.empty((1, W), device="cuda")
        topk = torch.empty((1, 2, 2), dtype=torch.int32, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def pick():
            L.check(be.lib.es_clip_pick(be._vision, be._bank, imgs, 1, be.logit_scale_exp, seg, 2, 2, C.c_void_p(logits.data_ptr()), C.c_void_p(probs.data_ptr()),
                                        C.c_void_p(topk.data_ptr()), C.c_void_p(ws.data_ptr()), need, stream), "es_clip_pick")
        for _ in range(args.warmup):
            pick()
        ev = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            pick()
            b.record()
            b.synchronize()
            ev.append(a.elapsed_time(b))
        print(f"native: es_clip_pick alone (photo on the device), device events: {spread(ev)}")
    finally:
        be.close()

    # ---- photo -> ehs: the device chain against picker -> string -> transformers tokenizer -> encode_ids ----
    from edgestyle_amd.text import NativeCLIPTextEncoder
    from edgestyle_amd.tokenizer import NativeCLIPTokenizer
    ntok = NativeCLIPTokenizer.from_pretrained(tmp, model_max_length=77)
    be2 = NativeBestEmbeddings.from_module(model, ntok, colors=colors, clothing_items=items, dtype=dtype, device="cuda", max_images=1, text_batch=64)
    text_sd = {k[len("text_model."):]: v for k, v in model.state_dict().items() if k.startswith("text_model.")}       # the text tower stands in for SD1.5's
    enc = NativeCLIPTextEncoder.from_state_dict(text_sd, cfg.text_config, dtype=dtype, device="cuda", max_n=1)
    try:
        def parent_path():
            text = be2([pil])[0] + " " + args.suffix
            return enc.encode_ids(tok([text], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids)

        def device_path():
            return be2.encode_prompts([pil], enc, suffix=args.suffix)
        timings = {}
        for name, fn in (("parent", parent_path), ("device", device_path)):
            for _ in range(args.warmup):
                fn()
            ms = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            timings[name] = ms
        same = torch.equal(parent_path(), device_path())
        print(f"photo -> ehs, parent path (picker call, transformers tokenizer, encode_ids), host clock: {spread(timings['parent'])}")
        print(f"photo -> ehs, encode_prompts (es_clip_pick -> es_prompt_assemble -> es_text_encode_dev), host clock: {spread(timings['device'])}")
        print(f"photo -> ehs: the two paths give the same bits: {same}; ratio of medians, parent / encode_prompts: "
              f"{statistics.median(timings['parent']) / statistics.median(timings['device']):.2f}")
    finally:
        enc.close()
        be2.close()
    if args.host_reps < 1:
        return

    # ---- the parent path: prompts.BestEmbeddings over transformers on the host ----
    proc = CLIPProcessor(image_processor=CLIPImageProcessor(size={"shortest_edge": rr}, crop_size={"height": rr, "width": rr}), tokenizer=tok)
    host = BestEmbeddings(model, proc, colors=colors, clothing_items=items)
    host_prompt = host([pil])[0]                                             # warm-up
    hs = []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        host([pil])
        hs.append((time.perf_counter() - t0) * 1e3)
    print(f"host:   prompts.BestEmbeddings (CLIPProcessor + CLIPModel fp32 on {torch.get_num_threads()} threads, both lists), host clock: {spread(hs)}")
    print(f"prompts: native {native_prompt!r}; host {host_prompt!r} (random weights: near-ties may rank differently in {args.dtype})")
    print(f"ratio of medians, host / native whole request: {statistics.median(hs) / statistics.median(whole):.1f}")


if __name__ == "__main__":
    main()

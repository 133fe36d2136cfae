"""The CLIP prompt picker on the HIP path: a ctypes driver of es_clip_vision / es_clip_bank / es_clip_pick (include/edgestyle_hip.h,
csrc/clip.hip).

`NativeBestEmbeddings` has the call surface of `prompts.BestEmbeddings` (model/utils.py:647-684): `picker(images)` gives one prompt
"<prefix>, c1, c2, i1, i2" per garment image.  The words' text embeddings are computed once, at construction, by the library's text
encoder into a bank on the device; a call then resizes the photos (Pillow's bicubic, transformers' crop), runs the image tower and
scores against the bank, all on the GPU.  The tokenizer is the caller's: transformers' CLIPTokenizer, or the library's own
(tokenizer.NativeCLIPTokenizer).  With the latter `encode_prompts` goes from the photos to the text states `ehs` without the host:
es_clip_pick -> es_prompt_assemble -> es_text_encode_dev on one stream.  There is no fallback: a refused configuration raises."""
import ctypes as C
import json
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import lib as L
from .lib import EdgeStyleHipError
from .prompts import DEFAULT_CLOTHING_ITEMS, DEFAULT_COLORS
from .text import NativeCLIPTextEncoder, _ACTS, _DT, state_dict_descriptors
from .tokenizer import NativeCLIPTokenizer

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
MAX_K = 8


def _get(config, key, default=None):
    if isinstance(config, dict):
        return config.get(key, default)
    return getattr(config, key, default)


def vision_config(config, projection_dim: int, image_mean=OPENAI_CLIP_MEAN, image_std=OPENAI_CLIP_STD) -> L.ClipVisionConfig:
    """CLIPVisionConfig (or a dict of its attribute names) -> es_clip_vision_config"""
    act = _get(config, "hidden_act")
    if act not in _ACTS:
        raise EdgeStyleHipError(f"NativeBestEmbeddings implements hidden_act 'quick_gelu' (OpenAI CLIP), not {act!r}")
    cfg = L.ClipVisionConfig(image_size=_get(config, "image_size"), patch_size=_get(config, "patch_size"), hidden=_get(config, "hidden_size"),
                             heads=_get(config, "num_attention_heads"), layers=_get(config, "num_hidden_layers"),
                             intermediate=_get(config, "intermediate_size"), projection_dim=int(projection_dim),
                             ln_eps=float(_get(config, "layer_norm_eps")), act=_ACTS[act])
    for c in range(3):
        cfg.image_mean[c], cfg.image_std[c] = float(image_mean[c]), float(image_std[c])
    return cfg


def eos_positions(input_ids: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    """the pooled position of every row as transformers' CLIP text model picks it: the argmax of the ids where the config has the legacy
    eos_token_id == 2, otherwise the first occurrence of eos_token_id"""
    ids = input_ids.to("cpu", torch.int64)
    if eos_token_id == 2:
        return ids.to(torch.int).argmax(dim=-1).to(torch.int32)
    return (ids == eos_token_id).int().argmax(dim=-1).to(torch.int32)


def image_bytes(img) -> np.ndarray:
    """a PIL image, or a uint8 HWC array / tensor with 3 or 4 channels -> a C-contiguous uint8 [H, W, 3 | 4] array (alpha is dropped by
    the library, as es_image_u8 says)"""
    if torch.is_tensor(img):
        img = img.detach().cpu().numpy()
    elif not isinstance(img, np.ndarray):
        img = np.array(img.convert("RGB") if img.mode not in ("RGB", "RGBA") else img)        # a copy: torch wants writable memory
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (3, 4):
        raise EdgeStyleHipError(f"an image must be uint8 [H, W, 3 | 4], got {img.dtype} {tuple(img.shape)}")
    return np.ascontiguousarray(img)


def check_comma_join(tokenizer, prefix: str, words: Sequence[str]) -> None:
    """Once per vocabulary, on the host, with the native tokenizer: es_prompt_assemble joins the pieces with spaces, the reference's
    string (and NativeBestEmbeddings.__call__'s) with ", ".  The two tokenise alike unless a piece ends with punctuation, which
    then runs into the comma ("t-shirt!, x" and "t-shirt! , x" differ): such a word is named here."""
    for w in [prefix] + list(words):
        if tokenizer.tokenize_ids(f"{prefix}, {w}, {w}") != tokenizer.tokenize_ids(f"{prefix} , {w} , {w}"):
            raise EdgeStyleHipError(f"the word {w!r} tokenises differently inside the comma-joined prompt than on its own (it ends with "
                                    "punctuation): encode_prompts could not give the ids of the prompt __call__ returns")


class NativeBestEmbeddings:
    """clip_state_dict: CLIPModel's state dict; clip_config: its CLIPConfig (or a dict with text_config, vision_config, projection_dim);
    tokenizer: the CLIPTokenizer of the checkpoint.  max_images: the most images one call scores."""

    def __init__(self, clip_state_dict, clip_config, tokenizer, colors: Optional[Sequence[str]] = None,
                 clothing_items: Optional[Sequence[str]] = None, prefix: str = "edgestyle", dtype=torch.float16, device="cuda",
                 image_mean=OPENAI_CLIP_MEAN, image_std=OPENAI_CLIP_STD, max_images: int = 4, text_batch: int = 32):
        if dtype not in _DT:
            raise EdgeStyleHipError(f"NativeBestEmbeddings computes in fp16 or bf16, not {dtype}")
        self.lib = L.load()
        self._vision = self._bank = None
        self.dtype, self.prefix, self.tokenizer = dtype, prefix, tokenizer
        self.colors = list(colors) if colors is not None else list(DEFAULT_COLORS)
        self.clothing_items = list(clothing_items) if clothing_items is not None else list(DEFAULT_CLOTHING_ITEMS)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise EdgeStyleHipError(f"NativeBestEmbeddings runs on a GPU, not on {self.device} (there is no CPU fallback)")
        self.device = torch.device("cuda", self.device.index if self.device.index is not None else torch.cuda.current_device())
        self.max_images, self.text_batch = int(max_images), int(text_batch)
        self._sd = {k: v for k, v in clip_state_dict.items() if torch.is_tensor(v) and v.is_floating_point()}
        self._text_cfg, vcfg = _get(clip_config, "text_config"), _get(clip_config, "vision_config")
        self.proj = int(_get(clip_config, "projection_dim"))
        self.eos_token_id = int(_get(self._text_cfg, "eos_token_id"))
        self.text_hidden, self.text_len = int(_get(self._text_cfg, "hidden_size")), int(_get(self._text_cfg, "max_position_embeddings"))
        self.logit_scale_exp = float(self._sd["logit_scale"].detach().double().exp())
        self.cfg = vision_config(vcfg, self.proj, image_mean, image_std)
        with torch.cuda.device(self.device):
            desc, keep = state_dict_descriptors({k: v for k, v in self._sd.items() if k.startswith("vision_model.") or k == "visual_projection.weight"})
            h = C.c_void_p()
            L.check(self.lib.es_clip_vision_create(C.byref(desc), C.byref(self.cfg), _DT[dtype], self.max_images, self.device.index, C.byref(h)),
                    "es_clip_vision_create")
            self._vision = h
            del keep
            try:
                self._bank = self._build_bank(self.colors + self.clothing_items)
            except Exception:
                self.close()
                raise
        self._segments = [len(self.colors), len(self.colors) + len(self.clothing_items)]
        self._tables = {}
        if isinstance(tokenizer, NativeCLIPTokenizer):
            try:
                check_comma_join(tokenizer, self.prefix, self.colors + self.clothing_items)
            except Exception:
                self.close()
                raise

    @classmethod
    def from_module(cls, model, tokenizer, **kw):
        """model: a transformers CLIPModel (its forward is not run)"""
        return cls(model.state_dict(), model.config, tokenizer, **kw)

    @classmethod
    def from_vocab_file(cls, clip_state_dict, clip_config, tokenizer, path: str, **kw):
        with open(path) as f:
            v = json.load(f)
        return cls(clip_state_dict, clip_config, tokenizer, colors=v["colors"], clothing_items=v["clothing_items"], **kw)

    @classmethod
    def from_pretrained(cls, directory: str, vocab_file: Optional[str] = None, **kw):
        """a CLIPModel directory as transformers saves it (config.json, model.safetensors, the tokenizer's and the processor's files)"""
        from safetensors.torch import load_file
        from transformers import CLIPConfig, CLIPTokenizer
        config = CLIPConfig.from_pretrained(directory)
        sd = load_file(os.path.join(directory, "model.safetensors"))
        pre = os.path.join(directory, "preprocessor_config.json")
        if os.path.exists(pre):
            with open(pre) as f:
                p = json.load(f)
            kw.setdefault("image_mean", p.get("image_mean", OPENAI_CLIP_MEAN))
            kw.setdefault("image_std", p.get("image_std", OPENAI_CLIP_STD))
        tok = CLIPTokenizer.from_pretrained(directory)
        if vocab_file:
            return cls.from_vocab_file(sd, config, tok, vocab_file, **kw)
        return cls(sd, config, tok, **kw)

    # ---- the word side: once per vocabulary ----
    def _build_bank(self, words: Sequence[str]) -> C.c_void_p:
        """text tower -> pooled rows -> text_projection -> unit rows, in runs of the text encoder's max_n.  The text encoder lives only here."""
        words = list(words)
        if not words:
            raise EdgeStyleHipError("an empty word list")
        ids = self.tokenizer(words, padding="max_length", max_length=self.text_len, truncation=True, return_tensors="pt").input_ids
        eos = eos_positions(ids, self.eos_token_id)
        nmax = min(self.text_batch, len(words))
        text_sd = {k[len("text_model."):]: v for k, v in self._sd.items() if k.startswith("text_model.")}
        desc, keep = state_dict_descriptors({"text_projection.weight": self._sd["text_projection.weight"]})
        bank = C.c_void_p()
        L.check(self.lib.es_clip_bank_create(C.byref(desc), self.text_hidden, self.proj, len(words), nmax, _DT[self.dtype], self.device.index,
                                             C.byref(bank)), "es_clip_bank_create")
        del keep
        enc = None
        try:
            enc = NativeCLIPTextEncoder(text_sd, self._text_cfg, dtype=self.dtype, device=self.device, max_n=nmax)
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            for a in range(0, len(words), nmax):
                ehs = enc.encode_ids(ids[a:a + nmax])
                e = eos[a:a + nmax].contiguous()
                L.check(self.lib.es_clip_text_pool(bank, C.c_void_p(ehs.data_ptr()), e.numpy().ctypes.data_as(C.POINTER(C.c_int32)), ehs.shape[0],
                                                   self.text_len, stream), "es_clip_text_pool")
            torch.cuda.synchronize(self.device)
        except Exception:
            self.lib.es_clip_bank_destroy(bank)
            raise
        finally:
            if enc is not None:
                enc.close()
        return bank

    # ---- the request side ----
    def score(self, images, bank, segments: Sequence[int], k: int):
        """(logits [n, W], probs [n, W], topk [n, nseg, k]) on the device for these images against `bank`"""
        out = self._pick(images, bank, segments, k)
        torch.cuda.synchronize(self.device)
        return out

    def _pick(self, images, bank, segments: Sequence[int], k: int):
        """score without the synchronisation: everything is queued on the current stream, and the tensors that go out of scope here
        return to torch's allocator, which hands them out again in that stream's order"""
        arrs = [image_bytes(im) for im in (images if isinstance(images, (list, tuple)) else [images])]
        n = len(arrs)
        if not 1 <= n <= self.max_images:
            raise EdgeStyleHipError(f"{n} images in one call; this picker was built for 1..{self.max_images} (max_images)")
        with torch.cuda.device(self.device):
            dev = [torch.from_numpy(a).to(self.device) for a in arrs]
            imgs = (L.ImageU8 * n)()
            for i, t in enumerate(dev):
                imgs[i].data, imgs[i].height, imgs[i].width, imgs[i].channels, imgs[i].row_stride = t.data_ptr(), t.shape[0], t.shape[1], t.shape[2], t.stride(0)
            need = self.lib.es_clip_pick_workspace_bytes(self._vision, imgs, n)
            if not need:
                L.check(-1, "es_clip_pick_workspace_bytes")
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            W = self.lib.es_clip_bank_rows(bank)
            seg = (C.c_int32 * len(segments))(*segments)
            logits = torch.empty((n, W), dtype=torch.float32, device=self.device)
            probs = torch.empty((n, W), dtype=torch.float32, device=self.device)
            topk = torch.empty((n, len(segments), k), dtype=torch.int32, device=self.device)
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            L.check(self.lib.es_clip_pick(self._vision, bank, imgs, n, self.logit_scale_exp, seg, len(segments), k, C.c_void_p(logits.data_ptr()),
                                          C.c_void_p(probs.data_ptr()), C.c_void_p(topk.data_ptr()), C.c_void_p(ws.data_ptr()), need, stream),
                    "es_clip_pick")
        return logits, probs, topk

    def prompt_table(self, suffix: str = ""):
        """the es_prompt_table of this picker's words for one suffix, built on first use (a device allocation and an upload) and kept"""
        if not isinstance(self.tokenizer, NativeCLIPTokenizer):
            raise EdgeStyleHipError("encode_prompts needs tokenizer=NativeCLIPTokenizer: the prompt is assembled from its token table")
        if suffix not in self._tables:
            self._tables[suffix] = self.tokenizer.prompt_table(self.colors + self.clothing_items, self._segments, prefix=self.prefix,
                                                               separator=",", suffix=suffix, device=self.device.index)
        return self._tables[suffix]

    def encode_prompts(self, images, text_encoder: NativeCLIPTextEncoder, suffix: str = "", out=None) -> torch.Tensor:
        """photos -> the text states of `picker(images)[i] + " " + suffix`, dtype [n, max_positions, hidden] on the device:
        es_clip_pick -> es_prompt_assemble -> es_text_encode_dev on the current stream, no synchronisation and no copy to the host."""
        table = self.prompt_table(suffix)
        with torch.cuda.device(self.device):
            _, _, topk = self._pick(images, self._bank, self._segments, 2)
            ids, _ = table.assemble(topk)
            return text_encoder.encode_ids_device(ids, out=out)

    def __call__(self, images) -> List[str]:
        """One prompt per image: "<prefix>, c1, c2, i1, i2" (MU:652-664) - both lists in ONE pass over the cached bank."""
        _, _, topk = self.score(images, self._bank, self._segments, 2)
        t = topk.cpu()
        return [self.prefix + ", " + ", ".join([self.colors[int(j)] for j in row[0]] + [self.clothing_items[int(j)] for j in row[1]]) for row in t]

    def find_best(self, items: Sequence[str], images, n: int = 2) -> List[List[str]]:
        """The n highest-probability entries of `items` for every image (MU:666-684).  One of the two built-in lists: the cached bank;
        any other list: a bank built for this call."""
        items = list(items)
        if not 1 <= n <= min(MAX_K, len(items)):
            raise EdgeStyleHipError(f"n = {n} is outside 1..{min(MAX_K, len(items))}")
        if items == self.colors or items == self.clothing_items:
            which = 0 if items == self.colors else 1
            if n > min(len(self.colors), len(self.clothing_items)):
                raise EdgeStyleHipError(f"n = {n} is above the shorter built-in list")
            _, _, topk = self.score(images, self._bank, self._segments, n)
            return [[items[int(j)] for j in row[which]] for row in topk.cpu()]
        with torch.cuda.device(self.device):
            bank = self._build_bank(items)
        try:
            _, _, topk = self.score(images, bank, [len(items)], n)
        finally:
            self.lib.es_clip_bank_destroy(bank)
        return [[items[int(j)] for j in row[0]] for row in topk.cpu()]

    def close(self):
        v, self._vision = getattr(self, "_vision", None), None
        b, self._bank = getattr(self, "_bank", None), None
        for t in getattr(self, "_tables", {}).values():
            t.close()
        self._tables = {}
        if b:
            self.lib.es_clip_bank_destroy(b)
        if v:
            self.lib.es_clip_vision_destroy(v)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

"""CLIP's byte-level BPE tokenizer in the library: a ctypes driver of es_tokenizer / es_prompt_table (include/edgestyle_hip.h,
csrc/bpe.h, csrc/prompt.hip).

`NativeCLIPTokenizer` is a drop-in for the `tokenizer=` of the pipeline and of `NativeBestEmbeddings`, for the one call both make:
`tokenizer(text, padding="max_length", max_length=L, truncation=True, return_tensors="pt").input_ids`.  Its ids are transformers'
CLIPTokenizer's on the accepted bytes (0x09-0x0D, 0x20-0x7E); any other text is refused, never approximated.  Needs no GPU."""
import ctypes as C
import os
from typing import List, Sequence, Union

import torch

from . import lib as L
from .lib import EdgeStyleHipError


class Encoding:
    """what the callers read of transformers' BatchEncoding"""

    def __init__(self, input_ids: torch.Tensor):
        self.input_ids = input_ids

    def __getitem__(self, key):
        if key != "input_ids":
            raise KeyError(key)
        return self.input_ids


def _bytes(text) -> bytes:
    if isinstance(text, bytes):
        return text
    if not isinstance(text, str):
        raise EdgeStyleHipError(f"a text must be str, got {type(text).__name__}")
    return text.encode("utf-8")          # a non-ASCII character becomes bytes >= 0x80, which the library refuses with their offset


class NativeCLIPTokenizer:
    def __init__(self, vocab_file: str, merges_file: str, model_max_length: int = 77):
        self.lib = L.load()
        self.vocab_file, self.merges_file = str(vocab_file), str(merges_file)
        h = C.c_void_p()
        L.check(self.lib.es_tokenizer_create(self.vocab_file.encode(), self.merges_file.encode(), int(model_max_length), C.byref(h)),
                "es_tokenizer_create")
        self._h = h
        self.model_max_length = int(model_max_length)
        self.vocab_size = self.lib.es_tokenizer_vocab_size(h)
        self.bos_token_id = self.lib.es_tokenizer_bos_id(h)
        self.eos_token_id = self.lib.es_tokenizer_eos_id(h)
        self.pad_token_id = self.lib.es_tokenizer_pad_id(h)

    @classmethod
    def from_pretrained(cls, directory: str, model_max_length: int = 77):
        """a tokenizer/ directory as transformers saves it: vocab.json and merges.txt"""
        return cls(os.path.join(directory, "vocab.json"), os.path.join(directory, "merges.txt"), model_max_length=model_max_length)

    def tokenize_ids(self, text) -> List[int]:
        """the ids of `text` without BOS / EOS, untruncated"""
        b = _bytes(text)
        n = self.lib.es_tokenize(self._h, b, len(b), None, 0)
        if n < 0:
            L.check(n, "es_tokenize")
        out = (C.c_int32 * max(n, 1))()
        L.check(min(self.lib.es_tokenize(self._h, b, len(b), out, n), 0), "es_tokenize")
        return list(out[:n])

    def padded(self, texts: Sequence, with_eos: bool = False):
        """int64 [n, model_max_length] rows (and, with_eos, the int32 [n] position of every row's first EOS)"""
        Lm = self.model_max_length
        rows = torch.empty((len(texts), Lm), dtype=torch.int32)
        eos = torch.empty((len(texts),), dtype=torch.int32)
        row_t, pos = C.POINTER(C.c_int32), C.c_int32()
        for i, t in enumerate(texts):
            b = _bytes(t)
            L.check(self.lib.es_tokenize_padded(self._h, b, len(b), C.cast(rows[i].data_ptr(), row_t), C.byref(pos)), "es_tokenize_padded")
            eos[i] = pos.value
        ids = rows.to(torch.int64)
        return (ids, eos) if with_eos else ids

    def __call__(self, text: Union[str, Sequence[str]], padding=None, max_length=None, truncation=None, return_tensors=None, **kw):
        if padding != "max_length" or truncation is not True or return_tensors != "pt" or any(v is not None for v in kw.values()):
            raise EdgeStyleHipError('NativeCLIPTokenizer implements the one call the pipeline makes: padding="max_length", truncation=True, '
                                    'return_tensors="pt" (and max_length = model_max_length)')
        if max_length is not None and int(max_length) != self.model_max_length:
            raise EdgeStyleHipError(f"max_length = {max_length}, but this tokenizer was built with model_max_length = {self.model_max_length}")
        texts = [text] if isinstance(text, (str, bytes)) else list(text)
        return Encoding(self.padded(texts))

    def prompt_table(self, words: Sequence[str], seg_ends: Sequence[int], prefix: str = "", separator: str = ",", suffix: str = "",
                     device: int = -1) -> "PromptTable":
        return PromptTable(self, words, seg_ends, prefix, separator, suffix, device)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self.lib.es_tokenizer_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PromptTable:
    """es_prompt_table: the words and the fixed pieces tokenised once; device -1 keeps it in host memory (assemble_host alone)"""

    def __init__(self, tokenizer: NativeCLIPTokenizer, words, seg_ends, prefix="", separator=",", suffix="", device: int = -1):
        self.lib, self.max_length, self.nseg, self.device = tokenizer.lib, tokenizer.model_max_length, len(seg_ends), int(device)
        enc = [_bytes(w) for w in words]
        if any(b"\0" in w for w in enc + [_bytes(prefix), _bytes(separator), _bytes(suffix)]):
            raise EdgeStyleHipError("a word or a fixed piece holds a NUL byte (they are passed NUL-terminated)")
        arr = (C.c_char_p * max(len(enc), 1))(*enc)
        seg = (C.c_int32 * max(len(seg_ends), 1))(*seg_ends)
        h = C.c_void_p()
        L.check(self.lib.es_prompt_table_create(tokenizer._h, arr, len(enc), seg, len(seg_ends), _bytes(prefix), _bytes(separator), _bytes(suffix),
                                                self.device, C.byref(h)), "es_prompt_table_create")
        self._h = h

    def assemble_host(self, topk: torch.Tensor):
        """topk: int [n, nseg, k] on the host -> (ids int32 [n, max_length], eos_pos int32 [n])"""
        t = topk.detach().to("cpu", torch.int32).contiguous()
        if t.dim() != 3 or t.shape[1] != self.nseg:
            raise EdgeStyleHipError(f"topk must be [n, {self.nseg}, k], got {tuple(t.shape)}")
        n, k = t.shape[0], t.shape[2]
        ids, eos = torch.empty((n, self.max_length), dtype=torch.int32), torch.empty((n,), dtype=torch.int32)
        p = C.POINTER(C.c_int32)
        L.check(self.lib.es_prompt_assemble_host(self._h, C.cast(t.data_ptr(), p), n, k, C.cast(ids.data_ptr(), p), C.cast(eos.data_ptr(), p)),
                "es_prompt_assemble_host")
        return ids, eos

    def assemble(self, topk: torch.Tensor, ids_out=None, eos_out=None):
        """topk: int32 [n, nseg, k] on the device -> (ids int32 [n, max_length], eos_pos int32 [n]) there, on the current stream"""
        if not topk.is_cuda or topk.dtype != torch.int32 or not topk.is_contiguous() or topk.dim() != 3 or topk.shape[1] != self.nseg:
            raise EdgeStyleHipError(f"topk must be a contiguous int32 [n, {self.nseg}, k] tensor on the device")
        n, k = topk.shape[0], topk.shape[2]
        with torch.cuda.device(topk.device):
            if ids_out is None:
                ids_out = torch.empty((n, self.max_length), dtype=torch.int32, device=topk.device)
            if eos_out is None:
                eos_out = torch.empty((n,), dtype=torch.int32, device=topk.device)
            stream = C.c_void_p(torch.cuda.current_stream(topk.device).cuda_stream)
            L.check(self.lib.es_prompt_assemble(self._h, C.c_void_p(topk.data_ptr()), n, k, C.c_void_p(ids_out.data_ptr()),
                                                C.c_void_p(eos_out.data_ptr()), stream), "es_prompt_assemble")
        return ids_out, eos_out

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self.lib.es_prompt_table_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

"""The CLIP text encoder on the HIP path: a ctypes driver of es_text_encoder (include/edgestyle_hip.h, csrc/text.hip).

`NativeCLIPTextEncoder` is a drop-in for the pipeline's `text_encoder=`: `encoder(input_ids)[0]` is CLIPTextModel's
last_hidden_state, computed by the library's kernels on the GPU instead of by transformers on the host's CPU threads.
The ids come from the caller's tokenizer - transformers' CLIPTokenizer, or the library's own (tokenizer.NativeCLIPTokenizer) - or,
already on the device, from es_prompt_assemble (`encode_ids_device`).  There is no fallback: a refused configuration raises."""
import ctypes as C

import torch

from . import lib as L
from .lib import EdgeStyleHipError

_DT = {torch.float16: L.ES_F16, torch.bfloat16: L.ES_BF16}
_TENSOR_DT = {torch.float32: L.ES_F32, torch.float16: L.ES_F16, torch.bfloat16: L.ES_BF16}
_ACTS = {"quick_gelu": 0}


def text_config(config) -> L.TextConfig:
    """CLIPTextConfig (or anything with its attribute names, or a dict of them) -> es_text_config"""
    get = (lambda k: config[k]) if isinstance(config, dict) else (lambda k: getattr(config, k))
    act = get("hidden_act")
    if act not in _ACTS:
        raise EdgeStyleHipError(f"NativeCLIPTextEncoder implements hidden_act 'quick_gelu' (SD1.5's CLIP ViT-L/14), not {act!r}")
    return L.TextConfig(vocab_size=get("vocab_size"), hidden=get("hidden_size"), heads=get("num_attention_heads"),
                        layers=get("num_hidden_layers"), intermediate=get("intermediate_size"),
                        max_positions=get("max_position_embeddings"), ln_eps=float(get("layer_norm_eps")), act=_ACTS[act])


def state_dict_descriptors(sd):
    """{key: tensor} -> (es_state_dict, keep-alive list).  Entries that are not fp32 / fp16 / bf16 tensors (the int64
    `position_ids` buffer of older checkpoints) are dropped: the builder ignores keys it does not know anyway."""
    items = [(k, v) for k, v in sd.items() if torch.is_tensor(v) and v.dtype in _TENSOR_DT and 1 <= v.dim() <= 4]
    arr = (L.Tensor * max(len(items), 1))()
    keep = [arr]
    for i, (k, v) in enumerate(items):
        v = v.detach().contiguous()
        kb = k.encode()
        keep += [v, kb]
        arr[i].key, arr[i].data, arr[i].ndim, arr[i].dtype = kb, v.data_ptr(), v.dim(), _TENSOR_DT[v.dtype]
        for j, s in enumerate(v.shape):
            arr[i].shape[j] = s
    return L.StateDict(arr, len(items)), keep


class NativeCLIPTextEncoder:
    """sd: CLIPTextModel's state dict (keys bare or with the `text_model.` prefix); config: its CLIPTextConfig.
    max_n: the most prompts one call encodes (the activations are allocated for it).  device: a CUDA device, or None / "dry"
    for a dry build without a GPU (arena_bytes is then all it can tell)."""

    def __init__(self, sd, config, dtype=torch.float16, device="cuda", max_n: int = 2):
        if dtype not in _DT:
            raise EdgeStyleHipError(f"NativeCLIPTextEncoder computes in fp16 or bf16, not {dtype}")
        self.lib = L.load()
        self.dtype, self.max_n = dtype, int(max_n)
        self.cfg = text_config(config)
        dry = device is None or device == "dry"
        self.device = None if dry else torch.device(device)
        if not dry and self.device.type != "cuda":
            raise EdgeStyleHipError(f"NativeCLIPTextEncoder runs on a GPU, not on {self.device} (there is no CPU fallback)")
        index = -1 if dry else (self.device.index if self.device.index is not None else torch.cuda.current_device())
        if not dry:
            self.device = torch.device("cuda", index)
        desc, keep = state_dict_descriptors(sd)
        handle = C.c_void_p()
        L.check(self.lib.es_text_encoder_create(C.byref(desc), C.byref(self.cfg), _DT[dtype], self.max_n, index, C.byref(handle)),
                "es_text_encoder_create")
        del keep
        self._h = handle

    @classmethod
    def from_module(cls, module, dtype=torch.float16, device="cuda", max_n: int = 2):
        """module: a transformers CLIPTextModel"""
        return cls(module.state_dict(), module.config, dtype=dtype, device=device, max_n=max_n)

    @classmethod
    def from_state_dict(cls, sd, config, dtype=torch.float16, device="cuda", max_n: int = 2):
        return cls(sd, config, dtype=dtype, device=device, max_n=max_n)

    @property
    def arena_bytes(self) -> int:
        return self.lib.es_text_encoder_arena_bytes(self._h)

    def to(self, *args, **kwargs):
        """No-op: the encoder stays on the device it was built on (pipeline.to() sends text encoders to "cpu")."""
        return self

    def encode_ids(self, ids_host: torch.Tensor, out=None) -> torch.Tensor:
        """ids_host: int [n, max_positions] on the host -> dtype [n, max_positions, hidden] on the device"""
        ids = ids_host.detach().to("cpu", torch.int32).contiguous()
        if ids.dim() != 2 or ids.shape[1] != self.cfg.max_positions:
            raise EdgeStyleHipError(f"input_ids must be [n, {self.cfg.max_positions}] (pad to max_length), got {tuple(ids.shape)}")
        n = ids.shape[0]
        if self.device is None:        # a dry build: the library says so (the output pointer is never touched)
            L.check(self.lib.es_text_encode(self._h, C.c_void_p(ids.data_ptr()), n, C.c_void_p(8), None), "es_text_encode")
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty((n, self.cfg.max_positions, self.cfg.hidden), dtype=self.dtype, device=self.device)
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            L.check(self.lib.es_text_encode(self._h, C.c_void_p(ids.data_ptr()), n, C.c_void_p(out.data_ptr()), stream), "es_text_encode")
        return out

    def encode_ids_device(self, ids_dev: torch.Tensor, out=None) -> torch.Tensor:
        """ids_dev: int32 [n, max_positions] on the device (es_prompt_assemble's rows) -> dtype [n, max_positions, hidden] there, on the
        current stream: no host copy, no synchronisation, capturable.  Bit-equal to encode_ids of the same ids."""
        if self.device is None:
            raise EdgeStyleHipError("this encoder is a dry build: it holds no device memory and cannot run")
        if not ids_dev.is_cuda or ids_dev.device != self.device or ids_dev.dtype != torch.int32 or not ids_dev.is_contiguous() \
                or ids_dev.dim() != 2 or ids_dev.shape[1] != self.cfg.max_positions:
            raise EdgeStyleHipError(f"ids_dev must be a contiguous int32 [n, {self.cfg.max_positions}] tensor on {self.device}")
        n = ids_dev.shape[0]
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty((n, self.cfg.max_positions, self.cfg.hidden), dtype=self.dtype, device=self.device)
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            L.check(self.lib.es_text_encode_dev(self._h, C.c_void_p(ids_dev.data_ptr()), n, C.c_void_p(out.data_ptr()), stream), "es_text_encode_dev")
        return out

    def __call__(self, input_ids, *args, **kwargs):
        if args or any(v is not None for v in kwargs.values()):
            raise EdgeStyleHipError("NativeCLIPTextEncoder takes input_ids alone (no attention mask, no clip_skip: the reference passes none)")
        return (self.encode_ids(input_ids),)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self.lib.es_text_encoder_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

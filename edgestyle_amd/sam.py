"""The EfficientViT-SAM image encoder on the HIP path: a ctypes driver of es_sam_encoder (include/edgestyle_hip.h, csrc/sam.hip).

`NativeSamImageEncoder` is callable like the module it replaces - `enc(x [B, 3, S, S] fp32) -> [B, out_dim, 64, 64] fp32` - so

    sam.image_encoder = NativeSamImageEncoder.from_module(sam.image_encoder)

makes the reference's EfficientViTSamPredictor.set_image (efficientvit/models/efficientvit/sam.py:274-293) run on it unchanged.

The reference builds FIVE predictors per photo (extract_dataset.py:371-425) whose fine-tuned models differ in the mask decoder only: the
training scripts freeze image_encoder and prompt_encoder.  All five therefore share this encoder: one `encode_u8(photo)` per photo feeds
every decoder -

    feats, hw = enc.encode_u8([photo])                      # photo bytes in: SamResize, ToTensor, Normalize, SamPad on the device
    for p in predictors:
        p.reset_image(); p.features = feats; p.original_size = photo.shape[:2]; p.input_size = tuple(hw[0]); p.is_image_set = True

- one pass of the network instead of five (fifteen per request of three photos).  The mask decoder and the prompt encoder stay with
the caller.  There is no fallback: a refused configuration raises."""
import ctypes as C
from typing import Sequence

import torch

from . import lib as L
from .clip import image_bytes
from .lib import EdgeStyleHipError
from .text import state_dict_descriptors

_DT = {torch.float16: L.ES_F16, torch.bfloat16: L.ES_BF16}
_MODELS = {"l0": ((1, 1, 1, 4, 4), 4), "l1": ((1, 1, 1, 6, 6), 8), "l2": ((1, 2, 2, 8, 8), 12)}      # depth_list, head_depth (sam.py:544-595)
PIXEL_MEAN = (123.675 / 255, 116.28 / 255, 103.53 / 255)      # EfficientViTSam.transform's Normalize (sam.py:215-218)
PIXEL_STD = (58.395 / 255, 57.12 / 255, 57.375 / 255)
NECK_SIZE = 64


def sam_config(name: str = "l2", image_size: int = 512, **over) -> L.SamConfig:
    """es_sam_config of efficientvit_sam_l0 | l1 | l2 (create_sam_model sets every norm's eps to 1e-6); `over` replaces single fields
    (widths, depths, head_width, head_depth, out_dim, bn_eps, ln_eps)"""
    if name not in _MODELS:
        raise EdgeStyleHipError(f"sam_config knows the models {sorted(_MODELS)}, not {name!r}")
    depths, head_depth = _MODELS[name]
    widths = tuple(over.pop("widths", (32, 64, 128, 256, 512)))
    depths = tuple(over.pop("depths", depths))
    cfg = L.SamConfig(image_size=int(image_size), qkv_dim=32, head_width=over.pop("head_width", 256), head_depth=over.pop("head_depth", head_depth),
                      out_dim=over.pop("out_dim", 256), bn_eps=over.pop("bn_eps", 1e-6), ln_eps=over.pop("ln_eps", 1e-6))
    if over:
        raise EdgeStyleHipError(f"sam_config: unknown fields {sorted(over)}")
    if len(widths) != 5 or len(depths) != 5:
        raise EdgeStyleHipError("sam_config: widths and depths have five entries each")
    for i in range(5):
        cfg.width[i], cfg.depth[i] = widths[i], depths[i]
    for i in range(3):
        cfg.pixel_mean[i], cfg.pixel_std[i] = PIXEL_MEAN[i], PIXEL_STD[i]
    return cfg


def config_of_state_dict(sd, image_size: int = 512) -> L.SamConfig:
    """the es_sam_config a state dict of the reference's encoder implies: widths and out_dim from the shapes, depths from the keys"""
    pre = "image_encoder." if any(k.startswith("image_encoder.") for k in sd) else ""

    def count(fmt, start):
        i = start
        while any(k.startswith(pre + fmt.format(i) + ".") for k in sd):
            i += 1
        return i - start
    widths = [sd[pre + "backbone.stages.0.op_list.0.conv.weight"].shape[0]]
    for s in (1, 2, 3, 4):
        widths.append(sd[pre + f"backbone.stages.{s}.op_list.0.main.point_conv.conv.weight"].shape[0])
    depths = [count("backbone.stages.0.op_list.{}", 1)] + [count(f"backbone.stages.{s}.op_list.{{}}", 1) for s in (1, 2, 3, 4)]
    out = sd[pre + "neck.output_ops.0.op_list.0.conv.weight"]
    return sam_config("l2", image_size, widths=widths, depths=depths, head_width=out.shape[1], head_depth=count("neck.middle.op_list.{}", 0),
                      out_dim=out.shape[0])


class NativeSamImageEncoder(torch.nn.Module):
    """An nn.Module without parameters, so that it can take the place of the `image_encoder` child of an EfficientViTSam.
    sd: the state dict of an EfficientViTSamImageEncoder (keys bare, or with the `image_encoder.` prefix of an EfficientViTSam
    checkpoint); config: an es_sam_config (sam_config / config_of_state_dict).  max_n: the most images one call encodes (the activations
    are allocated for it).  device: a CUDA device, or None / "dry" for a dry build without a GPU (arena_bytes is then all it can tell)."""

    def __init__(self, sd, config: L.SamConfig, dtype=torch.float16, device="cuda", max_n: int = 1):
        if dtype not in _DT:
            raise EdgeStyleHipError(f"NativeSamImageEncoder computes in fp16 or bf16, not {dtype}")
        super().__init__()
        self.lib = L.load()
        self.dtype, self.max_n, self.cfg = dtype, int(max_n), config
        dry = device is None or device == "dry"
        self.device = None if dry else torch.device(device)
        if not dry and self.device.type != "cuda":
            raise EdgeStyleHipError(f"NativeSamImageEncoder runs on a GPU, not on {self.device} (there is no CPU fallback)")
        index = -1 if dry else (self.device.index if self.device.index is not None else torch.cuda.current_device())
        if not dry:
            self.device = torch.device("cuda", index)
        desc, keep = state_dict_descriptors(sd)
        handle = C.c_void_p()
        L.check(self.lib.es_sam_encoder_create(C.byref(desc), C.byref(self.cfg), _DT[dtype], self.max_n, index, C.byref(handle)), "es_sam_encoder_create")
        del keep
        self._h = handle

    @classmethod
    def from_module(cls, image_encoder, dtype=torch.float16, device="cuda", max_n: int = 1, image_size: int = 512):
        """image_encoder: the reference's EfficientViTSamImageEncoder (or any module with its state_dict() names)"""
        sd = image_encoder.state_dict()
        return cls(sd, config_of_state_dict(sd, image_size), dtype=dtype, device=device, max_n=max_n)

    @classmethod
    def from_state_dict(cls, sd, config: L.SamConfig, dtype=torch.float16, device="cuda", max_n: int = 1):
        return cls(sd, config, dtype=dtype, device=device, max_n=max_n)

    @property
    def arena_bytes(self) -> int:
        return self.lib.es_sam_encoder_arena_bytes(self._h)

    @property
    def out_shape(self):
        return (self.cfg.out_dim, NECK_SIZE, NECK_SIZE)

    def to(self, *args, **kwargs):
        """No-op: the encoder stays on the device and in the dtype it was built with."""
        return self

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _need_device(self):
        if self.device is None:
            raise EdgeStyleHipError("this encoder is a dry build: it holds no device memory and cannot run")

    def forward(self, x: torch.Tensor, out=None) -> torch.Tensor:
        """x: fp32 [B, 3, S, S], normalised and padded (EfficientViTSam.transform's tensor), on any device -> fp32 [B, out_dim, 64, 64] on
        the encoder's device, on the current stream (capturable when x already is a contiguous fp32 tensor there)"""
        self._need_device()
        S = self.cfg.image_size
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, S, S):
            raise EdgeStyleHipError(f"the input must be [B, 3, {S}, {S}], got {tuple(x.shape)}")
        with torch.cuda.device(self.device):
            x = x.detach().to(self.device, torch.float32).contiguous()
            n = x.shape[0]
            if out is None:
                out = torch.empty((n,) + self.out_shape, dtype=torch.float32, device=self.device)
            L.check(self.lib.es_sam_encode(self._h, C.c_void_p(x.data_ptr()), n, C.c_void_p(out.data_ptr()), self._stream()), "es_sam_encode")
        return out

    def stage(self, stage: int, n: int) -> torch.Tensor:
        """the backbone's stage2 | stage3 | stage4 map of the last call, fp32 NCHW"""
        self._need_device()
        side = self.cfg.image_size >> (stage + 1)
        with torch.cuda.device(self.device):
            out = torch.empty((n, self.cfg.width[stage], side, side), dtype=torch.float32, device=self.device)
            L.check(self.lib.es_sam_encoder_stage(self._h, stage, n, C.c_void_p(out.data_ptr()), self._stream()), "es_sam_encoder_stage")
        return out

    def encode_u8(self, photos: Sequence, out=None):
        """photos: PIL images, or uint8 HWC arrays / tensors (3 or 4 channels) of any size -> (fp32 [n, out_dim, 64, 64] on the device, the
        resized (h, w) of each photo as a list of tuples: the `input_size` postprocess_masks needs)"""
        self._need_device()
        photos = photos if isinstance(photos, (list, tuple)) else [photos]
        n = len(photos)
        if not 1 <= n <= self.max_n:
            raise EdgeStyleHipError(f"{n} photos in one call; this encoder was built for 1..{self.max_n} (max_n)")
        with torch.cuda.device(self.device):
            dev = [p if (torch.is_tensor(p) and p.is_cuda) else torch.from_numpy(image_bytes(p)).to(self.device) for p in photos]
            imgs = (L.ImageU8 * n)()
            for i, t in enumerate(dev):
                if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] not in (3, 4) or t.stride(2) != 1 or t.stride(1) != t.shape[2]:
                    raise EdgeStyleHipError(f"photo {i} must be a uint8 [H, W, 3 | 4] tensor with dense pixels")
                imgs[i].data, imgs[i].height, imgs[i].width, imgs[i].channels = t.data_ptr(), t.shape[0], t.shape[1], t.shape[2]
                imgs[i].row_stride = t.stride(0) if t.shape[0] > 1 else t.shape[1] * t.shape[2]
            need = self.lib.es_sam_encode_u8_workspace_bytes(self._h, imgs, n)
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
            hw = (C.c_int32 * (2 * n))()
            if out is None:
                out = torch.empty((n,) + self.out_shape, dtype=torch.float32, device=self.device)
            L.check(self.lib.es_sam_encode_u8(self._h, imgs, n, C.c_void_p(out.data_ptr()), hw, C.c_void_p(ws.data_ptr()), need, self._stream()),
                    "es_sam_encode_u8")
        return out, [(hw[2 * i], hw[2 * i + 1]) for i in range(n)]

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self.lib.es_sam_encoder_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

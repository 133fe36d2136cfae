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

- one pass of the network instead of five (fifteen per request of three photos).  The prompt encoder and the mask decoder are
here too (csrc/sam_decoder.hip): `NativeSamMaskDecoder` drives es_sam_decoder, `NativeSamPredictor` has the reference predictor's surface,
and the kernels are callable one by one: `SamPromptWeights` + `prompt_tokens` (the
token matrix of a point / box prompt), `linear_tokens` (the token-side linear layers), `upscale_masks` (the fused upscaling tail), `postprocess_masks` (low-res logits to masks at the
photo's size) and masks.get_box (a mask's box, on the device, as the next decode's prompt).  There is no fallback: a refused
configuration raises."""
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


# ---- prompt encoder and mask decoder pieces (csrc/sam_decoder.hip) -------------------------------------------------------------------
_PROMPT_KEYS = ("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", "prompt_encoder.not_a_point_embed.weight",
                "mask_decoder.iou_token.weight", "mask_decoder.mask_tokens.weight")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream_of(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class SamPromptWeights:
    """The fp32 tensors es_sam_prompt_tokens reads, from a state dict with segment_anything's names (`prompt_encoder.*`, `mask_decoder.*`),
    bare or under a caller's prefix.  A missing key or a wrong shape raises with the key's name."""

    def __init__(self, sd, device="cuda", frame: int = 1024):
        first = _PROMPT_KEYS[0]
        hit = [k for k in sd if k.endswith(first)]
        if not hit:
            raise EdgeStyleHipError(f"SamPromptWeights: missing key {first}")
        pre = hit[0][:-len(first)]

        def get(key, shape):
            if pre + key not in sd:
                raise EdgeStyleHipError(f"SamPromptWeights: missing key {pre + key}")
            t = sd[pre + key]
            if tuple(t.shape) != tuple(shape):
                raise EdgeStyleHipError(f"SamPromptWeights: {pre + key} has shape {tuple(t.shape)}, expected {tuple(shape)}")
            return t.detach().to(device, torch.float32).contiguous()
        half = sd[hit[0]].shape[-1]
        E = self.embed_dim = 2 * half
        self.frame = int(frame)
        self.gauss = get(first, (2, half))
        self.point_embeddings = torch.cat([get(f"prompt_encoder.point_embeddings.{i}.weight", (1, E)) for i in range(4)], 0).contiguous()
        self.not_a_point = get(_PROMPT_KEYS[1], (1, E))
        self.iou_token = get(_PROMPT_KEYS[2], (1, E))
        mt = sd.get(pre + _PROMPT_KEYS[3])
        self.mask_tokens = get(_PROMPT_KEYS[3], (mt.shape[0] if mt is not None else 4, E))
        self.n_mask_tokens = self.mask_tokens.shape[0]
        self.device = self.gauss.device

    def desc(self, n, P, original_size, points=None, labels=None, boxes=None, tokens=None, query_pe=None, dtype=torch.float16) -> L.SamPromptDesc:
        d = L.SamPromptDesc()
        d.gauss, d.point_embeddings, d.not_a_point = self.gauss.data_ptr(), self.point_embeddings.data_ptr(), self.not_a_point.data_ptr()
        d.iou_token, d.mask_tokens = self.iou_token.data_ptr(), self.mask_tokens.data_ptr()
        for name, t in (("points", points), ("labels", labels), ("boxes", boxes), ("tokens", tokens), ("query_pe", query_pe)):
            setattr(d, name, t.data_ptr() if t is not None else None)
        d.n, d.P, d.embed_dim, d.n_mask_tokens, d.frame = n, P, self.embed_dim, self.n_mask_tokens, self.frame
        d.orig_h, d.orig_w, d.dtype = int(original_size[0]), int(original_size[1]), _DT.get(dtype, L.ES_F32)
        return d


def prompt_token_count(P: int, has_box: bool) -> int:
    return L.load().es_sam_prompt_token_count(int(P), 1 if has_box else 0)


def prompt_tokens(w: SamPromptWeights, original_size, points=None, labels=None, boxes=None, dtype=torch.float16, want_query_pe: bool = True):
    """points [n, P, 2] (x, y) and boxes [n, 4] in ORIGINAL-image pixels, labels [n, P] (1 | 0 | -1); boxes may be what masks.get_box left on
    the device.  -> (tokens, query_pe), each `dtype` [n, 1 + n_mask_tokens + T, embed_dim] on the device (query_pe None if not wanted)."""
    if dtype not in _DT:
        raise EdgeStyleHipError(f"prompt_tokens writes fp16 or bf16, not {dtype}")
    dev = w.device
    with torch.cuda.device(dev):
        pts = None if points is None else torch.as_tensor(points).to(dev, torch.float32).contiguous()
        lab = None if labels is None else torch.as_tensor(labels).to(dev, torch.int32).contiguous()
        box = None if boxes is None else torch.as_tensor(boxes).to(dev, torch.float32).contiguous()
        if pts is not None and (pts.dim() != 3 or pts.shape[2] != 2 or lab is None or tuple(lab.shape) != tuple(pts.shape[:2])):
            raise EdgeStyleHipError("prompt_tokens: points are [n, P, 2] with labels [n, P]")
        if box is not None and (box.dim() != 2 or box.shape[1] != 4 or (pts is not None and box.shape[0] != pts.shape[0])):
            raise EdgeStyleHipError("prompt_tokens: boxes are [n, 4], one per image")
        if pts is None and box is None:
            raise EdgeStyleHipError("prompt_tokens: no prompt: neither points nor a box")
        n = pts.shape[0] if pts is not None else box.shape[0]
        P = pts.shape[1] if pts is not None else 0
        rows = 1 + w.n_mask_tokens + prompt_token_count(P, box is not None)
        tokens = torch.empty((n, rows, w.embed_dim), dtype=dtype, device=dev)
        qpe = torch.empty_like(tokens) if want_query_pe else None
        d = w.desc(n, P, original_size, pts if P else None, lab if P else None, box, tokens, qpe, dtype)
        L.check(L.load().es_sam_prompt_tokens(C.byref(d), _stream_of(dev)), "es_sam_prompt_tokens")
    return tokens, qpe


def linear_tokens(x: torch.Tensor, w: torch.Tensor, bias=None, relu: bool = False, residual=None, out=None) -> torch.Tensor:
    """x [n, rows, K] (rows <= 32; the last dimension dense), w [N, K] or, one set per row, [rows, N, K], bias fp32 [N] | [rows, N] ->
    act(x w^T + bias) (+ residual) [n, rows, N], fp32 accumulation and one rounding (es_linear_tokens)."""
    if x.dim() != 3 or x.dtype not in _DT or w.dtype != x.dtype or not x.is_cuda or x.stride(2) != 1 or not w.is_contiguous():
        raise EdgeStyleHipError("linear_tokens: x is a CUDA fp16 | bf16 [n, rows, K] tensor with dense rows, w contiguous and of its dtype")
    n, rows, K = x.shape
    per_row = w.dim() == 3
    N = w.shape[-2]
    if w.shape[-1] != K or (per_row and w.shape[0] != rows):
        raise EdgeStyleHipError(f"linear_tokens: w {tuple(w.shape)} does not fit x {tuple(x.shape)}")
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or tuple(bias.shape) != ((rows, N) if per_row else (N,))):
        raise EdgeStyleHipError("linear_tokens: bias is a contiguous fp32 [N] tensor ([rows, N] with a weight set per row)")
    if out is None:
        out = torch.empty((n, rows, N), dtype=x.dtype, device=x.device)
    for name, t in (("residual", residual), ("out", out)):
        if t is not None and (t.dtype != x.dtype or tuple(t.shape) != (n, rows, N) or t.stride(2) != 1):
            raise EdgeStyleHipError(f"linear_tokens: {name} is [n, rows, N] in x's dtype with dense rows")
    d = L.LinearTokensDesc()
    d.x, d.w, d.bias, d.residual, d.out = x.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None, \
        residual.data_ptr() if residual is not None else None, out.data_ptr()
    d.n, d.rows, d.K, d.N = n, rows, K, N
    d.ldx, d.bsx = x.stride(1), x.stride(0)
    d.ldo, d.bso = out.stride(1), out.stride(0)
    if residual is not None:
        d.ldr, d.bsr = residual.stride(1), residual.stride(0)
    d.per_row_weights, d.relu, d.dtype = int(per_row), int(bool(relu)), _DT[x.dtype]
    with torch.cuda.device(x.device):
        L.check(L.load().es_linear_tokens(C.byref(d), _stream_of(x.device)), "es_linear_tokens")
    return out


def postprocess_masks(logits: torch.Tensor, input_size, original_size, frame: int = 1024, want_logits: bool = False, want_masks: bool = True):
    """EfficientViTSam.postprocess_masks and `> 0` as one launch: logits fp32 [n, M, L, L] on the device -> (fp32 [n, M, H, W] | None,
    uint8 [n, M, H, W] | None)"""
    if logits.dim() != 4 or logits.dtype != torch.float32 or not logits.is_cuda or logits.shape[2] != logits.shape[3]:
        raise EdgeStyleHipError("postprocess_masks: logits are a CUDA fp32 [n, M, L, L] tensor")
    logits = logits.contiguous()
    n, M, Lr, _ = logits.shape
    H, W = int(original_size[0]), int(original_size[1])
    with torch.cuda.device(logits.device):
        f = torch.empty((n, M, H, W), dtype=torch.float32, device=logits.device) if want_logits else None
        m = torch.empty((n, M, H, W), dtype=torch.uint8, device=logits.device) if want_masks else None
        L.check(L.load().es_sam_postprocess_masks(_ptr(logits), n * M, Lr, int(frame), int(input_size[0]), int(input_size[1]), H, W, _ptr(f), _ptr(m),
                                                  _stream_of(logits.device)), "es_sam_postprocess_masks")
    return f, m


def upscale_pack(w: torch.Tensor, dtype=torch.float16, device="cuda") -> torch.Tensor:
    """MaskDecoder.output_upscaling.3.weight [C1, C1 / 2, 2, 2] -> the operand es_sam_upscale_masks loads (es_sam_upscale_pack), on `device`"""
    if dtype not in _DT or w.dim() != 4 or tuple(w.shape[1:]) != (w.shape[0] // 2, 2, 2):
        raise EdgeStyleHipError(f"upscale_pack takes a [C1, C1 / 2, 2, 2] weight and fp16 or bf16, got {tuple(w.shape)}, {dtype}")
    src = w.detach().to("cpu", torch.float32).contiguous()
    out = torch.empty(2 * w.shape[0] * w.shape[0], dtype=dtype)
    L.check(L.load().es_sam_upscale_pack(_ptr(src), w.shape[0], _DT[dtype], _ptr(out)), "es_sam_upscale_pack")
    return out.to(device)


def upscale_masks(g: torch.Tensor, w_packed: torch.Tensor, ln_gamma, ln_beta, bias2, hyper: torch.Tensor, grid, eps: float = 1e-6, out=None):
    """g [n, Gh * Gw, 4 * C1] (ConvT1 as a 1x1 GEMM, column (2 dy + dx) * C1 + c), hyper [n, M, C1 / 2] (rows may be a slice of a wider token
    matrix) -> fp32 logits [n, M, 4 Gh, 4 Gw] (es_sam_upscale_masks); ln_gamma, ln_beta [C1] and bias2 [C1 / 2] fp32"""
    Gh, Gw = int(grid[0]), int(grid[1])
    if g.dim() != 3 or g.dtype not in _DT or not g.is_cuda or not g.is_contiguous() or g.shape[1] != Gh * Gw or g.shape[2] % 4:
        raise EdgeStyleHipError("upscale_masks: g is a contiguous CUDA fp16 | bf16 [n, Gh * Gw, 4 * C1] tensor")
    n, C1 = g.shape[0], g.shape[2] // 4
    if hyper.dim() != 3 or hyper.dtype != g.dtype or hyper.shape[0] != n or hyper.shape[2] != C1 // 2 or hyper.stride(2) != 1:
        raise EdgeStyleHipError("upscale_masks: hyper is [n, M, C1 / 2] in g's dtype with dense rows")
    if w_packed.dtype != g.dtype or w_packed.numel() != 2 * C1 * C1 or not w_packed.is_contiguous():
        raise EdgeStyleHipError("upscale_masks: w_packed is upscale_pack's tensor in g's dtype")
    for name, t, c in (("ln_gamma", ln_gamma, C1), ("ln_beta", ln_beta, C1), ("bias2", bias2, C1 // 2)):
        if t.dtype != torch.float32 or tuple(t.shape) != (c,) or not t.is_contiguous() or not t.is_cuda:
            raise EdgeStyleHipError(f"upscale_masks: {name} is a contiguous CUDA fp32 [{c}] tensor")
    M = hyper.shape[1]
    if out is None:
        out = torch.empty((n, M, 4 * Gh, 4 * Gw), dtype=torch.float32, device=g.device)
    d = L.SamUpscaleDesc()
    d.g, d.w_packed, d.ln_gamma, d.ln_beta, d.bias2, d.hyper, d.out = (t.data_ptr() for t in (g, w_packed, ln_gamma, ln_beta, bias2, hyper, out))
    d.n, d.grid_h, d.grid_w, d.C1, d.M, d.ldh, d.bsh, d.ln_eps, d.dtype = n, Gh, Gw, C1, M, hyper.stride(1), hyper.stride(0), eps, _DT[g.dtype]
    with torch.cuda.device(g.device):
        L.check(L.load().es_sam_upscale_masks(C.byref(d), _stream_of(g.device)), "es_sam_upscale_masks")
    return out


# ---- the mask decoder object ----------------------------------------------------------------------------------------------------------
def decoder_config_of_state_dict(sd, heads: int = 8, grid: int = 64, frame: int = 1024, ln_eps: float = 1e-5, ln2d_eps: float = 1e-6) -> L.SamDecoderConfig:
    """the es_sam_decoder_config a state dict with segment_anything's names implies: widths and depths from the shapes and the keys that
    exist (heads, the grid and the prompt frame are not in a state dict).  Keys that are missing leave their field 0: es_sam_decoder_create
    then names what it cannot build."""
    first = _PROMPT_KEYS[0]
    hit = [k for k in sd if k.endswith(first)]
    if not hit:
        raise EdgeStyleHipError(f"NativeSamMaskDecoder: missing key {first}")
    pre = hit[0][:-len(first)]

    def shape(key, i):
        t = sd.get(pre + key)
        return int(t.shape[i]) if t is not None and t.dim() > i else 0

    def count(fmt):
        i = 0
        while pre + fmt.format(i) in sd:
            i += 1
        return i
    E = 2 * int(sd[hit[0]].shape[-1])
    internal = shape("mask_decoder.transformer.final_attn_token_to_image.q_proj.weight", 0)
    return L.SamDecoderConfig(embed_dim=E, heads=int(heads), mlp_dim=shape("mask_decoder.transformer.layers.0.mlp.lin1.weight", 0),
                              depth=count("mask_decoder.transformer.layers.{}.norm1.weight"), grid=int(grid), frame=int(frame),
                              n_mask_tokens=shape("mask_decoder.mask_tokens.weight", 0),
                              iou_hidden=shape("mask_decoder.iou_prediction_head.layers.0.weight", 0),
                              iou_depth=count("mask_decoder.iou_prediction_head.layers.{}.weight"),
                              attn_downsample=E // internal if internal and E % internal == 0 else 0, ln_eps=ln_eps, ln2d_eps=ln2d_eps)


class NativeSamMaskDecoder:
    """segment_anything's PromptEncoder + MaskDecoder (as EfficientViT-SAM builds them, sam.py:522-540) on the HIP path: a ctypes driver of
    es_sam_decoder (include/edgestyle_hip.h, csrc/sam_decoder.hip).  One arena holds the packed weights, the per-decoder constants and the
    activations of max_n images; a decode allocates nothing inside the library and reads nothing back, so a decode's mask can prompt the next
    one (masks.get_box) without a host visit, and image i of a batch equals the image alone bit for bit.  sd: a state dict with
    segment_anything's names (`prompt_encoder.*`, `mask_decoder.*`), bare or under a prefix; mask_input is not supported (the reference never
    passes one).  device None / "dry": a dry build without a GPU (arena_bytes is then all it can tell)."""

    def __init__(self, sd, dtype=torch.float16, device="cuda", heads: int = 8, grid: int = 64, frame: int = 1024, ln_eps: float = 1e-5,
                 ln2d_eps: float = 1e-6, max_n: int = 3, max_points: int = 8, config: "L.SamDecoderConfig | None" = None):
        if dtype not in _DT:
            raise EdgeStyleHipError(f"NativeSamMaskDecoder computes in fp16 or bf16, not {dtype}")
        self.lib = L.load()
        self.dtype, self.max_n, self.max_points = dtype, int(max_n), int(max_points)
        dry = device is None or device == "dry"
        self.device = None if dry else torch.device(device)
        if not dry and self.device.type != "cuda":
            raise EdgeStyleHipError(f"NativeSamMaskDecoder runs on a GPU, not on {self.device} (there is no CPU fallback)")
        index = -1 if dry else (self.device.index if self.device.index is not None else torch.cuda.current_device())
        if not dry:
            self.device = torch.device("cuda", index)
        self.cfg = config if config is not None else decoder_config_of_state_dict(sd, heads, grid, frame, ln_eps, ln2d_eps)
        self.E, self.grid, self.frame, self.n_mask_tokens = self.cfg.embed_dim, self.cfg.grid, self.cfg.frame, self.cfg.n_mask_tokens
        desc, keep = state_dict_descriptors(sd)
        handle = C.c_void_p()
        L.check(self.lib.es_sam_decoder_create(C.byref(desc), C.byref(self.cfg), _DT[dtype], self.max_n, self.max_points, index, C.byref(handle)),
                "es_sam_decoder_create")
        del keep
        self._h = handle

    @classmethod
    def from_state_dict(cls, sd, dtype=torch.float16, device="cuda", **kw):
        return cls(sd, dtype=dtype, device=device, **kw)

    @classmethod
    def from_modules(cls, prompt_encoder, mask_decoder, dtype=torch.float16, device="cuda", **kw):
        """prompt_encoder, mask_decoder: segment_anything's modules (an EfficientViTSam's children), or any with their state_dict() names"""
        sd = {"prompt_encoder." + k: v for k, v in prompt_encoder.state_dict().items()}
        sd.update({"mask_decoder." + k: v for k, v in mask_decoder.state_dict().items()})
        return cls(sd, dtype=dtype, device=device, **kw)

    @property
    def arena_bytes(self) -> int:
        return self.lib.es_sam_decoder_arena_bytes(self._h)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self.lib.es_sam_decoder_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _prompts(self, emb, original_size, points, labels, boxes):
        g, E = self.grid, self.E
        if self.device is None:
            raise EdgeStyleHipError("this decoder is a dry build: it holds no device memory and cannot run")
        if emb.dim() != 4 or tuple(emb.shape[1:]) != (E, g, g) or not emb.is_cuda:
            raise EdgeStyleHipError(f"decode: the embedding must be a CUDA [n, {E}, {g}, {g}] tensor, got {tuple(emb.shape)}")
        dev = self.device
        emb = emb.to(dev, torch.float32).contiguous()
        pts = None if points is None else torch.as_tensor(points).to(dev, torch.float32).contiguous()
        lab = None if labels is None else torch.as_tensor(labels).to(dev, torch.int32).contiguous()
        box = None if boxes is None else torch.as_tensor(boxes).to(dev, torch.float32).contiguous()
        if pts is not None and (pts.dim() != 3 or pts.shape[2] != 2 or lab is None or tuple(lab.shape) != tuple(pts.shape[:2])):
            raise EdgeStyleHipError("decode: points are [n, P, 2] with labels [n, P]")
        if box is not None and (box.dim() != 2 or box.shape[1] != 4):
            raise EdgeStyleHipError("decode: boxes are [n, 4], one per image")
        n = emb.shape[0]
        for t in (pts, box):
            if t is not None and t.shape[0] != n:
                raise EdgeStyleHipError(f"decode: {t.shape[0]} prompts for {n} embeddings")
        p = L.SamPrompts()
        p.points, p.labels, p.boxes = (t.data_ptr() if t is not None and t.numel() else None for t in (pts, lab, box))
        p.P = pts.shape[1] if pts is not None else 0
        p.orig_h, p.orig_w = int(original_size[0]), int(original_size[1])
        return emb, p, (pts, lab, box)

    def decode(self, emb: torch.Tensor, original_size, points=None, labels=None, boxes=None, multimask: bool = True):
        """emb fp32 [n, E, grid, grid] on the device; points [n, P, 2] (x, y) and boxes [n, 4] in ORIGINAL-image pixels (boxes may be a device
        tensor, masks.get_box's), labels [n, P] -> (low-res logits fp32 [n, M, 4 grid, 4 grid], iou fp32 [n, M]), M = 3 with multimask, else 1"""
        emb, p, keep = self._prompts(emb, original_size, points, labels, boxes)
        n, M = emb.shape[0], (self.n_mask_tokens - 1 if multimask else 1)
        with torch.cuda.device(self.device):
            low = torch.empty((n, M, 4 * self.grid, 4 * self.grid), dtype=torch.float32, device=self.device)
            iou = torch.empty((n, M), dtype=torch.float32, device=self.device)
            L.check(self.lib.es_sam_decode(self._h, _ptr(emb), C.byref(p), n, int(bool(multimask)), _ptr(low), _ptr(iou), _stream_of(self.device)),
                    "es_sam_decode")
        del keep
        return low, iou

    def predict(self, emb, input_size, original_size, points=None, labels=None, boxes=None, multimask: bool = True, return_logits: bool = False):
        """es_sam_predict: decode + postprocess_masks -> (masks uint8 [n, M, H, W] (fp32 logits with return_logits), iou, low-res logits), all
        on the device.  input_size must be the prompt frame's resize of original_size (es_sam_resize_shape), which the library applies."""
        emb, p, keep = self._prompts(emb, original_size, points, labels, boxes)
        hw = (C.c_int32 * 2)()
        self.lib.es_sam_resize_shape(p.orig_h, p.orig_w, self.frame, hw)
        if (int(input_size[0]), int(input_size[1])) != (hw[0], hw[1]):
            raise EdgeStyleHipError(f"predict: input_size {tuple(input_size)} is not the frame's resize {(hw[0], hw[1])} of {tuple(original_size)}")
        n, M = emb.shape[0], (self.n_mask_tokens - 1 if multimask else 1)
        with torch.cuda.device(self.device):
            low = torch.empty((n, M, 4 * self.grid, 4 * self.grid), dtype=torch.float32, device=self.device)
            iou = torch.empty((n, M), dtype=torch.float32, device=self.device)
            out = torch.empty((n, M, p.orig_h, p.orig_w), dtype=torch.float32 if return_logits else torch.uint8, device=self.device)
            L.check(self.lib.es_sam_predict(self._h, _ptr(emb), C.byref(p), n, int(bool(multimask)), _ptr(low), _ptr(iou),
                                            None if return_logits else _ptr(out), _ptr(out) if return_logits else None, _stream_of(self.device)),
                    "es_sam_predict")
        del keep
        return out, iou, low


class NativeSamPredictor:
    """EfficientViTSamPredictor's surface (sam.py:242-457) over a NativeSamImageEncoder and a NativeSamMaskDecoder: set_image, predict,
    predict_torch, reset_image and the attributes features, original_size, input_size, is_image_set.  set_features lets one encode serve
    several predictors (the reference's five share one frozen encoder).  predict returns numpy arrays like the reference; predict_torch
    returns device tensors and reads nothing back."""

    def __init__(self, encoder, decoder: NativeSamMaskDecoder):
        self.encoder, self.decoder = encoder, decoder
        self.reset_image()

    def reset_image(self) -> None:
        self.is_image_set = False
        self.features = None
        self.original_size = None
        self.input_size = None

    def _input_size(self, original_size):
        hw = (C.c_int32 * 2)()
        L.load().es_sam_resize_shape(int(original_size[0]), int(original_size[1]), self.decoder.frame, hw)
        return (hw[0], hw[1])

    def set_features(self, features: torch.Tensor, original_size) -> None:
        """features: fp32 [1, E, 64, 64] on the device (NativeSamImageEncoder.encode_u8's), original_size: the photo's (H, W)"""
        self.reset_image()
        self.features = features
        self.original_size = (int(original_size[0]), int(original_size[1]))
        self.input_size = self._input_size(self.original_size)
        self.is_image_set = True

    def set_image(self, image, image_format: str = "RGB") -> None:
        assert image_format in ["RGB", "BGR"], f"image_format must be in ['RGB', 'BGR'], is {image_format}."
        arr = image_bytes(image)
        if image_format != "RGB":
            arr = arr[..., ::-1].copy()
        self.reset_image()
        features, _ = self.encoder.encode_u8([arr])
        self.set_features(features, arr.shape[:2])

    def _need_image(self):
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")

    def predict_device(self, point_coords=None, point_labels=None, box=None, multimask_output: bool = True, return_logits: bool = False):
        """predict without the read-back: prompts in original-image pixels (box may be a device fp32 [4] tensor, masks.get_box's) ->
        (masks [M, H, W], iou [M], low-res logits [M, 4 grid, 4 grid]) on the device"""
        self._need_image()
        if point_coords is not None:
            assert point_labels is not None, "point_labels must be supplied if point_coords is supplied."
        pts = None if point_coords is None else torch.as_tensor(point_coords)[None]
        lab = None if point_coords is None else torch.as_tensor(point_labels)[None]
        bx = None if box is None else torch.as_tensor(box).reshape(1, 4)
        m, iou, low = self.decoder.predict(self.features, self.input_size, self.original_size, pts, lab, bx, multimask_output, return_logits)
        return m[0], iou[0], low[0]

    def predict(self, point_coords=None, point_labels=None, box=None, mask_input=None, multimask_output: bool = True, return_logits: bool = False):
        self._need_image()
        if mask_input is not None:
            raise EdgeStyleHipError("NativeSamPredictor: mask_input is not supported (the reference never passes one)")
        m, iou, low = self.predict_device(point_coords, point_labels, box, multimask_output, return_logits)
        return (m.cpu().numpy() if return_logits else m.cpu().numpy().astype(bool)), iou.cpu().numpy(), low.cpu().numpy()

    def predict_torch(self, point_coords=None, point_labels=None, boxes=None, mask_input=None, multimask_output: bool = True,
                      return_logits: bool = False):
        """prompts already in the input frame, batched [B, N, 2] / [B, N] / [B, 4] -> (masks [B, M, H, W] bool or logits, iou, low-res logits)"""
        self._need_image()
        if mask_input is not None:
            raise EdgeStyleHipError("NativeSamPredictor: mask_input is not supported (the reference never passes one)")
        B = point_coords.shape[0] if point_coords is not None else boxes.shape[0]
        emb = self.features.expand(B, -1, -1, -1)
        f = self.decoder.frame
        low, iou = self.decoder.decode(emb, (f, f), point_coords, point_labels, boxes, multimask_output)      # a frame-sized "original": scale 1
        lg, m = postprocess_masks(low, self.input_size, self.original_size, f, want_logits=return_logits, want_masks=not return_logits)
        return (lg if return_logits else m.bool()), iou, low

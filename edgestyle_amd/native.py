"""Builders of a native execution context (es_ctx, include/edgestyle_hip.h): NativeEngine records one from a loaded pipeline
(this host walks the model); NativeContext, at the end of the file, has the library build it from raw state dicts
(es_load_weights: no model walk in Python at all).

The C ABI's step-level entry points — es_denoise_step (== OnnxUNetAndControlnets.forward, export_onnx.py:43-74),
es_denoise_loop (== the loop of model/edgestyle_pipeline.py:435-543) and es_vae_decode (PL:552-572) — execute recorded
launch lists (es_plan) against static device buffers.  Something has to build those once: pack the weights, allocate the
buffers and walk the model while the plans record.  That is this module; it is the only part that needs Python.  After
`NativeEngine(...)` returns, `engine.ctx` is a plain `es_ctx*` that any host can drive with raw device pointers
(INTEGRATION.md shows the C calls); the methods of _Context, which both classes share, do exactly that through ctypes and
nothing else.

The recorded pointers live in torch's graph-private memory pools (every plan is recorded inside a `torch.cuda.graph`
capture, which is also what keeps the activations of a plan from being handed to anybody else); the engine keeps those
graphs alive for as long as the context exists.  A context image of such a context is written by the library
(es_ctx_save_ranges): NativeEngine.save only tells it where torch's allocator keeps that memory.
"""
import ctypes as C
import struct
from typing import Optional, Sequence

import torch

from . import lib as L
from . import ops
from .lib import EdgeStyleHipError
from .schedulers import DDIMScheduler


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


class _Context:
    """What both builders end up with: an `es_ctx*` (self.ctx, of self.lib) and its geometry - B images per call, N = B or 2B
    samples, T steps, latent h x w, nn condition slots, the compute dtype, out_channels of the noise prediction and the
    (H, W) of an image.  The methods are thin ctypes drivers of the step-level entry points: raw device pointers in, raw
    device pointers out, and what the library refuses surfaces as EdgeStyleHipError with its text."""

    def set_options(self, cond_scales: Optional[Sequence[float]] = None, control_guidance_start: float = 0.0,
                    control_guidance_end: float = 1.0, use_graphs=True):
        """use_graphs: False = launch by launch, True = one hipGraph per plan, 2 = the whole loop as one hipGraph."""
        arr = None if cond_scales is None else (C.c_float * 6)(*([float(s) for s in cond_scales] + [1.0] * (6 - len(cond_scales))))
        L.check(self.lib.es_ctx_set_options(self.ctx, arr, control_guidance_start, control_guidance_end, int(use_graphs)),
                "es_ctx_set_options")

    def set_scheduler(self, scheduler: int):
        """L.SCHED_DDIM | L.SCHED_UNIPC (UniPCMultistepScheduler with the SD1.5 config, TT:273): the update es_denoise_loop
        applies (the recorded step list is the same)."""
        L.check(self.lib.es_ctx_set_scheduler(self.ctx, int(scheduler)), "es_ctx_set_scheduler")

    def set_alphas_cumprod(self, alphas_cumprod):
        """The scheduler's schedule (default: the library's own SD1.5 table, which equals torch's cumprod to 1e-6 only - hand
        over the scheduler's tensor where the DDIM coefficients must match a Python host's bit for bit)."""
        ac = alphas_cumprod.float().contiguous()
        L.check(self.lib.es_ctx_set_alphas_cumprod(self.ctx, ac.numpy().ctypes.data_as(C.POINTER(C.c_float)), ac.numel()),
                "es_ctx_set_alphas_cumprod")

    @staticmethod
    def _stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def denoise_step(self, sample, t: float, ehs, cond_embeds, scales=None, out=None):
        """sample [N,h,w,latent_pad], ehs [N,77,D], cond_embeds nn x [N,h,w,C0] (compute dtype, contiguous, device) -> [N,h,w,4]"""
        if out is None:
            out = torch.empty((self.N, self.h, self.w, self.out_channels), dtype=self.dtype, device=sample.device)
        ptrs = (C.c_void_p * len(cond_embeds))(*[c.data_ptr() for c in cond_embeds])
        sc = None if scales is None else (C.c_float * 6)(*([float(s) for s in scales] + [1.0] * (6 - len(scales))))
        L.check(self.lib.es_denoise_step(self.ctx, _p(sample), float(t), _p(ehs), ptrs, sc, _p(out), self._stream()), "es_denoise_step")
        return out

    def prepare_conds(self, images, noise=None):
        """images: nn x device fp32 [B,3,H,W]; noise: per slot None or device fp32 [N,L,h,w] (VAE-conditioned nets need it)"""
        imgs = [im.contiguous() for im in images]
        nz = [None if (noise is None or noise[i] is None) else noise[i].contiguous() for i in range(len(imgs))]
        ip = (C.c_void_p * len(imgs))(*[im.data_ptr() for im in imgs])
        npz = (C.c_void_p * len(imgs))(*[None if z is None else z.data_ptr() for z in nz])
        L.check(self.lib.es_prepare_conds(self.ctx, ip, npz, self._stream()), "es_prepare_conds")
        self._live = (imgs, nz)               # the copies are asynchronous: keep the sources until the next call

    def prepare_conds_u8(self, images, normalize: Sequence[bool], noise=None):
        """prepare_conds from decoded photos: nn x B uint8 HWC device tensors of any sizes (net-major: a flat list, or one list
        per net), resized, cropped and converted on the device (TT:29-48); normalize[i]: net i takes [-1,1] (the VAE-conditioned
        nets); noise as in prepare_conds."""
        nn, B = self.nn, self.B
        if len(images) == nn and not torch.is_tensor(images[0]):
            images = [im for per_net in images for im in per_net]
        if len(images) != nn * B:
            raise EdgeStyleHipError(f"prepare_conds_u8: {nn} nets x batch {B} = {nn * B} images, got {len(images)}")
        if len(normalize) != nn:
            raise EdgeStyleHipError(f"prepare_conds_u8: one normalize flag per net ({nn}), got {len(normalize)}")
        descs = ops.image_descriptors(images, "prepare_conds_u8")
        device = images[0].device
        need = ops.image_resize_workspace_bytes(descs, self.image_size[0])
        ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=device)
        nz = [None if (noise is None or noise[i] is None) else noise[i].to(device, torch.float32).contiguous() for i in range(nn)]
        npz = (C.c_void_p * nn)(*[None if z is None else z.data_ptr() for z in nz])
        nrm = (C.c_int32 * nn)(*[1 if f else 0 for f in normalize])
        L.check(self.lib.es_prepare_conds_u8(self.ctx, descs, nrm, npz, _p(ws), ws.numel(), self._stream()), "es_prepare_conds_u8")
        self._live = (list(images), nz, ws)       # asynchronous: keep the sources and the scratch until the next call

    def denoise_loop(self, latents, ehs, guidance_scale: float, timesteps):
        """latents fp32 [B,h,w,L] NHWC device (updated in place and returned); ehs [N,77,D] dtype; timesteps: host list"""
        ts = (C.c_float * len(timesteps))(*[float(t) for t in timesteps])
        L.check(self.lib.es_denoise_loop(self.ctx, _p(latents), _p(ehs), float(guidance_scale), ts, len(timesteps), self._stream()),
                "es_denoise_loop")
        return latents

    def vae_decode(self, latents, out=None):
        if out is None:
            out = torch.empty((self.B, 3) + self.image_size, dtype=torch.float32, device=latents.device)
        L.check(self.lib.es_vae_decode(self.ctx, _p(latents), _p(out), self._stream()), "es_vae_decode")
        return out

    def vae_decode_u8(self, latents, out=None):
        """vae_decode with the bytes of output_type "pil" as the result: uint8 [B,H,W,3] on the device."""
        if out is None:
            out = torch.empty((self.B,) + self.image_size + (3,), dtype=torch.uint8, device=latents.device)
        L.check(self.lib.es_vae_decode_u8(self.ctx, _p(latents), _p(out), self._stream()), "es_vae_decode_u8")
        return out

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.es_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeEngine(_Context):
    def __init__(self, pipe, batch_size: int = 1, guidance: bool = True, num_inference_steps: int = 50,
                 height: Optional[int] = None, width: Optional[int] = None, use_graphs: bool = True,
                 embed_conditions: bool = True, guess_mode: bool = False):
        """guess_mode: the recorded step is guess_mode's (CL:256-264, PL:453-459, 487-497).
        embed_conditions: also record ES_PLAN_CONDS (es_prepare_conds: RGB condition images -> embeddings), when every
        net's conditioning path is one this builder knows (VAE-conditioned ControlLoRA nets, conv-stack ControlNets)."""
        if not isinstance(pipe.scheduler, DDIMScheduler):
            raise EdgeStyleHipError("the native loop implements the DDIM update (the BASELINE metric's scheduler)")
        self.pipe, self.lib = pipe, L.load()
        dev = pipe.device
        ucfg, vcfg = pipe.unet.cfg, pipe.vae.cfg
        h = (height // vcfg.scale) if height else ucfg.sample_size
        w = (width // vcfg.scale) if width else ucfg.sample_size
        B, T = batch_size, num_inference_steps
        nn = len(pipe._nets)
        c0 = ucfg.block_out_channels[0]
        # 1. one ordinary pipeline call on placeholder inputs: builds the loop (static buffers), warms every kernel and
        #    sizes the split-K workspace
        g = torch.Generator().manual_seed(0)
        pe = torch.randn(B, 77, ucfg.cross_attention_dim, generator=g) * 0.5
        conds = [torch.randn(1, c0, h, w, generator=g) * 0.3 for _ in range(nn)]
        kw = dict(prompt_embeds=pe, negative_prompt_embeds=pe if guidance else None, image=conds if nn > 1 else conds[0],
                  latents=torch.randn(B, ucfg.in_channels, h, w, generator=g), guidance_scale=7.5 if guidance else 1.0,
                  num_inference_steps=T, guess_mode=bool(guess_mode))
        pipe(output_type="pt", **kw)
        guess = self.guess = bool(guess_mode)
        loop = self.loop = pipe._loops[(B, guidance, h, w, guess)]
        runner = self.runner = pipe._runner
        N = loop.N
        # the coefficient table the recorded scheduler call reads: room for UniPC's 12 columns (es_ctx_set_scheduler), the DDIM
        # rows the pipeline call left there in front
        self._coef = torch.zeros((T * 12,), dtype=torch.float32, device=dev)
        self._coef[:T * 4].copy_(loop.coef.reshape(-1))
        loop.coef = self._coef[:T * 4].view(T, 4)
        self.B, self.N, self.T, self.h, self.w, self.nn = B, N, T, h, w, nn
        self.dtype, self.out_channels, self.image_size = pipe.dtype, ucfg.out_channels, (h * vcfg.scale, w * vcfg.scale)
        self.ts_dev = torch.zeros((T,), dtype=torch.float32, device=dev)
        self.ts_dev.copy_(pipe.scheduler.set_timesteps(T).float())
        grouped_tables = runner.mode == "grouped" and not guess
        n_cn = loop.conds[0].shape[0]

        def prep():
            runner.state = loop.state
            runner.set_context(loop.ehs, guess, n_cn)
            if grouped_tables:
                runner.set_conds(loop.conds)
                runner.set_time_table(self.ts_dev, N)

        def generic():
            runner.state = loop.state
            runner.set_context(loop.ehs, guess, n_cn)
            if grouped_tables:
                runner.set_conds(loop.conds)
            runner.step(loop.model_in, loop.t_rows, loop.conds, [1.0] * nn, loop.scales_cur, out=loop.noise, step_idx=None,
                        guess_mode=guess)

        out = {}

        def decode():
            dec = pipe.vae.decode_nhwc(loop.model_in[:B], unscaled_latents=True)
            out["img"] = ops.nhwc_to_nchw(dec, channels=3, scale=0.5, shift=0.5, clamp01=True)

        # -- es_prepare_conds: static inputs + the embedding walk of pipeline.prepare_images as C-ABI launches only --------
        self.cond_img, self.cond_noise = [None] * nn, [None] * nn
        conds_fn = self._conds_fn(pipe, loop, B, guidance and not guess, h, w) if embed_conditions else None

        self._keep = []
        ctx = C.c_void_p()
        L.check(self.lib.es_ctx_create(dev.index or 0, C.byref(ctx)), "es_ctx_create")
        self.ctx = ctx
        geo = L.CtxGeometry(B=B, cfg=int(guidance), h=h, w=w, latent_channels=ucfg.in_channels,
                            latent_pad=pipe.unet.engine.in_pad, n_conds=nn, n_steps=T, dtype=L.ES_F16 if self.dtype == torch.float16 else L.ES_BF16,
                            guess_mode=int(guess))
        L.check(self.lib.es_ctx_set_geometry(ctx, C.byref(geo)), "es_ctx_set_geometry")
        self.plan_sizes = {}
        todo = [(L.PLAN_PREP, prep), (L.PLAN_STEP, loop.one_step), (L.PLAN_STEP_GENERIC, generic), (L.PLAN_DECODE, decode)]
        if conds_fn is not None:
            todo.append((L.PLAN_CONDS, conds_fn))
        if grouped_tables:
            # steps outside the control-guidance window (PL:419-427): the UNet alone + the fusion-of-zeros constants
            runner.state = loop.state
            runner.prepare_fused_zero(N)
            todo.append((L.PLAN_STEP_UNET, loop.one_step_unet))
        for which, fn in todo:
            fn()                                     # eager: anything that allocates scratch does it outside the capture
            torch.cuda.synchronize()
            plan = C.c_void_p(self.lib.es_plan_create())
            graph = torch.cuda.CUDAGraph()
            L.check(self.lib.es_plan_begin_record(plan), "es_plan_begin_record")
            try:
                with torch.cuda.graph(graph):
                    fn()
            finally:
                L.check(self.lib.es_plan_end_record(plan), "es_plan_end_record")
            self._keep.append(graph)                 # owns the memory the plan's pointers refer to
            self.plan_sizes[which] = self.lib.es_plan_size(plan)
            L.check(self.lib.es_ctx_set_plan(ctx, which, plan), "es_ctx_set_plan")
        self.image = out["img"]
        binds = {L.BUF_SAMPLE: loop.model_in, L.BUF_T_ROWS: loop.t_rows, L.BUF_EHS: loop.ehs, L.BUF_SCALES: loop.scales_cur,
                 L.BUF_NOISE: loop.noise, L.BUF_LATENTS: loop.latents, L.BUF_STEP_IDX: loop.step_idx, L.BUF_T_TABLE: loop.t_table,
                 L.BUF_SCALE_TABLE: loop.scale_table, L.BUF_COEF: self._coef, L.BUF_TIMESTEPS: self.ts_dev, L.BUF_IMAGE: self.image}
        for i in range(3):
            binds[L.BUF_HIST0 + i] = loop.hist[i]
        for i, c in enumerate(loop.conds):
            binds[L.BUF_COND0 + i] = c
            if conds_fn is not None:
                binds[L.BUF_COND_IMG0 + i] = self.cond_img[i]
                if self.cond_noise[i] is not None:
                    binds[L.BUF_COND_NOISE0 + i] = self.cond_noise[i]
        for slot, t in binds.items():
            L.check(self.lib.es_ctx_bind(ctx, slot, _p(t), t.numel() * t.element_size()), "es_ctx_bind")
        self.set_alphas_cumprod(pipe.scheduler.alphas_cumprod)
        self.set_options(use_graphs=use_graphs)
        # The recorded plans hold raw pointers into this loop's static buffers and StepState tensors (time-projection table,
        # batch-concatenated conditions, text K/V projections): the loop becomes PRIVATE to the engine.  It leaves the
        # pipeline's cache - a later pipe(...) with the same (B, cfg, h, w) builds its own loop and may replace ITS tables
        # (another num_inference_steps re-allocates tproj_table) without freeing anything a plan still reads - and every
        # tensor the plans can reference is pinned here for the life of the context.
        pipe._loops.pop((B, guidance, h, w, guess), None)
        if getattr(pipe, "_last_loop", None) is loop:
            pipe._last_loop = None
        from .models import StepState
        pinned = []

        def pin(o):
            if torch.is_tensor(o):
                pinned.append(o)
            elif isinstance(o, (list, tuple)):
                for x in o:
                    pin(x)
        for v in vars(loop.state).values():
            pin(v)
        for v in vars(loop).values():
            pin(v)
        self._keep.append(pinned)
        if runner.state is loop.state:
            runner.state = StepState()               # stand-alone StepRunner calls get a fresh default state again

    def _conds_fn(self, pipe, loop, B, guidance, h, w):
        """The one-time conditioning embedding (PL:352-377, 629-664; CL:28-42, 289-290) as pipeline.prepare_images does it -
        each shared encoder once over the un-duplicated images of all its nets, the VAE sampling noise per CFG half -
        on static inputs and through C-ABI launches only, so that a plan can record it.  None if a net's conditioning
        path is not one of the two known ones."""
        from .models import ControlLoRAModel, ControlNetModel
        nets = pipe._nets
        dev, dt = pipe.device, self.dtype
        rep = 2 if guidance else 1
        N = B * rep
        groups = {}
        for i, net in enumerate(nets):
            if isinstance(net, ControlLoRAModel) and net.config.uses_vae:
                if net._vae is None:
                    return None
                groups.setdefault(("vae", id(net._vae)), []).append(i)
            elif isinstance(net, ControlNetModel):
                groups.setdefault(("stack", id(net)), []).append(i)
            else:
                return None
        scale = pipe.vae.cfg.scale
        H, W = h * scale, w * scale
        gbufs = []
        for (kind, _), idx in groups.items():
            gb = torch.zeros((len(idx) * B, 3, H, W), dtype=torch.float32, device=dev)
            gbufs.append(gb)
            for k, i in enumerate(idx):
                self.cond_img[i] = gb[k * B:(k + 1) * B]
                if kind == "vae":
                    self.cond_noise[i] = torch.zeros((N, nets[i]._vae.cfg.latent_channels, h, w), dtype=torch.float32, device=dev)

        def fn():
            for ((kind, _), idx), gb in zip(groups.items(), gbufs):
                x8 = ops.nchw_to_nhwc(gb, dt, 8)
                if kind == "vae":
                    vae = nets[idx[0]]._vae
                    mom = vae.engine.encode_moments(x8)               # one encoder pass for all its nets, no CFG copy
                    for k, i in enumerate(idx):
                        mk = mom[k * B:(k + 1) * B]
                        if rep > 1:
                            mn = torch.empty((N,) + tuple(mk.shape[1:]), dtype=mk.dtype, device=dev)
                            ops.memcpy(mn[:B], mk)
                            ops.memcpy(mn[B:], mk)
                        else:
                            mn = mk
                        z = ops.vae_sample(mn, self.cond_noise[i], vae.cfg.latent_channels, nets[i].engine.in_pad, vae.cfg.scaling_factor)
                        ops.memcpy(loop.conds[i], nets[i].engine.embed_latent(z))
                else:
                    emb = nets[idx[0]].engine.embed_cond(x8)
                    for k, i in enumerate(idx):
                        e = emb[k * B:(k + 1) * B]
                        ops.memcpy(loop.conds[i][:B], e)
                        if rep > 1:
                            ops.memcpy(loop.conds[i][B:], e)
        return fn

    # -- the drivers of _Context, behind the checks this host can make: it holds the tensors the plans were recorded on ----------
    def denoise_step(self, sample: torch.Tensor, t: float, ehs: torch.Tensor, cond_embeds: Sequence[torch.Tensor],
                     scales: Optional[Sequence[float]] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        loop = self.loop
        for a, b in [(sample, loop.model_in), (ehs, loop.ehs)] + list(zip(cond_embeds, loop.conds)):
            if a.shape != b.shape or a.dtype != b.dtype or not a.is_contiguous() or not a.is_cuda:
                raise EdgeStyleHipError(f"denoise_step: expected a contiguous device tensor {tuple(b.shape)} {b.dtype}")
        return super().denoise_step(sample, t, ehs, cond_embeds, scales, out)

    def set_conds(self, cond_embeds: Sequence[torch.Tensor]):
        """The loop reads the condition embeddings last placed in the context's slots."""
        for dst, src in zip(self.loop.conds, cond_embeds):
            ops.memcpy(dst, src.contiguous())

    def denoise_loop(self, latents: torch.Tensor, ehs: torch.Tensor, guidance_scale: float,
                     timesteps: Optional[Sequence[float]] = None) -> torch.Tensor:
        if timesteps is None:
            timesteps = self.pipe.scheduler.set_timesteps(self.T).tolist()
        if latents.shape != self.loop.latents.shape or latents.dtype != torch.float32 or not latents.is_contiguous():
            raise EdgeStyleHipError(f"denoise_loop: latents must be fp32 contiguous {tuple(self.loop.latents.shape)}")
        return super().denoise_loop(latents, ehs.contiguous(), guidance_scale, timesteps)

    def _need_conds_plan(self):
        if L.PLAN_CONDS not in self.plan_sizes:
            raise EdgeStyleHipError("this context was built without ES_PLAN_CONDS")

    def prepare_conds(self, images: Sequence[torch.Tensor], noise: Optional[Sequence[Optional[torch.Tensor]]] = None):
        self._need_conds_plan()
        imgs = [im.to(self.pipe.device, torch.float32) for im in images]
        nz = [None if (noise is None or noise[i] is None) else noise[i].to(self.pipe.device, torch.float32) for i in range(len(imgs))]
        for i, im in enumerate(imgs):
            if im.shape != self.cond_img[i].shape:
                raise EdgeStyleHipError(f"prepare_conds: image {i} must be {tuple(self.cond_img[i].shape)}")
            if nz[i] is not None and self.cond_noise[i] is not None and nz[i].shape != self.cond_noise[i].shape:
                raise EdgeStyleHipError(f"prepare_conds: noise {i} must be {tuple(self.cond_noise[i].shape)}")
        super().prepare_conds(imgs, nz)

    def prepare_conds_u8(self, images, normalize: Sequence[bool], noise: Optional[Sequence[Optional[torch.Tensor]]] = None):
        self._need_conds_plan()
        super().prepare_conds_u8(images, normalize, noise)

    # -- context image: everything es_ctx_load needs to run this context without Python ---------------------------------
    def save(self, path: str) -> dict:
        """Write a context image for es_ctx_load (include/edgestyle_hip.h).  The library writes it (es_ctx_save_ranges: typed
        relocation into one arena that keeps the layout of every referenced allocator segment; only memory that the plans
        read and never write travels as data).  What only this host knows is where torch's allocator keeps the memory the
        recorded pointers refer to: its segments, and the blocks inside them - an activation freed during a capture is an
        inactive block the captured kernels still write."""
        torch.cuda.synchronize()
        dev_index = self.pipe.device.index or 0
        segs, blks = [], []
        for seg in torch.cuda.memory_snapshot():
            if seg.get("device", dev_index) != dev_index:
                continue
            segs.append((seg["address"], seg["total_size"]))
            a = seg["address"]
            for bk in seg.get("blocks", []):
                blks.append((bk.get("address", a), bk["size"]))
                a = bk.get("address", a) + bk["size"]
        info = L.CtxImageInfo()
        L.check(self.lib.es_ctx_save_ranges(self.ctx, str(path).encode(), (L.MemRange * len(segs))(*segs), len(segs),
                                            (L.MemRange * len(blks))(*blks), len(blks), C.byref(info)), "es_ctx_save_ranges")
        return dict(blocks=info.segments, arena_bytes=info.arena_bytes, data_bytes=info.data_bytes, extents=info.extents,
                    relocations={w: info.relocations[w] for w in range(L.PLAN_COUNT) if self.lib.es_ctx_plan(self.ctx, w)})

    def close(self):
        super().close()
        self._keep.clear()


# ======================================================================================================================
# es_load_weights: the same context, built by the library itself from raw tensors (no model walk in Python)
# ======================================================================================================================
def model_config(ucfg, vcfg, text_tokens: int = 77) -> "L.ModelConfig":
    """es_model_config of a UNetConfig / VAEConfig pair (edgestyle_amd/config.py)."""
    m = L.ModelConfig()
    m.in_channels, m.out_channels = ucfg.in_channels, ucfg.out_channels
    m.n_blocks = len(ucfg.block_out_channels)
    for i, c in enumerate(ucfg.block_out_channels):
        m.block_out_channels[i] = c
        m.down_has_attn[i] = int(ucfg.down_has_attn[i])
    m.layers_per_block, m.num_heads = ucfg.layers_per_block, ucfg.num_heads
    m.cross_attention_dim, m.norm_num_groups, m.norm_eps = ucfg.cross_attention_dim, ucfg.norm_num_groups, ucfg.norm_eps
    m.n_cond_embed = len(ucfg.conditioning_embedding_out_channels)
    for i, c in enumerate(ucfg.conditioning_embedding_out_channels):
        m.cond_embed_channels[i] = c
    m.conditioning_channels, m.text_tokens = ucfg.conditioning_channels, text_tokens
    m.vae_n_blocks = len(vcfg.block_out_channels)
    for i, c in enumerate(vcfg.block_out_channels):
        m.vae_block_out_channels[i] = c
    m.vae_layers_per_block, m.vae_latent_channels = vcfg.layers_per_block, vcfg.latent_channels
    m.vae_norm_num_groups, m.vae_norm_eps, m.vae_scaling_factor = vcfg.norm_num_groups, vcfg.norm_eps, vcfg.scaling_factor
    return m


_TENSOR_DT = {torch.float32: L.ES_F32, torch.float16: L.ES_F16, torch.bfloat16: L.ES_BF16}


def state_dict_descriptors(sd):
    """{key: tensor (host, or on the GPU the context is built for)} -> (es_state_dict, keep-alive list): descriptors only."""
    arr = (L.Tensor * max(len(sd), 1))()
    keep = [arr]
    for i, (k, v) in enumerate(sd.items()):
        if v.device.type not in ("cpu", "cuda") or v.dtype not in _TENSOR_DT:
            raise EdgeStyleHipError(f"es_load_weights takes host tensors in fp32 / fp16 / bf16: {k} is {v.dtype} on {v.device}")
        v = v.contiguous()
        kb = k.encode()
        keep += [v, kb]
        arr[i].key, arr[i].data, arr[i].ndim, arr[i].dtype = kb, v.data_ptr(), v.dim(), _TENSOR_DT[v.dtype]
        if v.dim() < 1 or v.dim() > 4:
            raise EdgeStyleHipError(f"{k}: tensors of 1..4 dimensions")
        for j, s in enumerate(v.shape):
            arr[i].shape[j] = s
    return L.StateDict(arr, len(sd)), keep


class NativeContext(_Context):
    """A context built by es_load_weights (include/edgestyle_hip.h) from state dicts in the reference's key layout, and thin
    ctypes drivers of the step-level entry points on raw device pointers.  Nothing of edgestyle_amd's model code (models.py,
    engine.py, ops.py) is involved: torch only hands over host pointers at build time and device pointers at run time.

    ws: {"unet", "vae", "fusion", <controlnet names>} state dicts; `controlnets`: [(name in ws, L.NET_*)] the distinct nets;
    net_of_cond: which of them serves each of the six condition slots (TT:252-258) - or ONE entry for a single ControlNet whose
    residuals go to the UNet without fusion blocks (PL:338-351; no "fusion" dict then).  device < 0: dry build (no GPU)."""

    def __init__(self, ws, ucfg, vcfg, batch_size: int = 1, guidance: bool = True, num_inference_steps: int = 50,
                 height: Optional[int] = None, width: Optional[int] = None, dtype=torch.float16, device: int = 0,
                 controlnets=(("lora0", L.NET_CONTROL_LORA_VAE), ("openpose", L.NET_CONTROLNET), ("lora1", L.NET_CONTROL_LORA_VAE)),
                 net_of_cond=(0, 1, 2, 1, 2, 1), guess_mode: bool = False):
        self.lib = L.load()
        self.ucfg, self.vcfg = ucfg, vcfg
        h = (height // vcfg.scale) if height else ucfg.sample_size
        w = (width // vcfg.scale) if width else ucfg.sample_size
        nn = len(net_of_cond)
        self.B, self.N, self.T, self.h, self.w, self.nn = batch_size, batch_size * (2 if guidance else 1), num_inference_steps, h, w, nn
        self.dtype, self.device = dtype, device
        self.out_channels, self.image_size = ucfg.out_channels, (h * vcfg.scale, w * vcfg.scale)
        wts = L.Weights()
        keep = []
        for name in ("unet", "vae", "fusion"):
            if name == "fusion" and nn == 1:
                continue
            d, k = state_dict_descriptors(ws[name])
            setattr(wts, name, d)
            keep.append(k)
        for i, (name, kind) in enumerate(controlnets):
            d, k = state_dict_descriptors(ws[name])
            wts.controlnet[i], wts.controlnet_kind[i] = d, kind
            keep.append(k)
        wts.n_controlnets = len(controlnets)
        for i, n in enumerate(net_of_cond):
            wts.net_of_cond[i] = n
        geo = L.CtxGeometry(B=batch_size, cfg=int(guidance), h=h, w=w, latent_channels=ucfg.in_channels,
                            latent_pad=(ucfg.in_channels + 7) // 8 * 8, n_conds=nn, n_steps=num_inference_steps,
                            dtype=L.ES_F16 if dtype == torch.float16 else L.ES_BF16, guess_mode=int(bool(guess_mode)))
        mc = model_config(ucfg, vcfg)
        ctx = C.c_void_p()
        L.check(self.lib.es_load_weights(C.byref(wts), C.byref(mc), C.byref(geo), device, C.byref(ctx)), "es_load_weights")
        self.ctx = ctx
        self.uses_noise = [controlnets[n][1] == L.NET_CONTROL_LORA_VAE for n in net_of_cond]
        del keep

    def plan_size(self, which: int) -> int:
        return self.lib.es_ctx_plan_size(self.ctx, which)


def plan_ops(lib, plan):
    """[(op kind, argument record, [positions of its pointer fields inside the record])] of an es_plan*, array ops expanded:
    the one reader in Python of an exported plan (es_plan_export: u64 n_ops, u64 blob bytes, n_ops x {i64 kind, u64 offset,
    u64 bytes}, blob) and of the library's pointer-field tables (es_plan_pointer_fields)."""
    if not plan:
        return []
    n = lib.es_plan_export(plan, None, 0)
    raw = (C.c_char * n)()
    lib.es_plan_export(plan, raw, n)
    img = bytes(raw)
    blob0 = 16 + 24 * int.from_bytes(img[:8], "little")
    out, fields = [], {}
    for kind, off, nbytes in struct.iter_unpack("<qQQ", img[16:blob0]):
        if kind not in fields:
            offs, uses, elem = (C.c_int32 * 64)(), (C.c_int32 * 64)(), C.c_int32(0)
            k = lib.es_plan_pointer_fields(kind, offs, uses, 64, C.byref(elem))
            fields[kind] = (offs[:k], elem.value)
        fl, elem = fields[kind]
        reps = max(1, nbytes // elem) if elem else 1
        out.append((kind, img[blob0 + off:blob0 + off + nbytes], [r * elem + fo for r in range(reps) for fo in fl]))
    return out


def plan_records(lib, ctx, which: int):
    """[(op kind, argument record with every pointer field replaced by 0 / 1 = null / set)] of one plan of a context: what two
    builders must agree on call by call (the addresses themselves belong to each builder's allocator)."""
    out = []
    for kind, rec, fields in plan_ops(lib, lib.es_ctx_plan(ctx, which)):
        rec = bytearray(rec)
        for pos in fields:
            rec[pos:pos + 8] = bytes([1 if any(rec[pos:pos + 8]) else 0]) + bytes(7)
        out.append((kind, bytes(rec)))
    return out

"""ctypes binding of libedgestyle_hip.so (the C ABI declared in include/edgestyle_hip.h).

The product path has NO fallback: if the shared library is missing or an entry point fails, this raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ES_HIP_LIB: tools only (ablation / experimental kernel builds); the product always loads the in-tree library
LIB_PATH = os.environ.get("ES_HIP_LIB") or os.path.join(_HERE, "lib", "libedgestyle_hip.so")

ES_F16, ES_BF16, ES_F32 = 0, 1, 2
ABI_VERSION = 7          # include/edgestyle_hip.h ES_ABI_VERSION
ACT_NONE, ACT_SILU, ACT_GEGLU, ACT_GELU_TANH = 0, 1, 2, 3


class GemmDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("x2", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("temb", C.c_void_p),
        ("residual", C.c_void_p), ("out_scale_dev", C.c_void_p), ("out", C.c_void_p), ("workspace", C.c_void_p),
        ("prof", C.c_void_p),
        ("N", C.c_int32), ("Hsrc", C.c_int32), ("Wsrc", C.c_int32), ("C1", C.c_int32), ("C2", C.c_int32),
        ("Hout", C.c_int32), ("Wout", C.c_int32), ("Cout", C.c_int32),
        ("rows_padded", C.c_int32), ("Kpad", C.c_int32),
        ("ksize", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
        ("upsample", C.c_int32), ("temb_stride", C.c_int32), ("act", C.c_int32), ("splitk", C.c_int32),
        ("bn", C.c_int32), ("dtype", C.c_int32),
        ("ngroups", C.c_int32), ("mt_end", C.c_int32 * 4), ("w_g", C.c_void_p * 4), ("bias_g", C.c_void_p * 4),
        ("stages", C.c_int32), ("xcd_m_fastest", C.c_int32), ("waves", C.c_int32),
        ("out_scale", C.c_float),
        ("ln_colsum", C.c_void_p), ("ln_colsum_g", C.c_void_p * 4), ("ln_eps", C.c_float),
        ("t1", C.c_void_p), ("t2", C.c_void_p), ("Ct1", C.c_int32), ("Ct2", C.c_int32),
        ("x_nmod", C.c_int32), ("korder", C.c_int32), ("residual_lo", C.c_void_p), ("out_lo", C.c_void_p),
        ("gn_part", C.c_void_p), ("gn_groups", C.c_int32),
    ]


class XsDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("out", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p),
        ("w_g", C.c_void_p * 4), ("bias_g", C.c_void_p * 4), ("prof", C.c_void_p),
        ("mt_end", C.c_int32 * 4), ("ngroups", C.c_int32),
        ("M", C.c_int32), ("K", C.c_int32), ("Cout", C.c_int32), ("rows_padded", C.c_int32),
        ("ldo", C.c_int32), ("geglu", C.c_int32), ("ln", C.c_int32), ("ln_eps", C.c_float),
        ("nslices", C.c_int32), ("chunks_per_slice", C.c_int32), ("dtype", C.c_int32),
        ("residual", C.c_void_p),
        ("gn_part", C.c_void_p), ("gn_gamma", C.c_void_p), ("gn_beta", C.c_void_p), ("gn_gamma_g", C.c_void_p * 4), ("gn_beta_g", C.c_void_p * 4),
        ("gn_groups", C.c_int32), ("gn_nchunk", C.c_int32), ("gn_hw", C.c_int32), ("gn_eps", C.c_float),
    ]


class CtxGeometry(C.Structure):
    _fields_ = [("B", C.c_int32), ("cfg", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("latent_channels", C.c_int32), ("latent_pad", C.c_int32), ("n_conds", C.c_int32),
                ("n_steps", C.c_int32), ("dtype", C.c_int32), ("guess_mode", C.c_int32)]


# es_plan / es_ctx enums (include/edgestyle_hip.h)
PLAN_STEP_GENERIC, PLAN_PREP, PLAN_STEP, PLAN_DECODE, PLAN_CONDS, PLAN_STEP_UNET = 0, 1, 2, 3, 4, 5
PLAN_COUNT = 6
(BUF_SAMPLE, BUF_T_ROWS, BUF_EHS, BUF_COND0, BUF_COND1, BUF_COND2, BUF_COND3, BUF_COND4, BUF_COND5, BUF_SCALES, BUF_NOISE,
 BUF_LATENTS, BUF_STEP_IDX, BUF_T_TABLE, BUF_SCALE_TABLE, BUF_COEF, BUF_TIMESTEPS, BUF_IMAGE) = range(18)
BUF_COND_IMG0, BUF_COND_NOISE0 = 18, 24          # + net index
BUF_HIST0, BUF_COUNT = 30, 33                    # UniPC state slots (+ 0..2)
SCHED_DDIM, SCHED_UNIPC = 0, 1
OP_CONV_GEMM, OP_LINEAR_XS, OP_ATTENTION = 1, 2, 3      # csrc/plan.h es_op_kind (es_plan_count)


class MemRange(C.Structure):        # es_mem_range
    _fields_ = [("addr", C.c_uint64), ("bytes", C.c_uint64)]


class CtxImageInfo(C.Structure):    # es_ctx_image_info
    _fields_ = [("arena_bytes", C.c_uint64), ("data_bytes", C.c_uint64), ("segments", C.c_int32), ("extents", C.c_int32),
                ("relocations", C.c_int32 * PLAN_COUNT)]


class AttnDesc(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("o", C.c_void_p),
        ("N", C.c_int32), ("heads", C.c_int32), ("Sq", C.c_int32), ("Skv", C.c_int32), ("d", C.c_int32),
        ("ldq", C.c_int32), ("ldk", C.c_int32), ("ldv", C.c_int32), ("ldo", C.c_int32),
        ("bsq", C.c_int64), ("bsk", C.c_int64), ("bsv", C.c_int64), ("bso", C.c_int64),
        ("scale", C.c_float), ("dtype", C.c_int32),
    ]


class AttnKnobs(C.Structure):       # es_attn_knobs
    _fields_ = [("big_thr", C.c_int64), ("kvres", C.c_int32), ("attn32", C.c_int32), ("qb", C.c_int32), ("pp", C.c_int32)]


class XsKnobs(C.Structure):         # es_xs_knobs
    _fields_ = [("pp", C.c_int32)]


class GnDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("x2", C.c_void_p), ("out", C.c_void_p),
        ("gamma", C.c_void_p), ("beta", C.c_void_p), ("partials", C.c_void_p),
        ("N", C.c_int32), ("HW", C.c_int32), ("C1", C.c_int32), ("C2", C.c_int32), ("groups", C.c_int32),
        ("eps", C.c_float), ("silu", C.c_int32), ("dtype", C.c_int32),
        ("ngroups", C.c_int32), ("n_end", C.c_int32 * 4), ("gamma_g", C.c_void_p * 4), ("beta_g", C.c_void_p * 4),
        ("ext_chunks", C.c_int32), ("stats_only", C.c_int32),
    ]


class LnDesc(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("out", C.c_void_p), ("gamma_g", C.c_void_p * 4), ("beta_g", C.c_void_p * 4),
        ("row_end", C.c_int32 * 4), ("ngroups", C.c_int32), ("M", C.c_int32), ("C", C.c_int32),
        ("eps", C.c_float), ("dtype", C.c_int32),
    ]


class FusionDesc(C.Structure):
    _fields_ = [
        ("res", C.c_void_p * 6), ("res_bs", C.c_int64 * 6),
        ("w1", C.c_void_p), ("b1", C.c_void_p), ("g1", C.c_void_p), ("be1", C.c_void_p),
        ("w2", C.c_void_p), ("b2", C.c_void_p), ("g2", C.c_void_p), ("be2", C.c_void_p),
        ("w3", C.c_void_p), ("b3", C.c_void_p),
        ("scratch", C.c_void_p), ("u", C.c_void_p), ("out", C.c_void_p),
        ("res_scale_dev", C.c_void_p), ("addend", C.c_void_p),
        ("res_scale", C.c_float * 6),
        ("N", C.c_int32), ("HW", C.c_int32), ("C", C.c_int32),
        ("eps", C.c_float), ("dtype", C.c_int32),
    ]


class ImageU8(C.Structure):         # es_image_u8
    _fields_ = [("data", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32), ("row_stride", C.c_int64)]


class JpegInfo(C.Structure):        # es_jpeg_info
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("components", C.c_int32), ("h", C.c_int32 * 3), ("v", C.c_int32 * 3),
                ("tq", C.c_int32 * 3), ("td", C.c_int32 * 3), ("ta", C.c_int32 * 3), ("hmax", C.c_int32), ("vmax", C.c_int32),
                ("mcus_x", C.c_int32), ("mcus_y", C.c_int32), ("blocks_w", C.c_int32 * 3), ("blocks_h", C.c_int32 * 3),
                ("restart_interval", C.c_int32)]


class JpegEncodeParams(C.Structure):    # es_jpeg_encode_params
    _fields_ = [("quality", C.c_int32), ("subsampling", C.c_int32), ("restart_interval", C.c_int32)]


JPEG_TABLES_BYTES = 8560            # ES_JPEG_TABLES_BYTES


class Philox(C.Structure):          # es_philox
    _fields_ = [("seed", C.c_uint64), ("offset", C.c_uint64)]


class RandnDesc(C.Structure):       # es_randn_desc
    _fields_ = [("seed", C.c_uint64), ("offset", C.c_uint64), ("numel", C.c_int64), ("blocks", C.c_int32), ("scale", C.c_float),
                ("round_dtype", C.c_int32), ("N", C.c_int64), ("C", C.c_int64), ("HW", C.c_int64), ("Cstride", C.c_int64)]


class TextConfig(C.Structure):      # es_text_config
    _fields_ = [(n, C.c_int32) for n in ("vocab_size", "hidden", "heads", "layers", "intermediate", "max_positions")] + \
        [("ln_eps", C.c_float), ("act", C.c_int32)]


class ClipVisionConfig(C.Structure):    # es_clip_vision_config
    _fields_ = [(n, C.c_int32) for n in ("image_size", "patch_size", "hidden", "heads", "layers", "intermediate", "projection_dim")] + \
        [("ln_eps", C.c_float), ("act", C.c_int32), ("image_mean", C.c_float * 3), ("image_std", C.c_float * 3)]


class SamConfig(C.Structure):       # es_sam_config
    _fields_ = [("image_size", C.c_int32), ("width", C.c_int32 * 5), ("depth", C.c_int32 * 5), ("qkv_dim", C.c_int32), ("head_width", C.c_int32),
                ("head_depth", C.c_int32), ("out_dim", C.c_int32), ("bn_eps", C.c_float), ("ln_eps", C.c_float),
                ("pixel_mean", C.c_float * 3), ("pixel_std", C.c_float * 3)]


class SamPromptDesc(C.Structure):  # es_sam_prompt_desc
    _fields_ = [(n, C.c_void_p) for n in ("gauss", "point_embeddings", "not_a_point", "iou_token", "mask_tokens", "points", "labels", "boxes",
                                          "tokens", "query_pe")] + \
        [(n, C.c_int32) for n in ("n", "P", "embed_dim", "n_mask_tokens", "frame", "orig_h", "orig_w", "dtype")]


class LinearTokensDesc(C.Structure):    # es_linear_tokens_desc
    _fields_ = [(n, C.c_void_p) for n in ("x", "w", "bias", "residual", "out")] + \
        [(n, C.c_int32) for n in ("n", "rows", "K", "N", "ldx", "ldr", "ldo")] + [(n, C.c_int64) for n in ("bsx", "bsr", "bso")] + \
        [(n, C.c_int32) for n in ("per_row_weights", "relu", "dtype")]


class SamDecoderConfig(C.Structure):    # es_sam_decoder_config
    _fields_ = [(n, C.c_int32) for n in ("embed_dim", "heads", "mlp_dim", "depth", "grid", "frame", "n_mask_tokens", "iou_hidden", "iou_depth",
                                         "attn_downsample")] + [("ln_eps", C.c_float), ("ln2d_eps", C.c_float)]


class SamPrompts(C.Structure):          # es_sam_prompts
    _fields_ = [(n, C.c_void_p) for n in ("points", "labels", "boxes", "mask_input")] + [(n, C.c_int32) for n in ("P", "orig_h", "orig_w")]


class SamUpscaleDesc(C.Structure):  # es_sam_upscale_desc
    _fields_ = [(n, C.c_void_p) for n in ("g", "w_packed", "ln_gamma", "ln_beta", "bias2", "hyper", "out")] + \
        [(n, C.c_int32) for n in ("n", "grid_h", "grid_w", "C1", "M", "ldh")] + [("bsh", C.c_int64), ("ln_eps", C.c_float), ("dtype", C.c_int32)]


FILTER_BILINEAR, FILTER_BICUBIC = 0, 1           # ES_FILTER_*
FILTER_LANCZOS = 2                               # ... es_image_resize_coeffs_ex and the windowed calls only
CROP_TORCHVISION, CROP_TRANSFORMERS = 0, 1       # ES_CROP_*
MASK_AND, MASK_OR, MASK_ANDNOT = 0, 1, 2         # ES_MASK_*


class Tensor(C.Structure):          # es_tensor
    _fields_ = [("key", C.c_char_p), ("data", C.c_void_p), ("shape", C.c_int64 * 4), ("ndim", C.c_int32), ("dtype", C.c_int32)]


class StateDict(C.Structure):       # es_state_dict
    _fields_ = [("tensors", C.POINTER(Tensor)), ("count", C.c_int32)]


NET_CONTROLNET, NET_CONTROL_LORA_VAE, NET_CONTROL_LORA = 0, 1, 2


class Weights(C.Structure):         # es_weights
    _fields_ = [("unet", StateDict), ("vae", StateDict), ("fusion", StateDict), ("controlnet", StateDict * 6),
                ("controlnet_kind", C.c_int32 * 6), ("n_controlnets", C.c_int32), ("net_of_cond", C.c_int32 * 6)]


class ModelConfig(C.Structure):     # es_model_config
    _fields_ = [("in_channels", C.c_int32), ("out_channels", C.c_int32),
                ("n_blocks", C.c_int32), ("block_out_channels", C.c_int32 * 4), ("down_has_attn", C.c_int32 * 4),
                ("layers_per_block", C.c_int32), ("num_heads", C.c_int32), ("cross_attention_dim", C.c_int32),
                ("norm_num_groups", C.c_int32), ("norm_eps", C.c_float),
                ("n_cond_embed", C.c_int32), ("cond_embed_channels", C.c_int32 * 4), ("conditioning_channels", C.c_int32),
                ("text_tokens", C.c_int32),
                ("vae_n_blocks", C.c_int32), ("vae_block_out_channels", C.c_int32 * 4), ("vae_layers_per_block", C.c_int32),
                ("vae_latent_channels", C.c_int32), ("vae_norm_num_groups", C.c_int32),
                ("vae_norm_eps", C.c_float), ("vae_scaling_factor", C.c_float)]


_I32 = C.c_int32


class LaunchQuery(C.Structure):     # es_launch_query
    _fields_ = [(n, C.c_longlong) for n in ("M", "hw", "w_numel", "src_numel")] + \
        [(n, _I32) for n in ("ksize", "stride", "upsample", "C1", "C2", "rows_padded", "kpad", "cin", "ctail", "cout", "geglu", "has_ln", "act",
                             "has_temb", "has_residual", "residual_dense", "unit_scale", "n_tails", "x_rep", "wide", "dtype", "gn_groups",
                             "ngroups", "n_counts")] + [("group_n", _I32 * 4)] + [(n, _I32) for n in ("groups_agree", "force_splitk", "stages")]


class LaunchKnobs(C.Structure):     # es_launch_knobs
    _fields_ = [(n, _I32) for n in ("xs_enabled", "xs_residual", "xs_min_m", "big_tile", "big_tile_256", "small_tile", "eight_waves", "deep_ring",
                                    "gn_handover", "wide_stream", "gn_fold", "force_bn", "force_waves", "force_stages", "xcd_order")]


class LaunchChoice(C.Structure):    # es_launch_choice
    _fields_ = [(n, _I32) for n in ("route", "bn", "splitk", "stages", "waves", "xcd_m_fastest", "gn_partials", "wide")]


ROUTE_CONV_GEMM, ROUTE_LINEAR_XS = 0, 1
# es_linear_xs_last_form: K / 32 in the low byte, then the template flags of the instantiation that ran
XS_FORM_KC_MASK, XS_FORM_GEGLU, XS_FORM_LN, XS_FORM_RES, XS_FORM_PP, XS_FORM_GN = 0xFF, 0x100, 0x200, 0x400, 0x800, 0x1000
GN_FORM_SLAB, GN_FORM_TWO_LAUNCHES = 1, 2        # ES_GN_FORM_*
GN_ROUTE_FIELDS = ("form", "gpb", "slots", "cpt", "ppb", "nchunk", "ps", "lanes", "blocks", "ipt", "general", "lds")     # ES_GN_ROUTE_*
ATTN_ROUTE_FIELDS = ("kernel", "q_per_wg", "q_per_wave", "grid_x", "grid_y", "grid_z", "threads", "lds", "qper")               # ES_ATTN_ROUTE_*
GEMM_ROUTE_FIELDS = ("kernel", "row", "family", "bn", "stages", "waves", "aligned", "grid", "threads", "lds", "reduce", "reduce_cb",
                     "reduce_grid", "reduce_threads", "runs", "samples_per_run")                                                # ES_GEMM_ROUTE_*
XS_ROUTE_FIELDS = ("form", "grid", "threads", "lds", "runs", "rows_per_run")                                                     # ES_XS_ROUTE_*
GEMM_REDUCE_NONE, GEMM_REDUCE_PLAIN, GEMM_REDUCE_GN = 0, 1, 2                                                                   # ES_GEMM_REDUCE_*
GEMM_ROWS_128, GEMM_ROWS_256 = 33, 6             # rows of the instantiation table: the 128-pixel kernel's, then the 256-pixel kernel's


def gemm_kernel_fields(kid: int) -> dict:
    """es_conv_gemm_last_kernel / the route's kernel id, unpacked (ES_GEMM_KERNEL_*)"""
    return dict(bn=kid & 0x1FF, bm=64 * (kid >> 9 & 7), stages=kid >> 12 & 7, waves=8 if kid & 0x8000 else 4, aligned=bool(kid & 0x10000),
                ln=bool(kid & 0x20000), ko=bool(kid & 0x40000), geglu=bool(kid & 0x80000), bf16=bool(kid & 0x100000))

# every symbol include/edgestyle_hip.h declares: (name, restype, argtypes)
_P, _I, _F, _L = C.c_void_p, C.c_int, C.c_float, C.c_int64
SYMBOLS = {
    "es_abi_version": (C.c_int, []),
    "es_set_operand_limit": (C.c_ulonglong, [C.c_ulonglong]),
    "es_last_error": (C.c_char_p, []),
    "es_sizeof_desc": (C.c_size_t, [_I]),
    "es_conv_gemm": (C.c_int, [C.POINTER(GemmDesc), _P]),
    "es_conv_gemm_workspace_bytes": (C.c_size_t, [C.POINTER(GemmDesc)]),
    "es_linear_xs": (C.c_int, [C.POINTER(XsDesc), _P]),
    "es_linear_xs_set_pp": (C.c_int, [_I]),
    "es_linear_xs_last_form": (C.c_int, []),
    "es_linear_xs_knobs": (None, [C.POINTER(XsKnobs)]),
    "es_linear_xs_route": (C.c_int, [C.POINTER(XsDesc), C.POINTER(XsKnobs), C.POINTER(C.c_int32)]),
    "es_conv_gemm_last_kernel": (C.c_int, []),
    "es_conv_gemm_route": (C.c_int, [C.POINTER(GemmDesc), C.POINTER(C.c_int32)]),
    "es_attention": (C.c_int, [C.POINTER(AttnDesc), _P]),
    "es_attention_set_kvres": (C.c_int, [_I]),
    "es_attention_last_kernel": (C.c_int, []),
    "es_attention_knobs": (None, [C.POINTER(AttnKnobs)]),
    "es_attention_route": (C.c_int, [C.POINTER(AttnDesc), C.POINTER(AttnKnobs), C.POINTER(C.c_int32)]),
    "es_group_norm": (C.c_int, [C.POINTER(GnDesc), _P]),
    "es_group_norm_partials_bytes": (C.c_size_t, [_I, _I]),
    "es_group_norm_is_slab": (C.c_int, [_I, _I, _I]),
    "es_group_norm_chunks": (C.c_int, [_I]),
    "es_group_norm_route": (C.c_int, [C.POINTER(GnDesc), C.POINTER(C.c_int32)]),
    "es_layer_norm_route": (C.c_int, [_I]),
    "es_layer_norm": (C.c_int, [_P, _P, _P, _P, _I, _I, _F, _I, _P]),
    "es_fusion_block": (C.c_int, [C.POINTER(FusionDesc), _P]),
    "es_fusion_scratch_bytes": (C.c_size_t, [_I]),
    "es_fusion_blocks": (C.c_int, [C.POINTER(FusionDesc), _I, _P]),
    "es_timestep_embedding": (C.c_int, [_P, _P, _I, _I, _I, _P]),
    "es_cfg_ddim_step": (C.c_int, [_P, _P, _P, _P, _P, _F, _I, _I, _I, _I, _I, _I, _I, _P]),
    "es_cfg_unipc_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _I, _I, _I, _I, _I, _I, _P]),
    "es_nchw_f32_to_nhwc": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "es_nhwc_to_nchw_f32": (C.c_int, [_P, _P, _I, _I, _I, _I, _F, _F, _I, _I, _P]),
    "es_add": (C.c_int, [_P, _P, _P, _L, _I, _P]),
    "es_vae_sample": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _F, _I, _P]),
    "es_incr": (C.c_int, [_P, _P]),
    "es_clock_probe": (C.c_int, [_P, C.c_uint, _P]),
    "es_gather_row": (C.c_int, [_P, _P, _P, _I, _I, _P]),
    "es_layer_norm_grouped": (C.c_int, [C.POINTER(LnDesc), _P]),
    "es_latents_to_input": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "es_memcpy": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "es_memcpy2d": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P]),
    "es_fill_f32": (C.c_int, [_P, _F, C.c_size_t, _P]),
    "es_plan_create": (_P, []),
    "es_plan_destroy": (None, [_P]),
    "es_plan_begin_record": (C.c_int, [_P]),
    "es_plan_end_record": (C.c_int, [_P]),
    "es_plan_size": (C.c_int, [_P]),
    "es_plan_count": (C.c_int, [_P, _I]),
    "es_plan_launch": (C.c_int, [_P, _P]),
    "es_ctx_create": (C.c_int, [_I, C.POINTER(_P)]),
    "es_ctx_destroy": (None, [_P]),
    "es_ctx_set_geometry": (C.c_int, [_P, C.POINTER(CtxGeometry)]),
    "es_ctx_set_plan": (C.c_int, [_P, _I, _P]),
    "es_ctx_bind": (C.c_int, [_P, _I, _P, C.c_size_t]),
    "es_ctx_buffer": (_P, [_P, _I, C.POINTER(C.c_size_t)]),
    "es_ctx_arena_bytes": (C.c_size_t, [_P]),
    "es_ctx_set_options": (C.c_int, [_P, C.POINTER(C.c_float), _F, _F, _I]),
    "es_ctx_set_scheduler": (C.c_int, [_P, _I]),
    "es_ctx_set_alphas_cumprod_f64": (C.c_int, [_P, C.POINTER(C.c_double), _I]),
    "es_unipc_coef_table": (C.c_int, [C.POINTER(C.c_double), _I, C.POINTER(C.c_float), _I, C.POINTER(C.c_float)]),
    "es_ctx_set_alphas_cumprod": (C.c_int, [_P, C.POINTER(C.c_float), _I]),
    "es_ctx_plan_size": (C.c_int, [_P, _I]),
    "es_ctx_plan": (_P, [_P, _I]),
    "es_ctx_load": (C.c_int, [C.c_char_p, _I, C.POINTER(_P)]),
    "es_ctx_save": (C.c_int, [_P, C.c_char_p]),
    "es_ctx_save_ranges": (C.c_int, [_P, C.c_char_p, C.POINTER(MemRange), _I, C.POINTER(MemRange), _I, C.POINTER(CtxImageInfo)]),
    "es_plan_export": (C.c_size_t, [_P, _P, C.c_size_t]),
    "es_plan_import": (_P, [_P, C.c_size_t]),
    "es_plan_pointer_fields": (C.c_int, [_I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, C.POINTER(C.c_int32)]),
    "es_ctx_launch_plan": (C.c_int, [_P, _I, C.POINTER(C.c_float), _P]),
    "es_ddim_coef_table": (C.c_int, [C.POINTER(C.c_float), _I, C.POINTER(C.c_float), _I, C.POINTER(C.c_float)]),
    "es_denoise_step": (C.c_int, [_P, _P, _F, _P, C.POINTER(_P), C.POINTER(C.c_float), _P, _P]),
    "es_denoise_loop": (C.c_int, [_P, _P, _P, _F, C.POINTER(C.c_float), _I, _P]),
    "es_vae_decode": (C.c_int, [_P, _P, _P, _P]),
    "es_prepare_conds": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), _P]),
    "es_load_weights": (C.c_int, [C.POINTER(Weights), C.POINTER(ModelConfig), C.POINTER(CtxGeometry), _I, C.POINTER(_P)]),
    "es_plan_gemm_choice": (C.c_int, [C.c_longlong, _I, _I, _I, C.POINTER(C.c_int), _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int)]),
    "es_linear_xs_eligible": (C.c_int, [C.c_longlong, _I, _I, _I, _I, _I, _I]),
    "es_launch_choose": (C.c_int, [C.POINTER(LaunchQuery), C.POINTER(LaunchKnobs), C.POINTER(LaunchChoice)]),
    "es_launch_route": (C.c_int, [C.POINTER(LaunchQuery), C.POINTER(LaunchKnobs)]),
    "es_launch_gn_fold": (C.c_int, [C.POINTER(LaunchQuery), _I, C.POINTER(LaunchKnobs)]),
    "es_launch_gn_handover": (C.c_int, [C.c_longlong, _I, _I, C.POINTER(LaunchKnobs)]),
    "es_launch_wide_stream": (C.c_int, [_I, C.POINTER(LaunchKnobs)]),
    "es_launch_default_knobs": (None, [C.POINTER(LaunchKnobs)]),
    "es_launch_xs_slices": (C.c_int, [C.c_longlong, _I, _I, _I, _I, C.POINTER(_I32), C.POINTER(_I32)]),
    "es_conv_gemm8p_form_ok": (C.c_int, [_I, _I, _I, C.c_longlong, _I]),
    "es_ctx_graph_hazard": (C.c_int, []),
    "es_plan_set_dry": (C.c_int, [_I]),
    "es_image_fit": (C.c_int, [_I, _I, _I, C.POINTER(C.c_int32)]),
    "es_image_resize_coeffs": (C.c_int, [_I, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I]),
    "es_image_resize_workspace_bytes": (C.c_size_t, [C.POINTER(ImageU8), _I, _I]),
    "es_image_resize_u8": (C.c_int, [C.POINTER(ImageU8), _I, _P, _I, _P, C.c_size_t, _P]),
    "es_image_u8_to_f32": (C.c_int, [_P, _P, _I, _I, _I, _I, _P]),
    "es_image_f32_to_u8": (C.c_int, [_P, _P, _I, _I, _I, _P]),
    "es_prepare_conds_u8": (C.c_int, [_P, C.POINTER(ImageU8), C.POINTER(C.c_int32), C.POINTER(_P), _P, C.c_size_t, _P]),
    "es_vae_decode_u8": (C.c_int, [_P, _P, _P, _P]),
    "es_philox4x32_10": (C.c_int, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "es_philox_block_cap": (C.c_int, [_I]),
    "es_philox_blocks": (C.c_int, [_L, _I]),
    "es_philox_advance": (_L, [_L, _I]),
    "es_randn": (C.c_int, [_P, C.POINTER(RandnDesc), _P]),
    "es_randn_host": (C.c_int, [_P, C.POINTER(RandnDesc)]),
    "es_ctx_draw_latents": (C.c_int, [_P, C.POINTER(Philox), _I, _F, _I, _P, _P]),
    "es_ctx_draw_cond_noise": (C.c_int, [_P, C.POINTER(Philox), _I, _P]),
    "es_attention_causal": (C.c_int, [C.POINTER(AttnDesc), _P]),
    "es_text_embed": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "es_text_encoder_create": (C.c_int, [C.POINTER(StateDict), C.POINTER(TextConfig), _I, _I, _I, C.POINTER(_P)]),
    "es_text_encoder_destroy": (None, [_P]),
    "es_text_encoder_arena_bytes": (C.c_size_t, [_P]),
    "es_text_encode": (C.c_int, [_P, _P, _I, _P, _P]),
    "es_image_fit_ex": (C.c_int, [_I, _I, _I, _I, C.POINTER(C.c_int32)]),
    "es_image_resize_coeffs_ex": (C.c_int, [_I, _I, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I]),
    "es_image_resize_workspace_bytes_ex": (C.c_size_t, [C.POINTER(ImageU8), _I, _I, _I, _I]),
    "es_image_resize_u8_ex": (C.c_int, [C.POINTER(ImageU8), _I, _P, _I, _I, _I, _P, C.c_size_t, _P]),
    "es_clip_patchify": (C.c_int, [_P, _P, _P, _I, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _I, _P]),
    "es_clip_embed": (C.c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _I, _P]),
    "es_clip_score": (C.c_int, [_P, _I, _P, _I, _I, _I, _F, C.POINTER(C.c_int32), _I, _I, _P, _P, _P, _P]),
    "es_clip_bank_create": (C.c_int, [C.POINTER(StateDict), _I, _I, _I, _I, _I, _I, C.POINTER(_P)]),
    "es_clip_bank_destroy": (None, [_P]),
    "es_clip_bank_rows": (C.c_int, [_P]),
    "es_clip_bank_data": (_P, [_P]),
    "es_clip_bank_append": (C.c_int, [_P, _P, _I, _P]),
    "es_clip_text_pool": (C.c_int, [_P, _P, C.POINTER(C.c_int32), _I, _I, _P]),
    "es_clip_vision_create": (C.c_int, [C.POINTER(StateDict), C.POINTER(ClipVisionConfig), _I, _I, _I, C.POINTER(_P)]),
    "es_clip_vision_destroy": (None, [_P]),
    "es_clip_vision_arena_bytes": (C.c_size_t, [_P]),
    "es_clip_vision_encode": (C.c_int, [_P, _P, _I, _P, _P]),
    "es_clip_pick_workspace_bytes": (C.c_size_t, [_P, C.POINTER(ImageU8), _I]),
    "es_clip_pick": (C.c_int, [_P, _P, C.POINTER(ImageU8), _I, _F, C.POINTER(C.c_int32), _I, _I, _P, _P, _P, _P, C.c_size_t, _P]),
    "es_text_encode_dev": (C.c_int, [_P, _P, _I, _P, _P]),
    "es_tokenizer_create": (C.c_int, [C.c_char_p, C.c_char_p, _I, C.POINTER(_P)]),
    "es_tokenizer_create_from_memory": (C.c_int, [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, _I, C.POINTER(_P)]),
    "es_tokenizer_destroy": (None, [_P]),
    "es_tokenizer_vocab_size": (C.c_int, [_P]),
    "es_tokenizer_max_length": (C.c_int, [_P]),
    "es_tokenizer_bos_id": (C.c_int, [_P]),
    "es_tokenizer_eos_id": (C.c_int, [_P]),
    "es_tokenizer_pad_id": (C.c_int, [_P]),
    "es_tokenize": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32), _I]),
    "es_tokenize_padded": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "es_prompt_table_create": (C.c_int, [_P, C.POINTER(C.c_char_p), _I, C.POINTER(C.c_int32), _I, C.c_char_p, C.c_char_p, C.c_char_p, _I,
                                         C.POINTER(_P)]),
    "es_prompt_table_destroy": (None, [_P]),
    "es_prompt_assemble": (C.c_int, [_P, _P, _I, _I, _P, _P, _P]),
    "es_prompt_assemble_host": (C.c_int, [_P, C.POINTER(C.c_int32), _I, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "es_mask_workspace_bytes": (C.c_size_t, [_I, _I, _I]),
    "es_mask_morph": (C.c_int, [_P, _P, _I, _I, _I, C.POINTER(C.c_int32), _I, _P, C.c_size_t, _P]),
    "es_mask_largest_component": (C.c_int, [_P, _P, _P, _I, _I, _I, _P, C.c_size_t, _P]),
    "es_mask_logic": (C.c_int, [_P, _P, _P, _L, _I, _P]),
    "es_image_mask_fill_u8": (C.c_int, [C.POINTER(ImageU8), _P, _P, _I, _I, _I, C.POINTER(C.c_uint8), _P]),
    "es_sam_compose": (C.c_int, [C.POINTER(ImageU8), _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, C.c_size_t, _P]),
    "es_dwconv": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "es_relu_linear_attention": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "es_sam_neck_merge": (C.c_int, [C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _P, _I, _I, _I, _P]),
    "es_sam_resize_shape": (None, [_I, _I, _I, C.POINTER(C.c_int32)]),
    "es_sam_preprocess_u8_workspace_bytes": (C.c_size_t, [C.POINTER(ImageU8), _I, _I]),
    "es_sam_preprocess_u8": (C.c_int, [C.POINTER(ImageU8), _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _I, _P, _P, _P, C.POINTER(C.c_int32), _P,
                                       C.c_size_t, _P]),
    "es_sam_encoder_create": (C.c_int, [C.POINTER(StateDict), C.POINTER(SamConfig), _I, _I, _I, C.POINTER(_P)]),
    "es_sam_encoder_destroy": (None, [_P]),
    "es_sam_encoder_arena_bytes": (C.c_size_t, [_P]),
    "es_sam_encode": (C.c_int, [_P, _P, _I, _P, _P]),
    "es_sam_encoder_stage": (C.c_int, [_P, _I, _I, _P, _P]),
    "es_sam_encode_u8_workspace_bytes": (C.c_size_t, [_P, C.POINTER(ImageU8), _I]),
    "es_sam_encode_u8": (C.c_int, [_P, C.POINTER(ImageU8), _I, _P, C.POINTER(C.c_int32), _P, C.c_size_t, _P]),
    "es_sam_prompt_token_count": (C.c_int, [_I, _I]),
    "es_sam_prompt_tokens": (C.c_int, [C.POINTER(SamPromptDesc), _P]),
    "es_sam_prompt_tokens_host": (C.c_int, [C.POINTER(SamPromptDesc), _P]),
    "es_linear_tokens": (C.c_int, [C.POINTER(LinearTokensDesc), _P]),
    "es_sam_upscale_pack": (C.c_int, [_P, _I, _I, _P]),
    "es_sam_upscale_masks": (C.c_int, [C.POINTER(SamUpscaleDesc), _P]),
    "es_sam_decoder_create": (C.c_int, [C.POINTER(StateDict), C.POINTER(SamDecoderConfig), _I, _I, _I, _I, C.POINTER(_P)]),
    "es_sam_decoder_destroy": (None, [_P]),
    "es_sam_decoder_arena_bytes": (C.c_size_t, [_P]),
    "es_sam_decode": (C.c_int, [_P, _P, C.POINTER(SamPrompts), _I, _I, _P, _P, _P]),
    "es_sam_predict": (C.c_int, [_P, _P, C.POINTER(SamPrompts), _I, _I, _P, _P, _P, _P, _P]),
    "es_sam_postprocess_masks": (C.c_int, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "es_sam_postprocess_masks_host": (C.c_int, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "es_mask_bbox": (C.c_int, [_P, _P, _I, _I, _I, _I, _P]),
    "es_mask_bbox_host": (C.c_int, [_P, _P, _I, _I, _I, _I]),
    "es_person_crop_fit": (C.c_int, [_I, _I, C.POINTER(C.c_double), _I, _I, C.c_double, C.POINTER(C.c_int32)]),
    "es_image_resize_window_u8_workspace_bytes": (C.c_size_t, [C.POINTER(ImageU8), _I, C.POINTER(C.c_int32), _I, _I, _I]),
    "es_image_resize_window_u8": (C.c_int, [C.POINTER(ImageU8), _I, C.POINTER(C.c_int32), _P, _I, _I, _I, _P, C.c_size_t, _P]),
    "es_person_crop_u8_workspace_bytes": (C.c_size_t, [C.POINTER(ImageU8), _I, C.POINTER(C.c_double)]),
    "es_person_crop_u8": (C.c_int, [C.POINTER(ImageU8), _I, C.POINTER(C.c_double), _P, _P, C.c_size_t, _P]),
    "es_pose_draw": (C.c_int, [_P, _P, _I, _I, _I, _P]),
    "es_pose_draw_host": (C.c_int, [_P, _P, _I, _I, _I]),
    "es_pose_select_host": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), _I]),
    "es_pose_points_host": (C.c_int, [_P, _I, _I, _P]),
    "es_jpeg_info_host": (C.c_int, [_P, C.c_size_t, C.POINTER(JpegInfo)]),
    "es_jpeg_coeff_count": (C.c_size_t, [C.POINTER(JpegInfo)]),
    "es_jpeg_entropy_decode_host": (C.c_int, [_P, C.c_size_t, C.POINTER(JpegInfo), _P, _P]),
    "es_jpeg_reconstruct_workspace_bytes": (C.c_size_t, [C.POINTER(JpegInfo), _I]),
    "es_jpeg_reconstruct": (C.c_int, [C.POINTER(JpegInfo), _I, C.POINTER(_P), C.POINTER(_P), C.POINTER(ImageU8), _P, C.c_size_t, _P]),
    "es_jpeg_reconstruct_host": (C.c_int, [C.POINTER(JpegInfo), _I, C.POINTER(_P), C.POINTER(_P), C.POINTER(ImageU8)]),
    "es_jpeg_decode_staging_bytes": (C.c_size_t, [C.POINTER(JpegInfo), _I]),
    "es_jpeg_decode_u8": (C.c_int, [C.POINTER(_P), C.POINTER(C.c_size_t), _I, C.POINTER(ImageU8), _P, _P, C.c_size_t, _P, C.c_size_t, _P]),
    "es_jpeg_segment_count": (C.c_size_t, [C.POINTER(JpegInfo)]),
    "es_jpeg_scan_prepare_host": (C.c_int, [_P, C.c_size_t, C.POINTER(JpegInfo), _P, _P, _P]),
    "es_jpeg_entropy_decode_workspace_bytes": (C.c_size_t, [C.POINTER(JpegInfo), _I]),
    "es_jpeg_entropy_decode": (C.c_int, [C.POINTER(JpegInfo), _I, C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(_P), C.POINTER(_P), _I,
                                         C.POINTER(_P), _P, _P, C.c_size_t, _P]),
    "es_jpeg_entropy_decode_parallel_host": (C.c_int, [C.POINTER(JpegInfo), _I, C.POINTER(_P), C.POINTER(C.c_size_t), C.POINTER(_P), C.POINTER(_P), _I, _I,
                                                       C.POINTER(_P), _P, C.POINTER(C.c_int32)]),
    "es_jpeg_status_text": (C.c_char_p, [_I]),
    "es_jpeg_decode_dev_staging_bytes": (C.c_size_t, [C.POINTER(JpegInfo), C.POINTER(C.c_size_t), _I, C.POINTER(C.c_size_t)]),
    "es_jpeg_decode_dev_u8": (C.c_int, [C.POINTER(_P), C.POINTER(C.c_size_t), _I, C.POINTER(ImageU8), _I, _P, _P, C.c_size_t, _P, C.c_size_t, _P,
                                        C.c_size_t, _P]),
    "es_jpeg_encode_info_host": (C.c_int, [_I, _I, _I, C.POINTER(JpegEncodeParams), C.POINTER(JpegInfo)]),
    "es_jpeg_header_host": (C.c_int, [C.POINTER(JpegInfo), C.POINTER(JpegEncodeParams), _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "es_jpeg_encode_capacity": (C.c_size_t, [C.POINTER(JpegInfo), C.POINTER(JpegEncodeParams)]),
    "es_jpeg_encode_workspace_bytes": (C.c_size_t, [C.POINTER(JpegInfo), _I, C.POINTER(JpegEncodeParams)]),
    "es_jpeg_forward": (C.c_int, [C.POINTER(ImageU8), _I, C.POINTER(JpegEncodeParams), C.POINTER(_P), _P, C.c_size_t, _P]),
    "es_jpeg_forward_host": (C.c_int, [C.POINTER(ImageU8), _I, C.POINTER(JpegEncodeParams), C.POINTER(_P)]),
    "es_jpeg_entropy_encode": (C.c_int, [C.POINTER(JpegInfo), _I, C.POINTER(JpegEncodeParams), C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_size_t), _P, _P,
                                         C.c_size_t, _P]),
    "es_jpeg_entropy_encode_host": (C.c_int, [C.POINTER(JpegInfo), _I, C.POINTER(JpegEncodeParams), C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_size_t), _P]),
    "es_jpeg_encode_u8": (C.c_int, [C.POINTER(ImageU8), _I, C.POINTER(JpegEncodeParams), C.POINTER(_P), C.POINTER(C.c_size_t), _P, _P, C.c_size_t, _P]),
    "es_jpeg_encode_host": (C.c_int, [C.POINTER(ImageU8), _I, C.POINTER(JpegEncodeParams), C.POINTER(_P), C.POINTER(C.c_size_t), _P]),
}

_lib = None


FUSION_MAX_BATCH = 13     # ES_FUSION_MAX_BATCH


class EdgeStyleHipError(RuntimeError):
    pass


def load():
    """Load the HIP library (once).  Raises EdgeStyleHipError — never falls back to another implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EdgeStyleHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)           # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.es_abi_version() != ABI_VERSION:
        raise EdgeStyleHipError("libedgestyle_hip.so ABI version mismatch")
    for i, st in enumerate((GemmDesc, AttnDesc, GnDesc, FusionDesc, LnDesc, XsDesc)):
        if lib.es_sizeof_desc(i) != C.sizeof(st):
            raise EdgeStyleHipError(f"descriptor layout mismatch for {st.__name__}: C {lib.es_sizeof_desc(i)} "
                                    f"vs ctypes {C.sizeof(st)}")
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().es_last_error()
        raise EdgeStyleHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def group_norm_route(N: int, HW: int, C1: int, C2: int, groups: int, stats_only: bool = False, ext_chunks: int = 0) -> dict:
    """es_group_norm_route as a dict keyed by GN_ROUTE_FIELDS (raises where es_group_norm would refuse the geometry)"""
    d = GnDesc()
    d.N, d.HW, d.C1, d.C2, d.groups, d.stats_only, d.ext_chunks = N, HW, C1, C2, groups, 1 if stats_only else 0, ext_chunks
    out = (C.c_int32 * len(GN_ROUTE_FIELDS))()
    check(load().es_group_norm_route(C.byref(d), out), "es_group_norm_route")
    return dict(zip(GN_ROUTE_FIELDS, out))


def gemm_route(desc: GemmDesc) -> dict:
    """es_conv_gemm_route as a dict keyed by GEMM_ROUTE_FIELDS (raises where es_conv_gemm would refuse the descriptor; its pointers
    count as present or absent only)"""
    out = (C.c_int32 * len(GEMM_ROUTE_FIELDS))()
    check(load().es_conv_gemm_route(C.byref(desc), out), "es_conv_gemm_route")
    return dict(zip(GEMM_ROUTE_FIELDS, out))


def xs_route(desc: XsDesc, knobs: "XsKnobs | None" = None) -> dict:
    """es_linear_xs_route as a dict keyed by XS_ROUTE_FIELDS (raises where es_linear_xs would refuse the descriptor).  knobs None: the
    process's own (ES_XS_PP and es_linear_xs_set_pp)."""
    out = (C.c_int32 * len(XS_ROUTE_FIELDS))()
    check(load().es_linear_xs_route(C.byref(desc), None if knobs is None else C.byref(knobs), out), "es_linear_xs_route")
    return dict(zip(XS_ROUTE_FIELDS, out))


def attention_route(N: int, heads: int, Sq: int, Skv: int, d: int, *, dtype: int = ES_F16, knobs: "AttnKnobs | None" = None, ld=None) -> dict:
    """es_attention_route as a dict keyed by ATTN_ROUTE_FIELDS (raises where es_attention would refuse the geometry).  knobs None: the
    process's own (environment and es_attention_set_kvres).  ld None: dense rows of heads * d elements, else the row stride of q | k | v | o."""
    a = AttnDesc()
    a.N, a.heads, a.Sq, a.Skv, a.d, a.dtype = N, heads, Sq, Skv, d, dtype
    a.ldq = a.ldk = a.ldv = a.ldo = heads * d if ld is None else ld
    out = (C.c_int32 * len(ATTN_ROUTE_FIELDS))()
    check(load().es_attention_route(C.byref(a), None if knobs is None else C.byref(knobs), out), "es_attention_route")
    return dict(zip(ATTN_ROUTE_FIELDS, out))

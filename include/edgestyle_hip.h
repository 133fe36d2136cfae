/*
 * edgestyle_hip.h — C ABI of libedgestyle_hip.so: the MI355X (gfx950) kernels behind EdgeStyle's
 * multi-ControlNet SD1.5 denoising hot path.
 *
 * The reference (andrei-ace/EdgeStyle) has no FFI: every FLOP of this path is a PyTorch/cuDNN op launched by
 * diffusers modules.  Each entry point below names the reference/diffusers op it replaces so a
 * maintainer can bind it (ctypes stub shown in INTEGRATION.md).  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (a torch tensor's data_ptr()); it must outlive the
 *     stream operation; nothing is allocated, freed or synchronised inside (hipGraph-capture safe);
 *   - activations are NHWC ([N,H,W,C], C contiguous) in `dtype` (ES_F16 / ES_BF16); accumulation is fp32;
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous w.r.t. it;
 *   - return 0 on success, <0 on error (es_last_error() gives the text); never throws across the boundary.
 */
#ifndef EDGESTYLE_HIP_H
#define EDGESTYLE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { ES_F16 = 0, ES_BF16 = 1, ES_F32 = 2 /* es_tensor sources only: the kernels compute in ES_F16 / ES_BF16 */ };
enum { ES_ACT_NONE = 0, ES_ACT_SILU = 1, ES_ACT_GEGLU = 2,
       ES_ACT_GELU_TANH = 3 /* nn.GELU(approximate="tanh"); es_conv_gemm on the 64- / 128- / 160-wide tiles and the split-K reduce only:
                               es_conv_gemm8p_form_ok and es_linear_xs refuse it, so the launch policy never routes it to them, and a
                               LayerNorm-folded launch (ln_colsum) with it is refused */ };

/* 7 (round 5): es_gemm_desc.bn = 256; es_xs_desc.gn_* and es_gn_desc.stats_only (both structs grew: GroupNorm in front of a row-stationary
 * projection); es_conv_gemm8p_form_ok, es_ctx_graph_hazard, es_linear_xs_set_pp, es_attention_set_kvres, es_set_operand_limit,
 * es_group_norm_chunks, es_clock_probe.  Context images carry the version and are rebuilt across it.
 * (Host-only helpers that no plan or image records - es_plan_gemm_choice, es_linear_xs_eligible, es_linear_xs_last_form, es_launch_choose and its siblings
 * es_launch_route / es_launch_gn_fold / es_launch_gn_handover / es_launch_wide_stream / es_launch_default_knobs / es_launch_xs_slices,
 * es_attention_route, es_attention_knobs,
 * es_conv_gemm_route, es_conv_gemm_last_kernel, es_linear_xs_route, es_linear_xs_knobs - come and go without a new version.) */
#define ES_ABI_VERSION 7
int es_abi_version(void);
/* sizeof the descriptor structs as compiled (0 gemm, 1 attn, 2 gn, 3 fusion, 4 ln, 5 xs): lets a binding verify its mirror */
size_t es_sizeof_desc(int which);
const char* es_last_error(void);

/* ---------------------------------------------------------------------------------------------------------
 * es_conv_gemm — implicit-GEMM convolution / linear on MFMA (16x16x32 f16|bf16, fp32 accumulate).
 * Replaces: torch conv2d 3x3 s1/s2 + 1x1 and nn.Linear as invoked by diffusers ResnetBlock2D.conv1/conv2,
 * conv_shortcut, Downsample2D, Upsample2D (nearest-2x fused into the loader), Transformer2DModel.proj_in/out,
 * Attention.to_q/k/v/to_out, GEGLU/FeedForward, TimestepEmbedding, ControlNet zero-convs
 * (model/controllora.py:197-254) and the skip-concat `torch.cat([h, res], 1)` of the UNet up blocks (x2).
 *   out[m, co] = act( sum_k A[m,k] * W[co,k] + bias[co] + temb[n(m), co] ) * out_scale (+ residual[m, co])
 * with m = (n, oy, ox), k = (ky, kx, c) tap-major over the channel-concatenated sources (x | x2).
 * W is pre-packed (ops.pack_weight / es_load_weights): [rows_padded][Kpad] K-contiguous, dtype; K order: `korder`.
 * --------------------------------------------------------------------------------------------------------- */
typedef struct {
  const void* x;          /* [N, Hsrc, Wsrc, C1] */
  const void* x2;         /* optional second source [N, Hsrc, Wsrc, C2] (channel concat), or NULL */
  const void* w;          /* packed weights [rows_padded][Kpad] */
  const float* bias;      /* [rows_padded] fp32 or NULL */
  const void* temb;       /* optional per-sample per-channel add, dtype, [N, temb_stride] (already offset) */
  const void* residual;   /* optional [M, Cout_store] dtype, added after act*scale */
  const float* out_scale_dev; /* optional device scalar multiplied into the result (conditioning_scale) */
  void* out;              /* [N, Hout, Wout, Cout_store] dtype */
  float* workspace;       /* split-K partials [splitk][M][rows_padded] fp32 (NULL if splitk == 1) */
  unsigned long long* prof; /* optional device u64[2]: every workgroup atomically mins its start / maxes its end
                               s_memrealtime stamp (100 MHz) -> launch duration as executed inside a hipGraph */
  int32_t N, Hsrc, Wsrc, C1, C2;
  int32_t Hout, Wout, Cout;   /* Cout = true GEMM N (before GEGLU halving) */
  int32_t rows_padded, Kpad;  /* packed weight geometry */
  int32_t ksize, stride, pad; /* ksize 1|3 ; input coord = o*stride + k - pad */
  int32_t upsample;           /* 1: sources are nearest-2x upsampled on the fly (Hin = 2*Hsrc) */
  int32_t temb_stride;
  int32_t act;                /* ES_ACT_* ; GEGLU halves the stored width (weights packed interleaved) */
  int32_t splitk;
  int32_t bn;                 /* N tile: 128 | 160 (128-pixel tile), 64 (64 x 64 tile, tiny launches), 320 (256 x 320 phase-interleaved
                               * tile, csrc/gemm_conv8p.hip: large launches with 64-aligned channels), 256 (its 256 x 256 form: the
                               * LayerNorm-folded / GEGLU linear layers, ln_colsum / ES_ACT_GEGLU allowed, no temb); rows_padded % bn == 0 */
  int32_t dtype;
  /* Grouped launch: ngroups (<= 4) problems of identical geometry but different weights run as ONE launch over the
   * batch-concatenated activations (the 3 batched ControlNet passes + the UNet encoder of a denoising step): M tiles
   * [mt_end[g-1], mt_end[g]) (units of 128 pixels) use w_g[g] / bias_g[g].  ngroups <= 1: plain launch (w, bias). */
  int32_t ngroups;
  int32_t mt_end[4];
  const void* w_g[4];
  const float* bias_g[4];
  int32_t stages;             /* LDS ring depth: 0 = auto, 2 (2 workgroups/CU), 3 or 4 (1 workgroup/CU) */
  int32_t xcd_m_fastest;      /* tile order inside an XCD's chunk: 1 = tile_m fastest (weights are the larger operand) */
  int32_t waves;              /* waves per 128-pixel workgroup: 0 / 4 = default, 8 = two per SIMD (launches that leave
                               * a workgroup alone on its CU: one wave per SIMD cannot overlap DMA issue, LDS reads and
                               * MFMAs with itself) */
  float out_scale;
  /* LayerNorm folded into a linear layer (the three LayerNorms of a BasicTransformerBlock feed exactly one Linear
   * each): x is the RAW residual stream, w holds W * gamma (per input channel), bias holds W beta + b, and
   * ln_colsum[j] = sum_k w[j][k] (fp32, of the rounded packed weights).  The kernel accumulates every row's sum and
   * sum of squares from the activation tiles it stages anyway and applies
   *   out[m][j] = rstd_m * (acc[m][j] - mean_m * ln_colsum[j]) + bias[j]
   * in the epilogue.  Needs ksize 1, one source, K == C1 (a multiple of 64), splitk 1, bn 64|128|160. */
  const float* ln_colsum;     /* NULL: plain launch */
  const float* ln_colsum_g[4];
  float ln_eps;
  /* 1x1 tail sources (ResnetBlock2D: conv2(h) + conv_shortcut(x) as ONE launch): after the ksize*ksize taps over
   * (x | x2) the K axis continues with ONE centre tap over the channel concat (t1 | t2), tensors of the OUTPUT's
   * spatial size [N, Hout, Wout, Ct1|Ct2]; the packed weights are [W_conv | W_shortcut] along K, the bias is the sum.
   * Needs stride 1, no upsample, 64-aligned C1, C2, Ct1, Ct2.  t1 == NULL: no tail. */
  const void* t1;
  const void* t2;
  int32_t Ct1, Ct2;
  /* source batch modulo: sample n of the launch reads source sample n % x_nmod of x (x then holds x_nmod samples): the
   * same tensor feeds several groups of a grouped launch (conv_in of all ControlNets + the UNet on ONE sample tensor,
   * CL:197-203; text states shared by the nets of a weight-sharing group) without a replicated copy.  0 = off.
   * Needs one source (no x2), no tail sources. */
  int32_t x_nmod;
  /* K order of the packed weights (and of the loader): 0 = tap-major, k = (ky, kx, c) over the channel concat;
   * 1 = chunk-major, k = (c / 64, ky, kx, c % 64): the nine taps of one 64-channel chunk back to back, so that eight of
   * the nine activation tiles a workgroup stages per chunk re-read lines it fetched one K-tile earlier (L2 hits instead
   * of Infinity-Cache round trips: with tap-major order the 32 workgroups of an XCD sweep 5-10 MB of activations between
   * two reads of the same line).  The 1x1 tail sources follow the k*k*Ctot main part in either order.
   * 1 needs ksize 3 and 64-aligned C1, C2; ops.pack_weight / es_load_weights pack every such convolution this way. */
  int32_t korder;
  /* WIDE RESIDUAL STREAM (bf16 pipelines, BASELINE configs[4]): the tensors every ResnetBlock / transformer block adds into
   * travel as TWO tensors of the compute dtype, hi + lo with hi = round(x), lo = round(x - hi) - 16 significant bits in bf16.
   * MFMA operands, GroupNorm and everything else read `hi` (the ordinary tensor); only the residual add sees both:
   *   sum = round(act(...) * scale) + residual + residual_lo   (fp32);   out = round(sum);   out_lo = round(sum - out)
   * so the rounding of the stream's sums no longer accumulates from block to block (it was 5 dB of the bf16 error budget:
   * profiles/r04_bf16_error_budget_2steps.txt).  out_lo needs `residual` and an output width that is a multiple of 8;
   * residual_lo needs out_lo.  Both NULL: the single-tensor stream of every fp16 pipeline. */
  const void* residual_lo;
  void* out_lo;
  /* GroupNorm statistics handed over by the producer: the epilogue (fused or split-K reduce) also writes, for every 64-pixel block
   * of its output and every GroupNorm group, the block's sum and sum of squares - fp32 [N][2 * HW/64][gn_groups][2]: entry
   * 2 * block + 0 holds the part of a group inside the N tile the group STARTS in, entry 2 * block + 1 the part inside the next
   * N tile (zero when the group ends in its first tile) - summed in ONE fixed order whatever tile, wave count or split-K the launch
   * uses (64 pixels as 8 sequential sub-blocks of 8, then the group's channels in order).  es_group_norm with
   * es_gn_desc.ext_chunks = 2 * HW/64 then normalises in a single pass: no statistics launch, no second read.  Needs the
   * output's H*W % 64 == 0, Cout % 8 == 0 and Cout / gn_groups <= the N tile.  NULL: no statistics. */
  float* gn_part;
  int32_t gn_groups;
} es_gemm_desc;
int es_conv_gemm(const es_gemm_desc* d, void* stream);
/* The kernels address each activation operand (sources, tail sources, output) through 32-bit buffer offsets: 2 GiB.  A launch whose
 * operands are larger is run by es_conv_gemm / es_linear_xs as several launches over runs of whole samples (per weight group, then as
 * many samples as fit), each with its operand pointers moved to its first sample - the tiles of a launch never interact, so the results
 * do not depend on the cuts.  Test knob: lower the limit so that small launches are cut (0 restores 2 GiB); returns the previous value. */
unsigned long long es_set_operand_limit(unsigned long long bytes);
size_t es_conv_gemm_workspace_bytes(const es_gemm_desc* d);
/* test query: the kernel instantiation the last es_conv_gemm launch of this process went to (of a launch cut into runs: the last run's),
 * packed from the template arguments the launcher instantiates, never from the route or the descriptor; 0 before the first launch, and a
 * dry recording call leaves it alone.  Bits 0-8: couts per workgroup (64 | 128 | 160 | 256 | 320), the rest as below. */
enum { ES_GEMM_KERNEL_BN_MASK = 0x1FF,
       ES_GEMM_KERNEL_BM64_SHIFT = 9, ES_GEMM_KERNEL_BM64_MASK = 0x7,        /* pixels per workgroup / 64: 1 | 2, 4 = the phase-interleaved kernel */
       ES_GEMM_KERNEL_STAGES_SHIFT = 12, ES_GEMM_KERNEL_STAGES_MASK = 0x7,   /* LDS ring depth 2 | 3 | 4 */
       ES_GEMM_KERNEL_WAVES8 = 0x8000,     /* 8 waves per workgroup (else 4) */
       ES_GEMM_KERNEL_ALIGNED = 0x10000,   /* channels in whole 64-deep K-steps */
       ES_GEMM_KERNEL_LN = 0x20000,        /* LayerNorm folded in */
       ES_GEMM_KERNEL_KO = 0x40000,        /* chunk-major K order */
       ES_GEMM_KERNEL_GEGLU = 0x80000,     /* phase-interleaved kernel: the GEGLU epilogue's own instantiation */
       ES_GEMM_KERNEL_BF16 = 0x100000 };
int es_conv_gemm_last_kernel(void);
/* host-only query (tests, tools): the launch es_conv_gemm would make for this descriptor.  Pointer fields are read as present or absent
 * only, so NULL x / w / out are fine and no GPU is needed; -1 with the text es_conv_gemm would refuse the descriptor with. */
enum { ES_GEMM_REDUCE_NONE = 0, ES_GEMM_REDUCE_PLAIN = 1, ES_GEMM_REDUCE_GN = 2 };
enum {
  ES_GEMM_ROUTE_KERNEL = 0,          /* the id es_conv_gemm_last_kernel reports after the launch */
  ES_GEMM_ROUTE_ROW = 1,             /* row of the library's instantiation table (the 33 of the 128-pixel kernel, then the 6 of the 256-pixel one) */
  ES_GEMM_ROUTE_FAMILY = 2,          /* 0: the 128- (64-) pixel kernel, 1: the phase-interleaved 256-pixel kernel */
  ES_GEMM_ROUTE_BN = 3,              /* couts per workgroup as they run: a recorded 320 | 256 whose epilogue form the big tile lacks runs on 160 | 128 */
  ES_GEMM_ROUTE_STAGES = 4,          /* ... LDS ring depth (0 = auto is 2) */
  ES_GEMM_ROUTE_WAVES = 5,
  ES_GEMM_ROUTE_ALIGNED = 6,         /* C1 and C1 + C2 multiples of 64 */
  ES_GEMM_ROUTE_GRID = 7,
  ES_GEMM_ROUTE_THREADS = 8,
  ES_GEMM_ROUTE_LDS = 9,             /* dynamic LDS bytes */
  ES_GEMM_ROUTE_REDUCE = 10,         /* split-K: ES_GEMM_REDUCE_* */
  ES_GEMM_ROUTE_REDUCE_CB = 11,      /* ... GroupNorm hand-over: channels per workgroup (64 | 80 | 128), else 0 */
  ES_GEMM_ROUTE_REDUCE_GRID = 12,
  ES_GEMM_ROUTE_REDUCE_THREADS = 13,
  ES_GEMM_ROUTE_RUNS = 14,           /* launches the call is cut into (operands beyond the 32-bit buffer offsets), else 1 */
  ES_GEMM_ROUTE_SAMPLES_PER_RUN = 15,/* ... samples per full run; grid and reduce grid are then the first run's */
  ES_GEMM_ROUTE_FIELDS = 16
};
int es_conv_gemm_route(const es_gemm_desc* d, int32_t out[ES_GEMM_ROUTE_FIELDS]);

/* ---------------------------------------------------------------------------------------------------------
 * es_linear_xs — row-stationary short-K linear layer (K = 320 | 640): out = epilogue(LayerNorm?(x) W^T + bias).
 * Replaces, at the 64x64 and 32x32 UNet / ControlNet levels: BasicTransformerBlock.norm1 -> attn1.to_q|k|v and
 * norm3 -> ff.net.0 (GEGLU) (diffusers, called under model/controllora.py:205-238) - the same math as es_conv_gemm with
 * ln_colsum / ES_ACT_GEGLU, organised for few K-steps and many output columns (csrc/linear_xs.hip).
 * x [M, K] dtype, raw residual stream when ln != 0 (gamma / beta are folded into w / bias: ops.pack_weight_ln);
 * w packed [rows_padded][K] (GEGLU: rows interleaved 16 hidden | 16 gate, as for es_conv_gemm); bias fp32
 * [rows_padded] (required); out [M, ldo] dtype, Cout (or Cout / 2 for GEGLU) columns written.
 * Workgroup = 256 rows x one slice of the output columns: grid = ceil(M / 256) * nslices, slice s covers the
 * `chunks_per_slice` column chunks (64 columns at K = 320, 32 at K = 640) starting at s * chunks_per_slice.
 * Grouped launch like es_conv_gemm: rows [mt_end[g-1], mt_end[g]) * 128 use w_g[g] / bias_g[g] (even mt_end only; the last,
 * ceil(M / 128), may be odd: a ragged last run).
 * --------------------------------------------------------------------------------------------------------- */
typedef struct {
  const void* x; void* out;
  const void* w; const float* bias;
  const void* w_g[4]; const float* bias_g[4];
  unsigned long long* prof;   /* as es_gemm_desc.prof */
  int32_t mt_end[4];
  int32_t ngroups;
  int32_t M, K, Cout, rows_padded;
  int32_t ldo;                /* output row pitch in elements */
  int32_t geglu, ln;
  float ln_eps;
  int32_t nslices, chunks_per_slice;
  int32_t dtype;
  /* optional: out = x W^T + bias + residual - rows of ldo elements, like out (Attention.to_out + residual, BasicTransformerBlock).
   * K = 320 only, no GEGLU, no LayerNorm fold */
  const void* residual;
  /* optional: GroupNorm in front (Transformer2DModel.norm -> proj_in: eps 1e-6, no activation).  x is then the RAW tensor [N, gn_hw, K];
   * gn_part holds the sums of x and x^2 per (sample, pixel chunk, GroupNorm group) - fp32 [N][gn_nchunk][gn_groups][2], as
   * es_group_norm(stats_only = 1) writes them (gn_nchunk = es_group_norm_chunks(gn_hw)) - and gn_gamma / gn_beta (gn_gamma_g / gn_beta_g
   * per weight group of a grouped launch) the affine parameters, fp32 [K].  The kernel normalises the rows it holds in registers:
   * one read of x instead of three passes over it.  Needs the plain projection (no GEGLU, LayerNorm fold or residual), gn_hw % 256 == 0,
   * M == N * gn_hw, at most 32 groups.  gn_part == NULL: off. */
  const float* gn_part;
  const float* gn_gamma; const float* gn_beta;
  const float* gn_gamma_g[4]; const float* gn_beta_g[4];
  int32_t gn_groups, gn_nchunk, gn_hw;
  float gn_eps;
} es_xs_desc;
int es_linear_xs(const es_xs_desc* d, void* stream);
/* tool / test knob: the form of the plain (no GEGLU) launches - 1 = two-barrier ping-pong between the wave groups (default; ES_XS_PP=0
 * in the environment, read on first use, turns it off), 0 = the one-barrier form.  Bit-identical outputs.  Returns the previous setting. */
int es_linear_xs_set_pp(int on);
typedef struct { int32_t pp; } es_xs_knobs;
void es_linear_xs_knobs(es_xs_knobs* out);        /* host-only: a copy of the process's knobs */
/* host-only query (tests, tools): the launch es_linear_xs would make for this descriptor under these knobs (NULL: the process's).  Pointer
 * fields are read as present or absent only, and no GPU is needed; -1 with the text es_linear_xs would refuse the descriptor with. */
enum {
  ES_XS_ROUTE_FORM = 0,              /* the id es_linear_xs_last_form reports after the launch (ES_XS_FORM_*) */
  ES_XS_ROUTE_GRID = 1,
  ES_XS_ROUTE_THREADS = 2,
  ES_XS_ROUTE_LDS = 3,               /* dynamic LDS bytes */
  ES_XS_ROUTE_RUNS = 4,              /* launches the call is cut into (operands beyond the 32-bit buffer offsets), else 1 */
  ES_XS_ROUTE_ROWS_PER_RUN = 5,      /* ... rows per full run; the grid is then the first run's */
  ES_XS_ROUTE_FIELDS = 6
};
int es_linear_xs_route(const es_xs_desc* d, const es_xs_knobs* knobs, int32_t out[ES_XS_ROUTE_FIELDS]);
/* test query: the kernel instantiation the last es_linear_xs launch of this process went to (of a launch cut into runs: the last run's) -
 * K / 32 (10 | 20) in the low byte, or'ed with the flags below; 0 before the first launch.  Set by the launcher from the template arguments
 * it instantiates, not recomputed from the descriptor.  (Host-only, recorded by no plan or image: no new ES_ABI_VERSION.) */
enum { ES_XS_FORM_KC_MASK = 0xFF, ES_XS_FORM_GEGLU = 0x100, ES_XS_FORM_LN = 0x200, ES_XS_FORM_RES = 0x400, ES_XS_FORM_PP = 0x800,
       ES_XS_FORM_GN = 0x1000 };
int es_linear_xs_last_form(void);

/* Fused attention softmax(Q K^T * scale) V (flash-style, online softmax, MFMA).
 * Replaces torch.nn.functional.scaled_dot_product_attention under diffusers Attention (attn1/attn2/VAE attn).
 * Q [N,Sq,ldq], K [N,Skv,ldk], V [N,Skv,ldv], O [N,Sq,ldo]; head h lives at column h*d of every row. */
typedef struct {
  const void* q; const void* k; const void* v; void* o;
  int32_t N, heads, Sq, Skv, d;
  int32_t ldq, ldk, ldv, ldo;         /* row strides in elements */
  int64_t bsq, bsk, bsv, bso;         /* batch strides in elements */
  float scale;
  int32_t dtype;
} es_attn_desc;
int es_attention(const es_attn_desc* d, void* stream);
/* tool / test knob: launches with Skv <= 96 and head_dim 40 | 80 (the text-token cross-attention of the two shallow UNet levels) on the
 * K/V-resident kernel - 0 never, 1 (default; ES_ATTN_KVRES in the environment) where it wins (>= 12 samples at head_dim 40, >= 64 at 80:
 * profiles/r05_xattn_bench.txt), 2 every eligible launch.  Returns the previous setting.  It edits `kvres` of the process's knobs below. */
int es_attention_set_kvres(int on);
/* test query: the kernel the last es_attention launch of this process went to - 1 generic tile, 2 generic tile with 32 queries per wave at
 * head_dim 40 | 48 | 80 in large launches (1 also names the widths that ALWAYS run 32 per wave - 8-32, 64, 128, 160: ES_ATTN_ROUTE_Q_PER_WAVE
 * states the geometry), 3 32x32 score tile, 4 32x32 score tile with two query blocks per wave, 5 | 6 head_dim-40 ping-pong kernel with
 * 32 | 64 queries per wave, 7 K/V-resident; 0 before the first launch.  Set by the launcher from the template arguments it instantiates. */
int es_attention_last_kernel(void);
/* The switches that bend the choice of kernel (tools, tests).  The process's own are read from the environment once, on first use - the
 * first launch, route query or es_attention_set_kvres (ES_ATTN_KVRES too: earlier versions read that one when the library was loaded). */
typedef struct {
  int64_t big_thr;   /* ES_ATTN_BIG, 512: blocks of 128 (256) queries from which a launch runs 32 (64) queries per wave */
  int32_t kvres;     /* ES_ATTN_KVRES, 1: see es_attention_set_kvres */
  int32_t attn32;    /* ES_ATTN32, 1: 0 = no 32x32 score tile (nor what builds on it: 4 - 6), 2 = also for head_dim 80 */
  int32_t qb;        /* ES_ATTN_QB, 2: 1 = never two query blocks per wave (kernel 4) */
  int32_t pp;        /* ES_ATTN_PP, -1: ping-pong kernel 0 = off, 1 | 2 = 32 | 64 queries per wave, -1 = 32 from 256 blocks of 256 queries on */
} es_attn_knobs;
void es_attention_knobs(es_attn_knobs* out);      /* host-only: a copy of the process's knobs */
/* host-only query (tests, tools): the launch es_attention would make for this descriptor (N, heads, Sq, Skv, d and the row strides are read;
 * no pointer is, and NULL pointers are accepted), computed by the launcher's own code: es_attention switches on this kernel id and launches
 * with this grid, block, LDS size and strip length.  knobs NULL: the process's own; else used as given.  0, or -1 with es_last_error()
 * where es_attention would refuse the geometry (same texts). */
enum {
  ES_ATTN_ROUTE_KERNEL = 0,      /* the ids of es_attention_last_kernel */
  ES_ATTN_ROUTE_Q_PER_WG = 1,    /* queries a workgroup covers (K/V-resident: its strip, = ES_ATTN_ROUTE_QPER) */
  ES_ATTN_ROUTE_Q_PER_WAVE = 2,  /* queries a wave holds at a time: 16 | 32 | 64 (K/V-resident: the 32-query blocks it walks its strip in) */
  ES_ATTN_ROUTE_GRID_X = 3,
  ES_ATTN_ROUTE_GRID_Y = 4,
  ES_ATTN_ROUTE_GRID_Z = 5,
  ES_ATTN_ROUTE_THREADS = 6,     /* threads per workgroup */
  ES_ATTN_ROUTE_LDS = 7,         /* dynamic LDS bytes */
  ES_ATTN_ROUTE_QPER = 8,        /* K/V-resident kernel: queries per strip; 0 otherwise */
  ES_ATTN_ROUTE_FIELDS = 9
};
int es_attention_route(const es_attn_desc* d, const es_attn_knobs* knobs, int32_t out[ES_ATTN_ROUTE_FIELDS]);

/* GroupNorm (+SiLU) over NHWC with optional channel-concat of two sources.
 * Replaces torch group_norm + silu of ResnetBlock2D.norm1/norm2, conv_norm_out, Transformer2DModel.norm.
 * partials: fp32 scratch of es_group_norm_partials_bytes(N, groups) bytes = [N][64][groups][2] floats.  The statistics pass cuts a sample into
 * chunks of max(16, ceil(HW / 64)) pixels and writes the first es_group_norm_chunks(HW) = ceil(HW / that) <= 64 rows of every sample, densely
 * ([N][nchunk][groups][2]); the one-launch slab form leaves the buffer untouched.
 * Refused: C > 8192, groups > 64, and a two-launch geometry with C + groups > 8064 (its scale / shift tables would pass 64 KB of LDS). */
typedef struct {
  const void* x; const void* x2; void* out;
  const float* gamma; const float* beta; float* partials;
  int32_t N, HW, C1, C2, groups;
  float eps;
  int32_t silu, dtype;
  /* grouped launch: samples [n_end[g-1], n_end[g]) use gamma_g[g] / beta_g[g] (ngroups <= 1: gamma, beta) */
  int32_t ngroups;
  int32_t n_end[4];
  const float* gamma_g[4];
  const float* beta_g[4];
  /* > 0: `partials` already HOLDS the statistics of x as ext_chunks partial sums per (sample, group) - written by the producing
   * es_conv_gemm launch (es_gemm_desc.gn_part, ext_chunks = 2 * HW/64): no statistics pass, one read of x.  One source only. */
  int32_t ext_chunks;
  /* 1: the statistics pass alone - `partials` receives the sums of x and x^2 per (sample, pixel chunk, group), fp32
   * [N][es_group_norm_chunks(HW)][groups][2]; nothing is normalised, out / gamma / beta are not read.  The consumer applies the
   * normalisation itself (es_xs_desc.gn_part: Transformer2DModel.norm -> proj_in as one read of x). */
  int32_t stats_only;
} es_gn_desc;
int es_group_norm(const es_gn_desc* d, void* stream);
size_t es_group_norm_partials_bytes(int N, int groups);
int es_group_norm_chunks(int HW);                       /* pixel chunks per sample of the statistics pass */
int es_group_norm_is_slab(int HW, int C, int groups);   /* 1: this geometry runs as ONE launch (slab form) */
/* host-only query (tests, tools): the launch es_group_norm would make for this descriptor (N, HW, C1, C2, groups, ext_chunks, stats_only are
 * read; no pointer is), computed by the launcher's own code.  0, or -1 with es_last_error() where es_group_norm would refuse the geometry.
 * Fields that do not apply to the form are 0. */
enum {
  ES_GN_ROUTE_FORM = 0,          /* ES_GN_FORM_SLAB | ES_GN_FORM_TWO_LAUNCHES */
  ES_GN_ROUTE_GPB = 1,           /* slab: groups per workgroup (1 | 2 | 4) */
  ES_GN_ROUTE_SLOTS = 2,         /* slab: pixel slots (pixels in flight per workgroup) */
  ES_GN_ROUTE_CPT = 3,           /* slab: register class, pixels per thread 8 | 16 | 24 */
  ES_GN_ROUTE_PPB = 4,           /* statistics pass: pixels per chunk */
  ES_GN_ROUTE_NCHUNK = 5,        /* ... chunks per sample = rows of `partials` written (ext_chunks where the producer wrote them) */
  ES_GN_ROUTE_PS = 6,            /* ... pixel slots */
  ES_GN_ROUTE_LANES = 7,         /* ... lanes that fold one group (8, or 4 for more than 32 groups) */
  ES_GN_ROUTE_BLOCKS = 8,        /* apply pass: workgroups per sample (0: stats_only) */
  ES_GN_ROUTE_IPT = 9,           /* ... items per thread the grid was sized for (4 | 8 | 16) */
  ES_GN_ROUTE_GENERAL = 10,      /* ... 1: the general loop (an index division per item), 0: the fixed-column loop */
  ES_GN_ROUTE_LDS = 11,          /* dynamic LDS bytes of the (last) launch */
  ES_GN_ROUTE_FIELDS = 12
};
enum { ES_GN_FORM_SLAB = 1, ES_GN_FORM_TWO_LAUNCHES = 2 };
int es_group_norm_route(const es_gn_desc* d, int32_t out[ES_GN_ROUTE_FIELDS]);

/* LayerNorm over the last dim of [M, C] (BasicTransformerBlock.norm1/2/3), eps 1e-5. */
int es_layer_norm(const void* x, void* out, const float* gamma, const float* beta, int M, int C, float eps,
                  int dtype, void* stream);
/* grouped LayerNorm: rows [row_end[g-1], row_end[g]) use gamma_g[g] / beta_g[g] */
typedef struct {
  const void* x; void* out;
  const float* gamma_g[4]; const float* beta_g[4];
  int32_t row_end[4];
  int32_t ngroups, M, C;
  float eps;
  int32_t dtype;
} es_ln_desc;
int es_layer_norm_grouped(const es_ln_desc* d, void* stream);
/* host-only query: 16-byte chunks per lane of the kernel instantiation that holds a row of C channels - 1 | 2 | 3 | 4 | 8 (C <= 512 | 1024 |
 * 1536 | 2048 | 4096); 0 where es_layer_norm refuses C (not a multiple of 8, or above 4096). */
int es_layer_norm_route(int C);

/* EdgeStyle fusion block: interleave (model/edgestyle_multicontrolnet.py:479-501) + ControlNetBlock
 * (model/edgestyle_multicontrolnet.py:23-63) without materialising the interleaved tensor.
 * res[i]: residual of net i, [N, HW, C] dtype (batch stride res_bs[i] elements so nets batched together can be
 * addressed in place).  Params are repacked pixel-major: w1[C][3][2], b1[C][3], g1/be1[HW][C][3] (dtype),
 * w2[C][3], b2[C], g2/be2[HW][C] (dtype), w3[C], b3[C] (fp32 unless noted).
 * scratch: fp32 [N][2][nchunk<=256][2] partial sums; u: dtype [N,HW,C] intermediate; out: [N,HW,C] dtype. */
typedef struct {
  const void* res[6];
  int64_t res_bs[6];
  const float* w1; const float* b1; const void* g1; const void* be1;
  const float* w2; const float* b2; const void* g2; const void* be2;
  const float* w3; const float* b3;
  float* scratch; void* u; void* out;
  const float* res_scale_dev;  /* optional device float[6]: per-net conditioning_scale (CL:266-270), graph-updatable */
  const void* addend;          /* optional [N,HW,C] dtype: the UNet skip / mid tensor this residual is added to
                                * (PL:500-510): out = round(block) + addend, rounded like the separate add */
  float res_scale[6];          /* per-net conditioning_scale applied to res[i] on load (multiplied with the above) */
  int32_t N, HW, C;
  float eps;
  int32_t dtype;
} es_fusion_desc;
int es_fusion_block(const es_fusion_desc* d, void* stream);
size_t es_fusion_scratch_bytes(int N);
/* All fusion blocks of one denoising step (MC:103-114, 160-169: 12 down + 1 mid) in three launches instead of 3 per
 * block: same arithmetic per block as es_fusion_block; every block needs its own scratch and u buffer; all share N and
 * dtype. */
#define ES_FUSION_MAX_BATCH 13
int es_fusion_blocks(const es_fusion_desc* descs, int count, void* stream);

/* Sinusoidal timestep features (diffusers Timesteps(dim, flip_sin_to_cos=True, freq_shift=0); CL:150-155):
 * out[n, :] = [cos(t_n f_i) | sin(t_n f_i)], dtype.  t: fp32 [N] device. */
int es_timestep_embedding(const float* t, void* out, int N, int dim, int dtype, void* stream);

/* CFG combine + DDIM(eta=0) step (model/edgestyle_pipeline.py:513-522):
 *   eps = e_u + g (e_c - e_u);  x0 = (x - sqrt(1-a_t) eps)/sqrt(a_t);  x <- sqrt(a_prev) x0 + sqrt(1-a_prev) eps
 * noise: [2B or B, HW, L] dtype NHWC (uncond first); latents fp32 [B,HW,L] in/out; model_in: dtype [2B or B,HW,Lstride]
 * rewritten for the next step (CFG duplicate, PL:443-447).  coef: device fp32 table [steps][4] =
 * {sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev)}, row selected by *step_idx (device int32). */
int es_cfg_ddim_step(const void* noise, float* latents, void* model_in, const float* coef, const int32_t* step_idx,
                     float guidance_scale, int B, int HW, int L, int Lstride, int cfg, int nsteps, int dtype,
                     void* stream);   /* *step_idx is clamped to [0, nsteps) */

/* CFG combine + one UniPCMultistepScheduler step (the scheduler the reference's callers swap in, TT:273 / APP:118):
 * bh2, solver_order <= 2, predict_x0, epsilon prediction.  The corrector/predictor updates are linear in
 * {last_sample, m0, m1, x0}; coef: device fp32 [steps][12] = {alpha_t, sigma_t, use_corrector, c_last, c_m0, c_m1,
 * c_x0, p_x, p_x0, p_m0, 0, 0} computed on the host (edgestyle_amd/schedulers.py).  last_sample/m0/m1: fp32 state
 * [B,HW,L], zero before the first step. */
int es_cfg_unipc_step(const void* noise, float* latents, float* last_sample, float* m0, float* m1, void* model_in,
                      const float* coef, const int32_t* step_idx, float guidance_scale, int B, int HW, int L,
                      int Lstride, int cfg, int nsteps, int dtype, void* stream);

/* Layout / dtype conversion at the drop-in boundary (callers hand NCHW fp32, TT:328-359). */
int es_nchw_f32_to_nhwc(const float* in, void* out, int N, int C, int HW, int Cpad, int dtype, void* stream);
int es_nhwc_to_nchw_f32(const void* in, float* out, int N, int C, int HW, int Cstride, float scale, float shift,
                        int clamp01, int dtype, void* stream);
/* y = a + b (elementwise, dtype), n elements (n % 8 == 0) */
int es_add(const void* a, const void* b, void* y, int64_t n, int dtype, void* stream);
/* DiagonalGaussianDistribution.sample()*scaling_factor (CL:39-40): moments [N,HW,2L] -> z [N,HW,Lpad] */
int es_vae_sample(const void* moments, const float* noise_nchw, void* z, int N, int HW, int L, int Lpad,
                  float scaling, int dtype, void* stream);
/* dst (int32 device) += 1  — advances the step counter inside a captured graph */
int es_incr(int32_t* ctr, void* stream);
/* Measurement tool (tools/clock_in_kernel.py; no reference counterpart): ONE wave on `stream` watches the shader-cycle counter against the
 * 100 MHz real-time counter for duration_us and writes {shader cycles, 100 MHz ticks} to out2 (device u64[2]) - launched on a side
 * stream it reports the clock the chip holds while the work on the other streams runs.  Not free: a resident wave keeps a workgroup of
 * the one-per-CU kernels (256 x 320 tile, linear_xs) off its CU, so a launch of exactly 256 such workgroups takes two rounds beside it -
 * which is why bench.py samples rocm-smi instead (same reading).  Never part of a plan. */
int es_clock_probe(unsigned long long* out2, unsigned int duration_us, void* stream);
/* out[0..row_len) = table[clamp(*idx, 0, nrows-1)][0..row_len) — selects this step's timestep / conditioning-scale row inside a
 * captured graph (PL:435, PL:464-470) so a replay needs no host-side scalar update */
int es_gather_row(const float* table, const int32_t* idx, float* out, int row_len, int nrows, void* stream);

/* DiagonalGaussian / scheduler glue used by the native loop: latents fp32 [B,HW,L] -> the networks' input (dtype,
 * channels zero-padded to Lstride, duplicated for CFG; PL:443-447) */
int es_latents_to_input(const float* latents, void* model_in, int B, int HW, int L, int Lstride, int cfg, int dtype,
                        void* stream);
/* device-to-device copy / strided copy / fp32 fill on `stream`, as C-ABI calls so that they are part of a recorded plan */
int es_memcpy(void* dst, const void* src, size_t bytes, void* stream);
int es_memcpy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, void* stream);
int es_fill_f32(float* dst, float value, size_t n, void* stream);

/* =========================================================================================================
 * Step-level ABI: a denoising step, the denoising loop and the VAE decode behind plain device pointers.
 *
 * es_plan — a recorded launch list.  Between es_plan_begin_record and es_plan_end_record every C-ABI call made on the
 * calling thread is appended to the plan (and still executed / stream-captured as usual); es_plan_launch re-issues the
 * list on any stream.  The pointers inside are the ones recorded: the builder keeps those buffers alive.
 * es_ctx  — owns up to ES_PLAN_COUNT plans plus the static device buffers they read and write (bound by slot), and
 * runs them: as hipGraphs instantiated from the launch lists (default) or launch by launch.
 * The reference has no FFI; what these entry points replace is Python:
 *   es_denoise_step  == OnnxUNetAndControlnets.forward                 export_onnx.py:43-74
 *   es_denoise_loop  == the loop of EdgeStyleStableDiffusionControlNetPipeline.__call__   model/edgestyle_pipeline.py:435-543
 *   es_vae_decode    == vae.decode(latents / scaling_factor) + postprocess               model/edgestyle_pipeline.py:552-572
 *   es_prepare_conds == prepare_image + CachedControlNetModel.preprocess_image            model/edgestyle_pipeline.py:629-664, controllora.py:289-290
 * A context is BUILT either by es_load_weights below (natively, from raw state-dict tensors) or by a host that walks the model
 * itself (edgestyle_amd/native.py NativeEngine: packs the weights, allocates the static buffers, records the plans); after that
 * no interpreter is involved in these calls.
 * ========================================================================================================= */
typedef struct es_plan es_plan;
typedef struct es_ctx es_ctx;
es_plan* es_plan_create(void);
void es_plan_destroy(es_plan* p);
int es_plan_begin_record(es_plan* p);
int es_plan_end_record(es_plan* p);
int es_plan_size(const es_plan* p);                    /* number of recorded calls */
int es_plan_count(const es_plan* p, int kind);         /* ... of one kind (csrc/plan.h: 1 = es_conv_gemm, 2 = es_linear_xs, ...) */
int es_plan_launch(const es_plan* p, void* stream);
/* flat image of a plan: returns the bytes needed; writes them when cap suffices.  The recorded device addresses inside
 * are NOT relocated (es_ctx_save_ranges builds the relocation tables es_ctx_load applies) */
size_t es_plan_export(const es_plan* p, void* out, size_t cap);
/* The pointer fields of a recorded call, by op kind (csrc/plan.h es_op_kind): byte offsets inside the argument record and how
 * the op uses the memory behind each (1 = reads, 2 = writes, 3 = both); *elem_bytes != 0: the record is an array of elements
 * of that size (es_fusion_blocks).  Returns the field count and fills at most `cap` entries.  This is what relocates a plan:
 * exactly these words are device addresses (es_ctx_save_ranges), nothing is guessed from bit patterns. */
int es_plan_pointer_fields(int kind, int32_t* offsets, int32_t* uses, int cap, int32_t* elem_bytes);
es_plan* es_plan_import(const void* data, size_t size);

enum { ES_PLAN_STEP_GENERIC = 0,   /* es_denoise_step: text K/V projections + condition slots + time embedding + step */
       ES_PLAN_PREP = 1,           /* es_denoise_loop, once: text K/V projections, condition slots, time-projection table */
       ES_PLAN_STEP = 2,           /* es_denoise_loop, per step: table-driven step + CFG + scheduler + counter */
       ES_PLAN_DECODE = 3,         /* es_vae_decode */
       ES_PLAN_CONDS = 4,          /* es_prepare_conds: RGB condition images -> the condition embeddings in ES_BUF_COND* */
       ES_PLAN_STEP_UNET = 5,      /* es_denoise_loop, per step OUTSIDE the control-guidance window (PL:419-427: every controlnet_keep is 0): the
                                    * UNet alone plus the constant residuals the fusion blocks return for zero inputs - the six ControlNet passes
                                    * and the fusion launches are skipped, not multiplied by zero.  Optional: without it such a step runs
                                    * ES_PLAN_STEP with scale 0, like the reference. */
       ES_PLAN_COUNT = 6 };
enum { ES_BUF_SAMPLE = 0,          /* dtype [N,h,w,latent_pad]: the networks' input (both CFG halves) */
       ES_BUF_T_ROWS, ES_BUF_EHS,  /* fp32 [kmax*N] timestep copies; dtype [N,77,D] text states */
       ES_BUF_COND0, ES_BUF_COND1, ES_BUF_COND2, ES_BUF_COND3, ES_BUF_COND4, ES_BUF_COND5,   /* dtype [N,h,w,C0] each */
       ES_BUF_SCALES,              /* fp32 [n_conds] conditioning scales of the current step */
       ES_BUF_NOISE,               /* dtype [N,h,w,out_channels] noise prediction */
       ES_BUF_LATENTS,             /* fp32 [B,h,w,L] */
       ES_BUF_STEP_IDX,            /* int32 device step counter */
       ES_BUF_T_TABLE, ES_BUF_SCALE_TABLE, ES_BUF_COEF, ES_BUF_TIMESTEPS,   /* fp32 [T,kmax*N], [T,n_conds], [T,4], [T] */
       ES_BUF_IMAGE,               /* fp32 [B,3,8h,8w] NCHW decoded image in [0,1] */
       /* es_prepare_conds inputs: the RGB condition image of net i, fp32 NCHW [B,3,8h,8w] (VAE-conditioned nets: in [-1,1],
        * pose nets: in [0,1], as the reference's callers pass them, TT:29-48), and - VAE-conditioned nets only - the
        * latent_dist.sample() noise of CL:39 for the CFG-duplicated batch, fp32 [N,latent_channels,h,w] */
       ES_BUF_COND_IMG0, ES_BUF_COND_IMG1, ES_BUF_COND_IMG2, ES_BUF_COND_IMG3, ES_BUF_COND_IMG4, ES_BUF_COND_IMG5,
       ES_BUF_COND_NOISE0, ES_BUF_COND_NOISE1, ES_BUF_COND_NOISE2, ES_BUF_COND_NOISE3, ES_BUF_COND_NOISE4, ES_BUF_COND_NOISE5,
       ES_BUF_HIST0, ES_BUF_HIST1, ES_BUF_HIST2,   /* UniPC multistep state: last_sample, m0, m1 - fp32 [B,h,w,L] each (es_ctx_set_scheduler) */
       ES_BUF_COUNT };
enum { ES_SCHED_DDIM = 0, ES_SCHED_UNIPC = 1 };
typedef struct {
  int32_t B, cfg;                  /* images per call; 1 = classifier-free guidance (N = 2B) */
  int32_t h, w;                    /* latent size */
  int32_t latent_channels, latent_pad;
  int32_t n_conds;                 /* 6 (the fused multi-ControlNet) or 1 (a single ControlNet) */
  int32_t n_steps;                 /* the ES_PLAN_PREP time table is built for this many steps */
  int32_t dtype;
  int32_t guess_mode;              /* 1: the recorded step is guess_mode's (CL:256-264, PL:453-459, 487-497): per-net chains with log-spaced
                                    * level scales; under CFG the ControlNets see the conditional half only - the condition slots then hold
                                    * B samples - and the fused residuals are added to that half */
} es_ctx_geometry;
int es_ctx_create(int device, es_ctx** out);
void es_ctx_destroy(es_ctx* c);                         /* destroys its plans too */
int es_ctx_set_geometry(es_ctx* c, const es_ctx_geometry* g);
int es_ctx_set_plan(es_ctx* c, int which, es_plan* p);  /* the context takes ownership of the plan */
int es_ctx_bind(es_ctx* c, int slot, void* dev, size_t bytes);
void* es_ctx_buffer(const es_ctx* c, int slot, size_t* bytes);
size_t es_ctx_arena_bytes(const es_ctx* c);   /* size of the context's own arena (es_load_weights / es_ctx_load; a dry build reports what it would be) */   /* the memory bound to a slot (borrowed; NULL if unbound) */
/* cond_scales: float[6] or NULL (keep); control guidance window (PL:419-427); use_graphs: 0 = re-issue launch by launch,
 * 1 = one hipGraph per plan (es_denoise_loop launches the step graph n times), 2 = additionally the preparation and all n
 * steps of es_denoise_loop as ONE graph (instantiated on first use per (n_steps, guidance scale)) */
int es_ctx_set_options(es_ctx* c, const float* cond_scales, float control_guidance_start, float control_guidance_end,
                       int use_graphs);
int es_ctx_set_alphas_cumprod(es_ctx* c, const float* alphas_cumprod, int n);   /* scheduler schedule (default: SD1.5's) */
/* The update es_denoise_loop applies after each step's noise prediction: ES_SCHED_DDIM (eta 0; the BASELINE metric's scheduler,
 * model/edgestyle_pipeline.py:520-522 with the pipeline's default) or ES_SCHED_UNIPC - UniPCMultistepScheduler with the SD1.5
 * scheduler config, bh2, order 2, the scheduler the reference's callers assign (test_text2image_pretrained_openpose.py:273,
 * app.py:118); its timesteps come from the caller like DDIM's (UniPC spaces them over n + 1 intervals: 951, 901, ... for 20
 * steps).  The recorded step list is the same: the context re-issues its scheduler call as es_cfg_unipc_step on the
 * ES_BUF_HIST* slots with a n_steps x 12 coefficient table in ES_BUF_COEF (contexts of es_load_weights and NativeEngine bind both). */
int es_ctx_set_scheduler(es_ctx* c, int scheduler);
/* UniPC works from a double-precision schedule like the Python scheduler (default: SD1.5's scaled_linear betas, derived in double;
 * the fp32 table of es_ctx_set_alphas_cumprod is the DDIM update's) */
int es_ctx_set_alphas_cumprod_f64(es_ctx* c, const double* alphas_cumprod, int n);
/* host-only: out[n][12], the UniPC coefficient rows of a timestep list (alphas_cumprod NULL = SD1.5's schedule, in double) */
int es_unipc_coef_table(const double* alphas_cumprod, int n_alphas, const float* timesteps, int n, float* out);
int es_ctx_plan_size(const es_ctx* c, int which);
es_plan* es_ctx_plan(es_ctx* c, int which);             /* borrowed */
/* Load a context image written by es_ctx_save / es_ctx_save_ranges: packed weights, tables, static buffers, the launch lists
 * and their pointer relocations.  No Python, torch or model code is needed to load or run it: build once (es_load_weights or
 * a Python host), ship the image, start in under a second. */
int es_ctx_load(const char* path, int device, es_ctx** out);
/* Write a context that owns its arena - one built by es_load_weights, or loaded by es_ctx_load - as such an image (same format):
 * build from checkpoints once (seconds), start from the image afterwards (one hipMalloc + copies).  It is es_ctx_save_ranges
 * with the arena as the one segment.  Contexts of a Python host hold pointers into the host's allocator pools instead of one
 * arena: those go through es_ctx_save_ranges. */
int es_ctx_save(const es_ctx* c, const char* path);
typedef struct { uint64_t addr, bytes; } es_mem_range;
typedef struct {
  uint64_t arena_bytes, data_bytes;       /* size of the arena es_ctx_load will allocate; bytes of it stored in the file */
  int32_t segments, extents;              /* used segments (= arena slots); data extents */
  int32_t relocations[ES_PLAN_COUNT];     /* non-null pointer fields per plan */
} es_ctx_image_info;
/* Write ANY launchable context as a context image; the one writer of the format.
 * segments: the allocator segments the context's pointers may fall into (any order; overlapping ones are refused).
 * blocks:   the allocator's blocks inside them, or NULL.
 * Every non-null pointer field of every recorded call (es_plan_pointer_fields; nothing else in a record is read as an address)
 * and every bound slot must lie in a segment: otherwise an error naming the op kind and the address.  The image's arena gets
 * one slot per USED segment, in address order, each rounded up to 256 bytes, and every such pointer becomes an offset into it
 * (the stored launch lists hold offsets too: no absolute address is written).  What travels as bytes: with `blocks`, every
 * referenced block that no call writes (the OR of the uses of all pointers into it lacks 2; a bound slot counts as written,
 * the host entry points fill it) and every referenced block of at most 64 KiB; without, the context's own recorded extents
 * (es_load_weights / es_ctx_load).  All else is zero-filled space.  The file is written as `path`.tmp and renamed on success.
 * path NULL: lay the image out and fill *info (may be NULL) only - no file, no HIP call. */
int es_ctx_save_ranges(const es_ctx* c, const char* path, const es_mem_range* segments, int n_segments,
                       const es_mem_range* blocks, int n_blocks, es_ctx_image_info* info);
/* ---------------------------------------------------------------------------------------------------------
 * es_load_weights - build a context from the reference's state dicts, natively.
 * Replaces, on the loading side: EdgeStyleMultiControlNetModel.from_pretrained + load_state_dict
 * (model/edgestyle_multicontrolnet.py:173-211, 289-430), ControlLoRAModel.tie_weights / load_state_dict / fuse
 * (model/controllora.py:600-632, 728-777) and the module construction of the diffusers UNet / ControlNet / AutoencoderKL
 * the reference instantiates (test_text2image_pretrained_openpose.py:224-261): everything between "tensors of a
 * checkpoint in host memory" and "a context es_denoise_loop can run".
 * Tensors are described, not copied: `key` is the state-dict key exactly as the reference's checkpoints spell it
 * (diffusers UNet2DConditionModel / ControlNetModel / AutoencoderKL names; `<linear>.lora_layer.{down,up}.weight` and
 * `controlnet_down_blocks.*` / `controlnet_mid_block.*` for a ControlLoRA net, CL:600-606; `multi_controlnet_down_blocks.{i}.*`
 * / `multi_controlnet_mid_block.*` for the fusion blocks, MC:173-193), `data` a pointer (host memory, or device memory of
 * `device`: read back first) to a C-contiguous tensor of `dtype` (ES_F32 / ES_F16 / ES_BF16) that stays valid during the call;
 * nothing is kept: the caller keeps ownership.  A safetensors file maps onto this directly.
 * The builder folds W + B.A into private copies (the UNet's tensors are never modified), folds every LayerNorm into the Linear
 * it feeds, ff.net.2 into proj_out and conv_shortcut behind conv2, packs everything into the kernels' layouts, lays out ONE
 * device arena (weights, static buffers, activations with lifetime-based reuse, split-K workspace), records the five launch
 * lists and binds the slots.  A missing key or a tensor of the wrong shape is an error naming the key.
 * Scope: the reference's configurations - six condition slots over 1..3 distinct ControlNets + the UNet through the fusion blocks
 * (TT:252-258), or n_conds = 1: ONE ControlNet whose 13 residuals go to the UNet directly (PL:338-351; `fusion` is not read) -
 * with 64-aligned channel widths; DDIM or UniPC (es_ctx_set_scheduler).  device -1: dry build - everything but the device allocation and the upload (plans keep
 * arena-relative addresses; for inspection with es_ctx_plan / es_plan_export on a host without a GPU); device -2: the same
 * with the arena in host memory, contents included (what tests read the packed weights from).  Neither can launch: every entry point that would
 * run one of their plans returns an error that says so.
 * --------------------------------------------------------------------------------------------------------- */
typedef struct {
  const char* key;
  const void* data;                /* host (or device) memory, C-contiguous; borrowed for the duration of the call */
  int64_t shape[4];
  int32_t ndim;                    /* 1..4 */
  int32_t dtype;                   /* ES_F32 | ES_F16 | ES_BF16 */
} es_tensor;
typedef struct { const es_tensor* tensors; int32_t count; } es_state_dict;
enum { ES_NET_CONTROLNET = 0,        /* ControlNetModel: its own encoder + conv-stack conditioning embedding (the openpose net, TT:247-250) */
       ES_NET_CONTROL_LORA_VAE = 1,  /* ControlLoRAModel(uses_vae): LoRA + zero-convs, encoder tied to the UNet, conditioned through the VAE (CL:28-42) */
       ES_NET_CONTROL_LORA = 2 };    /* ControlLoRAModel with its own conv-stack conditioning embedding */
typedef struct {
  es_state_dict unet, vae, fusion;
  es_state_dict controlnet[6];     /* the distinct nets */
  int32_t controlnet_kind[6];      /* ES_NET_* */
  int32_t n_controlnets;
  int32_t net_of_cond[6];          /* which net serves condition slot i (TT:252-258: {0, 1, 2, 1, 2, 1}); n_conds entries are read */
} es_weights;
typedef struct {                   /* config.json of the SD1.5 checkpoints (README.md:131-135; MC:73-102 hard-codes their consequences) */
  int32_t in_channels, out_channels;
  int32_t n_blocks, block_out_channels[4], down_has_attn[4];
  int32_t layers_per_block, num_heads, cross_attention_dim, norm_num_groups;
  float norm_eps;
  int32_t n_cond_embed, cond_embed_channels[4], conditioning_channels;
  int32_t text_tokens;             /* 77 */
  int32_t vae_n_blocks, vae_block_out_channels[4], vae_layers_per_block, vae_latent_channels, vae_norm_num_groups;
  float vae_norm_eps, vae_scaling_factor;
} es_model_config;
/* g: B, cfg, h, w, n_conds (6 | 1), n_steps, dtype are read; latent_channels / latent_pad are derived from the config */
int es_load_weights(const es_weights* w, const es_model_config* cfg, const es_ctx_geometry* g, int device, es_ctx** out);
/* The launch planner the builders share (host-only): the N tile (bn), split-K factor and LDS ring depth es_load_weights picks for
 * an es_conv_gemm launch of M output pixels among the candidate tiles `bns` (edgestyle_amd/ops.py plan_gemm makes the same
 * choice for the Python host; tests hold the two against each other), and whether a plain linear layer takes es_linear_xs. */
int es_plan_gemm_choice(long long M, int rows_padded, int kpad, int geglu, const int* bns, int n_bns, int allow_split,
                        int* bn, int* splitk, int* stages);
int es_linear_xs_eligible(long long M, int ksize, int kpad, int cin, int ctail, int cout, int geglu);
/* The launch policy (host-only): every decision between "this convolution / linear call is valid" and "its descriptor is
 * filled" - kernel, tile, split-K, ring depth, waves, XCD order, GroupNorm hand-over, two-word stream - taken in ONE place for
 * both hosts (edgestyle_amd/ops.py conv_gemm and es_load_weights), so that they issue the same launches by construction.
 * es_launch_query: the facts of one call the policy looks at. */
typedef struct {
  long long M, hw;                  /* output pixels of the launch / of one sample */
  long long w_numel, src_numel;     /* XCD rule: elements of one packed weight set / of the sources as the launch reads them */
  int32_t ksize, stride, upsample, C1, C2;
  int32_t rows_padded, kpad, cin, ctail, cout, geglu, has_ln;     /* packed-weight geometry (has_ln: LayerNorm folded in) */
  int32_t act;                      /* the caller's ES_ACT_* (GEGLU follows from the weights) */
  int32_t has_temb, has_residual;
  int32_t residual_dense;           /* the residual is a dense [M, Cout_store] tensor (es_linear_xs takes no other) */
  int32_t unit_scale;               /* out_scale == 1 and no device scale */
  int32_t n_tails, x_rep, wide;     /* wide: the caller asks for the two-word residual stream (granted by the knobs and dtype) */
  int32_t dtype, gn_groups;         /* gn_groups > 0: a GroupNorm over that many groups reads the output */
  int32_t ngroups;                  /* weight sets of a grouped launch (0: not grouped) */
  int32_t n_counts, group_n[4];     /* samples per group as the caller gave them (at most 4 are looked at) */
  int32_t groups_agree;             /* the groups' weights agree in what the rule compares: the LayerNorm fold (es_launch_choose),
                                       the fold and the geometry (es_launch_gn_fold) */
  int32_t force_splitk, stages;     /* caller overrides: split-K factor (0 = planned) and LDS ring depth (0 = planned) */
} es_launch_query;
/* every switch and tool knob that bends a decision (the Python host fills it from the attributes of edgestyle_amd.ops, es_load_weights
 * from the environment switches it honours: README.md) */
typedef struct {
  int32_t xs_enabled, xs_residual, xs_min_m;                 /* es_linear_xs: at all / with a residual / from M rows on (0: every shape it runs) */
  int32_t big_tile, big_tile_256, small_tile, eight_waves;   /* the 256 x 320, 256 x 256 and 64 x 64 tiles; 8 waves on short-K launches */
  int32_t deep_ring;                                         /* 0: a planned 4-deep LDS ring becomes 2 */
  int32_t gn_handover;                                       /* 0 off, 1 where the GroupNorm is the two-launch form, 2 everywhere */
  int32_t wide_stream;                                       /* -1 auto (bf16 only), 0, 1 */
  int32_t gn_fold;                                           /* GroupNorm in front of proj_in inside es_linear_xs */
  int32_t force_bn, force_waves, force_stages;               /* 0 = planned */
  int32_t xcd_order;                                         /* -1 auto, 0 tile_n fastest, 1 tile_m fastest */
} es_launch_knobs;
enum { ES_ROUTE_CONV_GEMM = 0, ES_ROUTE_LINEAR_XS = 1 };
typedef struct {
  int32_t route;                    /* ES_ROUTE_*; es_linear_xs: nothing below is set */
  int32_t bn, splitk, stages, waves, xcd_m_fastest;          /* es_gemm_desc fields of the same names */
  int32_t gn_partials;              /* emit the GroupNorm partial sums (es_gemm_desc.gn_part) */
  int32_t wide;                     /* carry the two-word stream (es_gemm_desc.residual_lo / out_lo) */
} es_launch_choice;
/* -1 (es_last_error) when no tile fits rows_padded */
int es_launch_choose(const es_launch_query* q, const es_launch_knobs* k, es_launch_choice* out);
/* the decisions taken outside a GEMM call: the kernel alone (ES_ROUTE_*, no tile planned); GroupNorm + proj_in as statistics pass +
 * es_linear_xs (q: the projection as es_launch_choose would get it, M / hw / weights / grouping are read); does a GEMM whose
 * [.., hw, c] output feeds a GroupNorm hand its statistics over; is the residual stream of this dtype carried in two words */
int es_launch_route(const es_launch_query* q, const es_launch_knobs* k);
int es_launch_gn_fold(const es_launch_query* q, int groups, const es_launch_knobs* k);
int es_launch_gn_handover(long long hw, int c, int groups, const es_launch_knobs* k);
int es_launch_wide_stream(int dtype, const es_launch_knobs* k);
/* the knobs as every host starts from them, before it reads its switches: every kernel and tile on (xs_enabled, xs_residual, big_tile,
 * big_tile_256, small_tile, eight_waves, deep_ring, gn_fold = 1), xs_min_m = 8192, xcd_order = wide_stream = -1, the rest 0 */
void es_launch_default_knobs(es_launch_knobs* k);
/* how an es_linear_xs launch of M rows, K = kpad, `cout` GEMM columns is cut into slices of whole 128-byte output lines
 * (es_xs_desc.nslices / chunks_per_slice): towards 256 workgroups, or towards `force_slices` slices where that is > 0 (a tool knob).
 * -1 (es_last_error) for a shape es_linear_xs does not run: K other than 320 | 640, no row, Cout not in whole lines. */
int es_launch_xs_slices(long long M, int kpad, int cout, int geglu, int force_slices, int32_t* nslices, int32_t* chunks_per_slice);
/* Does the 256 x 320 tile (bn = 320) implement the epilogue of a splitk == 1 launch with this form?  (It keeps the common
 * forms only - bias [+ one time-embedding row per 128-pixel half] [+ residual]; split-K launches write raw partials: every
 * form.)  1 = yes.  Both hosts ask BEFORE they fix bn, so that the tile a launch is planned, recorded and reported with is the
 * tile that runs (es_conv_gemm itself still falls back to the 128 x 160 tile for a caller that did not ask). */
int es_conv_gemm8p_form_ok(int act, int cout, int has_temb, long long out_hw, int has_residual);
/* 1 when this process runs under a profiler that intercepts the HSA queues (rocprofv3: ROCP_TOOL_LIBRARIES / a rocprofiler
 * library in LD_PRELOAD / a loaded rocprofiler_configure) while the HIP runtime still block-copies pre-built graph packets
 * (DEBUG_CLR_GRAPH_PACKET_CAPTURE unset or not 0): hipGraphLaunch of a context's graphs then faults inside the runtime
 * (profiles/r04_rocprof_graph_fault.txt).  The context replays its plans launch by launch in that case. */
int es_ctx_graph_hazard(void);
/* es_plan_set_dry(1): while a plan records on this thread, calls are validated and recorded but nothing is launched (the
 * pointers need not exist yet).  Returns the previous setting. */
int es_plan_set_dry(int on);

/* run ONE plan of the context on `stream` (guidance_scale: pointer to the CFG scale for the scheduler call of
 * ES_PLAN_STEP, or NULL = as recorded): single-stepping a prepared loop */
int es_ctx_launch_plan(es_ctx* c, int which, const float* guidance_scale, void* stream);
/* host-only helper: out[n][4] = {sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev)} for the DDIM (eta 0) update of
 * each timestep of the list, a_prev = alphas_cumprod of the next timestep (alphas_cumprod[0] after the last one: the
 * SD1.5 scheduler_config's set_alpha_to_one False); alphas_cumprod NULL = SD1.5's scaled_linear schedule */
int es_ddim_coef_table(const float* alphas_cumprod, int n_alphas, const float* timesteps, int n, float* out);
/* sample dtype [N,h,w,latent_pad]; ehs dtype [N,77,D]; cond_embeds[n_conds] dtype [N,h,w,C0]; scales float[n_conds] (host)
 * or NULL (ones); out_noise dtype [N,h,w,out_channels].  All device pointers except `scales`.
 * Stream capture: es_denoise_step and es_denoise_loop stage host values (timestep, scales, per-step tables) through pinned
 * memory and REFUSE a capturing stream (-1); they replay hipGraphs of their own (es_ctx_set_options use_graphs).  To place a
 * step inside a graph of yours, fill the bound buffers yourself and capture es_ctx_launch_plan, which es_vae_decode and
 * es_prepare_conds (device-to-device copies + one plan) also support. */
int es_denoise_step(es_ctx* c, const void* sample, float t, const void* ehs, const void* const* cond_embeds,
                    const float* scales, void* out_noise, void* stream);
/* latents fp32 [B,h,w,L] (device, in/out); ehs as above; timesteps: HOST float[n_steps] (981, 961, ... for 50 steps);
 * the condition embeddings are the ones last copied into ES_BUF_COND* (es_denoise_step does, or the builder). */
int es_denoise_loop(es_ctx* c, float* latents_inout, const void* ehs, float guidance_scale, const float* timesteps,
                    int n_steps, void* stream);
int es_vae_decode(es_ctx* c, const float* latents, float* out_img, void* stream);
/* == prepare_image + the one-time conditioning embedding (model/edgestyle_pipeline.py:352-377, 629-664;
 * model/controllora.py:28-42, 289-290): images[n_conds] device fp32 NCHW [B,3,8h,8w]; noise[n_conds] device fp32
 * [N,latent_channels,h,w] for the nets whose ES_BUF_COND_NOISE slot is bound (the VAE-conditioned ones: the caller's own
 * noise, what the reference's global generator would draw; NULL for such a net keeps what es_ctx_draw_cond_noise last drew
 * into the slot and is refused where nothing was drawn), ignored (may be NULL) for the others.  Each shared
 * encoder (the VAE of the LoRA nets, the conv stack of the pose net) runs once over the un-duplicated images of all its
 * nets; results land in ES_BUF_COND0.. as [N,h,w,C0], ready for es_denoise_loop / es_ctx_launch_plan. */
int es_prepare_conds(es_ctx* c, const float* const* images, const float* const* noise, void* stream);

/* =========================================================================================================
 * Byte images (csrc/image_io.hip): what a caller holds is a decoded photo - uint8, HWC, any size - and what it wants back is
 * bytes.  Replaces, on the input side, the transforms the reference's callers apply to every condition image
 * (test_text2image_pretrained_openpose.py:29-48): torchvision Resize(R, BILINEAR) on a PIL image -> CenterCrop(R) -> ToTensor
 * (-> Normalize(.5, .5) for the VAE-conditioned nets); on the output side image_processor.postprocess(output_type "pil")'s
 * (x * 255).round().astype(uint8) (model/edgestyle_pipeline.py:570-572).  The resize is Pillow's ImagingResample restated:
 * horizontal pass, then vertical pass, a uint8 image after each, per-pixel weights derived in double and quantised to 22 bits,
 * integer accumulation - the bytes EQUAL Pillow's.  A pass whose size does not change is skipped, as Pillow skips it.
 * Output size and crop are torchvision's: the shorter side becomes R, the longer (int)(R * long / short); the crop starts at
 * (int)rint((rh - R) / 2.0) (round half to even) and likewise for the columns.
 * None of these calls is ever part of a plan: while a plan records on the calling thread they return -1.  No new
 * ES_ABI_VERSION: no plan or context image records them.
 * ========================================================================================================= */
typedef struct {
  const uint8_t* data;             /* DEVICE memory: height rows of row_stride bytes, `channels` bytes per pixel (R, G, B[, A]) */
  int32_t height, width;
  int32_t channels;                /* 3 | 4 (the fourth byte is ignored) */
  int64_t row_stride;              /* bytes, >= width * channels */
} es_image_u8;
/* host-only: out = {rh, rw, top, left} - the size Resize(R) gives a height x width image and where CenterCrop(R) starts */
int es_image_fit(int height, int width, int R, int32_t out[4]);
/* host-only: the taps of one axis resampled from `in` to `out` pixels, computed by THE SAME code the kernels run (one
 * __host__ __device__ function): output pixel i reads source pixels xmin[i] .. xmin[i] + ntaps[i] - 1 with the 22-bit fixed-point
 * weights k[i * cap + 0 ..]; result = clip8(((1 << 21) + sum k * src) >> 22).  xmin / ntaps: [out] or NULL; k: [out][cap] or NULL.
 * Returns the longest run of taps (ask with k = NULL to size cap), -1 on bad arguments or a cap smaller than that. */
int es_image_resize_coeffs(int in, int out, int32_t* xmin, int32_t* ntaps, int32_t* k, int cap);
/* host-only: bytes of device scratch es_image_resize_u8 / es_prepare_conds_u8 need for these images (the uint8 image between
 * the two passes: the source rows the kept output rows read x the R kept columns, for every image whose width changes; may be
 * 0).  Only height / width of the descriptors are read.  0 with es_last_error() set on bad arguments. */
size_t es_image_resize_workspace_bytes(const es_image_u8* imgs, int count, int R);
/* imgs: HOST array of `count` descriptors (images of different sizes in one call: two launches per 16 images);
 * out: device uint8 [count, R, R, 3].  Asynchronous on `stream`, nothing is allocated: capturable. */
int es_image_resize_u8(const es_image_u8* imgs, int count, uint8_t* out, int R, void* workspace, size_t workspace_bytes, void* stream);
/* ToTensor (+ Normalize(.5, .5) if normalize): uint8 HWC [count,H,W,3] -> fp32 NCHW [count,3,H,W], y = x / 255.0f (correctly
 * rounded), then y = (y - 0.5f) / 0.5f - bitwise what numpy / torch compute on the host for the same bytes */
int es_image_u8_to_f32(const uint8_t* in, float* out_nchw, int count, int H, int W, int normalize, void* stream);
/* fp32 NCHW [B,3,H,W] in [0,1] -> uint8 HWC [B,H,W,3]: b = (uint8) clamp(rintf(x * 255.0f), 0, 255), no fused multiply-add ahead
 * of the rounding; four pixels per thread */
int es_image_f32_to_u8(const float* in_nchw, uint8_t* out_hwc, int B, int H, int W, void* stream);
/* The same four calls with the FILTER and the CROP RULE chosen (the calls above are ES_FILTER_BILINEAR with ES_CROP_TORCHVISION and keep
 * their bytes).  ES_FILTER_BICUBIC is Pillow's BICUBIC - the Keys cubic with a = -0.5, support 2.0 (stretched by the scale when shrinking),
 * negative weights quantised as (int)(-0.5 + w * (1 << 22)) - which transformers' CLIPImageProcessor resizes with (model/utils.py:647-684
 * through CLIPProcessor); its wider support widens the range of source rows the horizontal pass keeps for the vertical one.
 * ES_CROP_TRANSFORMERS is transformers.image_transforms.center_crop: top = (rh - R) // 2, left = (rw - R) // 2 (the half is dropped,
 * where torchvision rounds it to even).  The size rule is the same for both: shortest edge -> R, the other (int)(R * long / short). */
enum { ES_FILTER_BILINEAR = 0, ES_FILTER_BICUBIC = 1, ES_FILTER_LANCZOS = 2 /* coeffs_ex and the windowed calls below only */ };
enum { ES_CROP_TORCHVISION = 0, ES_CROP_TRANSFORMERS = 1 };
int es_image_fit_ex(int height, int width, int R, int crop, int32_t out[4]);
int es_image_resize_coeffs_ex(int filter, int in, int out, int32_t* xmin, int32_t* ntaps, int32_t* k, int cap);
size_t es_image_resize_workspace_bytes_ex(const es_image_u8* imgs, int count, int R, int filter, int crop);
int es_image_resize_u8_ex(const es_image_u8* imgs, int count, uint8_t* out, int R, int filter, int crop, void* workspace,
                          size_t workspace_bytes, void* stream);
/* es_prepare_conds from bytes: images[n_conds * B] (HOST array, net-major: image b of net i is images[i * B + b]) are resized,
 * cropped and converted straight into the bound ES_BUF_COND_IMG* slots (format unchanged: fp32 NCHW [B,3,8h,8w]; normalize[i] != 0
 * for the nets that take [-1,1], TT:29-48), the noise is copied and the unchanged ES_PLAN_CONDS runs, as in es_prepare_conds.
 * workspace: es_image_resize_workspace_bytes(images, n_conds * B, 8h) bytes.  The reference's transform is square: a context with
 * 8h != 8w is refused.  Capturable like es_prepare_conds. */
int es_prepare_conds_u8(es_ctx* c, const es_image_u8* images, const int32_t* normalize, const float* const* noise,
                        void* workspace, size_t workspace_bytes, void* stream);
/* es_vae_decode to bytes: the unchanged decode plan into ES_BUF_IMAGE, then es_image_f32_to_u8 from there;
 * out_hwc device uint8 [B,8h,8w,3].  Capturable like es_vae_decode. */
int es_vae_decode_u8(es_ctx* c, const float* latents, uint8_t* out_hwc, void* stream);

/* =========================================================================================================
 * Person crop (csrc/image_io.hip): create_processed_image (extract_dataset.py:112-171) - the photo resized with Pillow's LANCZOS so that
 * the person box with a 10 % margin fits 512 x 512, and a 512 x 512 window cut around the box centre - from a decoded photo and the
 * detector's box.  ES_FILTER_LANCZOS is Pillow's LANCZOS: sinc(x) * sinc(x / 3) on [-3, 3), support 3.0 (stretched by the scale when
 * shrinking), through the same coefficient code, 22-bit quantisation and two uint8 passes as the other filters: the bytes equal Pillow's.
 * es_image_resize_coeffs_ex and the windowed calls take it; the centre-crop calls above keep their two filters.
 * Opt-in: no existing call changes its bytes; never part of a plan (-1 while one records on the thread), ES_ABI_VERSION stays.
 * ========================================================================================================= */
/* host-only: lines 118-164 in double, in the reference's order of operations and with its int() truncations.  box = {xmin, ymin, xmax,
 * ymax} in pixels of the height x width photo; out = {new_w, new_h, left, top}: the size the photo is resized to and where the
 * final_w x final_h window starts in it.  left / top are NEGATIVE when the resized photo is smaller than the window (a tall narrow
 * photo: new_w - final_w < 0), as in the reference, whose PIL crop then pads with zeros.  -1: bad arguments, or a box that is empty
 * once the margin is added and it is cut to the photo (the reference divides by zero there). */
int es_person_crop_fit(int height, int width, const double box[4], int final_w, int final_h, double margin, int32_t out[4]);
/* imgs: HOST array of `count` descriptors (device bytes, any sizes, pitched rows, 3 | 4 channels); geom: HOST int32 [count][4] =
 * {new_w, new_h, left, top} per image.  Image i is resized to new_h x new_w with `filter` (any ES_FILTER_*; an axis whose size stays is
 * skipped, as Pillow skips it) and out[i] - device uint8 [count, out_h, out_w, 3] - receives the window whose corner is (top, left);
 * bytes of the window outside the resized image are 0.  Only the columns the window shows and the source rows its rows read are
 * computed.  workspace: the uint8 image between the passes, es_image_resize_window_u8_workspace_bytes (may be 0).  Asynchronous on
 * `stream`, nothing is allocated: capturable.  Two launches per 16 images. */
size_t es_image_resize_window_u8_workspace_bytes(const es_image_u8* imgs, int count, const int32_t* geom, int out_h, int out_w, int filter);
int es_image_resize_window_u8(const es_image_u8* imgs, int count, const int32_t* geom, uint8_t* out, int out_h, int out_w, int filter,
                              void* workspace, size_t workspace_bytes, void* stream);
/* create_processed_image in one call: es_person_crop_fit(.., 512, 512, 0.1) per image, then es_image_resize_window_u8(.., 512, 512,
 * ES_FILTER_LANCZOS).  boxes: HOST double [count][4]; out: device uint8 [count, 512, 512, 3] - the "processed" photo the SAM encoder,
 * es_sam_compose and es_clip_pick take. */
size_t es_person_crop_u8_workspace_bytes(const es_image_u8* imgs, int count, const double* boxes);
int es_person_crop_u8(const es_image_u8* imgs, int count, const double* boxes, uint8_t* out, void* workspace, size_t workspace_bytes,
                      void* stream);

/* =========================================================================================================
 * Pose rendering (csrc/pose.hip): controlnet_aux's draw_poses(.., draw_body=True, draw_hand=False, draw_face=False) on a black canvas,
 * as create_openpose calls it after detect_poses (extract_dataset.py:222-295), and the host logic around it.  The detectors themselves
 * (YOLOv5, OpenPose) are not part of this library.
 * KEY POINTS: fp32 [count, 18, 3] = (x, y, score), x and y normalised to [0, 1] as in the reference's JSON (OpenPose body order: nose,
 * neck, r-shoulder, r-elbow, r-wrist, l-shoulder, l-elbow, l-wrist, r-hip, r-knee, r-ankle, l-hip, l-knee, l-ankle, r-eye, l-eye, r-ear,
 * l-ear).  A key point is ABSENT iff its score is not > 0 (NaN counts as absent).  es_pose_draw moreover does not draw a present point
 * whose pixel position |x * W| or |y * H| is not below 65536 (or is NaN): it lies at least three canvases outside.
 * WHAT IS DRAWN, in this order, the last writer winning, clipped at the canvas edge:
 *  - limbs 1 .. 17 = (from, to), 1-based: (2,3) (2,6) (3,4) (4,5) (6,7) (7,8) (2,9) (9,10) (10,11) (2,12) (12,13) (13,14) (2,1) (1,15)
 *    (15,17) (1,16) (16,18), skipped when either end is absent, in colour int(c * 0.6) per channel of
 *    colours 1 .. 18 = (255,0,0) (255,85,0) (255,170,0) (255,255,0) (170,255,0) (85,255,0) (0,255,0) (0,255,85) (0,255,170) (0,255,255)
 *    (0,170,255) (0,85,255) (0,0,255) (85,0,255) (170,0,255) (255,0,255) (255,0,170) (255,0,85);
 *  - then every present key point i as a disc of radius 4 in colour i.
 * The result is uint8 HWC [count, H, W, 3], what es_prepare_conds_u8 takes (normalize 0) as it lies; the reference's trailing cv2.resize
 * to the same size is the identity.
 * WHICH PIXELS A SHAPE COVERS is OpenCV's polygon and circle rasteriser in the reference; here it is this rule, in integers:
 *  - X = (double)x * W, Y = (double)y * H (one IEEE product each).  A limb from P to Q has centre (cx, cy) = ((int)((X_P + X_Q) / 2),
 *    (int)((Y_P + Y_Q) / 2)); qx = (int64)((X_P - X_Q) * 256), qy likewise (every cast truncates toward zero, like Python's int());
 *    a = isqrt(qx^2 + qy^2) >> 9 is int(length / 2); its angle t = int(degrees(atan2(dy, dx))) is found without atan2: with
 *    S(t) = round(sin(t deg) * 2^30) from a fixed 91-entry table (and its symmetries; C(t) = S(t + 90)), t' is the first of 0 .. 180
 *    for which t' = 180 or C(t' + 1) * |qy| - S(t' + 1) * qx < 0, and t = t' or, when qy < 0, -t'.
 *  - The limb is the ellipse with semi-axes a + 1/2 along (C(t), S(t)) and 4 + 1/2 across it (the half pixel stands for the boundary
 *    OpenCV's fill includes); a point is the disc of radius 4 around ((int)X, (int)Y), rim included.  With A = 2a + 1, B = 9 (A = B = 8
 *    and t = 0 for a disc), pixel (px, py) is covered iff, for u = px - cx, v = py - cy,
 *      al = (u * C + v * S + 2^21) >> 22,  ac = (v * C - u * S + 2^21) >> 22      (floor; 1/256 pixel along and across)
 *      |al| <= 128 A  and  |ac| <= 128 B  and  al^2 B^2 + ac^2 A^2 <= 16384 A^2 B^2      (64-bit integers).
 *    A limb whose ends coincide (a = 0) is a stroke one pixel wide and nine long across its direction.
 * No atan2, sqrt, sin or cos is evaluated anywhere, so es_pose_draw_host - the same __host__ __device__ code - and the kernel agree bit
 * for bit.  Against the reference's own renderings of docs/test/{source,target}/openpose/N.json the rule reaches a whole-image PSNR of
 * 34.3 - 34.6 dB and an IoU of 0.93 (pixels whose largest channel exceeds 40), as tests/test_pose_cpu.py asserts; it is not OpenCV's
 * rasteriser byte for byte.
 * Never part of a plan (-1 while one records on the thread); ES_ABI_VERSION stays.
 * ========================================================================================================= */
/* kp: DEVICE fp32 [count, 18, 3]; out: DEVICE uint8 [count, H, W, 3], every byte written.  1 <= H, W <= 16384, count <= 65535.  One
 * launch for the whole batch, no atomics, nothing allocated: capturable. */
int es_pose_draw(const float* kp, uint8_t* out, int count, int H, int W, void* stream);
/* host-only: the same on HOST memory */
int es_pose_draw_host(const float* kp, uint8_t* out, int count, int H, int W);
/* host-only: create_openpose's filters and choice (lines 222-268) over n candidates - kps HOST fp32 [n, 18, 3], total_score and
 * total_parts HOST double [n].  Kept: score > 10, parts > 5, any of nose / neck / eyes / ears present, a shoulder present, a hip present.
 * Chosen: the largest area of the box around the present key points (in normalised coordinates), ties in input order.  Returns its
 * index, -1 when none remains (n = 0 included), -2 on bad arguments. */
int es_pose_select_host(const float* kps, const double* total_score, const double* total_parts, int n);
/* host-only: the SAM point prompt of create_sam_images:361-365 - the present key points of one pose (kp HOST fp32 [18, 3]) times (W, H),
 * in order, into out (HOST fp32 [18, 2], the first `count` rows written); returns count, -1 on bad arguments.  The rows are what
 * es_sam_prompts.points takes, with label 1 each. */
int es_pose_points_host(const float* kp, int W, int H, float* out);

/* =========================================================================================================
 * JPEG decoding (csrc/jpeg.h, csrc/jpeg.hip): the bytes of a baseline JPEG file -> uint8 [H, W, 3] RGB on the device, what Pillow's
 * Image.open(..).convert("RGB") gives (libjpeg's default decoder settings: JDCT_ISLOW, fancy upsampling), byte for byte.  Two halves that
 * meet at the quantised DCT coefficients: header parsing and Huffman decoding are serial and stay on the host (plain C++, csrc/jpeg.h;
 * that is the default - the Huffman decoding on the device, below es_jpeg_decode_u8, is opt-in);
 * dequantisation, the 8x8 inverse DCT, chroma upsampling and YCbCr -> RGB are two launches on the device, and es_jpeg_reconstruct_host
 * runs the same __host__ __device__ integer code on the CPU, bit for bit.
 * SUPPORTED: SOF0 / SOF1, 8-bit samples, Huffman coding, one interleaved scan; 1 component (gray -> R = G = B) or 3 components YCbCr
 * (JFIF, Adobe transform 1, or neither marker and component ids other than 'R','G','B') with luma sampling 1x1, 2x1 or 2x2 and chroma
 * 1x1 (4:4:4, 4:2:2, 4:2:0); 8- and 16-bit quantisation tables, any number of DQT / DHT segments, DRI with RST0-7, 0xFF fill bytes; APPn
 * and COM are skipped (EXIF orientation is not applied, as Pillow's open does not apply it).
 * REFUSED, with the reason in es_last_error(): progressive (SOF2), lossless, arithmetic coding, 12-bit samples, 4 components (CMYK),
 * Adobe transform 0 or RGB ids, other sampling factors, multi-scan files, a height or width of 0, anything truncated or malformed (a
 * bad Huffman code, a missing table, a run past coefficient 63, a missing or misnumbered RST, no EOI after the scan).  The parser never
 * reads past n and never writes outside the coefficient buffer, on any input.
 * THE ARITHMETIC: coef * q; the 13-bit fixed-point "islow" inverse DCT (columns descaled by (x + 1024) >> 11, rows by (x + 2^17) >> 18,
 * + 128, clamped to 0 .. 255); a component has ceil(W * h / hmax) x ceil(H * v / vmax) samples, the rest of its padded blocks is never
 * read.  Chroma of width dw > 2 is upsampled with libjpeg's triangle filters - 4:2:2: out[2i] = (3 in[i] + in[i-1] + 1) >> 2,
 * out[2i+1] = (3 in[i] + in[i+1] + 2) >> 2; 4:2:0: s[i] = 3 near[i] + far[i] (far: the chroma row above for even output rows, below for
 * odd ones), out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4 - every index clamped to the real samples;
 * dw <= 2: plain replication.  R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
 * B = Y + ((116130 cb + 32768) >> 16) with cb, cr less 128, arithmetic shifts, clamped.
 * HOSTILE COEFFICIENTS: the inverse DCT is computed modulo 2^32 (unsigned arithmetic, reinterpreted as two's complement before each
 * descaling shift): what the encoder of a real image wrote never gets near the limit, anything else gives defined, identical bytes on
 * both sides instead of undefined behaviour.
 * Opt-in: no existing call changes its bytes; never part of a plan (-1 while one records on the thread), ES_ABI_VERSION stays.
 * ========================================================================================================= */
typedef struct {
  int32_t width, height;
  int32_t components;              /* 1 | 3 */
  int32_t h[3], v[3];              /* sampling factors per component (a single component counts as 1 x 1: its scan is not interleaved) */
  int32_t tq[3], td[3], ta[3];     /* quantisation, DC and AC Huffman table selectors per component */
  int32_t hmax, vmax;
  int32_t mcus_x, mcus_y;          /* MCU grid: ceil(width / (8 hmax)) x ceil(height / (8 vmax)) */
  int32_t blocks_w[3], blocks_h[3];/* padded block grid per component: mcus_x * h x mcus_y * v */
  int32_t restart_interval;        /* MCUs between RSTn markers, 0: none */
} es_jpeg_info;
/* host-only: reads the headers up to the scan.  0, or -1 with the reason for a file this decoder refuses */
int es_jpeg_info_host(const uint8_t* bytes, size_t n, es_jpeg_info* info);
/* host-only: int16 coefficients of one image: 64 per block of every component's padded grid (0 with es_last_error() on a bad info) */
size_t es_jpeg_coeff_count(const es_jpeg_info* info);
/* host-only: Huffman decoding.  coeffs: HOST int16 [es_jpeg_coeff_count] - component after component, within one the blocks row by row
 * (block (by, bx) of component c at 64 * (by * blocks_w[c] + bx) past the component's start), each block in natural (row-major,
 * de-zigzagged) order, every value written.  qtables: HOST uint16 [components][64], the table of each COMPONENT in natural order.
 * `info` must be what es_jpeg_info_host gave for these bytes. */
int es_jpeg_entropy_decode_host(const uint8_t* bytes, size_t n, const es_jpeg_info* info, int16_t* coeffs, uint16_t* qtables);
/* bytes of device scratch es_jpeg_reconstruct needs (the uint8 component planes between its two launches); 0 with es_last_error() */
size_t es_jpeg_reconstruct_workspace_bytes(const es_jpeg_info* infos, int count);
/* infos: HOST array of `count` descriptors (images of different sizes and samplings in one call: two launches per 16 images);
 * coeffs_dev[i] / qtables_dev[i]: DEVICE copies of what es_jpeg_entropy_decode_host wrote for image i, each 16-byte aligned;
 * out[i]: DEVICE memory (`data` is written) of infos[i].height x infos[i].width, channels 3, any row_stride >= width * 3 - exactly
 * width * 3 bytes of each row are written.  Asynchronous on `stream`, nothing is allocated: capturable. */
int es_jpeg_reconstruct(const es_jpeg_info* infos, int count, const int16_t* const* coeffs_dev, const uint16_t* const* qtables_dev,
                        const es_image_u8* out, void* workspace, size_t workspace_bytes, void* stream);
/* host-only: the same on HOST memory (out[i].data included); needs no workspace */
int es_jpeg_reconstruct_host(const es_jpeg_info* infos, int count, const int16_t* const* coeffs, const uint16_t* const* qtables,
                             const es_image_u8* out);
/* Parse + upload + reconstruct for up to 64 files.  bytes[i] / n[i]: the files (HOST).  out[i]: as above, sized from
 * es_jpeg_info_host.  staging_host (HOST, pinned for an asynchronous upload) and staging_dev (DEVICE, 16-byte aligned) hold
 * es_jpeg_decode_staging_bytes each: the coefficients and tables of all images, copied by one hipMemcpyAsync on `stream`; staging_host
 * must stay untouched until that copy has run.  workspace: es_jpeg_reconstruct_workspace_bytes.  Nothing is allocated.  The Huffman
 * decoding runs on the calling thread, so this call is not one to capture. */
size_t es_jpeg_decode_staging_bytes(const es_jpeg_info* infos, int count);
int es_jpeg_decode_u8(const uint8_t* const* bytes, const size_t* n, int count, const es_image_u8* out, void* staging_host,
                      void* staging_dev, size_t staging_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Huffman decoding on the device (csrc/jpeg_entropy.hip), opt-in: THE DEFAULT IS STILL THE HOST DECODER - es_jpeg_decode_u8 and every
 * call above keep their code paths and bytes.  The file's bytes in device memory -> the int16 coefficient buffer that
 * es_jpeg_entropy_decode_host writes, bit for bit, in the layout es_jpeg_reconstruct takes.  The host keeps the header parse and one
 * walk over the scan that finds the SEGMENTS (the entropy-coded bytes between restart markers; a file without DRI has one) and checks
 * what the serial decoder checks around them (RSTn present and numbered, EOI after the last one) - no Huffman decoding.
 * One workgroup of 1024 decoders owns one segment (grid.y = image, 16 images per launch; sizes, samplings and segment counts mix).  The
 * segment's `len` raw bytes are cut into J = ceil(len / S) subsequences, S = max(subseq_bytes, ceil(len / 1024)), one decoder each.
 * Bits are read from the raw bytes (a byte carries data unless it is a 00 after an FF or an FF before an FF).  Huffman streams
 * re-synchronise: every decoder starts from a guessed state (position, block within the MCU, zigzag index), proposes its exit state to
 * its neighbour, and the rounds repeat until no entry changes - at most J + 1, a handful on real files (a decoder handed
 * the dead state of a neighbour that met an impossible code proposes from its own guess again; once the rounds have settled, the first
 * dead entry and everything behind it write nothing); then the counts of blocks
 * and the sums of DC differences are scanned across the workgroup and each decoder decodes once more from its true state and writes.
 * Workgroups never wait for one another.  Every store address comes from block counters checked against the geometry; blocks past a
 * segment's share are dropped, padding bits and stray bytes before a marker are not an error.
 * STATUS: one int32 per image in device memory, 0 or the first defect by (segment, block): 1 no DC code, 2 no AC code, 3 a zero run
 * past coefficient 63, 4 a DC coefficient outside 16 bits, 5 truncated (a needed symbol ends past the segment's bits, or the segment
 * holds fewer blocks than it must).  The call is asynchronous: read the word after synchronising; es_jpeg_status_text gives the text.
 * LIMIT: files below 256 MiB.  Every call here returns -1 while a plan records.  es_jpeg_entropy_decode_parallel_host is the twin: the
 * same __host__ __device__ code and the same rounds on the CPU.
 * --------------------------------------------------------------------------------------------------------- */
#define ES_JPEG_TABLES_BYTES 8560
typedef struct { uint32_t begin, end; } es_jpeg_segment;    /* [begin, end): offsets from the file's first byte */
/* host-only: the number of segments: ceil(MCUs / restart_interval), 1 without DRI (0 with es_last_error() on a bad info) */
size_t es_jpeg_segment_count(const es_jpeg_info* info);
/* host-only: segments: HOST [es_jpeg_segment_count]; tables: HOST, ES_JPEG_TABLES_BYTES (the Huffman tables of each component,
 * flattened); qtables: HOST uint16 [components][64] as es_jpeg_entropy_decode_host writes them.  0, or -1 with the serial decoder's
 * reason (a missing or misnumbered RSTn marker, no EOI after the scan, ...). */
int es_jpeg_scan_prepare_host(const uint8_t* bytes, size_t n, const es_jpeg_info* info, es_jpeg_segment* segments, void* tables,
                              uint16_t* qtables);
/* host-only: bytes of device scratch es_jpeg_entropy_decode needs (one status word per segment); 0 with es_last_error() */
size_t es_jpeg_entropy_decode_workspace_bytes(const es_jpeg_info* infos, int count);
/* bytes_dev[i]: DEVICE copy of file i, bytes_n[i] readable bytes (every offset of segments_dev is cut to it); segments_dev[i] /
 * tables_dev[i]: DEVICE copies of what es_jpeg_scan_prepare_host wrote, 4-byte aligned; subseq_bytes: 0 (the default, 128) or >= 4;
 * coeffs_dev[i]: DEVICE int16 [es_jpeg_coeff_count], 16-byte aligned, every value written (zeroed by a memset node first);
 * status_dev: DEVICE int32 [count].  Asynchronous on `stream`, nothing is allocated: capturable. */
int es_jpeg_entropy_decode(const es_jpeg_info* infos, int count, const uint8_t* const* bytes_dev, const size_t* bytes_n,
                           const es_jpeg_segment* const* segments_dev, const void* const* tables_dev, int subseq_bytes,
                           int16_t* const* coeffs_dev, int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream);
/* host-only: the twin, everything in HOST memory.  threads: 1 .. 1024, stands for the workgroup's size; status: int32 [count];
 * rounds_out (may be NULL): the largest number of synchronise rounds a segment of these images took. */
int es_jpeg_entropy_decode_parallel_host(const es_jpeg_info* infos, int count, const uint8_t* const* bytes, const size_t* bytes_n,
                                         const es_jpeg_segment* const* segments, const void* const* tables, int subseq_bytes, int threads,
                                         int16_t* const* coeffs, int32_t* status, int32_t* rounds_out);
const char* es_jpeg_status_text(int code);
/* Parse + prepare on the host, ONE upload of the files, segments and tables from pinned staging, Huffman decoding on the device,
 * es_jpeg_reconstruct: the host never touches a coefficient.  Up to 64 files.  es_jpeg_decode_dev_staging_bytes returns the size of
 * staging_dev (DEVICE, 16-byte aligned: the upload, then coefficients and scratch) and stores in *upload_bytes the size of
 * staging_host (HOST, pinned, 16-byte aligned; untouched until the copy has run).  status_dev: DEVICE int32 [count], as above.
 * workspace: es_jpeg_reconstruct_workspace_bytes.  Nothing is allocated. */
size_t es_jpeg_decode_dev_staging_bytes(const es_jpeg_info* infos, const size_t* n, int count, size_t* upload_bytes);
int es_jpeg_decode_dev_u8(const uint8_t* const* bytes, const size_t* n, int count, const es_image_u8* out, int subseq_bytes,
                          int32_t* status_dev, void* staging_host, size_t staging_host_bytes, void* staging_dev, size_t staging_dev_bytes,
                          void* workspace, size_t workspace_bytes, void* stream);

/* =========================================================================================================
 * JPEG encoding (csrc/jpeg.h, csrc/jpeg_encode.hip): uint8 [H, W, 3] RGB (or [H, W] gray) on the device -> the bytes of the file that
 * Pillow's Image.fromarray(a).save(f, "JPEG", quality=q, subsampling=s[, restart_marker_blocks=r]) writes (Pillow 12.2 over
 * libjpeg-turbo 3: the pair tests/golden/jpeg_encode.safetensors is pinned to), byte for byte.  The whole file is written by the device:
 * what crosses the bus afterwards is the finished file and its length.  Two stages that meet at the decoder's coefficient buffer
 * (es_jpeg_coeff_count int16: block-major per component, MCU-padded grid, natural order inside a block, dummy blocks included):
 *  FORWARD  colour conversion (Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + 128 << 16 + 32767)
 *   >> 16, Cr = (32768 R - 27439 G - 5329 B + 128 << 16 + 32767) >> 16; one channel is its own luma), edge replication at full
 *   resolution (rows only to a multiple of the vertical factor), box downsampling ((a + b + {0,1,0,1..}) >> 1 for 4:2:2,
 *   (a + b + c + d + {1,2,1,2..}) >> 2 for 4:2:0), replication of the downsampled plane's last row to whole blocks, the 13-bit "islow"
 *   forward DCT on sample - 128 and coef = sign(c) (|c| + 4 q) / (8 q) with the Annex K tables scaled by the quality
 *   (scale = q < 50 ? 5000 / q : 200 - 2 q; entry = clamp((base * scale + 50) / 100, 1, 255)).  A dummy block (luma of 4:2:2 / 4:2:0
 *   with an odd block count) has zero AC and the DC of the block to its left, or, below the last row, of the last block of the row above
 *   within its MCU.
 *  ENTROPY  the standard Huffman tables of Annex K.3, one interleaved scan; SOI, APP0 (JFIF 1.01, density 1 x 1), one DQT per table,
 *   SOF0, four DHT (two for gray), DRI when a restart interval is set, SOS, data, EOI; nothing else.
 * On the device the entropy stage is parallel over blocks: code length per block (the DC predecessor from the scan geometry), a prefix
 * sum that also byte-aligns every restart interval, emission with atomicOr into zeroed words, a second count-and-scan for the 0x00 after
 * every 0xFF, and a scatter that bounds every store by the capacity.  8 launches per 16 images for es_jpeg_encode_u8 (1 forward + 7
 * entropy), images of different sizes and samplings share each launch.  Nothing is allocated, nothing synchronises: capturable.
 * LIMITS: 1 or 3 channels (4: "cannot write mode RGBA as JPEG"), sides of 1 .. 65535, and es_jpeg_encode_capacity below 2^30 (the
 * device counts the bits of one file in 32: about 2.5 million blocks - 160 megapixels at 4:4:4); no optimised tables, no
 * progressive or arithmetic coding, no EXIF / ICC / comment / dpi.  Opt-in: no existing call changes; never part of a plan (-1 while
 * one records on the thread), ES_ABI_VERSION stays.
 * ========================================================================================================= */
enum { ES_JPEG_444 = 0, ES_JPEG_422 = 1, ES_JPEG_420 = 2 };   /* Pillow's subsampling numbers */
typedef struct {
  int32_t quality;                 /* 1 .. 100 (Pillow's default: 75) */
  int32_t subsampling;             /* ES_JPEG_444 | ES_JPEG_422 | ES_JPEG_420 (Pillow's default); ignored for one channel */
  int32_t restart_interval;        /* MCUs between RSTn markers (Pillow's restart_marker_blocks), 0: none */
} es_jpeg_encode_params;
/* host-only: the geometry of the file these pixels become, in the decoder's struct.  0, or -1 with the reason */
int es_jpeg_encode_info_host(int width, int height, int channels, const es_jpeg_encode_params* params, es_jpeg_info* info);
/* host-only: SOI through SOS into out[0 .. cap); *n = their number (at most 629).  -1 if cap is short (*n is still set) */
int es_jpeg_header_host(const es_jpeg_info* info, const es_jpeg_encode_params* params, uint8_t* out, size_t cap, size_t* n);
/* host-only: an upper bound of the file's size, never a guess: header + 2 x (ceil(blocks x 1660 bits / 8) + one padding byte per restart
 * interval + 2 marker bytes per interval after the first) + EOI.  1660 = 11 + 11 (the longest DC code and the largest DC category) +
 * 63 x (16 + 10) (the longest AC code and the largest AC category for every coefficient); x 2: every byte may be 0xFF and take a stuffed
 * 0x00.  0 with es_last_error() on bad arguments or when the bound reaches 2^30. */
size_t es_jpeg_encode_capacity(const es_jpeg_info* info, const es_jpeg_encode_params* params);
/* host-only: bytes of device scratch es_jpeg_encode_u8 needs for these images (es_jpeg_forward and es_jpeg_entropy_encode need no more);
 * 0 with es_last_error() */
size_t es_jpeg_encode_workspace_bytes(const es_jpeg_info* infos, int count, const es_jpeg_encode_params* params);
/* Pixels -> coefficients.  images: HOST array of `count` descriptors of DEVICE pixels, 1 or 3 channels, any row_stride >= width *
 * channels (only width * channels bytes of a row are read); coeffs_dev[i]: DEVICE int16 [es_jpeg_coeff_count], 16-byte aligned, every
 * value written.  One launch per 16 images.  Asynchronous on `stream`; the workspace is not used by this stage (may be NULL / 0). */
int es_jpeg_forward(const es_image_u8* images, int count, const es_jpeg_encode_params* params, int16_t* const* coeffs_dev, void* workspace,
                    size_t workspace_bytes, void* stream);
/* host-only: the same integer code on HOST memory */
int es_jpeg_forward_host(const es_image_u8* images, int count, const es_jpeg_encode_params* params, int16_t* const* coeffs);
/* Coefficients -> the whole file, header and EOI included.  infos: what es_jpeg_encode_info_host gave; coeffs_dev[i]: DEVICE, 16-byte
 * aligned; out_dev[i]: DEVICE memory of capacity[i] bytes (any alignment); lengths_dev: DEVICE uint32 [count]; workspace: DEVICE,
 * es_jpeg_encode_workspace_bytes.  lengths_dev[i] always receives the number of bytes the file needs; if that exceeds capacity[i]
 * nothing at or beyond out_dev[i] + capacity[i] is written, the content below is unspecified and the caller must check.  A coefficient
 * outside the baseline categories (|DC difference| >= 2048, |AC| >= 1024: no forward stage produces one) is coded as its low bits:
 * the bounds hold, the file is not a valid one.  7 launches per 16 images.  Asynchronous on `stream`. */
int es_jpeg_entropy_encode(const es_jpeg_info* infos, int count, const es_jpeg_encode_params* params, const int16_t* const* coeffs_dev,
                           uint8_t* const* out_dev, const size_t* capacity, uint32_t* lengths_dev, void* workspace, size_t workspace_bytes,
                           void* stream);
/* host-only: the same on HOST memory; lengths: HOST uint32 [count].  -1 for a coefficient outside the baseline categories. */
int es_jpeg_entropy_encode_host(const es_jpeg_info* infos, int count, const es_jpeg_encode_params* params, const int16_t* const* coeffs,
                                uint8_t* const* out, const size_t* capacity, uint32_t* lengths);
/* Both stages for up to 64 images: 8 launches per 16 images.  Contracts as above; nothing outside [0, capacity[i]) of an output and
 * nothing outside the workspace is written. */
int es_jpeg_encode_u8(const es_image_u8* images, int count, const es_jpeg_encode_params* params, uint8_t* const* out_dev,
                      const size_t* capacity, uint32_t* lengths_dev, void* workspace, size_t workspace_bytes, void* stream);
/* host-only: the twin, pixels and files in HOST memory */
int es_jpeg_encode_host(const es_image_u8* images, int count, const es_jpeg_encode_params* params, uint8_t* const* out, const size_t* capacity,
                        uint32_t* lengths);

/* =========================================================================================================
 * Seeded noise (csrc/rng.hip): the normal stream of torch's DEVICE generator, restated, so that a host without Python can take
 * "seed 42" as an input and get the latents torch.randn(shape, generator=torch.Generator(device).manual_seed(42), device=device)
 * gives the reference's callers (test_text2image_pretrained_openpose.py:274, app.py:119).  The generator is Philox4x32-10 (ten
 * rounds, multipliers D2511F53 / CD9E8D57, Weyl constants 9E3779B9 / BB67AE85, key {seed lo, seed hi}, counter {offset / 4 lo,
 * offset / 4 hi, subsequence lo, subsequence hi}); a draw of numel floats is laid out as torch's grid-stride kernel lays it out:
 * blocks = min(block_cap, ceil(numel / 256)), T = 256 * blocks; element li is component (li % 4T) / T of the four normals (two
 * Box-Muller pairs: words x, y -> 0, 1; z, w -> 2, 3) of counter offset / 4 + li / 4T in subsequence li % T, and the generator
 * moves on by ((numel - 1) / 4T + 1) * 4.  block_cap = multiProcessorCount * (maxThreadsPerMultiProcessor / 256) of the device,
 * so the values of draws longer than 256 * block_cap elements depend on the device, as torch's do.
 * Host noise - the caller's own arrays, as before - stays the default everywhere: the CPU oracle can reproduce it, a device
 * stream it cannot.  None of these calls is ever part of a plan: while a plan records on the calling thread they return -1.
 * No new ES_ABI_VERSION: no plan or context image records them.
 * ========================================================================================================= */
typedef struct { uint64_t seed, offset; } es_philox;      /* a generator: manual_seed(seed), get_offset() / set_offset(offset) */
typedef struct {
  uint64_t seed;
  uint64_t offset;                 /* the generator's offset before the draw: a multiple of 4 */
  int64_t numel;
  int32_t blocks;                  /* torch's grid for this draw (es_philox_blocks); 0 = derive it from the current device */
  float scale;                     /* the result is multiplied by it after any rounding (the scheduler's init_noise_sigma) */
  int32_t round_dtype;             /* ES_F32: none.  ES_F16 | ES_BF16: rounded to that type and widened again, as torch draws a
                                      half tensor (in float, then cast) */
  /* optional permutation, all four 0 = a plain linear write: the draw index runs over NCHW [N, C, HW] (N * C * HW == numel) and
   * the value lands at [n, p, c] of an [N, HW, Cstride] array (Cstride >= C; channels C .. Cstride - 1 are left untouched) */
  int64_t N, C, HW, Cstride;
} es_randn_desc;
/* host-only: one Philox4x32-10 block */
int es_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* block_cap of a device (needs a GPU; -2 without one) */
int es_philox_block_cap(int device);
/* host-only: min(block_cap, ceil(numel / 256)) */
int es_philox_blocks(int64_t numel, int block_cap);
/* host-only: by how much a draw of numel elements on `blocks` blocks advances the generator's offset */
int64_t es_philox_advance(int64_t numel, int blocks);
/* out: device fp32, numel elements (or the [N, HW, Cstride] array of the permutation).  Asynchronous on `stream`, nothing is
 * allocated: capturable.  Bit-equal to torch.randn on the same device for the same (seed, offset). */
int es_randn(float* out, const es_randn_desc* d, void* stream);
/* the same draw on the CPU (out: host memory; `blocks` must be given).  Integer layer, layout, rounding and scatter are the
 * kernel's own code; the float step uses the host's libm and no fused multiply-add, so values agree with the device's to a few
 * ulp, not bit for bit. */
int es_randn_host(float* out, const es_randn_desc* d);
/* == prepare_latents (model/edgestyle_pipeline.py: randn_tensor(shape, generator) * init_noise_sigma): fills latents_out, device
 * fp32 [B,h,w,L] - the layout es_denoise_loop takes.  n_gens == 1: one draw of [B,L,h,w]; n_gens == B: one draw of [1,L,h,w] per
 * image from its own generator (the reference's list of generators).  Every gens[i] is advanced in place.  Capturable. */
int es_ctx_draw_latents(es_ctx* c, es_philox* gens, int n_gens, float sigma, int round_dtype, float* latents_out, void* stream);
/* == latent_dist.sample() of the VAE-conditioned nets (model/controllora.py:39, the device's default generator): fills every bound
 * ES_BUF_COND_NOISE* slot, in net order, each with one draw of [N,L,h,w]; `gen` is advanced after each draw.  es_prepare_conds /
 * es_prepare_conds_u8 called afterwards with a NULL noise pointer for such a net keep what the slot holds. */
int es_ctx_draw_cond_noise(es_ctx* c, es_philox* gen, int round_dtype, void* stream);

/* =========================================================================================================
 * Text encoder (csrc/text.hip): token ids in, the text states `ehs` of es_denoise_step / es_denoise_loop out - CLIPTextModel's
 * last_hidden_state, which the reference computes per request with transformers (app.py:163-176: the prompt and the negative
 * prompt; model/edgestyle_pipeline.py encode_prompt).  The ids come from es_tokenize_padded or es_prompt_assemble (below), or from
 * any CLIP BPE tokenizer the caller links.
 * A self-contained object beside es_ctx: it owns one arena (fp32 embedding tables, packed weights, activations for max_n prompts)
 * and runs on the library's own kernels - es_conv_gemm through the launch policy (es_launch_choose; LayerNorm1 / LayerNorm2 folded
 * into q|k|v and fc1, residual adds in the epilogues of out_proj and fc2), the two kernels below and es_layer_norm.
 * None of these calls is ever part of a plan: while a plan records on the calling thread they return -1.  No new
 * ES_ABI_VERSION: no plan or context image records them.
 * ========================================================================================================= */
/* Causal self-attention O[n, i, h] = softmax over j <= i of (Q_i . K_j * scale) V_j, same descriptor as es_attention.  Scope: Sq == Skv
 * in 1..128 (all keys of a head stay on chip: no online softmax), head_dim 32 | 64, fp16 | bf16 with fp32 accumulation, any row and
 * batch strides that are multiples of 8 elements (Q, K, V may be column slices of one fused [M, 3C] projection output).  The mask is
 * applied before the row maximum and the row sum; masked probabilities are exactly 0.  Anything else is refused before a launch. */
int es_attention_causal(const es_attn_desc* d, void* stream);
/* out[r, :] = round_dtype(tok[ids[r], :] + pos[r % S, :]): ids device int32 [rows] (clamped to [0, vocab) by the kernel), tok fp32
 * [vocab, hidden], pos fp32 [S, hidden] (nn.Embedding stays fp32 under autocast), summed in fp32, rounded once; out dtype [rows, hidden];
 * hidden a multiple of 8. */
int es_text_embed(const int32_t* ids, const float* tok, const float* pos, void* out, int rows, int S, int hidden, int vocab, int dtype,
                  void* stream);
typedef struct {                   /* config.json of a text_encoder/ directory (CLIPTextConfig) */
  int32_t vocab_size, hidden, heads, layers, intermediate, max_positions;
  float ln_eps;
  int32_t act;                     /* 0 = quick_gelu (SD1.5's CLIP ViT-L/14); anything else is refused */
} es_text_config;
typedef struct es_text_encoder es_text_encoder;
/* sd: CLIPTextModel's state dict as es_tensor descriptors (host or device memory, ES_F32 | ES_F16 | ES_BF16), keys
 * embeddings.{token,position}_embedding.weight, encoder.layers.{i}.{layer_norm1,layer_norm2}.{weight,bias},
 * encoder.layers.{i}.self_attn.{q,k,v,out}_proj.{weight,bias}, encoder.layers.{i}.mlp.{fc1,fc2}.{weight,bias},
 * final_layer_norm.{weight,bias} - bare, as transformers 5 spells them, or with the `text_model.` prefix of the SD1.5 checkpoints
 * (test_text2image_pretrained_openpose.py:224-232).  Other keys are ignored; a missing key or a wrong shape is an error naming the key.
 * quick_gelu rides on the SiLU epilogue: fc1 is packed as 1.702 W, 1.702 b and launched with ES_ACT_SILU and out_scale 1 / 1.702.
 * Refused: hidden % 64 != 0 or above 4096, hidden / heads not 32 | 64, max_positions > 128, intermediate % 64 != 0, act != 0.
 * device -1: dry build - everything but the allocation and the upload; es_text_encoder_arena_bytes reports the size and
 * es_text_encode returns an error that says so. */
int es_text_encoder_create(const es_state_dict* sd, const es_text_config* cfg, int dtype, int max_n, int device, es_text_encoder** out);
void es_text_encoder_destroy(es_text_encoder* e);
size_t es_text_encoder_arena_bytes(const es_text_encoder* e);
/* ids_host: HOST int32 [n, max_positions], n <= max_n, every id in [0, vocab_size) (else -1 naming the position); rows in the order of
 * the `ehs` operand - under CFG the negative prompts first, then the prompts.  out_ehs: device dtype [n, max_positions, hidden].
 * The ids are staged through pinned memory: a capturing stream is refused, as es_denoise_step refuses it.  Asynchronous on `stream`. */
int es_text_encode(es_text_encoder* e, const int32_t* ids_host, int n, void* out_ehs, void* stream);
/* es_text_encode with the ids already on the device (ids_dev: DEVICE int32 [n, max_positions], for instance es_prompt_assemble's
 * output): no pinned staging, nothing allocated, so a capturing stream is accepted.  Everything after the id copy is es_text_encode's
 * own code: the same ids give the same bits.  The ids cannot be checked on the host; the embedding kernel clamps them to
 * [0, vocab_size). */
int es_text_encode_dev(es_text_encoder* e, const int32_t* ids_dev, int n, void* out_ehs, void* stream);

/* =========================================================================================================
 * CLIP prompt picker (csrc/clip.hip): garment bytes in, the best words of the caller's vocabularies out.  Replaces BestEmbeddings
 * (model/utils.py:647-684), which the reference's try_on runs inside every request (app.py:161-165): CLIPProcessor (bicubic resize,
 * centre crop, normalise), CLIPModel's image tower, its text tower over the colour and garment words, logits_per_image, softmax and the
 * two best words of each list.  The word side is computed ONCE per vocabulary into an es_clip_bank; a request is es_clip_pick.
 * The transformer layers are the text encoder's (csrc/encoder.h) without the causal mask: es_conv_gemm through the launch policy with
 * LayerNorm1 / LayerNorm2 folded into q|k|v and fc1, es_attention over Q, K, V as column slices of the [M, 3C] projection, residual adds
 * in the epilogues of out_proj and fc2, quick_gelu on the SiLU epilogue.  The words reach es_clip_text_pool as token ids: the
 * caller's tokenizer, or es_tokenize_padded (below), whose eos_pos_out is the position es_clip_text_pool asks for.
 * None of these calls is ever part of a plan: while a plan records on the calling thread they return -1.  No new
 * ES_ABI_VERSION: no plan or context image records them.
 * ========================================================================================================= */
/* CLIPImageProcessor's rescale + normalize and the unfold of the patch convolution (CLIPVisionEmbeddings.patch_embedding, a Conv2d with
 * kernel = stride = p): in device uint8 HWC [n, R, R, 3] -> out_rows dtype [n * (R/p)^2, Kpad], Kpad = roundup(3 p^2, 64), row = (image, patch
 * row, patch column), column = c * p^2 + ky * p + kx - the order of the flattened weight [hidden, 3, p, p]; columns 3 p^2 .. Kpad - 1 are
 * WRITTEN as zero (the GEMM multiplies them).  Value: ((b / 255) - mean[c]) / std[c] in fp32, both divisions correctly rounded, rounded
 * once to dtype.  out_nchw (may be NULL): the same fp32 values before that rounding as [n, 3, R, R], the processor's pixel_values.
 * out_rows may be NULL when out_nchw is given.  mean / std: host float[3]. */
int es_clip_patchify(const uint8_t* in, void* out_rows, float* out_nchw, int n, int R, int p, const float* mean, const float* std, int dtype,
                     void* stream);
/* CLIPVisionEmbeddings' class token + position embedding and CLIPVisionTransformer.pre_layrnorm (transformers spells it so) in one launch:
 * patch dtype [n * P, hidden] (the patch GEMM's output), cls fp32 [hidden], pos fp32 [1 + P, hidden]; x[n, 0] = cls + pos[0],
 * x[n, 1 + j] = patch[n, j] + pos[1 + j], summed in fp32 and rounded once to dtype; out[n, t] = LayerNorm(x[n, t]) (two-pass statistics
 * in fp32 over the rounded row, gamma / beta fp32), rounded once; out dtype [n, 1 + P, hidden].  hidden a multiple of 8, at most 4096. */
int es_clip_embed(const void* patch, const float* cls, const float* pos, const float* gamma, const float* beta, void* out, int n, int P,
                  int hidden, float eps, int dtype, void* stream);
/* logits_per_image, its softmax per vocabulary and the best words (model/utils.py:666-684): pooled [n, proj] in pooled_dtype (ES_F16 |
 * ES_BF16 | ES_F32: the projection GEMM's output), bank fp32 [W, proj] of unit rows, logit_scale_exp = exp(logit_scale); seg_ends: HOST
 * int32[nseg], increasing, the last == W - the vocabularies bank rows [seg_ends[s - 1], seg_ends[s]) (nseg <= 4).  Per image: the
 * embedding is L2-normalised in fp32; logits[n, W] = logit_scale_exp * <e, bank[w]>; probs[n, W] = softmax inside each segment;
 * topk[n, nseg, k] (int32, k <= 8) = segment-relative indices by descending logit, equal logits resolving to the lower index; entries
 * past the end of a segment shorter than k are -1.  fp32 throughout.  logits / probs / topk: device, any may be NULL.  proj % 4 == 0, proj <= 4096, W <= 4096. */
int es_clip_score(const void* pooled, int pooled_dtype, const float* bank, int n, int W, int proj, float logit_scale_exp,
                  const int32_t* seg_ends, int nseg, int k, float* logits, float* probs, int32_t* topk, void* stream);
/* es_clip_bank: a device array of up to `capacity` fp32 unit rows [proj] - the normalised text_embeds of the caller's words.  Rows come
 * from the host as raw fp32 (es_clip_bank_append: copied, then L2-normalised by the row-norm code es_clip_score runs on its embeddings),
 * or from the text side (es_clip_text_pool below; text_sd then holds `text_projection.weight` [proj, text_hidden], packed at create time;
 * text_sd NULL: a bank of raw rows only).  max_n: the most rows one es_clip_text_pool call appends.  dtype: the compute dtype of that
 * projection.  device -1 is refused: a bank is device memory. */
typedef struct es_clip_bank es_clip_bank;
int es_clip_bank_create(const es_state_dict* text_sd, int text_hidden, int proj, int capacity, int max_n, int dtype, int device,
                        es_clip_bank** out);
void es_clip_bank_destroy(es_clip_bank* b);
int es_clip_bank_rows(const es_clip_bank* b);                 /* rows appended so far */
const float* es_clip_bank_data(const es_clip_bank* b);        /* device fp32 [capacity, proj] (borrowed) */
int es_clip_bank_append(es_clip_bank* b, const float* rows_host, int count, void* stream);
/* CLIPModel.get_text_features behind es_text_encode: ehs device dtype [n, S, text_hidden] (an es_text_encoder's output, final_layer_norm
 * applied), eos_pos HOST int32[n] - the pooled position of every row as transformers picks it (the argmax of the ids where the config has
 * the legacy eos_token_id == 2, else the first occurrence of eos_token_id; the caller computes it).  Gathers those rows, applies
 * text_projection (no bias), L2-normalises in fp32 and appends n rows to the bank.  Once per vocabulary, not per request. */
int es_clip_text_pool(es_clip_bank* b, const void* ehs, const int32_t* eos_pos, int n, int S, void* stream);
typedef struct {                   /* vision_config of a CLIPModel's config.json + its preprocessor_config.json */
  int32_t image_size, patch_size, hidden, heads, layers, intermediate, projection_dim;
  float ln_eps;
  int32_t act;                     /* 0 = quick_gelu; anything else is refused */
  float image_mean[3], image_std[3];
} es_clip_vision_config;
typedef struct es_clip_vision es_clip_vision;
/* sd: CLIPModel's state dict as es_tensor descriptors, keys vision_model.embeddings.{class_embedding, patch_embedding.weight,
 * position_embedding.weight}, vision_model.pre_layrnorm.{weight,bias}, vision_model.encoder.layers.{i}.* (the text tower's names),
 * vision_model.post_layernorm.{weight,bias}, visual_projection.weight - or the vision_model.* ones without that prefix, as a bare
 * CLIPVisionModel spells them.  Other keys are ignored; a missing key or a wrong shape is an error naming the key.
 * Forward (es_clip_vision_encode): es_clip_patchify -> patch embedding (es_conv_gemm, ksize 1, K = Kpad, no bias) -> es_clip_embed -> the
 * layers -> class-token rows (es_memcpy2d) -> es_layer_norm (post_layernorm) -> visual_projection (no bias) -> pooled dtype [n, proj].
 * Refused: hidden % 64 != 0 or above 4096, hidden / heads not 32 | 64, image_size % patch_size != 0, more than 1025 tokens,
 * intermediate % 64 != 0, act != 0.  device -1: dry build - es_clip_vision_arena_bytes reports the size, es_clip_vision_encode and
 * es_clip_pick return an error that says so. */
int es_clip_vision_create(const es_state_dict* sd, const es_clip_vision_config* cfg, int dtype, int max_n, int device, es_clip_vision** out);
void es_clip_vision_destroy(es_clip_vision* e);
size_t es_clip_vision_arena_bytes(const es_clip_vision* e);
/* images: device uint8 HWC [n, image_size, image_size, 3], n <= max_n; out_pooled: device dtype [n, projection_dim] (image_embeds before
 * the normalisation).  Asynchronous on `stream`, nothing is allocated or staged: capturable. */
int es_clip_vision_encode(es_clip_vision* e, const uint8_t* images, int n, void* out_pooled, void* stream);
/* The request call: imgs HOST array of `count` <= max_n garment photos (device memory, any size) -> es_image_resize_u8_ex(ES_FILTER_BICUBIC,
 * ES_CROP_TRANSFORMERS) -> es_clip_vision_encode -> es_clip_score against the bank's rows; the outputs are es_clip_score's.  workspace:
 * es_clip_pick_workspace_bytes(e, imgs, count) bytes of device memory (0 with es_last_error() set on bad arguments).  Asynchronous on
 * `stream`; nothing is allocated inside. */
size_t es_clip_pick_workspace_bytes(const es_clip_vision* e, const es_image_u8* imgs, int count);
int es_clip_pick(es_clip_vision* e, const es_clip_bank* bank, const es_image_u8* imgs, int count, float logit_scale_exp,
                 const int32_t* seg_ends, int nseg, int k, float* logits, float* probs, int32_t* topk, void* workspace,
                 size_t workspace_bytes, void* stream);

/* =========================================================================================================
 * Tokenizer and prompt assembly (csrc/bpe.h, csrc/prompt.hip): the link between es_clip_pick and es_text_encode.  The reference joins
 * the picked words into "edgestyle, c1, c2, i1, i2" + " " + suffix on the host (model/utils.py:661, app.py:165) and runs transformers'
 * CLIPTokenizer over it; here the tokenizer is in the library, and the picker's topk becomes the id row on the device.
 * The tokenizer is CLIP's byte-level BPE as transformers' CLIPTokenizer (the `tokenizers` backend) computes it: NFC, white space runs
 * to one space, lowercase; split by 's|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+; BPE with the end-of-word suffix </w>;
 * unk = pad = eos = <|endoftext|> (a symbol missing from the vocabulary is one unk id); BOS ... EOS, truncation keeps the EOS in the
 * last slot, padding is EOS.  Domain: exact or refused.  Accepted bytes are 0x09-0x0D and 0x20-0x7E; any other byte (non-ASCII
 * needs Unicode tables the library does not ship; NUL: the text is pointer + length and is never cut) is refused with its offset in
 * es_last_error(), and so is a text that holds the literal <|startoftext|> or <|endoftext|> in any letter case.
 * An es_tokenizer caches the ids of the words it has seen and is NOT thread-safe: one per thread, or a lock around it.
 * None of the es_prompt_* calls nor es_text_encode_dev is ever part of a plan: while a plan records on the calling thread they
 * return -1.  No new ES_ABI_VERSION: no plan or context image records them.
 * ========================================================================================================= */
typedef struct es_tokenizer es_tokenizer;
/* vocab.json (one flat JSON object token -> id; keys in raw UTF-8 or with \uXXXX escapes) and merges.txt ("left right" per line, lines
 * starting with #version skipped) of a CLIPTokenizer directory.  max_length: the row length of es_tokenize_padded (77 for SD1.5).
 * An error names the line or key: a merge whose parts or result are not in the vocabulary, a missing special token, max_length < 2. */
int es_tokenizer_create(const char* vocab_json_path, const char* merges_txt_path, int max_length, es_tokenizer** out);
int es_tokenizer_create_from_memory(const char* vocab_json, size_t vocab_bytes, const char* merges_txt, size_t merges_bytes,
                                    int max_length, es_tokenizer** out);
void es_tokenizer_destroy(es_tokenizer* t);
int es_tokenizer_vocab_size(const es_tokenizer* t);
int es_tokenizer_max_length(const es_tokenizer* t);
int es_tokenizer_bos_id(const es_tokenizer* t);
int es_tokenizer_eos_id(const es_tokenizer* t);
int es_tokenizer_pad_id(const es_tokenizer* t);            /* == eos */
/* text[0 .. len) -> its ids without BOS / EOS, untruncated.  Returns their count (the first min(count, capacity) are written to
 * ids_out; ids_out may be NULL with capacity 0 to ask for the count), or -1 for a refused text. */
int es_tokenize(es_tokenizer* t, const char* text, size_t len, int32_t* ids_out, int capacity);
/* the row of tokenizer(text, padding="max_length", max_length=max_length, truncation=True): ids_out HOST int32 [max_length];
 * eos_pos_out (may be NULL): the position of the row's first EOS - what es_clip_text_pool asks its caller for.  0, or -1. */
int es_tokenize_padded(es_tokenizer* t, const char* text, size_t len, int32_t* ids_out, int32_t* eos_pos_out);
/* Every word of the picker's vocabularies (words[n_words], NUL-terminated; seg_ends / nseg as es_clip_score takes them, the last ==
 * n_words) and the three fixed pieces (NULL = empty), tokenised once and uploaded to `device`: tokens[W, Lw], len[W], the fixed ids,
 * bos, eos and the tokenizer's max_length.  device -1: a table in host memory alone, for es_prompt_assemble_host. */
typedef struct es_prompt_table es_prompt_table;
int es_prompt_table_create(es_tokenizer* tok, const char* const* words, int n_words, const int32_t* seg_ends, int nseg,
                           const char* prefix, const char* separator, const char* suffix, int device, es_prompt_table** out);
void es_prompt_table_destroy(es_prompt_table* t);
/* topk_dev: DEVICE int32 [n, nseg, k] (es_clip_pick's topk, k <= 8) -> ids_out_dev: DEVICE int32 [n, max_length]; eos_pos_dev: DEVICE
 * int32 [n], may be NULL.  Row = BOS, prefix, then for every segment and every j < k in topk order: separator, word; then suffix; cut
 * to max_length - 2 ids, then EOS, then EOS padding; eos_pos = 1 + min(total, max_length - 2).  A topk entry outside [0, segment
 * size) - es_clip_score's -1 is one - is skipped and never used as an index.  The row equals the tokenizer's row of the pieces joined
 * by single spaces (a piece boundary is always a split boundary); the reference's comma-joined string gives the same ids as long as
 * no piece ends with punctuation, which would run into the comma ("t-shirt!, x" and "t-shirt! , x" differ).  One wave per row, plain stores, nothing
 * allocated or staged: capturable. */
int es_prompt_assemble(const es_prompt_table* t, const int32_t* topk_dev, int n, int k, int32_t* ids_out_dev, int32_t* eos_pos_dev,
                       void* stream);
/* the same rows from HOST topk into HOST memory, by the kernel's own index code */
int es_prompt_assemble_host(const es_prompt_table* t, const int32_t* topk, int n, int k, int32_t* ids_out, int32_t* eos_pos);

/* =========================================================================================================
 * Mask post-processing (csrc/mask.hip): the arithmetic the reference runs between a segmenter's mask predictions and the images
 * try_on takes (extract_dataset.py:316-351 and :394-502, composed differently in inference.py:322-447), restated.  All of it is
 * integer-exact.  Masks are DEVICE uint8 [count, H, W]: nonzero reads as true, outputs are exactly 0 or 1.  H and W are each in
 * 1..4096 (no alignment asked), count in 1..4096.  Inside the library a mask is bit-packed, 64 pixels per word.
 *   Morphology: dilate by r = OR over the (2r+1)^2 window CLIPPED to the image, erode by r = AND over the clipped window; pixels
 *   outside the image never contribute.  That is cv2.dilate / cv2.erode with their default border, with a full k x k kernel and
 *   `iterations` = n at r = n(k-1)/2 (cv2 itself enlarges the kernel and runs once), and skimage's closing(x, square(k)) =
 *   erode(dilate(x)) at r = (k-1)/2.  smooth_mask(kernel_size 3, iterations 3) is the chain {+3, -3, -3, +3}.
 *   Largest component: 8-connectivity (skimage.measure.label's default in 2-D), area = pixel count, a tie goes to the component
 *   whose first pixel in row-major order comes first (the reference keeps `region.area > largest_area` over regions in label order).
 *   A mask with no true pixel gives an ALL-TRUE result: the reference then compares labeled_array == 0.  Restated, not repaired.
 * Integer atomics only: a result does not depend on the order of execution.  The number of launches depends on the arguments
 * alone, never on the pixels; nothing is allocated or read back: every call is capturable.  Like the byte-image calls none of
 * these is part of a plan (-1 while one records on the thread), so ES_ABI_VERSION stays as it is.
 * ========================================================================================================= */
/* host-only: bytes of device scratch that every call below needs at most for `count` masks of H x W (es_sam_compose's need: ten
 * packed masks and two int32 [H, W] arrays per image); 0 with es_last_error() set on bad arguments.  The workspace must be
 * 8-byte aligned. */
size_t es_mask_workspace_bytes(int H, int W, int count);
/* radii: HOST int32 [n], n <= 16, applied in order: r > 0 dilates by r, r < 0 erodes by -r, 0 does nothing; |r| <= 15.
 * in and out may be the same pointer.  One launch per nonzero radius, plus the packing and the unpacking. */
int es_mask_morph(const uint8_t* in, uint8_t* out, int count, int H, int W, const int32_t* radii, int n, void* ws, size_t ws_bytes,
                  void* stream);
/* out = the largest 8-connected component of each mask (all true for a mask without a true pixel, see above); area_out: DEVICE
 * int32 [count] or NULL, the winner's pixel count (0 for a mask without a true pixel).  in and out may be the same pointer.
 * Union-find on an int32 [H, W] array whose links always point to a smaller linear index: the root of a component is its first
 * pixel in row-major order. */
int es_mask_largest_component(const uint8_t* in, uint8_t* out, int32_t* area_out, int count, int H, int W, void* ws, size_t ws_bytes,
                              void* stream);
enum { ES_MASK_AND = 0, ES_MASK_OR = 1, ES_MASK_ANDNOT = 2 };      /* a & b, a | b, a & ~b */
/* out[i] = a[i] op b[i] over n bytes read as booleans; out may be a or b */
int es_mask_logic(const uint8_t* a, const uint8_t* b, uint8_t* out, int64_t n, int op, void* stream);
/* draw_binary_mask: out_hwc3 [count, H, W, 3] keeps the pixels of img[i] (H x W; a fourth channel is ignored and the row stride
 * honoured, as in the byte-image calls) where mask [count, H, W] is true and is `colour` elsewhere.  img_or_null: HOST array of
 * `count` descriptors, or NULL for images of zeros. */
int es_image_mask_fill_u8(const es_image_u8* img_or_null, const uint8_t* mask, uint8_t* out_hwc3, int count, int H, int W,
                          const uint8_t colour[3], void* stream);
/* create_sam_images (app.py:125-149 -> extract_dataset.py:394-502) after the networks: with sm = {+3, -3, -3, +3} and cK =
 * closing(square(K)) = {+(K-1)/2, -(K-1)/2},
 *   S = sm(c3(subject))  A = sm(c3(body))  C = sm(c3(clothes))  Hd = sm(c7(head))  ALL = sm(largest(S | C | Hd))
 *   agnostic = A & ~(A & C) & ALL   clothes_m = C & ~(A & C) & ALL   head_m = Hd & ALL
 * imgs: HOST array of `count` descriptors of H x W photos; subject / body / clothes / head: [count, H, W] each.
 * masks_out [count, 4, H, W]: ALL, agnostic, clothes_m, head_m.  images_out [count, 5, H, W, 3]: the photo where ALL holds and grey
 * 127 elsewhere; the reference's `mask` (black where agnostic holds, white 255 elsewhere); the photo under agnostic,
 * under clothes_m and under head_m on grey 127.  Either output may be NULL (not both).  The score test, getBox and which image goes
 * to which slot stay with the caller. */
int es_sam_compose(const es_image_u8* imgs, const uint8_t* subject, const uint8_t* body, const uint8_t* clothes, const uint8_t* head,
                   int count, int H, int W, uint8_t* masks_out, uint8_t* images_out, void* ws, size_t ws_bytes, void* stream);


/* =========================================================================================================
 * EfficientViT-SAM image encoder (csrc/sam.hip; the preprocessing in csrc/image_io.hip): photo bytes -> the image embedding the SAM mask
 * decoder (next section) takes.  Replaces the reference's EfficientViTSamImageEncoder forward (efficientvit/models/efficientvit/sam.py:174-190:
 * EfficientViTLargeBackbone -> SamNeck -> LayerNorm2d) and EfficientViTSam.transform (sam.py:211-221) that EfficientViTSamPredictor.set_image
 * (sam.py:274-293) runs per photo and per predictor (extract_dataset.py:371-425: five predictors whose fine-tuned models share ONE frozen
 * image encoder - one embedding per photo serves all five decoders). 
 * Like the text and CLIP objects none of these calls is ever part of a plan (-1 while one records on the thread), so ES_ABI_VERSION stays.
 * All tensors are DEVICE memory, NHWC in the storage dtype (ES_F16 | ES_BF16) unless stated otherwise.
 * ========================================================================================================= */
/* Depthwise convolution with "same" padding (k / 2): out[n, oy, ox, c] = act(sum_{ky, kx} x[n, oy s + ky - k/2, ox s + kx - k/2, c] w[ky k + kx, c] + bias[c]),
 * fp32 accumulation in tap order, one rounding.  x [N, H, W, C], w [k * k, C] (dtype), bias fp32 [C] or NULL, out [N, Ho, Wo, C] with
 * Ho = (H + 2 (k / 2) - k) / s + 1.  k = 3 with stride 1 | 2, k = 5 with stride 1; C a multiple of 8; act ES_ACT_NONE | ES_ACT_GELU_TANH.
 * Pointers 16-byte aligned.  A result does not depend on N or on how the launch is cut. */
int es_dwconv(const void* x, const void* w, const float* bias, void* out, int N, int H, int W, int C, int k, int stride, int act, int dtype,
              void* stream);
/* LiteMLA.relu_linear_att (efficientvit/models/nn/ops.py:397-434) over the concatenation [qkv ; aggreg(qkv)], which is never written:
 * a, b [N, HW, 3 * heads * 32] are its two halves (groups 0 .. heads - 1 read a, groups heads .. 2 heads - 1 read b; a group is 96 channels:
 * q, k, v of 32), out [N, HW, 2 * heads * 32], channel g * 32 + d.  Per (n, g), all in fp32: kv = relu(k)^T [v | 1] over the tokens in order,
 * o = relu(q) kv, out = o[:32] / (o[32] + 1e-15), one rounding.  A group whose relu(k) or relu(q) is all zero gives exactly 0.
 * HW >= 1 (no multiple of anything), heads in 1..1024. */
int es_relu_linear_attention(const void* a, const void* b, void* out, int N, int HW, int heads, int dtype, void* stream);
/* SamNeck's merge: out [N, 64, 64, C] = m0 + (m1 + m2) (list_sum's order; fp32, one rounding), each map [N, h_i, w_i, C] resampled to 64 x 64
 * with torch's bicubic (A = -0.75, align_corners = False, indices clamped at the border) in fp32; a map that already is 64 x 64 is read as
 * it is.  count in 1..3 maps, C a multiple of 8, h_i, w_i in 1..64. */
int es_sam_neck_merge(const void* const* maps, const int32_t* hs, const int32_t* ws, int count, void* out, int N, int C, int dtype, void* stream);
/* EfficientViTSam.transform.  Per image (HOST descriptors, device bytes, any size, 3 or 4 channels of which 3 are read): resized so that the
 * long side is S with Pillow's antialiased bilinear filter (target sizes int(x * S / long + 0.5); no resize when the long side is S),
 * x / 255, (x - mean) / std in fp32 (both divisions correctly rounded), placed at the top left of an S x S canvas whose remainder is
 * exactly 0.0.  Outputs, each optional: out_nhwc [count, S, S, 8] in `dtype` (channels 3..7 zero: the stem's input), out_nchw fp32
 * [count, 3, S, S] (the reference's tensor), out_u8 [count, S, S, 3] (the resized bytes, 0 outside them).  input_hw: HOST [count, 2] or
 * NULL, the resized (h, w) - the input_size postprocess_masks needs; es_sam_resize_shape is the same rule, host-only. */
void es_sam_resize_shape(int height, int width, int S, int32_t out_hw[2]);
size_t es_sam_preprocess_u8_workspace_bytes(const es_image_u8* imgs, int count, int S);
int es_sam_preprocess_u8(const es_image_u8* imgs, int count, int S, const float mean[3], const float std[3], int dtype, void* out_nhwc,
                         float* out_nchw, uint8_t* out_u8, int32_t* input_hw, void* workspace, size_t workspace_bytes, void* stream);
typedef struct { int32_t image_size, width[5], depth[5], qkv_dim, head_width, head_depth, out_dim;
                 float bn_eps, ln_eps, pixel_mean[3], pixel_std[3]; } es_sam_config;
typedef struct es_sam_encoder es_sam_encoder;
/* sd: the reference's state_dict() names, bare (backbone.*, neck.*, norm.*) or with the `image_encoder.` prefix of an EfficientViTSam
 * checkpoint; unknown keys (num_batches_tracked) are ignored, a missing key or a wrong shape is an error that names the key.  Whether a
 * ConvLayer has a bias and / or a BatchNorm is read from which keys exist.  BatchNorm (eval form) is folded into its convolution in fp64 and
 * rounded once; one arena holds the packed weights, the activations of max_n images and the split-K workspace.  device -1: a dry build
 * that reports the arena size.  Scope: widths multiples of 32, qkv_dim 32, head_width and out_dim multiples of 8, image_size a multiple of
 * 32 in [64, 512] (the neck's 64 x 64 output is hard-wired in the reference, sam.py:127), max_n >= 1. */
int es_sam_encoder_create(const es_state_dict* sd, const es_sam_config* cfg, int dtype, int max_n, int device, es_sam_encoder** out);
void es_sam_encoder_destroy(es_sam_encoder* e);
size_t es_sam_encoder_arena_bytes(const es_sam_encoder* e);
/* x_nchw fp32 [n, 3, S, S], already normalised and padded (the reference's tensor) -> out_nchw fp32 [n, out_dim, 64, 64].  Nothing is
 * allocated or staged: a capturing stream is accepted.  Image i of a batch equals the same image encoded alone bit for bit. */
int es_sam_encode(es_sam_encoder* e, const float* x_nchw, int n, float* out_nchw, void* stream);
/* the backbone's stage2 | stage3 | stage4 map of the last encode as fp32 NCHW [n, width[stage], S / 2^(stage+1), ...] (what the neck read) */
int es_sam_encoder_stage(es_sam_encoder* e, int stage, int n, float* out_nchw, void* stream);
size_t es_sam_encode_u8_workspace_bytes(const es_sam_encoder* e, const es_image_u8* imgs, int count);
/* es_sam_preprocess_u8 + es_sam_encode: imgs HOST array, device bytes, any size; input_hw HOST [count, 2] or NULL */
int es_sam_encode_u8(es_sam_encoder* e, const es_image_u8* imgs, int count, float* out_nchw, int32_t* input_hw, void* workspace,
                     size_t workspace_bytes, void* stream);


/* =========================================================================================================
 * SAM prompt encoder and mask decoder, the pieces that are no big GEMM (csrc/sam_decoder.hip): the prompt tokens, the token-side linear
 * layers of the TwoWayTransformer, the fused upscaling tail, postprocess_masks and getBox of segment_anything 1.0's PromptEncoder / MaskDecoder as EfficientViT-SAM
 * builds them (efficientvit/models/efficientvit/sam.py:522-540) and as extract_dataset.py:371-429 chains them: a decode's mask gives the box
 * of the next decode without a host visit.  es_sam_decoder strings them together with es_conv_gemm, es_layer_norm,
 * es_add and es_attention: a C++ host needs only the person box and the pose key points from outside (the two detectors' results;
 * es_pose_points_host turns the key points into the point prompt, es_person_crop_u8 the box into the photo these calls take).
 * No float atomics, nothing allocated or read back (capturable), image i of a batch equals the image alone bit for bit; never part of a
 * plan (-1 while one records on the thread), so ES_ABI_VERSION stays.  The *_host twins run the kernels' own index and weight code on the CPU.
 * ========================================================================================================= */
typedef struct {
  /* weights, fp32: PromptEncoder.pe_layer.positional_encoding_gaussian_matrix [2, embed_dim / 2], point_embeddings.{0..3}.weight as
   * [4, embed_dim], not_a_point_embed.weight [embed_dim]; MaskDecoder.iou_token.weight [embed_dim], mask_tokens.weight [n_mask_tokens, embed_dim] */
  const float *gauss, *point_embeddings, *not_a_point, *iou_token, *mask_tokens;
  /* prompts of n images in ORIGINAL-image pixels: points fp32 [n, P, 2] (x, y), labels int32 [n, P] (1 foreground, 0 background, -1 not a
   * point), boxes fp32 [n, 4] (x0, y0, x1, y1; what es_mask_bbox writes) or NULL: no box.  P == 0: points and labels are not read. */
  const float* points;
  const int32_t* labels;
  const float* boxes;
  void* tokens;      /* out, dtype [n, 1 + n_mask_tokens + T, embed_dim], T = es_sam_prompt_token_count(P, boxes != NULL) */
  void* query_pe;    /* out or NULL: the same values once more (the decoder's query_pe is its token matrix) */
  int32_t n, P, embed_dim, n_mask_tokens;
  int32_t frame;     /* the prompt frame's long side (1024) */
  int32_t orig_h, orig_w, dtype;
} es_sam_prompt_desc;
/* sparse tokens of a prompt: P points, then the box's two corners, or ONE padding point where there are points and no box; -1 for P < 0 */
int es_sam_prompt_token_count(int P, int has_box);
/* tokens = [iou_token; mask_tokens; sparse].  Sparse token of a point c with label 0 | 1: pe(c) + point_embeddings[label]; label -1:
 * not_a_point alone; any other label: pe(c) alone, which is what segment_anything's _embed_points leaves for it (the labels are device
 * memory and cannot be refused on the host); a box corner k: pe(corner) + point_embeddings[2 + k]; the padding point: not_a_point.  Coordinates go through
 * apply_coords first (x * (new_w / orig_w) in double, rounded once to fp32, (new_h, new_w) = es_sam_resize_shape(orig_h, orig_w, frame)); then
 * pe(c) = [sin | cos](2 pi ((2 (c + 0.5) / frame - 1) @ gauss)) in fp32 with the precise sinf / cosf.  One rounding to dtype.  All pointers
 * DEVICE memory.  Refused: no prompt at all, more than 32 tokens, an odd embed_dim. */
int es_sam_prompt_tokens(const es_sam_prompt_desc* d, void* stream);
/* the same values in fp32 from HOST pointers into HOST memory [n, 1 + n_mask_tokens + T, embed_dim] (tokens, query_pe and dtype are not read) */
int es_sam_prompt_tokens_host(const es_sam_prompt_desc* d, float* tokens_f32);
typedef struct {
  const void* x;           /* dtype, row r of sample i at x + i * bsx + r * ldx (elements); 16-byte aligned */
  const void* w;           /* dtype [N, K] (nn.Linear's layout), or [rows, N, K] with per_row_weights; 16-byte aligned */
  const float* bias;       /* fp32 [N] ([rows, N] with per_row_weights) or NULL */
  const void* residual;    /* dtype or NULL, addressed like out with bsr / ldr */
  void* out;               /* dtype, row r of sample i at out + i * bso + r * ldo */
  int32_t n, rows, K, N;   /* rows in 1..32; K a multiple of 8 in 8..2048; N a multiple of 4 in 4..2048 */
  int32_t ldx, ldr, ldo;   /* 0: dense (K, N, N); ldx a multiple of 8 */
  int64_t bsx, bsr, bso;   /* 0: dense (rows * ld); bsx a multiple of 8 */
  int32_t per_row_weights; /* 1: row r has weights and a bias of its own (MaskDecoder.output_hypernetworks_mlps as one launch) */
  int32_t relu, dtype;
} es_linear_tokens_desc;
/* out[i, r, :] = act(x[i, r, :] W^T + b) (+ residual[i, r, :]): fp32 accumulation in an order that depends on K alone, bias, ReLU and the
 * residual in fp32, one rounding.  The weights are shared by all samples. */
int es_linear_tokens(const es_linear_tokens_desc* d, void* stream);
typedef struct {
  const void* g;            /* dtype [n, grid_h * grid_w, 4 * C1]: MaskDecoder.output_upscaling.0 (ConvTranspose2d k2 s2) as a 1x1 GEMM with its bias,
                             * column (2 dy + dx) * C1 + c; 16-byte aligned */
  const void* w_packed;     /* dtype, C1 * 2 * C1 elements: output_upscaling.3.weight through es_sam_upscale_pack; 16-byte aligned */
  const float *ln_gamma, *ln_beta;      /* fp32 [C1]: output_upscaling.1 (LayerNorm2d) */
  const float* bias2;       /* fp32 [C1 / 2]: output_upscaling.3.bias */
  const void* hyper;        /* dtype, row m of image i at hyper + i * bsh + m * ldh, C1 / 2 values: the hypernetwork MLPs' outputs */
  float* out;               /* fp32 [n, M, 4 * grid_h, 4 * grid_w] */
  int32_t n, grid_h, grid_w, C1, M;     /* C1 = embed_dim / 4 in {32, 64}; M in 1..4 */
  int32_t ldh;              /* 0: dense (C1 / 2) */
  int64_t bsh;              /* 0: dense (M * ldh) */
  float ln_eps;
  int32_t dtype;
} es_sam_upscale_desc;
/* host-only: w fp32 [C1, C1 / 2, 2, 2] (ConvTranspose2d's layout) -> the MFMA B fragments es_sam_upscale_masks loads, C1 * 2 * C1 elements of dtype */
int es_sam_upscale_pack(const float* w, int C1, int dtype, void* out);
/* The mask decoder's tail behind ConvT1, fused: per (source pixel, sub-pixel) LayerNorm over the C1 channels (two-pass, eps ln_eps), erf-GELU,
 * rounded once to dtype, ConvT2 on the matrix core (K = C1, N = 2 * 2 * C1 / 2), bias and erf-GELU in fp32, and the dot with hyper[m]:
 * out[i, m, 4 py + 2 dy + dy2, 4 px + 2 dx + dx2].  The [C1 / 2, 4 grid, 4 grid] tensor is never written.  Fixed summation order: a result
 * does not depend on n. */
int es_sam_upscale_masks(const es_sam_upscale_desc* d, void* stream);
/* ---- the decoder object: prompts + embedding -> low-res logits / masks, one arena, nothing allocated or read back in a call ---- */
typedef struct { int32_t embed_dim, heads, mlp_dim, depth, grid, frame, n_mask_tokens, iou_hidden, iou_depth, attn_downsample;
                 float ln_eps, ln2d_eps; } es_sam_decoder_config;        /* EfficientViT-SAM: 256, 8, 2048, 2, 64, 1024, 4, 256, 3, 2, 1e-5, 1e-6 */
typedef struct {
  const float* points;      /* DEVICE fp32 [n, P, 2] in original-image pixels, or NULL with P == 0 */
  const int32_t* labels;    /* DEVICE int32 [n, P]: 1 | 0 | -1 (any other label gets the positional encoding alone, as segment_anything does) */
  const float* boxes;       /* DEVICE fp32 [n, 4] or NULL (es_mask_bbox's output) */
  const void* mask_input;   /* must be NULL: refused (the reference never passes one) */
  int32_t P, orig_h, orig_w;
} es_sam_prompts;
typedef struct es_sam_decoder es_sam_decoder;
/* sd: segment_anything 1.0's names (prompt_encoder.*, mask_decoder.*), bare or under one prefix that ends in "prompt_encoder." / "mask_decoder."
 * being stripped (e.g. "sam."); prompt_encoder.mask_downscaling.* is ignored; a missing key or a wrong shape is an error that names the key.
 * device -1: a dry build that reports the arena size.  Refused with the reason before anything is launched: embed_dim not a multiple of 64
 * (and, narrower, not 128 | 256: es_sam_upscale_masks), head widths other than es_attention's, more than 32 tokens
 * (1 + n_mask_tokens + max_points + 2), grid outside 1..64.  The image-side GEMMs take the tile es_launch_choose gives for ONE image, so image i
 * of a batch equals the image alone bit for bit. */
int es_sam_decoder_create(const es_state_dict* sd, const es_sam_decoder_config* cfg, int dtype, int max_n, int max_points, int device,
                          es_sam_decoder** out);
void es_sam_decoder_destroy(es_sam_decoder* d);
size_t es_sam_decoder_arena_bytes(const es_sam_decoder* d);
/* emb_nchw DEVICE fp32 [n, embed_dim, grid, grid] -> low_res DEVICE fp32 [n, M, 4 grid, 4 grid], iou DEVICE fp32 [n, M]; M = n_mask_tokens - 1
 * with multimask (rows 1..), else 1 (row 0); only those rows are computed.  A capturing stream is accepted. */
int es_sam_decode(es_sam_decoder* d, const float* emb_nchw, const es_sam_prompts* prompts, int n, int multimask, float* low_res, float* iou,
                  void* stream);
/* es_sam_decode + es_sam_postprocess_masks at (orig_h, orig_w): masks DEVICE uint8 [n, M, H, W] and / or mask_logits fp32 [n, M, H, W]
 * (either may be NULL, not both); low_res may be NULL (the arena then holds it) */
int es_sam_predict(es_sam_decoder* d, const float* emb_nchw, const es_sam_prompts* prompts, int n, int multimask, float* low_res, float* iou,
                   uint8_t* masks, float* mask_logits, void* stream);
/* EfficientViTSam.postprocess_masks (sam.py:223-239) and the predictor's `> mask_threshold` (0): logits fp32 [count, L, L] -> bilinear
 * (align_corners=False) to S x S, cropped to [:new_h, :new_w], bilinear to H x W, in torch's fp32 index and weight arithmetic (scale = in /
 * out, source = scale (dst + 0.5) - 0.5 clamped at 0); the S x S canvas is never stored.  out_f32 [count, H, W] and out_u8 [count, H, W]
 * (1 where the value is > 0, else 0): either may be NULL, not both.  One (new_h, new_w, H, W) per call, as for es_sam_compose. */
int es_sam_postprocess_masks(const float* logits, int count, int L, int S, int new_h, int new_w, int H, int W, float* out_f32, uint8_t* out_u8,
                             void* stream);
int es_sam_postprocess_masks_host(const float* logits, int count, int L, int S, int new_h, int new_w, int H, int W, float* out_f32,
                                  uint8_t* out_u8);
/* getBox (extract_dataset.py:298-313) of masks uint8 [count, H, W]: boxes fp32 [count, 4] = {max(0, xmin - margin), max(0, ymin - margin),
 * min(W, xmax + margin), min(H, ymax + margin)} over the nonzero pixels, zeros for a mask without one.  Integer min / max atomics on the box
 * buffer itself (int32 between the three launches), so there is no workspace. */
int es_mask_bbox(const uint8_t* masks, float* boxes, int count, int H, int W, int margin, void* stream);
int es_mask_bbox_host(const uint8_t* masks, float* boxes, int count, int H, int W, int margin);


#ifdef __cplusplus
}
#endif
#endif

// What es_conv_gemm decides before it launches, shared by gemm_conv.hip (the route, the 128-pixel kernel) and gemm_conv8p.hip (the
// 256-pixel phase-interleaved kernel).  Private to the library; the public side is es_conv_gemm_route / es_conv_gemm_last_kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/edgestyle_hip.h"

// Every instantiation of the two kernels that exists, per dtype: the ONE table the route's lookup, the dispatch switches and the
// kernels' LDS bytes are written from.
//   conv_gemm_kernel<T, BM, BN, ALIGNED, STAGES, FM, LN, KO>  (gemm_conv.hip)                X(BM, BN, ALIGNED, STAGES, FM, LN, KO)
#define ES_GEMM_TABLE(X)                                                                                                          \
  /* LayerNorm-folded linear layers: 64-aligned by definition, tap-major K */                                                       \
  X(64, 64, 1, 4, 2, 1, 0)    X(64, 64, 1, 2, 2, 1, 0)                                                                              \
  X(128, 128, 1, 4, 2, 1, 0)  X(128, 128, 1, 2, 2, 1, 0)  X(128, 128, 1, 4, 4, 1, 0)  X(128, 128, 1, 2, 4, 1, 0)                    \
  X(128, 160, 1, 2, 2, 1, 0)  X(128, 160, 1, 4, 4, 1, 0)  X(128, 160, 1, 2, 4, 1, 0)                                                \
  /* the 64 x 64 tile: four waves of two pixel fragments, 4 | 2 stages, chunk-major | tap-major K */                                \
  X(64, 64, 1, 4, 2, 0, 1)    X(64, 64, 1, 4, 2, 0, 0)    X(64, 64, 1, 2, 2, 0, 1)    X(64, 64, 1, 2, 2, 0, 0)                      \
  /* 128 x 128: 8 waves with 4 | 2 stages, 4 waves with 2 | 3 | 4, and the one form for channels that are no multiples of 64 */     \
  X(128, 128, 1, 4, 2, 0, 1)  X(128, 128, 1, 4, 2, 0, 0)  X(128, 128, 1, 2, 2, 0, 1)  X(128, 128, 1, 2, 2, 0, 0)                    \
  X(128, 128, 1, 2, 4, 0, 1)  X(128, 128, 1, 2, 4, 0, 0)  X(128, 128, 1, 3, 4, 0, 1)  X(128, 128, 1, 3, 4, 0, 0)                    \
  X(128, 128, 1, 4, 4, 0, 1)  X(128, 128, 1, 4, 4, 0, 0)  X(128, 128, 0, 2, 4, 0, 0)                                                \
  /* 128 x 160: the same without the 8-wave 4-stage form */                                                                         \
  X(128, 160, 1, 2, 2, 0, 1)  X(128, 160, 1, 2, 2, 0, 0)  X(128, 160, 1, 2, 4, 0, 1)  X(128, 160, 1, 2, 4, 0, 0)                    \
  X(128, 160, 1, 3, 4, 0, 1)  X(128, 160, 1, 3, 4, 0, 0)  X(128, 160, 1, 4, 4, 0, 1)  X(128, 160, 1, 4, 4, 0, 0)                    \
  X(128, 160, 0, 2, 4, 0, 0)
//   conv_gemm8p_kernel<T, KO, 256, FN, LN, GEGLU>  (gemm_conv8p.hip; BN = 64 * FN, two stages, 8 waves)      X(KO, FN, LN, GEGLU)
#define ES_GEMM8P_TABLE(X)                                                                                                        \
  X(0, 4, 1, 1)  X(0, 4, 1, 0)  X(0, 4, 0, 1)  X(0, 4, 0, 0)                                                                        \
  X(1, 5, 0, 0)  X(0, 5, 0, 0)

// table rows by name: the 128-pixel kernel's first, then the 256-pixel kernel's (GemmRoute::row, ES_GEMM_ROUTE_ROW)
#define ES_GEMM_ROW(BM, BN, AL, ST, FM, LN, KO) GEMM_ROW_##BM##_##BN##_##AL##ST##FM##LN##KO
#define ES_GEMM8P_ROW(KO, FN, LN, GG) GEMM8P_ROW_##KO##FN##LN##GG
enum GemmRowId {
#define X(BM, BN, AL, ST, FM, LN, KO) ES_GEMM_ROW(BM, BN, AL, ST, FM, LN, KO),
  ES_GEMM_TABLE(X)
#undef X
#define X(KO, FN, LN, GG) ES_GEMM8P_ROW(KO, FN, LN, GG),
  ES_GEMM8P_TABLE(X)
#undef X
  GEMM_ROWS
};

// dynamic LDS of an instantiation: its ring of K-steps, 64 deep, two bytes per element
constexpr int gemm_lds(int BM, int BN, int ST) { return ST * (BM + BN) * 64 * 2; }
constexpr int gemm8p_lds(int FN) { return gemm_lds(256, 64 * FN, 2); }

// es_conv_gemm_last_kernel / GemmRoute::kernel: an instantiation's template arguments, packed (ES_GEMM_KERNEL_* of the header)
constexpr int gemm_kernel_id(int bm, int bn, int stages, int waves, bool aligned, bool ln, bool ko, bool geglu, bool is_bf16) {
  return bn | (bm / 64) << ES_GEMM_KERNEL_BM64_SHIFT | stages << ES_GEMM_KERNEL_STAGES_SHIFT | (waves == 8 ? ES_GEMM_KERNEL_WAVES8 : 0) |
         (aligned ? ES_GEMM_KERNEL_ALIGNED : 0) | (ln ? ES_GEMM_KERNEL_LN : 0) | (ko ? ES_GEMM_KERNEL_KO : 0) |
         (geglu ? ES_GEMM_KERNEL_GEGLU : 0) | (is_bf16 ? ES_GEMM_KERNEL_BF16 : 0);
}

enum { GEMM_REDUCE_NONE = ES_GEMM_REDUCE_NONE, GEMM_REDUCE_PLAIN = ES_GEMM_REDUCE_PLAIN, GEMM_REDUCE_GN = ES_GEMM_REDUCE_GN };

// Everything es_conv_gemm decides, as numbers
struct GemmRoute {
  int kernel;                      // gemm_kernel_id of the row
  int row;                         // GemmRowId
  int family;                      // 0: conv_gemm_kernel (128 | 64 pixels per workgroup), 1: conv_gemm8p_kernel (256)
  int bn, stages, waves;           // as they run: after the tile downgrade, stages 0 -> 2, waves 0 -> the row's
  int aligned;                     // channels in whole 64-deep K-steps
  int grid, threads, lds;
  int reduce, reduce_cb;           // split-K: GEMM_REDUCE_*, and the channels per workgroup of the GroupNorm hand-over
  int reduce_grid, reduce_threads;
  int runs;                        // launches the call is cut into (1 unless an operand outgrows the 32-bit buffer offsets) ...
  int samples_per_run;             // ... and samples per full run; the fields above then describe the first run
};

// which instantiation the last launch of this process went to (es_conv_gemm_last_kernel: tests assert the tile they mean to run); written
// by the launchers of both files from their OWN template arguments, never copied from the route
extern int es_gemm_last_kernel_v;

// gemm_conv8p.hip: launches row r.row (a GEMM8P_ROW_*) on r.grid workgroups; called by es_conv_gemm for r.family == 1
int es_conv_gemm8p_launch(const es_gemm_desc& d, const GemmRoute& r, hipStream_t st);

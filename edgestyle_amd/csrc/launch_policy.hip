// The launch policy: every decision between "this convolution / linear call is valid" and "its descriptor is filled" - kernel, tile,
// split-K, ring depth, waves, XCD order, GroupNorm hand-over, two-word stream, the slices of an es_linear_xs launch - and the values the
// knobs that bend them start from.  It exists ONCE, here: the Python host (edgestyle_amd/ops.py) asks through the C entries at the end of
// this file, the native builders (builder.hip, encoder.h) through launch_policy.h.  Host code only; no kernel lives in this file.
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/edgestyle_hip.h"
#include "launch_policy.h"

extern "C" void es_set_error(const char* msg);

namespace es_policy {

// ---- the launch planner (es_plan_gemm_choice; tests/numerics.py plan_gemm_reference restates it and tests/test_load_weights_cpu.py sweeps both) ----
#pragma clang fp contract(off)
// A launch is described by (bn, splitk, stages); its cost model is in units of one K-step of a 128-wide tile on a CU shared by two
// workgroups (~0.77 us) and was fitted on tools/gemm_tune.py sweeps over the shapes of a batch-1 denoising step (total within 1.1 % of the
// per-shape best configuration, 6.4 % below the previous tiles-vs-target rules):
//   * 512 workgroups are resident at once (256 CUs x 2); a launch takes ceil(WGs / 512) rounds of one workgroup's time;
//   * a 160-wide tile costs 1.25x a 128-wide one per K-step; a workgroup alone on its CU runs ~10 % faster;
//   * split-K pays a reduce launch (~12 units) plus the fp32 slab round trip, needs >= 12 K-steps per slice and is never worth it for
//     K <= 640.
constexpr double PLAN_T160 = 1.25, PLAN_ALONE = 0.9, PLAN_TFIX = 2.0, PLAN_RED_FIX = 12.0, PLAN_SLAB_BYTES_PER_UNIT = 4.0e6;
//   * the big tile (256 px x 320 couts, one workgroup per CU, gemm_conv8p.hip) does the work of two 160-wide workgroups in ~8 % less time
//     (half the L2->LDS bytes) and is charged FRACTIONAL rounds; 1.03-1.15x the 128-pixel tile on launches of >= 1 round of 256 workgroups
//     with K >= 1024 (tools/gemm8p_bench.py: 1.07-1.30 PFLOP/s on the batch-8 3x3 launches).  Since round 4 (lean epilogue) it is offered
//     from 2048 pixels up, where it wins as a split-K launch of ~256 workgroups (the 16 x 16 decoder level at batch 8: 1.3-1.5x,
//     tools/plan_fit_bench.py).
constexpr double PLAN_T320 = 2.3, PLAN_T320_FIX = 3.0;
// the 256 x 256 tile of the LayerNorm-folded / GEGLU linear layers against the 128-wide tile on the same layers (tools/ln256_bench.py, round 5)
constexpr double PLAN_T256 = 2.6, PLAN_T256_FIX = 6.0, PLAN_T256_GEGLU = 7.0, PLAN_LN_TK = 1.55, PLAN_T256_MARGIN = 0.93;
constexpr int PLAN_BIG_MIN_M = 2048, PLAN_BIG_MIN_NK = 16;
//   * the 64x64 tile (tiny launches): a K-step costs 0.5 units with the CU to itself and 0.5 + 0.16 (w - 1)^2 with w workgroups per CU
//     (measured 0.87 at w = 2.5, 2.0 at w = 3.75); x1.5 for K > 2560, where MFMA throughput starts to matter and the small tile reads LDS
//     twice as often per FLOP; 1024 resident workgroups (32 KB of LDS each); offered up to 16k pixels.
constexpr double PLAN_T64_ALONE = 0.5, PLAN_T64 = 0.16, PLAN_T64_LONG = 1.5;
constexpr int PLAN_SMALL_MAX_M = 16384, PLAN_MIN_SLICE = 12, PLAN_NK_NOSPLIT = 10, PLAN_RESIDENT = 512;

// Tool knobs (tools/ab_env_bench.sh: A/Bs of the planner's constants INSIDE the pipeline - the constants were fitted on launches timed
// in isolation, and the step runs at the package power limit where the ranking can differ): ES_PLAN_T320 (cost of a K-step of the 256 x 320
// tile, default 2.3), ES_PLAN_BIG_MIN_NK (fewest K-steps it is offered for, 16), ES_PLAN_T256_MARGIN (0.93).  Unset: the fitted values.
double plan_env(const char* name, double dflt) { const char* e = getenv(name); return e && *e ? atof(e) : dflt; }
bool plan_gemm(long long M, int rows_padded, int kpad, bool geglu, const int* bns, int nb, bool allow_split, int* o_bn, int* o_sk, int* o_st) {
  static const double PLAN_T320 = plan_env("ES_PLAN_T320", es_policy::PLAN_T320), PLAN_T256_MARGIN = plan_env("ES_PLAN_T256_MARGIN", es_policy::PLAN_T256_MARGIN);
  static const int PLAN_BIG_MIN_NK = (int)plan_env("ES_PLAN_BIG_MIN_NK", es_policy::PLAN_BIG_MIN_NK);
  // The 256 x 256 phase-interleaved tile (round 5) is offered by the callers for the LayerNorm-folded / GEGLU linear layers whose N is a
  // multiple of 256.  The choice among the OTHER tiles is made first, exactly as before; the 256-wide tile then replaces it where a
  // model fitted on those layers (tools/ln256_bench.py, profiles/r05_ln256_bench.txt: a round of 512 workgroups of the 128-wide tile
  // takes nk x 1.55 + 6 units with the fold's statistics, a round of 256 workgroups of the 256 x 256 tile nk x 2.6 + 6, + 7 with the
  // GEGLU epilogue; WHOLE rounds - its last part-filled round costs a full tile time) says it is at least 7 % faster.
  int others[8], no = 0;
  bool has256 = false;
  for (int bi = 0; bi < nb; ++bi) { if (bns[bi] == 256) has256 = true; else if (no < 8) others[no++] = bns[bi]; }
  if (has256) {
    const int nk = kpad / BK;
    int obn = 0, osk = 1, ost = 2;
    const bool have_other = no > 0 && plan_gemm(M, rows_padded, kpad, geglu, others, no, allow_split, &obn, &osk, &ost);
    if (rows_padded % 256) { if (!have_other) return false; *o_bn = obn; *o_sk = osk; *o_st = ost; return true; }
    const long long t256 = ((M + 255) / 256) * (rows_padded / 256);
    const double c256 = (double)((t256 + 255) / 256) * ((double)nk * PLAN_T256 + PLAN_T256_FIX + (geglu ? PLAN_T256_GEGLU : 0.0));
    bool take = !have_other;
    if (have_other && M >= PLAN_BIG_MIN_M && nk >= PLAN_BIG_MIN_NK && osk == 1 && obn != 64) {
      const long long to = ((M + BM - 1) / BM) * (rows_padded / obn);
      const double co = (double)((to + PLAN_RESIDENT - 1) / PLAN_RESIDENT) * ((double)nk * PLAN_LN_TK * (obn == 160 ? PLAN_T160 : 1.0) + PLAN_T256_FIX);
      take = c256 < PLAN_T256_MARGIN * co;
    }
    if (take) { *o_bn = 256; *o_sk = 1; *o_st = 2; } else { *o_bn = obn; *o_sk = osk; *o_st = ost; }
    return true;
  }
  if (geglu) { *o_bn = 128; *o_sk = 1; *o_st = 2; return true; }
  const int nk = kpad / BK;
  bool have = false;
  double bt = 0; int bbn = 0, bsk = 0; long long bwgs = 0;
  for (int bi = 0; bi < nb; ++bi) {
    const int bn = bns[bi];
    if (rows_padded % bn) continue;
    if (bn == 320 && (M < PLAN_BIG_MIN_M || nk < PLAN_BIG_MIN_NK) && nb > 1) continue;
    if (bn == 64 && M > PLAN_SMALL_MAX_M && nb > 1) continue;
    const int bm = bn == 320 ? 256 : (bn == 64 ? 64 : BM);
    const int resident = bn == 320 ? PLAN_RESIDENT / 2 : (bn == 64 ? 2 * PLAN_RESIDENT : PLAN_RESIDENT);
    const long long tiles = ((M + bm - 1) / bm) * (rows_padded / bn);
    int last = 1;
    if (allow_split && tiles < resident / 2 && nk > PLAN_NK_NOSPLIT) last = std::max(1, std::min(nk / PLAN_MIN_SLICE, 32));
    for (int sk = 1; sk <= last; ++sk) {
      const long long wgs = tiles * sk;
      double tk;
      if (bn == 320) tk = PLAN_T320;
      else if (bn == 64) {
        if (sk > 1 && wgs > PLAN_RESIDENT) continue;
        const double w = (double)wgs / (double)(PLAN_RESIDENT / 2);
        const double ex = std::max(0.0, w - 1.0);
        tk = (PLAN_T64_ALONE + PLAN_T64 * (ex * ex)) * (nk <= 40 ? 1.0 : PLAN_T64_LONG);
      } else tk = (bn == 160 ? PLAN_T160 : 1.0) * (wgs <= PLAN_RESIDENT / 2 ? PLAN_ALONE : 1.0);
      // rounds of workgroups: whole ones for the two-per-CU tiles; the 256 x 320 tile (one workgroup per CU, long tiles) is measured to
      // cost its FRACTIONAL number of rounds - 896 tiles = 3.5 rounds run in 3.5 tile times, the CUs of a part-filled round run faster
      // (tools/plan_fit_bench.py, round 4) - and no less than 0.9 of a round
      const double rounds = bn == 320 ? std::max((double)wgs / 256.0, 0.9) : (double)((wgs + resident - 1) / resident);
      double t = rounds * (((double)nk / (double)sk) * tk + (bn == 320 ? PLAN_T320_FIX : PLAN_TFIX));
      if (sk > 1) t += PLAN_RED_FIX + (double)sk * (double)M * (double)rows_padded * 8.0 / PLAN_SLAB_BYTES_PER_UNIT;
      if (!have || t < bt) { have = true; bt = t; bbn = bn; bsk = sk; bwgs = wgs; }
    }
  }
  if (!have) return false;
  *o_bn = bbn; *o_sk = bsk;
  // at most one workgroup per CU: a 4-deep LDS ring (3 K-steps of DMA in flight) hides the HBM round trip that the 2-stage ring leaves
  // exposed when no second workgroup shares the CU (the deep_ring knob turns it off: launch_choose)
  if (bbn == 64) *o_st = (bwgs <= PLAN_RESIDENT && nk / bsk >= 6) ? 4 : 2;
  else *o_st = (bbn != 320 && bwgs <= PLAN_RESIDENT / 2 && nk / bsk >= 6) ? 4 : 2;
  return true;
}

constexpr int XS_TARGET_WGS = 256, XS_MIN_M = 8192;
bool xs_shape_fits(int ksize, int kpad, int cin, int ctail, int cout, bool geglu) {      // what the kernel can run at all
  if (ksize != 1 || (kpad != 320 && kpad != 640) || cin != kpad || ctail) return false;
  const int ch = kpad == 320 ? 64 : 32;
  const int line = ch * (128 / (geglu ? ch : 2 * ch));
  return !(cout % line || cout < 4 * line);
}
// ... and where it wins (min_m 0: everywhere).  tools/xs_bench.py, batch-1 shapes: 1.4-1.6x on the 14-sample launches of both levels and
// 1.05-1.1x on the decoder's wide K = 320 projections; it loses where a workgroup's share of N is a few chunks (the activation rows are
// re-read per slice and the 40 KB stages no longer amortise): small M with K = 640, narrow N at small M
bool xs_shape_ok(long long M, int ksize, int kpad, int cin, int ctail, int cout, bool geglu, long long min_m) {
  if (!xs_shape_fits(ksize, kpad, cin, ctail, cout, geglu)) return false;
  if (min_m && (M < min_m || (M < 4 * min_m && cout < (kpad == 320 ? 960 : 1920)))) return false;
  return true;
}
int choose_bn(int cout) { return (cout % 160 == 0 && cout % 128 != 0) ? 160 : 128; }

// The slices of an es_linear_xs launch: a workgroup holds 256 rows and walks a slice of whole 128-byte output lines; the lines are cut into
// as many slices as bring the launch to about XS_TARGET_WGS workgroups (`force_slices` > 0, a tool knob, replaces that target), every
// slice but the last of equal length, none empty.  Shapes of fewer than four lines, which the policy never routes here, are cut too:
// the kernel runs them and its tests launch them.
bool launch_xs_slices(long long M, int kpad, int cout, bool geglu, int force_slices, int32_t* nslices, int32_t* chunks_per_slice) {
  if (M < 1 || (kpad != 320 && kpad != 640)) return false;
  const int ch = kpad == 320 ? 64 : 32;
  const int pline = 128 / (geglu ? ch : 2 * ch);            // chunks per 128-byte output line
  if (cout < ch * pline || cout % (ch * pline)) return false;
  const int lines = cout / ch / pline;
  const long long rbs = (M + 255) / 256;
  long long want = std::max<long long>(1, std::min<long long>(lines, XS_TARGET_WGS / rbs));
  if (force_slices > 0) want = std::max(1, std::min(lines, force_slices));
  const int lps = (int)((lines + want - 1) / want);         // lines per slice
  *nslices = (lines + lps - 1) / lps;
  *chunks_per_slice = lps * pline;
  return true;
}

// ---- the launch policy (include/edgestyle_hip.h es_launch_choose): what BOTH hosts ask between validating a call and filling its
// descriptor - ops.conv_gemm / gn_proj_in / group_norm and the Builder of builder.hip -------------------------------------------------
bool wide_stream(int dtype, const es_launch_knobs& k) { return k.wide_stream == 1 || (k.wide_stream < 0 && dtype == ES_BF16); }
// a rule of the SHAPE alone (grouped and per-net launches of a layer must agree): where the stand-alone GroupNorm is the two-launch form -
// slabs too large for a workgroup's registers, the 64 x 64 level - the hand-over removes its statistics launch and second read
bool gn_handover(long long hw, int c, int groups, const es_launch_knobs& k) {
  if (!k.gn_handover || groups < 1 || c % 8 || hw % 64 || c % groups || c / groups > 64) return false;
  return k.gn_handover == 2 || !es_group_norm_is_slab((int)hw, c, groups);
}
bool groups_tile_256(const es_launch_query& q) {
  for (int g = 0; g < std::min(q.n_counts, 4); ++g) if ((q.group_n[g] * q.hw) % 256) return false;
  return true;
}
// does this plain linear launch go to es_linear_xs?  (A residual rides along at K = 320 - Attention.to_out / proj_out of the 64 x 64
// level - unless the launch carries the two-word residual stream, which only es_conv_gemm implements.)
bool launch_takes_xs(const es_launch_query& q, const es_launch_knobs& k) {
  const bool xs_res = !q.has_residual || (k.xs_residual && q.kpad == 320 && !q.geglu && !q.has_ln && q.residual_dense && !(q.wide && wide_stream(q.dtype, k)));
  if (!(q.ksize == 1 && q.stride == 1 && !q.upsample && !q.C2 && !q.has_temb && xs_res && !q.n_tails && q.x_rep == 1 && q.act == ES_ACT_NONE &&
        q.unit_scale && !q.force_splitk && !k.force_bn && k.xs_enabled)) return false;
  if (q.ngroups > 1 && (q.ngroups > 4 || !groups_tile_256(q) || !q.groups_agree)) return false;
  return xs_shape_ok(q.M, q.ksize, q.kpad, q.cin, q.ctail, q.cout, q.geglu != 0, k.xs_min_m);
}
bool launch_choose(const es_launch_query& q, const es_launch_knobs& k, es_launch_choice* o) {
  memset(o, 0, sizeof(*o));
  if (launch_takes_xs(q, k)) { o->route = ES_ROUTE_LINEAR_XS; return true; }
  const bool aligned = q.C1 % BK == 0 && q.C2 % BK == 0;
  const bool big_ok = k.big_tile && aligned && !q.geglu && !q.has_ln && groups_tile_256(q);
  const bool small_ok = k.small_tile && aligned && !q.geglu && k.force_waves != 8;
  // the 256 x 256 phase-interleaved tile: LayerNorm-folded and GEGLU linear layers whose N is a multiple of 256
  const bool ln256_ok = k.big_tile_256 && (q.geglu || q.has_ln) && q.ksize == 1 && q.stride == 1 && !q.upsample && !q.C2 && !q.n_tails && !q.has_temb &&
                        q.x_rep == 1 && q.C1 % BK == 0 && q.rows_padded % 256 == 0 && q.cout % 8 == 0 && !(q.geglu && q.has_residual) && !q.wide &&
                        q.gn_groups == 0 && k.force_waves != 8 && groups_tile_256(q);
  int cand[5], nc = 0;
  if (ln256_ok) cand[nc++] = 256;
  if (big_ok) cand[nc++] = 320;
  cand[nc++] = 160; cand[nc++] = 128;
  if (small_ok) cand[nc++] = 64;
  if (k.force_bn) { cand[0] = k.force_bn; nc = 1; }
  const bool geglu = q.geglu != 0, allow_split = !q.has_ln;
  int bn, splitk, stages;
  if (!plan_gemm(q.M, q.rows_padded, q.kpad, geglu, cand, nc, allow_split, &bn, &splitk, &stages)) return false;
  if (bn == 320 && !k.force_bn && (q.force_splitk ? q.force_splitk : splitk) == 1 &&
      !es_conv_gemm8p_form_ok(geglu ? ES_ACT_GEGLU : q.act, q.cout, q.has_temb, q.hw, q.has_residual)) {
    // the 256 x 320 tile does not implement this epilogue form (an activation, time-embedding rows that differ inside a 128-pixel half
    // or meet a residual): plan again without it, so that the tile planned, recorded and reported is the tile that runs
    const int at = (int)(std::find(cand, cand + nc, 320) - cand);
    std::copy(cand + at + 1, cand + nc, cand + at);
    if (!plan_gemm(q.M, q.rows_padded, q.kpad, geglu, cand, nc - 1, allow_split, &bn, &splitk, &stages)) return false;
  }
  if (stages == 4 && !k.deep_ring) stages = 2;
  if (q.force_splitk) { splitk = q.force_splitk; stages = q.stages; }       // (the planner's ring depth belongs to ITS split)
  else if (q.stages) stages = q.stages;
  if (!stages) stages = k.force_stages;
  o->bn = bn; o->splitk = splitk; o->stages = stages;
  // 1x1 convs / linears are short-K, latency-bound launches: two waves per SIMD on the same 128-pixel tile overlap DMA issue, fragment reads
  // and MFMAs (tools/gemm_tune.py: 3-15 % on every 1x1 shape of a batch-1 step, none on 3x3 or on the memory-bound 1x1 launches of large batches)
  if (k.force_waves) o->waves = k.force_waves;
  else if (k.eight_waves && q.ksize == 1 && q.M <= 65536 && aligned && bn != 64 && bn != 320 && bn != 256 && !(stages == 4 && bn != 128) && stages != 3) o->waves = 8;
  // XCD chunk order: keep the larger operand's tiles together on one XCD (gemm_conv.hip conv_gemm_kernel)
  o->xcd_m_fastest = k.xcd_order < 0 ? (q.ngroups <= 1 && splitk == 1 && q.M <= 2048 && q.w_numel > q.src_numel) : k.xcd_order;
  const int cstore = geglu ? q.cout / 2 : q.cout;
  o->gn_partials = q.gn_groups > 0 && gn_handover(q.hw, cstore, q.gn_groups, k) && !geglu && !q.has_ln && q.cout / q.gn_groups <= (bn == 320 ? 160 : bn);
  o->wide = q.wide && q.has_residual && wide_stream(q.dtype, k) && cstore % 8 == 0 && !geglu;
  return true;
}
// Transformer2DModel.norm -> proj_in as a statistics pass and the projection on es_linear_xs, which applies the GroupNorm to the rows it
// holds in registers: where the projection runs on that kernel anyway, and at K = 320 from 8192 rows on (profiles/r05_gn_proj_in.txt)
bool launch_gn_fold(const es_launch_query& q, int groups, const es_launch_knobs& k) {
  if (!(k.gn_fold && k.xs_enabled) || k.gn_handover || q.hw % 256 || groups < 1 || groups > 32) return false;
  if (q.geglu || q.has_ln || q.kpad % groups || !xs_shape_fits(q.ksize, q.kpad, q.cin, q.ctail, q.cout, false)) return false;
  if (q.M < (q.kpad == 320 ? 8192 : 32768)) return false;
  return !(q.ngroups > 1 && (q.ngroups > 4 || !groups_tile_256(q) || !q.groups_agree));
}
// The knobs before any switch is read: every kernel and tile on, es_linear_xs from 8192 rows, the GroupNorm hand-over off, the two-word
// stream for bf16 only, XCD order by the rule, nothing forced.  es_load_weights overlays the switches it honours (builder.hip
// read_build_env), the CLIP towers turn es_linear_xs off (encoder.h), the Python host builds its own set from the attributes of
// edgestyle_amd.ops and a test holds it to this one.
void launch_default_knobs(es_launch_knobs* k) {
  memset(k, 0, sizeof(*k));
  k->xs_enabled = k->big_tile = k->big_tile_256 = k->small_tile = k->eight_waves = k->deep_ring = k->xs_residual = k->gn_fold = 1;
  k->xs_min_m = XS_MIN_M; k->xcd_order = -1; k->wide_stream = -1;
}

}  // namespace es_policy

using namespace es_policy;

extern "C" int es_plan_gemm_choice(long long M, int rows_padded, int kpad, int geglu, const int* bns, int n_bns, int allow_split, int* bn, int* splitk, int* stages) {
  if (!bns || n_bns < 1 || !bn || !splitk || !stages) { es_set_error("es_plan_gemm_choice: null argument"); return -1; }
  if (!plan_gemm(M, rows_padded, kpad, geglu != 0, bns, n_bns, allow_split != 0, bn, splitk, stages)) { es_set_error("es_plan_gemm_choice: rows_padded fits no N tile"); return -1; }
  return 0;
}
extern "C" int es_linear_xs_eligible(long long M, int ksize, int kpad, int cin, int ctail, int cout, int geglu) {
  return xs_shape_ok(M, ksize, kpad, cin, ctail, cout, geglu != 0, XS_MIN_M) ? 1 : 0;
}
extern "C" int es_launch_choose(const es_launch_query* q, const es_launch_knobs* k, es_launch_choice* out) {
  if (!q || !k || !out) { es_set_error("es_launch_choose: null argument"); return -1; }
  if (!launch_choose(*q, *k, out)) { es_set_error("es_launch_choose: rows_padded fits no N tile"); return -1; }
  return 0;
}
extern "C" int es_launch_route(const es_launch_query* q, const es_launch_knobs* k) { return q && k && launch_takes_xs(*q, *k) ? ES_ROUTE_LINEAR_XS : ES_ROUTE_CONV_GEMM; }
extern "C" int es_launch_gn_fold(const es_launch_query* q, int groups, const es_launch_knobs* k) { return q && k && launch_gn_fold(*q, groups, *k); }
extern "C" int es_launch_gn_handover(long long hw, int c, int groups, const es_launch_knobs* k) { return k && gn_handover(hw, c, groups, *k); }
extern "C" int es_launch_wide_stream(int dtype, const es_launch_knobs* k) { return k && wide_stream(dtype, *k); }
extern "C" void es_launch_default_knobs(es_launch_knobs* k) { if (k) launch_default_knobs(k); }
extern "C" int es_launch_xs_slices(long long M, int kpad, int cout, int geglu, int force_slices, int32_t* nslices, int32_t* chunks_per_slice) {
  if (!nslices || !chunks_per_slice) { es_set_error("es_launch_xs_slices: null argument"); return -1; }
  if (!launch_xs_slices(M, kpad, cout, geglu != 0, force_slices, nslices, chunks_per_slice)) {
    es_set_error("es_launch_xs_slices: es_linear_xs runs K = 320 | 640 over at least one row and whole 128-byte output lines");
    return -1;
  }
  return 0;
}

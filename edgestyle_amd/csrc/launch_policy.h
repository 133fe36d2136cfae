// The launch policy (launch_policy.hip) as the native builders call it: builder.hip (es_load_weights) and encoder.h (the CLIP towers) ask
// these functions directly; every other host goes through the C entries of include/edgestyle_hip.h (es_launch_choose and its siblings),
// which wrap the same functions.
#pragma once
#include "../../include/edgestyle_hip.h"

namespace es_policy {

constexpr int BK = 64, BM = 128;      // K-step and pixel tile of es_conv_gemm (gemm_conv.hip)

// N tile a weight is PACKED for (rows_padded = cout rounded up to it); the tile a launch runs is launch_choose's
int choose_bn(int cout);
// false: rows_padded fits no N tile
bool launch_choose(const es_launch_query& q, const es_launch_knobs& k, es_launch_choice* out);
bool launch_gn_fold(const es_launch_query& q, int groups, const es_launch_knobs& k);
bool gn_handover(long long hw, int c, int groups, const es_launch_knobs& k);
// every knob at the value a host starts from before it reads its switches (es_launch_default_knobs)
void launch_default_knobs(es_launch_knobs* k);
// how an es_linear_xs launch over M rows is cut into slices of output lines (es_launch_xs_slices); false: no shape that kernel runs
bool launch_xs_slices(long long M, int kpad, int cout, bool geglu, int force_slices, int32_t* nslices, int32_t* chunks_per_slice);

}  // namespace es_policy

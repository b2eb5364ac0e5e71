// tok_h2.h -- launchers of the f16x2 token-chain kernels (tok_h2.hip), called by the four afd_tok_* entry points of
// tok.hip for C in {64, 128}.  Arguments as the entry points; max_wg > 0 caps the workgroups of the launch
// (afd_debug_tok_grid).  Each is ONE kernel launch and returns an AFD_* code (a failed LDS opt-in included).
#pragma once
#include "common.h"

namespace afd {

int tok_h2_head_fwd(const float* x, const float* gamma, const float* beta, const float* w, const float* bias, float* h_out,
                    float* stats_out, float* qkv, int B, int C, int P, float eps, int max_wg, hipStream_t s);
int tok_h2_tail_fwd(const float* att, const float* x, const float* wo, const float* bo, const float* gamma, const float* beta,
                    const float* w1, const float* b1, const float* w2, const float* b2, float* a_out, float* stats_out,
                    float* f_out, float* u_out, float* g_out, float* out, int B, int C, int P, float eps, int max_wg, hipStream_t s);
int tok_h2_tail_bwd(const float* d_out, const float* u, const float* a, const float* stats, const float* gamma, const float* w2,
                    const float* w1, const float* wo, float* du_out, float* df_out, float* da_out, float* datt_out, int B, int C,
                    int P, int max_wg, hipStream_t s);
int tok_h2_head_bwd(const float* dqkv, const float* x, const float* stats, const float* gamma, const float* w_in,
                    const float* d_res, float* dh_out, float* dx_out, int B, int C, int P, int max_wg, hipStream_t s);
void tok_h2_debug_tpw(int tpw);   // C = 64: 2 or 4 waves (= tiles) per workgroup, 0 = by the rule (C = 128 always runs 4)

}  // namespace afd

// attn_forms.h -- what attn.hip calls in attn_mfma.hip and attn_small.hip (internal), declared once and included by all three,
// so the compiler checks each definition against its declaration.
#pragma once
#include "common.h"

namespace afd {

// ---- attn_mfma.hip: d = 8 / 16 passes with the d-contractions on the matrix cores.  The *_ok / attn_fused_bwd results say
// whether the kernels cover the shape (attn_fused_bwd: true = launched); the others launch unconditionally
extern int g_attn_pv;               // afd_debug_attn_rows 20 / 21: rank-8 products of the d = 8 kernels on the vector pipe (round 2) / on the fp16 matrix pipe
extern int g_attn_pv16;             // afd_debug_attn_rows 40 / 41: d = 16 on the round-2 kernels / on attn_fwd_pv<16> and attn_bwd_fused<16, 1>
bool attn_mfma8_ok(int d, int L);
bool attn_fused_bwd(const float* qkv, const float* o, const float* d_o, const float* lse, float* dqkv, float* delta, int B, int heads,
                    int d, int L, float sc, hipStream_t s);
void attn_mfma8_fwd(const float* qkv, float* o, float* lse, int B, int heads, int d, int L, float sc, hipStream_t s);
void attn_mfma8_bwd_dq(const float* qkv, const float* o, const float* d_o, const float* lse, float* dqkv, float* delta,
                       int B, int heads, int d, int L, float sc, hipStream_t s);
void attn_mfma8_bwd_dkv(const float* qkv, const float* d_o, const float* lse, const float* delta, float* dqkv, int B, int heads, int L,
                        float sc, hipStream_t s);

// ---- attn_small.hip: d in {16,32}, L in {16,32,48,64}, one wave per (batch, head) on the fp32 matrix pipe.  attn_small_ok =
// the kernels cover the shape; the launchers launch unconditionally
bool attn_small_ok(int d, int L);
void attn_small_fwd_launch(const float* qkv, float* o, float* lse, int B, int heads, int d, int L, float sc, hipStream_t s);
void attn_small_bwd_launch(const float* qkv, const float* d_o, float* dqkv, int B, int heads, int d, int L, float sc, hipStream_t s);

}  // namespace afd

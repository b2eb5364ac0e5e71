// tok_common.h -- the T layout of the token-chain kernels (tok.hip, tok_h2.hip): tile type, pixel addressing, global <->
// register moves and the LayerNorm steps on a register-resident tile.  See the header comment of tok.hip.
#pragma once
#include "common.h"

namespace afd {

using f32x16 = __attribute__((ext_vector_type(16))) float;

template <int NB> struct TT { f32x16 b[NB]; };

__device__ __forceinline__ constexpr int tch(int j, int r) { return 32 * j + (r & 3) + 8 * (r >> 2); }   // + 4 * half

struct Pix { unsigned b, p, f; bool live; };
__device__ __forceinline__ Pix pix_of(int tile, int l31, unsigned total, unsigned P) {
  Pix q;
  q.f = (unsigned)tile * 32u + (unsigned)l31;
  q.live = q.f < total;
  const unsigned fc = q.live ? q.f : 0u;
  q.b = fc / P;
  q.p = fc - q.b * P;
  return q;
}
// element offset of (pixel, channel 4*half) in a tensor with Cx channels
__device__ __forceinline__ unsigned tbase(const Pix& q, unsigned Cx, unsigned P, int half) {
  return q.b * Cx * P + q.p + 4u * (unsigned)half * P;
}

template <int NB>
__device__ __forceinline__ void t_load(TT<NB>& z, const float* __restrict__ src, unsigned base, unsigned P, bool live) {
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) z.b[j][r] = live ? src[base + (unsigned)tch(j, r) * P] : 0.f;
}
template <int NB>
__device__ __forceinline__ void t_store(const TT<NB>& z, float* __restrict__ dst, unsigned base, unsigned P, bool live) {
  if (!live) return;
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[base + (unsigned)tch(j, r) * P] = z.b[j][r];
}

__device__ __forceinline__ f32x16 zero16() {
  f32x16 a;
#pragma unroll
  for (int r = 0; r < 16; ++r) a[r] = 0.f;
  return a;
}

// LayerNorm over the C channels of each pixel, T layout.  gs / bs: gamma / beta in LDS.
template <int KB>
__device__ __forceinline__ void t_ln_fwd(const TT<KB>& x, const float* __restrict__ gs, const float* __restrict__ bs, int half,
                                         float eps, TT<KB>& y, float& mean, float& rstd) {
  constexpr float invC = 1.0f / (32 * KB);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < KB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += x.b[j][r];
  s += __shfl_xor(s, 32, 64);
  mean = s * invC;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < KB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) { const float d = x.b[j][r] - mean; q = fmaf(d, d, q); }
  q += __shfl_xor(q, 32, 64);
  rstd = 1.0f / sqrtf(q * invC + eps);
#pragma unroll
  for (int j = 0; j < KB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = tch(j, r) + 4 * half;
      y.b[j][r] = (x.b[j][r] - mean) * rstd * gs[c] + bs[c];
    }
}
// dx = rstd * (g*dy - mean_c(g*dy) - xhat * mean_c(g*dy*xhat)) + add      (x: the LayerNorm input, in place in `dy`)
template <int KB>
__device__ __forceinline__ void t_ln_bwd(TT<KB>& dy, const TT<KB>& x, const float* __restrict__ gs, int half, float mean,
                                         float rstd, const TT<KB>& add) {
  constexpr float invC = 1.0f / (32 * KB);
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < KB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float gv = gs[tch(j, r) + 4 * half] * dy.b[j][r];
      const float xh = (x.b[j][r] - mean) * rstd;
      dy.b[j][r] = gv;
      s1 += gv;
      s2 = fmaf(gv, xh, s2);
    }
  s1 += __shfl_xor(s1, 32, 64);
  s2 += __shfl_xor(s2, 32, 64);
  const float m1 = s1 * invC, m2 = s2 * invC;
#pragma unroll
  for (int j = 0; j < KB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float xh = (x.b[j][r] - mean) * rstd;
      dy.b[j][r] = rstd * (dy.b[j][r] - m1 - xh * m2) + add.b[j][r];
    }
}

}  // namespace afd

// attn_small.hip -- F10 attention core for the small maps: d in {16, 32}, L in {16, 32, 48, 64}, on the fp32 matrix pipe.
//
// One wave owns one (batch, head) pair end to end and keeps the whole L x L score tile in registers; four independent
// waves per 256-thread workgroup, one per SIMD (B * heads = 1024 at B = 256: one wave per SIMD of the chip).  Waves never
// cooperate: no LDS, no barriers, no atomics.  All products are v_mfma_f32_16x16x4_f32 -- exact f32, a k-ordered fmaf
// chain like the vector kernels of attn.hip -- so the results stay in their error class and are bitwise reproducible.
//
// Operand maps of the 16x16x4 form (lane l: c = l & 15, g = l >> 4): A[i = c][k = g], B[k = g][j = c], and the
// accumulator holds column c, rows 4g + r in register r.  qkv is (D, L) per head with the token index contiguous, so an
// operand whose free index is the token is read from global memory straight in operand order (16 consecutive floats
// per k), and one whose CONTRACTED index is the token is read as one float4 per lane: tokens 4g .. 4g + 3 of a 16-block,
// which is exactly the k order in which an accumulator tile presents its rows when it is fed back as the B operand.
// So every product below takes the previous one's accumulator as its B operand with no lane movement:
//   forward : S^T = K Q^T (column = query) -> two-pass softmax per column -> O^T = V^T P^T
//   backward: S^T, dP^T = V dO^T (column = query) -> P^T, delta = colsum(P^T o dP^T), dS^T -> dQ^T = K^T dS^T;
//             S = Q K^T, dP = dO V^T (column = key: the same fmaf chains, the same bits) -> P, dS
//             -> dV^T = dO^T P, dK^T = Q^T dS.
// The backward computes S and dP in both orientations instead of transposing P and dS through LDS: two extra products of
// seven, and no memory of its own.  The two orientations share nothing, so they are two launches (PART 0: dQ, PART 1: dK
// and dV), each one wave per pair, each taking the softmax and delta = rowsum(P o dP) itself: no attn_delta_k, no read of
// o, lse or the delta workspace.  (The step's replay list keeps its length -- tests/test_gpu_clip.py pins it -- and the two
// halves could overlap.)  Both redo the two-pass softmax (max, exp2, sum) instead of P = exp2(S - lse): lse is stored in
// natural log, and at |lse| ~ 300 (a peaked row) its fp32 rounding alone is a 3e-5 relative error on every probability.
#include "attn_forms.h"

namespace afd {

namespace {
using f4 = __attribute__((ext_vector_type(4))) float;
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// the four lanes that share a column (lane groups g = 0..3) combine their partial results; every lane gets the same bits
__device__ __forceinline__ float col_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, kWave));
  return fmaxf(v, __shfl_xor(v, 32, kWave));
}
__device__ __forceinline__ float col_sum(float v) {
  v += __shfl_xor(v, 16, kWave);
  return v + __shfl_xor(v, 32, kWave);
}
// the sixteen lanes that share a row (c = 0..15 of one lane group): xor butterflies, every lane gets the same bits
__device__ __forceinline__ float row_max(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// X (D, L) j-major: the operand with the token as its free index, k = feature.  r[t][s]: token 16t + c, feature 4s + g
template <int D, int T>
__device__ __forceinline__ void load_free(const float* __restrict__ x, int c, int g, float mul, float (&r)[T][D / 4]) {
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int s = 0; s < D / 4; ++s) r[t][s] = x[(4 * s + g) * (16 * T) + 16 * t + c] * mul;
}
// the operand with the token as its contracted index: r[jt][t] = feature 16jt + c, tokens 16t + 4g .. + 3
template <int D, int T>
__device__ __forceinline__ void load_contr(const float* __restrict__ x, int c, int g, f4 (&r)[D / 16][T]) {
#pragma unroll
  for (int jt = 0; jt < D / 16; ++jt)
#pragma unroll
    for (int t = 0; t < T; ++t) r[jt][t] = *reinterpret_cast<const f4*>(x + (16 * jt + c) * (16 * T) + 16 * t + 4 * g);
}
// acc[a][b] += A-side rows a x B-side columns b over the D features
template <int D, int T>
__device__ __forceinline__ void prod_feat(const float (&a)[T][D / 4], const float (&b)[T][D / 4], f4 (&acc)[T][T]) {
#pragma unroll
  for (int s = 0; s < D / 4; ++s)
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
      for (int j = 0; j < T; ++j) acc[i][j] = mfma4(a[i][s], b[j][s], acc[i][j]);
}
// out^T[jt][column tile n] += sum over the row tokens (tile m, register r) of x[jt][m][r] * acc[m][n][r]
template <int D, int T>
__device__ __forceinline__ void prod_tok(const f4 (&x)[D / 16][T], const f4 (&acc)[T][T], f4 (&out)[D / 16][T]) {
#pragma unroll
  for (int m = 0; m < T; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int jt = 0; jt < D / 16; ++jt)
#pragma unroll
        for (int n = 0; n < T; ++n) out[jt][n] = mfma4(x[jt][m][r], acc[m][n][r], out[jt][n]);
}
// dst (D, L) j-major <- out^T * mul: feature 16jt + 4g + r, token 16n + c
template <int D, int T>
__device__ __forceinline__ void store_t(float* __restrict__ dst, int c, int g, const f4 (&out)[D / 16][T], const float (&mul)[T]) {
#pragma unroll
  for (int jt = 0; jt < D / 16; ++jt)
#pragma unroll
    for (int n = 0; n < T; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[(16 * jt + 4 * g + r) * (16 * T) + 16 * n + c] = out[jt][n][r] * mul[n];
}
template <int A, int B> __device__ __forceinline__ void zero(f4 (&x)[A][B]) {
#pragma unroll
  for (int i = 0; i < A; ++i)
#pragma unroll
    for (int j = 0; j < B; ++j) x[i][j] = (f4){0.f, 0.f, 0.f, 0.f};
}
}  // namespace

// L = 16 T.  pairs = B * heads; a wave past the end leaves at once (the wave index is read as a scalar: a uniform branch).
template <int D, int T>
__global__ __launch_bounds__(256) void attn_small_fwd(const float* __restrict__ qkv, float* __restrict__ o, float* __restrict__ lse,
                                                       int pairs, int heads, float scale) {
  constexpr int L = 16 * T;
  const int pair = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (pair >= pairs) return;
  const int c = threadIdx.x & 15, g = (threadIdx.x & 63) >> 4;
  const int b = pair / heads, h = pair - b * heads, C = heads * D;
  const float* qp = qkv + ((long)b * 3 * C + h * D) * L;
  const float* kp = qp + (long)C * L;
  const float* vp = kp + (long)C * L;
  float qa[T][D / 4], ka[T][D / 4];
  f4 vt[D / 16][T];
  load_free<D, T>(kp, c, g, 1.f, ka);
  load_free<D, T>(qp, c, g, scale * kLog2e, qa);           // scores in the log2 domain
  load_contr<D, T>(vp, c, g, vt);
  f4 st[T][T];                                             // st[kt][qt]: column = query 16qt + c, rows = keys 16kt + 4g + r
  zero(st);
  prod_feat<D, T>(ka, qa, st);
  float one[T];
#pragma unroll
  for (int qt = 0; qt < T; ++qt) {                         // two passes over the whole row: exact max, then exp and sum
    float m = st[0][qt][0];
#pragma unroll
    for (int kt = 0; kt < T; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) m = fmaxf(m, st[kt][qt][r]);
    m = col_max(m);
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < T; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) { st[kt][qt][r] = __builtin_amdgcn_exp2f(st[kt][qt][r] - m); l += st[kt][qt][r]; }
    l = col_sum(l);
    const float inv = 1.0f / l;                            // P is normalised BEFORE P V: these are the bits the backward rebuilds
#pragma unroll
    for (int kt = 0; kt < T; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) st[kt][qt][r] *= inv;
    one[qt] = 1.f;
    if (g == 0) lse[(long)pair * L + 16 * qt + c] = (m + __builtin_amdgcn_logf(l)) * kLn2;      // v_log_f32 = log2
  }
  f4 ot[D / 16][T];
  zero(ot);
  prod_tok<D, T>(vt, st, ot);                        // O^T[j][query] = sum_key V[key][j] P^T[key][query]
  store_t<D, T>(o + ((long)b * C + h * D) * L, c, g, ot, one);
}

template <int D, int T, int PART>
__global__ __launch_bounds__(256) void attn_small_bwd(const float* __restrict__ qkv, const float* __restrict__ d_o,
                                                       float* __restrict__ dqkv, int pairs, int heads, float scale) {
  constexpr int L = 16 * T;
  const int pair = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (pair >= pairs) return;
  const int c = threadIdx.x & 15, g = (threadIdx.x & 63) >> 4;
  const int b = pair / heads, h = pair - b * heads, C = heads * D;
  const float* qp = qkv + ((long)b * 3 * C + h * D) * L;
  const float* kp = qp + (long)C * L;
  const float* vp = kp + (long)C * L;
  const float* gp = d_o + ((long)b * C + h * D) * L;
  float* dqp = dqkv + ((long)b * 3 * C + h * D) * L;
  float qa[T][D / 4], ka[T][D / 4], va[T][D / 4], ga[T][D / 4];
  load_free<D, T>(kp, c, g, 1.f, ka);
  load_free<D, T>(qp, c, g, scale * kLog2e, qa);
  load_free<D, T>(vp, c, g, 1.f, va);
  load_free<D, T>(gp, c, g, 1.f, ga);
  float sc[T], one[T];
#pragma unroll
  for (int t = 0; t < T; ++t) { sc[t] = scale; one[t] = 1.f; }
  if constexpr (PART == 0) {   // ---- column = query: dQ
    f4 st[T][T], dp[T][T];                                 // [kt][qt]
    zero(st); zero(dp);
    prod_feat<D, T>(ka, qa, st);
    prod_feat<D, T>(va, ga, dp);
#pragma unroll
    for (int qt = 0; qt < T; ++qt) {
      float m = st[0][qt][0], l = 0.f, dl = 0.f;
#pragma unroll
      for (int kt = 0; kt < T; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, st[kt][qt][r]);
      m = col_max(m);
#pragma unroll
      for (int kt = 0; kt < T; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { st[kt][qt][r] = __builtin_amdgcn_exp2f(st[kt][qt][r] - m); l += st[kt][qt][r]; }
      l = col_sum(l);
      const float inv = 1.0f / l;
#pragma unroll
      for (int kt = 0; kt < T; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { st[kt][qt][r] *= inv; dl = fmaf(st[kt][qt][r], dp[kt][qt][r], dl); }
      dl = col_sum(dl);                                    // delta = rowsum(P o dP) (= rowsum(dO o O)), fixed order
#pragma unroll
      for (int kt = 0; kt < T; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) st[kt][qt][r] *= dp[kt][qt][r] - dl;
    }
    f4 kt4[D / 16][T], dq[D / 16][T];
    load_contr<D, T>(kp, c, g, kt4);
    zero(dq);
    prod_tok<D, T>(kt4, st, dq);                     // dQ^T[j][query] = sum_key K[key][j] dS^T[key][query]
    store_t<D, T>(dqp, c, g, dq, sc);
  } else {   // ---- column = key: dV and dK
    f4 s2[T][T], dp[T][T];                                 // [qt][kt]: rows = queries 16qt + 4g + r
    zero(s2); zero(dp);
    prod_feat<D, T>(qa, ka, s2);
    prod_feat<D, T>(ga, va, dp);
    f4 ds[T][T];
#pragma unroll
    for (int qt = 0; qt < T; ++qt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {                                  // query 16qt + 4g + r: its keys lie in the T tiles of 16 lanes
        float m = s2[qt][0][r], l = 0.f, dl = 0.f;
#pragma unroll
        for (int kt = 1; kt < T; ++kt) m = fmaxf(m, s2[qt][kt][r]);
        m = row_max(m);
#pragma unroll
        for (int kt = 0; kt < T; ++kt) { s2[qt][kt][r] = __builtin_amdgcn_exp2f(s2[qt][kt][r] - m); l += s2[qt][kt][r]; }
        const float inv = 1.0f / row_sum(l);
#pragma unroll
        for (int kt = 0; kt < T; ++kt) { s2[qt][kt][r] *= inv; dl = fmaf(s2[qt][kt][r], dp[qt][kt][r], dl); }
        dl = row_sum(dl);
#pragma unroll
        for (int kt = 0; kt < T; ++kt) ds[qt][kt][r] = s2[qt][kt][r] * (dp[qt][kt][r] - dl);
      }
    }
    f4 x4[D / 16][T], out[D / 16][T];
    load_contr<D, T>(gp, c, g, x4);
    zero(out);
    prod_tok<D, T>(x4, s2, out);                     // dV^T[j][key] = sum_query dO[query][j] P[query][key]
    store_t<D, T>(dqp + 2 * (long)C * L, c, g, out, one);
    load_contr<D, T>(qp, c, g, x4);
    zero(out);
    prod_tok<D, T>(x4, ds, out);                     // dK^T[j][key] = sum_query Q[query][j] dS[query][key]
    store_t<D, T>(dqp + (long)C * L, c, g, out, sc);
  }
}

bool attn_small_ok(int d, int L) { return (d == 16 || d == 32) && L % 16 == 0 && L >= 16 && L <= 64; }

template <int D> static void small_fwd_d(const float* qkv, float* o, float* lse, int pairs, int heads, int T, float sc, hipStream_t s) {
  const dim3 grid((pairs + 3) / 4), block(256);
  switch (T) {
    case 1: hipLaunchKernelGGL((attn_small_fwd<D, 1>), grid, block, 0, s, qkv, o, lse, pairs, heads, sc); break;
    case 2: hipLaunchKernelGGL((attn_small_fwd<D, 2>), grid, block, 0, s, qkv, o, lse, pairs, heads, sc); break;
    case 3: hipLaunchKernelGGL((attn_small_fwd<D, 3>), grid, block, 0, s, qkv, o, lse, pairs, heads, sc); break;
    default: hipLaunchKernelGGL((attn_small_fwd<D, 4>), grid, block, 0, s, qkv, o, lse, pairs, heads, sc); break;
  }
}
template <int D> static void small_bwd_d(const float* qkv, const float* d_o, float* dqkv, int pairs, int heads, int T,
                                         float sc, hipStream_t s) {
  const dim3 grid((pairs + 3) / 4), block(256);
  switch (T) {      // two independent launches: dQ; dK and dV
    case 1: hipLaunchKernelGGL((attn_small_bwd<D, 1, 0>), grid, block, 0, s, qkv, d_o, dqkv, pairs, heads, sc);
            hipLaunchKernelGGL((attn_small_bwd<D, 1, 1>), grid, block, 0, s, qkv, d_o, dqkv, pairs, heads, sc); break;
    case 2: hipLaunchKernelGGL((attn_small_bwd<D, 2, 0>), grid, block, 0, s, qkv, d_o, dqkv, pairs, heads, sc);
            hipLaunchKernelGGL((attn_small_bwd<D, 2, 1>), grid, block, 0, s, qkv, d_o, dqkv, pairs, heads, sc); break;
    case 3: hipLaunchKernelGGL((attn_small_bwd<D, 3, 0>), grid, block, 0, s, qkv, d_o, dqkv, pairs, heads, sc);
            hipLaunchKernelGGL((attn_small_bwd<D, 3, 1>), grid, block, 0, s, qkv, d_o, dqkv, pairs, heads, sc); break;
    default: hipLaunchKernelGGL((attn_small_bwd<D, 4, 0>), grid, block, 0, s, qkv, d_o, dqkv, pairs, heads, sc);
             hipLaunchKernelGGL((attn_small_bwd<D, 4, 1>), grid, block, 0, s, qkv, d_o, dqkv, pairs, heads, sc); break;
  }
}

void attn_small_fwd_launch(const float* qkv, float* o, float* lse, int B, int heads, int d, int L, float sc, hipStream_t s) {
  if (d == 16) small_fwd_d<16>(qkv, o, lse, B * heads, heads, L / 16, sc, s);
  else small_fwd_d<32>(qkv, o, lse, B * heads, heads, L / 16, sc, s);
}
void attn_small_bwd_launch(const float* qkv, const float* d_o, float* dqkv, int B, int heads, int d, int L, float sc,
                           hipStream_t s) {
  if (d == 16) small_bwd_d<16>(qkv, d_o, dqkv, B * heads, heads, L / 16, sc, s);
  else small_bwd_d<32>(qkv, d_o, dqkv, B * heads, heads, L / 16, sc, s);
}

}  // namespace afd

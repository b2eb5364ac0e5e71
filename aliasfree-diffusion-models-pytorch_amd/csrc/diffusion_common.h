// diffusion_common.h -- what sampler.hip and objective.hip share (internal): quads and the lane-wise helpers, the (row, quad)
// walk, the noising expression, classifier-free guidance, the DDPM rule, the launch helpers of the VEC kernel pairs and the
// grid-stride launch size gs_grid.
//
// Every fp32 expression here restates the reference's operation ORDER with one IEEE rounding per operation, so a * b + c must
// not fuse.  That is the including file's to say, for all of its code: each .hip file puts `#pragma clang fp contract(off)`
// BEFORE it includes this header (a pragma set here would silently cover the rest of whatever includes it).  Without it
// everything still compiles and every result changes in its last bits.
#pragma once
#include <algorithm>
#include <initializer_list>
#include "common.h"

namespace afd {

// workgroups of a grid-stride launch over `total` elements (both files' elementwise kernels)
static inline int gs_grid(long total, int block = 256) {
  long g = (total + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > 32768 ? 32768 : g));
}

// ---- quads: four consecutive floats of a row -------------------------------------------------------------------------------------
// lane i of a quad (i a constant after unrolling)
__device__ __forceinline__ float lane(const float4& v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }
// f applied lane by lane: {f(a.x, b.x, ...), f(a.y, b.y, ...), f(a.z, b.z, ...), f(a.w, b.w, ...)}; f has no side effects
template <class F, class... Q>
__device__ __forceinline__ float4 quad_map(F f, const Q&... q) {
  return make_float4(f(q.x...), f(q.y...), f(q.z...), f(q.w...));
}
// the quad at offset o of a row whose remaining length is `left` (>= 1): four values, zero past the row's end
template <bool VEC>
__device__ __forceinline__ float4 load_quad(const float* __restrict__ p, long o, long left) {
  if (VEC) return *reinterpret_cast<const float4*>(p + o);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  v.x = p[o];
  if (left > 1) v.y = p[o + 1];
  if (left > 2) v.z = p[o + 2];
  if (left > 3) v.w = p[o + 3];
  return v;
}
template <bool VEC>
__device__ __forceinline__ void store_quad(float* p, long o, long left, float4 v) {
  if (VEC) { *reinterpret_cast<float4*>(p + o) = v; return; }
  p[o] = v.x;
  if (left > 1) p[o + 1] = v.y;
  if (left > 2) p[o + 2] = v.z;
  if (left > 3) p[o + 3] = v.w;
}

// ---- the (row, 256-quad segment) walk ---------------------------------------------------------------------------------------------
// Work item `it` = (row b, segment g) of B rows of chw floats: the 256 threads of a workgroup take the 256 quads [4 q, 4 q + 4)
// of row b with q = 256 g + threadIdx.x, so whatever depends on the row alone is read once per item and is uniform over the
// workgroup.  body(RowQuad) runs once per item of this workgroup, in item order blockIdx.x, + gridDim.x, ...; it does its
// row-uniform loads first and then returns if rq.left <= 0 (the quad lies past the row's end).  256 is the workgroup size of
// every kernel that walks this way, a constant here: blockDim.x read in a __device__ body costs a load (see AFD_GRID_STRIDE).
struct RowQuad {
  long b;       // the row
  long left;    // floats from the quad's first to the row's end: <= 0 past the end, < 4 in a ragged last quad
  long o;       // the quad's offset in a (B, chw) tensor
  long o2;      // and in a (B, 2 chw) one (the learned-variance output: the prediction at o2, its coefficient at o2 + chw)
};
template <class Body>
__device__ __forceinline__ void for_row_quads(long items, long segs, long chw, Body body) {
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const long b = it / segs, q = (it - b * segs) * 256 + threadIdx.x;
    body(RowQuad{b, chw - 4 * q, b * chw + 4 * q, 2 * b * chw + 4 * q});
  }
}
// its launch geometry: at most `cap` workgroups, the item loop takes the rest
struct RowQuadGrid {
  long segs, items;
  int grid;
  RowQuadGrid(long B, long chw, int cap) : segs(((chw + 3) / 4 + 255) / 256), items(B * segs), grid((int)std::min<long>(items, cap)) {}
};

// ---- the expressions both files use -----------------------------------------------------------------------------------------------
// sqrt(a), sqrt(1 - a) of a = alpha_hat[t]
struct Roots {
  float sa, sb;
};
__device__ __forceinline__ Roots roots(float ah) { return Roots{sqrtf(ah), sqrtf(1.0f - ah)}; }
// x_t = sqrt(a) * x + sqrt(1 - a) * eps, the forward process (ddpm_models.py:317-321)
__device__ __forceinline__ float noised(float sa, float sb, float x, float e) {
  const float l = sa * x, r = sb * e;
  return l + r;
}

// classifier-free guidance: eps holds the 2n-row forward, element j of the conditional half at j, of the unconditional half at
// n + j, and e = torch.lerp(e_u, e_c, s) with ATen's scalar formula (aten/src/ATen/native/Lerp.h), one rounding per operation:
//   |s| < 0.5:  u + s * (c - u)        otherwise:  c - (c - u) * (1 - s)
struct Guidance {
  float s, one_minus_s;
  bool small;
};
__device__ __forceinline__ Guidance guidance(float s) { return Guidance{s, 1.0f - s, fabsf(s) < 0.5f}; }
__device__ __forceinline__ float cfg_lerp(float s, float one_minus_s, bool small, float ec, float eu) {
  const float d = ec - eu;
  return small ? eu + s * d : ec - d * one_minus_s;
}
template <bool kCfg>
__device__ __forceinline__ float guided_eps(const Guidance& g, float ec, float eu) {
  return kCfg ? cfg_lerp(g.s, g.one_minus_s, g.small, ec, eu) : ec;
}

// A sampler is a rule type: Args (what its kernel is handed), make(Args) (the coefficients, once per thread before the loop),
// update(x, e, z, gen_noise) (the per-element expression) and, for the masked form, t_prev() and gen_takes_noise().  Step
// indices given on the device (the *_dev pointers) let a captured graph replay for every step.

// DDPM, step -> step - 1:  x' = 1/sqrt(a) * (x - ((1-a)/sqrt(1-ah)) * eps) + sqrt(b) * noise
// masked: the generated region takes no noise at step 1 (the chain's last step)
// (here because the bound's decoder term and the learned-variance step use it)
struct Ddpm {
  struct Args {
    const float *alpha, *alpha_hat, *beta;
    int step;
    const int64_t* step_dev;
  };
  float c1, c2, sb;
  int step;
  __device__ __forceinline__ static Ddpm at(const float* alpha, const float* alpha_hat, const float* beta, int step) {
    const float a = alpha[step], ah = alpha_hat[step], bt = beta[step];
    Ddpm k;
    k.c1 = 1.0f / sqrtf(a);
    k.c2 = (1.0f - a) / sqrtf(1.0f - ah);
    k.sb = sqrtf(bt);
    k.step = step;
    return k;
  }
  __device__ __forceinline__ static Ddpm make(const Args& a) {
    return at(a.alpha, a.alpha_hat, a.beta, a.step_dev ? (int)a.step_dev[0] : a.step);
  }
  __device__ __forceinline__ float update(float x, float e, float nz_in, bool has_noise) const {
    const float pe = c2 * e;
    const float inner = x - pe;
    const float lhs = c1 * inner;
    const float nz = has_noise ? sb * nz_in : 0.0f;       // sqrt(beta) * zeros == +0
    return lhs + nz;
  }
  __device__ __forceinline__ int t_prev() const { return step > 0 ? step - 1 : 0; }
  __device__ __forceinline__ bool gen_takes_noise() const { return step > 1; }
};

// ---- host side: the VEC kernel pairs ----------------------------------------------------------------------------------------------
// 16-byte accesses when n % 4 == 0 and every pointer given is 16-byte aligned (an absent optional pointer, NULL, counts as
// aligned)
static inline bool vec_ok(long n, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (!aligned16(p)) return false;
  return n % 4 == 0;
}
// kern<true> when vec, else kern<false>, on `grid` workgroups of 256
template <class... P, class... A>
static inline void launch_vec(bool vec, void (*kv)(P...), void (*ks)(P...), long grid, hipStream_t st, A... args) {
  hipLaunchKernelGGL(vec ? kv : ks, dim3((unsigned)grid), dim3(256), 0, st, static_cast<P>(args)...);
}

}  // namespace afd

// ddpm.hip -- F14/F16 DDPM noise / denoise / quantise, MSE loss, fused AdamW.
//
// noise_images / denoise_step / quantize restate the reference's fp32 expression ORDER with one
// IEEE rounding per torch op (no FMA contraction, correctly rounded sqrt and divide), so given the
// same inputs they are bit-identical to the reference's CPU path (ddpm_models.py:317-321,367-374,381-385).
// hipcc keeps `/` and sqrtf correctly rounded by default; `#pragma clang fp contract(off)` below
// stops a*b+c from fusing.  (The __f*_rn intrinsics are NOT used: without
// OCML_BASIC_ROUNDED_OPERATIONS this toolchain maps __fsqrt_rn to the approximate native sqrt.)
#include "common.h"

#pragma clang fp contract(off)

namespace afd {

static inline int gs_grid(long total, int block = 256) {
  long g = (total + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > 32768 ? 32768 : g));
}
#define AFD_GRID_STRIDE(i, total) \
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (total); i += (long)gridDim.x * blockDim.x)
// the same loop's start and stride, taken in a kernel and handed to a __device__ body (inside the body, blockDim.x would be
// read without the kernel's uniform-work-group assumption: one extra load per thread)
#define AFD_GRID_START blockIdx.x * (long)blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x

// x_t = sqrt(ah[t]) * x + sqrt(1 - ah[t]) * eps
__global__ void noise_images_k(const float* __restrict__ x, const float* __restrict__ eps, const int64_t* __restrict__ t,
                               const float* __restrict__ alpha_hat, float* __restrict__ xt, long per, long total) {
  AFD_GRID_STRIDE(i, total) {
    const long b = i / per;
    const float ah = alpha_hat[t[b]];
    const float sa = sqrtf(ah);
    const float sb = sqrtf(1.0f - ah);
    const float l = sa * x[i], r = sb * eps[i];
    xt[i] = l + r;
  }
}

// x' = 1/sqrt(a) * (x - ((1-a)/sqrt(1-ah)) * eps) + sqrt(b) * noise
__global__ void denoise_step_k(const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ noise,
                               const float* __restrict__ alpha, const float* __restrict__ alpha_hat, const float* __restrict__ beta,
                               int step_arg, const int64_t* __restrict__ step_dev, float* __restrict__ out, long n) {
  const int step = step_dev ? (int)step_dev[0] : step_arg;     // device-resident index: a captured graph replays for every i
  const float a = alpha[step], ah = alpha_hat[step], bt = beta[step];
  const float c1 = 1.0f / sqrtf(a);
  const float c2 = (1.0f - a) / sqrtf(1.0f - ah);
  const float sb = sqrtf(bt);
  AFD_GRID_STRIDE(i, n) {
    const float pe = c2 * eps[i];
    const float inner = x[i] - pe;
    const float lhs = c1 * inner;
    const float nz = noise ? sb * noise[i] : 0.0f;       // sqrt(beta) * zeros == +0
    out[i] = lhs + nz;
  }
}

// ---- classifier-free guidance: the guided noise and the update above in one pass ------------------------------------
// eps2 holds the 2n-row forward: element j of the conditional half at j, of the unconditional half at n + j.
// e = torch.lerp(e_u, e_c, s) with ATen's scalar formula (aten/src/ATen/native/Lerp.h), one rounding per operation:
//   |s| < 0.5:  u + s * (c - u)        otherwise:  c - (c - u) * (1 - s)
// then exactly denoise_step_k's expression.  x_out may alias x (elementwise); x_out2 (optional) receives the same values:
// the sampler writes both halves of its 2n input buffer, so the next forward needs no concatenation.
struct CfgCoef {
  float c1, c2, sb, s, one_minus_s;
  bool small;
};
__device__ __forceinline__ CfgCoef cfg_coef(const float* alpha, const float* alpha_hat, const float* beta, int step, float s) {
  const float a = alpha[step], ah = alpha_hat[step], bt = beta[step];
  CfgCoef k;
  k.c1 = 1.0f / sqrtf(a);
  k.c2 = (1.0f - a) / sqrtf(1.0f - ah);
  k.sb = sqrtf(bt);
  k.s = s;
  k.one_minus_s = 1.0f - s;
  k.small = fabsf(s) < 0.5f;
  return k;
}
__device__ __forceinline__ float cfg_lerp(float s, float one_minus_s, bool small, float ec, float eu) {
  const float d = ec - eu;
  return small ? eu + s * d : ec - d * one_minus_s;
}
__device__ __forceinline__ float denoise_update(const CfgCoef& k, float x, float e, float nz_in, bool has_noise) {
  const float pe = k.c2 * e;
  const float inner = x - pe;
  const float lhs = k.c1 * inner;
  const float nz = has_noise ? k.sb * nz_in : 0.0f;
  return lhs + nz;
}
template <bool kCfg>
__device__ __forceinline__ float denoise_eps(const CfgCoef& k, float ec, float eu) {
  return kCfg ? cfg_lerp(k.s, k.one_minus_s, k.small, ec, eu) : ec;
}

// ---- masked step (inpainting, RePaint): the update above for the generated region, x0 noised to t_prev for the known one --
// known = t_prev == 0 ? x0 : (sqrt(a_p) * x0) + (sqrt(1 - a_p) * z), a_p = alpha_hat[t_prev] (noise_images_k's expression)
// out   = mask[j] ? known : gen.  One noise tensor z serves both regions (each element reads its z once).
struct KnownCoef {
  float sa, sb;
  bool clean;
};
__device__ __forceinline__ KnownCoef known_coef(const float* alpha_hat, int tp) {
  const float ah = alpha_hat[tp];
  KnownCoef k;
  k.sa = sqrtf(ah);
  k.sb = sqrtf(1.0f - ah);
  k.clean = tp == 0;
  return k;
}
__device__ __forceinline__ float known_value(const KnownCoef& k, float x0, float z) {
  if (k.clean) return x0;
  const float l = k.sa * x0, r = k.sb * z;
  return l + r;
}
__device__ __forceinline__ float4 masked4(const KnownCoef& k, uchar4 m, float4 x0, float4 z, float4 gen) {
  float4 r;
  r.x = m.x ? known_value(k, x0.x, z.x) : gen.x;
  r.y = m.y ? known_value(k, x0.y, z.y) : gen.y;
  r.z = m.z ? known_value(k, x0.z, z.z) : gen.z;
  r.w = m.w ? known_value(k, x0.w, z.w) : gen.w;
  return r;
}

// Bodies shared by the guided (kCfg) and masked (kMasked) kernels, so the generated region cannot drift from the unmasked
// update.  kMasked: the step is step -> step - 1, and its generated region takes no noise at step 1 (the chain's last step).
// 16-byte accesses (n % 4 == 0, every float pointer 16-byte aligned, mask 4-byte aligned); n4 = n / 4
template <bool kCfg, bool kMasked>
__device__ __forceinline__ void denoise_step_x4_body(long i0, long stride, const float* x, const float* __restrict__ eps, const float* __restrict__ noise,
                                                     const float* __restrict__ alpha, const float* __restrict__ alpha_hat,
                                                     const float* __restrict__ beta, int step_arg, const int64_t* __restrict__ step_dev,
                                                     float s, const float* __restrict__ x0, const uint8_t* __restrict__ mask,
                                                     float* x_out, float* x_out2, long n4) {
  const int step = step_dev ? (int)step_dev[0] : step_arg;
  const CfgCoef k = cfg_coef(alpha, alpha_hat, beta, step, s);
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const float4* ec4 = reinterpret_cast<const float4*>(eps);
  const float4* eu4 = ec4 + n4;                                // read only when kCfg
  const float4* nz4 = reinterpret_cast<const float4*>(noise);
  const bool has_noise = noise != nullptr;
  const bool gen_noise = kMasked ? has_noise && step > 1 : has_noise;
  const KnownCoef kn = kMasked ? known_coef(alpha_hat, step > 0 ? step - 1 : 0) : KnownCoef{};
  for (long i = i0; i < n4; i += stride) {
    const float4 xv = x4[i], c = ec4[i];
    const float4 u = kCfg ? eu4[i] : c;
    const float4 z = has_noise ? nz4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 r;
    r.x = denoise_update(k, xv.x, denoise_eps<kCfg>(k, c.x, u.x), z.x, gen_noise);
    r.y = denoise_update(k, xv.y, denoise_eps<kCfg>(k, c.y, u.y), z.y, gen_noise);
    r.z = denoise_update(k, xv.z, denoise_eps<kCfg>(k, c.z, u.z), z.z, gen_noise);
    r.w = denoise_update(k, xv.w, denoise_eps<kCfg>(k, c.w, u.w), z.w, gen_noise);
    if (kMasked)
      r = masked4(kn, reinterpret_cast<const uchar4*>(mask)[i], reinterpret_cast<const float4*>(x0)[i], z, r);
    reinterpret_cast<float4*>(x_out)[i] = r;
    if (x_out2) reinterpret_cast<float4*>(x_out2)[i] = r;
  }
}
template <bool kCfg, bool kMasked>
__device__ __forceinline__ void denoise_step_body(long i0, long stride, const float* x, const float* __restrict__ eps, const float* __restrict__ noise,
                                                  const float* __restrict__ alpha, const float* __restrict__ alpha_hat,
                                                  const float* __restrict__ beta, int step_arg, const int64_t* __restrict__ step_dev,
                                                  float s, const float* __restrict__ x0, const uint8_t* __restrict__ mask,
                                                  float* x_out, float* x_out2, long n) {
  const int step = step_dev ? (int)step_dev[0] : step_arg;
  const CfgCoef k = cfg_coef(alpha, alpha_hat, beta, step, s);
  const bool has_noise = noise != nullptr;
  const bool gen_noise = kMasked ? has_noise && step > 1 : has_noise;
  const KnownCoef kn = kMasked ? known_coef(alpha_hat, step > 0 ? step - 1 : 0) : KnownCoef{};
  for (long i = i0; i < n; i += stride) {
    const float z = has_noise ? noise[i] : 0.0f;
    float r = denoise_update(k, x[i], denoise_eps<kCfg>(k, eps[i], kCfg ? eps[n + i] : 0.0f), z, gen_noise);
    if (kMasked && mask[i]) r = known_value(kn, x0[i], z);
    x_out[i] = r;
    if (x_out2) x_out2[i] = r;
  }
}

__global__ __launch_bounds__(256) void denoise_step_cfg_x4_k(const float* x, const float* __restrict__ eps2, const float* __restrict__ noise,
                                                             const float* __restrict__ alpha, const float* __restrict__ alpha_hat,
                                                             const float* __restrict__ beta, int step_arg, const int64_t* __restrict__ step_dev,
                                                             float s, float* x_out, float* x_out2, long n4) {
  denoise_step_x4_body<true, false>(AFD_GRID_START, x, eps2, noise, alpha, alpha_hat, beta, step_arg, step_dev, s, nullptr, nullptr, x_out, x_out2, n4);
}
__global__ __launch_bounds__(256) void denoise_step_cfg_k(const float* x, const float* __restrict__ eps2, const float* __restrict__ noise,
                                                          const float* __restrict__ alpha, const float* __restrict__ alpha_hat,
                                                          const float* __restrict__ beta, int step_arg, const int64_t* __restrict__ step_dev,
                                                          float s, float* x_out, float* x_out2, long n) {
  denoise_step_body<true, false>(AFD_GRID_START, x, eps2, noise, alpha, alpha_hat, beta, step_arg, step_dev, s, nullptr, nullptr, x_out, x_out2, n);
}
// masked DDPM step, plain (eps: n elements) or guided (kCfg, eps: 2n)
template <bool kCfg>
__global__ __launch_bounds__(256) void denoise_step_masked_x4_k(const float* x, const float* __restrict__ eps, const float* __restrict__ noise,
                                                                const float* __restrict__ alpha, const float* __restrict__ alpha_hat,
                                                                const float* __restrict__ beta, int step_arg,
                                                                const int64_t* __restrict__ step_dev, float s, const float* __restrict__ x0,
                                                                const uint8_t* __restrict__ mask, float* x_out, float* x_out2, long n4) {
  denoise_step_x4_body<kCfg, true>(AFD_GRID_START, x, eps, noise, alpha, alpha_hat, beta, step_arg, step_dev, s, x0, mask, x_out, x_out2, n4);
}
template <bool kCfg>
__global__ __launch_bounds__(256) void denoise_step_masked_k(const float* x, const float* __restrict__ eps, const float* __restrict__ noise,
                                                             const float* __restrict__ alpha, const float* __restrict__ alpha_hat,
                                                             const float* __restrict__ beta, int step_arg,
                                                             const int64_t* __restrict__ step_dev, float s, const float* __restrict__ x0,
                                                             const uint8_t* __restrict__ mask, float* x_out, float* x_out2, long n) {
  denoise_step_body<kCfg, true>(AFD_GRID_START, x, eps, noise, alpha, alpha_hat, beta, step_arg, step_dev, s, x0, mask, x_out, x_out2, n);
}

static int launch_denoise_step_cfg(const float* x, const float* eps2, const float* noise, const float* alpha, const float* alpha_hat,
                                   const float* beta, int i, const int64_t* t_dev, float s, float* x_out, float* x_out2, long n,
                                   hipStream_t st) {
  auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = n % 4 == 0 && a16(x) && a16(eps2) && a16(x_out) && (!noise || a16(noise)) && (!x_out2 || a16(x_out2));
  const long work = vec ? n / 4 : n;
  const int grid = (int)std::min<long>(2048, std::max<long>(1, (work + 255) / 256));      // memory-bound: grid-stride the rest
  if (vec)
    hipLaunchKernelGGL(denoise_step_cfg_x4_k, dim3(grid), dim3(256), 0, st, x, eps2, noise, alpha, alpha_hat, beta, i, t_dev, s, x_out,
                       x_out2, work);
  else
    hipLaunchKernelGGL(denoise_step_cfg_k, dim3(grid), dim3(256), 0, st, x, eps2, noise, alpha, alpha_hat, beta, i, t_dev, s, x_out,
                       x_out2, n);
  return AFD_OK;
}

// ---- DDIM (Song et al. 2021): one step t -> t_prev of a strided chain ------------------------------------------------
// a_t = alpha_hat[t], a_p = alpha_hat[t_prev]; fp32, one rounding per operation, in this order:
//   x0  = (x - sqrt(1 - a_t) * e) / sqrt(a_t)
//   r   = (1 - a_p) / (1 - a_t)        q = 1 - a_t / a_p
//   var = (eta * eta) * (r * q)        sigma = sqrt(var)        dir = sqrt(max((1 - a_p) - var, 0))
//   out = ((sqrt(a_p) * x0) + (dir * e)) + (noise ? sigma * noise : +0)
// The division by sqrt(a_t) stays a division (a reciprocal would round differently).  With CFG, e is cfg_lerp of the
// conditional (j) and unconditional (n + j) halves of eps2 first.  x_out may alias x; x_out2 is optional (nullptr).
struct DdimCoef {
  float sq1m_at, sq_at, sq_ap, sigma, dir, s, one_minus_s;
  bool small;
};
__device__ __forceinline__ DdimCoef ddim_coef(const float* alpha_hat, int t, int tp, float eta, float s) {
  const float a_t = alpha_hat[t], a_p = alpha_hat[tp];
  DdimCoef k;
  k.sq1m_at = sqrtf(1.0f - a_t);
  k.sq_at = sqrtf(a_t);
  k.sq_ap = sqrtf(a_p);
  const float r = (1.0f - a_p) / (1.0f - a_t);
  const float q = 1.0f - a_t / a_p;
  const float var = (eta * eta) * (r * q);
  k.sigma = sqrtf(var);
  k.dir = sqrtf(fmaxf((1.0f - a_p) - var, 0.0f));
  k.s = s;
  k.one_minus_s = 1.0f - s;
  k.small = fabsf(s) < 0.5f;
  return k;
}
__device__ __forceinline__ float ddim_update(const DdimCoef& k, float x, float e, float z, bool has_noise) {
  const float pe = k.sq1m_at * e;
  const float x0 = (x - pe) / k.sq_at;
  const float mean = (k.sq_ap * x0) + (k.dir * e);
  const float nz = has_noise ? k.sigma * z : 0.0f;
  return mean + nz;
}
template <bool kCfg>
__device__ __forceinline__ float ddim_eps(const DdimCoef& k, float ec, float eu) {
  return kCfg ? cfg_lerp(k.s, k.one_minus_s, k.small, ec, eu) : ec;
}

// Bodies shared by the unmasked and masked (kMasked) kernels.  kMasked: the generated region takes no noise when eta == 0 or
// t_prev == 0; the known region is x0 noised to t_prev (known_value).
// 16-byte accesses (n % 4 == 0, every float pointer 16-byte aligned, mask 4-byte aligned); n4 = n / 4.  kCfg: eps holds 2n
// elements.
template <bool kCfg, bool kMasked>
__device__ __forceinline__ void ddim_step_x4_body(long i0, long stride, const float* x, const float* __restrict__ eps, const float* __restrict__ noise,
                                                  const float* __restrict__ alpha_hat, int t_arg, int tp_arg,
                                                  const int64_t* __restrict__ t_dev, const int64_t* __restrict__ tp_dev, float eta,
                                                  float s, const float* __restrict__ x0, const uint8_t* __restrict__ mask,
                                                  float* x_out, float* x_out2, long n4) {
  const int t = t_dev ? (int)t_dev[0] : t_arg;                 // device-resident indices: a captured graph replays every step
  const int tp = tp_dev ? (int)tp_dev[0] : tp_arg;
  const DdimCoef k = ddim_coef(alpha_hat, t, tp, eta, s);
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const float4* ec4 = reinterpret_cast<const float4*>(eps);
  const float4* eu4 = ec4 + n4;                                // read only when kCfg
  const float4* nz4 = reinterpret_cast<const float4*>(noise);
  const bool has_noise = noise != nullptr;
  const bool gen_noise = kMasked ? has_noise && eta != 0.0f && tp > 0 : has_noise;
  const KnownCoef kn = kMasked ? known_coef(alpha_hat, tp) : KnownCoef{};
  for (long i = i0; i < n4; i += stride) {
    const float4 xv = x4[i], c = ec4[i];
    const float4 u = kCfg ? eu4[i] : c;
    const float4 z = has_noise ? nz4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 r;
    r.x = ddim_update(k, xv.x, ddim_eps<kCfg>(k, c.x, u.x), z.x, gen_noise);
    r.y = ddim_update(k, xv.y, ddim_eps<kCfg>(k, c.y, u.y), z.y, gen_noise);
    r.z = ddim_update(k, xv.z, ddim_eps<kCfg>(k, c.z, u.z), z.z, gen_noise);
    r.w = ddim_update(k, xv.w, ddim_eps<kCfg>(k, c.w, u.w), z.w, gen_noise);
    if (kMasked)
      r = masked4(kn, reinterpret_cast<const uchar4*>(mask)[i], reinterpret_cast<const float4*>(x0)[i], z, r);
    reinterpret_cast<float4*>(x_out)[i] = r;
    if (x_out2) reinterpret_cast<float4*>(x_out2)[i] = r;
  }
}
template <bool kCfg, bool kMasked>
__device__ __forceinline__ void ddim_step_body(long i0, long stride, const float* x, const float* __restrict__ eps, const float* __restrict__ noise,
                                               const float* __restrict__ alpha_hat, int t_arg, int tp_arg,
                                               const int64_t* __restrict__ t_dev, const int64_t* __restrict__ tp_dev, float eta, float s,
                                               const float* __restrict__ x0, const uint8_t* __restrict__ mask, float* x_out,
                                               float* x_out2, long n) {
  const int t = t_dev ? (int)t_dev[0] : t_arg;
  const int tp = tp_dev ? (int)tp_dev[0] : tp_arg;
  const DdimCoef k = ddim_coef(alpha_hat, t, tp, eta, s);
  const bool has_noise = noise != nullptr;
  const bool gen_noise = kMasked ? has_noise && eta != 0.0f && tp > 0 : has_noise;
  const KnownCoef kn = kMasked ? known_coef(alpha_hat, tp) : KnownCoef{};
  for (long i = i0; i < n; i += stride) {
    const float e = ddim_eps<kCfg>(k, eps[i], kCfg ? eps[n + i] : 0.0f);
    const float z = has_noise ? noise[i] : 0.0f;
    float r = ddim_update(k, x[i], e, z, gen_noise);
    if (kMasked && mask[i]) r = known_value(kn, x0[i], z);
    x_out[i] = r;
    if (x_out2) x_out2[i] = r;
  }
}

template <bool kCfg>
__global__ __launch_bounds__(256) void ddim_step_x4_k(const float* x, const float* __restrict__ eps, const float* __restrict__ noise,
                                                      const float* __restrict__ alpha_hat, int t_arg, int tp_arg,
                                                      const int64_t* __restrict__ t_dev, const int64_t* __restrict__ tp_dev, float eta,
                                                      float s, float* x_out, float* x_out2, long n4) {
  ddim_step_x4_body<kCfg, false>(AFD_GRID_START, x, eps, noise, alpha_hat, t_arg, tp_arg, t_dev, tp_dev, eta, s, nullptr, nullptr, x_out, x_out2, n4);
}
template <bool kCfg>
__global__ __launch_bounds__(256) void ddim_step_k(const float* x, const float* __restrict__ eps, const float* __restrict__ noise,
                                                   const float* __restrict__ alpha_hat, int t_arg, int tp_arg,
                                                   const int64_t* __restrict__ t_dev, const int64_t* __restrict__ tp_dev, float eta,
                                                   float s, float* x_out, float* x_out2, long n) {
  ddim_step_body<kCfg, false>(AFD_GRID_START, x, eps, noise, alpha_hat, t_arg, tp_arg, t_dev, tp_dev, eta, s, nullptr, nullptr, x_out, x_out2, n);
}
template <bool kCfg>
__global__ __launch_bounds__(256) void ddim_step_masked_x4_k(const float* x, const float* __restrict__ eps, const float* __restrict__ noise,
                                                             const float* __restrict__ alpha_hat, int t_arg, int tp_arg,
                                                             const int64_t* __restrict__ t_dev, const int64_t* __restrict__ tp_dev,
                                                             float eta, float s, const float* __restrict__ x0,
                                                             const uint8_t* __restrict__ mask, float* x_out, float* x_out2, long n4) {
  ddim_step_x4_body<kCfg, true>(AFD_GRID_START, x, eps, noise, alpha_hat, t_arg, tp_arg, t_dev, tp_dev, eta, s, x0, mask, x_out, x_out2, n4);
}
template <bool kCfg>
__global__ __launch_bounds__(256) void ddim_step_masked_k(const float* x, const float* __restrict__ eps, const float* __restrict__ noise,
                                                          const float* __restrict__ alpha_hat, int t_arg, int tp_arg,
                                                          const int64_t* __restrict__ t_dev, const int64_t* __restrict__ tp_dev,
                                                          float eta, float s, const float* __restrict__ x0,
                                                          const uint8_t* __restrict__ mask, float* x_out, float* x_out2, long n) {
  ddim_step_body<kCfg, true>(AFD_GRID_START, x, eps, noise, alpha_hat, t_arg, tp_arg, t_dev, tp_dev, eta, s, x0, mask, x_out, x_out2, n);
}

template <bool kCfg>
static void launch_ddim_step(const float* x, const float* eps, const float* noise, const float* alpha_hat, int t, int tp,
                             const int64_t* t_dev, const int64_t* tp_dev, float eta, float s, float* x_out, float* x_out2, long n,
                             hipStream_t st) {
  auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = n % 4 == 0 && a16(x) && a16(eps) && a16(x_out) && (!noise || a16(noise)) && (!x_out2 || a16(x_out2));
  const long work = vec ? n / 4 : n;
  const int grid = (int)std::min<long>(2048, std::max<long>(1, (work + 255) / 256));      // memory-bound: grid-stride the rest
  if (vec)
    hipLaunchKernelGGL(ddim_step_x4_k<kCfg>, dim3(grid), dim3(256), 0, st, x, eps, noise, alpha_hat, t, tp, t_dev, tp_dev, eta, s,
                       x_out, x_out2, work);
  else
    hipLaunchKernelGGL(ddim_step_k<kCfg>, dim3(grid), dim3(256), 0, st, x, eps, noise, alpha_hat, t, tp, t_dev, tp_dev, eta, s,
                       x_out, x_out2, n);
}

// one masked launch: the 16-byte kernel when n % 4 == 0 and the pointers allow it, else the scalar one
static inline long step_grid(long work) { return std::min<long>(2048, std::max<long>(1, (work + 255) / 256)); }
static inline bool masked_vec(long n, const float* x, const float* eps, const float* noise, const float* x0, const uint8_t* mask,
                              const float* x_out, const float* x_out2) {
  auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  return n % 4 == 0 && a16(x) && a16(eps) && a16(x0) && a16(x_out) && (!noise || a16(noise)) && (!x_out2 || a16(x_out2)) &&
         (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
}
template <bool kCfg>
static void launch_denoise_step_masked(const float* x, const float* eps, const float* noise, const float* x0, const uint8_t* mask,
                                       const float* alpha, const float* alpha_hat, const float* beta, int i, const int64_t* t_dev,
                                       float s, float* x_out, float* x_out2, long n, hipStream_t st) {
  if (masked_vec(n, x, eps, noise, x0, mask, x_out, x_out2))
    hipLaunchKernelGGL(denoise_step_masked_x4_k<kCfg>, dim3(step_grid(n / 4)), dim3(256), 0, st, x, eps, noise, alpha, alpha_hat,
                       beta, i, t_dev, s, x0, mask, x_out, x_out2, n / 4);
  else
    hipLaunchKernelGGL(denoise_step_masked_k<kCfg>, dim3(step_grid(n)), dim3(256), 0, st, x, eps, noise, alpha, alpha_hat, beta, i,
                       t_dev, s, x0, mask, x_out, x_out2, n);
}
template <bool kCfg>
static void launch_ddim_step_masked(const float* x, const float* eps, const float* noise, const float* x0, const uint8_t* mask,
                                    const float* alpha_hat, int t, int tp, const int64_t* t_dev, const int64_t* tp_dev, float eta,
                                    float s, float* x_out, float* x_out2, long n, hipStream_t st) {
  if (masked_vec(n, x, eps, noise, x0, mask, x_out, x_out2))
    hipLaunchKernelGGL(ddim_step_masked_x4_k<kCfg>, dim3(step_grid(n / 4)), dim3(256), 0, st, x, eps, noise, alpha_hat, t, tp, t_dev,
                       tp_dev, eta, s, x0, mask, x_out, x_out2, n / 4);
  else
    hipLaunchKernelGGL(ddim_step_masked_k<kCfg>, dim3(step_grid(n)), dim3(256), 0, st, x, eps, noise, alpha_hat, t, tp, t_dev, tp_dev,
                       eta, s, x0, mask, x_out, x_out2, n);
}

// ---- renoise: q(x_{t_to} | x_{t_from}) of the forward process in one jump (RePaint's up-move) ---------------------------
// a = alpha_hat[t_to] / alpha_hat[t_from]; out = (sqrt(a) * x) + (sqrt(1 - a) * noise), one rounding per operation.
// x_out may alias x.  VEC: n % 4 == 0 and every pointer 16-byte aligned; then n counts float4s.
template <bool VEC>
__global__ __launch_bounds__(256) void renoise_k(const float* x, const float* __restrict__ noise, const float* __restrict__ alpha_hat,
                                                 int t_from, int t_to, float* x_out, long n) {
  const float a = alpha_hat[t_to] / alpha_hat[t_from];
  const float sa = sqrtf(a), sb = sqrtf(1.0f - a);
  AFD_GRID_STRIDE(i, n) {
    if (VEC) {
      const float4 xv = reinterpret_cast<const float4*>(x)[i], z = reinterpret_cast<const float4*>(noise)[i];
      float4 r;
      r.x = (sa * xv.x) + (sb * z.x);
      r.y = (sa * xv.y) + (sb * z.y);
      r.z = (sa * xv.z) + (sb * z.z);
      r.w = (sa * xv.w) + (sb * z.w);
      reinterpret_cast<float4*>(x_out)[i] = r;
    } else {
      x_out[i] = (sa * x[i]) + (sb * noise[i]);
    }
  }
}

// ---- DPM-Solver++(2M) (Lu et al. 2022): one multistep update t -> t_prev -------------------------------------------------
// coef (device, 5 floats, built on the host per step: Diffusion.dpmpp_coefficients) = [alpha_t, sigma_t, A, B0, B1];
// fp32, one rounding per operation, in this order:
//   x0  = (x - (sigma_t * e)) / alpha_t
//   out = ((A * x) + (B0 * x0)) + (x0_prev ? B1 * x0_prev : +0)        x0_out = x0
// With CFG, e is cfg_lerp of the two halves of eps2 first.  The coefficients are read on the device, so one launch serves the
// eager loop and graph replay.  x_out may alias x; x0_out may be x0_prev itself (each element reads its x0_prev before it
// writes x0_out) but overlaps nothing else; x_out2 is optional.  VEC: n % 4 == 0, every pointer 16-byte aligned; n counts float4s.
struct DpmCoef {
  float alpha, sigma, A, B0, B1, s, one_minus_s;
  bool small;
};
__device__ __forceinline__ float dpmpp_update(const DpmCoef& k, float x, float e, float xp, bool has_prev, float& x0) {
  const float pe = k.sigma * e;
  x0 = (x - pe) / k.alpha;
  const float l = k.A * x, r = k.B0 * x0;
  const float m = l + r;
  const float p = has_prev ? k.B1 * xp : 0.0f;
  return m + p;
}
template <bool kCfg>
__device__ __forceinline__ float dpmpp_eps(const DpmCoef& k, float ec, float eu) {
  return kCfg ? cfg_lerp(k.s, k.one_minus_s, k.small, ec, eu) : ec;
}
template <bool kCfg, bool VEC>
__global__ __launch_bounds__(256) void dpmpp_step_k(const float* x, const float* __restrict__ eps, const float* x0_prev,
                                                    const float* __restrict__ coef, float s, float* x_out, float* x_out2,
                                                    float* x0_out, long n) {
  DpmCoef k;
  k.alpha = coef[0];
  k.sigma = coef[1];
  k.A = coef[2];
  k.B0 = coef[3];
  k.B1 = coef[4];
  k.s = s;
  k.one_minus_s = 1.0f - s;
  k.small = fabsf(s) < 0.5f;
  const bool has_prev = x0_prev != nullptr;
  AFD_GRID_STRIDE(i, n) {
    if (VEC) {
      const float4 xv = reinterpret_cast<const float4*>(x)[i], c = reinterpret_cast<const float4*>(eps)[i];
      const float4 u = kCfg ? reinterpret_cast<const float4*>(eps)[n + i] : c;
      const float4 p = has_prev ? reinterpret_cast<const float4*>(x0_prev)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 r, x0;
      r.x = dpmpp_update(k, xv.x, dpmpp_eps<kCfg>(k, c.x, u.x), p.x, has_prev, x0.x);
      r.y = dpmpp_update(k, xv.y, dpmpp_eps<kCfg>(k, c.y, u.y), p.y, has_prev, x0.y);
      r.z = dpmpp_update(k, xv.z, dpmpp_eps<kCfg>(k, c.z, u.z), p.z, has_prev, x0.z);
      r.w = dpmpp_update(k, xv.w, dpmpp_eps<kCfg>(k, c.w, u.w), p.w, has_prev, x0.w);
      reinterpret_cast<float4*>(x_out)[i] = r;
      if (x_out2) reinterpret_cast<float4*>(x_out2)[i] = r;
      reinterpret_cast<float4*>(x0_out)[i] = x0;
    } else {
      float x0;
      const float e = dpmpp_eps<kCfg>(k, eps[i], kCfg ? eps[n + i] : 0.0f);
      const float r = dpmpp_update(k, x[i], e, has_prev ? x0_prev[i] : 0.0f, has_prev, x0);
      x_out[i] = r;
      if (x_out2) x_out2[i] = r;
      x0_out[i] = x0;
    }
  }
}
template <bool kCfg>
static void launch_dpmpp_step(const float* x, const float* eps, const float* x0_prev, const float* coef, float s, float* x_out,
                              float* x_out2, float* x0_out, long n, hipStream_t st) {
  auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = n % 4 == 0 && a16(x) && a16(eps) && a16(x_out) && a16(x0_out) && (!x0_prev || a16(x0_prev)) &&
                   (!x_out2 || a16(x_out2));
  const long work = vec ? n / 4 : n;
  const int grid = (int)std::min<long>(2048, std::max<long>(1, (work + 255) / 256));      // memory-bound: grid-stride the rest
  if (vec)
    hipLaunchKernelGGL((dpmpp_step_k<kCfg, true>), dim3(grid), dim3(256), 0, st, x, eps, x0_prev, coef, s, x_out, x_out2, x0_out, work);
  else
    hipLaunchKernelGGL((dpmpp_step_k<kCfg, false>), dim3(grid), dim3(256), 0, st, x, eps, x0_prev, coef, s, x_out, x_out2, x0_out, n);
}

// ---- likelihood (bits/dim, Ho et al. 2020 section 3.3): gathered noising, the bound's per-row terms, the prior ------------
// A row r pairs image img[r] of x0 with timestep t[r].  Every kernel below walks rows with whole workgroups (a row's
// coefficients are wave-uniform) and the row's `per` values with the threads; VEC: per % 4 == 0 and the float pointers
// 16-byte aligned, so every row starts on a 16-byte boundary; `per` then counts float4s.

// x_t[r] = sqrt(ah[t[r]]) * x0[img[r]] + sqrt(1 - ah[t[r]]) * eps[r]: noise_images_k's expression, operation for operation
template <bool VEC>
__global__ __launch_bounds__(256) void noise_images_gather_k(const float* __restrict__ x0, const int64_t* __restrict__ img,
                                                             const float* __restrict__ eps, const int64_t* __restrict__ t,
                                                             const float* __restrict__ alpha_hat, float* __restrict__ xt, long rows,
                                                             long per) {
  for (long r = blockIdx.x; r < rows; r += gridDim.x) {
    const float ah = alpha_hat[t[r]];
    const float sa = sqrtf(ah);
    const float sb = sqrtf(1.0f - ah);
    const long src = img[r] * per, dst = r * per;
    for (long j = threadIdx.x; j < per; j += blockDim.x) {
      if (VEC) {
        const float4 x = reinterpret_cast<const float4*>(x0)[src + j], e = reinterpret_cast<const float4*>(eps)[dst + j];
        float4 o;
        { const float l = sa * x.x, q = sb * e.x; o.x = l + q; }
        { const float l = sa * x.y, q = sb * e.y; o.y = l + q; }
        { const float l = sa * x.z, q = sb * e.z; o.z = l + q; }
        { const float l = sa * x.w, q = sb * e.w; o.w = l + q; }
        reinterpret_cast<float4*>(xt)[dst + j] = o;
      } else {
        const float l = sa * x0[src + j], q = sb * eps[dst + j];
        xt[dst + j] = l + q;
      }
    }
  }
}

// Sum of two fp64 values over a 256-thread workgroup in a fixed order: a shuffle tree inside each wave, then the four waves'
// partial sums in wave order.  The result is valid in thread 0.  red: 8 doubles of LDS.
__device__ __forceinline__ void block_sum2_f64(double& a, double& b, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_down(a, o, kWave);
    b += __shfl_down(b, o, kWave);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[2 * w] = a;
    red[2 * w + 1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = red[0];
    b = red[1];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) {
      a += red[2 * i];
      b += red[2 * i + 1];
    }
  }
}

// Ho et al.'s discretised Gaussian, log p of the 8-bit level x0 under N(mean, exp(2 log_scale)), in fp64: bins of half-width
// 1/255, the edge bins open below -0.999 and above 0.999, Phi by the tanh approximation, probabilities clamped at 1e-12.
__device__ __forceinline__ double approx_std_normal_cdf(double x) {
  return 0.5 * (1.0 + tanh(0.7978845608028654 * (x + 0.044715 * (x * x * x))));     // sqrt(2 / pi)
}
__device__ __forceinline__ double decoder_log_prob(double x, double mean, double inv_stdv) {
  const double c = x - mean;
  const double cdf_plus = approx_std_normal_cdf(inv_stdv * (c + 1.0 / 255.0));
  const double cdf_min = approx_std_normal_cdf(inv_stdv * (c - 1.0 / 255.0));
  if (x < -0.999) return log(fmax(cdf_plus, 1e-12));
  if (x > 0.999) return log(fmax(1.0 - cdf_min, 1e-12));
  return log(fmax(cdf_plus - cdf_min, 1e-12));
}

// One workgroup per row.  coef: the (T, 4) fp64 table of Diffusion.vlb_coefficients, row t = [w_t, c_t, log_scale_t, prior].
//   sq[r]   = sum_j (double(eps_hat_j) - double(eps_j))^2
//   term[r] = w_t * sq[r] + per * c_t                                                       t != 1: KL(q || p_theta)
//           = -sum_j decoder_log_prob(x0_j, mean_j, exp(-log_scale_1)),                    t == 1: the decoder
// with mean_j = denoise_step_k's fp32 expression at step 1 without noise, c1 * (x_t - c2 * eps_hat) (what the sampler returns).
// Only decoder rows read x0 and x_t.  Each thread sums its elements in index order (x, y, z, w within a float4).
template <bool VEC>
__global__ __launch_bounds__(256) void vlb_terms_k(const float* __restrict__ x0, const int64_t* __restrict__ img,
                                                   const float* __restrict__ xt, const float* __restrict__ eps,
                                                   const float* __restrict__ eps_hat, const int64_t* __restrict__ t,
                                                   const double* __restrict__ coef, const float* __restrict__ alpha,
                                                   const float* __restrict__ alpha_hat, const float* __restrict__ beta,
                                                   double* __restrict__ term, double* __restrict__ sq, long per, long n_elem) {
  __shared__ double red[8];
  const long r = blockIdx.x;
  const int tr = (int)t[r];
  const long row = r * per;
  double s_sq = 0.0, s_ll = 0.0;
  if (tr == 1) {                                    // uniform per workgroup
    const CfgCoef k = cfg_coef(alpha, alpha_hat, beta, 1, 0.0f);
    const double inv_stdv = exp(-coef[4 * 1 + 2]);              // row t = 1, log_scale
    const long src = img[r] * per;
    for (long j = threadIdx.x; j < per; j += blockDim.x) {
      if (VEC) {
        const float4 e = reinterpret_cast<const float4*>(eps)[row + j], h = reinterpret_cast<const float4*>(eps_hat)[row + j];
        const float4 x = reinterpret_cast<const float4*>(xt)[row + j], v = reinterpret_cast<const float4*>(x0)[src + j];
        const float ev[4] = {e.x, e.y, e.z, e.w}, hv[4] = {h.x, h.y, h.z, h.w}, xv[4] = {x.x, x.y, x.z, x.w};
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double d = (double)hv[q] - (double)ev[q];
          s_sq += d * d;
          s_ll += decoder_log_prob(vv[q], denoise_update(k, xv[q], hv[q], 0.0f, false), inv_stdv);
        }
      } else {
        const double d = (double)eps_hat[row + j] - (double)eps[row + j];
        s_sq += d * d;
        s_ll += decoder_log_prob(x0[src + j], denoise_update(k, xt[row + j], eps_hat[row + j], 0.0f, false), inv_stdv);
      }
    }
  } else {
    for (long j = threadIdx.x; j < per; j += blockDim.x) {
      if (VEC) {
        const float4 e = reinterpret_cast<const float4*>(eps)[row + j], h = reinterpret_cast<const float4*>(eps_hat)[row + j];
        const double dx = (double)h.x - (double)e.x, dy = (double)h.y - (double)e.y;
        const double dz = (double)h.z - (double)e.z, dw = (double)h.w - (double)e.w;
        s_sq += dx * dx;
        s_sq += dy * dy;
        s_sq += dz * dz;
        s_sq += dw * dw;
      } else {
        const double d = (double)eps_hat[row + j] - (double)eps[row + j];
        s_sq += d * d;
      }
    }
  }
  block_sum2_f64(s_sq, s_ll, red);
  if (threadIdx.x == 0) {
    const double* c = coef + 4 * (long)tr;
    term[r] = tr == 1 ? -s_ll : c[0] * s_sq + (double)n_elem * c[1];
    sq[r] = s_sq;
  }
}

// out[i] = half_ah * sum_j x0[i, j]^2 in fp64 (the data-dependent part of KL(q(x_{T-1} | x0) || N(0, I))); one workgroup per image
template <bool VEC>
__global__ __launch_bounds__(256) void vlb_prior_k(const float* __restrict__ x0, double half_ah, double* __restrict__ out, long per) {
  __shared__ double red[8];
  const long row = blockIdx.x * per;
  double s = 0.0, unused = 0.0;
  for (long j = threadIdx.x; j < per; j += blockDim.x) {
    if (VEC) {
      const float4 v = reinterpret_cast<const float4*>(x0)[row + j];
      s += (double)v.x * (double)v.x;
      s += (double)v.y * (double)v.y;
      s += (double)v.z * (double)v.z;
      s += (double)v.w * (double)v.w;
    } else {
      const double v = x0[row + j];
      s += v * v;
    }
  }
  block_sum2_f64(s, unused, red);
  if (threadIdx.x == 0) out[blockIdx.x] = half_ah * s;
}

// ((clamp(x,-1,1) + 1) / 2 * 255).type(uint8): truncation toward zero
__global__ void quantize_u8_k(const float* __restrict__ x, uint8_t* __restrict__ out, long n) {
  AFD_GRID_STRIDE(i, n) {
    float v = x[i];
    v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);            // NaN passes through like torch.clamp
    v = ((v + 1.0f) / 2.0f) * 255.0f;
    out[i] = (uint8_t)(int)v;
  }
}

// ---- MSE ------------------------------------------------------------------------------------
constexpr int kMseBlocks = 1024;
__global__ void mse_partial_k(const float* __restrict__ p, const float* __restrict__ t, float* __restrict__ part, long n) {
  __shared__ float red[16];
  float s = 0.f;
  AFD_GRID_STRIDE(i, n) { const float d = p[i] - t[i]; s += d * d; }
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ void mse_final_k(const float* __restrict__ part, float* __restrict__ loss, int nparts, float inv_n) {
  __shared__ float red[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) s += part[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) loss[0] = s * inv_n;
}
__global__ void mse_bwd_k(const float* __restrict__ p, const float* __restrict__ t, const float* __restrict__ dloss,
                          float* __restrict__ dp, long n, float two_over_n) {
  const float g = dloss[0] * two_over_n;
  AFD_GRID_STRIDE(i, n) dp[i] = (p[i] - t[i]) * g;
}

// ---- training objectives: eps / v / x0 prediction with a per-timestep loss weight ----------------------------------------
// Work item = (row b, segment g): the 256 threads of a workgroup take the 256 quads [4 q, 4 q + 4) of row b with
// q = 256 g + threadIdx.x, so sqrt(a), sqrt(1 - a) (noise_images_k's two expressions) and w[t_b] are read once per item and
// are uniform over the workgroup.  VEC (chw % 4 == 0, 16-byte aligned pointers): one 128-bit access per stream; otherwise the
// same quad element by element -- every thread sees the same values in the same order in both forms, so their results are
// bit-identical.  Streaming, 12-16 bytes per element: at B = 256, chw = 3072 this is 768 items, three workgroups per CU.
constexpr int kObjBlocks = 1024;      // cap on the partial sums (the workspace holds 4096 floats, as for mse)

// target: eps (AFD_PRED_EPS), sqrt(a) eps - sqrt(1 - a) x0 (AFD_PRED_V), x0 (AFD_PRED_X0); -> pred - target
__device__ __forceinline__ float objective_diff(int kind, float p, float x0, float e, float sa, float sb) {
  if (kind == AFD_PRED_V) {
    const float l = sa * e, r = sb * x0;
    return p - (l - r);
  }
  return p - (kind == AFD_PRED_X0 ? x0 : e);
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

// part[blockIdx.x] = sum over the workgroup's items of w[t_b] * sum_i (pred - target)^2: per thread in item order, then the
// workgroup's fixed tree (block_sum); mse_final_k sums the partials.  x0 (eps) is not read for AFD_PRED_EPS (AFD_PRED_X0).
template <bool VEC>
__global__ __launch_bounds__(256) void objective_partial_k(const float* __restrict__ pred, const float* __restrict__ x0,
                                                           const float* __restrict__ eps, const int64_t* __restrict__ t,
                                                           const float* __restrict__ alpha_hat, const float* __restrict__ w, int kind,
                                                           float* __restrict__ part, long items, long segs, long chw) {
  __shared__ float red[16];
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float s = 0.f;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const long b = it / segs, q = (it - b * segs) * 256 + threadIdx.x;
    const long tb = t[b], left = chw - 4 * q, o = b * chw + 4 * q;
    const float ah = alpha_hat[tb];
    const float sa = sqrtf(ah), sb = sqrtf(1.0f - ah);
    const float wb = w ? w[tb] : 1.0f;
    if (left <= 0) continue;
    const float4 p = load_quad<VEC>(pred, o, left);
    const float4 x = kind != AFD_PRED_EPS ? load_quad<VEC>(x0, o, left) : zero;
    const float4 e = kind != AFD_PRED_X0 ? load_quad<VEC>(eps, o, left) : zero;
    const float dx = objective_diff(kind, p.x, x.x, e.x, sa, sb), dy = objective_diff(kind, p.y, x.y, e.y, sa, sb);
    const float dz = objective_diff(kind, p.z, x.z, e.z, sa, sb), dw = objective_diff(kind, p.w, x.w, e.w, sa, sb);
    float r = dx * dx;
    if (left > 1) r += dy * dy;        // (a value past the row's end may be anything, NaN included: it is never added)
    if (left > 2) r += dz * dz;
    if (left > 3) r += dw * dw;
    s += wb * r;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// dpred = (dloss * 2 / (B chw) * w[t_b]) * (pred - target), the target recomputed; with w NULL and AFD_PRED_EPS: mse_bwd_k's values
template <bool VEC>
__global__ __launch_bounds__(256) void objective_bwd_k(const float* __restrict__ pred, const float* __restrict__ x0,
                                                       const float* __restrict__ eps, const int64_t* __restrict__ t,
                                                       const float* __restrict__ alpha_hat, const float* __restrict__ w, int kind,
                                                       const float* __restrict__ dloss, float* __restrict__ dpred, long items,
                                                       long segs, long chw, float two_over_n) {
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const float g0 = dloss[0] * two_over_n;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const long b = it / segs, q = (it - b * segs) * 256 + threadIdx.x;
    const long tb = t[b], left = chw - 4 * q, o = b * chw + 4 * q;
    const float ah = alpha_hat[tb];
    const float sa = sqrtf(ah), sb = sqrtf(1.0f - ah);
    const float g = w ? g0 * w[tb] : g0;
    if (left <= 0) continue;
    const float4 p = load_quad<VEC>(pred, o, left);
    const float4 x = kind != AFD_PRED_EPS ? load_quad<VEC>(x0, o, left) : zero;
    const float4 e = kind != AFD_PRED_X0 ? load_quad<VEC>(eps, o, left) : zero;
    float4 d;
    d.x = objective_diff(kind, p.x, x.x, e.x, sa, sb) * g;
    d.y = objective_diff(kind, p.y, x.y, e.y, sa, sb) * g;
    d.z = objective_diff(kind, p.z, x.z, e.z, sa, sb) * g;
    d.w = objective_diff(kind, p.w, x.w, e.w, sa, sb) * g;
    store_quad<VEC>(dpred, o, left, d);
  }
}

// the network's output -> eps, per row t: v: (sqrt(a) v) + (sqrt(1 - a) x_t);  x0: (x_t - sqrt(a) x0) / sqrt(1 - a).
// eps_out may be `out` itself (elementwise: every thread reads its quad before it writes it), hence no __restrict__ on them.
template <bool VEC>
__global__ __launch_bounds__(256) void pred_to_eps_k(const float* out, const float* __restrict__ xt, const int64_t* __restrict__ t,
                                                     const float* __restrict__ alpha_hat, int kind, float* eps_out, long items,
                                                     long segs, long chw) {
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const long b = it / segs, q = (it - b * segs) * 256 + threadIdx.x;
    const long left = chw - 4 * q, o = b * chw + 4 * q;
    const float ah = alpha_hat[t[b]];
    const float sa = sqrtf(ah), sb = sqrtf(1.0f - ah);
    if (left <= 0) continue;
    const float4 v = load_quad<VEC>(out, o, left), x = load_quad<VEC>(xt, o, left);
    float4 e;
    if (kind == AFD_PRED_V) {
      { const float l = sa * v.x, r = sb * x.x; e.x = l + r; }
      { const float l = sa * v.y, r = sb * x.y; e.y = l + r; }
      { const float l = sa * v.z, r = sb * x.z; e.z = l + r; }
      { const float l = sa * v.w, r = sb * x.w; e.w = l + r; }
    } else {
      { const float l = sa * v.x; e.x = (x.x - l) / sb; }
      { const float l = sa * v.y; e.y = (x.y - l) / sb; }
      { const float l = sa * v.z; e.z = (x.z - l) / sb; }
      { const float l = sa * v.w; e.w = (x.w - l) / sb; }
    }
    store_quad<VEC>(eps_out, o, left, e);
  }
}

// ---- learned reverse-process variances (Nichol & Dhariwal 2021): hybrid loss, ancestral step, bound ---------------------------
// The network's output row b holds 2 chw floats: the prediction p (eps, v or x0) and, chw floats later, the coefficient v of
//   logvar = ((v + 1) / 2) lb_t + (1 - (v + 1) / 2) lbt_t,      lb_t = log beta_t, lbt_t = log beta~_t
// lv_coef: the (T, 3) fp64 table [lb_t, lbt_t, k_t] of Diffusion.lvar_coefficients, k_t = beta_t^2 / (alpha_t (1 - ah_t)).
// Every per-element term and dL/dv is evaluated in fp64 from the fp32 inputs (in fp32, -1 + x + exp(-x) cancels), x + expm1(-x)
// in place of -1 + x + exp(-x).  The device functions below are shared by the loss kernels and the bound kernel.
__device__ __forceinline__ double lvar_logvar(double v, double lb, double lbt) {
  const double f = (v + 1.0) / 2.0;
  const double l = f * lb, r = (1.0 - f) * lbt;
  return l + r;
}
// pred - target in fp64 from the fp32 inputs, sa = sqrt(a), sb = sqrt(1 - a) of the widened a = alpha_hat[t]
__device__ __forceinline__ double lvar_diff(int kind, float p, float x0, float e, double sa, double sb) {
  if (kind == AFD_PRED_V) {
    const double l = sa * (double)e, r = sb * (double)x0;
    return (double)p - (l - r);
  }
  return (double)p - (double)(kind == AFD_PRED_X0 ? x0 : e);
}
// (eps_hat - eps)^2 = f2 (pred - target)^2: f2 = 1 (eps), a (v), a / (1 - a) (x0)
__device__ __forceinline__ double lvar_f2(int kind, double a) {
  return kind == AFD_PRED_V ? a : (kind == AFD_PRED_X0 ? a / (1.0 - a) : 1.0);
}
// the output -> eps in fp32: pred_to_eps_k's expressions
__device__ __forceinline__ float lvar_eps_hat(int kind, float p, float xt, float sa, float sb) {
  if (kind == AFD_PRED_V) {
    const float l = sa * p, r = sb * xt;
    return l + r;
  }
  if (kind == AFD_PRED_X0) {
    const float l = sa * p;
    return (xt - l) / sb;
  }
  return p;
}
// KL(q(x_{t-1} | x_t, x0) || p_theta) per element, t >= 2, nats, with the mean's part in its d-form k_t d^2 exp(-logvar);
// GRAD: dlv = d term / d logvar
template <bool GRAD>
__device__ __forceinline__ double lvar_kl(double d2, double v, double lb, double lbt, double kt, double& dlv) {
  const double lv = lvar_logvar(v, lb, lbt);
  const double x = lv - lbt;
  const double em = expm1(-x);
  const double q = (kt * d2) * exp(-lv);
  if (GRAD) dlv = 0.5 * (-em - q);
  return 0.5 * ((x + em) + q);
}
// d Phi / d z of approx_std_normal_cdf
__device__ __forceinline__ double approx_std_normal_cdf_slope(double z) {
  const double th = tanh(0.7978845608028654 * (z + 0.044715 * (z * z * z)));
  return (0.5 * (1.0 - th * th)) * (0.7978845608028654 * (1.0 + (3.0 * 0.044715) * (z * z)));
}
// -decoder_log_prob(x, mean, exp(-logvar / 2)) with a per-element logvar; GRAD: dlv = d term / d logvar through the tanh
// CDFs (z = exp(-logvar / 2) (c -+ 1/255), dz / dlogvar = -z / 2), zero where the 1e-12 clamp is active (as torch.clamp)
template <bool GRAD>
__device__ __forceinline__ double lvar_decoder(double x, double mean, double v, double lb, double lbt, double& dlv) {
  const double inv_stdv = exp(-(lvar_logvar(v, lb, lbt) / 2.0));
  const double c = x - mean;
  const double zp = inv_stdv * (c + 1.0 / 255.0), zm = inv_stdv * (c - 1.0 / 255.0);
  const double cp = approx_std_normal_cdf(zp), cm = approx_std_normal_cdf(zm);
  const bool lo = x < -0.999, hi = x > 0.999;
  const double P = lo ? cp : (hi ? 1.0 - cm : cp - cm);
  if (GRAD) {
    const double gp = hi ? 0.0 : approx_std_normal_cdf_slope(zp) * zp;
    const double gm = lo ? 0.0 : approx_std_normal_cdf_slope(zm) * zm;
    dlv = P >= 1e-12 ? (0.5 * (gp - gm)) / P : 0.0;
  }
  return -log(fmax(P, 1e-12));
}
// the bound's term of one element (GRAD: and d term / d logvar) and sq = (eps_hat - eps)^2; dec: the row is t = 1
struct LvarRow {
  double lb, lbt, kt, sa64, sb64, f2;
  float sa, sb;            // noise_images_k's two roots
  CfgCoef dec;             // denoise_step_k's coefficients at step 1
  bool is_dec;
};
__device__ __forceinline__ LvarRow lvar_row(const double* __restrict__ lv_coef, const float* __restrict__ alpha,
                                            const float* __restrict__ alpha_hat, const float* __restrict__ beta, long t, int kind) {
  LvarRow w;
  const float ah = alpha_hat[t];
  w.sa = sqrtf(ah);
  w.sb = sqrtf(1.0f - ah);
  const double a = (double)ah;
  w.sa64 = sqrt(a);
  w.sb64 = sqrt(1.0 - a);
  w.f2 = lvar_f2(kind, a);
  w.lb = lv_coef[3 * t];
  w.lbt = lv_coef[3 * t + 1];
  w.kt = lv_coef[3 * t + 2];
  w.is_dec = t == 1;
  w.dec = cfg_coef(alpha, alpha_hat, beta, 1, 0.0f);
  return w;
}
template <bool GRAD>
__device__ __forceinline__ double lvar_term(const LvarRow& w, int kind, float p, float v, float x0, float e, float xt, double& sq,
                                            double& dlv) {
  const double df = lvar_diff(kind, p, x0, e, w.sa64, w.sb64);
  sq = w.f2 * (df * df);
  if (w.is_dec) {
    const float mean = denoise_update(w.dec, xt, lvar_eps_hat(kind, p, xt, w.sa, w.sb), 0.0f, false);
    return lvar_decoder<GRAD>((double)x0, (double)mean, (double)v, w.lb, w.lbt, dlv);
  }
  return lvar_kl<GRAD>(sq, (double)v, w.lb, w.lbt, w.kt, dlv);
}
__device__ __forceinline__ float noised(float sa, float sb, float x0, float e) {      // noise_images_k's expression
  const float l = sa * x0, r = sb * e;
  return l + r;
}

// Work items as objective_partial_k.  part_s[blockIdx.x]: objective_partial_k's sum over the p half (L_simple, bit for bit);
// part_v[blockIdx.x]: the fp64 sum of the bound's terms, per thread in item and element order, then the workgroup's fixed tree.
template <bool VEC>
__global__ __launch_bounds__(256) void lvar_partial_k(const float* __restrict__ out2, const float* __restrict__ x0,
                                                      const float* __restrict__ eps, const int64_t* __restrict__ t,
                                                      const float* __restrict__ alpha, const float* __restrict__ alpha_hat,
                                                      const float* __restrict__ beta, const double* __restrict__ lv_coef,
                                                      const float* __restrict__ w, int kind, float* __restrict__ part_s,
                                                      double* __restrict__ part_v, long items, long segs, long chw) {
  __shared__ float red[16];
  __shared__ double red2[8];
  float s = 0.f;
  double sv = 0.0, unused = 0.0;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const long b = it / segs, q = (it - b * segs) * 256 + threadIdx.x;
    const long tb = t[b], left = chw - 4 * q, o = b * chw + 4 * q, op = 2 * b * chw + 4 * q;
    const LvarRow row = lvar_row(lv_coef, alpha, alpha_hat, beta, tb, kind);
    const float wb = w ? w[tb] : 1.0f;
    if (left <= 0) continue;
    const float4 p = load_quad<VEC>(out2, op, left), v = load_quad<VEC>(out2, op + chw, left);
    const float4 x = load_quad<VEC>(x0, o, left), e = load_quad<VEC>(eps, o, left);
    const float dx = objective_diff(kind, p.x, x.x, e.x, row.sa, row.sb), dy = objective_diff(kind, p.y, x.y, e.y, row.sa, row.sb);
    const float dz = objective_diff(kind, p.z, x.z, e.z, row.sa, row.sb), dw = objective_diff(kind, p.w, x.w, e.w, row.sa, row.sb);
    float r = dx * dx;
    if (left > 1) r += dy * dy;
    if (left > 2) r += dz * dz;
    if (left > 3) r += dw * dw;
    s += wb * r;
    const float pv[4] = {p.x, p.y, p.z, p.w}, vv[4] = {v.x, v.y, v.z, v.w}, xv[4] = {x.x, x.y, x.z, x.w}, ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < left) {
        double sq, dlv;
        sv += lvar_term<false>(row, kind, pv[i], vv[i], xv[i], ev[i], noised(row.sa, row.sb, xv[i], ev[i]), sq, dlv);
      }
    }
  }
  s = block_sum(s, red);
  block_sum2_f64(sv, unused, red2);
  if (threadIdx.x == 0) {
    part_s[blockIdx.x] = s;
    part_v[blockIdx.x] = sv;
  }
}
// loss_out = {L, L_vlb} in fp32, sums_out (optional) the same two in fp64:
//   L_simple = mse_final_k's value, L_vlb = sum / (N ln 2), L = L_simple + vlb_scale L_vlb
__global__ __launch_bounds__(256) void lvar_final_k(const float* __restrict__ part_s, const double* __restrict__ part_v, int nparts,
                                                    float inv_n, double n_ln2, double vlb_scale, float* __restrict__ loss_out,
                                                    double* __restrict__ sums_out) {
  __shared__ float red[16];
  __shared__ double red2[8];
  float s = 0.f;
  double sv = 0.0, unused = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
    s += part_s[i];
    sv += part_v[i];
  }
  s = block_sum(s, red);
  block_sum2_f64(sv, unused, red2);
  if (threadIdx.x == 0) {
    const double ls = (double)(s * inv_n), lv = sv / n_ln2, l = ls + vlb_scale * lv;
    loss_out[0] = (float)l;
    loss_out[1] = (float)lv;
    if (sums_out) {
      sums_out[0] = l;
      sums_out[1] = lv;
    }
  }
}
// dout2: the p half is objective_bwd_k's dpred (L_simple alone: the mean is stopped in L_vlb); the v half is
// (float)(dloss gv (d term / d logvar) (lb - lbt) / 2), gv = vlb_scale / (N ln 2), in fp64 and rounded once
template <bool VEC>
__global__ __launch_bounds__(256) void lvar_bwd_k(const float* __restrict__ out2, const float* __restrict__ x0,
                                                  const float* __restrict__ eps, const int64_t* __restrict__ t,
                                                  const float* __restrict__ alpha, const float* __restrict__ alpha_hat,
                                                  const float* __restrict__ beta, const double* __restrict__ lv_coef,
                                                  const float* __restrict__ w, int kind, const float* __restrict__ dloss,
                                                  float* __restrict__ dout2, long items, long segs, long chw, float two_over_n,
                                                  double gv) {
  const float g0 = dloss[0] * two_over_n;
  const double gd = (double)dloss[0] * gv;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const long b = it / segs, q = (it - b * segs) * 256 + threadIdx.x;
    const long tb = t[b], left = chw - 4 * q, o = b * chw + 4 * q, op = 2 * b * chw + 4 * q;
    const LvarRow row = lvar_row(lv_coef, alpha, alpha_hat, beta, tb, kind);
    const float g = w ? g0 * w[tb] : g0;
    const double gl = gd * ((row.lb - row.lbt) / 2.0);
    if (left <= 0) continue;
    const float4 p = load_quad<VEC>(out2, op, left), v = load_quad<VEC>(out2, op + chw, left);
    const float4 x = load_quad<VEC>(x0, o, left), e = load_quad<VEC>(eps, o, left);
    float4 d;
    d.x = objective_diff(kind, p.x, x.x, e.x, row.sa, row.sb) * g;
    d.y = objective_diff(kind, p.y, x.y, e.y, row.sa, row.sb) * g;
    d.z = objective_diff(kind, p.z, x.z, e.z, row.sa, row.sb) * g;
    d.w = objective_diff(kind, p.w, x.w, e.w, row.sa, row.sb) * g;
    store_quad<VEC>(dout2, op, left, d);
    const float pv[4] = {p.x, p.y, p.z, p.w}, vv[4] = {v.x, v.y, v.z, v.w}, xv[4] = {x.x, x.y, x.z, x.w}, ev[4] = {e.x, e.y, e.z, e.w};
    float dv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < left) {
        double sq, dlv;
        lvar_term<true>(row, kind, pv[i], vv[i], xv[i], ev[i], noised(row.sa, row.sb, xv[i], ev[i]), sq, dlv);
        dv[i] = (float)(gl * dlv);
      }
    }
    store_quad<VEC>(dout2, op + chw, left, make_float4(dv[0], dv[1], dv[2], dv[3]));
  }
}

// out2 (B rows of 2 chw) -> eps_out (B x chw; pred_to_eps_k's conversion, a copy for AFD_PRED_EPS) and, optionally, the v half
template <bool VEC>
__global__ __launch_bounds__(256) void split_pred_k(const float* __restrict__ out2, const float* __restrict__ xt,
                                                    const int64_t* __restrict__ t, const float* __restrict__ alpha_hat, int kind,
                                                    float* __restrict__ eps_out, float* __restrict__ v_out, long items, long segs,
                                                    long chw) {
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const long b = it / segs, q = (it - b * segs) * 256 + threadIdx.x;
    const long left = chw - 4 * q, o = b * chw + 4 * q, op = 2 * b * chw + 4 * q;
    const float ah = kind != AFD_PRED_EPS ? alpha_hat[t[b]] : 0.0f;
    const float sa = sqrtf(ah), sb = sqrtf(1.0f - ah);
    if (left <= 0) continue;
    const float4 p = load_quad<VEC>(out2, op, left);
    float4 r = p;
    if (kind != AFD_PRED_EPS) {
      const float4 x = load_quad<VEC>(xt, o, left);
      r.x = lvar_eps_hat(kind, p.x, x.x, sa, sb);
      r.y = lvar_eps_hat(kind, p.y, x.y, sa, sb);
      r.z = lvar_eps_hat(kind, p.z, x.z, sa, sb);
      r.w = lvar_eps_hat(kind, p.w, x.w, sa, sb);
    }
    store_quad<VEC>(eps_out, o, left, r);
    if (v_out) store_quad<VEC>(v_out, o, left, load_quad<VEC>(out2, op + chw, left));
  }
}

// Ancestral step with the learned variance: eps_hat from p (pred_to_eps_k's expression at x, per step), guided (kCfg: out2 holds
// 2 B rows, conditional then unconditional; cfg_lerp of the two eps; the variance from the conditional row), then
//   x_out = c1 (x - c2 eps_hat) + (float)exp(logvar / 2) noise,  denoise_step_k's mean; no noise at step 1 or with noise NULL.
// x_out may be x itself (each thread reads its quad before it writes it); x_out2 (optional) receives the same values.
__device__ __forceinline__ float lvar_update(const CfgCoef& k, float x, float e, float v, float z, double lb, double lbt, bool has_noise) {
  const float pe = k.c2 * e;
  const float inner = x - pe;
  const float lhs = k.c1 * inner;
  if (!has_noise) return lhs + 0.0f;
  const float sd = (float)exp(lvar_logvar((double)v, lb, lbt) / 2.0);
  return lhs + sd * z;
}
template <bool kCfg, bool VEC>
__global__ __launch_bounds__(256) void lvar_step_k(const float* x, const float* __restrict__ out2, const float* __restrict__ noise,
                                                   const float* __restrict__ alpha, const float* __restrict__ alpha_hat,
                                                   const float* __restrict__ beta, const double* __restrict__ lv_coef, int kind,
                                                   int step_arg, const int64_t* __restrict__ step_dev, float s, float* x_out,
                                                   float* x_out2, long items, long segs, long chw, long B) {
  const int step = step_dev ? (int)step_dev[0] : step_arg;
  const CfgCoef k = cfg_coef(alpha, alpha_hat, beta, step, s);
  const float ah = alpha_hat[step];
  const float sa = sqrtf(ah), sb = sqrtf(1.0f - ah);
  const double lb = lv_coef[3 * (long)step], lbt = lv_coef[3 * (long)step + 1];
  const bool has_noise = noise != nullptr && step > 1;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const long b = it / segs, q = (it - b * segs) * 256 + threadIdx.x;
    const long left = chw - 4 * q, o = b * chw + 4 * q, op = 2 * b * chw + 4 * q;
    if (left <= 0) continue;
    const float4 xv = load_quad<VEC>(x, o, left), c = load_quad<VEC>(out2, op, left), v = load_quad<VEC>(out2, op + chw, left);
    const float4 u = kCfg ? load_quad<VEC>(out2, op + 2 * B * chw, left) : c;
    const float4 z = has_noise ? load_quad<VEC>(noise, o, left) : zero;
    float4 r;
    r.x = lvar_update(k, xv.x, denoise_eps<kCfg>(k, lvar_eps_hat(kind, c.x, xv.x, sa, sb), lvar_eps_hat(kind, u.x, xv.x, sa, sb)), v.x, z.x, lb, lbt, has_noise);
    r.y = lvar_update(k, xv.y, denoise_eps<kCfg>(k, lvar_eps_hat(kind, c.y, xv.y, sa, sb), lvar_eps_hat(kind, u.y, xv.y, sa, sb)), v.y, z.y, lb, lbt, has_noise);
    r.z = lvar_update(k, xv.z, denoise_eps<kCfg>(k, lvar_eps_hat(kind, c.z, xv.z, sa, sb), lvar_eps_hat(kind, u.z, xv.z, sa, sb)), v.z, z.z, lb, lbt, has_noise);
    r.w = lvar_update(k, xv.w, denoise_eps<kCfg>(k, lvar_eps_hat(kind, c.w, xv.w, sa, sb), lvar_eps_hat(kind, u.w, xv.w, sa, sb)), v.w, z.w, lb, lbt, has_noise);
    store_quad<VEC>(x_out, o, left, r);
    if (x_out2) store_quad<VEC>(x_out2, o, left, r);
  }
}

// vlb_terms_k with the per-element variance: one workgroup per row r = (img[r], t[r]); out2: rows of 2 per floats.
//   sq[r] = sum_j (eps_hat_j - eps_j)^2 (d-form),  term[r] = sum_j lvar_term: the KL terms (t >= 2) or the decoder's (t == 1)
// x_t is what afd_noise_images_gather wrote.  Each thread sums its quads in index order, x, y, z, w within one.
template <bool VEC>
__global__ __launch_bounds__(256) void vlb_terms_lvar_k(const float* __restrict__ x0, const int64_t* __restrict__ img,
                                                        const float* __restrict__ xt, const float* __restrict__ eps,
                                                        const float* __restrict__ out2, const int64_t* __restrict__ t,
                                                        const double* __restrict__ lv_coef, const float* __restrict__ alpha,
                                                        const float* __restrict__ alpha_hat, const float* __restrict__ beta, int kind,
                                                        double* __restrict__ term, double* __restrict__ sq, long per) {
  __shared__ double red[8];
  const long r = blockIdx.x;
  const LvarRow row = lvar_row(lv_coef, alpha, alpha_hat, beta, t[r], kind);
  const long src = img[r] * per, dst = r * per, rp = 2 * r * per;
  double s_t = 0.0, s_sq = 0.0;
  for (long q = threadIdx.x; 4 * q < per; q += blockDim.x) {
    const long left = per - 4 * q;
    const float4 p = load_quad<VEC>(out2, rp + 4 * q, left), v = load_quad<VEC>(out2, rp + per + 4 * q, left);
    const float4 x = load_quad<VEC>(x0, src + 4 * q, left), e = load_quad<VEC>(eps, dst + 4 * q, left);
    const float4 n = row.is_dec ? load_quad<VEC>(xt, dst + 4 * q, left) : x;
    const float pv[4] = {p.x, p.y, p.z, p.w}, vv[4] = {v.x, v.y, v.z, v.w}, xv[4] = {x.x, x.y, x.z, x.w}, ev[4] = {e.x, e.y, e.z, e.w};
    const float nv[4] = {n.x, n.y, n.z, n.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < left) {
        double d2, dlv;
        s_t += lvar_term<false>(row, kind, pv[i], vv[i], xv[i], ev[i], nv[i], d2, dlv);
        s_sq += d2;
      }
    }
  }
  block_sum2_f64(s_t, s_sq, red);
  if (threadIdx.x == 0) {
    term[r] = s_t;
    sq[r] = s_sq;
  }
}

// ---- AdamW (torch.optim.AdamW semantics, decoupled weight decay) ---------------------------
__global__ void adamw_tick_k(float* state, float b1, float b2) {
  // state = {step, 1 - b1^step, 1 - b2^step, unused}; double keeps the powers exact enough for 1e6 steps
  const double step = (double)state[0] + 1.0;
  state[0] = (float)step;
  state[1] = (float)(1.0 - pow((double)b1, step));
  state[2] = (float)(1.0 - pow((double)b2, step));
}
__global__ void adamw_step_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                             long n, const float* __restrict__ state, float lr, float b1, float b2, float eps, float wd, float gscale) {
  const float bc1 = state[1], bc2 = state[2];
  const float step_size = lr / bc1, inv_sqrt_bc2 = 1.0f / sqrtf(bc2), decay = 1.0f - lr * wd;
  AFD_GRID_STRIDE(i, n) {
    const float gi = g[i] * gscale;
    const float pi = p[i] * decay;
    const float mi = m[i] + (gi - m[i]) * (1.0f - b1);            // lerp, as torch does
    const float vi = v[i] * b2 + gi * gi * (1.0f - b2);
    const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
    p[i] = pi - step_size * (mi / denom);
    m[i] = mi; v[i] = vi;
  }
}

// ---- EMA of the weights (training.EMA, modules/ddpm_utils.py:26-51) -------------------------------------------------------
// ema' = copy ? p : (ema * beta) + (p * omb), three roundings in that order (torch's `old * beta + (1 - beta) * new` on fp32
// tensors; omb = float(1.0 - beta) formed in double on the host).  VEC: every pointer 16-byte aligned -> float4 accesses.
__device__ __forceinline__ float ema_rule(float e, float p, int copy, float beta, float omb) {
  if (copy) return p;
  const float l = e * beta, r = p * omb;
  return l + r;
}
template <bool VEC>
__device__ __forceinline__ void ema_range(float* __restrict__ ema, const float* __restrict__ p, long lo, long hi, int copy,
                                          float beta, float omb) {
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  long s = lo;
  if (VEC && (lo & 3) == 0) {                   // lo % 4 == 0 keeps the 16-byte alignment of the base pointers
    const long n4 = (hi - lo) >> 2;
    float4* e4 = reinterpret_cast<float4*>(ema + lo);
    const float4* p4 = reinterpret_cast<const float4*>(p + lo);
    for (long k = tid; k < n4; k += stride) {
      const float4 pv = p4[k];
      float4 ev = e4[k];
      ev.x = ema_rule(ev.x, pv.x, copy, beta, omb); ev.y = ema_rule(ev.y, pv.y, copy, beta, omb);
      ev.z = ema_rule(ev.z, pv.z, copy, beta, omb); ev.w = ema_rule(ev.w, pv.w, copy, beta, omb);
      e4[k] = ev;
    }
    s = lo + 4 * n4;
  }
  for (long i = s + tid; i < hi; i += stride) ema[i] = ema_rule(ema[i], p[i], copy, beta, omb);
}
template <bool VEC>
__global__ void ema_step_k(float* __restrict__ ema, const float* __restrict__ p, long n, int copy, float beta, float omb) {
  ema_range<VEC>(ema, p, 0, n, copy, beta, omb);
}

// adamw_tick_k's arithmetic, plus the EMA's call counter: ema_state = {calls, copy}; copy = calls < start, then ++calls
// (the order of EMA.step_ema).  Device-resident so that a replayed step crosses `start` where the eager one would.
__global__ void adamw_ema_tick_k(float* state, float b1, float b2, int* ema_state, int start) {
  const double step = (double)state[0] + 1.0;
  state[0] = (float)step;
  state[1] = (float)(1.0 - pow((double)b1, step));
  state[2] = (float)(1.0 - pow((double)b2, step));
  const int calls = ema_state[0];
  ema_state[1] = calls < start ? 1 : 0;
  ema_state[0] = calls + 1;
}

// one AdamW element, the expressions and order of adamw_step_k
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float gscale, float decay, float b1, float b2,
                                           float step_size, float inv_sqrt_bc2, float eps) {
  const float gi = g * gscale;
  const float pi = p * decay;
  const float mi = m + (gi - m) * (1.0f - b1);
  const float vi = v * b2 + gi * gi * (1.0f - b2);
  const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
  p = pi - step_size * (mi / denom);
  m = mi; v = vi;
}

// AdamW over [0, n_active) with the EMA rule applied to the NEW p, then the EMA rule alone over [n_active, n_ema) (FlatParams'
// tail: parameters the optimiser never touches, which the reference's EMA still walks).  One pass: p, g, m, v, ema streamed once.
template <bool VEC>
__global__ void adamw_ema_step_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                 long n_active, const float* __restrict__ state, float lr, float b1, float b2, float eps, float wd,
                                 float gscale, float* __restrict__ ema, long n_ema, const int* __restrict__ ema_state, float beta,
                                 float omb) {
  const float bc1 = state[1], bc2 = state[2];
  const float step_size = lr / bc1, inv_sqrt_bc2 = 1.0f / sqrtf(bc2), decay = 1.0f - lr * wd;
  const int copy = ema_state[1];
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  long s = 0;
  if (VEC) {
    const long n4 = n_active >> 2;
    for (long k = tid; k < n4; k += stride) {
      float4 pv = reinterpret_cast<const float4*>(p)[k];
      const float4 gv = reinterpret_cast<const float4*>(g)[k];
      float4 mv = reinterpret_cast<const float4*>(m)[k], vv = reinterpret_cast<const float4*>(v)[k];
      float4 ev = reinterpret_cast<const float4*>(ema)[k];
      adamw_elem(pv.x, gv.x, mv.x, vv.x, gscale, decay, b1, b2, step_size, inv_sqrt_bc2, eps);
      adamw_elem(pv.y, gv.y, mv.y, vv.y, gscale, decay, b1, b2, step_size, inv_sqrt_bc2, eps);
      adamw_elem(pv.z, gv.z, mv.z, vv.z, gscale, decay, b1, b2, step_size, inv_sqrt_bc2, eps);
      adamw_elem(pv.w, gv.w, mv.w, vv.w, gscale, decay, b1, b2, step_size, inv_sqrt_bc2, eps);
      ev.x = ema_rule(ev.x, pv.x, copy, beta, omb); ev.y = ema_rule(ev.y, pv.y, copy, beta, omb);
      ev.z = ema_rule(ev.z, pv.z, copy, beta, omb); ev.w = ema_rule(ev.w, pv.w, copy, beta, omb);
      reinterpret_cast<float4*>(p)[k] = pv;
      reinterpret_cast<float4*>(m)[k] = mv;
      reinterpret_cast<float4*>(v)[k] = vv;
      reinterpret_cast<float4*>(ema)[k] = ev;
    }
    s = 4 * n4;
  }
  for (long i = s + tid; i < n_active; i += stride) {
    float pi = p[i], mi = m[i], vi = v[i];
    adamw_elem(pi, g[i], mi, vi, gscale, decay, b1, b2, step_size, inv_sqrt_bc2, eps);
    p[i] = pi; m[i] = mi; v[i] = vi;
    ema[i] = ema_rule(ema[i], pi, copy, beta, omb);
  }
  ema_range<VEC>(ema, p, n_active, n_ema, copy, beta, omb);
}

// ---- gradient-norm clipping and the learning-rate schedule, on the device (training.FusedAdamW(max_grad_norm=, lr_schedule=)) ----
// Squared L2 norm of g * gscale as kGradNormPartials fp64 partial sums.  Workgroup j owns the fixed slice [j*slice, (j+1)*slice)
// (slice a multiple of 4, chosen from n alone); inside it, thread t takes the quads t, t + 256, ... in ascending order into ONE
// fp64 accumulator, then the workgroup's fixed tree (block_sum2_f64).  Nothing depends on the grid, on timing or on VEC, which
// only turns four scalar loads into one 16-byte load: run to run, and aligned against misaligned, the bytes are identical.
constexpr int kGradNormPartials = 512;      // two 256-thread workgroups per CU; four quads in flight per thread = 32 KiB per CU
template <bool VEC>
__device__ __forceinline__ float4 load_quad(const float* __restrict__ g, long q) {
  if (VEC) return reinterpret_cast<const float4*>(g)[q];
  return make_float4(g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]);
}
__device__ __forceinline__ void sq_acc(double& s, float g, float gscale) {
  const float gi = g * gscale;                  // the product adamw_elem forms, in fp32
  s += (double)gi * (double)gi;                 // (exact in fp64: 48 significant bits)
}
__device__ __forceinline__ void sq_acc4(double& s, float4 v, float gscale) {
  sq_acc(s, v.x, gscale); sq_acc(s, v.y, gscale); sq_acc(s, v.z, gscale); sq_acc(s, v.w, gscale);
}
template <bool VEC>
__global__ void grad_sqnorm_partials_k(const float* __restrict__ g, long n, long slice, float gscale, double* __restrict__ partials) {
  __shared__ double red[8];
  const long lo = blockIdx.x * slice;
  long len = n - lo;
  len = len < 0 ? 0 : (len > slice ? slice : len);
  const float* gs = g + lo;
  const long nq = len >> 2;                     // whole quads of this slice
  double s = 0.0, unused = 0.0;
  long q = threadIdx.x;
  for (; q + 768 < nq; q += 1024) {             // four independent loads, then the four quads in order
    const float4 a = load_quad<VEC>(gs, q), b = load_quad<VEC>(gs, q + 256), c = load_quad<VEC>(gs, q + 512),
                 d = load_quad<VEC>(gs, q + 768);
    sq_acc4(s, a, gscale); sq_acc4(s, b, gscale); sq_acc4(s, c, gscale); sq_acc4(s, d, gscale);
  }
  for (; q < nq; q += 256) sq_acc4(s, load_quad<VEC>(gs, q), gscale);
  if (q == nq)                                  // the end of the buffer inside a quad: its elements, in the thread that quad belongs to
    for (long i = 4 * nq; i < len; ++i) sq_acc(s, gs[i], gscale);
  block_sum2_f64(s, unused, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ctl = device double[kCtlDoubles]: what the tick decides and the step reads (afd.h)
enum { kCtlLr = 0, kCtlCoef, kCtlNorm, kCtlSkip, kCtlNSkipped, kCtlSq, kCtlIndex, kCtlFactor, kCtlDoubles };
constexpr int kCtlMaxPartials = 1024;

__device__ __forceinline__ double lr_factor(const afd_opt_ctl& c, double k) {
  if (k < (double)c.warmup) return k / (double)(c.warmup > 1 ? c.warmup : 1);
  if (c.kind == AFD_LR_CONSTANT) return 1.0;
  const long span = c.total - c.warmup;
  double pr = (k - (double)c.warmup) / (double)(span > 1 ? span : 1);
  pr = pr < 1.0 ? pr : 1.0;
  const double base = c.kind == AFD_LR_COSINE ? 0.5 * (1.0 + cos(3.141592653589793 * pr)) : 1.0 - pr;
  return c.min_ratio + (1.0 - c.min_ratio) * base;
}

// One workgroup: the partials in index order -> norm -> clip coefficient; unless the step is skipped, adamw_tick_k (or
// adamw_ema_tick_k) and the learning rate of this update.  The partials go through LDS so that thread 0's chain of fp64 adds
// does not wait on one global load each.
__global__ void adamw_ctl_tick_k(float* state, float b1, float b2, int* ema_state, int start, const double* __restrict__ partials,
                                 int n_partials, afd_opt_ctl cfg, double* ctl) {
  __shared__ double sp[kCtlMaxPartials];
  for (int i = threadIdx.x; i < n_partials; i += blockDim.x) sp[i] = partials[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sq = 0.0, norm = 0.0, coef = 1.0;
  if (partials) {
    for (int i = 0; i < n_partials; ++i) sq += sp[i];
    norm = sqrt(sq);
    if (cfg.max_norm > 0.0) {
      const double c = cfg.max_norm / (norm + 1e-6);
      coef = c > 1.0 ? 1.0 : c;                 // (a NaN norm gives a NaN coefficient, as torch.clamp(max=1) does)
    }
  }
  ctl[kCtlSq] = sq;
  ctl[kCtlNorm] = norm;
  if (cfg.skip_nonfinite && !(fabs(norm) <= 1.79769313486231570e308)) {      // inf or NaN
    ctl[kCtlSkip] = 1.0;
    ctl[kCtlNSkipped] += 1.0;
    return;
  }
  const double step = (double)state[0] + 1.0;   // adamw_tick_k
  state[0] = (float)step;
  state[1] = (float)(1.0 - pow((double)b1, step));
  state[2] = (float)(1.0 - pow((double)b2, step));
  if (ema_state) {                              // adamw_ema_tick_k
    const int calls = ema_state[0];
    ema_state[1] = calls < start ? 1 : 0;
    ema_state[0] = calls + 1;
  }
  const double k = (double)state[0] - 1.0, factor = lr_factor(cfg, k);
  ctl[kCtlLr] = (double)(float)(cfg.base_lr * factor);
  ctl[kCtlCoef] = coef;
  ctl[kCtlSkip] = 0.0;
  ctl[kCtlIndex] = k;
  ctl[kCtlFactor] = factor;
}

// adamw_step_k (EMA = false) / adamw_ema_step_k (EMA = true) with lr and the clip coefficient read from ctl; every thread
// returns before its first access when ctl says skip.
template <bool VEC, bool EMA>
__global__ void adamw_ctl_step_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                 long n_active, const float* __restrict__ state, const double* __restrict__ ctl, float b1, float b2,
                                 float eps, float wd, float grad_scale, float* __restrict__ ema, long n_ema,
                                 const int* __restrict__ ema_state, float beta, float omb) {
  if (ctl[kCtlSkip] != 0.0) return;
  const float lr = (float)ctl[kCtlLr], gscale = grad_scale * (float)ctl[kCtlCoef];
  const float bc1 = state[1], bc2 = state[2];
  const float step_size = lr / bc1, inv_sqrt_bc2 = 1.0f / sqrtf(bc2), decay = 1.0f - lr * wd;
  const int copy = EMA ? ema_state[1] : 0;
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  long s = 0;
  if (VEC) {
    const long n4 = n_active >> 2;
    for (long k = tid; k < n4; k += stride) {
      float4 pv = reinterpret_cast<const float4*>(p)[k];
      const float4 gv = reinterpret_cast<const float4*>(g)[k];
      float4 mv = reinterpret_cast<const float4*>(m)[k], vv = reinterpret_cast<const float4*>(v)[k];
      adamw_elem(pv.x, gv.x, mv.x, vv.x, gscale, decay, b1, b2, step_size, inv_sqrt_bc2, eps);
      adamw_elem(pv.y, gv.y, mv.y, vv.y, gscale, decay, b1, b2, step_size, inv_sqrt_bc2, eps);
      adamw_elem(pv.z, gv.z, mv.z, vv.z, gscale, decay, b1, b2, step_size, inv_sqrt_bc2, eps);
      adamw_elem(pv.w, gv.w, mv.w, vv.w, gscale, decay, b1, b2, step_size, inv_sqrt_bc2, eps);
      reinterpret_cast<float4*>(p)[k] = pv;
      reinterpret_cast<float4*>(m)[k] = mv;
      reinterpret_cast<float4*>(v)[k] = vv;
      if (EMA) {
        float4 ev = reinterpret_cast<const float4*>(ema)[k];
        ev.x = ema_rule(ev.x, pv.x, copy, beta, omb); ev.y = ema_rule(ev.y, pv.y, copy, beta, omb);
        ev.z = ema_rule(ev.z, pv.z, copy, beta, omb); ev.w = ema_rule(ev.w, pv.w, copy, beta, omb);
        reinterpret_cast<float4*>(ema)[k] = ev;
      }
    }
    s = 4 * n4;
  }
  for (long i = s + tid; i < n_active; i += stride) {
    float pi = p[i], mi = m[i], vi = v[i];
    adamw_elem(pi, g[i], mi, vi, gscale, decay, b1, b2, step_size, inv_sqrt_bc2, eps);
    p[i] = pi; m[i] = mi; v[i] = vi;
    if (EMA) ema[i] = ema_rule(ema[i], pi, copy, beta, omb);
  }
  if (EMA) ema_range<VEC>(ema, p, n_active, n_ema, copy, beta, omb);
}

}  // namespace afd
using namespace afd;

extern "C" {

int afd_noise_images(const float* x, const float* eps, const int64_t* t, const float* alpha_hat, float* x_t,
                     int B, long per_sample, afd_stream_t st) {
  AFD_REQUIRE(x && eps && t && alpha_hat && x_t && B > 0 && per_sample > 0, "afd_noise_images: bad argument");
  const long total = (long)B * per_sample;
  hipLaunchKernelGGL(noise_images_k, dim3(gs_grid(total)), dim3(256), 0, as_stream(st), x, eps, t, alpha_hat, x_t, per_sample, total);
  return check_launch("afd_noise_images");
}
int afd_denoise_step(const float* x, const float* eps_pred, const float* noise, const float* alpha, const float* alpha_hat,
                     const float* beta, int i, float* x_out, long n, afd_stream_t st) {
  AFD_REQUIRE(x && eps_pred && alpha && alpha_hat && beta && x_out && n > 0 && i >= 0, "afd_denoise_step: bad argument");
  hipLaunchKernelGGL(denoise_step_k, dim3(gs_grid(n)), dim3(256), 0, as_stream(st), x, eps_pred, noise, alpha, alpha_hat, beta, i, (const int64_t*)nullptr, x_out, n);
  return check_launch("afd_denoise_step");
}
int afd_denoise_step_dev(const float* x, const float* eps_pred, const float* noise, const float* alpha, const float* alpha_hat,
                         const float* beta, const int64_t* t_dev, float* x_out, long n, afd_stream_t st) {
  AFD_REQUIRE(x && eps_pred && alpha && alpha_hat && beta && t_dev && x_out && n > 0, "afd_denoise_step_dev: bad argument");
  hipLaunchKernelGGL(denoise_step_k, dim3(gs_grid(n)), dim3(256), 0, as_stream(st), x, eps_pred, noise, alpha, alpha_hat, beta, 0, t_dev, x_out, n);
  return check_launch("afd_denoise_step_dev");
}
int afd_denoise_step_cfg(const float* x, const float* eps2, const float* noise, const float* alpha, const float* alpha_hat,
                         const float* beta, int i, float cfg_scale, float* x_out, float* x_out2, long n, afd_stream_t st) {
  AFD_REQUIRE(x && eps2 && alpha && alpha_hat && beta && x_out && n > 0 && i >= 0, "afd_denoise_step_cfg: bad argument");
  launch_denoise_step_cfg(x, eps2, noise, alpha, alpha_hat, beta, i, nullptr, cfg_scale, x_out, x_out2, n, as_stream(st));
  return check_launch("afd_denoise_step_cfg");
}
int afd_denoise_step_cfg_dev(const float* x, const float* eps2, const float* noise, const float* alpha, const float* alpha_hat,
                             const float* beta, const int64_t* t_dev, float cfg_scale, float* x_out, float* x_out2, long n,
                             afd_stream_t st) {
  AFD_REQUIRE(x && eps2 && alpha && alpha_hat && beta && t_dev && x_out && n > 0, "afd_denoise_step_cfg_dev: bad argument");
  launch_denoise_step_cfg(x, eps2, noise, alpha, alpha_hat, beta, 0, t_dev, cfg_scale, x_out, x_out2, n, as_stream(st));
  return check_launch("afd_denoise_step_cfg_dev");
}
int afd_ddim_step(const float* x, const float* eps, const float* noise, const float* alpha_hat, int t, int t_prev, float eta,
                  float* x_out, long n, afd_stream_t st) {
  AFD_REQUIRE(x && eps && alpha_hat && x_out, "afd_ddim_step: x, eps, alpha_hat and x_out must not be NULL");
  AFD_REQUIRE(n > 0, "afd_ddim_step: n must be positive (got %ld)", n);
  AFD_REQUIRE(t_prev >= 0 && t_prev < t, "afd_ddim_step: need 0 <= t_prev < t (got t = %d, t_prev = %d)", t, t_prev);
  AFD_REQUIRE(eta >= 0.0f, "afd_ddim_step: eta must be >= 0");
  launch_ddim_step<false>(x, eps, noise, alpha_hat, t, t_prev, nullptr, nullptr, eta, 0.0f, x_out, nullptr, n, as_stream(st));
  return check_launch("afd_ddim_step");
}
int afd_ddim_step_dev(const float* x, const float* eps, const float* noise, const float* alpha_hat, const int64_t* t_dev,
                      const int64_t* t_prev_dev, float eta, float* x_out, long n, afd_stream_t st) {
  AFD_REQUIRE(x && eps && alpha_hat && t_dev && t_prev_dev && x_out,
              "afd_ddim_step_dev: x, eps, alpha_hat, t_dev, t_prev_dev and x_out must not be NULL");
  AFD_REQUIRE(n > 0, "afd_ddim_step_dev: n must be positive (got %ld)", n);
  AFD_REQUIRE(eta >= 0.0f, "afd_ddim_step_dev: eta must be >= 0");
  launch_ddim_step<false>(x, eps, noise, alpha_hat, 0, 0, t_dev, t_prev_dev, eta, 0.0f, x_out, nullptr, n, as_stream(st));
  return check_launch("afd_ddim_step_dev");
}
int afd_ddim_step_cfg(const float* x, const float* eps2, const float* noise, const float* alpha_hat, int t, int t_prev, float eta,
                      float cfg_scale, float* x_out, float* x_out2, long n, afd_stream_t st) {
  AFD_REQUIRE(x && eps2 && alpha_hat && x_out, "afd_ddim_step_cfg: x, eps2, alpha_hat and x_out must not be NULL");
  AFD_REQUIRE(n > 0, "afd_ddim_step_cfg: n must be positive (got %ld)", n);
  AFD_REQUIRE(t_prev >= 0 && t_prev < t, "afd_ddim_step_cfg: need 0 <= t_prev < t (got t = %d, t_prev = %d)", t, t_prev);
  AFD_REQUIRE(eta >= 0.0f, "afd_ddim_step_cfg: eta must be >= 0");
  launch_ddim_step<true>(x, eps2, noise, alpha_hat, t, t_prev, nullptr, nullptr, eta, cfg_scale, x_out, x_out2, n, as_stream(st));
  return check_launch("afd_ddim_step_cfg");
}
int afd_ddim_step_cfg_dev(const float* x, const float* eps2, const float* noise, const float* alpha_hat, const int64_t* t_dev,
                          const int64_t* t_prev_dev, float eta, float cfg_scale, float* x_out, float* x_out2, long n, afd_stream_t st) {
  AFD_REQUIRE(x && eps2 && alpha_hat && t_dev && t_prev_dev && x_out,
              "afd_ddim_step_cfg_dev: x, eps2, alpha_hat, t_dev, t_prev_dev and x_out must not be NULL");
  AFD_REQUIRE(n > 0, "afd_ddim_step_cfg_dev: n must be positive (got %ld)", n);
  AFD_REQUIRE(eta >= 0.0f, "afd_ddim_step_cfg_dev: eta must be >= 0");
  launch_ddim_step<true>(x, eps2, noise, alpha_hat, 0, 0, t_dev, t_prev_dev, eta, cfg_scale, x_out, x_out2, n, as_stream(st));
  return check_launch("afd_ddim_step_cfg_dev");
}
static inline bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

// ---- masked steps (inpainting) and renoise ---------------------------------------------------------------------------------
static inline bool overlaps(const void* a, long abytes, const void* b, long bbytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return b && pa < pb + (uintptr_t)bbytes && pb < pa + (uintptr_t)abytes;
}
// x0 and mask are read by every element while x_out / x_out2 are written: they must not share memory
static inline bool masked_inputs_apart(const float* x0, const uint8_t* mask, const float* x_out, const float* x_out2, long n) {
  const long fb = n * (long)sizeof(float);
  return !overlaps(x0, fb, x_out, fb) && !overlaps(x0, fb, x_out2, fb) && !overlaps(mask, n, x_out, fb) && !overlaps(mask, n, x_out2, fb);
}
#define AFD_MASKED_CHECKS(name, x0, mask, x_out, x_out2, n)                                                                   \
  AFD_REQUIRE(n > 0, name ": n must be positive (got %ld)", n);                                                           \
  AFD_REQUIRE(masked_inputs_apart(x0, mask, x_out, x_out2, n), name ": x0 and mask must not overlap x_out or x_out2")

int afd_denoise_step_masked(const float* x, const float* eps_pred, const float* noise, const float* x0, const uint8_t* mask,
                            const float* alpha, const float* alpha_hat, const float* beta, int i, float* x_out, long n,
                            afd_stream_t st) {
  AFD_REQUIRE(x && eps_pred && x0 && mask && alpha && alpha_hat && beta && x_out,
              "afd_denoise_step_masked: x, eps_pred, x0, mask, alpha, alpha_hat, beta and x_out must not be NULL");
  AFD_MASKED_CHECKS("afd_denoise_step_masked", x0, mask, x_out, (const float*)nullptr, n);
  AFD_REQUIRE(i >= 1, "afd_denoise_step_masked: need i >= 1 (the step i -> i - 1; got i = %d)", i);
  AFD_REQUIRE(noise || i == 1, "afd_denoise_step_masked: noise must not be NULL when i > 1 (it noises the known region)");
  launch_denoise_step_masked<false>(x, eps_pred, noise, x0, mask, alpha, alpha_hat, beta, i, nullptr, 0.0f, x_out, nullptr, n,
                                    as_stream(st));
  return check_launch("afd_denoise_step_masked");
}
int afd_denoise_step_masked_dev(const float* x, const float* eps_pred, const float* noise, const float* x0, const uint8_t* mask,
                                const float* alpha, const float* alpha_hat, const float* beta, const int64_t* t_dev, float* x_out,
                                long n, afd_stream_t st) {
  AFD_REQUIRE(x && eps_pred && noise && x0 && mask && alpha && alpha_hat && beta && t_dev && x_out,
              "afd_denoise_step_masked_dev: x, eps_pred, noise, x0, mask, alpha, alpha_hat, beta, t_dev and x_out must not be NULL");
  AFD_MASKED_CHECKS("afd_denoise_step_masked_dev", x0, mask, x_out, (const float*)nullptr, n);
  launch_denoise_step_masked<false>(x, eps_pred, noise, x0, mask, alpha, alpha_hat, beta, 0, t_dev, 0.0f, x_out, nullptr, n,
                                    as_stream(st));
  return check_launch("afd_denoise_step_masked_dev");
}
int afd_denoise_step_masked_cfg(const float* x, const float* eps2, const float* noise, const float* x0, const uint8_t* mask,
                                const float* alpha, const float* alpha_hat, const float* beta, int i, float cfg_scale, float* x_out,
                                float* x_out2, long n, afd_stream_t st) {
  AFD_REQUIRE(x && eps2 && x0 && mask && alpha && alpha_hat && beta && x_out,
              "afd_denoise_step_masked_cfg: x, eps2, x0, mask, alpha, alpha_hat, beta and x_out must not be NULL");
  AFD_MASKED_CHECKS("afd_denoise_step_masked_cfg", x0, mask, x_out, x_out2, n);
  AFD_REQUIRE(i >= 1, "afd_denoise_step_masked_cfg: need i >= 1 (the step i -> i - 1; got i = %d)", i);
  AFD_REQUIRE(noise || i == 1, "afd_denoise_step_masked_cfg: noise must not be NULL when i > 1 (it noises the known region)");
  launch_denoise_step_masked<true>(x, eps2, noise, x0, mask, alpha, alpha_hat, beta, i, nullptr, cfg_scale, x_out, x_out2, n,
                                   as_stream(st));
  return check_launch("afd_denoise_step_masked_cfg");
}
int afd_denoise_step_masked_cfg_dev(const float* x, const float* eps2, const float* noise, const float* x0, const uint8_t* mask,
                                    const float* alpha, const float* alpha_hat, const float* beta, const int64_t* t_dev,
                                    float cfg_scale, float* x_out, float* x_out2, long n, afd_stream_t st) {
  AFD_REQUIRE(x && eps2 && noise && x0 && mask && alpha && alpha_hat && beta && t_dev && x_out,
              "afd_denoise_step_masked_cfg_dev: x, eps2, noise, x0, mask, alpha, alpha_hat, beta, t_dev and x_out must not be NULL");
  AFD_MASKED_CHECKS("afd_denoise_step_masked_cfg_dev", x0, mask, x_out, x_out2, n);
  launch_denoise_step_masked<true>(x, eps2, noise, x0, mask, alpha, alpha_hat, beta, 0, t_dev, cfg_scale, x_out, x_out2, n,
                                   as_stream(st));
  return check_launch("afd_denoise_step_masked_cfg_dev");
}
int afd_ddim_step_masked(const float* x, const float* eps, const float* noise, const float* x0, const uint8_t* mask,
                         const float* alpha_hat, int t, int t_prev, float eta, float* x_out, long n, afd_stream_t st) {
  AFD_REQUIRE(x && eps && x0 && mask && alpha_hat && x_out, "afd_ddim_step_masked: x, eps, x0, mask, alpha_hat and x_out must not be NULL");
  AFD_MASKED_CHECKS("afd_ddim_step_masked", x0, mask, x_out, (const float*)nullptr, n);
  AFD_REQUIRE(t_prev >= 0 && t_prev < t, "afd_ddim_step_masked: need 0 <= t_prev < t (got t = %d, t_prev = %d)", t, t_prev);
  AFD_REQUIRE(eta >= 0.0f, "afd_ddim_step_masked: eta must be >= 0");
  AFD_REQUIRE(noise || t_prev == 0, "afd_ddim_step_masked: noise must not be NULL when t_prev > 0 (it noises the known region)");
  launch_ddim_step_masked<false>(x, eps, noise, x0, mask, alpha_hat, t, t_prev, nullptr, nullptr, eta, 0.0f, x_out, nullptr, n,
                                 as_stream(st));
  return check_launch("afd_ddim_step_masked");
}
int afd_ddim_step_masked_dev(const float* x, const float* eps, const float* noise, const float* x0, const uint8_t* mask,
                             const float* alpha_hat, const int64_t* t_dev, const int64_t* t_prev_dev, float eta, float* x_out, long n,
                             afd_stream_t st) {
  AFD_REQUIRE(x && eps && noise && x0 && mask && alpha_hat && t_dev && t_prev_dev && x_out,
              "afd_ddim_step_masked_dev: x, eps, noise, x0, mask, alpha_hat, t_dev, t_prev_dev and x_out must not be NULL");
  AFD_MASKED_CHECKS("afd_ddim_step_masked_dev", x0, mask, x_out, (const float*)nullptr, n);
  AFD_REQUIRE(eta >= 0.0f, "afd_ddim_step_masked_dev: eta must be >= 0");
  launch_ddim_step_masked<false>(x, eps, noise, x0, mask, alpha_hat, 0, 0, t_dev, t_prev_dev, eta, 0.0f, x_out, nullptr, n,
                                 as_stream(st));
  return check_launch("afd_ddim_step_masked_dev");
}
int afd_ddim_step_masked_cfg(const float* x, const float* eps2, const float* noise, const float* x0, const uint8_t* mask,
                             const float* alpha_hat, int t, int t_prev, float eta, float cfg_scale, float* x_out, float* x_out2, long n,
                             afd_stream_t st) {
  AFD_REQUIRE(x && eps2 && x0 && mask && alpha_hat && x_out,
              "afd_ddim_step_masked_cfg: x, eps2, x0, mask, alpha_hat and x_out must not be NULL");
  AFD_MASKED_CHECKS("afd_ddim_step_masked_cfg", x0, mask, x_out, x_out2, n);
  AFD_REQUIRE(t_prev >= 0 && t_prev < t, "afd_ddim_step_masked_cfg: need 0 <= t_prev < t (got t = %d, t_prev = %d)", t, t_prev);
  AFD_REQUIRE(eta >= 0.0f, "afd_ddim_step_masked_cfg: eta must be >= 0");
  AFD_REQUIRE(noise || t_prev == 0, "afd_ddim_step_masked_cfg: noise must not be NULL when t_prev > 0 (it noises the known region)");
  launch_ddim_step_masked<true>(x, eps2, noise, x0, mask, alpha_hat, t, t_prev, nullptr, nullptr, eta, cfg_scale, x_out, x_out2, n,
                                as_stream(st));
  return check_launch("afd_ddim_step_masked_cfg");
}
int afd_ddim_step_masked_cfg_dev(const float* x, const float* eps2, const float* noise, const float* x0, const uint8_t* mask,
                                 const float* alpha_hat, const int64_t* t_dev, const int64_t* t_prev_dev, float eta, float cfg_scale,
                                 float* x_out, float* x_out2, long n, afd_stream_t st) {
  AFD_REQUIRE(x && eps2 && noise && x0 && mask && alpha_hat && t_dev && t_prev_dev && x_out,
              "afd_ddim_step_masked_cfg_dev: x, eps2, noise, x0, mask, alpha_hat, t_dev, t_prev_dev and x_out must not be NULL");
  AFD_MASKED_CHECKS("afd_ddim_step_masked_cfg_dev", x0, mask, x_out, x_out2, n);
  AFD_REQUIRE(eta >= 0.0f, "afd_ddim_step_masked_cfg_dev: eta must be >= 0");
  launch_ddim_step_masked<true>(x, eps2, noise, x0, mask, alpha_hat, 0, 0, t_dev, t_prev_dev, eta, cfg_scale, x_out, x_out2, n,
                                as_stream(st));
  return check_launch("afd_ddim_step_masked_cfg_dev");
}
int afd_renoise(const float* x, const float* noise, const float* alpha_hat, int t_from, int t_to, float* x_out, long n,
                afd_stream_t st) {
  AFD_REQUIRE(x && noise && alpha_hat && x_out, "afd_renoise: x, noise, alpha_hat and x_out must not be NULL");
  AFD_REQUIRE(n > 0, "afd_renoise: n must be positive (got %ld)", n);
  AFD_REQUIRE(t_from >= 0 && t_from < t_to, "afd_renoise: need 0 <= t_from < t_to (got t_from = %d, t_to = %d)", t_from, t_to);
  if (n % 4 == 0 && aligned16(x) && aligned16(noise) && aligned16(x_out))
    hipLaunchKernelGGL(renoise_k<true>, dim3(step_grid(n / 4)), dim3(256), 0, as_stream(st), x, noise, alpha_hat, t_from, t_to, x_out,
                       n / 4);
  else
    hipLaunchKernelGGL(renoise_k<false>, dim3(step_grid(n)), dim3(256), 0, as_stream(st), x, noise, alpha_hat, t_from, t_to, x_out, n);
  return check_launch("afd_renoise");
}

// ---- DPM-Solver++(2M) ------------------------------------------------------------------------------------------------------
// x0_out is written while x, eps, x_out and x_out2 are read or written by other elements: it must share no memory with them.
// x0_prev may be x0_out itself (the sampler's in-place state) but may not overlap it partly.
static inline bool dpmpp_apart(const float* x, const float* eps, long eps_n, const float* x0_prev, float* x_out, float* x_out2,
                               float* x0_out, long n) {
  const long fb = n * (long)sizeof(float);
  return !overlaps(x0_out, fb, x, fb) && !overlaps(x0_out, fb, eps, eps_n * (long)sizeof(float)) && !overlaps(x0_out, fb, x_out, fb) &&
         !overlaps(x0_out, fb, x_out2, fb) && (x0_prev == x0_out || !overlaps(x0_out, fb, x0_prev, fb));
}
int afd_dpmpp_step(const float* x, const float* eps, const float* x0_prev, const float* coef, float* x_out, float* x0_out, long n,
                   afd_stream_t st) {
  AFD_REQUIRE(x && eps && coef && x_out && x0_out, "afd_dpmpp_step: x, eps, coef, x_out and x0_out must not be NULL");
  AFD_REQUIRE(n > 0, "afd_dpmpp_step: n must be positive (got %ld)", n);
  AFD_REQUIRE(dpmpp_apart(x, eps, n, x0_prev, x_out, nullptr, x0_out, n),
              "afd_dpmpp_step: x0_out must not overlap x, eps or x_out, and must be x0_prev itself or apart from it");
  launch_dpmpp_step<false>(x, eps, x0_prev, coef, 0.0f, x_out, nullptr, x0_out, n, as_stream(st));
  return check_launch("afd_dpmpp_step");
}
int afd_dpmpp_step_cfg(const float* x, const float* eps2, const float* x0_prev, const float* coef, float cfg_scale, float* x_out,
                       float* x_out2, float* x0_out, long n, afd_stream_t st) {
  AFD_REQUIRE(x && eps2 && coef && x_out && x0_out, "afd_dpmpp_step_cfg: x, eps2, coef, x_out and x0_out must not be NULL");
  AFD_REQUIRE(n > 0, "afd_dpmpp_step_cfg: n must be positive (got %ld)", n);
  AFD_REQUIRE(dpmpp_apart(x, eps2, 2 * n, x0_prev, x_out, x_out2, x0_out, n),
              "afd_dpmpp_step_cfg: x0_out must not overlap x, eps2, x_out or x_out2, and must be x0_prev itself or apart from it");
  launch_dpmpp_step<true>(x, eps2, x0_prev, coef, cfg_scale, x_out, x_out2, x0_out, n, as_stream(st));
  return check_launch("afd_dpmpp_step_cfg");
}
// ---- likelihood (bits/dim) ------------------------------------------------------------------------------------------------
// img and t are read on the device and not range-checked here (the Python layer checks them); every output must share no
// memory with any input.
static inline int row_grid(long rows) { return (int)std::min<long>(rows, 4096); }
int afd_noise_images_gather(const float* x0, long n_img, const int64_t* img, const float* eps, const int64_t* t, const float* alpha_hat,
                            float* x_t, long rows, long per, afd_stream_t st) {
  AFD_REQUIRE(x0 && img && eps && t && alpha_hat && x_t, "afd_noise_images_gather: x0, img, eps, t, alpha_hat and x_t must not be NULL");
  AFD_REQUIRE(n_img > 0 && rows > 0 && per > 0, "afd_noise_images_gather: n_img, rows and per must be positive (got %ld, %ld, %ld)",
              n_img, rows, per);
  const long fb = rows * per * (long)sizeof(float), ib = rows * (long)sizeof(int64_t);
  AFD_REQUIRE(!overlaps(x_t, fb, x0, n_img * per * (long)sizeof(float)) && !overlaps(x_t, fb, eps, fb) && !overlaps(x_t, fb, img, ib) &&
                  !overlaps(x_t, fb, t, ib),
              "afd_noise_images_gather: x_t must not overlap x0, eps, img or t");
  if (per % 4 == 0 && aligned16(x0) && aligned16(eps) && aligned16(x_t))
    hipLaunchKernelGGL(noise_images_gather_k<true>, dim3(row_grid(rows)), dim3(256), 0, as_stream(st), x0, img, eps, t, alpha_hat, x_t,
                       rows, per / 4);
  else
    hipLaunchKernelGGL(noise_images_gather_k<false>, dim3(row_grid(rows)), dim3(256), 0, as_stream(st), x0, img, eps, t, alpha_hat, x_t,
                       rows, per);
  return check_launch("afd_noise_images_gather");
}
int afd_vlb_terms(const float* x0, long n_img, const int64_t* img, const float* x_t, const float* eps, const float* eps_hat,
                  const int64_t* t, const double* coef, long T, const float* alpha, const float* alpha_hat, const float* beta,
                  double* term, double* sq, long rows, long per, afd_stream_t st) {
  AFD_REQUIRE(x0 && img && x_t && eps && eps_hat && t && coef && alpha && alpha_hat && beta && term && sq,
              "afd_vlb_terms: no pointer may be NULL");
  AFD_REQUIRE(n_img > 0 && rows > 0 && per > 0 && T >= 2, "afd_vlb_terms: n_img, rows and per must be positive and T >= 2 (got %ld, %ld, %ld, %ld)",
              n_img, rows, per, T);
  AFD_REQUIRE(rows <= 0x7fffffffL, "afd_vlb_terms: at most 2^31 - 1 rows per call (got %ld)", rows);
  const long db = rows * (long)sizeof(double), fb = rows * per * (long)sizeof(float), ib = rows * (long)sizeof(int64_t);
  const long tb = T * (long)sizeof(float);
  const void* in[] = {x0, img, x_t, eps, eps_hat, t, coef, alpha, alpha_hat, beta};
  const long in_b[] = {n_img * per * (long)sizeof(float), ib, fb, fb, fb, ib, 4 * T * (long)sizeof(double), tb, tb, tb};
  bool apart = !overlaps(term, db, sq, db);
  for (int i = 0; i < 10; ++i) apart = apart && !overlaps(term, db, in[i], in_b[i]) && !overlaps(sq, db, in[i], in_b[i]);
  AFD_REQUIRE(apart, "afd_vlb_terms: term and sq must not overlap each other or any input");
  if (per % 4 == 0 && aligned16(x0) && aligned16(x_t) && aligned16(eps) && aligned16(eps_hat))
    hipLaunchKernelGGL(vlb_terms_k<true>, dim3((unsigned)rows), dim3(256), 0, as_stream(st), x0, img, x_t, eps, eps_hat, t, coef, alpha,
                       alpha_hat, beta, term, sq, per / 4, per);
  else
    hipLaunchKernelGGL(vlb_terms_k<false>, dim3((unsigned)rows), dim3(256), 0, as_stream(st), x0, img, x_t, eps, eps_hat, t, coef, alpha,
                       alpha_hat, beta, term, sq, per, per);
  return check_launch("afd_vlb_terms");
}
int afd_vlb_prior(const float* x0, double half_ah, double* out, long n_img, long per, afd_stream_t st) {
  AFD_REQUIRE(x0 && out, "afd_vlb_prior: x0 and out must not be NULL");
  AFD_REQUIRE(n_img > 0 && per > 0, "afd_vlb_prior: n_img and per must be positive (got %ld, %ld)", n_img, per);
  AFD_REQUIRE(n_img <= 0x7fffffffL, "afd_vlb_prior: at most 2^31 - 1 images per call (got %ld)", n_img);
  AFD_REQUIRE(!overlaps(out, n_img * (long)sizeof(double), x0, n_img * per * (long)sizeof(float)), "afd_vlb_prior: out must not overlap x0");
  if (per % 4 == 0 && aligned16(x0))
    hipLaunchKernelGGL(vlb_prior_k<true>, dim3((unsigned)n_img), dim3(256), 0, as_stream(st), x0, half_ah, out, per / 4);
  else
    hipLaunchKernelGGL(vlb_prior_k<false>, dim3((unsigned)n_img), dim3(256), 0, as_stream(st), x0, half_ah, out, per);
  return check_launch("afd_vlb_prior");
}
int afd_quantize_u8(const float* x, uint8_t* out, long n, afd_stream_t st) {
  AFD_REQUIRE(x && out && n > 0, "afd_quantize_u8: bad argument");
  hipLaunchKernelGGL(quantize_u8_k, dim3(gs_grid(n)), dim3(256), 0, as_stream(st), x, out, n);
  return check_launch("afd_quantize_u8");
}
int afd_mse_fwd(const float* pred, const float* target, float* loss_out, float* workspace, long n, afd_stream_t st) {
  AFD_REQUIRE(pred && target && loss_out && workspace && n > 0, "afd_mse_fwd: bad argument");
  const int nb = gs_grid(n) < kMseBlocks ? gs_grid(n) : kMseBlocks;
  hipLaunchKernelGGL(mse_partial_k, dim3(nb), dim3(256), 0, as_stream(st), pred, target, workspace, n);
  hipLaunchKernelGGL(mse_final_k, dim3(1), dim3(256), 0, as_stream(st), workspace, loss_out, nb, 1.0f / (float)n);
  return check_launch("afd_mse_fwd");
}
int afd_mse_bwd(const float* pred, const float* target, const float* dloss, float* dpred, long n, afd_stream_t st) {
  AFD_REQUIRE(pred && target && dloss && dpred && n > 0, "afd_mse_bwd: bad argument");
  hipLaunchKernelGGL(mse_bwd_k, dim3(gs_grid(n)), dim3(256), 0, as_stream(st), pred, target, dloss, dpred, n, 2.0f / (float)n);
  return check_launch("afd_mse_bwd");
}

// items / segments of the objective kernels' (row, 256-quad segment) walk, and its grid
static inline long obj_segs(long chw) { return ((chw + 3) / 4 + 255) / 256; }
static inline int obj_grid(long items) { return (int)(items < kObjBlocks ? items : kObjBlocks); }
static inline bool kind_ok(int kind) { return kind == AFD_PRED_EPS || kind == AFD_PRED_V || kind == AFD_PRED_X0; }

int afd_objective_loss_fwd(const float* pred, const float* x0, const float* eps, const int64_t* t, const float* alpha_hat,
                           const float* w, int kind, float* loss_out, float* workspace, long B, long chw, afd_stream_t st) {
  AFD_REQUIRE(pred && x0 && eps && t && alpha_hat && loss_out && workspace,
              "afd_objective_loss_fwd: pred, x0, eps, t, alpha_hat, loss_out and workspace must not be NULL");
  AFD_REQUIRE(kind_ok(kind), "afd_objective_loss_fwd: kind must be AFD_PRED_EPS, AFD_PRED_V or AFD_PRED_X0 (got %d)", kind);
  AFD_REQUIRE(B > 0 && chw > 0, "afd_objective_loss_fwd: B and chw must be positive (got %ld, %ld)", B, chw);
  const long segs = obj_segs(chw), items = B * segs;
  const int nb = obj_grid(items);
  const float inv_n = 1.0f / (float)(B * chw);
  if (chw % 4 == 0 && aligned16(pred) && aligned16(x0) && aligned16(eps))
    hipLaunchKernelGGL(objective_partial_k<true>, dim3(nb), dim3(256), 0, as_stream(st), pred, x0, eps, t, alpha_hat, w, kind,
                       workspace, items, segs, chw);
  else
    hipLaunchKernelGGL(objective_partial_k<false>, dim3(nb), dim3(256), 0, as_stream(st), pred, x0, eps, t, alpha_hat, w, kind,
                       workspace, items, segs, chw);
  hipLaunchKernelGGL(mse_final_k, dim3(1), dim3(256), 0, as_stream(st), workspace, loss_out, nb, inv_n);
  return check_launch("afd_objective_loss_fwd");
}
int afd_objective_loss_bwd(const float* pred, const float* x0, const float* eps, const int64_t* t, const float* alpha_hat,
                           const float* w, int kind, const float* dloss, float* dpred, long B, long chw, afd_stream_t st) {
  AFD_REQUIRE(pred && x0 && eps && t && alpha_hat && dloss && dpred,
              "afd_objective_loss_bwd: pred, x0, eps, t, alpha_hat, dloss and dpred must not be NULL");
  AFD_REQUIRE(kind_ok(kind), "afd_objective_loss_bwd: kind must be AFD_PRED_EPS, AFD_PRED_V or AFD_PRED_X0 (got %d)", kind);
  AFD_REQUIRE(B > 0 && chw > 0, "afd_objective_loss_bwd: B and chw must be positive (got %ld, %ld)", B, chw);
  const long segs = obj_segs(chw), items = B * segs;
  const float two_over_n = 2.0f / (float)(B * chw);
  if (chw % 4 == 0 && aligned16(pred) && aligned16(x0) && aligned16(eps) && aligned16(dpred))
    hipLaunchKernelGGL(objective_bwd_k<true>, dim3(obj_grid(items)), dim3(256), 0, as_stream(st), pred, x0, eps, t, alpha_hat, w, kind,
                       dloss, dpred, items, segs, chw, two_over_n);
  else
    hipLaunchKernelGGL(objective_bwd_k<false>, dim3(obj_grid(items)), dim3(256), 0, as_stream(st), pred, x0, eps, t, alpha_hat, w, kind,
                       dloss, dpred, items, segs, chw, two_over_n);
  return check_launch("afd_objective_loss_bwd");
}
int afd_pred_to_eps(const float* out, const float* x_t, const int64_t* t, const float* alpha_hat, int kind, float* eps_out, long B,
                    long chw, afd_stream_t st) {
  AFD_REQUIRE(out && x_t && t && alpha_hat && eps_out, "afd_pred_to_eps: out, x_t, t, alpha_hat and eps_out must not be NULL");
  AFD_REQUIRE(kind == AFD_PRED_V || kind == AFD_PRED_X0,
              "afd_pred_to_eps: kind must be AFD_PRED_V or AFD_PRED_X0 (got %d; an eps output needs no conversion)", kind);
  AFD_REQUIRE(B > 0 && chw > 0, "afd_pred_to_eps: B and chw must be positive (got %ld, %ld)", B, chw);
  const long segs = obj_segs(chw), items = B * segs;
  if (chw % 4 == 0 && aligned16(out) && aligned16(x_t) && aligned16(eps_out))
    hipLaunchKernelGGL(pred_to_eps_k<true>, dim3(obj_grid(items)), dim3(256), 0, as_stream(st), out, x_t, t, alpha_hat, kind, eps_out,
                       items, segs, chw);
  else
    hipLaunchKernelGGL(pred_to_eps_k<false>, dim3(obj_grid(items)), dim3(256), 0, as_stream(st), out, x_t, t, alpha_hat, kind, eps_out,
                       items, segs, chw);
  return check_launch("afd_pred_to_eps");
}

// ---- learned variances ----------------------------------------------------------------------------------------------------
// whether the n_out outputs share no memory with each other or with any of the n_in inputs (NULL entries are skipped)
static inline bool all_apart(const void* const* out, const long* out_b, int n_out, const void* const* in, const long* in_b, int n_in) {
  for (int i = 0; i < n_out; ++i) {
    if (!out[i]) continue;
    for (int j = i + 1; j < n_out; ++j)
      if (overlaps(out[i], out_b[i], out[j], out_b[j])) return false;
    for (int j = 0; j < n_in; ++j)
      if (overlaps(out[i], out_b[i], in[j], in_b[j])) return false;
  }
  return true;
}
constexpr long kLvarWsFloats = 3 * kObjBlocks;      // kObjBlocks fp32 partials, then kObjBlocks fp64 partials

int afd_lvar_loss_fwd(const float* out2, const float* x0, const float* eps, const int64_t* t, const float* alpha,
                      const float* alpha_hat, const float* beta, const double* lv_coef, const float* w, int kind, double vlb_scale,
                      float* loss_out, double* sums_out, float* workspace, long B, long chw, afd_stream_t st) {
  AFD_REQUIRE(out2 && x0 && eps && t && alpha && alpha_hat && beta && lv_coef && loss_out && workspace,
              "afd_lvar_loss_fwd: out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef, loss_out and workspace must not be NULL");
  AFD_REQUIRE(kind_ok(kind), "afd_lvar_loss_fwd: kind must be AFD_PRED_EPS, AFD_PRED_V or AFD_PRED_X0 (got %d)", kind);
  AFD_REQUIRE(B > 0 && chw > 0, "afd_lvar_loss_fwd: B and chw must be positive (got %ld, %ld)", B, chw);
  AFD_REQUIRE(std::isfinite(vlb_scale) && vlb_scale >= 0.0, "afd_lvar_loss_fwd: vlb_scale must be finite and >= 0 (got %g)", vlb_scale);
  AFD_REQUIRE(((uintptr_t)workspace & 7) == 0, "afd_lvar_loss_fwd: workspace must be 8-byte aligned");
  const long fb = B * chw * (long)sizeof(float);
  const void* out[] = {loss_out, sums_out, workspace};
  const long out_b[] = {2 * (long)sizeof(float), 2 * (long)sizeof(double), kLvarWsFloats * (long)sizeof(float)};
  const void* in[] = {out2, x0, eps, t};
  const long in_b[] = {2 * fb, fb, fb, B * (long)sizeof(int64_t)};
  AFD_REQUIRE(all_apart(out, out_b, 3, in, in_b, 4), "afd_lvar_loss_fwd: loss_out, sums_out and workspace must not overlap each other or an input");
  const long segs = obj_segs(chw), items = B * segs;
  const int nb = obj_grid(items);
  double* part_v = reinterpret_cast<double*>(workspace + kObjBlocks);
  const double n = (double)B * (double)chw;
  if (chw % 4 == 0 && aligned16(out2) && aligned16(x0) && aligned16(eps))
    hipLaunchKernelGGL(lvar_partial_k<true>, dim3(nb), dim3(256), 0, as_stream(st), out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef, w,
                       kind, workspace, part_v, items, segs, chw);
  else
    hipLaunchKernelGGL(lvar_partial_k<false>, dim3(nb), dim3(256), 0, as_stream(st), out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef, w,
                       kind, workspace, part_v, items, segs, chw);
  hipLaunchKernelGGL(lvar_final_k, dim3(1), dim3(256), 0, as_stream(st), workspace, part_v, nb, 1.0f / (float)(B * chw),
                     n * 0.6931471805599453, vlb_scale, loss_out, sums_out);
  return check_launch("afd_lvar_loss_fwd");
}
int afd_lvar_loss_bwd(const float* out2, const float* x0, const float* eps, const int64_t* t, const float* alpha,
                      const float* alpha_hat, const float* beta, const double* lv_coef, const float* w, int kind, double vlb_scale,
                      const float* dloss, float* dout2, long B, long chw, afd_stream_t st) {
  AFD_REQUIRE(out2 && x0 && eps && t && alpha && alpha_hat && beta && lv_coef && dloss && dout2,
              "afd_lvar_loss_bwd: out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef, dloss and dout2 must not be NULL");
  AFD_REQUIRE(kind_ok(kind), "afd_lvar_loss_bwd: kind must be AFD_PRED_EPS, AFD_PRED_V or AFD_PRED_X0 (got %d)", kind);
  AFD_REQUIRE(B > 0 && chw > 0, "afd_lvar_loss_bwd: B and chw must be positive (got %ld, %ld)", B, chw);
  AFD_REQUIRE(std::isfinite(vlb_scale) && vlb_scale >= 0.0, "afd_lvar_loss_bwd: vlb_scale must be finite and >= 0 (got %g)", vlb_scale);
  const long fb = B * chw * (long)sizeof(float);
  const void* out[] = {dout2};
  const long out_b[] = {2 * fb};
  const void* in[] = {out2, x0, eps, t, dloss};
  const long in_b[] = {2 * fb, fb, fb, B * (long)sizeof(int64_t), (long)sizeof(float)};
  AFD_REQUIRE(all_apart(out, out_b, 1, in, in_b, 5), "afd_lvar_loss_bwd: dout2 must not overlap an input");
  const long segs = obj_segs(chw), items = B * segs;
  const double n = (double)B * (double)chw;
  const float two_over_n = 2.0f / (float)(B * chw);
  const double gv = vlb_scale / (n * 0.6931471805599453);
  if (chw % 4 == 0 && aligned16(out2) && aligned16(x0) && aligned16(eps) && aligned16(dout2))
    hipLaunchKernelGGL(lvar_bwd_k<true>, dim3(obj_grid(items)), dim3(256), 0, as_stream(st), out2, x0, eps, t, alpha, alpha_hat, beta,
                       lv_coef, w, kind, dloss, dout2, items, segs, chw, two_over_n, gv);
  else
    hipLaunchKernelGGL(lvar_bwd_k<false>, dim3(obj_grid(items)), dim3(256), 0, as_stream(st), out2, x0, eps, t, alpha, alpha_hat, beta,
                       lv_coef, w, kind, dloss, dout2, items, segs, chw, two_over_n, gv);
  return check_launch("afd_lvar_loss_bwd");
}
int afd_split_pred(const float* out2, const float* x_t, const int64_t* t, const float* alpha_hat, int kind, float* eps_out,
                   float* v_out, long B, long chw, afd_stream_t st) {
  AFD_REQUIRE(out2 && eps_out, "afd_split_pred: out2 and eps_out must not be NULL");
  AFD_REQUIRE(kind_ok(kind), "afd_split_pred: kind must be AFD_PRED_EPS, AFD_PRED_V or AFD_PRED_X0 (got %d)", kind);
  AFD_REQUIRE(kind == AFD_PRED_EPS || (x_t && t && alpha_hat), "afd_split_pred: x_t, t and alpha_hat must not be NULL for AFD_PRED_V / AFD_PRED_X0");
  AFD_REQUIRE(B > 0 && chw > 0, "afd_split_pred: B and chw must be positive (got %ld, %ld)", B, chw);
  const long fb = B * chw * (long)sizeof(float);
  const void* out[] = {eps_out, v_out};
  const long out_b[] = {fb, fb};
  const void* in[] = {out2, x_t, t};
  const long in_b[] = {2 * fb, fb, B * (long)sizeof(int64_t)};
  AFD_REQUIRE(all_apart(out, out_b, 2, in, in_b, 3), "afd_split_pred: eps_out and v_out must not overlap each other, out2, x_t or t");
  const long segs = obj_segs(chw), items = B * segs;
  if (chw % 4 == 0 && aligned16(out2) && aligned16(eps_out) && (!x_t || aligned16(x_t)) && (!v_out || aligned16(v_out)))
    hipLaunchKernelGGL(split_pred_k<true>, dim3(obj_grid(items)), dim3(256), 0, as_stream(st), out2, x_t, t, alpha_hat, kind, eps_out,
                       v_out, items, segs, chw);
  else
    hipLaunchKernelGGL(split_pred_k<false>, dim3(obj_grid(items)), dim3(256), 0, as_stream(st), out2, x_t, t, alpha_hat, kind, eps_out,
                       v_out, items, segs, chw);
  return check_launch("afd_split_pred");
}

// x_out may be x itself, and must otherwise share no memory with x; x_out and x_out2 share none with each other or any other input
static int launch_lvar_step(bool kCfg, const char* name, const float* x, const float* out2, const float* noise, const float* alpha,
                            const float* alpha_hat, const float* beta, const double* lv_coef, int kind, int i, const int64_t* t_dev,
                            bool dev, float s, float* x_out, float* x_out2, long B, long chw, hipStream_t st) {
  AFD_REQUIRE(x && out2 && alpha && alpha_hat && beta && lv_coef && x_out && (!dev || t_dev),
              "%s: x, out2, alpha, alpha_hat, beta, lv_coef%s and x_out must not be NULL", name, dev ? ", t_dev" : "");
  AFD_REQUIRE(kind_ok(kind), "%s: kind must be AFD_PRED_EPS, AFD_PRED_V or AFD_PRED_X0 (got %d)", name, kind);
  AFD_REQUIRE(B > 0 && chw > 0, "%s: B and chw must be positive (got %ld, %ld)", name, B, chw);
  AFD_REQUIRE(dev || i >= 1, "%s: need i >= 1 (the step i -> i - 1; got i = %d)", name, i);
  const long fb = B * chw * (long)sizeof(float);
  const void* out[] = {x_out, x_out2};
  const long out_b[] = {fb, fb};
  const void* in[] = {out2, noise, t_dev, x_out == x ? nullptr : x};
  const long in_b[] = {(kCfg ? 4 : 2) * fb, fb, (long)sizeof(int64_t), fb};
  AFD_REQUIRE(all_apart(out, out_b, 2, in, in_b, 4) && !(x_out2 && overlaps(x_out2, fb, x, fb)),
              "%s: x_out must be x itself or apart from it, and x_out / x_out2 must not overlap each other, out2, noise or t_dev", name);
  const long segs = obj_segs(chw), items = B * segs;
  const bool vec = chw % 4 == 0 && aligned16(x) && aligned16(out2) && aligned16(x_out) && (!noise || aligned16(noise)) &&
                   (!x_out2 || aligned16(x_out2));
  auto kern = kCfg ? (vec ? lvar_step_k<true, true> : lvar_step_k<true, false>) : (vec ? lvar_step_k<false, true> : lvar_step_k<false, false>);
  hipLaunchKernelGGL(kern, dim3(obj_grid(items)), dim3(256), 0, st, x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, i, t_dev, s,
                     x_out, x_out2, items, segs, chw, B);
  return check_launch(name);
}
int afd_denoise_step_lvar(const float* x, const float* out2, const float* noise, const float* alpha, const float* alpha_hat,
                          const float* beta, const double* lv_coef, int kind, int i, float* x_out, long B, long chw, afd_stream_t st) {
  return launch_lvar_step(false, "afd_denoise_step_lvar", x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, i, nullptr, false, 0.0f,
                                 x_out, nullptr, B, chw, as_stream(st));
}
int afd_denoise_step_lvar_dev(const float* x, const float* out2, const float* noise, const float* alpha, const float* alpha_hat,
                              const float* beta, const double* lv_coef, int kind, const int64_t* t_dev, float* x_out, long B, long chw,
                              afd_stream_t st) {
  return launch_lvar_step(false, "afd_denoise_step_lvar_dev", x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, 0, t_dev, true, 0.0f,
                                 x_out, nullptr, B, chw, as_stream(st));
}
int afd_denoise_step_lvar_cfg(const float* x, const float* out2, const float* noise, const float* alpha, const float* alpha_hat,
                              const float* beta, const double* lv_coef, int kind, int i, float cfg_scale, float* x_out, float* x_out2,
                              long B, long chw, afd_stream_t st) {
  return launch_lvar_step(true, "afd_denoise_step_lvar_cfg", x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, i, nullptr, false,
                                cfg_scale, x_out, x_out2, B, chw, as_stream(st));
}
int afd_denoise_step_lvar_cfg_dev(const float* x, const float* out2, const float* noise, const float* alpha, const float* alpha_hat,
                                  const float* beta, const double* lv_coef, int kind, const int64_t* t_dev, float cfg_scale, float* x_out,
                                  float* x_out2, long B, long chw, afd_stream_t st) {
  return launch_lvar_step(true, "afd_denoise_step_lvar_cfg_dev", x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, 0, t_dev, true,
                                cfg_scale, x_out, x_out2, B, chw, as_stream(st));
}
int afd_vlb_terms_lvar(const float* x0, long n_img, const int64_t* img, const float* x_t, const float* eps, const float* out2,
                       const int64_t* t, const double* lv_coef, long T, const float* alpha, const float* alpha_hat, const float* beta,
                       int kind, double* term, double* sq, long rows, long per, afd_stream_t st) {
  AFD_REQUIRE(x0 && img && x_t && eps && out2 && t && lv_coef && alpha && alpha_hat && beta && term && sq,
              "afd_vlb_terms_lvar: no pointer may be NULL");
  AFD_REQUIRE(kind_ok(kind), "afd_vlb_terms_lvar: kind must be AFD_PRED_EPS, AFD_PRED_V or AFD_PRED_X0 (got %d)", kind);
  AFD_REQUIRE(n_img > 0 && rows > 0 && per > 0 && T >= 2,
              "afd_vlb_terms_lvar: n_img, rows and per must be positive and T >= 2 (got %ld, %ld, %ld, %ld)", n_img, rows, per, T);
  AFD_REQUIRE(rows <= 0x7fffffffL, "afd_vlb_terms_lvar: at most 2^31 - 1 rows per call (got %ld)", rows);
  const long db = rows * (long)sizeof(double), fb = rows * per * (long)sizeof(float), ib = rows * (long)sizeof(int64_t);
  const long tb = T * (long)sizeof(float);
  const void* out[] = {term, sq};
  const long out_b[] = {db, db};
  const void* in[] = {x0, img, x_t, eps, out2, t, lv_coef, alpha, alpha_hat, beta};
  const long in_b[] = {n_img * per * (long)sizeof(float), ib, fb, fb, 2 * fb, ib, 3 * T * (long)sizeof(double), tb, tb, tb};
  AFD_REQUIRE(all_apart(out, out_b, 2, in, in_b, 10), "afd_vlb_terms_lvar: term and sq must not overlap each other or any input");
  if (per % 4 == 0 && aligned16(x0) && aligned16(x_t) && aligned16(eps) && aligned16(out2))
    hipLaunchKernelGGL(vlb_terms_lvar_k<true>, dim3((unsigned)rows), dim3(256), 0, as_stream(st), x0, img, x_t, eps, out2, t, lv_coef,
                       alpha, alpha_hat, beta, kind, term, sq, per);
  else
    hipLaunchKernelGGL(vlb_terms_lvar_k<false>, dim3((unsigned)rows), dim3(256), 0, as_stream(st), x0, img, x_t, eps, out2, t, lv_coef,
                       alpha, alpha_hat, beta, kind, term, sq, per);
  return check_launch("afd_vlb_terms_lvar");
}
int afd_adamw_tick(float* state, float b1, float b2, afd_stream_t st) {
  AFD_REQUIRE(state, "afd_adamw_tick: state is NULL");
  hipLaunchKernelGGL(adamw_tick_k, dim3(1), dim3(1), 0, as_stream(st), state, b1, b2);
  return check_launch("afd_adamw_tick");
}
int afd_adamw_step(float* p, const float* g, float* m, float* v, long n, const float* state,
                   float lr, float b1, float b2, float eps, float wd, float gscale, afd_stream_t st) {
  AFD_REQUIRE(p && g && m && v && state && n > 0, "afd_adamw_step: bad argument");
  hipLaunchKernelGGL(adamw_step_k, dim3(gs_grid(n)), dim3(256), 0, as_stream(st), p, g, m, v, n, state, lr, b1, b2, eps, wd, gscale);
  return check_launch("afd_adamw_step");
}

static inline bool beta_ok(float beta, float omb) { return beta >= 0.0f && beta <= 1.0f && omb >= 0.0f && omb <= 1.0f; }
int afd_ema_step(float* ema, const float* p, long n, int copy, float beta, float one_minus_beta, afd_stream_t st) {
  AFD_REQUIRE(ema && p, "afd_ema_step: ema or p is NULL");
  AFD_REQUIRE(n > 0, "afd_ema_step: n must be positive (got %ld)", n);
  AFD_REQUIRE(beta_ok(beta, one_minus_beta), "afd_ema_step: beta and 1 - beta must lie in [0, 1] (got %g, %g)", (double)beta,
              (double)one_minus_beta);
  const int c = copy != 0;
  if (aligned16(ema) && aligned16(p))
    hipLaunchKernelGGL(ema_step_k<true>, dim3(gs_grid((n + 3) / 4)), dim3(256), 0, as_stream(st), ema, p, n, c, beta, one_minus_beta);
  else
    hipLaunchKernelGGL(ema_step_k<false>, dim3(gs_grid(n)), dim3(256), 0, as_stream(st), ema, p, n, c, beta, one_minus_beta);
  return check_launch("afd_ema_step");
}
int afd_adamw_ema_tick(float* adam_state, float b1, float b2, int* ema_state, int start, afd_stream_t st) {
  AFD_REQUIRE(adam_state && ema_state, "afd_adamw_ema_tick: adam_state or ema_state is NULL");
  AFD_REQUIRE(start >= 0, "afd_adamw_ema_tick: start must be >= 0 (got %d)", start);
  hipLaunchKernelGGL(adamw_ema_tick_k, dim3(1), dim3(1), 0, as_stream(st), adam_state, b1, b2, ema_state, start);
  return check_launch("afd_adamw_ema_tick");
}
int afd_adamw_ema_step(float* p, const float* g, float* m, float* v, long n_active, const float* adam_state, float lr, float b1,
                       float b2, float eps, float wd, float gscale, float* ema, long n_ema, const int* ema_state, float beta,
                       float one_minus_beta, afd_stream_t st) {
  AFD_REQUIRE(p && g && m && v && adam_state && ema && ema_state, "afd_adamw_ema_step: a pointer is NULL");
  AFD_REQUIRE(n_active > 0 && n_ema > 0, "afd_adamw_ema_step: n_active and n_ema must be positive (got %ld, %ld)", n_active, n_ema);
  AFD_REQUIRE(n_active <= n_ema, "afd_adamw_ema_step: n_active > n_ema (%ld > %ld)", n_active, n_ema);
  AFD_REQUIRE(beta_ok(beta, one_minus_beta), "afd_adamw_ema_step: beta and 1 - beta must lie in [0, 1] (got %g, %g)",
              (double)beta, (double)one_minus_beta);
  if (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(ema))
    hipLaunchKernelGGL(adamw_ema_step_k<true>, dim3(gs_grid((n_ema + 3) / 4)), dim3(256), 0, as_stream(st), p, g, m, v, n_active,
                       adam_state, lr, b1, b2, eps, wd, gscale, ema, n_ema, ema_state, beta, one_minus_beta);
  else
    hipLaunchKernelGGL(adamw_ema_step_k<false>, dim3(gs_grid(n_ema)), dim3(256), 0, as_stream(st), p, g, m, v, n_active,
                       adam_state, lr, b1, b2, eps, wd, gscale, ema, n_ema, ema_state, beta, one_minus_beta);
  return check_launch("afd_adamw_ema_step");
}

int afd_grad_sqnorm_n_partials(void) { return kGradNormPartials; }
int afd_grad_sqnorm_partials(const float* g, long n, float grad_scale, double* partials, int n_partials, afd_stream_t st) {
  AFD_REQUIRE(g && partials, "afd_grad_sqnorm_partials: g or partials is NULL");
  AFD_REQUIRE(n > 0, "afd_grad_sqnorm_partials: n must be positive (got %ld)", n);
  AFD_REQUIRE(n_partials == kGradNormPartials, "afd_grad_sqnorm_partials: n_partials must be afd_grad_sqnorm_n_partials() = %d (got %d)",
              kGradNormPartials, n_partials);
  AFD_REQUIRE(!overlaps(partials, kGradNormPartials * (long)sizeof(double), g, n * (long)sizeof(float)),
              "afd_grad_sqnorm_partials: partials must not overlap g");
  const long slice = 4 * ((n + 4L * kGradNormPartials - 1) / (4L * kGradNormPartials));
  if (aligned16(g))
    hipLaunchKernelGGL(grad_sqnorm_partials_k<true>, dim3(kGradNormPartials), dim3(256), 0, as_stream(st), g, n, slice, grad_scale, partials);
  else
    hipLaunchKernelGGL(grad_sqnorm_partials_k<false>, dim3(kGradNormPartials), dim3(256), 0, as_stream(st), g, n, slice, grad_scale, partials);
  return check_launch("afd_grad_sqnorm_partials");
}
int afd_adamw_ctl_tick(float* adam_state, float b1, float b2, int* ema_state, int ema_start, const double* partials, int n_partials,
                       const afd_opt_ctl* cfg, double* ctl, afd_stream_t st) {
  AFD_REQUIRE(adam_state && cfg && ctl, "afd_adamw_ctl_tick: adam_state, cfg or ctl is NULL");
  AFD_REQUIRE(!ema_state || ema_start >= 0, "afd_adamw_ctl_tick: ema_start must be >= 0 (got %d)", ema_start);
  AFD_REQUIRE(!partials || (n_partials >= 1 && n_partials <= kCtlMaxPartials), "afd_adamw_ctl_tick: n_partials must lie in [1, %d] (got %d)",
              kCtlMaxPartials, n_partials);
  AFD_REQUIRE(std::isfinite(cfg->base_lr) && cfg->base_lr >= 0.0, "afd_adamw_ctl_tick: base_lr must be finite and >= 0 (got %g)", cfg->base_lr);
  AFD_REQUIRE(cfg->warmup >= 0, "afd_adamw_ctl_tick: warmup must be >= 0 (got %ld)", cfg->warmup);
  AFD_REQUIRE(cfg->kind == AFD_LR_CONSTANT || cfg->kind == AFD_LR_LINEAR || cfg->kind == AFD_LR_COSINE,
              "afd_adamw_ctl_tick: unknown schedule kind %d", cfg->kind);
  AFD_REQUIRE(cfg->kind == AFD_LR_CONSTANT || cfg->total >= cfg->warmup, "afd_adamw_ctl_tick: total < warmup (%ld < %ld)", cfg->total,
              cfg->warmup);
  AFD_REQUIRE(cfg->min_ratio >= 0.0 && cfg->min_ratio <= 1.0, "afd_adamw_ctl_tick: min_ratio must lie in [0, 1] (got %g)", cfg->min_ratio);
  AFD_REQUIRE(!std::isnan(cfg->max_norm), "afd_adamw_ctl_tick: max_norm is NaN");
  hipLaunchKernelGGL(adamw_ctl_tick_k, dim3(1), dim3(256), 0, as_stream(st), adam_state, b1, b2, ema_state, ema_start, partials,
                     partials ? n_partials : 0, *cfg, ctl);
  return check_launch("afd_adamw_ctl_tick");
}
int afd_adamw_ctl_step(float* p, const float* g, float* m, float* v, long n_active, const float* adam_state, const double* ctl,
                       float b1, float b2, float eps, float wd, float grad_scale, float* ema, long n_ema, const int* ema_state,
                       float beta, float one_minus_beta, afd_stream_t st) {
  AFD_REQUIRE(p && g && m && v && adam_state && ctl, "afd_adamw_ctl_step: a pointer is NULL");
  AFD_REQUIRE(n_active > 0, "afd_adamw_ctl_step: n_active must be positive (got %ld)", n_active);
  if (!ema) {
    if (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v))
      hipLaunchKernelGGL((adamw_ctl_step_k<true, false>), dim3(gs_grid((n_active + 3) / 4)), dim3(256), 0, as_stream(st), p, g, m, v,
                         n_active, adam_state, ctl, b1, b2, eps, wd, grad_scale, (float*)nullptr, 0L, (const int*)nullptr, 0.0f, 0.0f);
    else
      hipLaunchKernelGGL((adamw_ctl_step_k<false, false>), dim3(gs_grid(n_active)), dim3(256), 0, as_stream(st), p, g, m, v, n_active,
                         adam_state, ctl, b1, b2, eps, wd, grad_scale, (float*)nullptr, 0L, (const int*)nullptr, 0.0f, 0.0f);
    return check_launch("afd_adamw_ctl_step");
  }
  AFD_REQUIRE(ema_state, "afd_adamw_ctl_step: ema is given but ema_state is NULL");
  AFD_REQUIRE(n_ema > 0 && n_active <= n_ema, "afd_adamw_ctl_step: 0 < n_active <= n_ema is required (got %ld, %ld)", n_active, n_ema);
  AFD_REQUIRE(beta_ok(beta, one_minus_beta), "afd_adamw_ctl_step: beta and 1 - beta must lie in [0, 1] (got %g, %g)", (double)beta,
              (double)one_minus_beta);
  if (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(ema))
    hipLaunchKernelGGL((adamw_ctl_step_k<true, true>), dim3(gs_grid((n_ema + 3) / 4)), dim3(256), 0, as_stream(st), p, g, m, v, n_active,
                       adam_state, ctl, b1, b2, eps, wd, grad_scale, ema, n_ema, ema_state, beta, one_minus_beta);
  else
    hipLaunchKernelGGL((adamw_ctl_step_k<false, true>), dim3(gs_grid(n_ema)), dim3(256), 0, as_stream(st), p, g, m, v, n_active,
                       adam_state, ctl, b1, b2, eps, wd, grad_scale, ema, n_ema, ema_state, beta, one_minus_beta);
  return check_launch("afd_adamw_ctl_step");
}

}  // extern "C"

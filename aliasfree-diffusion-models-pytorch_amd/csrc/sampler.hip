// sampler.hip -- the diffusion math: noising, the sampler steps (DDPM, DDIM, DPM-Solver++(2M), learned variances; plain, guided
// and masked), renoise, the likelihood bound, the training objectives and quantisation.  (The optimizer is optim.hip.)
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

// ---- sampler steps: DDPM and DDIM, plain, guided (kCfg), masked (kMasked) or both, one kernel template --------------------------
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

// DDIM (Song et al. 2021), one step t -> t_prev of a strided chain.  a_t = alpha_hat[t], a_p = alpha_hat[t_prev]; fp32, one
// rounding per operation, in this order:
//   x0  = (x - sqrt(1 - a_t) * e) / sqrt(a_t)
//   r   = (1 - a_p) / (1 - a_t)        q = 1 - a_t / a_p
//   var = (eta * eta) * (r * q)        sigma = sqrt(var)        dir = sqrt(max((1 - a_p) - var, 0))
//   out = ((sqrt(a_p) * x0) + (dir * e)) + (noise ? sigma * noise : +0)
// The division by sqrt(a_t) stays a division (a reciprocal would round differently).
// masked: the generated region takes no noise when eta == 0 or t_prev == 0
struct Ddim {
  struct Args {
    const float* alpha_hat;
    int t, t_prev;
    const int64_t *t_dev, *t_prev_dev;
    float eta;
  };
  float sq1m_at, sq_at, sq_ap, sigma, dir, eta;
  int tp;
  __device__ __forceinline__ static Ddim make(const Args& a) {
    const int t = a.t_dev ? (int)a.t_dev[0] : a.t;
    const float eta = a.eta;
    Ddim k;
    k.tp = a.t_prev_dev ? (int)a.t_prev_dev[0] : a.t_prev;
    k.eta = eta;
    const float a_t = a.alpha_hat[t], a_p = a.alpha_hat[k.tp];
    k.sq1m_at = sqrtf(1.0f - a_t);
    k.sq_at = sqrtf(a_t);
    k.sq_ap = sqrtf(a_p);
    const float r = (1.0f - a_p) / (1.0f - a_t);
    const float q = 1.0f - a_t / a_p;
    const float var = (eta * eta) * (r * q);
    k.sigma = sqrtf(var);
    k.dir = sqrtf(fmaxf((1.0f - a_p) - var, 0.0f));
    return k;
  }
  __device__ __forceinline__ float update(float x, float e, float z, bool has_noise) const {
    const float pe = sq1m_at * e;
    const float x0 = (x - pe) / sq_at;
    const float mean = (sq_ap * x0) + (dir * e);
    const float nz = has_noise ? sigma * z : 0.0f;
    return mean + nz;
  }
  __device__ __forceinline__ int t_prev() const { return tp; }
  __device__ __forceinline__ bool gen_takes_noise() const { return eta != 0.0f && tp > 0; }
};

// masked step (inpainting, RePaint): the rule's update for the generated region, x0 noised to t_prev for the known one:
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

// The one loop of the family.  kCfg: eps holds 2n elements and s is the guidance scale.  kMasked: x0 and mask are read.  x_out
// may alias x (elementwise); x_out2 (optional) receives the same values: the guided sampler writes both halves of its 2n input
// buffer, so the next forward needs no concatenation.  VEC: 16-byte accesses and n counts float4s (launch_step decides).
// The loop stays in the kernel: in a __device__ body, blockDim.x would be read without the kernel's uniform-work-group
// assumption, one extra load per thread.
template <class Rule, bool kCfg, bool kMasked, bool VEC>
__global__ __launch_bounds__(256) void step_k(const float* x, const float* __restrict__ eps, const float* __restrict__ noise,
                                              const typename Rule::Args args, float s, const float* __restrict__ x0,
                                              const uint8_t* __restrict__ mask, float* x_out, float* x_out2, long n) {
  const Rule k = Rule::make(args);
  const Guidance g = guidance(s);
  const bool has_noise = noise != nullptr;
  const bool gen_noise = kMasked ? has_noise && k.gen_takes_noise() : has_noise;
  const KnownCoef kn = kMasked ? known_coef(args.alpha_hat, k.t_prev()) : KnownCoef{};
  auto gen = [&](float xv, float ec, float eu, float z) { return k.update(xv, guided_eps<kCfg>(g, ec, eu), z, gen_noise); };
  AFD_GRID_STRIDE(i, n) {
    if (VEC) {
      const float4 xv = reinterpret_cast<const float4*>(x)[i], c = reinterpret_cast<const float4*>(eps)[i];
      const float4 u = kCfg ? reinterpret_cast<const float4*>(eps)[n + i] : c;
      const float4 z = has_noise ? reinterpret_cast<const float4*>(noise)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 r = make_float4(gen(xv.x, c.x, u.x, z.x), gen(xv.y, c.y, u.y, z.y), gen(xv.z, c.z, u.z, z.z), gen(xv.w, c.w, u.w, z.w));
      if (kMasked)
        r = masked4(kn, reinterpret_cast<const uchar4*>(mask)[i], reinterpret_cast<const float4*>(x0)[i], z, r);
      reinterpret_cast<float4*>(x_out)[i] = r;
      if (x_out2) reinterpret_cast<float4*>(x_out2)[i] = r;
    } else {
      const float z = has_noise ? noise[i] : 0.0f;
      float r = gen(x[i], eps[i], kCfg ? eps[n + i] : 0.0f, z);
      if (kMasked && mask[i]) r = known_value(kn, x0[i], z);
      x_out[i] = r;
      if (x_out2) x_out2[i] = r;
    }
  }
}

// Launch geometry of the streaming step kernels (these, renoise, DPM++): 16-byte accesses when n % 4 == 0 and every pointer
// given is 16-byte aligned (an absent optional pointer, NULL, counts as aligned); memory-bound, so at most 2048 workgroups and
// the loop takes the rest.
static inline bool vec_ok(long n, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (!aligned16(p)) return false;
  return n % 4 == 0;
}
static inline long step_grid(long work) { return std::min<long>(2048, std::max<long>(1, (work + 255) / 256)); }

template <class Rule, bool kCfg, bool kMasked>
static void launch_step(const float* x, const float* eps, const float* noise, const typename Rule::Args& args, float s,
                        const float* x0, const uint8_t* mask, float* x_out, float* x_out2, long n, hipStream_t st) {
  // The plain DDPM step keeps the geometry it has always had, scalar accesses on up to 32768 workgroups (gs_grid): the 16-byte
  // form has not been shown to be as fast on the flagship's sampling loop.
  const bool plain_ddpm = !kCfg && !kMasked && std::is_same<Rule, Ddpm>::value;
  const bool vec = !plain_ddpm && vec_ok(n, {x, eps, noise, x0, x_out, x_out2}) && (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
  const long work = vec ? n / 4 : n;
  auto kern = vec ? step_k<Rule, kCfg, kMasked, true> : step_k<Rule, kCfg, kMasked, false>;
  hipLaunchKernelGGL(kern, dim3(plain_ddpm ? gs_grid(n) : step_grid(work)), dim3(256), 0, st, x, eps, noise, args, s, x0, mask, x_out,
                     x_out2, work);
}

// ---- the checks of the step family's entry points ----
// Which of a sampler's eight entry points is being served: its name (for messages), whether the step indices are read on the
// device, whether eps holds the guided 2n rows, whether x0 / mask select a known region.
struct StepForm {
  const char* name;
  bool dev, cfg, masked;
};
// x0 and mask are read by every element while x_out / x_out2 are written: they must not share memory
static inline bool masked_inputs_apart(const float* x0, const uint8_t* mask, const float* x_out, const float* x_out2, long n) {
  const long fb = n * (long)sizeof(float);
  return !overlaps(x0, fb, x_out, fb) && !overlaps(x0, fb, x_out2, fb) && !overlaps(mask, n, x_out, fb) && !overlaps(mask, n, x_out2, fb);
}
// The checks both samplers share, before their own: the pointers (tables_ok: the sampler's schedule tables and device indices,
// named by `tables`), n, and the masked forms' x0 / mask against the outputs.
static int check_step_buffers(const StepForm& f, bool tables_ok, const char* tables, const float* x, const float* eps,
                              const float* x0, const uint8_t* mask, const float* x_out, const float* x_out2, long n) {
  AFD_REQUIRE(x && eps && x_out && tables_ok && (!f.masked || (x0 && mask)), "%s: x, %s%s, %s and x_out must not be NULL", f.name,
              f.cfg ? "eps2" : "eps", f.masked ? ", x0, mask" : "", tables);
  AFD_REQUIRE(n > 0, "%s: n must be positive (got %ld)", f.name, n);
  AFD_REQUIRE(!f.masked || masked_inputs_apart(x0, mask, x_out, x_out2, n), "%s: x0 and mask must not overlap x_out or x_out2", f.name);
  return AFD_OK;
}
// After the sampler's own checks: the known region is x0 noised to t_prev, so it needs the noise unless t_prev == 0.  t_prev < 0:
// not known on the host (a *_dev form), where the noise is always required.
static int check_known_noise(const StepForm& f, const float* noise, int t_prev) {
  AFD_REQUIRE(!f.masked || noise || t_prev == 0, "%s: noise must not be NULL %s(it noises the known region)", f.name,
              f.dev ? "" : "when t_prev > 0 ");
  return AFD_OK;
}
template <class Rule>
static int launch_step_form(const StepForm& f, const float* x, const float* eps, const float* noise, const typename Rule::Args& args,
                            float s, const float* x0, const uint8_t* mask, float* x_out, float* x_out2, long n, afd_stream_t st) {
  auto launch = f.cfg ? (f.masked ? launch_step<Rule, true, true> : launch_step<Rule, true, false>)
                      : (f.masked ? launch_step<Rule, false, true> : launch_step<Rule, false, false>);
  launch(x, eps, noise, args, s, x0, mask, x_out, x_out2, n, as_stream(st));
  return check_launch(f.name);
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
  float alpha, sigma, A, B0, B1;
};
__device__ __forceinline__ float dpmpp_update(const DpmCoef& k, float x, float e, float xp, bool has_prev, float& x0) {
  const float pe = k.sigma * e;
  x0 = (x - pe) / k.alpha;
  const float l = k.A * x, r = k.B0 * x0;
  const float m = l + r;
  const float p = has_prev ? k.B1 * xp : 0.0f;
  return m + p;
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
  const Guidance g = guidance(s);
  const bool has_prev = x0_prev != nullptr;
  AFD_GRID_STRIDE(i, n) {
    if (VEC) {
      const float4 xv = reinterpret_cast<const float4*>(x)[i], c = reinterpret_cast<const float4*>(eps)[i];
      const float4 u = kCfg ? reinterpret_cast<const float4*>(eps)[n + i] : c;
      const float4 p = has_prev ? reinterpret_cast<const float4*>(x0_prev)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 r, x0;
      r.x = dpmpp_update(k, xv.x, guided_eps<kCfg>(g, c.x, u.x), p.x, has_prev, x0.x);
      r.y = dpmpp_update(k, xv.y, guided_eps<kCfg>(g, c.y, u.y), p.y, has_prev, x0.y);
      r.z = dpmpp_update(k, xv.z, guided_eps<kCfg>(g, c.z, u.z), p.z, has_prev, x0.z);
      r.w = dpmpp_update(k, xv.w, guided_eps<kCfg>(g, c.w, u.w), p.w, has_prev, x0.w);
      reinterpret_cast<float4*>(x_out)[i] = r;
      if (x_out2) reinterpret_cast<float4*>(x_out2)[i] = r;
      reinterpret_cast<float4*>(x0_out)[i] = x0;
    } else {
      float x0;
      const float e = guided_eps<kCfg>(g, eps[i], kCfg ? eps[n + i] : 0.0f);
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
  const bool vec = vec_ok(n, {x, eps, x0_prev, x_out, x_out2, x0_out});
  const long work = vec ? n / 4 : n;
  const long grid = step_grid(work);
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
// with mean_j = Ddpm::update's fp32 expression at step 1 without noise, c1 * (x_t - c2 * eps_hat) (what the sampler returns).
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
    const Ddpm k = Ddpm::at(alpha, alpha_hat, beta, 1);
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
          s_ll += decoder_log_prob(vv[q], k.update(xv[q], hv[q], 0.0f, false), inv_stdv);
        }
      } else {
        const double d = (double)eps_hat[row + j] - (double)eps[row + j];
        s_sq += d * d;
        s_ll += decoder_log_prob(x0[src + j], k.update(xt[row + j], eps_hat[row + j], 0.0f, false), inv_stdv);
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
  Ddpm dec;                // the DDPM rule at step 1
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
  w.dec = Ddpm::at(alpha, alpha_hat, beta, 1);
  return w;
}
template <bool GRAD>
__device__ __forceinline__ double lvar_term(const LvarRow& w, int kind, float p, float v, float x0, float e, float xt, double& sq,
                                            double& dlv) {
  const double df = lvar_diff(kind, p, x0, e, w.sa64, w.sb64);
  sq = w.f2 * (df * df);
  if (w.is_dec) {
    const float mean = w.dec.update(xt, lvar_eps_hat(kind, p, xt, w.sa, w.sb), 0.0f, false);
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
//   x_out = c1 (x - c2 eps_hat) + (float)exp(logvar / 2) noise,  Ddpm::update's mean; no noise at step 1 or with noise NULL.
// x_out may be x itself (each thread reads its quad before it writes it); x_out2 (optional) receives the same values.
__device__ __forceinline__ float lvar_update(const Ddpm& k, float x, float e, float v, float z, double lb, double lbt, bool has_noise) {
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
  const Ddpm k = Ddpm::at(alpha, alpha_hat, beta, step);
  const Guidance g = guidance(s);
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
    r.x = lvar_update(k, xv.x, guided_eps<kCfg>(g, lvar_eps_hat(kind, c.x, xv.x, sa, sb), lvar_eps_hat(kind, u.x, xv.x, sa, sb)), v.x, z.x, lb, lbt, has_noise);
    r.y = lvar_update(k, xv.y, guided_eps<kCfg>(g, lvar_eps_hat(kind, c.y, xv.y, sa, sb), lvar_eps_hat(kind, u.y, xv.y, sa, sb)), v.y, z.y, lb, lbt, has_noise);
    r.z = lvar_update(k, xv.z, guided_eps<kCfg>(g, lvar_eps_hat(kind, c.z, xv.z, sa, sb), lvar_eps_hat(kind, u.z, xv.z, sa, sb)), v.z, z.z, lb, lbt, has_noise);
    r.w = lvar_update(k, xv.w, guided_eps<kCfg>(g, lvar_eps_hat(kind, c.w, xv.w, sa, sb), lvar_eps_hat(kind, u.w, xv.w, sa, sb)), v.w, z.w, lb, lbt, has_noise);
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
// ---- sampler steps: afd_denoise_step* (DDPM) and afd_ddim_step* (DDIM) -----------------------------------------------------------
// DDPM: i >= 0, and i >= 1 for the masked forms (the step i -> i - 1)
static int ddpm_step(const StepForm& f, const float* x, const float* eps, const float* noise, const float* x0, const uint8_t* mask,
                     const float* alpha, const float* alpha_hat, const float* beta, int i, const int64_t* t_dev, float s, float* x_out,
                     float* x_out2, long n, afd_stream_t st) {
  if (int rc = check_step_buffers(f, alpha && alpha_hat && beta && (!f.dev || t_dev), f.dev ? "alpha, alpha_hat, beta, t_dev" : "alpha, alpha_hat, beta",
                                  x, eps, x0, mask, x_out, x_out2, n))
    return rc;
  AFD_REQUIRE(f.dev || i >= (f.masked ? 1 : 0), "%s: need i >= %d (got i = %d)", f.name, f.masked ? 1 : 0, i);
  if (int rc = check_known_noise(f, noise, f.dev ? -1 : i - 1)) return rc;
  return launch_step_form<Ddpm>(f, x, eps, noise, Ddpm::Args{alpha, alpha_hat, beta, i, t_dev}, s, x0, mask, x_out, x_out2, n, st);
}
int afd_denoise_step(const float* x, const float* eps_pred, const float* noise, const float* alpha, const float* alpha_hat,
                     const float* beta, int i, float* x_out, long n, afd_stream_t st) {
  return ddpm_step({"afd_denoise_step", false, false, false}, x, eps_pred, noise, nullptr, nullptr, alpha, alpha_hat, beta, i, nullptr,
                   0.0f, x_out, nullptr, n, st);
}
int afd_denoise_step_dev(const float* x, const float* eps_pred, const float* noise, const float* alpha, const float* alpha_hat,
                         const float* beta, const int64_t* t_dev, float* x_out, long n, afd_stream_t st) {
  return ddpm_step({"afd_denoise_step_dev", true, false, false}, x, eps_pred, noise, nullptr, nullptr, alpha, alpha_hat, beta, 0, t_dev,
                   0.0f, x_out, nullptr, n, st);
}
int afd_denoise_step_cfg(const float* x, const float* eps2, const float* noise, const float* alpha, const float* alpha_hat,
                         const float* beta, int i, float cfg_scale, float* x_out, float* x_out2, long n, afd_stream_t st) {
  return ddpm_step({"afd_denoise_step_cfg", false, true, false}, x, eps2, noise, nullptr, nullptr, alpha, alpha_hat, beta, i, nullptr,
                   cfg_scale, x_out, x_out2, n, st);
}
int afd_denoise_step_cfg_dev(const float* x, const float* eps2, const float* noise, const float* alpha, const float* alpha_hat,
                             const float* beta, const int64_t* t_dev, float cfg_scale, float* x_out, float* x_out2, long n,
                             afd_stream_t st) {
  return ddpm_step({"afd_denoise_step_cfg_dev", true, true, false}, x, eps2, noise, nullptr, nullptr, alpha, alpha_hat, beta, 0, t_dev,
                   cfg_scale, x_out, x_out2, n, st);
}
int afd_denoise_step_masked(const float* x, const float* eps_pred, const float* noise, const float* x0, const uint8_t* mask,
                            const float* alpha, const float* alpha_hat, const float* beta, int i, float* x_out, long n,
                            afd_stream_t st) {
  return ddpm_step({"afd_denoise_step_masked", false, false, true}, x, eps_pred, noise, x0, mask, alpha, alpha_hat, beta, i, nullptr, 0.0f,
                   x_out, nullptr, n, st);
}
int afd_denoise_step_masked_dev(const float* x, const float* eps_pred, const float* noise, const float* x0, const uint8_t* mask,
                                const float* alpha, const float* alpha_hat, const float* beta, const int64_t* t_dev, float* x_out,
                                long n, afd_stream_t st) {
  return ddpm_step({"afd_denoise_step_masked_dev", true, false, true}, x, eps_pred, noise, x0, mask, alpha, alpha_hat, beta, 0, t_dev, 0.0f,
                   x_out, nullptr, n, st);
}
int afd_denoise_step_masked_cfg(const float* x, const float* eps2, const float* noise, const float* x0, const uint8_t* mask,
                                const float* alpha, const float* alpha_hat, const float* beta, int i, float cfg_scale, float* x_out,
                                float* x_out2, long n, afd_stream_t st) {
  return ddpm_step({"afd_denoise_step_masked_cfg", false, true, true}, x, eps2, noise, x0, mask, alpha, alpha_hat, beta, i, nullptr,
                   cfg_scale, x_out, x_out2, n, st);
}
int afd_denoise_step_masked_cfg_dev(const float* x, const float* eps2, const float* noise, const float* x0, const uint8_t* mask,
                                    const float* alpha, const float* alpha_hat, const float* beta, const int64_t* t_dev,
                                    float cfg_scale, float* x_out, float* x_out2, long n, afd_stream_t st) {
  return ddpm_step({"afd_denoise_step_masked_cfg_dev", true, true, true}, x, eps2, noise, x0, mask, alpha, alpha_hat, beta, 0, t_dev,
                   cfg_scale, x_out, x_out2, n, st);
}

// DDIM: 0 <= t_prev < t where the host knows them, eta >= 0 (a NaN eta fails the comparison)
static int ddim_step(const StepForm& f, const float* x, const float* eps, const float* noise, const float* x0, const uint8_t* mask,
                     const float* alpha_hat, int t, int t_prev, const int64_t* t_dev, const int64_t* t_prev_dev, float eta, float s,
                     float* x_out, float* x_out2, long n, afd_stream_t st) {
  if (int rc = check_step_buffers(f, alpha_hat && (!f.dev || (t_dev && t_prev_dev)), f.dev ? "alpha_hat, t_dev, t_prev_dev" : "alpha_hat", x, eps,
                                  x0, mask, x_out, x_out2, n))
    return rc;
  AFD_REQUIRE(f.dev || (t_prev >= 0 && t_prev < t), "%s: need 0 <= t_prev < t (got t = %d, t_prev = %d)", f.name, t, t_prev);
  AFD_REQUIRE(eta >= 0.0f, "%s: eta must be >= 0", f.name);
  if (int rc = check_known_noise(f, noise, f.dev ? -1 : t_prev)) return rc;
  return launch_step_form<Ddim>(f, x, eps, noise, Ddim::Args{alpha_hat, t, t_prev, t_dev, t_prev_dev, eta}, s, x0, mask, x_out, x_out2, n,
                                st);
}
int afd_ddim_step(const float* x, const float* eps, const float* noise, const float* alpha_hat, int t, int t_prev, float eta,
                  float* x_out, long n, afd_stream_t st) {
  return ddim_step({"afd_ddim_step", false, false, false}, x, eps, noise, nullptr, nullptr, alpha_hat, t, t_prev, nullptr, nullptr, eta, 0.0f,
                   x_out, nullptr, n, st);
}
int afd_ddim_step_dev(const float* x, const float* eps, const float* noise, const float* alpha_hat, const int64_t* t_dev,
                      const int64_t* t_prev_dev, float eta, float* x_out, long n, afd_stream_t st) {
  return ddim_step({"afd_ddim_step_dev", true, false, false}, x, eps, noise, nullptr, nullptr, alpha_hat, 0, 0, t_dev, t_prev_dev, eta, 0.0f,
                   x_out, nullptr, n, st);
}
int afd_ddim_step_cfg(const float* x, const float* eps2, const float* noise, const float* alpha_hat, int t, int t_prev, float eta,
                      float cfg_scale, float* x_out, float* x_out2, long n, afd_stream_t st) {
  return ddim_step({"afd_ddim_step_cfg", false, true, false}, x, eps2, noise, nullptr, nullptr, alpha_hat, t, t_prev, nullptr, nullptr, eta,
                   cfg_scale, x_out, x_out2, n, st);
}
int afd_ddim_step_cfg_dev(const float* x, const float* eps2, const float* noise, const float* alpha_hat, const int64_t* t_dev,
                          const int64_t* t_prev_dev, float eta, float cfg_scale, float* x_out, float* x_out2, long n, afd_stream_t st) {
  return ddim_step({"afd_ddim_step_cfg_dev", true, true, false}, x, eps2, noise, nullptr, nullptr, alpha_hat, 0, 0, t_dev, t_prev_dev, eta,
                   cfg_scale, x_out, x_out2, n, st);
}
int afd_ddim_step_masked(const float* x, const float* eps, const float* noise, const float* x0, const uint8_t* mask,
                         const float* alpha_hat, int t, int t_prev, float eta, float* x_out, long n, afd_stream_t st) {
  return ddim_step({"afd_ddim_step_masked", false, false, true}, x, eps, noise, x0, mask, alpha_hat, t, t_prev, nullptr, nullptr, eta, 0.0f,
                   x_out, nullptr, n, st);
}
int afd_ddim_step_masked_dev(const float* x, const float* eps, const float* noise, const float* x0, const uint8_t* mask,
                             const float* alpha_hat, const int64_t* t_dev, const int64_t* t_prev_dev, float eta, float* x_out, long n,
                             afd_stream_t st) {
  return ddim_step({"afd_ddim_step_masked_dev", true, false, true}, x, eps, noise, x0, mask, alpha_hat, 0, 0, t_dev, t_prev_dev, eta, 0.0f,
                   x_out, nullptr, n, st);
}
int afd_ddim_step_masked_cfg(const float* x, const float* eps2, const float* noise, const float* x0, const uint8_t* mask,
                             const float* alpha_hat, int t, int t_prev, float eta, float cfg_scale, float* x_out, float* x_out2, long n,
                             afd_stream_t st) {
  return ddim_step({"afd_ddim_step_masked_cfg", false, true, true}, x, eps2, noise, x0, mask, alpha_hat, t, t_prev, nullptr, nullptr, eta,
                   cfg_scale, x_out, x_out2, n, st);
}
int afd_ddim_step_masked_cfg_dev(const float* x, const float* eps2, const float* noise, const float* x0, const uint8_t* mask,
                                 const float* alpha_hat, const int64_t* t_dev, const int64_t* t_prev_dev, float eta, float cfg_scale,
                                 float* x_out, float* x_out2, long n, afd_stream_t st) {
  return ddim_step({"afd_ddim_step_masked_cfg_dev", true, true, true}, x, eps2, noise, x0, mask, alpha_hat, 0, 0, t_dev, t_prev_dev, eta,
                   cfg_scale, x_out, x_out2, n, st);
}

// ---- renoise (the inpainting sampler's up-move) -----------------------------------------------------------------------------------
int afd_renoise(const float* x, const float* noise, const float* alpha_hat, int t_from, int t_to, float* x_out, long n,
                afd_stream_t st) {
  AFD_REQUIRE(x && noise && alpha_hat && x_out, "afd_renoise: x, noise, alpha_hat and x_out must not be NULL");
  AFD_REQUIRE(n > 0, "afd_renoise: n must be positive (got %ld)", n);
  AFD_REQUIRE(t_from >= 0 && t_from < t_to, "afd_renoise: need 0 <= t_from < t_to (got t_from = %d, t_to = %d)", t_from, t_to);
  if (vec_ok(n, {x, noise, x_out}))
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
  const bool vec = vec_ok(chw, {x, out2, noise, x_out, x_out2});
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

}  // extern "C"

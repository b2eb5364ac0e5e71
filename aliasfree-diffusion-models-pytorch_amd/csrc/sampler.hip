// sampler.hip -- the samplers: noising, the sampler steps (DDPM, DDIM, DPM-Solver++(2M), UniPC; plain, guided and masked), the ascending
// DDIM step of the inversion, renoise and quantisation.  (Losses, learned variances and the likelihood bound are objective.hip, the optimizer is optim.hip.)
//
// noise_images / denoise_step / quantize restate the reference's fp32 expression ORDER with one
// IEEE rounding per torch op (no FMA contraction, correctly rounded sqrt and divide), so given the
// same inputs they are bit-identical to the reference's CPU path (ddpm_models.py:317-321,367-374,381-385).
// hipcc keeps `/` and sqrtf correctly rounded by default; `#pragma clang fp contract(off)` below
// stops a*b+c from fusing.  (The __f*_rn intrinsics are NOT used: without
// OCML_BASIC_ROUNDED_OPERATIONS this toolchain maps __fsqrt_rn to the approximate native sqrt.)
#include "common.h"

#pragma clang fp contract(off)

#include "diffusion_common.h"

namespace afd {

// x_t = sqrt(ah[t]) * x + sqrt(1 - ah[t]) * eps
__global__ void noise_images_k(const float* __restrict__ x, const float* __restrict__ eps, const int64_t* __restrict__ t,
                               const float* __restrict__ alpha_hat, float* __restrict__ xt, long per, long total) {
  AFD_GRID_STRIDE(i, total) {
    const long b = i / per;
    const Roots k = roots(alpha_hat[t[b]]);
    xt[i] = noised(k.sa, k.sb, x[i], eps[i]);
  }
}

// ---- sampler steps: DDPM and DDIM, plain, guided (kCfg), masked (kMasked) or both, one kernel template --------------------------
// (Guidance and the Ddpm rule: diffusion_common.h.)

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

// DDIM with the noise scale read from a table (Analytic-DPM, Bao et al. 2022): sig (T floats) holds the optimal sigma of the step
// that leaves t, built on the host (analytic.py).  Everything but sigma is Ddim's, from the same fp32 expressions, so the mean is
// DDIM's at that eta and the output is Ddim's bit for bit whenever sig[t] holds Ddim's own sigma.  No masked form: t_prev() and
// gen_takes_noise() are here because step_k names them.
struct DdimVar {
  struct Args : Ddim::Args {
    const float* sig;
  };
  Ddim k;
  __device__ __forceinline__ static DdimVar make(const Args& a) {
    DdimVar v;
    v.k = Ddim::make(a);
    v.k.sigma = a.sig[a.t_dev ? (int)a.t_dev[0] : a.t];
    return v;
  }
  __device__ __forceinline__ float update(float x, float e, float z, bool has_noise) const { return k.update(x, e, z, has_noise); }
  __device__ __forceinline__ int t_prev() const { return k.tp; }
  __device__ __forceinline__ bool gen_takes_noise() const { return k.tp > 0; }
};

// The ascending DDIM step (inversion), one move s -> u of a chain walked upwards, 0 <= s < u.  a_s = alpha_hat[s],
// a_u = alpha_hat[u]; fp32, one rounding per operation, in this order:
//   x0  = (x - sqrt(1 - a_s) * e) / sqrt(a_s)
//   out = (sqrt(a_u) * x0) + (sqrt(1 - a_u) * e)
// the algebraic inverse of Ddim's eta = 0 step u -> s for the e that step used (there dir = sqrt(1 - a_s) and no noise term).
// It takes no noise and has no masked form: t_prev() and gen_takes_noise() are here because step_k names them.
struct DdimInvert {
  struct Args {
    const float* alpha_hat;
    int s, u;
    const int64_t *s_dev, *u_dev;
  };
  float sq1m_as, sq_as, sq_au, sq1m_au;
  __device__ __forceinline__ static DdimInvert make(const Args& a) {
    const int s = a.s_dev ? (int)a.s_dev[0] : a.s, u = a.u_dev ? (int)a.u_dev[0] : a.u;
    const float a_s = a.alpha_hat[s], a_u = a.alpha_hat[u];
    DdimInvert k;
    k.sq1m_as = sqrtf(1.0f - a_s);
    k.sq_as = sqrtf(a_s);
    k.sq_au = sqrtf(a_u);
    k.sq1m_au = sqrtf(1.0f - a_u);
    return k;
  }
  __device__ __forceinline__ float update(float x, float e, float, bool) const {
    const float pe = sq1m_as * e;
    const float x0 = (x - pe) / sq_as;
    return noised(sq_au, sq1m_au, x0, e);
  }
  __device__ __forceinline__ int t_prev() const { return 0; }
  __device__ __forceinline__ bool gen_takes_noise() const { return false; }
};

// masked step (inpainting, RePaint): the rule's update for the generated region, x0 noised to t_prev for the known one:
// known = t_prev == 0 ? x0 : (sqrt(a_p) * x0) + (sqrt(1 - a_p) * z), a_p = alpha_hat[t_prev] (noised)
// out   = mask[j] ? known : gen.  One noise tensor z serves both regions (each element reads its z once).
struct KnownCoef {
  Roots rt;
  bool clean;
};
__device__ __forceinline__ KnownCoef known_coef(const float* alpha_hat, int tp) { return KnownCoef{roots(alpha_hat[tp]), tp == 0}; }
__device__ __forceinline__ float known_value(const KnownCoef& k, float x0, float z) {
  return k.clean ? x0 : noised(k.rt.sa, k.rt.sb, x0, z);
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

// Launch geometry of the streaming step kernels (these, renoise, DPM++, UniPC): 16-byte accesses when vec_ok; memory-bound, so at most
// 2048 workgroups and the loop takes the rest.
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
      reinterpret_cast<float4*>(x_out)[i] = quad_map([=](float xi, float zi) { return noised(sa, sb, xi, zi); }, xv, z);
    } else {
      x_out[i] = noised(sa, sb, x[i], noise[i]);
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
  launch_vec(vec, dpmpp_step_k<kCfg, true>, dpmpp_step_k<kCfg, false>, step_grid(work), st, x, eps, x0_prev, coef, s, x_out, x_out2,
             x0_out, work);
}

// ---- UniPC (Zhao et al. 2023), orders 1-3: the corrector of the last move and the predictor of the next, one launch -------------
// coef (device, 12 floats, one row of Diffusion.unipc_coefficients) = [alpha, sigma, Ac, c0, c1, c2, c3, Ap, p0, p1, p2, slot];
// fp32, one rounding per operation, in this order:
//   m  = (x - (sigma * e)) / alpha
//   xc = ((((Ac * xc) + (c0 * m)) + (c1 * h1)) + (c2 * h2)) + (c3 * h3)
//   xn = (((Ap * xc) + (p0 * m)) + (p1 * h1)) + (p2 * h2)
// hist is a ring of three n-element planes: h_j is plane (slot - j) mod 3 and m goes to plane `slot`, which is h3's (each element
// reads its h3 before it writes m).  slot is read on the device and clamped into {0, 1, 2}.  Every term is always evaluated:
// the table's zero weights meet a zeroed or finite history.  xc is updated in place; xn goes to x_out (may alias x) and to the
// optional x_out2.  With CFG, e is cfg_lerp of the two halves of eps2 first.  VEC: n % 4 == 0, every pointer 16-byte aligned
// (then the planes are too); n counts float4s.
struct UniCoef {
  float alpha, sigma, Ac, c0, c1, c2, c3, Ap, p0, p1, p2;
};
__device__ __forceinline__ float unipc_update(const UniCoef& k, float x, float e, float h1, float h2, float h3, float& xc, float& m) {
  const float pe = k.sigma * e;
  m = (x - pe) / k.alpha;
  float c = (k.Ac * xc) + (k.c0 * m);
  c = c + (k.c1 * h1);
  c = c + (k.c2 * h2);
  c = c + (k.c3 * h3);
  xc = c;
  float p = (k.Ap * c) + (k.p0 * m);
  p = p + (k.p1 * h1);
  return p + (k.p2 * h2);
}
template <bool kCfg, bool VEC>
__global__ __launch_bounds__(256) void unipc_step_k(const float* x, const float* __restrict__ eps, float* __restrict__ xc, float* hist,
                                                    const float* __restrict__ coef, float s, float* x_out, float* x_out2, long n) {
  const UniCoef k{coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], coef[6], coef[7], coef[8], coef[9], coef[10]};
  const float sf = coef[11];
  const int slot = sf >= 1.5f ? 2 : (sf >= 0.5f ? 1 : 0);          // clamped; anything else (a NaN too) reads as 0
  const long plane = VEC ? 4 * n : n;                           // floats per plane of the ring
  const float* h1 = hist + ((slot + 2) % 3) * plane;
  const float* h2 = hist + ((slot + 1) % 3) * plane;
  float* h3 = hist + slot * plane;                              // read as h3, then written with m
  const Guidance g = guidance(s);
  AFD_GRID_STRIDE(i, n) {
    if (VEC) {
      const float4 xv = reinterpret_cast<const float4*>(x)[i], c = reinterpret_cast<const float4*>(eps)[i];
      const float4 u = kCfg ? reinterpret_cast<const float4*>(eps)[n + i] : c;
      const float4 a1 = reinterpret_cast<const float4*>(h1)[i], a2 = reinterpret_cast<const float4*>(h2)[i];
      const float4 a3 = reinterpret_cast<const float4*>(h3)[i];
      float4 cv = reinterpret_cast<const float4*>(xc)[i], r, m;
      r.x = unipc_update(k, xv.x, guided_eps<kCfg>(g, c.x, u.x), a1.x, a2.x, a3.x, cv.x, m.x);
      r.y = unipc_update(k, xv.y, guided_eps<kCfg>(g, c.y, u.y), a1.y, a2.y, a3.y, cv.y, m.y);
      r.z = unipc_update(k, xv.z, guided_eps<kCfg>(g, c.z, u.z), a1.z, a2.z, a3.z, cv.z, m.z);
      r.w = unipc_update(k, xv.w, guided_eps<kCfg>(g, c.w, u.w), a1.w, a2.w, a3.w, cv.w, m.w);
      reinterpret_cast<float4*>(x_out)[i] = r;
      if (x_out2) reinterpret_cast<float4*>(x_out2)[i] = r;
      reinterpret_cast<float4*>(xc)[i] = cv;
      reinterpret_cast<float4*>(h3)[i] = m;
    } else {
      const float e = guided_eps<kCfg>(g, eps[i], kCfg ? eps[n + i] : 0.0f);
      float cv = xc[i], m;
      const float r = unipc_update(k, x[i], e, h1[i], h2[i], h3[i], cv, m);
      x_out[i] = r;
      if (x_out2) x_out2[i] = r;
      xc[i] = cv;
      h3[i] = m;
    }
  }
}
template <bool kCfg>
static void launch_unipc_step(const float* x, const float* eps, float* xc, float* hist, const float* coef, float s, float* x_out,
                              float* x_out2, long n, hipStream_t st) {
  const bool vec = vec_ok(n, {x, eps, xc, hist, x_out, x_out2});
  const long work = vec ? n / 4 : n;
  launch_vec(vec, unipc_step_k<kCfg, true>, unipc_step_k<kCfg, false>, step_grid(work), st, x, eps, xc, hist, coef, s, x_out, x_out2,
             work);
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

// DDIM with sigma from a table (Analytic-DPM): ddim_step's checks, sig among the tables.  sig[t] is read on the device, unchecked.
static int ddim_step_var(const StepForm& f, const float* x, const float* eps, const float* noise, const float* alpha_hat,
                         const float* sig, int t, int t_prev, const int64_t* t_dev, const int64_t* t_prev_dev, float eta, float s,
                         float* x_out, float* x_out2, long n, afd_stream_t st) {
  if (int rc = check_step_buffers(f, alpha_hat && sig && (!f.dev || (t_dev && t_prev_dev)),
                                  f.dev ? "alpha_hat, sig, t_dev, t_prev_dev" : "alpha_hat, sig", x, eps, nullptr, nullptr, x_out, x_out2, n))
    return rc;
  AFD_REQUIRE(f.dev || (t_prev >= 0 && t_prev < t), "%s: need 0 <= t_prev < t (got t = %d, t_prev = %d)", f.name, t, t_prev);
  AFD_REQUIRE(eta >= 0.0f, "%s: eta must be >= 0", f.name);
  auto launch = f.cfg ? launch_step<DdimVar, true, false> : launch_step<DdimVar, false, false>;      // (no masked kernels)
  launch(x, eps, noise, DdimVar::Args{{alpha_hat, t, t_prev, t_dev, t_prev_dev, eta}, sig}, s, nullptr, nullptr, x_out, x_out2, n,
         as_stream(st));
  return check_launch(f.name);
}
int afd_ddim_step_var(const float* x, const float* eps, const float* noise, const float* alpha_hat, const float* sig, int t, int t_prev,
                      float eta, float* x_out, long n, afd_stream_t st) {
  return ddim_step_var({"afd_ddim_step_var", false, false, false}, x, eps, noise, alpha_hat, sig, t, t_prev, nullptr, nullptr, eta, 0.0f,
                       x_out, nullptr, n, st);
}
int afd_ddim_step_var_dev(const float* x, const float* eps, const float* noise, const float* alpha_hat, const float* sig,
                          const int64_t* t_dev, const int64_t* t_prev_dev, float eta, float* x_out, long n, afd_stream_t st) {
  return ddim_step_var({"afd_ddim_step_var_dev", true, false, false}, x, eps, noise, alpha_hat, sig, 0, 0, t_dev, t_prev_dev, eta, 0.0f,
                       x_out, nullptr, n, st);
}
int afd_ddim_step_var_cfg(const float* x, const float* eps2, const float* noise, const float* alpha_hat, const float* sig, int t,
                          int t_prev, float eta, float cfg_scale, float* x_out, float* x_out2, long n, afd_stream_t st) {
  return ddim_step_var({"afd_ddim_step_var_cfg", false, true, false}, x, eps2, noise, alpha_hat, sig, t, t_prev, nullptr, nullptr, eta,
                       cfg_scale, x_out, x_out2, n, st);
}
int afd_ddim_step_var_cfg_dev(const float* x, const float* eps2, const float* noise, const float* alpha_hat, const float* sig,
                              const int64_t* t_dev, const int64_t* t_prev_dev, float eta, float cfg_scale, float* x_out, float* x_out2,
                              long n, afd_stream_t st) {
  return ddim_step_var({"afd_ddim_step_var_cfg_dev", true, true, false}, x, eps2, noise, alpha_hat, sig, 0, 0, t_dev, t_prev_dev, eta,
                       cfg_scale, x_out, x_out2, n, st);
}

// The ascending DDIM step: 0 <= s < u where the host knows them.  x_out is normally apart from x (the refinement re-reads the
// base state) and may be x itself; eps is read by other elements while x_out / x_out2 are written, so they share no memory.
static int ddim_invert_step(const StepForm& f, const float* x, const float* eps, const float* alpha_hat, int s, int u,
                            const int64_t* s_dev, const int64_t* u_dev, float scale, float* x_out, float* x_out2, long n,
                            afd_stream_t st) {
  if (int rc = check_step_buffers(f, alpha_hat && (!f.dev || (s_dev && u_dev)), f.dev ? "alpha_hat, s_dev, u_dev" : "alpha_hat", x, eps,
                                  nullptr, nullptr, x_out, x_out2, n))
    return rc;
  AFD_REQUIRE(f.dev || (s >= 0 && s < u), "%s: need 0 <= s < u (got s = %d, u = %d)", f.name, s, u);
  const long fb = n * (long)sizeof(float), eb = (f.cfg ? 2 : 1) * fb;
  AFD_REQUIRE(!overlaps(eps, eb, x_out, fb) && !overlaps(eps, eb, x_out2, fb), "%s: x_out and x_out2 must not overlap %s", f.name,
              f.cfg ? "eps2" : "eps");
  AFD_REQUIRE((x_out == x || !overlaps(x, fb, x_out, fb)) && (x_out2 == x || !overlaps(x, fb, x_out2, fb)),
              "%s: x_out and x_out2 must each be x itself or apart from it", f.name);
  auto launch = f.cfg ? launch_step<DdimInvert, true, false> : launch_step<DdimInvert, false, false>;      // (no masked kernels)
  launch(x, eps, nullptr, DdimInvert::Args{alpha_hat, s, u, s_dev, u_dev}, scale, nullptr, nullptr, x_out, x_out2, n, as_stream(st));
  return check_launch(f.name);
}
int afd_ddim_invert_step(const float* x, const float* eps, const float* alpha_hat, int s, int u, float* x_out, long n, afd_stream_t st) {
  return ddim_invert_step({"afd_ddim_invert_step", false, false, false}, x, eps, alpha_hat, s, u, nullptr, nullptr, 0.0f, x_out, nullptr, n,
                          st);
}
int afd_ddim_invert_step_dev(const float* x, const float* eps, const float* alpha_hat, const int64_t* s_dev, const int64_t* u_dev,
                             float* x_out, long n, afd_stream_t st) {
  return ddim_invert_step({"afd_ddim_invert_step_dev", true, false, false}, x, eps, alpha_hat, 0, 0, s_dev, u_dev, 0.0f, x_out, nullptr, n,
                          st);
}
int afd_ddim_invert_step_cfg(const float* x, const float* eps2, const float* alpha_hat, int s, int u, float cfg_scale, float* x_out,
                             float* x_out2, long n, afd_stream_t st) {
  return ddim_invert_step({"afd_ddim_invert_step_cfg", false, true, false}, x, eps2, alpha_hat, s, u, nullptr, nullptr, cfg_scale, x_out,
                          x_out2, n, st);
}
int afd_ddim_invert_step_cfg_dev(const float* x, const float* eps2, const float* alpha_hat, const int64_t* s_dev, const int64_t* u_dev,
                                 float cfg_scale, float* x_out, float* x_out2, long n, afd_stream_t st) {
  return ddim_invert_step({"afd_ddim_invert_step_cfg_dev", true, true, false}, x, eps2, alpha_hat, 0, 0, s_dev, u_dev, cfg_scale, x_out,
                          x_out2, n, st);
}

// ---- renoise (the inpainting sampler's up-move) -----------------------------------------------------------------------------------
int afd_renoise(const float* x, const float* noise, const float* alpha_hat, int t_from, int t_to, float* x_out, long n,
                afd_stream_t st) {
  AFD_REQUIRE(x && noise && alpha_hat && x_out, "afd_renoise: x, noise, alpha_hat and x_out must not be NULL");
  AFD_REQUIRE(n > 0, "afd_renoise: n must be positive (got %ld)", n);
  AFD_REQUIRE(t_from >= 0 && t_from < t_to, "afd_renoise: need 0 <= t_from < t_to (got t_from = %d, t_to = %d)", t_from, t_to);
  const bool vec = vec_ok(n, {x, noise, x_out});
  const long work = vec ? n / 4 : n;
  launch_vec(vec, renoise_k<true>, renoise_k<false>, step_grid(work), as_stream(st), x, noise, alpha_hat, t_from, t_to, x_out, work);
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
// ---- UniPC ---------------------------------------------------------------------------------------------------------------------
// xc (n values) and hist (3n) are read and written per element while x and eps are read and the outputs written by other
// elements: the two share no memory with each other, with x, with eps or with the outputs.
static inline bool unipc_apart(const float* x, const float* eps, long eps_n, const float* xc, const float* hist, const float* x_out,
                               const float* x_out2, long n) {
  const long fb = n * (long)sizeof(float);
  auto apart = [&](const float* q, long qb) {
    return !overlaps(q, qb, x, fb) && !overlaps(q, qb, eps, eps_n * (long)sizeof(float)) && !overlaps(q, qb, x_out, fb) &&
           !overlaps(q, qb, x_out2, fb);
  };
  if (!apart(xc, fb) || !apart(hist, 3 * fb)) return false;
  return !overlaps(xc, fb, hist, 3 * fb);
}
int afd_unipc_step(const float* x, const float* eps, float* xc, float* hist, const float* coef, float* x_out, long n, afd_stream_t st) {
  AFD_REQUIRE(x && eps && xc && hist && coef && x_out, "afd_unipc_step: x, eps, xc, hist, coef and x_out must not be NULL");
  AFD_REQUIRE(n > 0, "afd_unipc_step: n must be positive (got %ld)", n);
  AFD_REQUIRE(unipc_apart(x, eps, n, xc, hist, x_out, nullptr, n),
              "afd_unipc_step: xc and hist must not overlap each other, x, eps or x_out");
  launch_unipc_step<false>(x, eps, xc, hist, coef, 0.0f, x_out, nullptr, n, as_stream(st));
  return check_launch("afd_unipc_step");
}
int afd_unipc_step_cfg(const float* x, const float* eps2, float* xc, float* hist, const float* coef, float cfg_scale, float* x_out,
                       float* x_out2, long n, afd_stream_t st) {
  AFD_REQUIRE(x && eps2 && xc && hist && coef && x_out, "afd_unipc_step_cfg: x, eps2, xc, hist, coef and x_out must not be NULL");
  AFD_REQUIRE(n > 0, "afd_unipc_step_cfg: n must be positive (got %ld)", n);
  AFD_REQUIRE(unipc_apart(x, eps2, 2 * n, xc, hist, x_out, x_out2, n),
              "afd_unipc_step_cfg: xc and hist must not overlap each other, x, eps2, x_out or x_out2");
  launch_unipc_step<true>(x, eps2, xc, hist, coef, cfg_scale, x_out, x_out2, n, as_stream(st));
  return check_launch("afd_unipc_step_cfg");
}
int afd_quantize_u8(const float* x, uint8_t* out, long n, afd_stream_t st) {
  AFD_REQUIRE(x && out && n > 0, "afd_quantize_u8: bad argument");
  hipLaunchKernelGGL(quantize_u8_k, dim3(gs_grid(n)), dim3(256), 0, as_stream(st), x, out, n);
  return check_launch("afd_quantize_u8");
}

}  // extern "C"

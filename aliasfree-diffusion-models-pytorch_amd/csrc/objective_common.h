// objective_common.h -- the per-element device functions that objective.hip (the losses, the bound) and tsampler.hip (the
// per-row losses of the timestep sampler) share (internal): the objectives' pred - target, L_simple of a quad, the output ->
// eps conversion, Ho et al.'s discretised Gaussian and the learned-variance terms; and the entry points' shared checks.
//
// As in diffusion_common.h, every fp32 expression here promises one IEEE rounding per operation, so the including file puts
// `#pragma clang fp contract(off)` BEFORE it includes this header.
#pragma once
#include <cmath>
#include "diffusion_common.h"

namespace afd {

// ---- training objectives: eps / v / x0 prediction ------------------------------------------------------------------------------
// target: eps (AFD_PRED_EPS), sqrt(a) eps - sqrt(1 - a) x0 (AFD_PRED_V), x0 (AFD_PRED_X0); -> pred - target
__device__ __forceinline__ float objective_diff(int kind, float p, float x0, float e, float sa, float sb) {
  if (kind == AFD_PRED_V) {
    const float l = sa * e, r = sb * x0;
    return p - (l - r);
  }
  return p - (kind == AFD_PRED_X0 ? x0 : e);
}
__device__ __forceinline__ float4 objective_diff4(int kind, float4 p, float4 x0, float4 e, Roots k) {
  return quad_map([=](float pi, float xi, float ei) { return objective_diff(kind, pi, xi, ei, k.sa, k.sb); }, p, x0, e);
}
// L_simple of one quad, sum_i d_i^2 over its first `left` lanes, left to right (a value past the row's end may be anything,
// NaN included: it is never added), and its gradient g d
__device__ __forceinline__ float lsimple_sum(float4 d, long left) {
  float r = d.x * d.x;
  if (left > 1) r += d.y * d.y;
  if (left > 2) r += d.z * d.z;
  if (left > 3) r += d.w * d.w;
  return r;
}
__device__ __forceinline__ float4 lsimple_grad(float4 d, float g) {
  return quad_map([=](float di) { return di * g; }, d);
}
// the network's output -> eps, at x_t: eps: itself;  v: (sqrt(a) v) + (sqrt(1 - a) x_t);  x0: (x_t - sqrt(a) x0) / sqrt(1 - a)
__device__ __forceinline__ float eps_of_pred(int kind, float p, float xt, float sa, float sb) {
  if (kind == AFD_PRED_V) return noised(sa, sb, p, xt);
  if (kind == AFD_PRED_X0) {
    const float l = sa * p;
    return (xt - l) / sb;
  }
  return p;
}
__device__ __forceinline__ float4 eps_of_pred4(int kind, float4 p, float4 xt, Roots k) {
  return quad_map([=](float pi, float xi) { return eps_of_pred(kind, pi, xi, k.sa, k.sb); }, p, xt);
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
  Roots k;                 // of the fp32 alpha_hat[t]
  Ddpm dec;                // the DDPM rule at step 1
  bool is_dec;
};
__device__ __forceinline__ LvarRow lvar_row(const double* __restrict__ lv_coef, const float* __restrict__ alpha,
                                            const float* __restrict__ alpha_hat, const float* __restrict__ beta, long t, int kind) {
  LvarRow w;
  const float ah = alpha_hat[t];
  w.k = roots(ah);
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
    const float mean = w.dec.update(xt, eps_of_pred(kind, p, xt, w.k.sa, w.k.sb), 0.0f, false);
    return lvar_decoder<GRAD>((double)x0, (double)mean, (double)v, w.lb, w.lbt, dlv);
  }
  return lvar_kl<GRAD>(sq, (double)v, w.lb, w.lbt, w.kt, dlv);
}

}  // namespace afd

// ---- the checks the entry points share (their message texts are part of the interface) -------------------------------------------
static inline bool kind_ok(int kind) { return kind == AFD_PRED_EPS || kind == AFD_PRED_V || kind == AFD_PRED_X0; }
#define AFD_REQUIRE_KIND(name, kind) \
  AFD_REQUIRE(kind_ok(kind), "%s: kind must be AFD_PRED_EPS, AFD_PRED_V or AFD_PRED_X0 (got %d)", name, kind)
#define AFD_REQUIRE_B_CHW(name, B, chw) AFD_REQUIRE((B) > 0 && (chw) > 0, "%s: B and chw must be positive (got %ld, %ld)", name, B, chw)
#define AFD_REQUIRE_VLB_SCALE(name, s) \
  AFD_REQUIRE(std::isfinite(s) && (s) >= 0.0, "%s: vlb_scale must be finite and >= 0 (got %g)", name, s)

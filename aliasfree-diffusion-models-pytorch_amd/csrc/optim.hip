// optim.hip -- fused AdamW, the EMA of the weights, gradient-norm clipping and the learning-rate controller.
//
// fp32, one IEEE rounding per torch op (no FMA contraction, correctly rounded sqrt and divide), so AdamW matches torch's
// bit for bit; `#pragma clang fp contract(off)` below stops a*b+c from fusing.
#include "common.h"

#pragma clang fp contract(off)

namespace afd {

static inline int gs_grid(long total, int block = 256) {
  long g = (total + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > 32768 ? 32768 : g));
}

// ---- AdamW (torch.optim.AdamW semantics, decoupled weight decay) ---------------------------
// state = {step, 1 - b1^step, 1 - b2^step, unused}; double keeps the powers exact enough for 1e6 steps
__device__ __forceinline__ void adam_advance(float* state, float b1, float b2) {
  const double step = (double)state[0] + 1.0;
  state[0] = (float)step;
  state[1] = (float)(1.0 - pow((double)b1, step));
  state[2] = (float)(1.0 - pow((double)b2, step));
}
// the EMA's call counter: ema_state = {calls, copy}; copy = calls < start, then ++calls (the order of EMA.step_ema).
// Device-resident so that a replayed step crosses `start` where the eager one would.
__device__ __forceinline__ void ema_count(int* ema_state, int start) {
  const int calls = ema_state[0];
  ema_state[1] = calls < start ? 1 : 0;
  ema_state[0] = calls + 1;
}
__global__ void adamw_tick_k(float* state, float b1, float b2, int* ema_state, int start) {
  adam_advance(state, b1, b2);
  if (ema_state) ema_count(ema_state, start);
}
// one AdamW element: one rounding per operation, in the order written (m is a lerp, as torch does); adamw_k below is its only
// caller, and tests/test_gpu_optim.py restates it in numpy fp32 and compares the bits
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

// One workgroup: the partials in index order -> norm -> clip coefficient; unless the step is skipped, adamw_tick_k's two
// advances and the learning rate of this update.  The partials go through LDS so that thread 0's chain of fp64 adds does not
// wait on one global load each.
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
  adam_advance(state, b1, b2);
  if (ema_state) ema_count(ema_state, start);
  const double k = (double)state[0] - 1.0, factor = lr_factor(cfg, k);
  ctl[kCtlLr] = (double)(float)(cfg.base_lr * factor);
  ctl[kCtlCoef] = coef;
  ctl[kCtlSkip] = 0.0;
  ctl[kCtlIndex] = k;
  ctl[kCtlFactor] = factor;
}

// ---- the AdamW step, every form of it ---------------------------------------------------------------------------------------
// AdamW over [0, n_active).  CTL: lr and the clip coefficient come from ctl, and every thread returns before its first access
// when ctl says skip; otherwise lr and gscale are the arguments.  EMA: the EMA rule on the NEW p in the same pass, then the rule
// alone over [n_active, n_ema) (FlatParams' tail: parameters the optimiser never touches, which the reference's EMA still
// walks).  VEC: every pointer 16-byte aligned -> float4 accesses.  p, g, m, v (and ema) are streamed once.
template <bool VEC, bool EMA, bool CTL>
__global__ void adamw_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                        long n_active, const float* __restrict__ state, float lr, const double* __restrict__ ctl, float b1, float b2,
                        float eps, float wd, float gscale, float* __restrict__ ema, long n_ema, const int* __restrict__ ema_state,
                        float beta, float omb) {
  if (CTL) {
    if (ctl[kCtlSkip] != 0.0) return;
    lr = (float)ctl[kCtlLr];
    gscale = gscale * (float)ctl[kCtlCoef];
  }
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

static inline bool beta_ok(float beta, float omb) { return beta >= 0.0f && beta <= 1.0f && omb >= 0.0f && omb <= 1.0f; }

// The one launcher of adamw_k.  `who` is the entry point, for the messages; ctl and ema select the form (NULL: lr by value, no
// EMA), and the float4 instance runs when every pointer the kernel walks is 16-byte aligned.
static int launch_adamw(const char* who, float* p, const float* g, float* m, float* v, long n_active, const float* state, float lr,
                        const double* ctl, float b1, float b2, float eps, float wd, float gscale, float* ema, long n_ema,
                        const int* ema_state, float beta, float omb, afd_stream_t st) {
  AFD_REQUIRE(p && g && m && v && state, "%s: a pointer is NULL", who);
  AFD_REQUIRE(!ema || ema_state, "%s: ema is given but ema_state is NULL", who);
  AFD_REQUIRE(!ema || (n_active > 0 && n_ema > 0), "%s: n_active and n_ema must be positive (got %ld, %ld)", who, n_active, n_ema);
  AFD_REQUIRE(n_active > 0, "%s: n_active must be positive (got %ld)", who, n_active);
  AFD_REQUIRE(!ema || n_active <= n_ema, "%s: n_active > n_ema (%ld > %ld)", who, n_active, n_ema);
  AFD_REQUIRE(!ema || beta_ok(beta, omb), "%s: beta and 1 - beta must lie in [0, 1] (got %g, %g)", who, (double)beta, (double)omb);
  using kernel_t = decltype(&adamw_k<false, false, false>);
  static const kernel_t kernels[2][2][2] = {      // [VEC][EMA][CTL]
      {{adamw_k<false, false, false>, adamw_k<false, false, true>}, {adamw_k<false, true, false>, adamw_k<false, true, true>}},
      {{adamw_k<true, false, false>, adamw_k<true, false, true>}, {adamw_k<true, true, false>, adamw_k<true, true, true>}}};
  const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && (!ema || aligned16(ema));
  const long items = ema ? n_ema : n_active;
  hipLaunchKernelGGL(kernels[vec][ema != nullptr][ctl != nullptr], dim3(gs_grid(vec ? (items + 3) / 4 : items)), dim3(256), 0,
                     as_stream(st), p, g, m, v, n_active, state, lr, ctl, b1, b2, eps, wd, gscale, ema, n_ema, ema_state, beta, omb);
  return check_launch(who);
}

extern "C" {

int afd_adamw_tick(float* state, float b1, float b2, afd_stream_t st) {
  AFD_REQUIRE(state, "afd_adamw_tick: state is NULL");
  hipLaunchKernelGGL(adamw_tick_k, dim3(1), dim3(1), 0, as_stream(st), state, b1, b2, (int*)nullptr, 0);
  return check_launch("afd_adamw_tick");
}
int afd_adamw_step(float* p, const float* g, float* m, float* v, long n, const float* state,
                   float lr, float b1, float b2, float eps, float wd, float gscale, afd_stream_t st) {
  return launch_adamw("afd_adamw_step", p, g, m, v, n, state, lr, nullptr, b1, b2, eps, wd, gscale, nullptr, 0, nullptr, 0.0f, 0.0f, st);
}

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
  hipLaunchKernelGGL(adamw_tick_k, dim3(1), dim3(1), 0, as_stream(st), adam_state, b1, b2, ema_state, start);
  return check_launch("afd_adamw_ema_tick");
}
int afd_adamw_ema_step(float* p, const float* g, float* m, float* v, long n_active, const float* adam_state, float lr, float b1,
                       float b2, float eps, float wd, float gscale, float* ema, long n_ema, const int* ema_state, float beta,
                       float one_minus_beta, afd_stream_t st) {
  AFD_REQUIRE(ema && ema_state, "afd_adamw_ema_step: a pointer is NULL");
  return launch_adamw("afd_adamw_ema_step", p, g, m, v, n_active, adam_state, lr, nullptr, b1, b2, eps, wd, gscale, ema, n_ema,
                      ema_state, beta, one_minus_beta, st);
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
  AFD_REQUIRE(ctl, "afd_adamw_ctl_step: a pointer is NULL");
  AFD_REQUIRE(!ema || n_ema <= 0 || n_active <= n_ema, "afd_adamw_ctl_step: 0 < n_active <= n_ema is required (got %ld, %ld)", n_active,
              n_ema);                              // (this entry point's wording of the launcher's range check)
  return launch_adamw("afd_adamw_ctl_step", p, g, m, v, n_active, adam_state, 0.0f, ctl, b1, b2, eps, wd, grad_scale, ema, n_ema,
                      ema_state, beta, one_minus_beta, st);
}

}  // extern "C"

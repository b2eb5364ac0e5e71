// objective.hip -- what is computed FROM the network's output: MSE, the training objectives (eps / v / x0 prediction) and
// pred_to_eps, the learned reverse-process variances (hybrid loss, split, ancestral step, bound) and the likelihood bound's
// kernels.  (The samplers' own steps are sampler.hip, the optimizer is optim.hip.)
//
// As in sampler.hip, every fp32 expression restates the reference's operation ORDER with one IEEE rounding per torch op (no FMA
// contraction, correctly rounded sqrt and divide): the loss kernels promise the bits of a plain fp32 evaluation, L_simple of the
// hybrid loss promises the objective loss's bits, and the converted eps feeds the bit-exact sampler steps.  hipcc keeps `/` and
// sqrtf correctly rounded by default; `#pragma clang fp contract(off)` below stops a*b+c from fusing.  Without it this file
// still compiles and every result changes in its last bits.
#include "common.h"

#pragma clang fp contract(off)

#include "objective_common.h"

namespace afd {

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
// The kernels below walk (row, quad) items (for_row_quads), so sqrt(a), sqrt(1 - a) and w[t_b] are read once per item and are
// uniform over the workgroup.  VEC (chw % 4 == 0, 16-byte aligned pointers): one 128-bit access per stream; otherwise the
// same quad element by element -- every thread sees the same values in the same order in both forms, so their results are
// bit-identical.  Streaming, 12-16 bytes per element: at B = 256, chw = 3072 this is 768 items, three workgroups per CU.
constexpr int kObjBlocks = 1024;      // cap on the partial sums (the workspace holds 4096 floats, as for mse)

// (objective_diff, lsimple_sum / lsimple_grad and eps_of_pred are objective_common.h's)

// part[blockIdx.x] = sum over the workgroup's items of w[t_b] * sum_i (pred - target)^2: per thread in item order, then the
// workgroup's fixed tree (block_sum); mse_final_k sums the partials.  x0 (eps) is not read for AFD_PRED_EPS (AFD_PRED_X0).
template <bool VEC>
__global__ __launch_bounds__(256) void objective_partial_k(const float* __restrict__ pred, const float* __restrict__ x0,
                                                           const float* __restrict__ eps, const int64_t* __restrict__ t,
                                                           const float* __restrict__ alpha_hat, const float* __restrict__ w, int kind,
                                                           float* __restrict__ part, long items, long segs, long chw) {
  __shared__ float red[16];
  float s = 0.f;
  for_row_quads(items, segs, chw, [&](const RowQuad& rq) {
    const long tb = t[rq.b];
    const Roots k = roots(alpha_hat[tb]);
    const float wb = w ? w[tb] : 1.0f;
    if (rq.left <= 0) return;
    const float4 p = load_quad<VEC>(pred, rq.o, rq.left);
    const float4 x = kind != AFD_PRED_EPS ? load_quad<VEC>(x0, rq.o, rq.left) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 e = kind != AFD_PRED_X0 ? load_quad<VEC>(eps, rq.o, rq.left) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float r = lsimple_sum(objective_diff4(kind, p, x, e, k), rq.left);
    s += wb * r;
  });
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
  const float g0 = dloss[0] * two_over_n;
  for_row_quads(items, segs, chw, [&](const RowQuad& rq) {
    const long tb = t[rq.b];
    const Roots k = roots(alpha_hat[tb]);
    const float g = w ? g0 * w[tb] : g0;
    if (rq.left <= 0) return;
    const float4 p = load_quad<VEC>(pred, rq.o, rq.left);
    const float4 x = kind != AFD_PRED_EPS ? load_quad<VEC>(x0, rq.o, rq.left) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 e = kind != AFD_PRED_X0 ? load_quad<VEC>(eps, rq.o, rq.left) : make_float4(0.f, 0.f, 0.f, 0.f);
    store_quad<VEC>(dpred, rq.o, rq.left, lsimple_grad(objective_diff4(kind, p, x, e, k), g));
  });
}

// the network's output -> eps (eps_of_pred), per row t.  eps_out may be `out` itself (elementwise: every thread reads its quad
// before it writes it), hence no __restrict__ on them.
template <bool VEC>
__global__ __launch_bounds__(256) void pred_to_eps_k(const float* out, const float* __restrict__ xt, const int64_t* __restrict__ t,
                                                     const float* __restrict__ alpha_hat, int kind, float* eps_out, long items,
                                                     long segs, long chw) {
  for_row_quads(items, segs, chw, [&](const RowQuad& rq) {
    const Roots k = roots(alpha_hat[t[rq.b]]);
    if (rq.left <= 0) return;
    const float4 v = load_quad<VEC>(out, rq.o, rq.left), x = load_quad<VEC>(xt, rq.o, rq.left);
    store_quad<VEC>(eps_out, rq.o, rq.left, eps_of_pred4(kind, v, x, k));
  });
}

// ---- likelihood (bits/dim, Ho et al. 2020 section 3.3): gathered noising, the bound's per-row terms, the prior ------------
// A row r pairs image img[r] of x0 with timestep t[r].  The three kernels below walk rows with whole workgroups (a row's
// coefficients are wave-uniform) and the row's `per` values with the threads; VEC: per % 4 == 0 and the float pointers
// 16-byte aligned, so every row starts on a 16-byte boundary; `per` then counts float4s.  (Not the quad walk: the per-thread
// summation sets of the two forms differ, and the fp64 sums with them.)

// x_t[r] = noised(x0[img[r]], eps[r]) at t[r]
template <bool VEC>
__global__ __launch_bounds__(256) void noise_images_gather_k(const float* __restrict__ x0, const int64_t* __restrict__ img,
                                                             const float* __restrict__ eps, const int64_t* __restrict__ t,
                                                             const float* __restrict__ alpha_hat, float* __restrict__ xt, long rows,
                                                             long per) {
  for (long r = blockIdx.x; r < rows; r += gridDim.x) {
    const Roots k = roots(alpha_hat[t[r]]);
    const long src = img[r] * per, dst = r * per;
    for (long j = threadIdx.x; j < per; j += blockDim.x) {
      if (VEC) {
        const float4 x = reinterpret_cast<const float4*>(x0)[src + j], e = reinterpret_cast<const float4*>(eps)[dst + j];
        reinterpret_cast<float4*>(xt)[dst + j] = quad_map([=](float xi, float ei) { return noised(k.sa, k.sb, xi, ei); }, x, e);
      } else {
        xt[dst + j] = noised(k.sa, k.sb, x0[src + j], eps[dst + j]);
      }
    }
  }
}

// (Ho et al.'s discretised Gaussian, decoder_log_prob, is objective_common.h's)

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
#pragma unroll
      for (int q = 0; q < 4; ++q) s += (double)lane(v, q) * (double)lane(v, q);
    } else {
      const double v = x0[row + j];
      s += v * v;
    }
  }
  block_sum2_f64(s, unused, red);
  if (threadIdx.x == 0) out[blockIdx.x] = half_ah * s;
}

// ---- learned reverse-process variances (Nichol & Dhariwal 2021): hybrid loss, ancestral step, bound ---------------------------
// (the per-element device functions -- lvar_logvar ... lvar_term, LvarRow -- are objective_common.h's)

// Walk as objective_partial_k.  part_s[blockIdx.x]: objective_partial_k's sum over the p half (L_simple, bit for bit);
// part_v[blockIdx.x]: the fp64 sum of the bound's terms, per thread in item and element order, then the workgroup's fixed tree.
// vw (may be NULL): a second per-timestep table, vw[t_b] multiplies each of row b's terms (the timestep sampler's importance
// weight); with NULL the terms are added as they are, so the sum keeps its bits.
template <bool VEC>
__global__ __launch_bounds__(256) void lvar_partial_k(const float* __restrict__ out2, const float* __restrict__ x0,
                                                      const float* __restrict__ eps, const int64_t* __restrict__ t,
                                                      const float* __restrict__ alpha, const float* __restrict__ alpha_hat,
                                                      const float* __restrict__ beta, const double* __restrict__ lv_coef,
                                                      const float* __restrict__ w, const float* __restrict__ vw, int kind,
                                                      float* __restrict__ part_s, double* __restrict__ part_v, long items,
                                                      long segs, long chw) {
  __shared__ float red[16];
  __shared__ double red2[8];
  float s = 0.f;
  double sv = 0.0, unused = 0.0;
  for_row_quads(items, segs, chw, [&](const RowQuad& rq) {
    const long tb = t[rq.b];
    const LvarRow row = lvar_row(lv_coef, alpha, alpha_hat, beta, tb, kind);
    const float wb = w ? w[tb] : 1.0f;
    const double vwb = vw ? (double)vw[tb] : 1.0;
    if (rq.left <= 0) return;
    const float4 p = load_quad<VEC>(out2, rq.o2, rq.left), v = load_quad<VEC>(out2, rq.o2 + chw, rq.left);
    const float4 x = load_quad<VEC>(x0, rq.o, rq.left), e = load_quad<VEC>(eps, rq.o, rq.left);
    const float r = lsimple_sum(objective_diff4(kind, p, x, e, row.k), rq.left);
    s += wb * r;
    const float pv[4] = {p.x, p.y, p.z, p.w}, vv[4] = {v.x, v.y, v.z, v.w}, xv[4] = {x.x, x.y, x.z, x.w}, ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < rq.left) {
        double sq, dlv;
        const double term = lvar_term<false>(row, kind, pv[i], vv[i], xv[i], ev[i], noised(row.k.sa, row.k.sb, xv[i], ev[i]), sq, dlv);
        sv += vw ? vwb * term : term;
      }
    }
  });
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
// (float)(dloss gv (d term / d logvar) (lb - lbt) / 2), gv = vlb_scale / (N ln 2), in fp64 and rounded once; vw (may be NULL):
// vw[t_b] multiplies row b's v half, as in the forward
template <bool VEC>
__global__ __launch_bounds__(256) void lvar_bwd_k(const float* __restrict__ out2, const float* __restrict__ x0,
                                                  const float* __restrict__ eps, const int64_t* __restrict__ t,
                                                  const float* __restrict__ alpha, const float* __restrict__ alpha_hat,
                                                  const float* __restrict__ beta, const double* __restrict__ lv_coef,
                                                  const float* __restrict__ w, const float* __restrict__ vw, int kind,
                                                  const float* __restrict__ dloss, float* __restrict__ dout2, long items, long segs,
                                                  long chw, float two_over_n, double gv) {
  const float g0 = dloss[0] * two_over_n;
  const double gd = (double)dloss[0] * gv;
  for_row_quads(items, segs, chw, [&](const RowQuad& rq) {
    const long tb = t[rq.b];
    const LvarRow row = lvar_row(lv_coef, alpha, alpha_hat, beta, tb, kind);
    const float g = w ? g0 * w[tb] : g0;
    const double gl0 = gd * ((row.lb - row.lbt) / 2.0);
    const double gl = vw ? gl0 * (double)vw[tb] : gl0;
    if (rq.left <= 0) return;
    const float4 p = load_quad<VEC>(out2, rq.o2, rq.left), v = load_quad<VEC>(out2, rq.o2 + chw, rq.left);
    const float4 x = load_quad<VEC>(x0, rq.o, rq.left), e = load_quad<VEC>(eps, rq.o, rq.left);
    store_quad<VEC>(dout2, rq.o2, rq.left, lsimple_grad(objective_diff4(kind, p, x, e, row.k), g));
    const float pv[4] = {p.x, p.y, p.z, p.w}, vv[4] = {v.x, v.y, v.z, v.w}, xv[4] = {x.x, x.y, x.z, x.w}, ev[4] = {e.x, e.y, e.z, e.w};
    float dv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < rq.left) {
        double sq, dlv;
        lvar_term<true>(row, kind, pv[i], vv[i], xv[i], ev[i], noised(row.k.sa, row.k.sb, xv[i], ev[i]), sq, dlv);
        dv[i] = (float)(gl * dlv);
      }
    }
    store_quad<VEC>(dout2, rq.o2 + chw, rq.left, make_float4(dv[0], dv[1], dv[2], dv[3]));
  });
}

// out2 (B rows of 2 chw) -> eps_out (B x chw; pred_to_eps_k's conversion, a copy for AFD_PRED_EPS) and, optionally, the v half
template <bool VEC>
__global__ __launch_bounds__(256) void split_pred_k(const float* __restrict__ out2, const float* __restrict__ xt,
                                                    const int64_t* __restrict__ t, const float* __restrict__ alpha_hat, int kind,
                                                    float* __restrict__ eps_out, float* __restrict__ v_out, long items, long segs,
                                                    long chw) {
  for_row_quads(items, segs, chw, [&](const RowQuad& rq) {
    const Roots k = roots(kind != AFD_PRED_EPS ? alpha_hat[t[rq.b]] : 0.0f);
    if (rq.left <= 0) return;
    float4 r = load_quad<VEC>(out2, rq.o2, rq.left);
    if (kind != AFD_PRED_EPS) r = eps_of_pred4(kind, r, load_quad<VEC>(xt, rq.o, rq.left), k);
    store_quad<VEC>(eps_out, rq.o, rq.left, r);
    if (v_out) store_quad<VEC>(v_out, rq.o, rq.left, load_quad<VEC>(out2, rq.o2 + chw, rq.left));
  });
}

// Ancestral step with the learned variance: eps_hat from p (eps_of_pred at x, per step), guided (kCfg: out2 holds 2 B rows,
// conditional then unconditional; cfg_lerp of the two eps; the variance from the conditional row), then
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
  const Roots rt = roots(alpha_hat[step]);
  const double lb = lv_coef[3 * (long)step], lbt = lv_coef[3 * (long)step + 1];
  const bool has_noise = noise != nullptr && step > 1;
  for_row_quads(items, segs, chw, [&](const RowQuad& rq) {
    if (rq.left <= 0) return;
    const float4 xv = load_quad<VEC>(x, rq.o, rq.left), c = load_quad<VEC>(out2, rq.o2, rq.left);
    const float4 v = load_quad<VEC>(out2, rq.o2 + chw, rq.left);
    const float4 u = kCfg ? load_quad<VEC>(out2, rq.o2 + 2 * B * chw, rq.left) : c;
    const float4 z = has_noise ? load_quad<VEC>(noise, rq.o, rq.left) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 r = quad_map(
        [&](float xi, float ci, float ui, float vi, float zi) {
          const float e = guided_eps<kCfg>(g, eps_of_pred(kind, ci, xi, rt.sa, rt.sb), eps_of_pred(kind, ui, xi, rt.sa, rt.sb));
          return lvar_update(k, xi, e, vi, zi, lb, lbt, has_noise);
        },
        xv, c, u, v, z);
    store_quad<VEC>(x_out, rq.o, rq.left, r);
    if (x_out2) store_quad<VEC>(x_out2, rq.o, rq.left, r);
  });
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
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < left) {
        double d2, dlv;
        s_t += lvar_term<false>(row, kind, lane(p, i), lane(v, i), lane(x, i), lane(e, i), lane(n, i), d2, dlv);
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

// ---- progressive distillation (Salimans & Ho 2022): two DDIM steps of a teacher, per row, folded into one student target ------
// Row b goes t -> t_mid -> t_prev (eta = 0).  With a = alpha_hat[.], al = sqrt(a), sg = sqrt(1 - a); the chain's last level
// t_prev = 0 is alpha_hat[0], as the DDIM rule of sampler.hip reads it (Ddim::make), so the target matches the sampler's last step:
//   (x_hat, eps_hat) of a raw output p at z:  eps: (z - sg p) / al, p;   v: al z - sg p, sg z + al p;   x0: p, (z - al p) / sg
//   z_mid   = al' x_hat_1 + sg' eps_hat_1                               (distill_mid_k;    out1 is the output at (z_t, t))
//   z_prev  = al'' x_hat_2 + sg'' eps_hat_2                             (distill_target_k; out2 is the output at (z_mid, t_mid))
//   x_tilde = (z_prev - r z_t) / (al'' - r al),  r = sg'' / sg
//   eps_tilde = (z_t - al x_tilde) / sg
// so that one DDIM step from z_t with (x_tilde, eps_tilde) lands on z_prev.  The denominator is sin(phi - phi'') / sg with
// al = cos(phi), a few 1e-3 between neighbouring levels, and the numerator cancels to the same order: every element is widened
// to fp64, the roots are taken in fp64 from the fp32 table, and the result is rounded once on the store (as the lvar kernels).
// An output may be one of the inputs (each thread reads its quad of every input before it writes), hence no __restrict__.
struct Level64 {
  double al, sg;
};
__device__ __forceinline__ Level64 level64(const float* __restrict__ alpha_hat, long t) {
  const double a = (double)alpha_hat[t];
  return Level64{sqrt(a), sqrt(1.0 - a)};
}
__device__ __forceinline__ void distill_split(int kind, double p, double z, const Level64& k, double& x, double& e) {
  if (kind == AFD_PRED_V) {
    x = k.al * z - k.sg * p;
    e = k.sg * z + k.al * p;
  } else if (kind == AFD_PRED_X0) {
    x = p;
    e = (z - k.al * p) / k.sg;
  } else {
    e = p;
    x = (z - k.sg * p) / k.al;
  }
}
// the DDIM step (eta = 0) of the raw output p at z, level k -> level n, in fp64
__device__ __forceinline__ double distill_ddim(int kind, float p, float z, const Level64& k, const Level64& n) {
  double x, e;
  distill_split(kind, (double)p, (double)z, k, x, e);
  return n.al * x + n.sg * e;
}
template <bool VEC>
__global__ __launch_bounds__(256) void distill_mid_k(const float* out1, const float* z_t, const int64_t* __restrict__ t,
                                                     const int64_t* __restrict__ t_mid, const float* __restrict__ alpha_hat, int kind,
                                                     float* z_mid, long items, long segs, long chw) {
  for_row_quads(items, segs, chw, [&](const RowQuad& rq) {
    const Level64 k = level64(alpha_hat, t[rq.b]), n = level64(alpha_hat, t_mid[rq.b]);
    if (rq.left <= 0) return;
    const float4 p = load_quad<VEC>(out1, rq.o, rq.left), z = load_quad<VEC>(z_t, rq.o, rq.left);
    store_quad<VEC>(z_mid, rq.o, rq.left, quad_map([&](float pi, float zi) { return (float)distill_ddim(kind, pi, zi, k, n); }, p, z));
  });
}
template <bool VEC>
__global__ __launch_bounds__(256) void distill_target_k(const float* out2, const float* z_mid, const float* z_t,
                                                        const int64_t* __restrict__ t, const int64_t* __restrict__ t_mid,
                                                        const int64_t* __restrict__ t_prev, const float* __restrict__ alpha_hat,
                                                        int kind, float* x_tilde, float* eps_tilde, long items, long segs, long chw) {
  for_row_quads(items, segs, chw, [&](const RowQuad& rq) {
    const Level64 k = level64(alpha_hat, t[rq.b]), m = level64(alpha_hat, t_mid[rq.b]), n = level64(alpha_hat, t_prev[rq.b]);
    const double r = n.sg / k.sg;
    const double den = n.al - r * k.al;
    if (rq.left <= 0) return;
    const float4 p = load_quad<VEC>(out2, rq.o, rq.left), zm = load_quad<VEC>(z_mid, rq.o, rq.left);
    const float4 z = load_quad<VEC>(z_t, rq.o, rq.left);
    float xs[4], es[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double zi = (double)lane(z, i);
      const double zp = distill_ddim(kind, lane(p, i), lane(zm, i), m, n);
      const double x = (zp - r * zi) / den;
      xs[i] = (float)x;
      es[i] = (float)((zi - k.al * x) / k.sg);
    }
    store_quad<VEC>(x_tilde, rq.o, rq.left, make_float4(xs[0], xs[1], xs[2], xs[3]));
    store_quad<VEC>(eps_tilde, rq.o, rq.left, make_float4(es[0], es[1], es[2], es[3]));
  });
}

// ---- consistency distillation (Song et al. 2023; Luo et al. 2023): the consistency function, its target and the sampler's step ----
// coef: the (T, 2) fp64 table [c_skip, c_out] of Diffusion.consistency_coefficients, row 0 exactly (1, 0).  With x_hat the split
// above (distill_split) of a raw output p at z on level t:
//   f(z, t)   = c_skip[t] z + c_out[t] x_hat(p, z; t)                   (consistency_fn_k, consistency_step_k)
//   f_tgt     = f(z_prev, t_prev) of the target network's output         (consistency_target_k)
//   x_tilde   = (f_tgt - c_skip[t] z_t) / c_out[t]
//   eps_tilde = (z_t - al x_tilde) / sg
// so that a student predicting x_tilde at (z_t, t) has f(z_t, t) = f_tgt.  Where c_out == 0 (t = 0, the boundary) f IS z: p is
// not used there, whatever it holds (a product 0 * NaN would poison the row).  fp64 per element as above, one rounding on the store.
struct Consist64 {
  double cs, co;
};
__device__ __forceinline__ Consist64 consist64(const double* __restrict__ coef, long t) { return Consist64{coef[2 * t], coef[2 * t + 1]}; }
// f in fp64 (c.co != 0)
__device__ __forceinline__ double consistency_f64(int kind, float p, float z, const Level64& k, const Consist64& c) {
  double x, e;
  distill_split(kind, (double)p, (double)z, k, x, e);
  return c.cs * (double)z + c.co * x;
}
// f rounded once; z's own bits at the boundary
__device__ __forceinline__ float consistency_f(int kind, float p, float z, const Level64& k, const Consist64& c) {
  return c.co == 0.0 ? z : (float)consistency_f64(kind, p, z, k, c);
}
template <bool VEC>
__global__ __launch_bounds__(256) void consistency_fn_k(const float* out, const float* z_in, const int64_t* __restrict__ t,
                                                        const float* __restrict__ alpha_hat, const double* __restrict__ coef, int kind,
                                                        float* f_out, long items, long segs, long chw) {
  for_row_quads(items, segs, chw, [&](const RowQuad& rq) {
    const long tb = t[rq.b];
    const Level64 k = level64(alpha_hat, tb);
    const Consist64 c = consist64(coef, tb);
    if (rq.left <= 0) return;
    const float4 p = load_quad<VEC>(out, rq.o, rq.left), z = load_quad<VEC>(z_in, rq.o, rq.left);
    store_quad<VEC>(f_out, rq.o, rq.left, quad_map([&](float pi, float zi) { return consistency_f(kind, pi, zi, k, c); }, p, z));
  });
}
template <bool VEC>
__global__ __launch_bounds__(256) void consistency_target_k(const float* out_tgt, const float* z_prev, const float* z_t,
                                                            const int64_t* __restrict__ t, const int64_t* __restrict__ t_prev,
                                                            const float* __restrict__ alpha_hat, const double* __restrict__ coef,
                                                            int kind, float* x_tilde, float* eps_tilde, long items, long segs,
                                                            long chw) {
  for_row_quads(items, segs, chw, [&](const RowQuad& rq) {
    const long tb = t[rq.b], tp = t_prev[rq.b];
    const Level64 k = level64(alpha_hat, tb), n = level64(alpha_hat, tp);
    const Consist64 c = consist64(coef, tb), cn = consist64(coef, tp);
    if (rq.left <= 0) return;
    const float4 p = load_quad<VEC>(out_tgt, rq.o, rq.left), zp = load_quad<VEC>(z_prev, rq.o, rq.left);
    const float4 z = load_quad<VEC>(z_t, rq.o, rq.left);
    float xs[4], es[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double zi = (double)lane(z, i);
      const double f = cn.co == 0.0 ? (double)lane(zp, i) : consistency_f64(kind, lane(p, i), lane(zp, i), n, cn);
      const double x = (f - c.cs * zi) / c.co;
      xs[i] = (float)x;
      es[i] = (float)((zi - k.al * x) / k.sg);
    }
    store_quad<VEC>(x_tilde, rq.o, rq.left, make_float4(xs[0], xs[1], xs[2], xs[3]));
    store_quad<VEC>(eps_tilde, rq.o, rq.left, make_float4(es[0], es[1], es[2], es[3]));
  });
}
// the sampler's move at one level for every row: f rounded to fp32, then afd_noise_images' fp32 expression towards t_next
// (`noised`), or f itself at t_next == 0.  t / t_next come from the host or, DEV, from element 0 of t_dev / t_next_dev.
template <bool VEC>
__global__ __launch_bounds__(256) void consistency_step_k(const float* out, const float* z_in, const float* noise,
                                                          const float* __restrict__ alpha_hat, const double* __restrict__ coef, int kind,
                                                          int t_host, int t_next_host, const int64_t* __restrict__ t_dev,
                                                          const int64_t* __restrict__ t_next_dev, float* x_out, long items, long segs,
                                                          long chw) {
  const long t = t_dev ? (long)t_dev[0] : t_host, tn = t_next_dev ? (long)t_next_dev[0] : t_next_host;
  const Level64 k = level64(alpha_hat, t);
  const Consist64 c = consist64(coef, t);
  const Roots r = roots(alpha_hat[tn]);
  const bool renoise = tn > 0, has_noise = noise != nullptr;
  for_row_quads(items, segs, chw, [&](const RowQuad& rq) {
    if (rq.left <= 0) return;
    const float4 p = load_quad<VEC>(out, rq.o, rq.left), z = load_quad<VEC>(z_in, rq.o, rq.left);
    const float4 nz = renoise && has_noise ? load_quad<VEC>(noise, rq.o, rq.left) : make_float4(0.f, 0.f, 0.f, 0.f);
    store_quad<VEC>(x_out, rq.o, rq.left, quad_map([&](float pi, float zi, float ni) {
                      const float f = consistency_f(kind, pi, zi, k, c);
                      return renoise ? noised(r.sa, r.sb, f, ni) : f;
                    }, p, z, nz));
  });
}

}  // namespace afd
using namespace afd;

// (the checks the entry points share -- kind_ok, AFD_REQUIRE_KIND, ... -- are objective_common.h's)

// whether the outputs share no memory with each other or with any of the inputs (NULL entries are skipped)
struct Span {
  const void* p;
  long bytes;
};
static bool all_apart(std::initializer_list<Span> outs, std::initializer_list<Span> ins) {
  for (const Span* a = outs.begin(); a != outs.end(); ++a) {
    if (!a->p) continue;
    for (const Span* b = a + 1; b != outs.end(); ++b)
      if (overlaps(a->p, a->bytes, b->p, b->bytes)) return false;
    for (const Span& b : ins)
      if (overlaps(a->p, a->bytes, b.p, b.bytes)) return false;
  }
  return true;
}
constexpr long kF = sizeof(float), kD = sizeof(double), kI = sizeof(int64_t);

// the four learned-variance step entry points.  x_out may be x itself, and must otherwise share no memory with x; x_out and x_out2 share none with each other or any other input
template <bool kCfg>
static int launch_lvar_step(const char* name, const float* x, const float* out2, const float* noise, const float* alpha,
                            const float* alpha_hat, const float* beta, const double* lv_coef, int kind, int i, const int64_t* t_dev,
                            bool dev, float s, float* x_out, float* x_out2, long B, long chw, hipStream_t st) {
  AFD_REQUIRE(x && out2 && alpha && alpha_hat && beta && lv_coef && x_out && (!dev || t_dev),
              "%s: x, out2, alpha, alpha_hat, beta, lv_coef%s and x_out must not be NULL", name, dev ? ", t_dev" : "");
  AFD_REQUIRE_KIND(name, kind);
  AFD_REQUIRE_B_CHW(name, B, chw);
  AFD_REQUIRE(dev || i >= 1, "%s: need i >= 1 (the step i -> i - 1; got i = %d)", name, i);
  const long fb = B * chw * kF;
  AFD_REQUIRE(all_apart({{x_out, fb}, {x_out2, fb}}, {{out2, (kCfg ? 4 : 2) * fb}, {noise, fb}, {t_dev, kI}, {x_out == x ? nullptr : x, fb}}) &&
                  !(x_out2 && overlaps(x_out2, fb, x, fb)),
              "%s: x_out must be x itself or apart from it, and x_out / x_out2 must not overlap each other, out2, noise or t_dev", name);
  const RowQuadGrid g(B, chw, kObjBlocks);
  launch_vec(vec_ok(chw, {x, out2, noise, x_out, x_out2}), lvar_step_k<kCfg, true>, lvar_step_k<kCfg, false>, g.grid, st, x, out2, noise,
             alpha, alpha_hat, beta, lv_coef, kind, i, t_dev, s, x_out, x_out2, g.items, g.segs, chw, B);
  return check_launch(name);
}

extern "C" {

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

// ---- training objectives --------------------------------------------------------------------------------------------------
int afd_objective_loss_fwd(const float* pred, const float* x0, const float* eps, const int64_t* t, const float* alpha_hat,
                           const float* w, int kind, float* loss_out, float* workspace, long B, long chw, afd_stream_t st) {
  AFD_REQUIRE(pred && x0 && eps && t && alpha_hat && loss_out && workspace,
              "afd_objective_loss_fwd: pred, x0, eps, t, alpha_hat, loss_out and workspace must not be NULL");
  AFD_REQUIRE_KIND("afd_objective_loss_fwd", kind);
  AFD_REQUIRE_B_CHW("afd_objective_loss_fwd", B, chw);
  const RowQuadGrid g(B, chw, kObjBlocks);
  launch_vec(vec_ok(chw, {pred, x0, eps}), objective_partial_k<true>, objective_partial_k<false>, g.grid, as_stream(st), pred, x0, eps,
             t, alpha_hat, w, kind, workspace, g.items, g.segs, chw);
  hipLaunchKernelGGL(mse_final_k, dim3(1), dim3(256), 0, as_stream(st), workspace, loss_out, g.grid, 1.0f / (float)(B * chw));
  return check_launch("afd_objective_loss_fwd");
}
int afd_objective_loss_bwd(const float* pred, const float* x0, const float* eps, const int64_t* t, const float* alpha_hat,
                           const float* w, int kind, const float* dloss, float* dpred, long B, long chw, afd_stream_t st) {
  AFD_REQUIRE(pred && x0 && eps && t && alpha_hat && dloss && dpred,
              "afd_objective_loss_bwd: pred, x0, eps, t, alpha_hat, dloss and dpred must not be NULL");
  AFD_REQUIRE_KIND("afd_objective_loss_bwd", kind);
  AFD_REQUIRE_B_CHW("afd_objective_loss_bwd", B, chw);
  const RowQuadGrid g(B, chw, kObjBlocks);
  launch_vec(vec_ok(chw, {pred, x0, eps, dpred}), objective_bwd_k<true>, objective_bwd_k<false>, g.grid, as_stream(st), pred, x0, eps, t,
             alpha_hat, w, kind, dloss, dpred, g.items, g.segs, chw, 2.0f / (float)(B * chw));
  return check_launch("afd_objective_loss_bwd");
}
int afd_pred_to_eps(const float* out, const float* x_t, const int64_t* t, const float* alpha_hat, int kind, float* eps_out, long B,
                    long chw, afd_stream_t st) {
  AFD_REQUIRE(out && x_t && t && alpha_hat && eps_out, "afd_pred_to_eps: out, x_t, t, alpha_hat and eps_out must not be NULL");
  AFD_REQUIRE(kind == AFD_PRED_V || kind == AFD_PRED_X0,
              "afd_pred_to_eps: kind must be AFD_PRED_V or AFD_PRED_X0 (got %d; an eps output needs no conversion)", kind);
  AFD_REQUIRE_B_CHW("afd_pred_to_eps", B, chw);
  const RowQuadGrid g(B, chw, kObjBlocks);
  launch_vec(vec_ok(chw, {out, x_t, eps_out}), pred_to_eps_k<true>, pred_to_eps_k<false>, g.grid, as_stream(st), out, x_t, t, alpha_hat,
             kind, eps_out, g.items, g.segs, chw);
  return check_launch("afd_pred_to_eps");
}

// ---- progressive distillation -----------------------------------------------------------------------------------------------
// an output may be one of the B x chw inputs itself (the same pointer); otherwise it shares no memory with it
static bool same_or_apart(const float* out, long fb, std::initializer_list<const float*> ins) {
  for (const float* in : ins)
    if (out != in && overlaps(out, fb, in, fb)) return false;
  return true;
}
int afd_distill_mid(const float* out1, const float* z_t, const int64_t* t, const int64_t* t_mid, const float* alpha_hat, int kind,
                    float* z_mid, long B, long chw, afd_stream_t st) {
  AFD_REQUIRE(out1 && z_t && t && t_mid && alpha_hat && z_mid,
              "afd_distill_mid: out1, z_t, t, t_mid, alpha_hat and z_mid must not be NULL");
  AFD_REQUIRE_KIND("afd_distill_mid", kind);
  AFD_REQUIRE_B_CHW("afd_distill_mid", B, chw);
  const long fb = B * chw * kF, ib = B * kI;
  AFD_REQUIRE(same_or_apart(z_mid, fb, {out1, z_t}) && all_apart({{z_mid, fb}}, {{t, ib}, {t_mid, ib}}),
              "afd_distill_mid: z_mid must be out1 or z_t itself or apart from them, and must not overlap t or t_mid");
  const RowQuadGrid g(B, chw, kObjBlocks);
  launch_vec(vec_ok(chw, {out1, z_t, z_mid}), distill_mid_k<true>, distill_mid_k<false>, g.grid, as_stream(st), out1, z_t, t, t_mid,
             alpha_hat, kind, z_mid, g.items, g.segs, chw);
  return check_launch("afd_distill_mid");
}
int afd_distill_target(const float* out2, const float* z_mid, const float* z_t, const int64_t* t, const int64_t* t_mid,
                       const int64_t* t_prev, const float* alpha_hat, int kind, float* x_tilde, float* eps_tilde, long B, long chw,
                       afd_stream_t st) {
  AFD_REQUIRE(out2 && z_mid && z_t && t && t_mid && t_prev && alpha_hat && x_tilde && eps_tilde,
              "afd_distill_target: out2, z_mid, z_t, t, t_mid, t_prev, alpha_hat, x_tilde and eps_tilde must not be NULL");
  AFD_REQUIRE_KIND("afd_distill_target", kind);
  AFD_REQUIRE_B_CHW("afd_distill_target", B, chw);
  const long fb = B * chw * kF, ib = B * kI;
  AFD_REQUIRE(same_or_apart(x_tilde, fb, {out2, z_mid, z_t}) && same_or_apart(eps_tilde, fb, {out2, z_mid, z_t}) &&
                  all_apart({{x_tilde, fb}, {eps_tilde, fb}}, {{t, ib}, {t_mid, ib}, {t_prev, ib}}),
              "afd_distill_target: x_tilde and eps_tilde must each be an input itself or apart from it, and must not overlap each "
              "other, t, t_mid or t_prev");
  const RowQuadGrid g(B, chw, kObjBlocks);
  launch_vec(vec_ok(chw, {out2, z_mid, z_t, x_tilde, eps_tilde}), distill_target_k<true>, distill_target_k<false>, g.grid, as_stream(st),
             out2, z_mid, z_t, t, t_mid, t_prev, alpha_hat, kind, x_tilde, eps_tilde, g.items, g.segs, chw);
  return check_launch("afd_distill_target");
}

// ---- consistency distillation --------------------------------------------------------------------------------------------------
int afd_consistency_fn(const float* out, const float* z, const int64_t* t, const float* alpha_hat, const double* coef, int kind,
                       float* f_out, long B, long chw, afd_stream_t st) {
  AFD_REQUIRE(out && z && t && alpha_hat && coef && f_out,
              "afd_consistency_fn: out, z, t, alpha_hat, coef and f_out must not be NULL");
  AFD_REQUIRE_KIND("afd_consistency_fn", kind);
  AFD_REQUIRE_B_CHW("afd_consistency_fn", B, chw);
  const long fb = B * chw * kF;
  AFD_REQUIRE(same_or_apart(f_out, fb, {out, z}) && all_apart({{f_out, fb}}, {{t, B * kI}}),
              "afd_consistency_fn: f_out must be out or z itself or apart from them, and must not overlap t");
  const RowQuadGrid g(B, chw, kObjBlocks);
  launch_vec(vec_ok(chw, {out, z, f_out}), consistency_fn_k<true>, consistency_fn_k<false>, g.grid, as_stream(st), out, z, t, alpha_hat,
             coef, kind, f_out, g.items, g.segs, chw);
  return check_launch("afd_consistency_fn");
}
int afd_consistency_target(const float* out_tgt, const float* z_prev, const float* z_t, const int64_t* t, const int64_t* t_prev,
                           const float* alpha_hat, const double* coef, int kind, float* x_tilde, float* eps_tilde, long B, long chw,
                           afd_stream_t st) {
  AFD_REQUIRE(out_tgt && z_prev && z_t && t && t_prev && alpha_hat && coef && x_tilde && eps_tilde,
              "afd_consistency_target: out_tgt, z_prev, z_t, t, t_prev, alpha_hat, coef, x_tilde and eps_tilde must not be NULL");
  AFD_REQUIRE_KIND("afd_consistency_target", kind);
  AFD_REQUIRE_B_CHW("afd_consistency_target", B, chw);
  const long fb = B * chw * kF, ib = B * kI;
  AFD_REQUIRE(same_or_apart(x_tilde, fb, {out_tgt, z_prev, z_t}) && same_or_apart(eps_tilde, fb, {out_tgt, z_prev, z_t}) &&
                  all_apart({{x_tilde, fb}, {eps_tilde, fb}}, {{t, ib}, {t_prev, ib}}),
              "afd_consistency_target: x_tilde and eps_tilde must each be an input itself or apart from it, and must not overlap "
              "each other, t or t_prev");
  const RowQuadGrid g(B, chw, kObjBlocks);
  launch_vec(vec_ok(chw, {out_tgt, z_prev, z_t, x_tilde, eps_tilde}), consistency_target_k<true>, consistency_target_k<false>, g.grid,
             as_stream(st), out_tgt, z_prev, z_t, t, t_prev, alpha_hat, coef, kind, x_tilde, eps_tilde, g.items, g.segs, chw);
  return check_launch("afd_consistency_target");
}
// the two step entry points: t / t_next from the host, or read on the device (dev)
static int consistency_step(const char* name, bool dev, const float* out, const float* z, const float* noise, const float* alpha_hat,
                            const double* coef, int kind, int t, int t_next, const int64_t* t_dev, const int64_t* t_next_dev,
                            float* x_out, long n_rows, long chw, afd_stream_t st) {
  AFD_REQUIRE(out && z && alpha_hat && coef && x_out && (!dev || (t_dev && t_next_dev)),
              "%s: out, z, alpha_hat, coef%s and x_out must not be NULL", name, dev ? ", t_dev, t_next_dev" : "");
  AFD_REQUIRE_KIND(name, kind);
  AFD_REQUIRE_B_CHW(name, n_rows, chw);
  AFD_REQUIRE(dev || (t_next >= 0 && t_next < t), "%s: need 0 <= t_next < t (got t = %d, t_next = %d)", name, t, t_next);
  AFD_REQUIRE(dev || noise || t_next == 0, "%s: noise must not be NULL unless t_next == 0", name);
  const long fb = n_rows * chw * kF;
  AFD_REQUIRE(same_or_apart(x_out, fb, {out, z}) && all_apart({{x_out, fb}}, {{noise, fb}, {t_dev, kI}, {t_next_dev, kI}}),
              "%s: x_out must be out or z itself or apart from them, and must not overlap noise%s", name,
              dev ? ", t_dev or t_next_dev" : "");
  const RowQuadGrid g(n_rows, chw, kObjBlocks);
  launch_vec(vec_ok(chw, {out, z, noise, x_out}), consistency_step_k<true>, consistency_step_k<false>, g.grid, as_stream(st), out, z,
             noise, alpha_hat, coef, kind, t, t_next, t_dev, t_next_dev, x_out, g.items, g.segs, chw);
  return check_launch(name);
}
int afd_consistency_step(const float* out, const float* z, const float* noise, const float* alpha_hat, const double* coef, int kind,
                         int t, int t_next, float* x_out, long n_rows, long chw, afd_stream_t st) {
  return consistency_step("afd_consistency_step", false, out, z, noise, alpha_hat, coef, kind, t, t_next, nullptr, nullptr, x_out,
                          n_rows, chw, st);
}
int afd_consistency_step_dev(const float* out, const float* z, const float* noise, const float* alpha_hat, const double* coef,
                             int kind, const int64_t* t_dev, const int64_t* t_next_dev, float* x_out, long n_rows, long chw,
                             afd_stream_t st) {
  return consistency_step("afd_consistency_step_dev", true, out, z, noise, alpha_hat, coef, kind, 0, 0, t_dev, t_next_dev, x_out,
                          n_rows, chw, st);
}

// ---- likelihood (bits/dim) ------------------------------------------------------------------------------------------------
// img and t are read on the device and not range-checked here (the Python layer checks them); every output must share no
// memory with any input.
int afd_noise_images_gather(const float* x0, long n_img, const int64_t* img, const float* eps, const int64_t* t, const float* alpha_hat,
                            float* x_t, long rows, long per, afd_stream_t st) {
  AFD_REQUIRE(x0 && img && eps && t && alpha_hat && x_t, "afd_noise_images_gather: x0, img, eps, t, alpha_hat and x_t must not be NULL");
  AFD_REQUIRE(n_img > 0 && rows > 0 && per > 0, "afd_noise_images_gather: n_img, rows and per must be positive (got %ld, %ld, %ld)",
              n_img, rows, per);
  const long fb = rows * per * kF, ib = rows * kI;
  AFD_REQUIRE(all_apart({{x_t, fb}}, {{x0, n_img * per * kF}, {eps, fb}, {img, ib}, {t, ib}}),
              "afd_noise_images_gather: x_t must not overlap x0, eps, img or t");
  const bool vec = vec_ok(per, {x0, eps, x_t});
  launch_vec(vec, noise_images_gather_k<true>, noise_images_gather_k<false>, std::min<long>(rows, 4096), as_stream(st), x0, img, eps, t,
             alpha_hat, x_t, rows, vec ? per / 4 : per);
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
  const long db = rows * kD, fb = rows * per * kF, ib = rows * kI, tb = T * kF;
  AFD_REQUIRE(all_apart({{term, db}, {sq, db}}, {{x0, n_img * per * kF}, {img, ib}, {x_t, fb}, {eps, fb}, {eps_hat, fb}, {t, ib},
                                                 {coef, 4 * T * kD}, {alpha, tb}, {alpha_hat, tb}, {beta, tb}}),
              "afd_vlb_terms: term and sq must not overlap each other or any input");
  const bool vec = vec_ok(per, {x0, x_t, eps, eps_hat});
  launch_vec(vec, vlb_terms_k<true>, vlb_terms_k<false>, rows, as_stream(st), x0, img, x_t, eps, eps_hat, t, coef, alpha, alpha_hat, beta,
             term, sq, vec ? per / 4 : per, per);
  return check_launch("afd_vlb_terms");
}
int afd_vlb_prior(const float* x0, double half_ah, double* out, long n_img, long per, afd_stream_t st) {
  AFD_REQUIRE(x0 && out, "afd_vlb_prior: x0 and out must not be NULL");
  AFD_REQUIRE(n_img > 0 && per > 0, "afd_vlb_prior: n_img and per must be positive (got %ld, %ld)", n_img, per);
  AFD_REQUIRE(n_img <= 0x7fffffffL, "afd_vlb_prior: at most 2^31 - 1 images per call (got %ld)", n_img);
  AFD_REQUIRE(!overlaps(out, n_img * kD, x0, n_img * per * kF), "afd_vlb_prior: out must not overlap x0");
  const bool vec = vec_ok(per, {x0});
  launch_vec(vec, vlb_prior_k<true>, vlb_prior_k<false>, n_img, as_stream(st), x0, half_ah, out, vec ? per / 4 : per);
  return check_launch("afd_vlb_prior");
}

// ---- learned variances ----------------------------------------------------------------------------------------------------
constexpr long kLvarWsFloats = 3 * kObjBlocks;      // kObjBlocks fp32 partials, then kObjBlocks fp64 partials

// the _tw forms take vw, the second per-timestep table (NULL: none); afd_lvar_loss_fwd / _bwd are they with NULL
int afd_lvar_loss_fwd_tw(const float* out2, const float* x0, const float* eps, const int64_t* t, const float* alpha,
                         const float* alpha_hat, const float* beta, const double* lv_coef, const float* w, const float* vw, int kind,
                         double vlb_scale, float* loss_out, double* sums_out, float* workspace, long B, long chw, afd_stream_t st) {
  AFD_REQUIRE(out2 && x0 && eps && t && alpha && alpha_hat && beta && lv_coef && loss_out && workspace,
              "afd_lvar_loss_fwd: out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef, loss_out and workspace must not be NULL");
  AFD_REQUIRE_KIND("afd_lvar_loss_fwd", kind);
  AFD_REQUIRE_B_CHW("afd_lvar_loss_fwd", B, chw);
  AFD_REQUIRE_VLB_SCALE("afd_lvar_loss_fwd", vlb_scale);
  AFD_REQUIRE(((uintptr_t)workspace & 7) == 0, "afd_lvar_loss_fwd: workspace must be 8-byte aligned");
  const long fb = B * chw * kF;
  AFD_REQUIRE(all_apart({{loss_out, 2 * kF}, {sums_out, 2 * kD}, {workspace, kLvarWsFloats * kF}}, {{out2, 2 * fb}, {x0, fb}, {eps, fb}, {t, B * kI}}),
              "afd_lvar_loss_fwd: loss_out, sums_out and workspace must not overlap each other or an input");
  const RowQuadGrid g(B, chw, kObjBlocks);
  double* part_v = reinterpret_cast<double*>(workspace + kObjBlocks);
  const double n = (double)B * (double)chw;
  launch_vec(vec_ok(chw, {out2, x0, eps}), lvar_partial_k<true>, lvar_partial_k<false>, g.grid, as_stream(st), out2, x0, eps, t, alpha,
             alpha_hat, beta, lv_coef, w, vw, kind, workspace, part_v, g.items, g.segs, chw);
  hipLaunchKernelGGL(lvar_final_k, dim3(1), dim3(256), 0, as_stream(st), workspace, part_v, g.grid, 1.0f / (float)(B * chw),
                     n * 0.6931471805599453, vlb_scale, loss_out, sums_out);
  return check_launch("afd_lvar_loss_fwd");
}
int afd_lvar_loss_bwd_tw(const float* out2, const float* x0, const float* eps, const int64_t* t, const float* alpha,
                         const float* alpha_hat, const float* beta, const double* lv_coef, const float* w, const float* vw, int kind,
                         double vlb_scale, const float* dloss, float* dout2, long B, long chw, afd_stream_t st) {
  AFD_REQUIRE(out2 && x0 && eps && t && alpha && alpha_hat && beta && lv_coef && dloss && dout2,
              "afd_lvar_loss_bwd: out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef, dloss and dout2 must not be NULL");
  AFD_REQUIRE_KIND("afd_lvar_loss_bwd", kind);
  AFD_REQUIRE_B_CHW("afd_lvar_loss_bwd", B, chw);
  AFD_REQUIRE_VLB_SCALE("afd_lvar_loss_bwd", vlb_scale);
  const long fb = B * chw * kF;
  AFD_REQUIRE(all_apart({{dout2, 2 * fb}}, {{out2, 2 * fb}, {x0, fb}, {eps, fb}, {t, B * kI}, {dloss, kF}}),
              "afd_lvar_loss_bwd: dout2 must not overlap an input");
  const RowQuadGrid g(B, chw, kObjBlocks);
  const double n = (double)B * (double)chw;
  launch_vec(vec_ok(chw, {out2, x0, eps, dout2}), lvar_bwd_k<true>, lvar_bwd_k<false>, g.grid, as_stream(st), out2, x0, eps, t, alpha,
             alpha_hat, beta, lv_coef, w, vw, kind, dloss, dout2, g.items, g.segs, chw, 2.0f / (float)(B * chw),
             vlb_scale / (n * 0.6931471805599453));
  return check_launch("afd_lvar_loss_bwd");
}
int afd_lvar_loss_fwd(const float* out2, const float* x0, const float* eps, const int64_t* t, const float* alpha,
                      const float* alpha_hat, const float* beta, const double* lv_coef, const float* w, int kind, double vlb_scale,
                      float* loss_out, double* sums_out, float* workspace, long B, long chw, afd_stream_t st) {
  return afd_lvar_loss_fwd_tw(out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef, w, nullptr, kind, vlb_scale, loss_out, sums_out,
                              workspace, B, chw, st);
}
int afd_lvar_loss_bwd(const float* out2, const float* x0, const float* eps, const int64_t* t, const float* alpha,
                      const float* alpha_hat, const float* beta, const double* lv_coef, const float* w, int kind, double vlb_scale,
                      const float* dloss, float* dout2, long B, long chw, afd_stream_t st) {
  return afd_lvar_loss_bwd_tw(out2, x0, eps, t, alpha, alpha_hat, beta, lv_coef, w, nullptr, kind, vlb_scale, dloss, dout2, B, chw, st);
}
int afd_split_pred(const float* out2, const float* x_t, const int64_t* t, const float* alpha_hat, int kind, float* eps_out,
                   float* v_out, long B, long chw, afd_stream_t st) {
  AFD_REQUIRE(out2 && eps_out, "afd_split_pred: out2 and eps_out must not be NULL");
  AFD_REQUIRE_KIND("afd_split_pred", kind);
  AFD_REQUIRE(kind == AFD_PRED_EPS || (x_t && t && alpha_hat), "afd_split_pred: x_t, t and alpha_hat must not be NULL for AFD_PRED_V / AFD_PRED_X0");
  AFD_REQUIRE_B_CHW("afd_split_pred", B, chw);
  const long fb = B * chw * kF;
  AFD_REQUIRE(all_apart({{eps_out, fb}, {v_out, fb}}, {{out2, 2 * fb}, {x_t, fb}, {t, B * kI}}),
              "afd_split_pred: eps_out and v_out must not overlap each other, out2, x_t or t");
  const RowQuadGrid g(B, chw, kObjBlocks);
  launch_vec(vec_ok(chw, {out2, eps_out, x_t, v_out}), split_pred_k<true>, split_pred_k<false>, g.grid, as_stream(st), out2, x_t, t,
             alpha_hat, kind, eps_out, v_out, g.items, g.segs, chw);
  return check_launch("afd_split_pred");
}

int afd_denoise_step_lvar(const float* x, const float* out2, const float* noise, const float* alpha, const float* alpha_hat,
                          const float* beta, const double* lv_coef, int kind, int i, float* x_out, long B, long chw, afd_stream_t st) {
  return launch_lvar_step<false>("afd_denoise_step_lvar", x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, i, nullptr, false, 0.0f,
                                 x_out, nullptr, B, chw, as_stream(st));
}
int afd_denoise_step_lvar_dev(const float* x, const float* out2, const float* noise, const float* alpha, const float* alpha_hat,
                              const float* beta, const double* lv_coef, int kind, const int64_t* t_dev, float* x_out, long B, long chw,
                              afd_stream_t st) {
  return launch_lvar_step<false>("afd_denoise_step_lvar_dev", x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, 0, t_dev, true, 0.0f,
                                 x_out, nullptr, B, chw, as_stream(st));
}
int afd_denoise_step_lvar_cfg(const float* x, const float* out2, const float* noise, const float* alpha, const float* alpha_hat,
                              const float* beta, const double* lv_coef, int kind, int i, float cfg_scale, float* x_out, float* x_out2,
                              long B, long chw, afd_stream_t st) {
  return launch_lvar_step<true>("afd_denoise_step_lvar_cfg", x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, i, nullptr, false,
                                cfg_scale, x_out, x_out2, B, chw, as_stream(st));
}
int afd_denoise_step_lvar_cfg_dev(const float* x, const float* out2, const float* noise, const float* alpha, const float* alpha_hat,
                                  const float* beta, const double* lv_coef, int kind, const int64_t* t_dev, float cfg_scale, float* x_out,
                                  float* x_out2, long B, long chw, afd_stream_t st) {
  return launch_lvar_step<true>("afd_denoise_step_lvar_cfg_dev", x, out2, noise, alpha, alpha_hat, beta, lv_coef, kind, 0, t_dev, true,
                                cfg_scale, x_out, x_out2, B, chw, as_stream(st));
}
int afd_vlb_terms_lvar(const float* x0, long n_img, const int64_t* img, const float* x_t, const float* eps, const float* out2,
                       const int64_t* t, const double* lv_coef, long T, const float* alpha, const float* alpha_hat, const float* beta,
                       int kind, double* term, double* sq, long rows, long per, afd_stream_t st) {
  AFD_REQUIRE(x0 && img && x_t && eps && out2 && t && lv_coef && alpha && alpha_hat && beta && term && sq,
              "afd_vlb_terms_lvar: no pointer may be NULL");
  AFD_REQUIRE_KIND("afd_vlb_terms_lvar", kind);
  AFD_REQUIRE(n_img > 0 && rows > 0 && per > 0 && T >= 2,
              "afd_vlb_terms_lvar: n_img, rows and per must be positive and T >= 2 (got %ld, %ld, %ld, %ld)", n_img, rows, per, T);
  AFD_REQUIRE(rows <= 0x7fffffffL, "afd_vlb_terms_lvar: at most 2^31 - 1 rows per call (got %ld)", rows);
  const long db = rows * kD, fb = rows * per * kF, ib = rows * kI, tb = T * kF;
  AFD_REQUIRE(all_apart({{term, db}, {sq, db}}, {{x0, n_img * per * kF}, {img, ib}, {x_t, fb}, {eps, fb}, {out2, 2 * fb}, {t, ib},
                                                 {lv_coef, 3 * T * kD}, {alpha, tb}, {alpha_hat, tb}, {beta, tb}}),
              "afd_vlb_terms_lvar: term and sq must not overlap each other or any input");
  launch_vec(vec_ok(per, {x0, x_t, eps, out2}), vlb_terms_lvar_k<true>, vlb_terms_lvar_k<false>, rows, as_stream(st), x0, img, x_t, eps,
             out2, t, lv_coef, alpha, alpha_hat, beta, kind, term, sq, per);
  return check_launch("afd_vlb_terms_lvar");
}

}  // extern "C"
